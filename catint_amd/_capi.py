"""ctypes binding of the C-ABI in ``include/catint_pnp.h`` (the drop-in boundary).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``catint_amd.build.build_library()`` into ``catint_amd/lib/libcatint_pnp.so``.  There is no
CPU fallback: if the library is missing, or no HIP device is visible, the transport path
raises (``PnpLibraryError`` / ``PnpError``).
"""
import ctypes as C
import importlib
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CATINT_PNP_LIB') or os.path.join(_HERE, 'lib', 'libcatint_pnp.so')   # (env: diagnosis builds of tools/probe)

PNP_MAX_SPECIES = 16
PNP_MAX_REACTIONS = 16
PNP_MAX_REACTANTS = 4

METHOD_CRANK_NICOLSON = 0
METHOD_FTCS = 1
METHOD_NEWTON = 2      # physical mode: fully implicit coupled Newton (what the reference asks COMSOL for)
METHODS = {'Crank-Nicolson': METHOD_CRANK_NICOLSON, 'FTCS': METHOD_FTCS, 'Newton': METHOD_NEWTON}
PNP_NEWTON_MAX_SPECIES = 8

PB_DD, PB_VWALL_GBULK, PB_GWALL_VBULK, PB_VWALL_GWALL, PB_VBULK_GBULK = range(5)

STATUS_OK, STATUS_MAXIT, STATUS_NAN, STATUS_NEGATIVE = 0, 1, 2, 3

# every symbol include/catint_pnp.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    'pnp_create', 'pnp_destroy', 'pnp_last_error', 'pnp_version', 'pnp_set_species', 'pnp_set_reactions',
    'pnp_set_batch', 'pnp_set_flux', 'pnp_set_pb', 'pnp_step', 'pnp_integrate', 'pnp_mol_rhs', 'pnp_integrate_dopri5', 'pnp_integrate_dop853', 'pnp_integrate_rkc', 'pnp_get_state',
    'pnp_get_surface', 'pnp_get_status', 'pnp_synchronize', 'pnp_timer_start', 'pnp_timer_stop',
    'pnp_device_bytes', 'pnp_row_pitch', 'pnp_step_row_chunks', 'pnp_set_newton', 'pnp_solve_stationary', 'pnp_get_newton_iterations',
    'pnp_set_potential', 'pnp_set_convection', 'pnp_set_option', 'pnp_get_lane_order', 'pnp_autotune', 'pnp_autotune_name', 'pnp_autotune_default', 'pnp_tune_placement', 'pnp_set_lanes', 'pnp_set_lane_mask', 'pnp_set_wall_kinetics', 'pnp_set_wall_rate_law', 'pnp_set_grid', 'pnp_solve_surface', 'pnp_scf_cycle', 'pnp_scf_cycle_fn', 'pnp_get_device_view',
    'pnp_set_lanes_device',
]


class PnpLibraryError(RuntimeError):
    pass


class PnpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('catint_pnp error %d: %s' % (code, msg))
        self.code = code


class PnpConfig(C.Structure):
    _fields_ = [
        ('struct_size', C.c_int32), ('device', C.c_int32), ('nspecies', C.c_int32), ('nx', C.c_int32),
        ('method', C.c_int32), ('pb_mode', C.c_int32), ('lax_friedrich', C.c_int32), ('use_migration', C.c_int32),
        ('batch_capacity', C.c_int64), ('dx', C.c_double), ('dt', C.c_double), ('beta', C.c_double),
        ('eps', C.c_double),
    ]


class PnpNewtonParams(C.Structure):
    _fields_ = [
        ('struct_size', C.c_int32), ('wall_bc', C.c_int32), ('maxit', C.c_int32), ('error_estimate', C.c_int32),
        ('stern_capacitance', C.c_double), ('phi_pzc', C.c_double), ('tol', C.c_double), ('dphi_max', C.c_double),
        ('time_order', C.c_int32), ('predictor', C.c_int32),
    ]


class PnpScfParams(C.Structure):
    _fields_ = [
        ('struct_size', C.c_int32), ('istep', C.c_int32), ('max_iter', C.c_int32), ('check_every', C.c_int32),
        ('species_H', C.c_int32), ('species_OH', C.c_int32), ('tau_scf', C.c_double), ('faraday', C.c_double),
    ]


class PnpOdeParams(C.Structure):
    _fields_ = [
        ('struct_size', C.c_int32), ('nsteps', C.c_int32), ('rtol', C.c_double), ('atol', C.c_double),
        ('first_step', C.c_double), ('max_step', C.c_double), ('safety', C.c_double), ('ifactor', C.c_double),
        ('dfactor', C.c_double), ('beta', C.c_double), ('nstiff', C.c_int32), ('check_every', C.c_int32),
    ]


class PnpScfState(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_double)) for n in (
        'surface_concentration', 'surface_concentration_old', 'flux', 'current_density_old', 'mix', 'accuracy',
        'surface_pH', 'surface_potential', 'surface_efield')] + [(n, C.POINTER(C.c_int32)) for n in (
            'step_to_check', 'active', 'failed')]


class PnpScfDevice(C.Structure):
    """pnp_scf_device: what the flux function of pnp_scf_cycle_fn is handed (device addresses)"""
    _fields_ = [
        ('struct_size', C.c_int32), ('nspecies', C.c_int32), ('istep', C.c_int32), ('reserved', C.c_int32), ('batch', C.c_int64),
        ('surface_concentration', C.c_void_p), ('surface_potential', C.c_void_p), ('surface_efield', C.c_void_p),
        ('surface_pH', C.c_void_p), ('active', C.c_void_p), ('flux', C.c_void_p), ('stream', C.c_void_p),
    ]


# pnp_scf_flux_fn
PnpScfFluxFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(PnpScfDevice))


_lib = None


def load_library():
    """dlopen the HIP library; raises PnpLibraryError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PnpLibraryError(
            'HIP extension %s is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950). There is no CPU fallback for the transport path.' % LIB_PATH)
    if os.path.exists(os.path.join(_HERE, 'lib', '.partial')) and not os.environ.get('CATINT_ALLOW_PARTIAL'):   # dev runs set it
        raise PnpLibraryError(
            '%s was built by tools/devbuild.sh with only one Newton block size instantiated (marker lib/.partial): rebuild the '
            'full library with `python -c "import __graft_entry__ as g; g.build()"`.' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    vp = C.c_void_p
    lib.pnp_create.argtypes = [C.POINTER(PnpConfig), C.POINTER(vp)]
    lib.pnp_create.restype = C.c_int
    lib.pnp_destroy.argtypes = [vp]
    lib.pnp_destroy.restype = None
    lib.pnp_last_error.argtypes = [vp]
    lib.pnp_last_error.restype = C.c_char_p
    lib.pnp_version.argtypes = []
    lib.pnp_version.restype = C.c_char_p
    lib.pnp_set_species.argtypes = [vp, dp, dp]
    lib.pnp_set_reactions.argtypes = [vp, C.c_int32, ip, ip, ip, ip, dp, dp]
    lib.pnp_set_batch.argtypes = [vp, C.c_int64, dp, dp, dp, dp]
    lib.pnp_set_flux.argtypes = [vp, dp]
    lib.pnp_set_pb.argtypes = [vp, dp, dp]
    lib.pnp_step.argtypes = [vp, C.c_int32, C.c_int32]
    lib.pnp_integrate.argtypes = [vp, C.c_int32, ip, C.c_int32, dp, ip]
    lib.pnp_mol_rhs.argtypes = [vp, dp, dp]
    lib.pnp_get_state.argtypes = [vp, dp, dp, dp, dp]
    lib.pnp_get_surface.argtypes = [vp, dp, dp, dp]
    lib.pnp_get_status.argtypes = [vp, ip]
    lib.pnp_synchronize.argtypes = [vp]
    lib.pnp_timer_start.argtypes = [vp]
    lib.pnp_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    lib.pnp_set_newton.argtypes = [vp, C.POINTER(PnpNewtonParams), dp]
    lib.pnp_solve_stationary.argtypes = [vp, C.c_double, C.c_int32, ip]
    lib.pnp_get_newton_iterations.argtypes = [vp, ip]
    lib.pnp_set_potential.argtypes = [vp, dp]
    lib.pnp_set_lanes.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64), dp, dp]
    lib.pnp_set_lanes.restype = C.c_int
    lib.pnp_set_lanes_device.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    lib.pnp_set_lanes_device.restype = C.c_int
    lib.pnp_set_lane_mask.argtypes = [vp, ip]
    lib.pnp_set_lane_mask.restype = C.c_int
    lib.pnp_set_wall_kinetics.argtypes = [vp, C.c_int32, ip, dp, dp]
    lib.pnp_set_wall_kinetics.restype = C.c_int
    lib.pnp_integrate_dopri5.argtypes = [vp, C.POINTER(PnpOdeParams), C.c_int32, ip, C.c_int32, dp, ip, C.POINTER(C.c_int64), dp]
    lib.pnp_integrate_dopri5.restype = C.c_int
    lib.pnp_integrate_dop853.argtypes = lib.pnp_integrate_dopri5.argtypes
    lib.pnp_integrate_dop853.restype = C.c_int
    lib.pnp_integrate_rkc.argtypes = lib.pnp_integrate_dopri5.argtypes
    lib.pnp_integrate_rkc.restype = C.c_int
    lib.pnp_set_wall_rate_law.argtypes = [vp, C.c_int32, dp, dp]
    lib.pnp_set_wall_rate_law.restype = C.c_int
    lib.pnp_set_grid.argtypes = [vp, dp]
    lib.pnp_set_grid.restype = C.c_int
    lib.pnp_set_convection.argtypes = [vp, C.c_double]
    lib.pnp_set_convection.restype = C.c_int
    lib.pnp_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    lib.pnp_set_option.restype = C.c_int
    lib.pnp_get_lane_order.argtypes = [vp, ip]
    lib.pnp_get_lane_order.restype = C.c_int64
    lib.pnp_autotune.argtypes = [vp, C.c_int32, dp, ip]
    lib.pnp_autotune.restype = C.c_int
    lib.pnp_autotune_name.argtypes = [C.c_int32]
    lib.pnp_autotune_name.restype = C.c_char_p
    lib.pnp_autotune_default.argtypes = [vp]
    lib.pnp_autotune_default.restype = C.c_int32
    lib.pnp_tune_placement.argtypes = [vp, C.c_int32, C.c_int32, dp]
    lib.pnp_tune_placement.restype = C.c_int
    lib.pnp_solve_surface.argtypes = [vp, dp, C.c_int32, dp, dp, dp, ip]
    lib.pnp_solve_surface.restype = C.c_int
    lib.pnp_scf_cycle.argtypes = [vp, C.POINTER(PnpScfParams), dp, dp, C.POINTER(PnpScfState), ip]
    lib.pnp_scf_cycle.restype = C.c_int
    lib.pnp_scf_cycle_fn.argtypes = [vp, C.POINTER(PnpScfParams), dp, dp, C.POINTER(PnpScfState), C.c_void_p, C.c_void_p, ip]
    lib.pnp_scf_cycle_fn.restype = C.c_int
    for name in ('pnp_set_newton', 'pnp_solve_stationary', 'pnp_get_newton_iterations', 'pnp_set_potential'):
        getattr(lib, name).restype = C.c_int
    for name in ('pnp_set_species', 'pnp_set_reactions', 'pnp_set_batch', 'pnp_set_flux', 'pnp_set_pb', 'pnp_step',
                 'pnp_integrate', 'pnp_mol_rhs', 'pnp_get_state', 'pnp_get_surface', 'pnp_get_status', 'pnp_synchronize',
                 'pnp_timer_start', 'pnp_timer_stop'):
        getattr(lib, name).restype = C.c_int
    lib.pnp_get_device_view.argtypes = [vp, C.c_void_p]
    lib.pnp_get_device_view.restype = C.c_int
    lib.pnp_device_bytes.argtypes = [vp]
    lib.pnp_device_bytes.restype = C.c_int64
    lib.pnp_row_pitch.argtypes = [vp]
    lib.pnp_row_pitch.restype = C.c_int32
    lib.pnp_step_row_chunks.argtypes = [vp, C.c_int32]
    lib.pnp_step_row_chunks.restype = C.c_int32
    _lib = lib
    return lib


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError('expected shape %s, got %s' % (tuple(shape), a.shape))
    return a


def flatten_reactions(reactions):
    """[(lhs indices, rhs indices, kf, kr)] -> (n, n_lhs, lhs, n_rhs, rhs, kf, kr), the arrays of pnp_set_reactions (and of
    catbal_params).  A side longer than PNP_MAX_REACTANTS keeps its length in n_lhs / n_rhs and its first entries in lhs / rhs:
    the callee rejects it."""
    n = len(reactions)
    n_lhs = np.zeros(max(n, 1), np.int32)
    n_rhs = np.zeros(max(n, 1), np.int32)
    lhs = np.zeros((max(n, 1), PNP_MAX_REACTANTS), np.int32)
    rhs = np.zeros((max(n, 1), PNP_MAX_REACTANTS), np.int32)
    kf = np.zeros(max(n, 1))
    kr = np.zeros(max(n, 1))
    for r, (l, rr, f, b) in enumerate(reactions):
        n_lhs[r], n_rhs[r] = len(l), len(rr)
        lhs[r, :min(len(l), PNP_MAX_REACTANTS)] = list(l)[:PNP_MAX_REACTANTS]
        rhs[r, :min(len(rr), PNP_MAX_REACTANTS)] = list(rr)[:PNP_MAX_REACTANTS]
        kf[r], kr[r] = f, b
    return n, n_lhs, lhs, n_rhs, rhs, kf, kr


class PnpSolver(object):
    """Thin object wrapper over one ``pnp_handle`` (one GPU)."""

    # the contexts of the satellite libraries a solver opens on first use (_satellite) and close() destroys, in this order:
    # attribute -> (module of this package, class)
    SATELLITES = {'_observer': ('_observe', 'Observer'), '_balancer': ('_balance', 'Balancer'), '_regridder': ('_regrid', 'Regridder'),
                  '_equilibrator': ('_equil', 'Equilibrator'), '_responder': ('_response', 'Responder'),
                  '_kinetics': ('_kinetics', 'KineticsSolver'), '_coupler': ('_couple', 'Coupler'), '_sensitizer': ('_sens', 'Sensitizer'),
                  '_rate_control': ('_drc', 'RateControl'), '_transient': ('_kintrans', 'TransientKinetics'),
                  '_impedance': ('_eis', 'Impedance'), '_interact': ('_interact', 'InteractingKinetics'),
                  '_mode_solver': ('_modes', 'ModeSolver')}

    def __init__(self, nspecies, nx, dx, dt, beta, eps, D, charges, method='Crank-Nicolson', pb_mode=PB_DD,
                 lax_friedrich=False, use_migration=True, batch_capacity=1, device=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        if method not in METHODS:
            raise PnpError(-1, 'No calculator found with this name: %r' % (method,))
        cfg = PnpConfig(C.sizeof(PnpConfig), int(device), int(nspecies), int(nx), METHODS[method], int(pb_mode),
                        int(bool(lax_friedrich)), int(bool(use_migration)), int(batch_capacity), float(dx), float(dt),
                        float(beta), float(eps))
        rc = self._lib.pnp_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = self._lib.pnp_last_error(None).decode()
            self._h = C.c_void_p()
            raise PnpError(rc, msg)
        self.N, self.nx, self.B = int(nspecies), int(nx), 0
        self.dt_ode = float(dt)      # interval length of integrate_dopri5 (cfg.dt)
        self.method = method
        self._check(self._lib.pnp_set_species(self._h, _dptr(_f64(D, (self.N,))), _dptr(_f64(charges, (self.N,)))))
        # what get_electrolyte hands to the observables library: the problem as this solver was given it
        self._obs = {'D': np.array(D, float), 'charges': np.array(charges, float), 'beta': float(beta), 'x': np.arange(self.nx) * float(dx),
                     'mpb_radius': None, 'velocity': 0.0, 'device': int(device),
                     # ... and what get_balance hands to the balance library on top of that (recording only)
                     'reactions': [], 'wall': None, 'flux': None, 'phiM': None, 'flux_stale': False, 'wall_stale': False,
                     'explicit_kinetics': False,
                     # ... and what equilibrium / set_equilibrium hand to the equilibrium library
                     'eps': float(eps), 'dx': float(dx), 'wall_bc': 'dirichlet', 'stern_capacitance': 0.0, 'phi_pzc': 0.0,
                     'c_bulk': None, 'phi_bulk': None}
        for attr in self.SATELLITES:
            setattr(self, attr, None)

    def _check(self, rc):
        if rc != 0:
            raise PnpError(rc, self._lib.pnp_last_error(self._h).decode())

    def _satellite(self, attr):
        """The context of a satellite library, opened on this solver's device at its first use"""
        handle = getattr(self, attr, None)
        if handle is None:
            module, cls = self.SATELLITES[attr]
            handle = getattr(importlib.import_module('.' + module, __package__), cls)(self._obs['device'])
            setattr(self, attr, handle)
        return handle

    def close(self):
        for attr in self.SATELLITES:          # (getattr: close() also ends an object whose constructor raised)
            if getattr(self, attr, None) is not None:
                getattr(self, attr).close()
                setattr(self, attr, None)
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.pnp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- parameters ------------------------------------------------------------------------
    def set_reactions(self, reactions):
        """reactions: list of (lhs_indices, rhs_indices, kf, kr) in the reference's dict order."""
        for r, (l, rr, f, b) in enumerate(reactions):
            if len(l) > PNP_MAX_REACTANTS or len(rr) > PNP_MAX_REACTANTS:
                raise PnpError(-1, 'too many reactants in reaction %d' % r)
        n, n_lhs, lhs, n_rhs, rhs, kf, kr = flatten_reactions(reactions)
        self._check(self._lib.pnp_set_reactions(self._h, n, _iptr(n_lhs), _iptr(lhs), _iptr(n_rhs), _iptr(rhs),
                                                _dptr(kf), _dptr(kr)))
        self._obs['reactions'] = [(list(l), list(rr), float(f), float(b)) for (l, rr, f, b) in reactions]

    def set_batch(self, c0, pb, vzeta, flux):
        c0 = np.ascontiguousarray(c0, dtype=np.float64)
        B = c0.shape[0]
        c0 = _f64(c0.reshape(B, self.N, self.nx))
        pb = np.nan_to_num(_f64(pb, (B, 4)), nan=0.0)
        self._check(self._lib.pnp_set_batch(self._h, B, _dptr(c0), _dptr(pb), _dptr(_f64(vzeta, (B,))),
                                            _dptr(_f64(flux, (B, self.N)))))
        self.B = B
        self._obs.update(flux=np.array(_f64(flux, (B, self.N))), phiM=pb[:, 0].copy(), flux_stale=False, explicit_kinetics=False,
                         c_bulk=c0[:, :, -1].copy(), phi_bulk=pb[:, 1].copy())
        # pnp_set_batch keeps the handle's wall table, but its rate constants are per lane of the batch they were set for: with another
        # batch size the recorded ones no longer say what the solver applies (get_balance refuses until set_wall_kinetics is called)
        if self._obs['wall'] is not None and len(self._obs['wall']['k']) != B:
            self._obs['wall_stale'] = True

    def set_flux(self, flux):
        self._check(self._lib.pnp_set_flux(self._h, _dptr(_f64(flux, (self.B, self.N)))))
        self._obs.update(flux=np.array(_f64(flux, (self.B, self.N))), flux_stale=False)

    def set_pb(self, pb, vzeta):
        pb = np.nan_to_num(_f64(pb, (self.B, 4)), nan=0.0)
        self._check(self._lib.pnp_set_pb(self._h, _dptr(pb), _dptr(_f64(vzeta, (self.B,)))))
        self._obs.update(phiM=pb[:, 0].copy(), phi_bulk=pb[:, 1].copy())

    # -- physical mode ---------------------------------------------------------------------
    def set_newton(self, wall_bc='dirichlet', stern_capacitance=0.0, phi_pzc=0.0, tol=1e-10, maxit=50, dphi_max=0.05,
                   mpb_radius=None, error_estimate=False, time_order=1, predictor=False):
        """Boundary model and Newton controls of the physical mode (tp.system['Stern capacitance'], ['phiPZC'],
        tp.species[sp]['MPB_radius']; comsol_model.py:613,:982,:1041-1063).  time_order=2: BDF2 timesteps (the reference's transient
        study: BDF, maxorder 2, comsol_model.py:518-531) instead of backward Euler; predictor=True: every timestep's Newton iteration
        starts from the linear extrapolation of the two previous time levels."""
        p = PnpNewtonParams(C.sizeof(PnpNewtonParams), {'dirichlet': 0, 'stern': 1}[wall_bc], int(maxit), int(bool(error_estimate)),
                            float(stern_capacitance), float(phi_pzc), float(tol), float(dphi_max), int(time_order), int(bool(predictor)))
        r = None if mpb_radius is None else _f64(mpb_radius, (self.N,))
        self._check(self._lib.pnp_set_newton(self._h, C.byref(p), _dptr(r)))
        self._obs.update(mpb_radius=None if r is None else r.copy(), wall_bc=wall_bc, stern_capacitance=float(stern_capacitance),
                         phi_pzc=float(phi_pzc))

    def set_option(self, key, value):
        """Debug / tuning switch of this handle (pnp_set_option): e.g. set_option('NEWTON_KERNEL', 'lane2').  The CATINT_* environment
        variables only provide the defaults at construction."""
        self._check(self._lib.pnp_set_option(self._h, str(key).encode(), str(value).encode()))

    def lane_order(self):
        """Debug: operating point of every slot of the most recent lane-kernel launch (pnp_get_lane_order); empty if none was used."""
        n = int(self._lib.pnp_get_lane_order(self._h, None))
        perm = np.zeros(max(n, 0), np.int32)
        if n > 0:
            self._lib.pnp_get_lane_order(self._h, _iptr(perm))
        return perm

    def default_family(self):
        """Name of the kernel family the library's thresholds choose for the current batch (pnp_autotune_default); None without one."""
        i = int(self._lib.pnp_autotune_default(self._h))
        return None if i < 0 else self._lib.pnp_autotune_name(i).decode()

    def tune_placement(self, nsteps=2, trials=4):
        """Lane kernels: allocate the workspace up to `trials` times, keep the placement on which `nsteps` timesteps run fastest
        (pnp_tune_placement); the state is left as it was.  Returns the time per timestep (ms) of the trials that were made."""
        ms = np.full(int(trials), -1.0)
        self._check(self._lib.pnp_tune_placement(self._h, int(nsteps), int(trials), _dptr(ms)))
        return [float(v) for v in ms if v >= 0.0]

    def autotune(self, nsteps=2):
        """Physical mode: pick the kernel family by measurement on this device and batch (pnp_autotune).  Returns (name of the chosen
        family, {family: ms per timestep} of every family that supports the shape); the state and its history are left as they were."""
        n = 8
        ms = np.zeros(n)
        chosen = np.zeros(1, np.int32)
        self._check(self._lib.pnp_autotune(self._h, int(nsteps), _dptr(ms), _iptr(chosen)))
        names = [self._lib.pnp_autotune_name(i).decode() for i in range(n)]
        return names[int(chosen[0])], {names[i]: float(ms[i]) for i in range(n) if ms[i] >= 0.0}

    def set_convection(self, velocity):
        """Constant convection velocity (m/s) of the physical mode: tp.system['flow rate'] (comsol_model.py:901-903)."""
        self._check(self._lib.pnp_set_convection(self._h, float(velocity)))
        self._obs['velocity'] = float(velocity)

    def set_grid(self, x):
        """Non-uniform grid x[nx] of the physical mode (electrode at x[0]); dx of the constructor stays the scaling length."""
        self._check(self._lib.pnp_set_grid(self._h, _dptr(_f64(x, (self.nx,)))))
        self._obs['x'] = np.array(x, float)

    def set_wall_kinetics(self, species, nu, k, alpha=None, saturation=None):
        """Surface reactions coupled implicitly: species [n] (index, -1 = zeroth order), nu [n][N] stoichiometry of the flux
        into the domain, k [B][n] rate constants per lane.  Empty lists remove the table.  alpha [n] (1/V) / saturation [n]
        (m^3/mol): Butler-Volmer factor exp(alpha (phiM - phi(x=0))) and Langmuir saturation c/(1 + K c) (pnp_set_wall_rate_law);
        None: first order."""
        n = len(species)
        if n == 0:
            self._check(self._lib.pnp_set_wall_kinetics(self._h, 0, None, None, None))
            self._obs.update(wall=None, wall_stale=False)
            return
        sp = np.ascontiguousarray(species, dtype=np.int32)
        self._check(self._lib.pnp_set_wall_kinetics(self._h, n, _iptr(sp), _dptr(_f64(nu, (n, self.N))),
                                                    _dptr(_f64(k, (self.B, n)))))
        if alpha is not None or saturation is not None:
            al = _f64(np.zeros(n) if alpha is None else alpha, (n,))
            ks = _f64(np.zeros(n) if saturation is None else saturation, (n,))
            self._check(self._lib.pnp_set_wall_rate_law(self._h, n, _dptr(al), _dptr(ks)))
        self._obs['wall'] = {'species': sp.copy(), 'nu': np.array(_f64(nu, (n, self.N))), 'k': np.array(_f64(k, (self.B, n))),
                             'alpha': None if alpha is None and saturation is None else al.copy(),
                             'saturation': None if alpha is None and saturation is None else ks.copy()}
        self._obs['wall_stale'] = False

    def solve_stationary(self, tol=0.0, maxit=0):
        st = np.zeros(self.B, np.int32)
        self._check(self._lib.pnp_solve_stationary(self._h, float(tol), int(maxit), _iptr(st)))
        self._obs['explicit_kinetics'] = False
        return st

    def solve_surface(self, flux=None, nsteps=0):
        """New wall fluxes in, surface state out, one synchronisation: (csurf [B][N], vsurf [B], esurf [B], status [B]);
        nsteps = 0 solves the stationary problem, otherwise nsteps backward-Euler steps."""
        cs = np.zeros((self.B, self.N)); vs = np.zeros(self.B); es = np.zeros(self.B); st = np.zeros(self.B, np.int32)
        f = None if flux is None else _f64(flux, (self.B, self.N))
        self._check(self._lib.pnp_solve_surface(self._h, _dptr(f), int(nsteps), _dptr(cs), _dptr(vs), _dptr(es), _iptr(st)))
        self._obs['explicit_kinetics'] = False
        if f is not None:
            self._obs.update(flux=np.array(f), flux_stale=False)
        return cs, vs, es, st

    def scf_cycle(self, state, istep, max_iter, tau_scf, faraday, nel=None, nprod=None, species_H=-1, species_OH=-1,
                  check_every=8, flux_fn=None, user=None):
        """Device SCF loop (pnp_scf_cycle) from iteration istep+1 on.  `state`: dict of the loop arrays
        ('surface_concentration', 'surface_concentration_old', 'flux', 'current_density_old' [B][N]; 'mix', 'accuracy',
        'surface_pH', 'surface_potential', 'surface_efield' [B]; 'step_to_check', 'active', 'failed' [B] int) -- updated in
        place (fresh contiguous arrays are put back into the dict).  Returns the last iteration number that had active lanes.
        flux_fn, user: the addresses (two integers) of a pnp_scf_flux_fn and of its argument; with flux_fn the wall fluxes come from that
        function (pnp_scf_cycle_fn) and the wall table is not consulted."""
        B, N = self.B, self.N
        st = PnpScfState()
        for name, ctype in PnpScfState._fields_:
            if ctype == C.POINTER(C.c_double):
                shape = (B, N) if name in ('surface_concentration', 'surface_concentration_old', 'flux', 'current_density_old') else (B,)
                arr = np.array(_f64(state[name], shape))
                setattr(st, name, _dptr(arr))
            else:
                arr = np.ascontiguousarray(np.asarray(state[name]).reshape(B), dtype=np.int32).copy()
                setattr(st, name, _iptr(arr))
            state[name] = arr
        p = PnpScfParams(struct_size=C.sizeof(PnpScfParams), istep=int(istep), max_iter=int(max_iter), check_every=int(check_every),
                         species_H=int(species_H), species_OH=int(species_OH), tau_scf=float(tau_scf), faraday=float(faraday))
        nel = None if nel is None else _f64(nel, (N,))
        nprod = None if nprod is None else _f64(nprod, (N,))
        it = C.c_int32(0)
        if flux_fn is None:
            self._check(self._lib.pnp_scf_cycle(self._h, C.byref(p), _dptr(nel), _dptr(nprod), C.byref(st), C.byref(it)))
        else:
            self._check(self._lib.pnp_scf_cycle_fn(self._h, C.byref(p), _dptr(nel), _dptr(nprod), C.byref(st), C.c_void_p(int(flux_fn)),
                                                   C.c_void_p(None if user is None else int(user)), C.byref(it)))
        # the loop updated the wall fluxes on the device: the recorded table is no longer theirs.  And its solves took the wall reactions
        # through those fluxes (explicitly, from the mixed surface state), not through the wall table: the state it leaves conserves
        # state['flux'] alone
        self._obs.update(flux_stale=True, explicit_kinetics=True)
        return int(it.value)

    def newton_iterations(self):
        it = np.zeros(self.B, np.int32)
        self._check(self._lib.pnp_get_newton_iterations(self._h, _iptr(it)))
        return it

    def set_potential(self, phi):
        self._check(self._lib.pnp_set_potential(self._h, _dptr(_f64(phi, (self.B, self.nx)))))

    def set_lanes(self, lanes, c, phi=None):
        """State of a few lanes (c [n][N][nx] or [n][N*nx], phi [n][nx] or None) without touching the rest of the batch, its counters
        or its flags (pnp_set_lanes)."""
        idx = np.ascontiguousarray(lanes, dtype=np.int64)
        n = len(idx)
        cc = _f64(np.asarray(c, float).reshape(n, self.N, self.nx), (n, self.N, self.nx))
        pp = None if phi is None else _f64(phi, (n, self.nx))
        self._check(self._lib.pnp_set_lanes(self._h, n, idx.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(cc), _dptr(pp)))

    def set_lanes_device(self, c_dev, phi_dev=None, n=None, lanes=None):
        """set_lanes from device memory of this handle's device (pnp_set_lanes_device): c_dev / phi_dev are integer device addresses
        of [n][N][row_pitch] / [n][row_pitch] rows with this handle's row pitch, e.g. what resample(..., to_host=False) of another
        handle returned.  lanes None: lanes 0 .. n-1."""
        idx = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.int64).reshape(-1)
        n = (self.B if idx is None else len(idx)) if n is None else int(n)
        if idx is not None and len(idx) != n:
            raise ValueError('set_lanes_device: %d lanes for n = %d' % (len(idx), n))
        self._check(self._lib.pnp_set_lanes_device(self._h, n, None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                   C.c_void_p(c_dev), C.c_void_p(phi_dev)))

    def resample(self, x_target, lanes=None, to_host=True, max_waves=0):
        """The state of the lanes `lanes` (None: all, in order) resampled on the device onto the grid x_target, with the interpolant the
        discretisation implies inside a cell (include/catint_regrid.h).  D, charges, ion radii, grid and velocity are the ones this
        solver was given.  to_host: (c [n][N][nx_target], phi [n][nx_target]); otherwise nothing crosses PCIe and the result is
        (c_dev, phi_dev), integer device addresses of rows with the pitch of a handle of len(x_target) points, valid until the next
        resample / resample_to / close of this solver (set_lanes_device of such a handle takes them)."""
        o = self._obs
        out = self._satellite('_regridder').resample(self.device_view(), o['D'], o['charges'], o['x'], o['beta'], x_target,
                                                     mpb_radius=o['mpb_radius'], velocity=o['velocity'], lanes=lanes, to_host=to_host,
                                                     device=not to_host, max_waves=max_waves)
        return (out['c'], out['phi']) if to_host else (out['c_dev'], out['phi_dev'])

    def resample_to(self, other, lanes=None, dst_lanes=None):
        """The device path of a grid transfer: the lanes `lanes` of this solver (None: all) resampled onto the grid of `other` (a
        PnpSolver of the physical mode on the same device, with a batch set) and written into its lanes `dst_lanes` (None: 0 .. n-1)
        by set_lanes_device.  No state crosses PCIe."""
        if other.N != self.N:
            raise ValueError('resample_to: %d species here, %d there' % (self.N, other.N))
        if other._obs['device'] != self._obs['device']:
            raise ValueError('resample_to: the two solvers live on different devices')
        n = self.B if lanes is None else len(lanes)
        c_dev, phi_dev = self.resample(other._obs['x'], lanes=lanes, to_host=False)
        other.set_lanes_device(c_dev, phi_dev, n=n, lanes=dst_lanes)

    def equilibrium(self, phiM=None, lanes=None, to_host=True, tol=1e-10, maxit=100, max_waves=0):
        """The zero-flux (equilibrium) state of the lanes `lanes` (None: all, in order; repeats allowed) at the wall potentials phiM
        ([n], None: what set_batch / set_pb gave those lanes), solved on the device as a discrete size-modified Poisson-Boltzmann
        problem (include/catint_equil.h): a root of this solver's own stationary residual with zero wall flux.  Bulk values, wall
        model, ion radii and grid are the ones this solver was given.  The handle's state is not touched.  Returns a dict: 'status'
        [n] (0, or 1: not converged within maxit), 'iterations' [n]; with to_host 'c' [n][N][nx] and 'phi' [n][nx]; otherwise nothing
        but the flags crosses PCIe and 'c_dev' / 'phi_dev' are integer device addresses of rows with this handle's pitch, valid until
        the next equilibrium / set_equilibrium / close of this solver (set_lanes_device takes them)."""
        o = self._obs
        if o['c_bulk'] is None:
            raise ValueError('equilibrium: no batch was set')
        idx = self._lanes('equilibrium', lanes)
        pm = o['phiM'][idx] if phiM is None else np.broadcast_to(np.asarray(phiM, float), (len(idx),))
        return self._satellite('_equilibrator').solve(self.device_view(), o['charges'], o['x'], o['beta'], o['eps'], o['dx'], pm,
                                                      o['phi_bulk'][idx], o['c_bulk'][idx], mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'],
                                                      stern_capacitance=o['stern_capacitance'], phi_pzc=o['phi_pzc'], tol=tol, maxit=maxit,
                                                      to_host=to_host, device=not to_host, max_waves=max_waves)

    def set_equilibrium(self, phiM=None, lanes=None, tol=1e-10, maxit=100):
        """The device path of an equilibrium start: equilibrium(...) of the lanes `lanes` (None: all) written into those lanes by
        set_lanes_device.  No state crosses PCIe; the other lanes, the counters and the flags stay as they are.  Returns
        {'status', 'iterations'}."""
        out = self.equilibrium(phiM=phiM, lanes=lanes, to_host=False, tol=tol, maxit=maxit)
        n = len(out['status'])
        if n:
            self.set_lanes_device(out['c_dev'], out['phi_dev'], n=n, lanes=lanes)
        return {'status': out['status'], 'iterations': out['iterations']}

    def set_lane_mask(self, mask=None):
        """Only lanes with a non-zero mask take part in the following solves of the physical mode (None: all lanes again)."""
        if mask is None:
            self._check(self._lib.pnp_set_lane_mask(self._h, None))
            return
        m = np.ascontiguousarray(np.asarray(mask).astype(np.int32).reshape(self.B))
        self._check(self._lib.pnp_set_lane_mask(self._h, _iptr(m)))

    # -- hot path --------------------------------------------------------------------------
    def step(self, nsteps=1, steps_per_launch=0):
        self._check(self._lib.pnp_step(self._h, int(nsteps), int(steps_per_launch)))
        self._obs['explicit_kinetics'] = False

    def integrate(self, nt, itout):
        """Reference loop + outputs: returns (cout[n_out, B, N*nx], status[B])."""
        itout = np.ascontiguousarray(itout, dtype=np.int32)
        cout = np.zeros((len(itout), self.B, self.N * self.nx))
        status = np.zeros(self.B, np.int32)
        self._check(self._lib.pnp_integrate(self._h, int(nt), _iptr(itout), len(itout), _dptr(cout), _iptr(status)))
        return cout, status

    def mol_rhs(self, c):
        """ode_func for the current batch: c [B][N*nx] -> dc/dt [B][N*nx] (calculator_old.py:827-935)."""
        c = _f64(np.asarray(c, dtype=np.float64).reshape(self.B, self.N * self.nx))
        out = np.zeros_like(c)
        self._check(self._lib.pnp_mol_rhs(self._h, _dptr(c), _dptr(out)))
        return out

    def integrate_dopri5(self, nt, itout, rtol=1e-6, atol=1e-12, nsteps=500, first_step=0.0, max_step=0.0, safety=0.9, ifactor=10.0,
                         dfactor=0.2, beta=0.0, nstiff=1000, check_every=0):
        """scipy.integrate.ode('dopri5') of every lane on the device, one integrate(t + dt) per interval (calculator_old.py:955-963;
        keyword names and defaults are scipy's).  Returns (cout[n_out, B, N*nx] = state after interval itout[j], idid[B], stats[B, 5] =
        attempted / accepted / rejected steps, RHS evaluations, interval of the last call, t_end[B])."""
        return self._integrate_rk(self._lib.pnp_integrate_dopri5, nt, itout, rtol, atol, nsteps, first_step, max_step, safety, ifactor,
                                  dfactor, beta, nstiff, check_every)

    def integrate_dop853(self, nt, itout, rtol=1e-6, atol=1e-12, nsteps=500, first_step=0.0, max_step=0.0, safety=0.9, ifactor=6.0,
                         dfactor=0.3, beta=0.0, nstiff=1000, check_every=0):
        """scipy.integrate.ode('dop853') of every lane on the device (keyword names and defaults are scipy's for this integrator)."""
        return self._integrate_rk(self._lib.pnp_integrate_dop853, nt, itout, rtol, atol, nsteps, first_step, max_step, safety, ifactor,
                                  dfactor, beta, nstiff, check_every)

    def integrate_rkc(self, nt, itout, rtol=1e-6, atol=1e-12, nsteps=100000, max_step=0.0, check_every=0):
        """Stiff method-of-lines integration of every lane on the device (pnp_integrate_rkc: Runge-Kutta-Chebyshev with error control,
        the batched counterpart of odeint / ode('vode' | 'lsoda'), calculator_old.py:946-963).  Returns (cout[n_out, B, N*nx] = state
        after interval itout[j], idid[B], stats[B, 7] = attempted / accepted / rejected steps, RHS evaluations of the steps, interval
        of the last call, RHS evaluations of the spectral-radius estimates, largest stage count; t_end[B])."""
        itout = np.ascontiguousarray(itout, dtype=np.int32)
        cout = np.zeros((len(itout), self.B, self.N * self.nx))
        idid = np.zeros(self.B, np.int32)
        stats = np.zeros((self.B, 7), np.int64)
        t_end = np.zeros(self.B)
        p = PnpOdeParams(C.sizeof(PnpOdeParams), int(nsteps), float(rtol), float(atol), 0.0, float(max_step), 0.0, 0.0, 0.0, 0.0, 0,
                         int(check_every))
        self._check(self._lib.pnp_integrate_rkc(self._h, C.byref(p), int(nt), _iptr(itout), len(itout), _dptr(cout), _iptr(idid),
                                                stats.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(t_end)))
        return cout, idid, stats, t_end

    def _integrate_rk(self, fn, nt, itout, rtol, atol, nsteps, first_step, max_step, safety, ifactor, dfactor, beta, nstiff, check_every):
        itout = np.ascontiguousarray(itout, dtype=np.int32)
        cout = np.zeros((len(itout), self.B, self.N * self.nx))
        idid = np.zeros(self.B, np.int32)
        stats = np.zeros((self.B, 5), np.int64)
        t_end = np.zeros(self.B)
        p = PnpOdeParams(C.sizeof(PnpOdeParams), int(nsteps), float(rtol), float(atol), float(first_step), float(max_step), float(safety),
                         float(ifactor), float(dfactor), float(beta), int(nstiff), int(check_every))
        self._check(fn(self._h, C.byref(p), int(nt), _iptr(itout), len(itout), _dptr(cout), _iptr(idid),
                       stats.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(t_end)))
        return cout, idid, stats, t_end

    # -- read-back -------------------------------------------------------------------------
    def get_state(self, potential=True, derived=True):
        """(c, v, grad_v, lapl_v); potential=False: c alone; derived=False: (c, v) -- in the physical mode two plain copies, without
        the host loops that derive the gradient and the charge row."""
        c = np.zeros((self.B, self.N, self.nx))
        if potential and not derived:
            v = np.zeros((self.B, self.nx))
            self._check(self._lib.pnp_get_state(self._h, _dptr(c), _dptr(v), None, None))
            return c, v
        if potential:
            v = np.zeros((self.B, self.nx)); g = np.zeros((self.B, self.nx)); l = np.zeros((self.B, self.nx))
            self._check(self._lib.pnp_get_state(self._h, _dptr(c), _dptr(v), _dptr(g), _dptr(l)))
            return c, v, g, l
        self._check(self._lib.pnp_get_state(self._h, _dptr(c), None, None, None))
        return c

    def get_surface(self):
        cs = np.zeros((self.B, self.N)); vs = np.zeros(self.B); es = np.zeros(self.B)
        self._check(self._lib.pnp_get_surface(self._h, _dptr(cs), _dptr(vs), _dptr(es)))
        return cs, vs, es

    def device_view(self):
        """Where the state lives on the device (pnp_get_device_view): a catint_amd._observe.PnpDeviceView, valid until the next
        set_batch / close.  No copy, no synchronisation."""
        from ._observe import PnpDeviceView
        view = PnpDeviceView()
        self._check(self._lib.pnp_get_device_view(self._h, C.byref(view)))
        return view

    # -- the rules the get_* methods share; `method` is the caller's name, for its messages ------
    def _lanes(self, method, lanes):
        """the lane list checked against the batch; None: all lanes, in order"""
        idx = np.arange(self.B, dtype=np.int64) if lanes is None else np.ascontiguousarray(lanes, dtype=np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= self.B):
            raise ValueError('%s: lane index outside [0, %d)' % (method, self.B))
        return idx

    def _wall_table(self, method):
        """the wall table a library is given: none after scf_cycle, whose solves took the wall reactions through the prescribed flux"""
        o = self._obs
        wall = None if o['explicit_kinetics'] else o['wall']
        if wall is not None and o['wall_stale']:
            raise ValueError('%s: set_batch changed the batch size after set_wall_kinetics; the handle still applies a wall table whose rate '
                             'constants were not recorded for this batch: call set_wall_kinetics again' % method)
        return wall

    def _recorded_flux(self, method, flux):
        """flux, or the wall fluxes this solver was given last"""
        if flux is None:
            if self._obs['flux_stale']:
                raise ValueError('%s: scf_cycle updated the wall fluxes on the device; pass flux= (state["flux"] of the loop)' % method)
            flux = self._obs['flux']
        return flux

    @staticmethod
    def _model_tables(model_or_tables, site_density):
        tables = model_or_tables.tables() if hasattr(model_or_tables, 'tables') else dict(model_or_tables)
        if site_density is not None:
            tables['site_density'] = float(site_density)
        return tables

    def _kinetic_points(self, method, lanes, phiM, csurf, phi_surface):
        """(host, idx, phiM) of a microkinetic call: host: the surface state comes from csurf / phi_surface, not from this handle; idx:
        the lane list (None on the host path with phiM given: one point per entry of phiM); phiM: as given, or that of the lanes"""
        host = csurf is not None or phi_surface is not None
        if lanes is not None:
            idx = np.ascontiguousarray(lanes, dtype=np.int64).reshape(-1)
        elif host and phiM is not None:
            idx = None
        else:
            idx = np.arange(self.B, dtype=np.int64)
        if phiM is None:
            if self._obs['phiM'] is None:
                raise ValueError('%s: no batch was set' % method)
            if idx is not None and len(idx) and (idx.min() < 0 or idx.max() >= self.B):
                raise ValueError('%s: lane index outside [0, %d)' % (method, self.B))
            phiM = np.asarray(self._obs['phiM'], float)[idx]
        return host, idx, phiM

    def _kinetic_common(self, potential_drop, stern_capacitance=None, phi_pzc=None, **more):
        """the arguments every microkinetic library takes; None: the Stern layer this solver was given (set_newton)"""
        o = self._obs
        return dict(potential_drop=potential_drop, stern_capacitance=o['stern_capacitance'] if stern_capacitance is None else stern_capacitance,
                    phi_pzc=o['phi_pzc'] if phi_pzc is None else phi_pzc, **more)

    @staticmethod
    def _impedance_of(admittance):
        """1 / admittance, inf where it is 0"""
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(admittance == 0, np.inf, 1.0 / np.where(admittance == 0, 1.0, admittance))

    @staticmethod
    def _ask(names, needed):
        """the fields to ask a library for: `names` and what the method needs on top of them; _trim deletes the latter afterwards"""
        return list(names) + [k for k in needed if k not in names]

    @staticmethod
    def _trim(res, ask, names):
        for k in ask:
            if k not in names:
                del res[k]
        return res

    def get_electrolyte(self, fields=None, scalars=True, species_H=-1, species_OH=-1, max_waves=0):
        """Electrolyte observables of the physical mode derived on the device (include/catint_observe.h): a dict of the rows named in
        `fields` (catint_amd._observe.FIELDS; None: all of them; without species_H and species_OH no 'pH') and, with scalars, 'scalars'
        [B][NSCALARS] (columns: catint_amd._observe.SCALARS).  D, charges, ion radii, grid and velocity are the ones this solver was
        given.  Only what is asked for crosses PCIe: a scalars-only call moves 80 bytes per operating point."""
        from . import _observe
        observer = self._satellite('_observer')
        names = list(_observe.FIELDS) if fields is None else list(fields)
        if species_H < 0 and species_OH < 0 and fields is None:
            names.remove('pH')
        o = self._obs
        return observer.electrolyte(self.device_view(), o['D'], o['charges'], o['x'], o['beta'], mpb_radius=o['mpb_radius'],
                                    velocity=o['velocity'], species_H=species_H, species_OH=species_OH, fields=names, scalars=scalars,
                                    max_waves=max_waves)

    def get_balance(self, fields=None, scalars=True, flux=None, phiM=None, max_waves=0):
        """The per-species picture of the physical mode derived on the device (include/catint_balance.h): a dict of the rows named in
        `fields` (catint_amd._balance.FIELDS: 'flux' [B][N][nx-1], 'reaction_rate' [B][R][nx], 'source' [B][N][nx], 'wall_rate' [B][n_wall],
        'wall_flux' [B][N], 'imbalance' [B][N][nx]; None: all of them) and, with scalars, 'scalars' [B][N][NSCALARS] (columns:
        catint_amd._balance.SCALARS).  D, charges, ion radii, grid, velocity, reactions and wall table are the ones this solver was
        given; flux [B][N] and phiM [B] default to what set_batch / set_flux / set_pb / solve_surface(flux=...) were given last.
        After scf_cycle the wall fluxes live on the device and the recorded ones are stale: pass `flux` = state['flux'] of the loop
        (ValueError otherwise).  The loop's solves took the wall reactions through that flux, not through the wall table, so until the
        next solve_stationary / solve_surface / step the balance is formed without the table: 'wall_flux' is the flux passed,
        'wall_rate' is empty.  After a set_batch with another batch size the recorded rate constants of the wall table are not the
        ones the handle applies: ValueError until set_wall_kinetics is called again."""
        o = self._obs
        wall = self._wall_table('get_balance')
        flux = self._recorded_flux('get_balance', flux)
        phiM = o['phiM'] if phiM is None else phiM
        if flux is None or phiM is None:
            raise ValueError('get_balance: no batch was set')
        return self._satellite('_balancer').species(self.device_view(), o['D'], o['charges'], o['x'], o['beta'], flux, phiM,
                                                    mpb_radius=o['mpb_radius'], velocity=o['velocity'], reactions=o['reactions'], wall=wall,
                                                    fields=fields, scalars=scalars, max_waves=max_waves)

    def get_response(self, omega=(0.0,), perturbation='phiM', lanes=None, profiles=False, max_waves=0):
        """The linear response of the stationary state this handle holds (include/catint_response.h), solved on the device: how the
        state answers a small change of the electrode potential (perturbation='phiM', per volt) or of the prescribed wall flux of
        species k (('flux', k), per mol m^-2 s^-1), for every lane of `lanes` (None: all, in order; repeats allowed) and every angular
        frequency of `omega` (rad/s, >= 0; 0: the exact tangent of the stationary solution).  Returns a dict of complex128 arrays:
        'dphi_surface' [n][F], 'dc_surface' [n][F][N], 'dsigma' [n][F] (C m^-2), 'dwall_flux' [n][F][N], 'admittance' [n][F] (A m^-2),
        with profiles 'dc' [n][F][N][nx] and 'dphi' [n][F][nx]; 'status' [n][F] (0; 1: non-finite result or vanishing pivot; 2: the
        lane's solver status was not 0, outputs NaN); and 'omega' [F], 'impedance' = 1 / admittance (inf where the admittance is 0),
        'differential_capacitance' [n] = Re dsigma at the first omega = 0 of the list (absent without one; F m^-2 for 'phiM').
        D, charges, ion radii, grid, wall model, velocity, reactions, wall table and electrode potentials are the ones this solver was
        given.  Rate constants (set_wall_kinetics k) are numbers per lane and are held fixed: a dependence of a rate on the potential is
        part of the response only through `alpha`, never through a host function K(phiM) that produced k.  'status' 1 also marks a
        system whose elimination met a pivot more than 1e8 times smaller than an entry below it (CATRESP_PIVOT_GROWTH_LIMIT): its
        numbers must not be used.  The response is that of the STATIONARY operator about the state found: after a transient step it has no physical
        meaning.  After scf_cycle the solves took the wall reactions through the prescribed flux, so the response is formed without
        the wall table (the rule of get_balance); after a set_batch with another batch size the recorded rate constants of the wall
        table are not the ones the handle applies: ValueError until set_wall_kinetics is called again."""
        o = self._obs
        wall = self._wall_table('get_response')
        if o['phiM'] is None:
            raise ValueError('get_response: no batch was set')
        responder = self._satellite('_responder')
        om = np.atleast_1d(np.asarray(omega, float)).reshape(-1)
        out = responder.solve(self.device_view(), o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], o['phiM'], omega=om,
                              perturbation=perturbation, lanes=lanes, mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'],
                              stern_capacitance=o['stern_capacitance'], velocity=o['velocity'], reactions=o['reactions'], wall=wall,
                              profiles=profiles, max_waves=max_waves)
        out['omega'] = om.copy()
        out['impedance'] = self._impedance_of(out['admittance'])
        zero = np.flatnonzero(om == 0.0)
        if len(zero):
            out['differential_capacitance'] = out['dsigma'][:, zero[0]].real.copy()
        return out

    def get_kinetics(self, model_or_tables, phiM=None, lanes=None, csurf=None, phi_surface=None, theta_guess=None, fields=None,
                     potential_drop='stern', stern_capacitance=None, phi_pzc=None, sigma=None, off=None, gamma=None, site_density=None,
                     tol=None, maxit=None, max_waves=0, rescue=False, ramp=None):
        """The steady state of a mean-field surface microkinetic model (include/catint_kinetics.h) solved on the device, one operating
        point per entry of `lanes` (None: all lanes, in order; repeats allowed): coverages, step rates, the wall fluxes into the
        electrolyte and, when asked for, their sensitivities to the surface concentrations and potentials.  model_or_tables: a
        catint_amd.microkinetics.MeanFieldModel or the dict of its tables().  The surface state is the one this handle holds on the
        device (nothing crosses PCIe on the way in), or csurf [n][N] and phi_surface [n] when given (what an SCF loop holds: the mixed
        surface concentrations).  phiM [n] defaults to the electrode potentials of the selected lanes, stern_capacitance and phi_pzc to
        the ones this solver was given (set_newton); sigma [n], off [n][R][2], gamma [n][N] and theta_guess [n][S+1] are per selected
        point.  fields: names out of catint_amd._kinetics.FIELDS (None: 'theta', 'rate', 'rate_gross', 'flux', 'flux_scale'; also
        'dflux_dc' [n][N][N], 'dflux_dphi' [n][N][2]).  Returns a dict of these arrays and 'status' [n] (0 converged; 1 stopped at
        maxit; 2 the lane's solver status is not 0 or an input is not finite: NaN; 3 a zero or non-finite pivot), 'iterations' [n].
        The number of digits of 'flux' is what flux / flux_scale leaves of 16.
        rescue=True (default False: the call above and nothing else; needs theta_guess None): the points that come back with status 1
        or 3 are integrated in time from the uniform start until they are stationary (include/catint_kintrans.h: to 1e12 s with rtol
        1e-2, stopped at a scaled residual of 1e-6) and the ones that get there are solved again from that state; the rows of those
        that now converge replace the failed ones and the result gains 'rescued' [n] (bool).  A point whose second solve fails as
        well keeps its first rows and status.
        A model with lateral interactions or several site types (catint_amd.interactions.InteractingModel, or a dict with its keys)
        goes to include/catint_interact.h instead: theta_guess is [n][T], fields come from catint_amd._interact.FIELDS (also
        'energy_shift' [n][S] in kT), the result gains 'ramp_reached' [n], and ramp is the number of stages the interaction strength
        is raised in (None: 10 from the uniform start, 1 from a theta_guess).  rescue=True is an error there: the transient library
        is mean-field."""
        from . import _kinetics
        from .interactions import has_interactions
        if rescue and theta_guess is not None:
            raise ValueError('get_kinetics: rescue=True starts from the uniform surface and excludes theta_guess')
        tables = self._model_tables(model_or_tables, site_density)
        host, idx, phiM = self._kinetic_points('get_kinetics', lanes, phiM, csurf, phi_surface)
        interacting = has_interactions(tables)
        if interacting:
            from . import _interact
            if rescue:
                raise ValueError('get_kinetics: rescue=True integrates the mean-field model (include/catint_kintrans.h); this model has '
                                 'lateral interactions or several site types')
        elif ramp is not None:
            raise ValueError('get_kinetics: ramp belongs to a model with lateral interactions or several site types')
        solver = self._satellite('_interact' if interacting else '_kinetics')
        view = None if host else self.device_view()
        common = self._kinetic_common(potential_drop, stern_capacitance, phi_pzc, tol=_kinetics.DEFAULT_TOL if tol is None else tol,
                                      maxit=_kinetics.DEFAULT_MAXIT if maxit is None else maxit, fields=fields, max_waves=max_waves)
        if interacting:
            return solver.solve(view, tables, phiM, lanes=None if host else idx, csurf=csurf, phi_surface=phi_surface, sigma=sigma, off=off,
                                gamma=gamma, theta_guess=theta_guess,
                                ramp=(_interact.SCF_RAMP if theta_guess is None else 1) if ramp is None else ramp, **common)
        res = solver.solve(view, tables, phiM, lanes=None if host else idx, csurf=csurf, phi_surface=phi_surface, sigma=sigma, off=off,
                           gamma=gamma, theta_guess=theta_guess, **common)
        if rescue:
            from . import _kintrans
            _kintrans.rescue(solver, self._satellite('_transient'), view, tables, phiM, res, lanes=None if host else idx,
                             per_point=dict(csurf=csurf, phi_surface=phi_surface, sigma=sigma, off=off, gamma=gamma), **common)
        return res

    def get_kinetics_transient(self, model_or_tables, t_out, phiM=None, lanes=None, csurf=None, phi_surface=None, theta0=None, rtol=1e-4,
                               atol=1e-12, steady_tol=0.0, fields=None, potential_drop='stern', stern_capacitance=None, phi_pzc=None,
                               sigma=None, off=None, gamma=None, site_density=None, h0=0.0, newton_tol=None, newton_maxit=None, max_steps=None,
                               max_waves=0):
        """The transient of the microkinetic model at a constant surface state (include/catint_kintrans.h) integrated on the device, one
        operating point per entry of `lanes`, every point with its own step size: how the coverages relax after a step of the potential
        or of the surface concentrations, and the kinetic time scale to set beside the transport's (get_modes).  The model, the surface
        state (this handle's, or csurf and phi_surface) and phiM, stern_capacitance, phi_pzc, sigma, off, gamma are those of
        get_kinetics.  t_out [n_out]: output times in s, positive and increasing, common to the points; theta0 [n][S+1]: the coverages
        at t = 0, e.g. get_kinetics(...)['theta'] at the state before the step (the free-site entry is recomputed from the site
        balance), None: the uniform surface.  rtol, atol: per step, on the coverages; steady_tol > 0 stops a point whose scaled
        residual max |G_s| / D_s falls below it.  fields: names out of catint_amd._kintrans.FIELDS (None: all).  Returns a dict of
        'theta' [n][n_out][S+1], 'flux', 'flux_scale' [n][n_out][N], 'drift' [n][n_out], 't_reached' [n], 'status' [n] (0 every output
        time reached; 1 stopped stationary, the remaining rows hold that state; 2 unsolved lane or non-finite input: NaN; 3 max_steps
        were not enough, the rows not reached are NaN) and 'steps' [n][3] (accepted, rejected, Newton iterations)."""
        from . import _kintrans
        tables = self._model_tables(model_or_tables, site_density)
        host, idx, phiM = self._kinetic_points('get_kinetics_transient', lanes, phiM, csurf, phi_surface)
        return self._satellite('_transient').solve(
            None if host else self.device_view(), tables, phiM, t_out, lanes=None if host else idx, csurf=csurf, phi_surface=phi_surface,
            theta0=theta0, rtol=rtol, atol=atol, steady_tol=steady_tol, h0=h0,
            newton_tol=_kintrans.DEFAULT_NEWTON_TOL if newton_tol is None else newton_tol,
            newton_maxit=_kintrans.DEFAULT_NEWTON_MAXIT if newton_maxit is None else newton_maxit,
            max_steps=_kintrans.DEFAULT_MAX_STEPS if max_steps is None else max_steps, fields=fields, max_waves=max_waves,
            **self._kinetic_common(potential_drop, stern_capacitance, phi_pzc, sigma=sigma, off=off, gamma=gamma))

    def get_voltammogram(self, model_or_tables, E_start, E_vertex, scan_rate, n_segments=2, samples=200, electrons=None, lanes=None, csurf=None,
                         phi_surface=None, theta0=None, rtol=None, atol=None, rate_floor=None, kT=None, fields=None, potential_drop='stern',
                         stern_capacitance=None, phi_pzc=None, sigma=None, off=None, gamma=None, site_density=None, h0=0.0, newton_tol=None,
                         newton_maxit=None, max_steps=None, max_waves=0, hold_time=None, start_ramp=None):
        """The voltammogram of the microkinetic model at a constant surface state (include/catint_voltam.h) integrated on the device,
        one operating point per entry of `lanes`, every point with its own potential program and step size: the adsorption and
        desorption peaks of a linear or cyclic sweep, their shift with the scan rate and the charge under them.  The model, the surface
        state (this handle's, or csurf and phi_surface), stern_capacitance, phi_pzc, sigma, off, gamma and the handling of lanes are
        those of get_kinetics_transient; the electrode potential of the lanes is replaced by the program: E_start, E_vertex [n] in V
        (a scalar: the same for every point), scan_rate [n] in V/s, n_segments segments of `samples` output times each.  electrons [R]:
        None takes the model's electrons() (a dict of tables needs them given).  Everything else, and the dict returned ('theta',
        'current', 'current_scale', 'charge', 'E_out', 't_reached', 'mean_current', 'status', 'steps'), is that of
        catint_amd.voltammetry.Voltammetry.sweep.  The electrolyte does not answer the sweep: its surface concentrations and surface
        potential stay what they are.
        A model with lateral interactions or several site types (catint_amd.interactions.InteractingModel, or a dict with its keys)
        goes to include/catint_iasweep.h instead (catint_amd.iasweep.InteractingVoltammetry.sweep): theta0 and 'theta' have T = G + S
        columns, fields may name 'energy_shift' [n][n_out][S], hold_time [n] holds the points whose E_vertex equals E_start at that
        potential, and start_ramp is the number of stages of the steady solve at E_start (None: 10 from the uniform start, 1 with
        theta0).  hold_time and start_ramp are errors for a mean-field model.
        The context of the library is opened for this call and closed after it: for repeated sweeps hold a
        catint_amd.voltammetry.Voltammetry (catint_amd.iasweep.InteractingVoltammetry) and call its sweep with device_view()."""
        from . import voltammetry
        from .interactions import has_interactions
        model = model_or_tables if hasattr(model_or_tables, 'tables') else None
        tables = self._model_tables(model_or_tables, site_density)
        if electrons is None and model is not None:
            electrons = model.electrons()
        if kT is None and model is not None:
            kT = model.kT
        if lanes is None and csurf is None and phi_surface is None:
            n = self.B
        elif lanes is not None:
            n = np.size(lanes)
        else:
            n = np.size(phi_surface) if phi_surface is not None else np.size(E_start)
        es = np.broadcast_to(np.asarray(E_start, float).reshape(-1), (n,)) if np.size(E_start) == 1 else np.asarray(E_start, float).reshape(-1)
        host, idx, es = self._kinetic_points('get_voltammogram', lanes, es, csurf, phi_surface)
        opts = {k: v for k, v in dict(rtol=rtol, atol=atol, newton_tol=newton_tol, newton_maxit=newton_maxit, max_steps=max_steps).items()
                if v is not None}
        more = {}
        if has_interactions(tables):
            from . import iasweep
            opened = iasweep.InteractingVoltammetry
            more = dict(hold_time=hold_time, start_ramp=start_ramp)
        elif hold_time is not None or start_ramp is not None:
            raise ValueError('get_voltammogram: hold_time and start_ramp belong to a model with lateral interactions or several site types')
        else:
            opened = voltammetry.Voltammetry
        with opened(self._obs['device']) as vm:
            return vm.sweep(None if host else self.device_view(), tables, electrons, es, E_vertex, scan_rate, n_segments=n_segments,
                            samples=samples, lanes=None if host else idx, csurf=csurf, phi_surface=phi_surface, theta0=theta0,
                            rate_floor=rate_floor, kT=kT, h0=h0, fields=fields, max_waves=max_waves,
                            **self._kinetic_common(potential_drop, stern_capacitance, phi_pzc, sigma=sigma, off=off, gamma=gamma), **opts,
                            **more)

    def get_rate_control(self, model_or_tables, theta=None, phiM=None, lanes=None, csurf=None, phi_surface=None, fields=None,
                         potential_drop='stern', stern_capacitance=None, phi_pzc=None, sigma=None, off=None, gamma=None, site_density=None,
                         residual_tol=1e-8, max_waves=0, kin=None, coupling=None, rf=1.0):
        """The degree of rate control of the microkinetic steady state (include/catint_drc.h), computed on the device, one operating
        point per entry of `lanes`: which transition state and which intermediate control each wall flux.  The arguments and their
        defaults are those of get_kinetics.  theta [n][S+1]: the steady-state coverages at the same arguments (None: get_kinetics is
        called first and its coverages are used).  fields: names out of catint_amd._drc.FIELDS (None: 'drc' [n][R][N] Campbell's degree
        of rate control of step r's transition state for the flux of species k, 'tdrc' [n][S][N] the thermodynamic one of adsorbate
        s + 1, the raw derivatives 'dflux_drc', 'dflux_dG', and 'flux', 'flux_scale'; also 'dflux_dlnkf', 'dflux_dlnkb' [n][R][N],
        'dy_drc' [n][R][S+1]).  Returns a dict of these and 'status' [n] (0; 1: the residual of the state is above residual_tol; 2:
        unsolved lane or non-finite input, NaN; 3: bad pivot), 'residual' [n].  These are INTRINSIC derivatives, at a fixed surface
        state.  With kin (get_kinetics(..., fields=('dflux_dc', 'dflux_dphi')) and coupling (get_coupling's 'T_c', 'T_phi') for the
        same lanes the result also carries the APPARENT ones of the coupled electrode, where the surface state answers the flux
        through mass transport: 'dflux_drc_apparent', 'dflux_dG_apparent' = M^-1 (rf dflux), M = I - rf (K_c T_c + K_phi (x) T_phi)
        formed per point on the host, and 'drc_apparent', 'tdrc_apparent' normalised by rf flux (NaN rows where M is singular).
        A model with lateral interactions or several site types (catint_amd.interactions.InteractingModel, or a dict with its keys)
        goes to include/catint_iacontrol.h instead (catint_amd.iacontrol.InteractingRateControl.solve): the Jacobian carries the
        coverage dependence of the energies, theta and 'dy_drc' have T = G + S columns, fields come from
        catint_amd.iacontrol.FIELDS, which add 'dflux_dstrength' [n][N], 'dy_dstrength' [n][T] and 'strength_control' [n][N] =
        strength dflux_dstrength / flux, the share of each flux owed to the interactions (with kin and coupling also
        'dflux_dstrength_apparent', 'strength_control_apparent').  The context of that library is opened for this call and closed
        after it: for repeated calls hold a catint_amd.iacontrol.InteractingRateControl and call its solve with device_view()."""
        from . import _drc
        from .interactions import has_interactions
        tables = self._model_tables(model_or_tables, site_density)
        if (kin is None) != (coupling is None):
            raise ValueError('get_rate_control: kin and coupling come together')
        host, idx, phiM = self._kinetic_points('get_rate_control', lanes, phiM, csurf, phi_surface)
        common = self._kinetic_common(potential_drop, stern_capacitance, phi_pzc, sigma=sigma, off=off, gamma=gamma)
        if theta is None:
            theta = self.get_kinetics(tables, phiM=phiM, lanes=lanes, csurf=csurf, phi_surface=phi_surface, fields=('theta',), max_waves=max_waves,
                                      **common)['theta']
        interacting = has_interactions(tables)
        if interacting:
            from . import iacontrol
        names = list((iacontrol if interacting else _drc).DEFAULT_FIELDS) if fields is None else list(fields)
        needed = ('dflux_drc', 'dflux_dG', 'flux') + (('dflux_dstrength',) if interacting else ())
        ask = self._ask(names, needed if kin is not None else ())
        args = (None if host else self.device_view(), tables, phiM, theta)
        kw = dict(lanes=None if host else idx, csurf=csurf, phi_surface=phi_surface, residual_tol=residual_tol, fields=ask, max_waves=max_waves,
                  **common)
        if interacting:
            with iacontrol.InteractingRateControl(self._obs['device']) as rc:
                res = rc.solve(*args, **kw)
        else:
            res = self._satellite('_rate_control').solve(*args, **kw)
        if kin is not None:
            for raw, norm in (('dflux_drc', 'drc'), ('dflux_dG', 'tdrc')):
                res[raw + '_apparent'] = _drc.apparent(res[raw], kin, coupling, rf=rf)
                res[norm + '_apparent'] = _drc.normalised(res[raw + '_apparent'], rf * res['flux'], tables['nu'])
            if interacting:
                one = _drc.apparent(res['dflux_dstrength'][:, None, :], kin, coupling, rf=rf)
                res['dflux_dstrength_apparent'] = one[:, 0, :]
                res['strength_control_apparent'] = float(tables.get('strength', 1.0)) * _drc.normalised(one, rf * res['flux'], tables['nu'])[:, 0, :]
        return self._trim(res, ask, names)

    def get_coupling(self, flux, kin, rf=1.0, lanes=None, dphi_max=0.05, fields=None, max_waves=0):
        """One Newton step of the self-consistency between kinetics and transport (include/catint_couple.h), formed on the device
        about the stationary state this handle holds, for every lane of `lanes` (None: all, in order; repeats allowed).  flux [B][N]:
        the prescribed wall fluxes the state was solved with (what set_flux / solve_surface were given; None: the recorded ones).
        kin: the kinetic half at that state, indexed by the position in the call as get_kinetics(lanes=lanes, fields=('flux',
        'dflux_dc', 'dflux_dphi')) returns it: 'flux' [n][N], 'dflux_dc' [n][N][N], 'dflux_dphi' [n][N][2] (its column d/d phi_0 is
        used).  rf: the roughness factor, the transport sees rf times the kinetic flux.  Returns a dict of the rows named in `fields`
        (catint_amd._couple.FIELDS; None: all): 'T_c' [n][N][N] = d c_k(0) / d flux_j and 'T_phi' [n][N] = d phi(0) / d flux_j (all
        columns from one elimination), 'dflux' [n][N] the Newton step, 'lambda' [n] its damping (no positive surface concentration
        falls below a tenth of its value, the surface potential moves by dphi_max at most; dphi_max <= 0: no limit), 'flux_new' [n][N]
        = flux + lambda dflux, 'dc_surface' [n][N] and 'dphi_surface' [n] the predicted change of the surface state; and 'status' [n]
        (0; 1: non-finite number or failed pivot check in the elimination; 2: the lane's solver status was not 0 or an input is not
        finite, outputs NaN; 3: the Newton matrix is singular).  D, charges, ion radii, grid, wall model, velocity and reactions are the
        ones this solver was given.  The state must have been solved with prescribed fluxes only: with a wall table set
        (set_wall_kinetics) the call raises ValueError."""
        o = self._obs
        if o['wall'] is not None and not o['explicit_kinetics']:
            raise ValueError('get_coupling: the handle applies a wall table (set_wall_kinetics); the coupling is defined for a state solved '
                             'with prescribed wall fluxes only')
        if flux is None:
            if o['flux_stale'] or o['flux'] is None:
                raise ValueError('get_coupling: no recorded wall fluxes; pass flux=')
            flux = o['flux']
        g = np.asarray(_f64(flux, (self.B, self.N)))
        idx = self._lanes('get_coupling', lanes)
        n = len(idx)
        K = np.asarray(kin['flux'], float).reshape(n, self.N)
        Kc = np.asarray(kin['dflux_dc'], float).reshape(n, self.N, self.N)
        Kphi = np.ascontiguousarray(np.asarray(kin['dflux_dphi'], float).reshape(n, self.N, 2)[:, :, 1])
        return self._satellite('_coupler').solve(self.device_view(), o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], g[idx], K, Kc,
                                                 Kphi, rf=rf, dphi_max=dphi_max, lanes=idx, mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'],
                                                 stern_capacitance=o['stern_capacitance'], velocity=o['velocity'], reactions=o['reactions'],
                                                 fields=fields, max_waves=max_waves)

    def get_kinetic_admittance(self, model_or_tables, omega, theta=None, phiM=None, lanes=None, csurf=None, phi_surface=None, fields=None,
                               potential_drop='stern', stern_capacitance=None, phi_pzc=None, sigma=None, off=None, gamma=None,
                               site_density=None, residual_tol=1e-8, max_waves=0):
        """The intrinsic kinetic admittance of the microkinetic model at a fixed surface state (include/catint_eis.h: cateis_kinetic),
        on the device, one operating point per entry of `lanes` and one column per angular frequency of `omega` (rad/s, >= 0): how the
        wall fluxes answer a small harmonic change of the surface concentrations and of the two potentials when the adsorbates store
        charge-free matter, i omega theta.  The model, the surface state (this handle's, or csurf and phi_surface) and phiM,
        stern_capacitance, phi_pzc, sigma, off, gamma are those of get_kinetics; theta [n][S+1]: the stationary coverages (None:
        get_kinetics is called first).  fields: names out of catint_amd._eis.KINETIC_FIELDS and 'residual' (None: 'Kc', 'Kphi',
        'residual').  Returns complex128 'Kc' [n][F][N][N] = dflux_k / dc_j, 'Kphi' [n][F][N][2] = d/dphiM, d/dphi_0, 'dy'
        [n][F][S+1][N+2] = d ln theta, 'residual' [n] = max_s |G_s| / D_s, 'status' [n][F] (0; 2: unsolved lane or non-finite input,
        NaN; 3: bad pivot; 4: residual above residual_tol) and 'omega' [F].  At omega = 0 Kc and Kphi are get_kinetics' dflux_dc and
        dflux_dphi."""
        tables = self._model_tables(model_or_tables, site_density)
        host, idx, phiM = self._kinetic_points('get_kinetic_admittance', lanes, phiM, csurf, phi_surface)
        common = self._kinetic_common(potential_drop, stern_capacitance, phi_pzc, sigma=sigma, off=off, gamma=gamma)
        if theta is None:
            theta = self.get_kinetics(tables, phiM=phiM, lanes=lanes, csurf=csurf, phi_surface=phi_surface, fields=('theta',), max_waves=max_waves,
                                      **common)['theta']
        om = np.atleast_1d(np.asarray(omega, float)).reshape(-1)
        out = self._satellite('_impedance').kinetic(None if host else self.device_view(), tables, phiM, theta, om, lanes=None if host else idx,
                                                    csurf=csurf, phi_surface=phi_surface, residual_tol=residual_tol, fields=fields,
                                                    max_waves=max_waves, **common)
        out['omega'] = om.copy()
        return out

    def get_impedance(self, model_or_tables, omega, theta=None, rf=1.0, lanes=None, fields=None, phiM=None, potential_drop='stern', sigma=None,
                      off=None, gamma=None, site_density=None, residual_tol=1e-8, max_waves=0):
        """The impedance of the working electrode with the microkinetic model at its surface (include/catint_eis.h: cateis_solve), on
        the device, about the stationary state this handle holds: for every lane of `lanes` (None: all, in order; repeats allowed) and
        every angular frequency of `omega` (rad/s, >= 0) the linearised surface kinetics with adsorbate storage, the transport transfer
        functions at the same frequency and the Stern layer are closed at the wall.  The model and phiM, sigma, off, gamma are those of
        get_kinetics; theta [n][S+1]: the stationary coverages (None: get_kinetics is called first); rf: the roughness factor the SCF
        loop used (0: the blocking electrode).  fields: names out of catint_amd._eis.FIELDS (None: 'admittance', 'faradaic',
        'double_layer', 'dflux', 'dc_surface', 'dphi_surface', 'dsigma', 'residual').  Returns complex128 arrays: 'admittance' [n][F] in
        A m^-2 V^-1 = 'double_layer' (i omega dsigma) + 'faradaic' (sum_k q_k dflux_k), 'dflux', 'dc_surface' [n][F][N],
        'dphi_surface', 'dsigma' [n][F] per volt of phiM; on request the transfer functions 'Tc' [n][F][N][N], 'Tphi', 'tc' [n][F][N],
        'tphi' [n][F], the kinetic 'Kc', 'Kphi', 'dy'; 'residual' [n]; 'status' [n][F] (0; 1: failed pivot check in the transport
        elimination; 2: unsolved lane or non-finite input, NaN; 3: singular kinetic or coupled matrix; 4: the coverages are not
        stationary, residual above residual_tol); 'omega' [F]; 'impedance' = 1 / admittance (inf where it is 0);
        'polarization_resistance' [n] = 1 / Re admittance at the first omega = 0 of the list (absent without one): the slope of the
        polarisation curve of the coupled electrode.  'dtheta' [n][F][S+1] = theta_t (sum_j dy_tj dc_j + dy_t,phiM + dy_t,phi0 dphi_0) is
        the answer of the coverages per volt.  It is a field name of this method only (in the default list; otherwise name it in
        `fields`): the library is asked for 'dy', 'dc_surface' and 'dphi_surface', the chain rule is formed on the host, and of those
        three the result keeps the ones `fields` names (the default list names 'dc_surface' and 'dphi_surface', not 'dy').  The state
        must be stationary and solved with prescribed wall fluxes (the SCF loop of the microkinetic model): with a wall table set
        (set_wall_kinetics) the call raises ValueError.  Adsorbates carry no charge of their own and C_S is constant."""
        o = self._obs
        if o['wall'] is not None and not o['explicit_kinetics']:
            raise ValueError('get_impedance: the handle applies a wall table (set_wall_kinetics); the impedance of the microkinetic electrode is '
                             'defined for a state solved with prescribed wall fluxes only')
        if o['phiM'] is None:
            raise ValueError('get_impedance: no batch was set')
        tables = self._model_tables(model_or_tables, site_density)
        idx = self._lanes('get_impedance', lanes)
        if phiM is None:
            phiM = np.asarray(o['phiM'], float)[idx]
        common = self._kinetic_common(potential_drop, sigma=sigma, off=off, gamma=gamma)
        if theta is None:
            theta = self.get_kinetics(tables, phiM=phiM, lanes=idx, fields=('theta',), max_waves=max_waves, **common)['theta']
        om = np.atleast_1d(np.asarray(omega, float)).reshape(-1)
        from . import _eis
        names = list(_eis.DEFAULT_FIELDS) + ['dtheta'] if fields is None else list(fields)
        ask = self._ask([k for k in names if k != 'dtheta'], ('dy', 'dc_surface', 'dphi_surface') if 'dtheta' in names else ())
        out = self._satellite('_impedance').solve(self.device_view(), tables, phiM, theta, om, o['D'], o['charges'], o['x'], o['beta'], o['eps'],
                                                  o['dx'], rf=rf, lanes=idx, mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'],
                                                  velocity=o['velocity'], reactions=o['reactions'], residual_tol=residual_tol, fields=ask,
                                                  max_waves=max_waves, **common)
        out['omega'] = om.copy()
        if 'admittance' in out:
            out['impedance'] = self._impedance_of(out['admittance'])
            zero = np.flatnonzero(om == 0.0)
            if len(zero):
                with np.errstate(divide='ignore', invalid='ignore'):
                    out['polarization_resistance'] = 1.0 / out['admittance'][:, zero[0]].real
        if 'dtheta' in names:
            N = self.N
            dy = out['dy']
            th = np.asarray(theta, float).reshape(len(idx), 1, -1)
            out['dtheta'] = th * (np.einsum('nftj,nfj->nft', dy[..., :N], out['dc_surface']) + dy[..., N] + dy[..., N + 1] * out['dphi_surface'][..., None])
        return self._trim(out, ask, names)

    def get_sensitivities(self, parameters, lanes=None, fields=None, flux=None, max_waves=0):
        """The sensitivities of the stationary state this handle holds to its model parameters (include/catint_sens.h), solved on the
        device: for every lane of `lanes` (None: all, in order; repeats allowed) and every entry of `parameters` the exact derivative
        of the surface state, the charge on the metal and the wall fluxes.  An entry is 'phiM' (per volt), ('flux', k) (the prescribed
        wall flux of species k), ('c_bulk', k), ('c_bulk', weights [N]) (a direction in bulk composition, e.g. an electroneutral salt:
        the weighted sum of the single-species columns, formed on the host), ('D', k), ('kf', r), ('kr', r) (reaction r of
        set_reactions), ('wall_k', r) (the lane's own rate constant of wall reaction r), 'stern_capacitance' or 'velocity'.  Returns a
        dict of the rows named in `fields` (catint_amd._sens.FIELDS; None: all): 'dphi_surface' [n][P], 'dc_surface' [n][P][N], 'dsigma'
        [n][P], 'dwall_flux' [n][P][N], 'dcurrent' [n][P] = sum_k q_k dwall_flux_k; 'status' [n] (0; 1: failed pivot check or non-finite
        number; 2: the lane's solver status was not 0 or an input is not finite, outputs NaN); 'parameters' (the list as given); and
        'elasticity': {'dcurrent' [n][P], 'dwall_flux' [n][P][N]} = d ln|y| / d ln p (what 'dcurrent' and 'dwall_flux' were asked
        for), NaN where y or p is 0; for a direction p is the multiplier of the weights, 1.  Medium, tables, potentials and fluxes are
        the ones this solver was given, with the rules of get_response / get_balance: after scf_cycle pass flux= (ValueError otherwise)
        and the wall table is left out; after a set_batch with another batch size the wall table must be set again (ValueError)."""
        from . import _sens
        o = self._obs
        wall = self._wall_table('get_sensitivities')
        flux = self._recorded_flux('get_sensitivities', flux)
        if flux is None or o['phiM'] is None:
            raise ValueError('get_sensitivities: no batch was set')
        g = np.asarray(_f64(flux, (self.B, self.N)))
        idx = self._lanes('get_sensitivities', lanes)
        n, N = len(idx), self.N
        names = list(_sens.FIELDS) if fields is None else list(fields)
        # the columns the device solves: one per distinct (kind, index); a direction takes the single-species columns it weighs
        specs, cols, plan = list(parameters), {}, []
        if not specs:
            raise ValueError('get_sensitivities: no parameters')

        def column(name, i=0):
            return cols.setdefault((name, int(i)), len(cols))
        for spec in specs:
            if isinstance(spec, str):
                if spec not in _sens.KINDS or spec in _sens.INDEXED:
                    raise ValueError('get_sensitivities: unknown parameter %r' % (spec,))
                plan.append([(column(spec), 1.0)])
            elif spec[0] == 'c_bulk' and np.ndim(spec[1]) > 0:
                wts = np.asarray(spec[1], float).reshape(-1)
                if len(wts) != N:
                    raise ValueError("get_sensitivities: ('c_bulk', weights) needs %d weights" % N)
                plan.append([(column('c_bulk', k), float(wts[k])) for k in range(N) if wts[k] != 0.0])
            else:
                if spec[0] not in _sens.INDEXED:
                    raise ValueError('get_sensitivities: unknown parameter %r' % (spec,))
                plan.append([(column(spec[0], spec[1]), 1.0)])
        if len(cols) > _sens.MAX_PARAMS:
            raise ValueError('get_sensitivities: %d columns, at most %d in one call' % (len(cols), _sens.MAX_PARAMS))
        sensitizer = self._satellite('_sensitizer')
        dev = [k if k[0] in _sens.INDEXED else k[0] for k in sorted(cols, key=cols.get)]
        raw = sensitizer.solve(self.device_view(), o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], o['phiM'], g[idx], dev, lanes=idx,
                               mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'], stern_capacitance=o['stern_capacitance'], phi_pzc=o['phi_pzc'],
                               velocity=o['velocity'], reactions=o['reactions'], wall=wall, fields=names, max_waves=max_waves)
        out = {'status': raw['status'], 'parameters': specs}
        for name in names:
            a = raw[name]
            res = np.empty((n, len(specs)) + a.shape[2:])
            for m, terms in enumerate(plan):
                if len(terms) == 1 and terms[0][1] == 1.0:
                    res[:, m] = a[:, terms[0][0]]
                else:
                    acc = np.zeros((n,) + a.shape[2:])
                    for col, wt in terms:
                        acc = acc + wt * a[:, col]
                    res[:, m] = acc
            out[name] = res
        # elasticities d ln|y| / d ln p of the current and the wall fluxes
        el = {}
        if 'dcurrent' in out or 'dwall_flux' in out:
            q = np.asarray(o['charges'], float)
            wf = g[idx].copy()                                  # the flux into the domain: prescribed + wall table
            if wall is not None:
                cs, vs, _ = self.get_surface()
                al = np.zeros(len(wall['species'])) if wall['alpha'] is None else wall['alpha']
                ks = np.zeros(len(wall['species'])) if wall['saturation'] is None else wall['saturation']
                for r, s in enumerate(wall['species']):
                    c_s = cs[idx, s] if s >= 0 else np.ones(n)
                    gr = c_s / (1.0 + ks[r] * c_s) * np.exp(al[r] * (o['phiM'][idx] - vs[idx]))
                    wf = wf + wall['nu'][r][None, :] * (wall['k'][idx, r] * gr)[:, None]
            pv = np.empty((n, len(specs)))
            for m, spec in enumerate(specs):
                name, i = (spec, 0) if isinstance(spec, str) else (spec[0], spec[1])
                if name == 'phiM':
                    pv[:, m] = o['phiM'][idx]
                elif name == 'flux':
                    pv[:, m] = g[idx, int(i)]
                elif name == 'c_bulk':
                    pv[:, m] = 1.0 if np.ndim(i) > 0 else (np.nan if o['c_bulk'] is None else o['c_bulk'][idx, int(i)])
                elif name == 'D':
                    pv[:, m] = o['D'][int(i)]
                elif name in ('kf', 'kr'):
                    pv[:, m] = o['reactions'][int(i)][2 if name == 'kf' else 3]
                elif name == 'wall_k':
                    pv[:, m] = wall['k'][idx, int(i)]
                elif name == 'stern_capacitance':
                    pv[:, m] = o['stern_capacitance']
                else:
                    pv[:, m] = o['velocity']
            with np.errstate(divide='ignore', invalid='ignore'):
                if 'dcurrent' in out:
                    y = (wf * q[None, :]).sum(axis=1)[:, None]
                    el['dcurrent'] = np.where((y == 0) | (pv == 0), np.nan, out['dcurrent'] * pv / np.where(y == 0, 1.0, y))
                if 'dwall_flux' in out:
                    y = wf[:, None, :]
                    el['dwall_flux'] = np.where((y == 0) | (pv[:, :, None] == 0), np.nan,
                                                out['dwall_flux'] * pv[:, :, None] / np.where(y == 0, 1.0, y))
        out['elasticity'] = el
        return out

    def get_relaxation(self, nmodes=3, subspace=8, iterations=12, lanes=None, rtol=1e-8, profiles=False, start=None, seed=0, max_waves=0):
        """The slowest relaxation modes of the stationary state this handle holds (include/catint_modes.h): perturbations of the state
        decay as exp(-lambda t) with J v = lambda S v, J the Jacobian of the stationary residual and S the storage matrix of
        get_response.  For every lane of `lanes` (None: all, in order; repeats allowed) the device runs `iterations` passes of subspace
        iteration on J^-1 S with `subspace` columns (1 .. 8, at most N (nx - 1)) from `start` [subspace][N+1][nx] (None: standard normal
        numbers of RandomState(seed), the same for every lane); the small eigenproblem is solved here.  Returns a dict: 'rates'
        [n][nmodes] complex, 1/s, ascending in |lambda| (complex pairs are legitimate: J is not symmetric); 'time_constants' = 1 / Re
        lambda (inf where Re lambda = 0); 'residual' [n][nmodes], the relative residual of each Ritz pair; 'converged' = residual <=
        rtol; 'stable' [n] (object): True when every converged rate has Re lambda > 0, False when one has not, None where none
        converged; 'status' [n] (0; 1: failed pivot check or non-finite number; 2: the lane's solver status was not 0 or an input is not
        finite, outputs NaN; 3: Gram-Schmidt breakdown, e.g. linearly dependent start vectors); 'ritz', 'gram' [n][subspace][subspace],
        the device's B = Q^T W and G = (W - Q B)^T (W - Q B) of the last pass; with profiles 'dc' [n][nmodes][N][nx] and 'dphi'
        [n][nmodes][nx], the mode shapes Q s_j (complex, each scaled to unit Euclidean norm).  nmodes is cut to subspace.  Lanes whose
        status is not 0 have NaN rates and residuals and converged False.  Medium, tables and potentials are the ones this solver was
        given, with the rules of get_response: after scf_cycle the wall table is left out; after a set_batch with another batch size
        the wall table must be set again (ValueError)."""
        from . import _modes
        o = self._obs
        wall = self._wall_table('get_relaxation')
        if o['phiM'] is None:
            raise ValueError('get_relaxation: no batch was set')
        idx = self._lanes('get_relaxation', lanes)
        m, N, nx = int(subspace), self.N, self.nx
        if not 1 <= m <= min(_modes.MAX_SUBSPACE, N * (nx - 1)):
            raise ValueError('get_relaxation: subspace = %d outside [1, %d]' % (m, min(_modes.MAX_SUBSPACE, N * (nx - 1))))
        if not 1 <= int(iterations) <= _modes.MAX_ITERATIONS:
            raise ValueError('get_relaxation: iterations = %d outside [1, %d]' % (iterations, _modes.MAX_ITERATIONS))
        if int(nmodes) < 1:
            raise ValueError('get_relaxation: nmodes < 1')
        q0 = _modes.default_start(m, N, nx, seed) if start is None else np.asarray(start, float)
        if q0.shape != (m, N + 1, nx):
            raise ValueError('get_relaxation: start has shape %r, the call needs %r' % (q0.shape, (m, N + 1, nx)))
        raw = self._satellite('_mode_solver').solve(
            self.device_view(), o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], o['phiM'], q0, subspace=m, iterations=iterations,
            lanes=idx, mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'], stern_capacitance=o['stern_capacitance'], velocity=o['velocity'],
            reactions=o['reactions'], wall=wall, fields=['ritz', 'gram'] + (['basis'] if profiles else []), max_waves=max_waves)
        n, k = len(idx), min(int(nmodes), m)
        rates, res = np.full((n, k), np.nan + 0j), np.full((n, k), np.nan)
        stable = np.full(n, None, dtype=object)
        if profiles:
            dc, dphi = np.full((n, k, N, nx), np.nan + 0j), np.full((n, k, nx), np.nan + 0j)
        for i in range(n):
            if raw['status'][i] != 0:
                continue
            theta, s, r = _modes.ritz_pairs(raw['ritz'][i], raw['gram'][i])
            with np.errstate(divide='ignore', invalid='ignore'):
                rates[i] = 1.0 / theta[:k]
            res[i] = r[:k]
            ok = np.isfinite(res[i]) & (res[i] <= rtol)
            if ok.any():
                stable[i] = bool((rates[i][ok].real > 0).all())
            if profiles:
                v = np.einsum('jke,jm->mke', raw['basis'][i], s[:, :k])
                v = v / np.sqrt((np.abs(v) ** 2).sum(axis=(1, 2)))[:, None, None]
                dc[i], dphi[i] = v[:, :N], v[:, N]
        with np.errstate(divide='ignore', invalid='ignore'):
            tau = np.where(rates.real == 0, np.inf, 1.0 / np.where(rates.real == 0, 1.0, rates.real))
        out = {'rates': rates, 'time_constants': tau, 'residual': res, 'converged': np.isfinite(res) & (res <= rtol), 'stable': stable,
               'status': raw['status'], 'ritz': raw['ritz'], 'gram': raw['gram']}
        if profiles:
            out['dc'], out['dphi'] = dc, dphi
        return out

    def get_status(self):
        st = np.zeros(self.B, np.int32)
        self._check(self._lib.pnp_get_status(self._h, _iptr(st)))
        return st

    def synchronize(self):
        self._check(self._lib.pnp_synchronize(self._h))

    def timer_start(self):
        self._check(self._lib.pnp_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float(0)
        self._check(self._lib.pnp_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)

    @property
    def grid(self):
        """The grid x[nx] this solver works on (set_grid, or the uniform one of the constructor)"""
        return self._obs['x']

    @property
    def device_bytes(self):
        return int(self._lib.pnp_device_bytes(self._h))

    @property
    def row_pitch(self):
        return int(self._lib.pnp_row_pitch(self._h))

    def step_row_chunks(self, launches):
        """Row chunks (HIP streams) a step() call of `launches` launches is cut into."""
        return int(self._lib.pnp_step_row_chunks(self._h, int(launches)))
