"""In-tree build of the HIP library (gfx950 only; cross-compiles without a GPU)."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
LIB_DIR = os.path.join(_HERE, 'lib')
LIB = os.path.join(LIB_DIR, 'libcatint_pnp.so')
SOURCES = ['pnp_kernels.hip', 'pnp_stream.hip', 'pnp_newton.hip', 'pnp_lane.hip', 'pnp_lane2.hip', 'pnp_lane4.hip', 'pnp_scf.hip', 'pnp_ode.hip', 'pnp_rkc.hip', 'pnp_capi.hip']
HEADERS = [os.path.join(CSRC, 'pnp_internal.h'), os.path.join(CSRC, 'pnp_lane_common.h'), os.path.join(CSRC, 'pnp_lane_cols.h'), os.path.join(CSRC, 'pnp_wave.h'), os.path.join(CSRC, 'pnp_step_table.h'), os.path.join(CSRC, 'pnp_math.h'), os.path.join(CSRC, 'pnp_dop853_coeffs.h'), os.path.join(_HERE, '..', 'include', 'catint_pnp.h')]
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-Wall', '-Wno-unused-function']


_INCLUDE = os.path.join(_HERE, '..', 'include')
# what every library that derives quantities from a device-resident state includes (csrc/pnp_post.h); tests/test_build_deps.py follows
# the #include lines of the first three libraries and compares with the lists here (tests/test_regrid_abi.py: the fourth)
_POST_HEADERS = [os.path.join(CSRC, h) for h in ('pnp_post.h', 'pnp_stage.h', 'pnp_wave.h', 'pnp_math.h', 'pnp_internal.h')] + [os.path.join(_INCLUDE, 'catint_pnp.h')]
# what the two libraries that eliminate the stationary Jacobian with a team of lanes per system include on top (csrc/pnp_team.h)
_TEAM_HEADERS = _POST_HEADERS + [os.path.join(CSRC, 'pnp_team.h')]
# what the two libraries that work on a microkinetic model with one operating point per lane include on top (csrc/pnp_kin.h)
_KIN_HEADERS = _POST_HEADERS + [os.path.join(CSRC, 'pnp_kin.h')]

# second library (include/catint_observe.h): observables derived from a device-resident state.  Its kernels stay out of SOURCES:
# the solver library holds the solver's kernels and nothing else (tests/test_kernel_census.py)
OBSERVE_DIR = os.path.join(CSRC, 'observe')
OBSERVE_LIB = os.path.join(LIB_DIR, 'libcatint_observe.so')
OBSERVE_SOURCES = ['catobs.hip']
OBSERVE_HEADERS = _POST_HEADERS + [os.path.join(_INCLUDE, 'catint_observe.h')]

# third library (include/catint_balance.h): species fluxes, reaction rates and the discrete mass balance of a device-resident state.  The
# kernel and symbol sets of the other two libraries are pinned by their tests, so it is a library of its own
BALANCE_DIR = os.path.join(CSRC, 'balance')
BALANCE_LIB = os.path.join(LIB_DIR, 'libcatint_balance.so')
BALANCE_SOURCES = ['catbal.hip']
BALANCE_HEADERS = _POST_HEADERS + [os.path.join(_INCLUDE, 'catint_balance.h')]

# fourth library (include/catint_regrid.h): a device-resident state resampled onto another grid.  Again a library of its own: the kernel
# and symbol sets of the other three stay what their tests pin
REGRID_DIR = os.path.join(CSRC, 'regrid')
REGRID_LIB = os.path.join(LIB_DIR, 'libcatint_regrid.so')
REGRID_SOURCES = ['catgrid.hip']
REGRID_HEADERS = _POST_HEADERS + [os.path.join(_INCLUDE, 'catint_regrid.h')]

# fifth library (include/catint_equil.h): the zero-flux (Poisson-Boltzmann) state of the physical mode solved on the device.  A library of
# its own for the same reason: the solver library's kernel set is pinned (tests/test_kernel_census.py), and so are the other three
EQUIL_DIR = os.path.join(CSRC, 'equil')
EQUIL_LIB = os.path.join(LIB_DIR, 'libcatint_equil.so')
EQUIL_SOURCES = ['cateq.hip']
EQUIL_HEADERS = _POST_HEADERS + [os.path.join(_INCLUDE, 'catint_equil.h')]

# sixth library (include/catint_response.h): the linear response of a stationary state (differential capacitance, slope of the currents,
# admittance spectrum), one block-tridiagonal solve per operating point and frequency.  A library of its own as the four before it
RESPONSE_DIR = os.path.join(CSRC, 'response')
RESPONSE_LIB = os.path.join(LIB_DIR, 'libcatint_response.so')
RESPONSE_SOURCES = ['catresp.hip']
RESPONSE_HEADERS = _TEAM_HEADERS + [os.path.join(_INCLUDE, 'catint_response.h')]

# seventh library (include/catint_kinetics.h): the steady state of a mean-field surface microkinetic model per operating point, and the
# wall fluxes and sensitivities that follow from it.  A library of its own as the five before it
KINETICS_DIR = os.path.join(CSRC, 'kinetics')
KINETICS_LIB = os.path.join(LIB_DIR, 'libcatint_kinetics.so')
KINETICS_SOURCES = ['catkin.hip']
KINETICS_HEADERS = _KIN_HEADERS + [os.path.join(_INCLUDE, 'catint_kinetics.h')]

# eighth library (include/catint_couple.h): one Newton step of the self-consistency between kinetics and transport per operating
# point -- the transport tangent from one block elimination, the Newton matrix and the damped step at the wall.  A library of its
# own as the six before it
COUPLE_DIR = os.path.join(CSRC, 'couple')
COUPLE_LIB = os.path.join(LIB_DIR, 'libcatint_couple.so')
COUPLE_SOURCES = ['catcpl.hip']
COUPLE_HEADERS = _TEAM_HEADERS + [os.path.join(_INCLUDE, 'catint_couple.h')]

# ninth library (include/catint_sens.h): the sensitivities of a stationary state to its model parameters (bulk concentrations, diffusion
# coefficients, rate constants, Stern capacitance, velocity) -- right-hand sides at every grid row carried through the team's block
# elimination.  A library of its own as the seven before it
SENS_DIR = os.path.join(CSRC, 'sens')
SENS_LIB = os.path.join(LIB_DIR, 'libcatint_sens.so')
SENS_SOURCES = ['catsens.hip']
SENS_HEADERS = _TEAM_HEADERS + [os.path.join(_INCLUDE, 'catint_sens.h')]

# tenth library (include/catint_drc.h): the degree of rate control of a microkinetic steady state -- the derivatives of the wall fluxes
# with respect to every rate constant, transition state and adsorbate energy from one factorisation per operating point.  A library of
# its own as the eight before it
DRC_DIR = os.path.join(CSRC, 'drc')
DRC_LIB = os.path.join(LIB_DIR, 'libcatint_drc.so')
DRC_SOURCES = ['catdrc.hip']
DRC_HEADERS = _KIN_HEADERS + [os.path.join(_INCLUDE, 'catint_drc.h')]

# eleventh library (include/catint_modes.h): the relaxation modes of a stationary state -- a subspace iteration on J^-1 S per operating
# point, every pass one team block elimination with the subspace as carried right-hand sides, records and a substitution to the bulk, all
# passes inside one launch.  A library of its own as the nine before it
MODES_DIR = os.path.join(CSRC, 'modes')
MODES_LIB = os.path.join(LIB_DIR, 'libcatint_modes.so')
MODES_SOURCES = ['catmodes.hip']
MODES_HEADERS = _TEAM_HEADERS + [os.path.join(_INCLUDE, 'catint_modes.h')]

# twelfth library (include/catint_scfkin.h): the wall fluxes of the microkinetic model inside the device SCF loop -- the function
# pnp_scf_cycle_fn calls once per iteration, one launch, the coverages of every lane kept on the device as the next start.  A library of
# its own as the ten before it: the kinetics library is pinned to one kernel and six symbols (tests/test_kinetics_abi.py)
SCFKIN_DIR = os.path.join(CSRC, 'scfkin')
SCFKIN_LIB = os.path.join(LIB_DIR, 'libcatint_scfkin.so')
SCFKIN_SOURCES = ['catscfkin.hip']
SCFKIN_HEADERS = _KIN_HEADERS + [os.path.join(_INCLUDE, 'catint_scfkin.h')]

# thirteenth library (include/catint_kintrans.h): the transient of the microkinetic model -- implicit Euler with step doubling in the
# log-coverages, every operating point with its own step size, all steps inside one launch.  A library of its own as the eleven before it
KINTRANS_DIR = os.path.join(CSRC, 'kintrans')
KINTRANS_LIB = os.path.join(LIB_DIR, 'libcatint_kintrans.so')
KINTRANS_SOURCES = ['catkt.hip']
KINTRANS_HEADERS = _KIN_HEADERS + [os.path.join(_INCLUDE, 'catint_kinetics.h'), os.path.join(_INCLUDE, 'catint_kintrans.h')]

# fourteenth library (include/catint_eis.h): the impedance of the microkinetic electrode -- the linearised surface kinetics with adsorbate
# storage per (operating point, frequency) in one kernel, the transport transfer functions at the same frequency and the closure at the
# wall in a second one that reads what the first wrote.  It includes both shared headers.  A library of its own as the twelve before it
EIS_DIR = os.path.join(CSRC, 'eis')
EIS_LIB = os.path.join(LIB_DIR, 'libcatint_eis.so')
EIS_SOURCES = ['cateis.hip']
EIS_HEADERS = _POST_HEADERS + [os.path.join(CSRC, 'pnp_team.h'), os.path.join(CSRC, 'pnp_kin.h'), os.path.join(_INCLUDE, 'catint_eis.h')]

# fifteenth library (include/catint_interact.h): the steady state of a microkinetic model with lateral interactions and several site types
# -- coverage-dependent rate constants, one site row per type, the interaction strength ramped in stages inside one launch.  It includes
# pnp_kin.h as it is.  A library of its own as the thirteen before it: the kinetics library is pinned to one kernel and six symbols
INTERACT_DIR = os.path.join(CSRC, 'interact')
INTERACT_LIB = os.path.join(LIB_DIR, 'libcatint_interact.so')
INTERACT_SOURCES = ['catia.hip']
INTERACT_HEADERS = _KIN_HEADERS + [os.path.join(_INCLUDE, 'catint_interact.h')]

# sixteenth library (include/catint_voltam.h): the voltammogram of the microkinetic model -- the implicit Euler integrator of the thirteenth
# along a linear potential program, the current in the error norm and the extrapolated state accepted, with current and charge as outputs.
# It includes pnp_kin.h as it is.  A library of its own as the fourteen before it: the method's definition differs from the thirteenth's,
# whose bits are pinned
VOLTAM_DIR = os.path.join(CSRC, 'voltam')
VOLTAM_LIB = os.path.join(LIB_DIR, 'libcatint_voltam.so')
VOLTAM_SOURCES = ['catvm.hip']
VOLTAM_HEADERS = _KIN_HEADERS + [os.path.join(_INCLUDE, 'catint_kinetics.h'), os.path.join(_INCLUDE, 'catint_voltam.h')]

# seventeenth library (include/catint_iasweep.h): the voltammogram of the model of the fifteenth library -- the step loop of the sixteenth
# over coverage-dependent rate constants and one site row per type, and a hold at constant potential.  It includes pnp_kin.h as it is and
# restates what it takes from the two.  A library of its own as the fifteen before it: the bits and the kernel sets of both are pinned
IASWEEP_DIR = os.path.join(CSRC, 'iasweep')
IASWEEP_LIB = os.path.join(LIB_DIR, 'libcatint_iasweep.so')
IASWEEP_SOURCES = ['catis.hip']
IASWEEP_HEADERS = _KIN_HEADERS + [os.path.join(_INCLUDE, h) for h in ('catint_kinetics.h', 'catint_interact.h', 'catint_voltam.h', 'catint_iasweep.h')]

# eighteenth library (include/catint_iacontrol.h): the degree of rate control of the model of the fifteenth library -- the columns and the
# refinement step of the tenth over the full Jacobian of the fifteenth, and a column for the interaction strength.  It includes pnp_kin.h as
# it is and restates what it takes from the two.  A library of its own as the seventeen before it: the bits and the kernel sets of both are
# pinned
IACONTROL_DIR = os.path.join(CSRC, 'iacontrol')
IACONTROL_LIB = os.path.join(LIB_DIR, 'libcatint_iacontrol.so')
IACONTROL_SOURCES = ['catic.hip']
IACONTROL_HEADERS = _KIN_HEADERS + [os.path.join(_INCLUDE, 'catint_iacontrol.h')]

# test-only harness (tests/csrc/primitives_harness.hip): the shared device functions of the headers below, each behind a kernel of its own
# in namespace catunit (tests/test_gpu_primitives.py).  Not part of the product: nothing links against it and no package module loads it
UNITTEST_DIR = os.path.join(_HERE, '..', 'tests', 'csrc')
UNITTEST_LIB = os.path.join(LIB_DIR, 'libcatint_unittest.so')
UNITTEST_SOURCES = ['primitives_harness.hip']
UNITTEST_HEADERS = _KIN_HEADERS + [os.path.join(CSRC, 'pnp_lane_common.h'), os.path.join(CSRC, 'pnp_lane_cols.h')]

PARTIAL = os.path.join(LIB_DIR, '.partial')      # left by tools/devbuild.sh: the library holds only one block size


def needs_build():
    if not os.path.exists(LIB) or os.path.exists(PARTIAL):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src, obj, verbose):
    cmd = [HIPCC] + [f for f in FLAGS if f != '-shared'] + ['-c', src, '-o', obj]
    if verbose:
        print(' '.join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc failed on %s:\n%s%s' % (src, r.stdout, r.stderr))


def build_library(force=False, verbose=False):
    """hipcc --offload-arch=gfx950: one object per source (kept under lib/obj, recompiled when the source or a header is newer),
    linked into catint_amd/lib/libcatint_pnp.so"""
    if not force and not needs_build():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    obj_dir = os.path.join(LIB_DIR, 'obj')
    os.makedirs(obj_dir, exist_ok=True)
    newest_header = max(os.path.getmtime(h) for h in HEADERS)
    jobs, objs = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(obj_dir, s.replace('.hip', '.o'))
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), newest_header):
            jobs.append((src, obj))
    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        for f in [ex.submit(_compile, src, obj, verbose) for src, obj in jobs]:
            f.result()
    cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC'] + objs + ['-o', LIB]
    if verbose:
        print(' '.join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc link failed:\n' + r.stdout + r.stderr)
    if os.path.exists(PARTIAL):
        os.remove(PARTIAL)
    return LIB


def _unit_needs_build(src_dir, sources, headers, lib):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(d) > t for d in [os.path.join(src_dir, s) for s in sources] + headers)


def _build_unit(src_dir, sources, headers, lib, force, verbose):
    """One hipcc --offload-arch=gfx950 command from the sources under src_dir to lib (the library is one translation unit)"""
    if not force and not _unit_needs_build(src_dir, sources, headers, lib):
        return lib
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [HIPCC] + FLAGS + [os.path.join(src_dir, s) for s in sources] + ['-o', lib]
    if verbose:
        print(' '.join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc failed on %s:\n%s%s' % (os.path.basename(lib), r.stdout, r.stderr))
    return lib


def observe_needs_build():
    return _unit_needs_build(OBSERVE_DIR, OBSERVE_SOURCES, OBSERVE_HEADERS, OBSERVE_LIB)


def build_observe_library(force=False, verbose=False):
    """catint_amd/csrc/observe into catint_amd/lib/libcatint_observe.so"""
    return _build_unit(OBSERVE_DIR, OBSERVE_SOURCES, OBSERVE_HEADERS, OBSERVE_LIB, force, verbose)


def balance_needs_build():
    return _unit_needs_build(BALANCE_DIR, BALANCE_SOURCES, BALANCE_HEADERS, BALANCE_LIB)


def build_balance_library(force=False, verbose=False):
    """catint_amd/csrc/balance into catint_amd/lib/libcatint_balance.so"""
    return _build_unit(BALANCE_DIR, BALANCE_SOURCES, BALANCE_HEADERS, BALANCE_LIB, force, verbose)


def regrid_needs_build():
    return _unit_needs_build(REGRID_DIR, REGRID_SOURCES, REGRID_HEADERS, REGRID_LIB)


def build_regrid_library(force=False, verbose=False):
    """catint_amd/csrc/regrid into catint_amd/lib/libcatint_regrid.so"""
    return _build_unit(REGRID_DIR, REGRID_SOURCES, REGRID_HEADERS, REGRID_LIB, force, verbose)


def equil_needs_build():
    return _unit_needs_build(EQUIL_DIR, EQUIL_SOURCES, EQUIL_HEADERS, EQUIL_LIB)


def build_equil_library(force=False, verbose=False):
    """catint_amd/csrc/equil into catint_amd/lib/libcatint_equil.so"""
    return _build_unit(EQUIL_DIR, EQUIL_SOURCES, EQUIL_HEADERS, EQUIL_LIB, force, verbose)


def response_needs_build():
    return _unit_needs_build(RESPONSE_DIR, RESPONSE_SOURCES, RESPONSE_HEADERS, RESPONSE_LIB)


def build_response_library(force=False, verbose=False):
    """catint_amd/csrc/response into catint_amd/lib/libcatint_response.so"""
    return _build_unit(RESPONSE_DIR, RESPONSE_SOURCES, RESPONSE_HEADERS, RESPONSE_LIB, force, verbose)


def kinetics_needs_build():
    return _unit_needs_build(KINETICS_DIR, KINETICS_SOURCES, KINETICS_HEADERS, KINETICS_LIB)


def build_kinetics_library(force=False, verbose=False):
    """catint_amd/csrc/kinetics into catint_amd/lib/libcatint_kinetics.so"""
    return _build_unit(KINETICS_DIR, KINETICS_SOURCES, KINETICS_HEADERS, KINETICS_LIB, force, verbose)


def couple_needs_build():
    return _unit_needs_build(COUPLE_DIR, COUPLE_SOURCES, COUPLE_HEADERS, COUPLE_LIB)


def build_couple_library(force=False, verbose=False):
    """catint_amd/csrc/couple into catint_amd/lib/libcatint_couple.so"""
    return _build_unit(COUPLE_DIR, COUPLE_SOURCES, COUPLE_HEADERS, COUPLE_LIB, force, verbose)


def sens_needs_build():
    return _unit_needs_build(SENS_DIR, SENS_SOURCES, SENS_HEADERS, SENS_LIB)


def build_sens_library(force=False, verbose=False):
    """catint_amd/csrc/sens into catint_amd/lib/libcatint_sens.so"""
    return _build_unit(SENS_DIR, SENS_SOURCES, SENS_HEADERS, SENS_LIB, force, verbose)


def drc_needs_build():
    return _unit_needs_build(DRC_DIR, DRC_SOURCES, DRC_HEADERS, DRC_LIB)


def build_drc_library(force=False, verbose=False):
    """catint_amd/csrc/drc into catint_amd/lib/libcatint_drc.so"""
    return _build_unit(DRC_DIR, DRC_SOURCES, DRC_HEADERS, DRC_LIB, force, verbose)


def modes_needs_build():
    return _unit_needs_build(MODES_DIR, MODES_SOURCES, MODES_HEADERS, MODES_LIB)


def build_modes_library(force=False, verbose=False):
    """catint_amd/csrc/modes into catint_amd/lib/libcatint_modes.so"""
    return _build_unit(MODES_DIR, MODES_SOURCES, MODES_HEADERS, MODES_LIB, force, verbose)


def scfkin_needs_build():
    return _unit_needs_build(SCFKIN_DIR, SCFKIN_SOURCES, SCFKIN_HEADERS, SCFKIN_LIB)


def build_scfkin_library(force=False, verbose=False):
    """catint_amd/csrc/scfkin into catint_amd/lib/libcatint_scfkin.so"""
    return _build_unit(SCFKIN_DIR, SCFKIN_SOURCES, SCFKIN_HEADERS, SCFKIN_LIB, force, verbose)


def kintrans_needs_build():
    return _unit_needs_build(KINTRANS_DIR, KINTRANS_SOURCES, KINTRANS_HEADERS, KINTRANS_LIB)


def build_kintrans_library(force=False, verbose=False):
    """catint_amd/csrc/kintrans into catint_amd/lib/libcatint_kintrans.so"""
    return _build_unit(KINTRANS_DIR, KINTRANS_SOURCES, KINTRANS_HEADERS, KINTRANS_LIB, force, verbose)


def eis_needs_build():
    return _unit_needs_build(EIS_DIR, EIS_SOURCES, EIS_HEADERS, EIS_LIB)


def build_eis_library(force=False, verbose=False):
    """catint_amd/csrc/eis into catint_amd/lib/libcatint_eis.so"""
    return _build_unit(EIS_DIR, EIS_SOURCES, EIS_HEADERS, EIS_LIB, force, verbose)


def interact_needs_build():
    return _unit_needs_build(INTERACT_DIR, INTERACT_SOURCES, INTERACT_HEADERS, INTERACT_LIB)


def build_interact_library(force=False, verbose=False):
    """catint_amd/csrc/interact into catint_amd/lib/libcatint_interact.so"""
    return _build_unit(INTERACT_DIR, INTERACT_SOURCES, INTERACT_HEADERS, INTERACT_LIB, force, verbose)


def voltam_needs_build():
    return _unit_needs_build(VOLTAM_DIR, VOLTAM_SOURCES, VOLTAM_HEADERS, VOLTAM_LIB)


def build_voltam_library(force=False, verbose=False):
    """catint_amd/csrc/voltam into catint_amd/lib/libcatint_voltam.so"""
    return _build_unit(VOLTAM_DIR, VOLTAM_SOURCES, VOLTAM_HEADERS, VOLTAM_LIB, force, verbose)


def iasweep_needs_build():
    return _unit_needs_build(IASWEEP_DIR, IASWEEP_SOURCES, IASWEEP_HEADERS, IASWEEP_LIB)


def build_iasweep_library(force=False, verbose=False):
    """catint_amd/csrc/iasweep into catint_amd/lib/libcatint_iasweep.so"""
    return _build_unit(IASWEEP_DIR, IASWEEP_SOURCES, IASWEEP_HEADERS, IASWEEP_LIB, force, verbose)


def iacontrol_needs_build():
    return _unit_needs_build(IACONTROL_DIR, IACONTROL_SOURCES, IACONTROL_HEADERS, IACONTROL_LIB)


def build_iacontrol_library(force=False, verbose=False):
    """catint_amd/csrc/iacontrol into catint_amd/lib/libcatint_iacontrol.so"""
    return _build_unit(IACONTROL_DIR, IACONTROL_SOURCES, IACONTROL_HEADERS, IACONTROL_LIB, force, verbose)


def unittest_needs_build():
    return _unit_needs_build(UNITTEST_DIR, UNITTEST_SOURCES, UNITTEST_HEADERS, UNITTEST_LIB)


def build_unittest_library(force=False, verbose=False):
    """tests/csrc into catint_amd/lib/libcatint_unittest.so"""
    return _build_unit(UNITTEST_DIR, UNITTEST_SOURCES, UNITTEST_HEADERS, UNITTEST_LIB, force, verbose)
