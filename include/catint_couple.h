/*
 * catint_couple.h -- C-ABI of libcatint_couple: ONE NEWTON STEP OF THE SELF-CONSISTENCY between electrode kinetics and electrolyte
 * transport, for a batch of operating points, formed ON THE DEVICE from the stationary state a pnp_handle holds there
 * (pnp_get_device_view, catint_pnp.h).  The transport half is the tangent of the stationary solution with respect to the prescribed
 * wall fluxes (what catint_response.h calls CATRESP_WALL_FLUX, all N columns from one elimination); the kinetic half is what
 * catkin_solve (catint_kinetics.h) returns: the flux and its derivatives with respect to the surface state.  The library shares no
 * code with the Newton kernels or with libcatint_response: the Jacobian is restated here from the definitions of catint_response.h.
 *
 * Conventions (those of catint_response.h): plain C; every pointer is a HOST pointer to C-contiguous fp64 / int32 / int64 owned by the
 * caller (the device pointers live in the pnp_device_view); every entry point returns 0 or a negative CATCPL_E* code and
 * catcpl_last_error gives the message; a context is not thread-safe, distinct contexts are independent.  The library reads the view,
 * nothing else.
 *
 * Definitions.  Per selected operating point, u = (c, phi) is the stationary state of the physical mode, solved with PRESCRIBED wall
 * fluxes g[N] only: g is what pnp_set_flux / pnp_solve_surface was given.  The solve had NO wall table (pnp_set_wall_kinetics): the
 * library cannot see a table and linearises without one.
 *   J          = (L, M, U), the block-tridiagonal Jacobian of the stationary residual, exactly as catint_response.h defines it with
 *                n_wall = 0: Scharfetter-Gummel fluxes, convection, steric coupling, mass-action reactions, Stern or Dirichlet wall,
 *                identity rows at the bulk point
 *   W          the wall Schur block D'_0 of the block elimination from the bulk: D'_{nx-1} = M_{nx-1},
 *                D'_{i-1} = M_{i-1} - U_{i-1} D'_i^-1 L_i
 *   T          = W^-1 E, (N+1) x N, the transport tangent.  E[k][k] = dx / D_k and zero elsewhere (the Poisson row is zero).
 *                Rows: T_c[k][j] = d c_k(0) / d g_j;  T_phi[j] = d phi(0) / d g_j.  All N columns come from ONE elimination
 *   K, Kc, Kphi  the kinetic inputs per point, all from catkin_solve: the flux [N], dflux_dc [N][N], and the column d/d phi_0 of
 *                dflux_dphi [N].  rf is the roughness factor: the transport sees rf K
 *   G          = g - rf K, the residual of the self-consistency
 *   A          = I - rf (Kc T_c + Kphi (x) T_phi), the Newton matrix, N x N
 *   dflux      = -A^-1 G, the Newton step of the wall fluxes
 *   dc_surface = T_c dflux, dphi_surface = T_phi dflux: the predicted change of the surface state
 *   lambda     in (0, 1], the damping: the largest value for which
 *                no surface concentration with c_k(0) > 0 and dc_surface_k < 0 falls below a tenth of its value
 *                  (lambda <= 0.9 c_k(0) / (-dc_surface_k)), and
 *                lambda |dphi_surface| <= dphi_max (dphi_max <= 0 switches this condition off)
 *   flux_new   = g + lambda dflux
 *   status     0 ok
 *              1 a non-finite number or a failed pivot check in the block elimination or in W: no row exchanges inside a block, and
 *                the check is that of catint_response.h (a pivot that is zero or not finite, or an entry below it more than
 *                CATCPL_PIVOT_GROWTH_LIMIT = CATRESP_PIVOT_GROWTH_LIMIT = 1e8 times its magnitude).  The numbers are returned as
 *                computed and must not be used
 *              2 the lane's solver status is non-zero, or an input of the point (g, K, Kc, Kphi) is not finite: every output of the
 *                point is NaN
 *              3 A is singular.  A is eliminated with partial row pivoting; a pivot that is zero, is not finite, or is below
 *                CATCPL_SINGULAR = 1e-12 times the largest magnitude in A gives 3: a turning point of the coupled problem.  The
 *                magnitude is taken over the entries of A AND the two terms each is the difference of (I and rf (Kc T_c + Kphi (x)
 *                T_phi)): where these cancel throughout, the entries of A are rounding noise and their own size measures nothing.
 *                The numbers are returned as computed and must not be used
 *              (2 goes before 1, 1 before 3.)
 *
 * The step is defined for a STATIONARY state that was solved with the fluxes g; the library cannot tell.
 */
#ifndef CATINT_COUPLE_H
#define CATINT_COUPLE_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATCPL_OK 0
#define CATCPL_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATCPL_ENOMEM (-2)
#define CATCPL_EDEVICE (-3)  /* HIP runtime error */

#define CATCPL_MAX_SPECIES 8 /* = CATRESP_MAX_SPECIES */
#define CATCPL_MAX_NX 4098
#define CATCPL_PIVOT_GROWTH_LIMIT 1e8 /* = CATRESP_PIVOT_GROWTH_LIMIT */
#define CATCPL_SINGULAR 1e-12         /* status 3 when a pivot of A falls below this many times the largest magnitude in A */

#define CATCPL_WALL_DIRICHLET 0
#define CATCPL_WALL_STERN 1

typedef struct catcpl_ctx catcpl_ctx;

typedef struct catcpl_params {
  int32_t struct_size;       /* = sizeof(catcpl_params) */
  int32_t max_waves;         /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t wall_bc;           /* CATCPL_WALL_* */
  int32_t nreactions;        /* <= PNP_MAX_REACTIONS; the table of pnp_set_reactions: */
  int64_t nlanes;            /* n: operating points to answer for; 0 is valid and makes no device call */
  const int64_t* lanes;      /* [n] indices into the handle's batch, repeats allowed; NULL: lanes 0 .. n-1 */
  const double* D;           /* [N] m^2/s */
  const double* charges;     /* [N] z F */
  const double* mpb_radius;  /* [N] m, NULL or all zero: point ions */
  const double* x;           /* [nx] strictly increasing */
  double beta;               /* 1/(R T) */
  double eps;                /* permittivity, F/m */
  double dx;                 /* the solver's reference length of the row scaling */
  double velocity;           /* convection velocity of pnp_set_convection */
  double stern_capacitance;  /* F/m^2, CATCPL_WALL_STERN */
  const int32_t* n_lhs;      /* [nreactions], each <= PNP_MAX_REACTANTS */
  const int32_t* lhs;        /* [nreactions][PNP_MAX_REACTANTS] species indices */
  const int32_t* n_rhs;      /* [nreactions] */
  const int32_t* rhs;        /* [nreactions][PNP_MAX_REACTANTS] */
  const double* kf;          /* [nreactions] */
  const double* kr;          /* [nreactions] */
  double rf;                 /* roughness factor, positive and finite */
  double dphi_max;           /* V, finite; <= 0: no limit on the step of the surface potential */
  /* per selected point, indexed by the position in the call (as the outputs are): */
  const double* flux;        /* [n][N] g, the prescribed wall fluxes the state was solved with, mol m^-2 s^-1 */
  const double* K;           /* [n][N] the kinetic flux (catkin_outputs.flux) */
  const double* Kc;          /* [n][N][N] catkin_outputs.dflux_dc */
  const double* Kphi;        /* [n][N] the column d/d phi_0 of catkin_outputs.dflux_dphi */
} catcpl_params;

/* n = nlanes.  Any pointer may be NULL: that row is not copied.  Rows not asked for are not touched. */
typedef struct catcpl_outputs {
  int32_t struct_size;       /* = sizeof(catcpl_outputs) */
  int32_t reserved;          /* 0 */
  double* T_c;               /* [n][N][N] */
  double* T_phi;             /* [n][N] */
  double* dflux;             /* [n][N] */
  double* lambda;            /* [n] */
  double* flux_new;          /* [n][N] */
  double* dc_surface;        /* [n][N] */
  double* dphi_surface;      /* [n] */
  int32_t* status;           /* [n] */
} catcpl_outputs;

/* No device call is made before the first catcpl_solve that passes validation with nlanes > 0. */
int catcpl_create(int32_t device, catcpl_ctx** out);
void catcpl_destroy(catcpl_ctx* ctx);
const char* catcpl_last_error(const catcpl_ctx* ctx); /* ctx may be NULL: last catcpl_create error */
/* Census-form name of the kernel instance the last successful call launched, e.g. "catcpl::couple_kernel<9>" (block size N + 1);
 * "" before the first one. */
const char* catcpl_last_kernel(const catcpl_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catcpl_last_kernel_ms(const catcpl_ctx* ctx);

/* One Newton step per selected operating point about the state behind `view` (valid until the next pnp_set_batch / pnp_destroy of its
 * handle).  The kernel and the copies run on view->stream, behind whatever the handle enqueued there, and the call returns when the
 * outputs are on the host.  The state, the status flags and the counters of the handle are only read.  Nothing is kept between block
 * rows: there is no workspace.  The results do not depend on max_waves, on the selection of lanes or on which outputs are asked for.
 * CATCPL_EINVAL, before any device call: NULL argument, wrong struct_size (view, params or outputs), a view without a potential row
 * (compat handle) or without a status row, nx < 3 or > CATCPL_MAX_NX, more than CATCPL_MAX_SPECIES species, x not strictly
 * increasing, a D that is not positive and finite, a charge or velocity that is not finite, beta, eps or dx not positive and finite, a
 * negative or non-finite radius, nreactions outside its limits, n_lhs / n_rhs above PNP_MAX_REACTANTS, a species index of the reaction
 * table outside [0, N), an unknown wall_bc, a Stern wall without a positive finite capacitance, rf not positive and finite, dphi_max
 * not finite, flux, K, Kc or Kphi NULL (with nlanes > 0), negative max_waves or nlanes, a lane index outside the batch (or nlanes
 * above it when lanes is NULL). */
int catcpl_solve(catcpl_ctx* ctx, const pnp_device_view* view, const catcpl_params* params, const catcpl_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_COUPLE_H */
