/*
 * catint_kinetics.h -- C-ABI of libcatint_kinetics: the STEADY STATE of a mean-field surface microkinetic model (adsorbed
 * intermediates competing for the sites of one site type) solved ON THE DEVICE for a batch of operating points, and the wall fluxes
 * and their sensitivities that follow from it.  It is the kinetic half of the reference's self-consistency loop (where CatMAP sat):
 * the surface state (concentrations and potential at x = 0) goes in, wall fluxes come out.  The surface state is taken either from
 * host arrays (what the SCF loop holds: the mixed concentrations) or from the state a pnp_handle holds on the device
 * (pnp_get_device_view, catint_pnp.h).
 *
 * Conventions (those of catint_equil.h): plain C; every pointer of the parameters and outputs is a HOST pointer to C-contiguous fp64 /
 * int32 / int64 owned by the caller; every entry point returns 0 or a negative CATKIN_E* code and catkin_last_error gives the message;
 * a context is not thread-safe, distinct contexts are independent.  The view is read, never written.
 *
 * Definition.  Per operating point b = 0 .. n-1: solution species j = 0 .. N-1 (the handle's species), coverages theta_t, t = 0 .. S,
 * where t = 0 is the free site and 1 <= S <= 8 adsorbates; site counts n_t, n_0 = 1, n_t in {1, 2, 3}; R <= 16 elementary steps;
 * unknowns y_t = ln theta_t.  Everything is in units of kT, so the tables are dimensionless apart from V^-1, m^2/C and m^4/C^2.
 *   tables     order_f[R][N+S+1], order_b[R][N+S+1]: int32 in 0 .. 3; column j < N is a solution species, column N + t a coverage.
 *              Every step conserves sites: sum_t n_t (order_b - order_f)[r][N+t] = 0.
 *              nu[R][N]: moles of species k released into the electrolyte per forward turnover (educts negative, as in
 *              pnp_set_wall_kinetics); cref[N] > 0; site_density in mol/m^2.
 *   potential  V_b = phiM[b] - w phi_0[b], w in {0, 1} (w = 1: the Stern-layer drop); phi_0 = phi(x = 0)
 *   charge     sigma_b = C_S (phiM[b] - phi_PZC - phi_0[b]), or the per-point array sigma[n] (then a constant for the derivatives)
 *   constants  dG_r = a0 + a1 V + a2 sigma + a3 sigma^2      (reaction free energy of step r; dG[r] = a0 .. a3)
 *              Ea_r = e0 + e1 V + e2 sigma + e3 sigma^2      (TS - IS; e0 = -INFINITY: no transition state)
 *              Ga_r = max(Ea_r, dG_r, 0)                     (ties: the first of the three, for the derivatives)
 *              ln kf_r = lnA_r - Ga_r + off[b][r][0]         ln kb_r = lnA_r - (Ga_r - dG_r) + off[b][r][1]
 *              off: optional [n][R][2], NULL: zeros; constant for the derivatives.  kf / kb = exp(-dG) holds by construction when off
 *              is zero.
 *   activities a_j = gamma[b][j] max(c_j(0), 0) / cref_j; gamma optional [n][N], NULL: 1.  A negative surface concentration counts
 *              as zero.
 *   rates      rf_r = kf_r prod_j a_j^order_f[r][j] exp(sum_t order_f[r][N+t] y_t)      (rb_r likewise with kb_r and order_b)
 *              m[r][t] = order_b[r][N+t] - order_f[r][N+t]
 *   residual   F_0 = sum_t n_t exp(y_t) - 1
 *              F_s = (sum_r m[r][s] (rf_r - rb_r)) / D_s,   D_s = sum_r |m[r][s]| (rf_r + rb_r),   s = 1 .. S
 *              A row with D_s = 0 (nothing produces or consumes the adsorbate) is replaced by y_s = CATKIN_MIN_LOG: the unknown is set
 *              to that value and its row keeps it there.
 *   iteration  start from y_t = ln(1 / sum_t n_t), or from theta_guess[n][S+1] clamped into [exp(CATKIN_MIN_LOG), 1].  Newton with the
 *              analytic Jacobian of the scaled rows, D_s held fixed within an iteration:
 *                dF_s/dy_t = sum_r m[r][s] (rf_r order_f[r][N+t] - rb_r order_b[r][N+t]) / D_s,   dF_0/dy_t = n_t exp(y_t),
 *              solved by Gaussian elimination with partial row pivoting (with the site row first its diagonal is theta_*, which
 *              reaches 5e-8 where other entries are of order 1).  The update is scaled by min(1, 3 / max|dy|), y is clamped to
 *              >= CATKIN_MIN_LOG; the iteration stops when max|dy| < tol (the update is still applied) or after maxit iterations.
 * Outputs, each nullable (an entry the caller did not ask for is not touched):
 *   theta[n][S+1]; rate[n][R] = rf - rb; rate_gross[n][R] = rf + rb;
 *   flux[n][N] = site_density sum_r nu[r][k] rate_r;   flux_scale[n][N] = site_density sum_r |nu[r][k]| (rf_r + rb_r).
 *   The number of digits of flux is what flux / flux_scale leaves of 16: a net rate that is the difference of two gross rates 1e10
 *   times larger has six digits, and no arithmetic in fp64 can return more.
 *   dflux_dc[n][N][N] = d flux_k / d c_j(0);  dflux_dphi[n][N][2] = d/d phiM at fixed phi_0, d/d phi_0 at fixed phiM.
 *   Sensitivities: implicit function theorem at the converged y, J dy/dp = -dF/dp with the factorisation of that J, then
 *     dflux_k/dp = dflux_k/dp|_y + site_density sum_r nu[r][k] sum_t (rf_r order_f[r][N+t] - rb_r order_b[r][N+t]) dy_t/dp.
 *   d/dc_j is formed as the product with one factor left out, so it is finite at c_j = 0; it is zero where c_j < 0 was clamped.
 *   status[n]: 0 converged; 1 stopped at maxit, the numbers are returned as computed; 2 the handle's status of the lane is non-zero
 *   (view path) or an input of the point is not finite: every output of the point is NaN, other points are unaffected; 3 a zero or
 *   non-finite pivot.   iterations[n].
 * Surface state: host arrays csurf[n][N] and phi_surface[n] (view may then be NULL); or both NULL, and the kernel reads
 * c_dev[(lane N + k) row_pitch] and phi_dev[lane row_pitch] of lanes[n] from the view (repeats allowed, lanes NULL: 0 .. n-1), ordered
 * on view->stream.  Both paths give the same bits for the same numbers.  Every per-point array ([n]...) is indexed by the position in
 * the call, not by the handle's lane.
 */
#ifndef CATINT_KINETICS_H
#define CATINT_KINETICS_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATKIN_OK 0
#define CATKIN_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATKIN_ENOMEM (-2)
#define CATKIN_EDEVICE (-3)  /* HIP runtime error */

#define CATKIN_MAX_SPECIES 8     /* = PNP_NEWTON_MAX_SPECIES */
#define CATKIN_MAX_ADSORBATES 8
#define CATKIN_MAX_STEPS 16
#define CATKIN_MAX_ORDER 3
#define CATKIN_MAX_SITES 3
#define CATKIN_MIN_LOG (-700.0)

#define CATKIN_DROP_FULL 0       /* V = phiM */
#define CATKIN_DROP_STERN 1      /* V = phiM - phi(x = 0) */

#define CATKIN_CONVERGED 0
#define CATKIN_MAXIT 1
#define CATKIN_INPUT 2
#define CATKIN_PIVOT 3

typedef struct catkin_ctx catkin_ctx;

typedef struct catkin_params {
  int32_t struct_size;        /* = sizeof(catkin_params) */
  int32_t max_waves;          /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t nspecies;           /* N, 0 .. CATKIN_MAX_SPECIES; the view's on the view path */
  int32_t nadsorbates;        /* S, 1 .. CATKIN_MAX_ADSORBATES */
  int32_t nsteps;             /* R, 1 .. CATKIN_MAX_STEPS */
  int32_t maxit;              /* >= 1 */
  int32_t potential_drop;     /* w: CATKIN_DROP_* */
  int32_t reserved;
  int64_t n;                  /* operating points; 0 is valid and makes no device call */
  const int64_t* lanes;       /* view path: [n] indices into the handle's batch, repeats allowed; NULL: 0 .. n-1 */
  const int32_t* order_f;     /* [R][N+S+1] */
  const int32_t* order_b;     /* [R][N+S+1] */
  const double* nu;           /* [R][N] */
  const double* cref;         /* [N] mol/m^3 */
  const double* site_count;   /* [S+1], site_count[0] = 1 */
  const double* dG;           /* [R][4] a0 .. a3 */
  const double* Ea;           /* [R][4] e0 .. e3 */
  const double* lnA;          /* [R] */
  double site_density;        /* mol/m^2 */
  double tol;                 /* on max|dy| */
  double stern_capacitance;   /* C_S, F/m^2; used when sigma is NULL */
  double phi_pzc;             /* V */
  const double* phiM;         /* [n] */
  const double* sigma;        /* [n] C/m^2, or NULL: from C_S */
  const double* off;          /* [n][R][2], or NULL */
  const double* gamma;        /* [n][N], or NULL */
  const double* theta_guess;  /* [n][S+1], or NULL */
  const double* csurf;        /* [n][N], or NULL: the view */
  const double* phi_surface;  /* [n], or NULL: the view */
} catkin_params;

typedef struct catkin_outputs {
  int32_t struct_size;        /* = sizeof(catkin_outputs) */
  int32_t reserved;
  double* theta;              /* [n][S+1] */
  double* rate;               /* [n][R] 1/s per site */
  double* rate_gross;         /* [n][R] */
  double* flux;               /* [n][N] mol m^-2 s^-1 */
  double* flux_scale;         /* [n][N] */
  double* dflux_dc;           /* [n][N][N] */
  double* dflux_dphi;         /* [n][N][2] */
  int32_t* status;            /* [n] CATKIN_CONVERGED .. CATKIN_PIVOT */
  int32_t* iterations;        /* [n] */
} catkin_outputs;

/* No device call is made before the first catkin_solve that passes validation with n > 0. */
int catkin_create(int32_t device, catkin_ctx** out);
void catkin_destroy(catkin_ctx* ctx);
const char* catkin_last_error(const catkin_ctx* ctx); /* ctx may be NULL: last catkin_create error */
/* Census-form name of the kernel the last successful call launched ("catkin::steady_kernel"); "" before the first one. */
const char* catkin_last_kernel(const catkin_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catkin_last_kernel_ms(const catkin_ctx* ctx);

/* One steady-state solve per operating point.  view may be NULL when csurf and phi_surface are given (the kernel then runs on the
 * default stream); otherwise the kernel and the copies run on view->stream, behind whatever the handle enqueued there.  The call
 * returns when the outputs are on the host.  The state, the status flags and the counters of the handle are only read.
 * CATKIN_EINVAL, before any device call: NULL ctx, params or outputs, or a wrong struct_size (params, outputs, view); N > 8, S < 1 or
 * S > 8, R < 1 or R > 16; a missing table; an order outside 0 .. 3, a step that does not conserve sites, a step with all orders zero
 * on a side together with nu all zero (an empty step); cref, site_density, tol or a site count that is not positive and finite (a
 * site count is 1, 2 or 3, that of the free site 1); maxit < 1, potential_drop outside {0, 1}, negative max_waves or n; a non-finite
 * table entry other than e0 = -INFINITY; phiM NULL; only one of csurf and phi_surface; on the view path a NULL view, a view without a
 * potential row (compat handle), a lane index out of range (or n above the batch when lanes is NULL), N different from the view's;
 * neither sigma nor a finite stern_capacitance and phi_pzc. */
int catkin_solve(catkin_ctx* ctx, const pnp_device_view* view, const catkin_params* params, const catkin_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_KINETICS_H */
