/*
 * catint_drc.h -- C-ABI of libcatint_drc: the DEGREE OF RATE CONTROL of the steady state of a mean-field surface microkinetic model,
 * computed ON THE DEVICE for a batch of operating points.  Which transition state and which intermediate control a wall flux: the
 * exact derivatives of the fluxes with respect to ln kf_r and ln kb_r of every step (the per-point offsets off[n][R][2] of
 * catint_kinetics.h), with respect to the height of every transition state at fixed reaction free energy (Campbell's degree of rate
 * control) and with respect to the free energy of every adsorbate at fixed transition states (the thermodynamic degree of rate
 * control).  CatMAP's rate_control takes these by finite differences, one re-solve per energy; here they follow from the implicit
 * function theorem on the factorised Jacobian of the steady state: one factorisation and up to 3 R + S right-hand sides per point.
 *
 * Conventions (those of catint_kinetics.h): plain C; every pointer of the parameters and outputs is a HOST pointer to C-contiguous
 * fp64 / int32 / int64 owned by the caller; every entry point returns 0 or a negative CATDRC_E* code and catdrc_last_error gives the
 * message; a context is not thread-safe, distinct contexts are independent.  The view is read, never written.
 *
 * Definition.  Everything up to the scaled system is catint_kinetics.h word for word, with the same tables and limits (N <= 8,
 * 1 <= S <= 8, R <= 16, orders 0 .. 3).  Per operating point b = 0 .. n-1, in units of kT:
 *   potential  V_b = phiM[b] - w phi_0[b], w in {0, 1} (w = 1: the Stern-layer drop); phi_0 = phi(x = 0)
 *   charge     sigma_b = C_S (phiM[b] - phi_PZC - phi_0[b]), or the per-point array sigma[n]
 *   constants  dG_r = a0 + a1 V + a2 sigma + a3 sigma^2      Ea_r = e0 + e1 V + e2 sigma + e3 sigma^2 (e0 = -INFINITY: no transition state)
 *              Ga_r = max(Ea_r, dG_r, 0)                     (ties: the first of the three; the branch taken is the branch differentiated)
 *              ln kf_r = lnA_r - Ga_r + off[b][r][0]         ln kb_r = lnA_r - (Ga_r - dG_r) + off[b][r][1]      (off NULL: zeros)
 *   activities a_j = gamma[b][j] max(c_j(0), 0) / cref_j; gamma optional [n][N], NULL: 1
 *   rates      rf_r = kf_r prod_j a_j^order_f[r][j] exp(sum_t order_f[r][N+t] y_t)      (rb_r likewise with kb_r and order_b)
 *              m[r][t] = order_b[r][N+t] - order_f[r][N+t]
 *   rows       F_0 = sum_t n_t exp(y_t) - 1
 *              F_s = (sum_r m[r][s] (rf_r - rb_r)) / D_s,   D_s = sum_r |m[r][s]| (rf_r + rb_r),   s = 1 .. S
 *              J[s][t] = sum_r m[r][s] (rf_r order_f[r][N+t] - rb_r order_b[r][N+t]) / D_s,   J[0][t] = n_t exp(y_t)
 *              A row with D_s = 0 (nothing produces or consumes the adsorbate) is the dead row: y_s = CATDRC_MIN_LOG, J[s][.] = e_s,
 *              F_s = 0 and every right-hand side is 0 there.
 * The state is an INPUT: theta[n][S+1] is required and is what catkin_solve returned.  The unknowns are y_t = ln theta_t, clamped by
 * the rule of catkin's theta_guess: y = 0 for theta >= 1, ln theta for 0 < theta < 1, CATDRC_MIN_LOG otherwise and below it.  The
 * library does not iterate; it reports residual[n] = max_s |F_s| (s = 0 .. S) at that state.
 *
 * With W[r][t] = rf_r order_f[r][N+t] - rb_r order_b[r][N+t], a parameter p with d ln kf_r / dp = alpha_r, d ln kb_r / dp = beta_r has
 *   dnet_r = rf_r alpha_r - rb_r beta_r
 *   rhs_0 = 0,  rhs_s = -(sum_r m[r][s] dnet_r) / D_s        (0 on a dead row)
 *   J dy = rhs                                                (J factorised once per point, Gaussian elimination, partial row pivoting)
 *   one step of refinement: rho_0 = -sum_t n_t theta_t dy_t,  rho_s = -(sum_r m[r][s] (dnet_r + sum_t W[r][t] dy_t)) / D_s  (-dy_s on
 *   a dead row), J delta = rho with the same factors, dy += delta.  rho is the row's total derivative formed from the rates, not from
 *   the entries of J, which are sums that cancel: without the step a stiff network loses three digits of the sum of terms.
 *   dflux_k/dp = site_density sum_r nu[r][k] (dnet_r + sum_t W[r][t] dy_t)
 * Column families, each nullable (an output the caller did not ask for is not touched):
 *   dflux_dlnkf[n][R][N]   alpha = e_r, beta = 0: the derivative with respect to off[b][r][0]
 *   dflux_dlnkb[n][R][N]   alpha = 0, beta = e_r: the derivative with respect to off[b][r][1]
 *   dflux_drc[n][R][N], dy_drc[n][R][S+1]
 *                          alpha = beta = e_r: the transition state of step r lowered by one kT at fixed reaction free energy;
 *                          dnet_r = rf_r - rb_r is formed as that difference.  drc[n][R][N] = dflux_drc / flux is Campbell's degree
 *                          of rate control X_rc.
 *   dflux_dG[n][S][N]      p = -G_s / kT of adsorbate s = 1 .. S with the transition states fixed (row s - 1): ddG_r = -m[r][s],
 *                          dEa_r = +order_f[r][N+s]; dGa_r follows the branch of Ga_r (Ea: dEa, dG: ddG, zero: 0);
 *                          alpha_r = -dGa_r, beta_r = -(dGa_r - ddG_r).  tdrc[n][S][N] = dflux_dG / flux is the thermodynamic
 *                          degree of rate control.
 *   flux[n][N], flux_scale[n][N]   as in catint_kinetics.h, at this y
 *   residual[n]
 *   status[n]   CATDRC_OK_POINT 0; CATDRC_RESIDUAL 1: residual > residual_tol, the numbers are returned as computed;
 *               CATDRC_INPUT 2: the lane's solver status is non-zero (view path) or an input of the point (theta included) is not
 *               finite: every output of the point is NaN, other points are unaffected; CATDRC_PIVOT 3: a zero or non-finite pivot.
 * A normalised entry (drc, tdrc) is exactly 0 when column k of nu is all zero (the species takes no part in the mechanism).  Otherwise
 * it is the IEEE quotient of the two outputs beside it, dflux / flux, as the kernel formed them: its number of digits is what
 * flux / flux_scale leaves of 16 (a net flux that is the difference of gross rates 1e10 times larger leaves six), and a flux of exactly
 * zero gives inf or NaN.  The sum rule sum_r dflux_drc[r][k] = flux_k holds to rounding at a state whose residual is at rounding.
 * Surface state: host arrays csurf[n][N] and phi_surface[n] (view may then be NULL); or both NULL, and the kernel reads
 * c_dev[(lane N + k) row_pitch] and phi_dev[lane row_pitch] of lanes[n] from the view (repeats allowed, lanes NULL: 0 .. n-1), ordered
 * on view->stream.  Both paths give the same bits for the same numbers.  Every per-point array ([n]...) is indexed by the position in
 * the call, not by the handle's lane; a point's numbers do not depend on where in the batch it stands.
 */
#ifndef CATINT_DRC_H
#define CATINT_DRC_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATDRC_OK 0
#define CATDRC_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATDRC_ENOMEM (-2)
#define CATDRC_EDEVICE (-3)  /* HIP runtime error */

#define CATDRC_MAX_SPECIES 8     /* = CATKIN_MAX_SPECIES */
#define CATDRC_MAX_ADSORBATES 8
#define CATDRC_MAX_STEPS 16
#define CATDRC_MAX_ORDER 3
#define CATDRC_MAX_SITES 3
#define CATDRC_MIN_LOG (-700.0)

#define CATDRC_DROP_FULL 0       /* V = phiM */
#define CATDRC_DROP_STERN 1      /* V = phiM - phi(x = 0) */

#define CATDRC_OK_POINT 0
#define CATDRC_RESIDUAL 1
#define CATDRC_INPUT 2
#define CATDRC_PIVOT 3

typedef struct catdrc_ctx catdrc_ctx;

typedef struct catdrc_params {
  int32_t struct_size;        /* = sizeof(catdrc_params) */
  int32_t max_waves;          /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t nspecies;           /* N, 0 .. CATDRC_MAX_SPECIES; the view's on the view path */
  int32_t nadsorbates;        /* S, 1 .. CATDRC_MAX_ADSORBATES */
  int32_t nsteps;             /* R, 1 .. CATDRC_MAX_STEPS */
  int32_t potential_drop;     /* w: CATDRC_DROP_* */
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
  double residual_tol;        /* on max_s |F_s|; positive and finite */
  double stern_capacitance;   /* C_S, F/m^2; used when sigma is NULL */
  double phi_pzc;             /* V */
  const double* phiM;         /* [n] */
  const double* sigma;        /* [n] C/m^2, or NULL: from C_S */
  const double* off;          /* [n][R][2], or NULL */
  const double* gamma;        /* [n][N], or NULL */
  const double* theta;        /* [n][S+1]: the coverages of the steady state (catkin_solve's theta); required */
  const double* csurf;        /* [n][N], or NULL: the view */
  const double* phi_surface;  /* [n], or NULL: the view */
} catdrc_params;

typedef struct catdrc_outputs {
  int32_t struct_size;        /* = sizeof(catdrc_outputs) */
  int32_t reserved;
  double* dflux_dlnkf;        /* [n][R][N] mol m^-2 s^-1 */
  double* dflux_dlnkb;        /* [n][R][N] */
  double* dflux_drc;          /* [n][R][N] */
  double* dy_drc;             /* [n][R][S+1] */
  double* drc;                /* [n][R][N] = dflux_drc / flux */
  double* dflux_dG;           /* [n][S][N] */
  double* tdrc;               /* [n][S][N] = dflux_dG / flux */
  double* flux;               /* [n][N] */
  double* flux_scale;         /* [n][N] */
  double* residual;           /* [n] */
  int32_t* status;            /* [n] CATDRC_OK_POINT .. CATDRC_PIVOT */
} catdrc_outputs;

/* No device call is made before the first catdrc_solve that passes validation with n > 0. */
int catdrc_create(int32_t device, catdrc_ctx** out);
void catdrc_destroy(catdrc_ctx* ctx);
const char* catdrc_last_error(const catdrc_ctx* ctx); /* ctx may be NULL: last catdrc_create error */
/* Census-form name of the kernel the last successful call launched ("catdrc::control_kernel"); "" before the first one. */
const char* catdrc_last_kernel(const catdrc_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catdrc_last_kernel_ms(const catdrc_ctx* ctx);

/* The rate-control analysis of every operating point in one launch.  view may be NULL when csurf and phi_surface are given (the
 * kernel then runs on the default stream); otherwise the kernel and the copies run on view->stream, behind whatever the handle
 * enqueued there.  The call returns when the outputs are on the host.  The state, the status flags and the counters of the handle are
 * only read.
 * CATDRC_EINVAL, before any device call: NULL ctx, params or outputs, or a wrong struct_size (params, outputs, view); N > 8, S < 1 or
 * S > 8, R < 1 or R > 16; a missing table; an order outside 0 .. 3, a step that does not conserve sites, a step with all orders zero
 * on a side together with nu all zero (an empty step); cref, site_density, residual_tol or a site count that is not positive and
 * finite (a site count is 1, 2 or 3, that of the free site 1); potential_drop outside {0, 1}, negative max_waves or n; a non-finite
 * table entry other than e0 = -INFINITY; phiM or theta NULL; only one of csurf and phi_surface; on the view path a NULL view, a view
 * without a potential row (compat handle), a lane index out of range (or n above the batch when lanes is NULL), N different from the
 * view's; neither sigma nor a finite stern_capacitance and phi_pzc. */
int catdrc_solve(catdrc_ctx* ctx, const pnp_device_view* view, const catdrc_params* params, const catdrc_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_DRC_H */
