/*
 * catint_iacontrol.h -- C-ABI of libcatint_iacontrol: the DEGREE OF RATE CONTROL of the steady state of a surface microkinetic model with
 * LATERAL INTERACTIONS and SEVERAL SITE TYPES (the model of catint_interact.h), computed ON THE DEVICE for a batch of operating points.
 * It is what catint_drc.h gives for the mean-field model: the exact derivatives of the wall fluxes with respect to ln kf_r and ln kb_r
 * of every step, to the height of every transition state (Campbell's degree of rate control) and to the free energy of every adsorbate
 * (the thermodynamic degree of rate control), by the implicit function theorem on the factorised Jacobian of the steady state -- here
 * the FULL Jacobian, with the coverage dependence of the energies in it -- and one column more: the derivative with respect to the
 * interaction strength itself.  CatMAP takes these by finite differences, one ramped re-solve per energy.
 *
 * Conventions, error codes, context functions, the two surface-state paths and the per-point status values are those of catint_drc.h;
 * the model (site types, columns, response, shifts, contractions EG and EA, rate constants, rows, dead-row rule) is that of
 * catint_interact.h at lambda = strength.  Only what differs from the two is stated here.
 *
 * The state is an INPUT: theta[n][T], T = G + S, is required and is what catia_solve returned at `strength`.  y_t = ln theta_t, clamped
 * by the rule of catdrc's theta.  The library does not iterate and has no ramp; it reports residual[n] = max |F| over all T rows (the
 * G site rows F_g = (sum_{t on g} n_t theta_t) / x_g - 1 and the scaled adsorbate rows F_s) at that state.
 *
 * Jacobian: that of catint_interact.h, the shifts included through the effective orders, the branch of Ga_r held as found at the state:
 *   ofe[r][t] = order_f[r][N+t] - theta_t dGa_r/dtheta_t
 *   obe[r][t] = order_b[r][N+t] - theta_t (dGa_r/dtheta_t - ddG_r/dtheta_t)        (a free-site column carries its integer orders)
 *   W[r][t] = rf_r ofe[r][t] - rb_r obe[r][t]
 *   J[s][t] = sum_r m[r][s] W[r][t] / D_s for an adsorbate row s = G .. T-1,   J[g][t] = n_t theta_t / x_g for t on g, else 0
 * A parameter p with d ln kf_r / dp = alpha_r and d ln kb_r / dp = beta_r AT FIXED COVERAGES has
 *   dnet_r = rf_r alpha_r - rb_r beta_r
 *   rhs_g = 0,  rhs_s = -(sum_r m[r][s] dnet_r) / D_s                  (0 on a dead row)
 *   J dy = rhs                                                          (J factorised once per point, partial row pivoting)
 *   one step of refinement with rho formed from the rates:  rho_g = -(sum_{t on g} n_t theta_t dy_t) / x_g,
 *   rho_s = -(sum_r m[r][s] (dnet_r + sum_t W[r][t] dy_t)) / D_s  (-dy_s on a dead row), J delta = rho, dy += delta
 *   dflux_k/dp = site_density sum_r nu[r][k] (dnet_r + sum_t W[r][t] dy_t)
 * With coverage-dependent energies the answer is not the mean-field one at other coverages: the shifts enter J, and they enter the
 * part of every flux derivative that goes through dy.
 * Column families, each nullable (an output the caller did not ask for is not touched):
 *   dflux_dlnkf, dflux_dlnkb [n][R][N]                    as in catint_drc.h
 *   dflux_drc [n][R][N], dy_drc [n][R][T], drc [n][R][N]  alpha = beta = e_r, dnet_r formed as rf_r - rb_r.  The sum rule
 *                          sum_r dflux_drc[r][k] = flux_k still holds: scaling every rate constant by one factor leaves the
 *                          coverages unchanged, and with them the shifts.
 *   dflux_dG [n][S][N], tdrc [n][S][N]   the formation energy of adsorbate a (column G + a) lowered by one kT at fixed transition
 *                          states: ddG_r = -m[r][G+a], dEa_r = +order_f[r][N+G+a], the branch of Ga_r decides (catint_drc.h).  The
 *                          interaction changes only J and W.
 *   dflux_dstrength [n][N], dy_dstrength [n][T], strength_control [n][N] = strength dflux_dstrength / flux
 *                          p = lambda, the interaction strength: at fixed theta ddG_r/dlambda = sum_u EG[r][u] w_u and
 *                          dEa_r/dlambda = sum_u EA[r][u] w_u (w_u = f_{site_of[u]} theta_u, u ascending; no transition state: 0),
 *                          dGa_r/dlambda follows the branch, alpha_r = -dGa_r/dlambda, beta_r = -(dGa_r/dlambda - ddG_r/dlambda).
 *                          strength_control is the share of each flux that is owed to the interactions, to first order.
 *   flux, flux_scale [n][N]; residual [n]; status [n] CATIC_OK_POINT 0, CATIC_RESIDUAL 1 (residual > residual_tol, numbers as
 *   computed), CATIC_INPUT 2 (unsolved lane or non-finite input, theta included: every output of the point NaN), CATIC_PIVOT 3.
 * A normalised entry (drc, tdrc, strength_control) is exactly 0 when column k of nu is all zero; otherwise it is the IEEE quotient of
 * the two outputs beside it (strength_control: strength times the quotient), with the digits flux / flux_scale leaves of 16.
 * A point's bits do not depend on its position in the batch, on max_waves, on the outputs asked for, or on the surface-state path.
 * With G = 1 and strength = 0 the outputs of the four families of catint_drc.h, flux, flux_scale, residual and status have the bits of
 * catdrc_solve on the same tables.
 */
#ifndef CATINT_IACONTROL_H
#define CATINT_IACONTROL_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATIC_OK 0
#define CATIC_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATIC_ENOMEM (-2)
#define CATIC_EDEVICE (-3)  /* HIP runtime error */

#define CATIC_MAX_SPECIES 8
#define CATIC_MAX_SITE_TYPES 3
#define CATIC_MAX_COLUMNS 9      /* T = G + S */
#define CATIC_MAX_STEPS 16
#define CATIC_MAX_ORDER 3
#define CATIC_MAX_SITES 3
#define CATIC_MIN_LOG (-700.0)

#define CATIC_DROP_FULL 0
#define CATIC_DROP_STERN 1

#define CATIC_LINEAR 0
#define CATIC_PIECEWISE 1

#define CATIC_OK_POINT 0
#define CATIC_RESIDUAL 1
#define CATIC_INPUT 2
#define CATIC_PIVOT 3

typedef struct catic_ctx catic_ctx;

typedef struct catic_params {
  int32_t struct_size;        /* = sizeof(catic_params) */
  int32_t max_waves;          /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t nspecies;           /* N, 0 .. CATIC_MAX_SPECIES; the view's on the view path */
  int32_t nadsorbates;        /* S >= 1 */
  int32_t nsteps;             /* R, 1 .. CATIC_MAX_STEPS */
  int32_t potential_drop;     /* CATIC_DROP_* */
  int32_t nsitetypes;         /* G, 1 .. CATIC_MAX_SITE_TYPES; G + S <= CATIC_MAX_COLUMNS */
  int32_t response;           /* CATIC_LINEAR or CATIC_PIECEWISE */
  int64_t n;                  /* operating points; 0 is valid and makes no device call */
  const int64_t* lanes;       /* view path: [n] indices into the handle's batch, repeats allowed; NULL: 0 .. n-1 */
  const int32_t* order_f;     /* [R][N+T] */
  const int32_t* order_b;     /* [R][N+T] */
  const double* nu;           /* [R][N] */
  const double* cref;         /* [N] mol/m^3 */
  const double* site_count;   /* [T], 1 for the free sites */
  const int32_t* site_of;     /* [T], site_of[t] = t for t < G */
  const double* site_fraction;/* [G] */
  const double* dG;           /* [R][4] */
  const double* Ea;           /* [R][4] */
  const double* lnA;          /* [R] */
  const double* eps;          /* [S][S] kT */
  const double* eps_ts;       /* [R][S] kT, or NULL: zeros */
  const double* cutoff;       /* [G], CATIC_PIECEWISE only */
  const double* smoothing;    /* [G] > 0, CATIC_PIECEWISE only */
  double site_density;        /* mol/m^2 of all sites */
  double residual_tol;        /* on max |F|; positive and finite */
  double stern_capacitance;
  double phi_pzc;
  double strength;            /* lambda the state was solved at */
  const double* phiM;         /* [n] */
  const double* sigma;        /* [n] C/m^2, or NULL: from C_S */
  const double* off;          /* [n][R][2], or NULL */
  const double* gamma;        /* [n][N], or NULL */
  const double* theta;        /* [n][T]: the coverages of the steady state (catia_solve's theta at `strength`); required */
  const double* csurf;        /* [n][N], or NULL: the view */
  const double* phi_surface;  /* [n], or NULL: the view */
} catic_params;

typedef struct catic_outputs {
  int32_t struct_size;        /* = sizeof(catic_outputs) */
  int32_t reserved;
  double* dflux_dlnkf;        /* [n][R][N] mol m^-2 s^-1 */
  double* dflux_dlnkb;        /* [n][R][N] */
  double* dflux_drc;          /* [n][R][N] */
  double* dy_drc;             /* [n][R][T] */
  double* drc;                /* [n][R][N] = dflux_drc / flux */
  double* dflux_dG;           /* [n][S][N] */
  double* tdrc;               /* [n][S][N] = dflux_dG / flux */
  double* dflux_dstrength;    /* [n][N] */
  double* dy_dstrength;       /* [n][T] */
  double* strength_control;   /* [n][N] = strength (dflux_dstrength / flux) */
  double* flux;               /* [n][N] */
  double* flux_scale;         /* [n][N] */
  double* residual;           /* [n] */
  int32_t* status;            /* [n] CATIC_OK_POINT .. CATIC_PIVOT */
} catic_outputs;

/* No device call is made before the first catic_solve that passes validation with n > 0. */
int catic_create(int32_t device, catic_ctx** out);
void catic_destroy(catic_ctx* ctx);
const char* catic_last_error(const catic_ctx* ctx); /* ctx may be NULL: last catic_create error */
/* Census-form name of the kernel the last successful call launched ("catic::control_kernel"); "" before the first one. */
const char* catic_last_kernel(const catic_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catic_last_kernel_ms(const catic_ctx* ctx);

/* The rate-control analysis of every operating point in one launch; view, stream and return as catdrc_solve.
 * CATIC_EINVAL, before any device call: for the tables everything catia_solve reports (G outside 1 .. 3; S < 1 or G + S > 9; a missing
 * table, site_of, site_fraction or eps; an order outside 0 .. 3; a step that breaks the site balance of one type; an empty step; a
 * site_of outside [0, G) or a free-site column that is not on its own type or whose site count is not 1; cref, site_density, a site
 * fraction or a site count that is not positive and finite; a non-finite table entry other than e0 = -INFINITY; a non-finite eps,
 * eps_ts or strength; a response outside the two; in the piecewise mode a missing or non-finite cutoff or a smoothing that is not
 * positive and finite), and for the state and the points everything catdrc_solve reports (NULL ctx, params or outputs, a wrong
 * struct_size; residual_tol not positive and finite; potential_drop outside {0, 1}, negative max_waves or n; phiM or theta NULL; only
 * one of csurf and phi_surface; on the view path a NULL view, a view without a potential row, a lane index out of range or n above the
 * batch when lanes is NULL, N different from the view's; neither sigma nor a finite stern_capacitance and phi_pzc). */
int catic_solve(catic_ctx* ctx, const pnp_device_view* view, const catic_params* params, const catic_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_IACONTROL_H */
