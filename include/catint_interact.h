/*
 * catint_interact.h -- C-ABI of libcatint_interact: the STEADY STATE of a surface microkinetic model with LATERAL INTERACTIONS between
 * the adsorbates and SEVERAL SITE TYPES, solved ON THE DEVICE for a batch of operating points, and the wall fluxes and their
 * sensitivities that follow from it.  It is what include/catint_kinetics.h (mean field, one site type) leaves to a host callback: a
 * binding energy that depends on the coverages (CatMAP's first-order adsorbate interaction model) and adsorbates that compete for the
 * sites of up to three types (terrace and step).  The strength of the interaction is ramped from zero to its value in stages inside
 * one launch, each stage starting from the one before (the reference's n_inter).
 *
 * Conventions, error codes, context functions, the two surface-state paths (host arrays or a pnp_device_view), potential, charge,
 * activities, the off and gamma rows and the status values are those of catint_kinetics.h; only what differs is stated here.
 *
 * Definition.  G site types, 1 <= G <= 3, type g holding the fraction x_g = site_fraction[g] > 0 of all sites.  Coverage columns
 * t = 0 .. T-1, T = G + S, S >= 1, T <= 9, every coverage counted per TOTAL site: column t < G is the free site of type t (n_t = 1,
 * site_of[t] = t), column t >= G an adsorbate on type site_of[t] in [0, G) with n_t in {1, 2, 3}.  With G = 1 the column layout is that
 * of catint_kinetics.h.  order_f, order_b are [R][N+T]; every step conserves the sites of EACH type separately:
 *   sum_{site_of[t] = g} n_t (order_b - order_f)[r][N+t] = 0 for every g.  Unknowns y_t = ln theta_t.
 *   crowding   Theta_g = (sum_{adsorbates t on g} n_t theta_t) / x_g
 *   response   f_g(Theta_g):  CATIA_LINEAR     f = 1, f' = 0
 *                             CATIA_PIECEWISE  with c = cutoff[g], s = smoothing[g] > 0:  f = 0 for Theta <= c - s,
 *                                              f = (Theta - c + s)^2 / (4 s) inside (c - s, c + s), f = Theta - c beyond; f' follows
 *   shifts     with lambda the strength of the stage (below), u over the adsorbates, eps [S][S] and eps_ts [R][S] in kT (adsorbate a is
 *              column G + a):
 *                dE_t  = lambda sum_u eps[t][u] f_{site_of[u]} theta_u        (adsorbates; a free site carries no shift)
 *                dEts_r = lambda sum_u eps_ts[r][u] f_{site_of[u]} theta_u    (transition states)
 *              With CATIA_LINEAR this is CatMAP's first-order model with the linear response.  The piecewise mode LEAVES OUT CatMAP's
 *              second term, 1/2 f' sum eps theta theta: the shift is the first term alone.
 *   constants  dG_r(theta) = dG_r + sum_t m[r][t] dE_t,   m[r][t] = order_b[r][N+t] - order_f[r][N+t]
 *              Ea_r(theta) = Ea_r + dEts_r - sum_t order_f[r][N+t] dE_t     (where e0 is finite; otherwise no transition state)
 *              Both are linear in w_u = f_{site_of[u]} theta_u; the library contracts the rows once on the host,
 *                EG[r][u] = sum_t m[r][t] eps[t][u],   EA[r][u] = eps_ts[r][u] - sum_t order_f[r][N+t] eps[t][u]   (t ascending),
 *              and evaluates dG_r + lambda sum_u EG[r][u] w_u and Ea_r + lambda sum_u EA[r][u] w_u (u ascending).
 *              Ga, ln kf, ln kb, the activities, rf, rb: catint_kinetics.h, with dG_r(theta) and Ea_r(theta).
 *   residual   F_g = (sum_{site_of[t] = g} n_t theta_t) / x_g - 1,   g = 0 .. G-1        (one site row per type)
 *              F_s, D_s and the dead-row rule of catint_kinetics.h for the adsorbates s = G .. T-1
 *   Jacobian   analytic, the branch of Ga held fixed, D_s held fixed within an iteration:
 *                dF_s/dy_v = sum_r m[r][s] (rf_r (of_rv + theta_v dln kf_r/dtheta_v) - rb_r (ob_rv + theta_v dln kb_r/dtheta_v)) / D_s
 *                dln kf/dtheta_v = -dGa/dtheta_v,   dln kb/dtheta_v = -(dGa/dtheta_v - ddG/dtheta_v)
 *                ddE_t/dtheta_v = lambda (eps[t][v] f_g(v) + (n_v / x_g(v)) f'_g(v) sum_{u on g(v)} eps[t][u] theta_u)   (v an adsorbate)
 *                dF_g/dy_t = n_t theta_t / x_g for t on g
 *   iteration  that of catint_kinetics.h (partial pivoting, the update scaled by min(1, 3 / max|dy|), the clamp at CATKIN_MIN_LOG, tol,
 *              maxit PER STAGE) from y_t = ln(x_g / sum_{site_of[u] = g} n_u), g = site_of[t], or from theta_guess[n][T].
 *   ramp       K = ramp >= 1 stages, lambda_k = strength k / (K - 1) for k = 0 .. K-2 and lambda_{K-1} = strength exactly (K = 1: the
 *              one stage has lambda = strength).  Each stage starts from the y the stage before ended with.  A stage that ends with a
 *              status other than 0 ends the point with that status; ramp_reached[n] is the stage the point ended in (K - 1 for a point
 *              that ran them all, 0 for status 2), its outputs are those at that stage's lambda.  iterations[n] is the sum over the
 *              stages.  Every loop is bounded by K maxit and ends when no lane of the wave iterates.
 * Outputs, each nullable: theta[n][T]; rate, rate_gross [n][R]; flux, flux_scale [n][N] = site_density sum_r nu rate (coverages and
 * rates per total site); dflux_dc[n][N][N], dflux_dphi[n][N][2] by the implicit function theorem with the FULL Jacobian above (the
 * shifts included in d rate / dy); energy_shift[n][S] = dE_t at the returned state (the reference's interacting_energy, in kT);
 * status[n] 0 .. 3 as CATKIN_*; iterations[n]; ramp_reached[n].
 * A point's bits do not depend on its position in the batch, on max_waves, on the outputs asked for, or on the surface-state path.
 */
#ifndef CATINT_INTERACT_H
#define CATINT_INTERACT_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATIA_OK 0
#define CATIA_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATIA_ENOMEM (-2)
#define CATIA_EDEVICE (-3)  /* HIP runtime error */

#define CATIA_MAX_SPECIES 8
#define CATIA_MAX_SITE_TYPES 3
#define CATIA_MAX_COLUMNS 9      /* T = G + S */
#define CATIA_MAX_STEPS 16
#define CATIA_MAX_ORDER 3
#define CATIA_MAX_SITES 3
#define CATIA_MIN_LOG (-700.0)

#define CATIA_DROP_FULL 0
#define CATIA_DROP_STERN 1

#define CATIA_LINEAR 0
#define CATIA_PIECEWISE 1

#define CATIA_CONVERGED 0
#define CATIA_MAXIT 1
#define CATIA_INPUT 2
#define CATIA_PIVOT 3

typedef struct catia_ctx catia_ctx;

typedef struct catia_params {
  int32_t struct_size;        /* = sizeof(catia_params) */
  int32_t max_waves;          /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t nspecies;           /* N, 0 .. CATIA_MAX_SPECIES; the view's on the view path */
  int32_t nadsorbates;        /* S >= 1 */
  int32_t nsteps;             /* R, 1 .. CATIA_MAX_STEPS */
  int32_t maxit;              /* >= 1, per stage */
  int32_t potential_drop;     /* CATIA_DROP_* */
  int32_t nsitetypes;         /* G, 1 .. CATIA_MAX_SITE_TYPES; G + S <= CATIA_MAX_COLUMNS */
  int32_t response;           /* CATIA_LINEAR or CATIA_PIECEWISE */
  int32_t ramp;               /* K >= 1 stages */
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
  const double* cutoff;       /* [G], CATIA_PIECEWISE only */
  const double* smoothing;    /* [G] > 0, CATIA_PIECEWISE only */
  double site_density;        /* mol/m^2 of all sites */
  double tol;                 /* on max|dy| */
  double stern_capacitance;
  double phi_pzc;
  double strength;            /* lambda of the last stage */
  const double* phiM;         /* [n] */
  const double* sigma;        /* [n] C/m^2, or NULL: from C_S */
  const double* off;          /* [n][R][2], or NULL */
  const double* gamma;        /* [n][N], or NULL */
  const double* theta_guess;  /* [n][T], or NULL */
  const double* csurf;        /* [n][N], or NULL: the view */
  const double* phi_surface;  /* [n], or NULL: the view */
} catia_params;

typedef struct catia_outputs {
  int32_t struct_size;        /* = sizeof(catia_outputs) */
  int32_t reserved;
  double* theta;              /* [n][T] */
  double* rate;               /* [n][R] 1/s per total site */
  double* rate_gross;         /* [n][R] */
  double* flux;               /* [n][N] mol m^-2 s^-1 */
  double* flux_scale;         /* [n][N] */
  double* dflux_dc;           /* [n][N][N] */
  double* dflux_dphi;         /* [n][N][2] */
  double* energy_shift;       /* [n][S] kT */
  int32_t* status;            /* [n] */
  int32_t* iterations;        /* [n] summed over the stages */
  int32_t* ramp_reached;      /* [n] */
} catia_outputs;

/* No device call is made before the first catia_solve that passes validation with n > 0. */
int catia_create(int32_t device, catia_ctx** out);
void catia_destroy(catia_ctx* ctx);
const char* catia_last_error(const catia_ctx* ctx); /* ctx may be NULL: last catia_create error */
/* Census-form name of the kernel the last successful call launched ("catia::interact_kernel"); "" before the first one. */
const char* catia_last_kernel(const catia_ctx* ctx);
/* Device time of that kernel alone, in milliseconds; -1 before the first one. */
float catia_last_kernel_ms(const catia_ctx* ctx);

/* One ramped steady-state solve per operating point; view, stream and return as catkin_solve.
 * CATIA_EINVAL, before any device call: everything catkin_solve reports (with N+T columns and the site counts [T]), and: G outside
 * 1 .. 3; S < 1 or G + S > 9; a missing site_of, site_fraction or eps; a site_of outside [0, G) or a free-site column that is not on
 * its own type (or whose site count is not 1); a site fraction that is not positive and finite; a step that breaks the site balance
 * of one type; a non-finite eps, eps_ts or strength; ramp < 1; a response outside the two; in the piecewise mode a missing or
 * non-finite cutoff or a smoothing that is not positive and finite. */
int catia_solve(catia_ctx* ctx, const pnp_device_view* view, const catia_params* params, const catia_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_INTERACT_H */
