/*
 * catint_kintrans.h -- C-ABI of libcatint_kintrans: the TRANSIENT of a mean-field surface microkinetic model, d theta / dt integrated
 * stiffly ON THE DEVICE for a batch of operating points, every point with its own step size.  It answers how the surface gets to the
 * steady state of catint_kinetics.h after a step of the potential or of the surface concentrations (the surface state is constant over
 * the integration), and, followed to long times, it is pseudo-transient continuation: the globally convergent route to that steady
 * state where the damped Newton iteration of catkin_solve from the uniform start does not converge.
 *
 * Conventions: those of catint_kinetics.h (plain C; host pointers to C-contiguous fp64 / int32 / int64 owned by the caller; 0 or a
 * negative CATKT_E* code and catkt_last_error; a context is not thread-safe; the view is read, never written).
 *
 * Definition.  Tables, V, sigma, ln kf, ln kb, activities a_j, rates rf_r, rb_r and m[r][t] are those of catint_kinetics.h.  Unknowns
 * y_t = ln theta_t, t = 0 .. S, of which t = 0 is the free site.
 *   system     d theta_s / dt = G_s(y) = sum_r m[r][s] (rf_r - rb_r),  s = 1 .. S;   sum_t n_t exp(y_t) = 1  (row 0).
 *              The free site is never integrated: conservation is exact.   D_s = sum_r |m[r][s]| (rf_r + rb_r).
 *   start      theta0[n][S+1], each entry to y = ln theta clamped into [CATKIN_MIN_LOG, 0] as theta_guess of catkin_solve is; the
 *              free-site entry is ignored and recomputed, theta_0 = 1 - sum_{t>=1} n_t exp(y_t).  A point whose theta0 is not finite or
 *              leaves theta_0 <= 0 ends CATKT_INPUT.  theta0 NULL: y_t = ln(1 / sum_t n_t), the uniform start of catkin_solve.
 *   BE(y_old, h)  one implicit Euler step, a Newton iteration from y = y_old with theta_old = exp(y_old):
 *                F_s  = (theta_s - theta_old_s - h G_s) / w_s,          w_s = theta_s + h D_s,               s = 1 .. S
 *                A_st = (delta_st theta_s - h Jraw_st) / w_s,           Jraw_st = sum_r m[r][s] (rf_r order_f[r][N+t] - rb_r order_b[r][N+t])
 *                F_0  = sum_t n_t exp(y_t) - 1,                         A_0t = n_t exp(y_t)
 *              A dy = -F by Gaussian elimination with partial row pivoting; the update is scaled by min(1, 3 / max|dy|) and y clamped
 *              to >= CATKIN_MIN_LOG; converged when max|dy| < newton_tol (the update is still applied); failed after newton_maxit
 *              iterations, on a zero or non-finite pivot, or on a non-finite update.  A row with D_s = 0 needs no special case: it
 *              reads theta_s = theta_old_s.
 *   step       of size hh from (t, y) by step doubling: y1 = BE(y, hh); ya = BE(y, hh/2); yb = BE(ya, hh/2), in this order; after a
 *              failed solve the later ones are not run, the step is rejected and h <- hh / 4.  Otherwise
 *                err = max_t |theta_b,t - theta_1,t| / (atol + rtol max(theta_b,t, theta_1,t)),   fac = min(5, max(0.2, 0.9 / sqrt(err)))
 *              (err = 0: fac = 5; err not a number: rejected, fac = 0.2).  err <= 1: yb is accepted as it is (no extrapolation: it
 *              would break the site balance); otherwise the step is rejected and h <- fac hh.
 *   outputs    t_out[n_out]: positive, strictly increasing, the same for every point.  hh = min(h, t_next - t); a step with
 *              t_next - t <= h lands on t_next exactly.  After an accepted step h <- max(h, fac hh) if the step was shortened
 *              (t_next - t < h) and h <- fac hh otherwise.
 *   first step h0 as given; h0 <= 0: 0.01 / max_s (D_s / theta_s) over the rows with D_s > 0 at the start, and t_out[0] if there is none.
 *   drift      after every accepted step: max over s >= 1 with D_s > 0 of |G_s| / D_s, the scaled steady residual of
 *              catint_kinetics.h (0 if there is no such row).  With steady_tol > 0 a point whose drift is below it stops there: every
 *              output row it has not written yet is filled with that state, status CATKT_STEADY, t_reached the time it stopped at.
 *   bounds     a point ends CATKT_STEPS after max_steps attempted steps (accepted or rejected) or when h falls below 1e-300; the
 *              output rows it has not reached are NaN and t_reached is the time it got to.  max_steps <= 1 000 000: no launch runs
 *              unbounded.
 * Outputs, each nullable:
 *   theta[n][n_out][S+1]; flux[n][n_out][N], flux_scale[n][n_out][N]: the instantaneous wall fluxes, the sums of catint_kinetics.h at
 *   the state of the output time; drift[n][n_out]; t_reached[n] (t_out[n_out-1] for CATKT_DONE, NaN for CATKT_INPUT);
 *   status[n]: CATKT_DONE every output time reached; CATKT_STEADY; CATKT_INPUT the handle's status of the lane is non-zero (view path),
 *   an input of the point is not finite or its start leaves no free site: every output of the point is NaN, other points are
 *   unaffected; CATKT_STEPS.   steps[n][3]: accepted steps, rejected steps, inner Newton iterations (those whose update was applied).
 * Surface state: host arrays or the view, exactly as in catkin_solve.  A point's bits do not depend on its position in the batch, on
 * max_waves, on which outputs were asked for or on where the surface state came from.
 */
#ifndef CATINT_KINTRANS_H
#define CATINT_KINTRANS_H

#include <stdint.h>

#include "catint_kinetics.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATKT_OK 0
#define CATKT_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATKT_ENOMEM (-2)
#define CATKT_EDEVICE (-3)  /* HIP runtime error */

#define CATKT_DONE 0
#define CATKT_STEADY 1
#define CATKT_INPUT 2
#define CATKT_STEPS 3

#define CATKT_MAX_STEPS 1000000
#define CATKT_MIN_STEP 1e-300

typedef struct catkt_ctx catkt_ctx;

typedef struct catkt_params {
  int32_t struct_size;        /* = sizeof(catkt_params) */
  int32_t max_waves;          /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t nspecies;           /* N, 0 .. CATKIN_MAX_SPECIES; the view's on the view path */
  int32_t nadsorbates;        /* S, 1 .. CATKIN_MAX_ADSORBATES */
  int32_t nsteps;             /* R, 1 .. CATKIN_MAX_STEPS */
  int32_t newton_maxit;       /* >= 1; iterations of one implicit Euler solve */
  int32_t potential_drop;     /* w: CATKIN_DROP_* */
  int32_t max_steps;          /* 1 .. CATKT_MAX_STEPS attempted steps per point */
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
  double stern_capacitance;   /* C_S, F/m^2; used when sigma is NULL */
  double phi_pzc;             /* V */
  const double* phiM;         /* [n] */
  const double* sigma;        /* [n] C/m^2, or NULL: from C_S */
  const double* off;          /* [n][R][2], or NULL */
  const double* gamma;        /* [n][N], or NULL */
  const double* theta0;       /* [n][S+1], or NULL: the uniform start */
  const double* csurf;        /* [n][N], or NULL: the view */
  const double* phi_surface;  /* [n], or NULL: the view */
  const double* t_out;        /* [n_out] s, positive and strictly increasing */
  int64_t n_out;              /* >= 1 */
  double rtol;                /* > 0, on the coverages */
  double atol;                /* >= 0 */
  double newton_tol;          /* > 0, on max|dy| of an implicit Euler solve */
  double steady_tol;          /* >= 0; 0: no point stops before t_out[n_out-1] */
  double h0;                  /* s; <= 0: the library's choice */
} catkt_params;

typedef struct catkt_outputs {
  int32_t struct_size;        /* = sizeof(catkt_outputs) */
  int32_t reserved;
  double* theta;              /* [n][n_out][S+1] */
  double* flux;               /* [n][n_out][N] mol m^-2 s^-1 */
  double* flux_scale;         /* [n][n_out][N] */
  double* drift;              /* [n][n_out] */
  double* t_reached;          /* [n] s */
  int32_t* status;            /* [n] CATKT_DONE .. CATKT_STEPS */
  int32_t* steps;             /* [n][3] accepted, rejected, Newton iterations */
} catkt_outputs;

/* No device call is made before the first catkt_solve that passes validation with n > 0. */
int catkt_create(int32_t device, catkt_ctx** out);
void catkt_destroy(catkt_ctx* ctx);
const char* catkt_last_error(const catkt_ctx* ctx); /* ctx may be NULL: last catkt_create error */
/* Census-form name of the kernel the last successful call launched ("catkt::transient_kernel"); "" before the first one. */
const char* catkt_last_kernel(const catkt_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catkt_last_kernel_ms(const catkt_ctx* ctx);

/* One integration per operating point.  view, stream and return as in catkin_solve.
 * CATKT_EINVAL, before any device call: everything catkin_solve reports (its tol and maxit aside), and: t_out NULL, n_out < 1, a t_out
 * that is not finite, not positive or not strictly increasing; rtol or newton_tol not positive and finite; atol or steady_tol negative
 * or not a number; newton_maxit < 1; max_steps outside 1 .. CATKT_MAX_STEPS; an h0 that is not a number. */
int catkt_solve(catkt_ctx* ctx, const pnp_device_view* view, const catkt_params* params, const catkt_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_KINTRANS_H */
