/*
 * catint_voltam.h -- C-ABI of libcatint_voltam: the VOLTAMMOGRAM of a mean-field surface microkinetic model, d theta / dt integrated
 * stiffly ON THE DEVICE along a linear potential program E(t) (linear sweep, cyclic, several cycles) for a batch of operating points,
 * every point with its own program and its own step size.  It answers what catint_kintrans.h cannot: the adsorption and desorption
 * peaks of a sweep, their shift and broadening with the scan rate, the hysteresis between the branches and the charge under a peak.
 * The surface concentrations and the potential of the reaction plane phi_0 are constant over the sweep: THE ELECTROLYTE DOES NOT
 * ANSWER.  Double-layer charging, ohmic drop and depletion in front of the electrode are not part of the current returned here; the
 * transient coupled to transport is out of the scope of this library.
 *
 * Conventions: those of catint_kintrans.h (plain C; host pointers to C-contiguous fp64 / int32 / int64 owned by the caller; 0 or a
 * negative CATVM_E* code and catvm_last_error; a context is not thread-safe; the view is read, never written).
 *
 * Definition.  Tables, ln kf, ln kb, activities a_j, rates rf_r, rb_r, m[r][t], G_s, D_s, the unknowns y_t = ln theta_t and the
 * implicit Euler solve are those of catint_kintrans.h; what is new is that V and sigma move in time and that the current is part of
 * the step control.
 *   program    per point: tau = |E_vertex - E_start| / scan_rate; segment k = 0 .. n_segments-1 runs from E_a = E_start to
 *              E_z = E_vertex for even k and back (E_a = E_vertex, E_z = E_start) for odd k,
 *                E(t) = E_a + (E_z - E_a) ((t - k tau) / tau)   on [k tau, (k+1) tau].
 *              Output times t_{k,m} = (k + m / K) tau, m = 1 .. K = samples: n_out = n_segments K rows per point, row k K + m - 1.
 *              Every vertex is an output time, so no step crosses a kink.  E_out is E(t_{k,m}) by the formula above with its own k.
 *              A point whose E_start or E_vertex is not finite, whose E_vertex equals E_start, or whose tau or n_segments tau is not
 *              finite ends CATVM_INPUT.
 *   potential  an implicit Euler solve that ENDS at time t_e (in segment k) is done at E = E(t_e):  V = E - w phi_0 and
 *              sigma = C_S ((E - phi_PZC) - phi_0), or the caller's sigma[n], which then stays constant over the sweep (a caller who
 *              wants the charge to follow the potential leaves sigma NULL).  The rate constants follow from V and sigma as in
 *              catint_kinetics.h, the branch of Ga chosen anew at every solve.
 *   turnover   i(y, E) = sum_r ne_r (rf_r - rb_r),   g(y, E) = sum_r |ne_r| (rf_r + rb_r),   1/s per site, summed in the order of r;
 *              ne_r = electrons[r], the electrons on the reactant side of step r (negative: released).
 *              current = -F site_density i in A/m^2 (a reduction is negative), current_scale = F site_density g; F = 96485.33289 C/mol.
 *              The number of digits of current is what current / current_scale leaves of 16, as for flux and flux_scale of
 *              catint_kinetics.h: near equilibrium the current is a small difference of large gross rates.
 *   start      theta0 NULL: the damped Newton iteration of catint_kinetics.h at E_start from the uniform start with tol = newton_tol
 *              and maxit = 100 (its iterations are not counted in steps); a point where it does not converge ends CATVM_INPUT.
 *              theta0[n][S+1] given: used exactly as catkt_solve uses it (clamped logarithms, the free site recomputed; a start that is
 *              not finite or leaves no free site ends CATVM_INPUT), and no steady solve runs.
 *   BE(y_old, h, E)   the implicit Euler solve of catint_kintrans.h with the rate constants at E.
 *   step       of size hh from (t, y) in segment k; t_e = t + hh, or the output time itself when the step lands on it:
 *                y1 = BE(y, hh, E(t_e));   ya = BE(y, hh/2, E(t + hh/2));   yb = BE(ya, hh/2, E(t_e)),   in this order,
 *              and i_1, g_1, i_a, i_b, g_b the turnovers at (y1, E(t_e)), (ya, E(t + hh/2)), (yb, E(t_e)).  After a failed solve the
 *              later ones are not run, the step is rejected and h <- hh / 4.  Otherwise
 *                err_theta = max_t |theta_b,t - theta_1,t| / (atol + rtol max(theta_b,t, theta_1,t))
 *                err_i     = |i_b - i_1| / (rtol (max(|i_b|, |i_1|) + rate_floor scan_rate) + newton_tol max(g_b, g_1)),  0 if i_b == i_1
 *                err = max(err_theta, err_i),   fac = min(5, max(0.2, 0.9 / sqrt(err)))
 *              (err = 0: fac = 5; err not a number: rejected, fac = 0.2).  The second term of err_i's denominator is what the Newton
 *              tolerance leaves of a current that is the difference of gross rates: without it a step with a kT/h prefactor could
 *              never be accepted.  err <= 1: accepted; otherwise rejected and h <- fac hh.
 *   acceptance the Richardson-extrapolated state theta_e,t = 2 theta_b,t - theta_1,t for t >= 1, theta_e,0 = 1 - sum_{t>=1} n_t theta_e,t
 *              (the site balance is linear, so it stays exact).  If every theta_e,t > 0, t = 0 .. S, the new state is y = ln theta_e
 *              clamped to >= CATKIN_MIN_LOG; otherwise yb is accepted as it is and the step is counted as not extrapolated.
 *   charge     dq_1 = hh i_1;  dq_b = (hh/2) (i_a + i_b);  the accepted dq = 2 dq_b - dq_1 for an extrapolated step and dq_b otherwise;
 *              charge = -F site_density sum dq in C/m^2, cumulative from t = 0.
 *              Identity: if there is a vector w with ne_r = sum_s w_s m[r][s] for every step (surface-confined redox has one), every
 *              implicit Euler solve satisfies h i = sum_s w_s (theta_s - theta_old,s) up to the Newton tolerance, so
 *              sum dq = sum_s w_s (theta_s(t) - theta_s(0)) at every output time; extrapolation is linear in both sides and keeps it.
 *   landing    hh = min(h, t_next - t); a step with t_next - t <= h lands on t_next exactly.  After an accepted step
 *              h <- max(h, fac hh) if the step was shortened (t_next - t < h) and h <- fac hh otherwise.
 *   first step h0 as given; h0 <= 0: 0.01 / max_s (D_s / theta_s) over the rows with D_s > 0 at the start, and t_{0,1} if there is none.
 *   bounds     a point ends CATVM_STEPS after max_steps attempted steps (accepted or rejected) or when h falls below 1e-300; the
 *              output rows it has not reached are NaN and t_reached is the time it got to.  There is no steady stop.
 * Outputs, each nullable:
 *   theta[n][n_out][S+1] (exp of the accepted y); current, current_scale, charge, E_out [n][n_out]; flux, flux_scale [n][n_out][N]:
 *   the instantaneous wall fluxes at the state and potential of the output time; t_reached[n] (n_segments tau for CATVM_DONE, NaN for
 *   CATVM_INPUT); status[n]: CATVM_DONE every output time reached; CATVM_INPUT the handle's status of the lane is non-zero (view
 *   path), an input of the point is not finite, its program is empty or its start fails: every output of the point is NaN, other
 *   points are unaffected; CATVM_STEPS.  The value 1 is unused: the codes line up with catint_kintrans.h.
 *   steps[n][4]: accepted steps, rejected steps, inner Newton iterations (those whose update was applied), accepted steps that were
 *   not extrapolated.
 * Surface state: host arrays or the view, exactly as in catkt_solve.  A point's bits do not depend on its position in the batch, on
 * max_waves, on which outputs were asked for or on where the surface state came from.
 */
#ifndef CATINT_VOLTAM_H
#define CATINT_VOLTAM_H

#include <stdint.h>

#include "catint_kinetics.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATVM_OK 0
#define CATVM_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATVM_ENOMEM (-2)
#define CATVM_EDEVICE (-3)  /* HIP runtime error */

#define CATVM_DONE 0
#define CATVM_INPUT 2
#define CATVM_STEPS 3

#define CATVM_MAX_STEPS 1000000
#define CATVM_MIN_STEP 1e-300
#define CATVM_MAX_SEGMENTS 64
#define CATVM_MAX_SAMPLES 4096
#define CATVM_START_MAXIT 100
#define CATVM_FARADAY 96485.33289

typedef struct catvm_ctx catvm_ctx;

typedef struct catvm_params {
  int32_t struct_size;        /* = sizeof(catvm_params) */
  int32_t max_waves;          /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t nspecies;           /* N, 0 .. CATKIN_MAX_SPECIES; the view's on the view path */
  int32_t nadsorbates;        /* S, 1 .. CATKIN_MAX_ADSORBATES */
  int32_t nsteps;             /* R, 1 .. CATKIN_MAX_STEPS */
  int32_t newton_maxit;       /* >= 1; iterations of one implicit Euler solve */
  int32_t potential_drop;     /* w: CATKIN_DROP_* */
  int32_t max_steps;          /* 1 .. CATVM_MAX_STEPS attempted steps per point */
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
  const double* electrons;    /* [R] ne_r, finite; all zero is allowed */
  double site_density;        /* mol/m^2 */
  double stern_capacitance;   /* C_S, F/m^2; used when sigma is NULL */
  double phi_pzc;             /* V */
  const double* E_start;      /* [n] V */
  const double* E_vertex;     /* [n] V */
  const double* scan_rate;    /* [n] V/s, positive and finite */
  const double* sigma;        /* [n] C/m^2, constant over the sweep, or NULL: from C_S at every solve */
  const double* off;          /* [n][R][2], or NULL */
  const double* gamma;        /* [n][N], or NULL */
  const double* theta0;       /* [n][S+1], or NULL: the steady state at E_start */
  const double* csurf;        /* [n][N], or NULL: the view */
  const double* phi_surface;  /* [n], or NULL: the view */
  int32_t n_segments;         /* 1 .. CATVM_MAX_SEGMENTS */
  int32_t samples;            /* K, 1 .. CATVM_MAX_SAMPLES output times per segment */
  double rate_floor;          /* 1/V, >= 0: rate_floor scan_rate is the turnover below which the current is not resolved relatively */
  double rtol;                /* > 0, on the coverages and on the turnover */
  double atol;                /* >= 0, on the coverages */
  double newton_tol;          /* > 0, on max|dy| of an implicit Euler solve and of the start */
  double h0;                  /* s; <= 0: the library's choice */
} catvm_params;

typedef struct catvm_outputs {
  int32_t struct_size;        /* = sizeof(catvm_outputs) */
  int32_t reserved;
  double* theta;              /* [n][n_out][S+1] */
  double* current;            /* [n][n_out] A/m^2 */
  double* current_scale;      /* [n][n_out] A/m^2 */
  double* charge;             /* [n][n_out] C/m^2 */
  double* E_out;              /* [n][n_out] V */
  double* flux;               /* [n][n_out][N] mol m^-2 s^-1 */
  double* flux_scale;         /* [n][n_out][N] */
  double* t_reached;          /* [n] s */
  int32_t* status;            /* [n] CATVM_DONE, CATVM_INPUT, CATVM_STEPS */
  int32_t* steps;             /* [n][4] accepted, rejected, Newton iterations, accepted without extrapolation */
} catvm_outputs;

/* No device call is made before the first catvm_solve that passes validation with n > 0. */
int catvm_create(int32_t device, catvm_ctx** out);
void catvm_destroy(catvm_ctx* ctx);
const char* catvm_last_error(const catvm_ctx* ctx); /* ctx may be NULL: last catvm_create error */
/* Census-form name of the kernel the last successful call launched ("catvm::sweep_kernel"); "" before the first one. */
const char* catvm_last_kernel(const catvm_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catvm_last_kernel_ms(const catvm_ctx* ctx);

/* One sweep per operating point.  view, stream and return as in catkt_solve.
 * CATVM_EINVAL, before any device call: everything catkt_solve reports for the members the two structs share, and: electrons NULL or
 * not finite; E_start, E_vertex or scan_rate NULL; a scan_rate that is not positive and finite; n_segments outside
 * 1 .. CATVM_MAX_SEGMENTS; samples outside 1 .. CATVM_MAX_SAMPLES; a rate_floor that is negative or not finite.  A non-finite E_start
 * or E_vertex of one point is that point's CATVM_INPUT, not an error of the call. */
int catvm_solve(catvm_ctx* ctx, const pnp_device_view* view, const catvm_params* params, const catvm_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_VOLTAM_H */
