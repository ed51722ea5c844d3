/*
 * catint_iasweep.h -- C-ABI of libcatint_iasweep: the VOLTAMMOGRAM of a surface microkinetic model with LATERAL INTERACTIONS between
 * the adsorbates and SEVERAL SITE TYPES, d theta / dt integrated stiffly ON THE DEVICE along a linear potential program (or held at a
 * constant potential) for a batch of operating points, every point with its own program and its own step size.  It joins its two
 * parents: the model is that of catint_interact.h, the method that of catint_voltam.h.  It answers what neither can: the Frumkin
 * broadening or sharpening of an adsorption peak, its shift with the coverage, the hysteresis under attraction, and the relaxation of
 * the interacting model at a constant potential.  As in catint_voltam.h THE ELECTROLYTE DOES NOT ANSWER.
 *
 * Conventions: those of catint_voltam.h (plain C; host pointers to C-contiguous fp64 / int32 / int64 owned by the caller; 0 or a
 * negative CATIS_E* code and catis_last_error; a context is not thread-safe; the view is read, never written).  Only what differs
 * from the two parents is stated here.
 *
 * Model: catint_interact.h.  G site types and T = G + S <= 9 coverage columns, the free sites first; site_of, site_fraction (x_g),
 *   site_count[T] (n_t), eps[S][S], eps_ts[R][S], response, cutoff, smoothing, strength; the per-type site balance of every step and
 *   the host-side contractions EG, EA are those of catint_interact.h.  The rate constants of a rate evaluation are those of
 *   catint_interact.h at lambda = strength, at the lane's CURRENT coverages and at the potential of the solve; the branch of Ga is
 *   chosen anew at every evaluation.  There is no ramp in time.
 * Program, potential, turnover, step, error, acceptance, charge, landing, first step, bounds, statuses: catint_voltam.h, with
 *   BE(y_old, h, E)   rows of the adsorbates s = G .. T-1:   ((theta_s - theta_old,s) - h G_s(y, E)) / w_s,   w_s = theta_s + h D_s
 *              Jacobian row:  ((s == v) theta_s - h dG_s/dy_v) / w_s,   dG_s/dy_v = sum_r m[r][s] (rf_r ofe_rv - rb_r obe_rv)
 *              with ofe, obe the effective orders d ln rf / dy_v, d ln rb / dy_v of catint_interact.h (the shifts inside, the branch
 *              of Ga held within an iteration).  Rows g = 0 .. G-1: the site rows of catint_interact.h.  The update, its damping
 *              min(1, 3 / max|dy|), the clamp, newton_tol, newton_maxit and the pivot rule are those of catvm_solve's solve.
 *   extrapolation   adsorbates theta_e,t = 2 theta_b,t - theta_1,t; the free site of every type from that type's own balance,
 *              theta_e,g = x_g - sum_{adsorbates t on g} n_t theta_e,t (summed from the last adsorbate down).  The extrapolated state
 *              is accepted only if every column is positive; otherwise yb is accepted and the step counts as not extrapolated.
 *   first step D_s / theta_s over the adsorbates s = G .. T-1.
 *   start      theta0 NULL: the ramped steady solve of catint_interact.h at E_start with start_ramp >= 1 stages, tol = newton_tol and
 *              CATIS_START_MAXIT iterations per stage; any status other than converged is the point's CATIS_INPUT.
 *              theta0[n][T] given: the adsorbates as catvm_solve takes them (clamped logarithms), the free site of each type
 *              recomputed from its balance, x_g - sum n_t theta_t; a type left with no free site is CATIS_INPUT.  No steady solve runs.
 *   hold       hold_time[n], nullable.  A point with E_vertex == E_start and a positive, finite hold_time runs at the constant
 *              potential E_start with tau = hold_time: segments, output times and everything else unchanged (the transient of
 *              catint_kintrans.h for the interacting model, with this header's step rule).  scan_rate is still required and only sets
 *              the floor of the current.  A point with E_vertex == E_start and no such hold_time ends CATIS_INPUT as in catvm_solve.
 * Outputs: those of catvm_outputs with theta[n][n_out][T], and energy_shift[n][n_out][S]: dE_t at the output state in kT, nullable.
 * Invariance: a point's bits do not depend on its position in the batch, on max_waves, on which outputs were asked for or on where
 *   the surface state came from.
 * Reduction: with G = 1, strength = 0, start_ramp = 1 and no hold every output has the bits of catvm_solve on the same tables (the
 *   sums are taken in catvm_solve's order), as catia_solve has those of catkin_solve.
 */
#ifndef CATINT_IASWEEP_H
#define CATINT_IASWEEP_H

#include <stdint.h>

#include "catint_interact.h"
#include "catint_voltam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATIS_OK 0
#define CATIS_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATIS_ENOMEM (-2)
#define CATIS_EDEVICE (-3)  /* HIP runtime error */

#define CATIS_DONE 0
#define CATIS_INPUT 2
#define CATIS_STEPS 3

#define CATIS_MAX_STEPS 1000000
#define CATIS_MIN_STEP 1e-300
#define CATIS_MAX_SEGMENTS 64
#define CATIS_MAX_SAMPLES 4096
#define CATIS_START_MAXIT 100
#define CATIS_FARADAY 96485.33289

typedef struct catis_ctx catis_ctx;

typedef struct catis_params {
  int32_t struct_size;        /* = sizeof(catis_params) */
  int32_t max_waves;          /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t nspecies;           /* N, 0 .. CATIA_MAX_SPECIES; the view's on the view path */
  int32_t nadsorbates;        /* S >= 1 */
  int32_t nsteps;             /* R, 1 .. CATIA_MAX_STEPS */
  int32_t newton_maxit;       /* >= 1; iterations of one implicit Euler solve */
  int32_t potential_drop;     /* CATIA_DROP_* */
  int32_t max_steps;          /* 1 .. CATIS_MAX_STEPS attempted steps per point */
  int32_t nsitetypes;         /* G, 1 .. CATIA_MAX_SITE_TYPES; G + S <= CATIA_MAX_COLUMNS */
  int32_t response;           /* CATIA_LINEAR or CATIA_PIECEWISE */
  int32_t start_ramp;         /* >= 1 stages of the steady solve at E_start (theta0 NULL) */
  int32_t reserved;
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
  const double* electrons;    /* [R] ne_r, finite; all zero is allowed */
  double site_density;        /* mol/m^2 of all sites */
  double stern_capacitance;   /* C_S, F/m^2; used when sigma is NULL */
  double phi_pzc;             /* V */
  double strength;            /* lambda of every rate evaluation and of the last stage of the start */
  const double* E_start;      /* [n] V */
  const double* E_vertex;     /* [n] V */
  const double* scan_rate;    /* [n] V/s, positive and finite */
  const double* hold_time;    /* [n] s, or NULL: no point holds */
  const double* sigma;        /* [n] C/m^2, constant over the sweep, or NULL: from C_S at every solve */
  const double* off;          /* [n][R][2], or NULL */
  const double* gamma;        /* [n][N], or NULL */
  const double* theta0;       /* [n][T], or NULL: the steady state at E_start */
  const double* csurf;        /* [n][N], or NULL: the view */
  const double* phi_surface;  /* [n], or NULL: the view */
  int32_t n_segments;         /* 1 .. CATIS_MAX_SEGMENTS */
  int32_t samples;            /* K, 1 .. CATIS_MAX_SAMPLES output times per segment */
  double rate_floor;          /* 1/V, >= 0 */
  double rtol;                /* > 0, on the coverages and on the turnover */
  double atol;                /* >= 0, on the coverages */
  double newton_tol;          /* > 0, on max|dy| of an implicit Euler solve and of the start */
  double h0;                  /* s; <= 0: the library's choice */
} catis_params;

typedef struct catis_outputs {
  int32_t struct_size;        /* = sizeof(catis_outputs) */
  int32_t reserved;
  double* theta;              /* [n][n_out][T] */
  double* current;            /* [n][n_out] A/m^2 */
  double* current_scale;      /* [n][n_out] A/m^2 */
  double* charge;             /* [n][n_out] C/m^2 */
  double* E_out;              /* [n][n_out] V */
  double* flux;               /* [n][n_out][N] mol m^-2 s^-1 */
  double* flux_scale;         /* [n][n_out][N] */
  double* t_reached;          /* [n] s */
  double* energy_shift;       /* [n][n_out][S] kT */
  int32_t* status;            /* [n] CATIS_DONE, CATIS_INPUT, CATIS_STEPS */
  int32_t* steps;             /* [n][4] accepted, rejected, Newton iterations, accepted without extrapolation */
} catis_outputs;

/* No device call is made before the first catis_solve that passes validation with n > 0. */
int catis_create(int32_t device, catis_ctx** out);
void catis_destroy(catis_ctx* ctx);
const char* catis_last_error(const catis_ctx* ctx); /* ctx may be NULL: last catis_create error */
/* Census-form name of the kernel the last successful call launched ("catis::sweep_kernel"); "" before the first one. */
const char* catis_last_kernel(const catis_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catis_last_kernel_ms(const catis_ctx* ctx);

/* One sweep (or hold) per operating point.  view, stream and return as in catvm_solve.
 * CATIS_EINVAL, before any device call: everything catvm_solve reports for the members the structs share (with N+T columns and the
 * site counts [T]) and everything catia_solve reports for the members it brings (G, S and T out of range; site_of, site_fraction, eps
 * missing; a site_of outside [0, G) or a free-site column not on its own type; a site fraction that is not positive and finite; a step
 * that breaks the site balance of one type; a non-finite eps, eps_ts or strength; start_ramp < 1; a response outside the two; in the
 * piecewise mode a missing or non-finite cutoff or a smoothing that is not positive and finite).  A hold_time that is not positive and
 * finite is that point's matter (CATIS_INPUT if its E_vertex equals its E_start), not an error of the call. */
int catis_solve(catis_ctx* ctx, const pnp_device_view* view, const catis_params* params, const catis_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_IASWEEP_H */
