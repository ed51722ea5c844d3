/*
 * catint_scfkin.h -- C-ABI of libcatint_scfkin: the kinetic half of the self-consistency loop between a mean-field surface
 * microkinetic model and the transport solve, ON THE DEVICE and inside the loop.  pnp_scf_cycle_fn (catint_pnp.h) runs mixing, pH,
 * the transport solve and the convergence test of every lane on the device and asks a function of the caller for the wall fluxes once
 * per iteration; catsk_flux_fn is such a function.  It enqueues one launch of catsk::flux_kernel on the loop's stream: per active
 * lane the steady state of the microkinetic model at the loop's mixed surface state, warm-started from the coverages the lane found
 * in the previous iteration, which stay on the device.  No copy, no allocation and no synchronisation per iteration.
 *
 * Conventions (those of catint_kinetics.h): plain C; every pointer of the parameters and outputs is a HOST pointer to C-contiguous
 * fp64 / int32 owned by the caller; every entry point returns 0 or a negative CATSK_E* code and catsk_last_error gives the message; a
 * context is not thread-safe, distinct contexts are independent.
 *
 * Definition.  The model, its tables, the rate constants, the residual and the Newton iteration are those of catint_kinetics.h (the
 * two kernels compile the iteration and the flux sums from one text, csrc/pnp_kin.h).  sigma and off of catkin_params are not
 * offered: the charge is C_S (phiM - phi_PZC - phi_0).  Per-lane arrays are indexed by the lane of the batch.
 * Per call of the flux function and lane b with active[b] != 0 (a lane with active[b] == 0 reads and writes nothing):
 *   surface state  c_j(0) = surface_concentration[b][j], phi_0 = surface_potential[b] of pnp_scf_device; a negative concentration
 *                  counts as zero; a non-finite input gives status CATSK_INPUT.
 *   start          y_t = ln theta[b][t] (clamped into [CATSK_MIN_LOG, 0]) when every stored coverage of the lane is finite, else the
 *                  uniform start y_t = ln(1 / sum_t n_t).  theta[b] is the guess of catsk_begin before the lane's first call (NaN:
 *                  none) and what the lane's last call found afterwards.
 *   results        theta[b], flux_scale[b], status[b], iterations_last[b] are written, iterations_total[b] grows by the iterations
 *                  taken and calls[b] by one.  Status 0: flux[b][k] = flux_last[b][k] = site_density sum_r nu[r][k] rate_r.  Any
 *                  other status: flux[b][k] = NaN -- the transport solve of pnp_scf_cycle_fn then ends non-finite and the lane
 *                  leaves its loop with failed = 1 -- and flux_last[b] keeps its previous value.  CATSK_INPUT: theta[b] and
 *                  flux_scale[b] are NaN.
 * For the same inputs the numbers are those of catkin_solve, bit for bit.
 */
#ifndef CATINT_SCFKIN_H
#define CATINT_SCFKIN_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATSK_OK 0
#define CATSK_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATSK_ENOMEM (-2)
#define CATSK_EDEVICE (-3)  /* HIP runtime error */

#define CATSK_MAX_SPECIES 8      /* = CATKIN_MAX_SPECIES */
#define CATSK_MAX_ADSORBATES 8
#define CATSK_MAX_STEPS 16
#define CATSK_MIN_LOG (-700.0)

#define CATSK_DROP_FULL 0        /* V = phiM */
#define CATSK_DROP_STERN 1       /* V = phiM - phi(x = 0) */

#define CATSK_CONVERGED 0        /* the CATKIN_* values */
#define CATSK_MAXIT 1
#define CATSK_INPUT 2
#define CATSK_PIVOT 3

typedef struct catsk_ctx catsk_ctx;

typedef struct catsk_params {
  int32_t struct_size;        /* = sizeof(catsk_params) */
  int32_t max_waves;          /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t nspecies;           /* N, 0 .. CATSK_MAX_SPECIES: the handle's */
  int32_t nadsorbates;        /* S, 1 .. CATSK_MAX_ADSORBATES */
  int32_t nsteps;             /* R, 1 .. CATSK_MAX_STEPS */
  int32_t maxit;              /* >= 1 */
  int32_t potential_drop;     /* w: CATSK_DROP_* */
  int32_t reserved;
  int64_t batch;              /* B >= 1: the handle's batch */
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
  double stern_capacitance;   /* C_S, F/m^2 */
  double phi_pzc;             /* V */
  const double* phiM;         /* [B] */
  const double* gamma;        /* [B][N], or NULL */
  const double* theta_guess;  /* [B][S+1], or NULL */
} catsk_params;

typedef struct catsk_outputs {
  int32_t struct_size;        /* = sizeof(catsk_outputs) */
  int32_t reserved;
  double* theta;              /* [B][S+1] */
  double* flux_scale;         /* [B][N] of the lane's last call */
  double* flux_last;          /* [B][N] of the lane's last call with status 0 */
  int32_t* status;            /* [B] of the lane's last call */
  int32_t* iterations_last;   /* [B] */
  int32_t* iterations_total;  /* [B] over all calls since catsk_begin */
  int32_t* calls;             /* [B] calls since catsk_begin in which the lane was active */
} catsk_outputs;

/* No device call is made before the first catsk_begin that passes validation. */
int catsk_create(int32_t device, catsk_ctx** out);
void catsk_destroy(catsk_ctx* ctx);
const char* catsk_last_error(const catsk_ctx* ctx); /* ctx may be NULL: last catsk_create error */
/* Census-form name of the kernel the last call launched ("catsk::flux_kernel"); "" before the first one. */
const char* catsk_last_kernel(const catsk_ctx* ctx);

/* Validates, then uploads the model and the per-lane inputs once and allocates the per-lane buffers that stay on the device until
 * the next catsk_begin: theta [B][S+1] (the guess, NaN where none was given), flux_scale, flux_last [B][N], status, iterations_last,
 * iterations_total, calls [B], all zero.  CATSK_EINVAL, before any device call: the rules of catkin_solve for the fields the two
 * structures share, batch < 1, a non-finite stern_capacitance or phi_pzc. */
int catsk_begin(catsk_ctx* ctx, const catsk_params* params);

/* The address of a function of type pnp_scf_flux_fn whose `user` is the catsk_ctx*.  It returns non-zero, and launches nothing, when
 * the context is NULL or catsk_begin has not been called (1), or d's struct_size (2), batch (3) or nspecies (4) differ from what
 * catsk_begin was given, or the launch failed (5); catsk_last_error has the message.  Otherwise it enqueues one launch of
 * catsk::flux_kernel on d->stream and returns 0. */
pnp_scf_flux_fn catsk_flux_fn(void);

/* The kinetic half of a host-driven loop: csurf [B][N], phi_surface [B], active [B] and flux [B][N] go to device buffers of the
 * context, the function of catsk_flux_fn runs on the default stream, flux comes back (rows of inactive lanes as they went in), and
 * the call returns when it is on the host.  The warm starts stay on the device between calls. */
int catsk_step_host(catsk_ctx* ctx, const double* csurf, const double* phi_surface, const int32_t* active, double* flux);

/* Waits for the device and copies what was asked for (a NULL field is not touched) to the host.  The buffers stay as they are: the loop
 * can go on, and the context can catsk_begin again. */
int catsk_end(catsk_ctx* ctx, const catsk_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_SCFKIN_H */
