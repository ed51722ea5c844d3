/*
 * catint_equil.h -- C-ABI of libcatint_equil: the equilibrium (zero wall flux) state of the physical mode (PNP_METHOD_NEWTON) solved
 * ON THE DEVICE as a discrete size-modified Poisson-Boltzmann problem.  With zero wall flux the Scharfetter-Gummel flux of the
 * solver's discretisation vanishes on every edge exactly when c_k exp(q_k beta phi + w) is the same at every node, so the stationary
 * system collapses to one scalar nonlinear tridiagonal equation for phi; the concentrations follow in closed form.  The result is a
 * root of the solver's own residual: a stationary solve of a zero-flux handle started from it converges at once, and a solve with
 * fluxes and kinetics starts from the fully formed double layer instead of walking a continuation path towards it.  It stays on the
 * device in the row layout of the handle behind the view, so that pnp_set_lanes_device (catint_pnp.h) takes it without a copy over
 * PCIe; the host gets it only when it asks.
 *
 * Conventions (those of catint_regrid.h): plain C; every pointer of the parameters is a HOST pointer to C-contiguous fp64 / int32 /
 * int64 owned by the caller; every entry point returns 0 or a negative CATEQ_E* code and cateq_last_error gives the message; a
 * context is not thread-safe, distinct contexts are independent.  Of the view the library reads the geometry (species, points, row
 * pitch, batch) and the stream, nothing else: the state behind it is neither read nor written.
 *
 * Definition (grid x[nx], edge e between points e and e+1, h_e = x[e+1] - x[e]; the grid weights are the solver's: w_e = dx / h_e,
 * v_i = V_i / dx with V_i the control volume (half cells at both ends), pe = dx^2 / eps; q_k = z_k F).  Per operating point the
 * unknowns are phi_i, and
 *   E_k,i = exp(-q_k beta (phi_i - phi_bulk))          exponent clamped to |.| <= CATEQ_MAX_EXPONENT
 *   a_k,i = c_bulk,k E_k,i / (1 - phi0_bulk)           phi0_bulk = sum_k vol_k c_bulk,k, vol_k = N_A a_k^3 (0: point ions)
 *   S_i   = sum_k vol_k a_k,i
 *   c_k,i = a_k,i / (1 + S_i)                          so 1 - phi0_i = 1 / (1 + S_i), formed without cancellation
 *   rho_i = sum_k q_k c_k,i
 *   interior: w_i (phi_{i+1} - phi_i) - w_{i-1} (phi_i - phi_{i-1}) + pe v_i rho_i = 0
 *   wall:     phi_0 = phiM   (Dirichlet)   or   w_0 (phi_1 - phi_0) + (dx C_S / eps) (phiM - phi_PZC - phi_0) = 0   (Stern)
 *   bulk:     phi_{nx-1} = phi_bulk
 * which are the Poisson rows of the solver with the Boltzmann concentrations put in.
 *
 * Iteration: damped Newton from phi = phi_bulk everywhere with the scalar tridiagonal Jacobian, whose diagonal is
 * -(w_i + w_{i-1}) + pe v_i d rho / d phi_i with d rho / d phi = -beta sum_k q_k^2 c_k + beta rho sum_k vol_k q_k c_k; a positive
 * d rho / d phi_i (possible only with unequal radii) is replaced by 0: the matrix stays diagonally dominant and the root is the same.
 * With m = max_k |q_k beta| max_i |dphi_i| the update is scaled by min(1, 2 / m); the iteration stops when m < tol (the update is
 * still applied), or after maxit iterations.  Per operating point: status 0, or 1 when it stopped at maxit, and the iteration count.
 */
#ifndef CATINT_EQUIL_H
#define CATINT_EQUIL_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATEQ_OK 0
#define CATEQ_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATEQ_ENOMEM (-2)
#define CATEQ_EDEVICE (-3)  /* HIP runtime error */

#define CATEQ_MAX_SPECIES 8 /* = PNP_NEWTON_MAX_SPECIES */
#define CATEQ_MAX_NX 4098   /* 4 waves x 64 lanes x 16 points + the two boundary points */
#define CATEQ_MAX_EXPONENT 500.0
#define CATEQ_MAX_ITERATIONS 1000

#define CATEQ_WALL_DIRICHLET 0
#define CATEQ_WALL_STERN 1

typedef struct cateq_ctx cateq_ctx;

typedef struct cateq_params {
  int32_t struct_size;       /* = sizeof(cateq_params) */
  int32_t max_waves;         /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  const double* charges;     /* [N] z F */
  const double* mpb_radius;  /* [N] m, NULL or all zero: point ions */
  const double* x;           /* [nx] the grid, strictly increasing */
  double beta;               /* 1/(R T) */
  double eps;                /* permittivity */
  double dx;                 /* the row-scaling length of the handle (cfg.dx) */
  int32_t wall_bc;           /* CATEQ_WALL_DIRICHLET / CATEQ_WALL_STERN */
  int32_t maxit;             /* >= 1; clamped to CATEQ_MAX_ITERATIONS */
  double stern_capacitance;  /* Stern wall: > 0 */
  double phi_pzc;
  double tol;                /* > 0 */
  const double* phiM;        /* [n] wall potential of every requested operating point */
  const double* phi_bulk;    /* [n] */
  const double* c_bulk;      /* [n][N] */
  int64_t nlanes;            /* n: operating points to solve (result rows) */
} cateq_params;

/* n = params.nlanes; pitch = the view's row pitch.  Any pointer may be NULL. */
typedef struct cateq_outputs {
  double* c;                 /* host [n][N][nx] */
  double* phi;               /* host [n][nx] */
  int32_t* status;           /* host [n]: 0, or 1: not converged within maxit */
  int32_t* iterations;       /* host [n] */
  const double** c_dev;      /* receives the device address of the result [n][N][pitch] in the context's buffer (pads are zero) */
  const double** phi_dev;    /* receives the device address of [n][pitch] */
} cateq_outputs;

/* No device call is made before the first cateq_solve that passes validation. */
int cateq_create(int32_t device, cateq_ctx** out);
void cateq_destroy(cateq_ctx* ctx);
const char* cateq_last_error(const cateq_ctx* ctx); /* ctx may be NULL: last cateq_create error */
/* Census-form name of the kernel instance the last successful call launched, e.g. "cateq::pb_kernel<16, 2, true>" (points per lane,
 * waves per operating point, steric); "" before the first one. */
const char* cateq_last_kernel(const cateq_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float cateq_last_kernel_ms(const cateq_ctx* ctx);

/* n operating points solved on the grid of the handle behind `view` (valid until the next pnp_set_batch / pnp_destroy of its handle).
 * The kernel and the copies run on view->stream, behind whatever the handle enqueued there, and the call returns with the result
 * complete: on the host where c / phi / status / iterations were given, and in the context's device buffer, whose addresses
 * *c_dev / *phi_dev stay valid until the next call on the context or its destruction.
 * CATEQ_EINVAL, before any device call: NULL argument, wrong struct_size (view or params), a view without a potential row (compat
 * handle), nx < 3 or > CATEQ_MAX_NX, more than CATEQ_MAX_SPECIES species, charges or x NULL, x not strictly increasing, a charge that
 * is not finite, a beta / eps / dx / tol that is not positive and finite, a negative max_waves, a maxit
 * below 1, a negative or non-finite radius, a wall_bc that is neither, a Stern wall with a capacitance that is not positive and finite
 * or a phi_pzc that is not finite, nlanes < 0, with nlanes > 0 a NULL phiM / phi_bulk / c_bulk, a non-finite phiM or phi_bulk, a
 * negative or non-finite c_bulk, phi0_bulk >= 1.  n == 0: nothing is done. */
int cateq_solve(cateq_ctx* ctx, const pnp_device_view* view, const cateq_params* params, const cateq_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_EQUIL_H */
