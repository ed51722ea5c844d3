/*
 * catint_regrid.h -- C-ABI of libcatint_regrid: the state a pnp_handle of the physical mode (PNP_METHOD_NEWTON) holds on the device
 * (pnp_get_device_view, catint_pnp.h) resampled ON THE DEVICE onto another grid, with the interpolant the solver's own discretisation
 * implies inside a cell.  The result stays on the device in the row layout of a handle of the target grid, so that
 * pnp_set_lanes_device (catint_pnp.h) hands it to such a handle without a copy over PCIe; the host gets it only when it asks.
 *
 * Conventions (those of catint_balance.h): plain C; every pointer of the parameters is a HOST pointer to C-contiguous fp64 / int32 /
 * int64 owned by the caller (the device pointers live in the pnp_device_view); every entry point returns 0 or a negative CATGRID_E*
 * code and catgrid_last_error gives the message; a context is not thread-safe, distinct contexts are independent.  The library reads
 * the view, nothing else.
 *
 * Definition (source grid x[nx], edge e between points e and e+1, h_e = x[e+1] - x[e]; q_k = z_k F; phi0 = N_A sum_k a_k^3 c_k,
 * w = -ln(1 - phi0), 0 for point ions; B(u) = u / (exp(u) - 1), by its series below |u| = 0.05: the solver's evaluation).  Inside a
 * cell the Scharfetter-Gummel flux assumes a linear potential (and a linear w) and a constant flux; under that assumption c_k(x) is an
 * exponential profile between the two node values.  A target point X lies in source cell e, the largest e <= nx-2 with x[e] <= X;
 * with s = (X - x[e]) / h_e:
 *   phi(X) = phi_e + s dphi,  dphi = phi_{e+1} - phi_e                       (and w(X) = w_e + s dw, which is what u below carries)
 *   u      = q_k beta dphi + dw - velocity h_e / D_k                         the solver's u (catint_balance.h: flux), clamped to |u| <= 500
 *   c_k(X) = H c_k[e] + G c_k[e+1],  G = s B(-u) / B(-u s),  H = (1 - s) B(u) / B(u (1 - s))
 * All four B are evaluated directly (B(u) = B(-u) - u cancels for large u).  G + H = 1 and both weights are >= 0: the result is a
 * convex combination of the two node values, without cancellation, positive wherever the source is.  Sub-edges of a nested refinement
 * carry the parent edge's flux, and an equilibrium profile c = c_b exp(-q beta phi) is reproduced exactly.  s == 0 copies the node
 * value bit for bit; that includes the last node X == x[nx-1] (e = nx-1, s = 0).  There is no extrapolation.
 */
#ifndef CATINT_REGRID_H
#define CATINT_REGRID_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATGRID_OK 0
#define CATGRID_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATGRID_ENOMEM (-2)
#define CATGRID_EDEVICE (-3)  /* HIP runtime error */

#define CATGRID_MAX_SPECIES 8 /* = PNP_NEWTON_MAX_SPECIES */
#define CATGRID_MAX_NX 4098   /* source and target grid: 4 waves x 64 lanes x 16 points + the two boundary points */
#define CATGRID_MAX_U 500.0   /* |u| is clamped here */

typedef struct catgrid_ctx catgrid_ctx;

typedef struct catgrid_params {
  int32_t struct_size;       /* = sizeof(catgrid_params) */
  int32_t max_waves;         /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  const double* D;           /* [N] m^2/s */
  const double* charges;     /* [N] z F */
  const double* mpb_radius;  /* [N] m, NULL or all zero: point ions */
  double beta;               /* 1/(R T) */
  double velocity;           /* convection velocity of pnp_set_convection */
  const double* x;           /* [nx] the source grid, strictly increasing */
  int32_t nx_target;         /* 3 .. CATGRID_MAX_NX */
  int32_t reserved;
  const double* x_target;    /* [nx_target] strictly increasing, inside [x[0], x[nx-1]] */
  int64_t nlanes;            /* with lanes: how many */
  const int64_t* lanes;      /* [nlanes] source operating points to resample, in this order (repeats allowed); NULL: all, n = batch */
} catgrid_params;

/* n = nlanes, or the view's batch when lanes is NULL; pitch = nx_target rounded up to 16 doubles: the row pitch of a handle of
 * nx_target points (pnp_row_pitch).  Any pointer may be NULL. */
typedef struct catgrid_outputs {
  double* c;                 /* host [n][N][nx_target] */
  double* phi;               /* host [n][nx_target] */
  const double** c_dev;      /* receives the device address of the result [n][N][pitch] in the context's buffer (pads are zero) */
  const double** phi_dev;    /* receives the device address of [n][pitch] */
} catgrid_outputs;

/* No device call is made before the first catgrid_resample that passes validation. */
int catgrid_create(int32_t device, catgrid_ctx** out);
void catgrid_destroy(catgrid_ctx* ctx);
const char* catgrid_last_error(const catgrid_ctx* ctx); /* ctx may be NULL: last catgrid_create error */
/* Census-form name of the kernel instance the last successful call launched, e.g. "catgrid::regrid_kernel<2, true>" (waves per
 * operating point, steric); "" before the first one. */
const char* catgrid_last_kernel(const catgrid_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catgrid_last_kernel_ms(const catgrid_ctx* ctx);

/* One pass over the state behind `view` (valid until the next pnp_set_batch / pnp_destroy of its handle).  The kernel and the copies
 * run on view->stream, behind whatever the handle enqueued there, and the call returns with the result complete: on the host where
 * c / phi were given, and in the context's device buffer, whose addresses *c_dev / *phi_dev stay valid until the next call on the
 * context or its destruction.  The state and the status flags of the handle are only read.
 * CATGRID_EINVAL, before any device call: NULL argument, wrong struct_size (view or params), a view without a potential row (compat
 * handle), nx < 3 or > CATGRID_MAX_NX, more than CATGRID_MAX_SPECIES species, x not strictly increasing, a D that is not positive and
 * finite, a charge or velocity that is not finite, a beta that is not positive and finite, a negative or non-finite radius, nx_target
 * outside [3, CATGRID_MAX_NX], x_target NULL or not strictly increasing, a target point outside [x[0], x[nx-1]], nlanes < 0, a lane
 * index outside [0, batch).  n == 0: nothing is done. */
int catgrid_resample(catgrid_ctx* ctx, const pnp_device_view* view, const catgrid_params* params, const catgrid_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_REGRID_H */
