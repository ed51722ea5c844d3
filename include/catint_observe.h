/*
 * catint_observe.h -- C-ABI of libcatint_observe: electrolyte observables of the physical mode (PNP_METHOD_NEWTON) derived ON THE
 * DEVICE from the state a pnp_handle holds there (pnp_get_device_view, catint_pnp.h), so that only what was asked for crosses PCIe.
 *
 * The quantities are the ones the reference's COMSOL model defines next to the transport equations (comsol_model.py:1010-1063) and
 * its reader puts into tp.alldata (comsol_reader.py:57-90, :196-279): field, charge density, activity coefficient, pH, conductivity,
 * electrolyte current density and the ohmic / diffusion potential drops.
 *
 * Conventions: plain C; every pointer is a HOST pointer to C-contiguous fp64 owned by the caller (the device pointers live in the
 * pnp_device_view); every entry point returns 0 or a negative CATOBS_E* code and catobs_last_error gives the message; a context is
 * not thread-safe, distinct contexts are independent.  The library holds no solver code: it reads the view, nothing else.
 *
 * Definitions (grid x[nx], edge e between points e and e+1, h_e = x[e+1] - x[e], q_k = z_k F, w = -ln(1 - phi0),
 * phi0 = N_A sum_k a_k^3 c_k, B(u) = u / (exp(u) - 1)):
 *   efield          -(phi[i+1] - phi[i-1]) / (x[i+1] - x[i-1]), one-sided at both ends                                [B][nx]
 *   charge_density  sum_k q_k c_k                                                                                     [B][nx]
 *   gamma           1 / (1 - phi0)                                                                                    [B][nx]
 *   pH              -log10(c_H / 1000) - log10 gamma, without H+: 14 + log10(c_OH / 1000) - log10 gamma               [B][nx]
 *   conductivity    beta sum_k q_k^2 D_k (c_k[e] + c_k[e+1]) / 2  (= F^2 sum z^2 D/(RT) c)                            [B][nx-1]
 *   current_density sum_k q_k J_k with the Scharfetter-Gummel edge flux THE SOLVER CONSERVES:
 *                   J_k = -(D_k / h_e) ((B(u) + u) c_k[e+1] - B(u) c_k[e]),  u = q_k beta dphi + dw - velocity h_e / D_k      [B][nx-1]
 *   dphi_iR         prefix sum over edges of -(current_density / conductivity) h_e, leading zero                      [B][nx]
 *   dphi_diff       prefix sum over edges of (sum_k q_k J_k^diff / conductivity) h_e, J_k^diff = -(D_k / h_e) (c_k[e+1] - c_k[e]),
 *                   leading zero; an edge with conductivity <= 0 contributes zero to both sums                        [B][nx]
 * The host path of catint_amd.calculator (Calculator._alldata_arrays) leaves the convection term out of u; at velocity = 0 the two
 * definitions are the same.
 */
#ifndef CATINT_OBSERVE_H
#define CATINT_OBSERVE_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATOBS_OK 0
#define CATOBS_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATOBS_ENOMEM (-2)
#define CATOBS_EDEVICE (-3)  /* HIP runtime error */

#define CATOBS_MAX_SPECIES 8 /* = PNP_NEWTON_MAX_SPECIES */
#define CATOBS_MAX_NX 4098   /* 4 waves x 64 lanes x 16 points + the two boundary points */

/* columns of catobs_outputs.scalars */
#define CATOBS_SURFACE_POTENTIAL 0    /* phi(x = 0) */
#define CATOBS_SURFACE_EFIELD 1       /* efield[0] */
#define CATOBS_SURFACE_GAMMA 2        /* gamma[0] */
#define CATOBS_SURFACE_PH 3           /* pH[0] */
#define CATOBS_DELTA_PHI_IR_INF 4     /* dphi_iR[nx-1] */
#define CATOBS_DELTA_PHI_DIFF_INF 5   /* dphi_diff[nx-1] */
#define CATOBS_DELTA_PHI_INF 6        /* phi[nx-1] - phi[0] */
#define CATOBS_DELTA_PHI_INF_MIN_IR 7 /* phi[nx-1] - phi[0] - dphi_iR[nx-1] */
#define CATOBS_WALL_CURRENT_DENSITY 8 /* current_density[0] */
#define CATOBS_BULK_CONDUCTIVITY 9    /* conductivity[nx-2] */
#define CATOBS_NSCALARS 10

typedef struct catobs_ctx catobs_ctx;

typedef struct catobs_params {
  int32_t struct_size;      /* = sizeof(catobs_params) */
  int32_t species_H;        /* index of H+, -1: absent */
  int32_t species_OH;       /* index of OH- (used without H+), -1: absent; with neither, pH is NaN */
  int32_t max_waves;        /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts: with few waves every
                             * wave walks several operating points (tests) */
  const double* D;          /* [N] m^2/s */
  const double* charges;    /* [N] z F */
  const double* mpb_radius; /* [N] m, NULL or all zero: point ions */
  const double* x;          /* [nx] strictly increasing */
  double beta;              /* 1/(R T) */
  double velocity;          /* convection velocity of pnp_set_convection */
} catobs_params;

/* Any pointer may be NULL: that row is not copied, and not computed where nothing else needs it. */
typedef struct catobs_outputs {
  double* efield;           /* [B][nx] */
  double* charge_density;   /* [B][nx] */
  double* gamma;            /* [B][nx] */
  double* pH;               /* [B][nx] */
  double* conductivity;     /* [B][nx-1] */
  double* current_density;  /* [B][nx-1] */
  double* dphi_iR;          /* [B][nx] */
  double* dphi_diff;        /* [B][nx] */
  double* scalars;          /* [B][CATOBS_NSCALARS]: a scalars-only call moves 80 B bytes to the host */
} catobs_outputs;

/* No device call is made before the first catobs_electrolyte that passes validation. */
int catobs_create(int32_t device, catobs_ctx** out);
void catobs_destroy(catobs_ctx* ctx);
const char* catobs_last_error(const catobs_ctx* ctx); /* ctx may be NULL: last catobs_create error */
/* Census-form name of the kernel instance the last successful call launched, e.g. "catobs::electrolyte_kernel<16, 2, true>"
 * (points per lane, waves per operating point, steric); "" before the first one. */
const char* catobs_last_kernel(const catobs_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catobs_last_kernel_ms(const catobs_ctx* ctx);

/* One pass over the state behind `view` (valid until the next pnp_set_batch / pnp_destroy of its handle).  The kernel and the copies
 * run on view->stream, behind whatever the handle enqueued there, and the call returns when the outputs are on the host.  The state
 * and the status flags of the handle are only read.
 * CATOBS_EINVAL, before any device call: NULL argument, wrong struct_size (view or params), a view without a potential row (compat
 * handle), nx < 3 or > CATOBS_MAX_NX, more than CATOBS_MAX_SPECIES species, x not strictly increasing, species_H / species_OH outside
 * [-1, N). */
int catobs_electrolyte(catobs_ctx* ctx, const pnp_device_view* view, const catobs_params* params, const catobs_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_OBSERVE_H */
