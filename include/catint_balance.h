/*
 * catint_balance.h -- C-ABI of libcatint_balance: the per-species picture of the physical mode (PNP_METHOD_NEWTON) derived ON THE
 * DEVICE from the state a pnp_handle holds there (pnp_get_device_view, catint_pnp.h): edge fluxes, homogeneous reaction rates and
 * species sources, wall-reaction rates and wall fluxes, and the discrete conservation law itself -- the dc_k/dt that fluxes, sources
 * and wall terms of a returned state imply at every grid point.  The library shares no code with the Newton kernels: its balance is
 * evidence about a solution that does not come from the solver that produced it.
 *
 * Conventions (those of catint_observe.h): plain C; every pointer is a HOST pointer to C-contiguous fp64 / int32 owned by the caller
 * (the device pointers live in the pnp_device_view); every entry point returns 0 or a negative CATBAL_E* code and catbal_last_error
 * gives the message; a context is not thread-safe, distinct contexts are independent.  The library reads the view, nothing else.
 *
 * Definitions -- the ones the solver conserves (grid x[nx], edge e between points e and e+1, h_e = x[e+1] - x[e]; V_i the control
 * volume in metres: (h_{i-1} + h_i) / 2, half cells h_0 / 2 and h_{nx-2} / 2 at the ends; q_k = z_k F; phi0 = N_A sum_k a_k^3 c_k,
 * w = -ln(1 - phi0), gamma = 1 / (1 - phi0); B(u) = u / (exp(u) - 1), by its series below |u| = 0.05):
 *   flux          J_k = -(D_k / h_e) ((B(u) + u) c_k[e+1] - B(u) c_k[e]),  u = q_k beta dphi + dw - velocity h_e / D_k   [B][N][nx-1]
 *                 (the flux catint_observe.h sums into current_density)
 *   reaction_rate forward minus backward, mass action in activities: kf gamma^m prod c_lhs - kr gamma^m' prod c_rhs, m / m' the
 *                 number of entries of the side; a side whose rate constant is 0 contributes nothing; a species that is
 *                 listed twice enters twice                                                                              [B][R][nx]
 *   source        R_k = sum_r (n_rhs(k, r) - n_lhs(k, r)) rate_r, n_side(k, r) = how often k is listed on that side       [B][N][nx]
 *   wall_rate     k[b][r] c_s / (1 + saturation_r c_s) exp(alpha_r (phiM[b] - phi(0))), c_s = c_species[r](0), 1 for species -1
 *                                                                                                                        [B][n_wall]
 *   wall_flux     flux[b][k] + sum_r nu[r][k] wall_rate_r: the flux into the domain                                      [B][N]
 *   imbalance     the dc_k/dt the discrete law implies: (J_{i-1/2} - J_{i+1/2}) / V_i + R_k,i at interior points,
 *                 (wall_flux_k - J_{1/2}) / V_0 + R_k,0 at the wall, 0 at the Dirichlet point nx-1.  Zero on a stationary
 *                 solution, the time derivative on a transient one                                                      [B][N][nx]
 *   scalars       per species, see the CATBAL_* columns below                                                [B][N][CATBAL_NSCALARS]
 * scale_i of CATBAL_MAX_IMBALANCE_REL is the sum of the absolute values of every term that enters imbalance_i: both Bernoulli
 * products of both edges, (D_k / h_e) (|(B(u) + u) c_k[e+1]| + |B(u) c_k[e]|) / V_i; at the wall |flux[b][k]| / V_0 and
 * |nu[r][k] wall_rate_r| / V_0 of every wall reaction; and (n_lhs(k, r) + n_rhs(k, r)) (|forward_r| + |backward_r|) of every
 * reaction.  A point whose scale is 0 counts as 0.
 */
#ifndef CATINT_BALANCE_H
#define CATINT_BALANCE_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATBAL_OK 0
#define CATBAL_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATBAL_ENOMEM (-2)
#define CATBAL_EDEVICE (-3)  /* HIP runtime error */

#define CATBAL_MAX_SPECIES 8 /* = PNP_NEWTON_MAX_SPECIES */
#define CATBAL_MAX_NX 4098   /* 4 waves x 64 lanes x 16 points + the two boundary points */

/* columns of catbal_outputs.scalars */
#define CATBAL_WALL_FLUX 0          /* wall_flux_k */
#define CATBAL_BULK_FLUX 1          /* J_k on the last edge */
#define CATBAL_SOURCE_INTEGRAL 2    /* sum_{i < nx-1} V_i R_k,i */
#define CATBAL_DEFECT 3             /* sum_{i < nx-1} V_i imbalance_i, accumulated from the imbalances: on exact arithmetic
                                     * WALL_FLUX - BULK_FLUX + SOURCE_INTEGRAL (the sum telescopes) */
#define CATBAL_MAX_IMBALANCE_REL 4  /* max_i |imbalance_i| / scale_i */
#define CATBAL_INVENTORY 5          /* sum_i V_i c_k,i, mol/m^2 */
#define CATBAL_NSCALARS 6

typedef struct catbal_ctx catbal_ctx;

typedef struct catbal_params {
  int32_t struct_size;       /* = sizeof(catbal_params) */
  int32_t max_waves;         /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t nreactions;        /* <= PNP_MAX_REACTIONS; the table of pnp_set_reactions: */
  int32_t n_wall;            /* <= PNP_MAX_WALL_REACTIONS; the table of pnp_set_wall_kinetics / pnp_set_wall_rate_law below */
  const double* D;           /* [N] m^2/s */
  const double* charges;     /* [N] z F */
  const double* mpb_radius;  /* [N] m, NULL or all zero: point ions */
  const double* x;           /* [nx] strictly increasing */
  double beta;               /* 1/(R T) */
  double velocity;           /* convection velocity of pnp_set_convection */
  const int32_t* n_lhs;      /* [nreactions], each <= PNP_MAX_REACTANTS */
  const int32_t* lhs;        /* [nreactions][PNP_MAX_REACTANTS] species indices */
  const int32_t* n_rhs;      /* [nreactions] */
  const int32_t* rhs;        /* [nreactions][PNP_MAX_REACTANTS] */
  const double* kf;          /* [nreactions] */
  const double* kr;          /* [nreactions] */
  const int32_t* species;    /* [n_wall] species whose wall concentration drives the reaction, -1: zeroth order */
  const double* nu;          /* [n_wall][N] stoichiometry of the flux into the domain */
  const double* k;           /* [B][n_wall] rate constants per operating point; required when n_wall > 0 */
  const double* alpha;       /* [n_wall] 1/V, NULL: zeros */
  const double* saturation;  /* [n_wall] m^3/mol, NULL: zeros */
  const double* flux;        /* [B][N] prescribed wall flux into the domain (pnp_set_batch / pnp_set_flux) */
  const double* phiM;        /* [B] electrode potential (pb[b][0] of pnp_set_batch / pnp_set_pb) */
} catbal_params;

/* Any pointer may be NULL: that row is not copied, and not computed where nothing else needs it. */
typedef struct catbal_outputs {
  double* flux;              /* [B][N][nx-1] */
  double* reaction_rate;     /* [B][nreactions][nx] */
  double* source;            /* [B][N][nx] */
  double* wall_rate;         /* [B][n_wall] */
  double* wall_flux;         /* [B][N] */
  double* imbalance;         /* [B][N][nx] */
  double* scalars;           /* [B][N][CATBAL_NSCALARS]: scalars and wall_rate alone move 8 (N CATBAL_NSCALARS + n_wall) bytes per point */
} catbal_outputs;

/* No device call is made before the first catbal_species that passes validation. */
int catbal_create(int32_t device, catbal_ctx** out);
void catbal_destroy(catbal_ctx* ctx);
const char* catbal_last_error(const catbal_ctx* ctx); /* ctx may be NULL: last catbal_create error */
/* Census-form name of the kernel instance the last successful call launched, e.g. "catbal::species_kernel<16, 2, true>"
 * (points per lane, waves per operating point, steric); "" before the first one. */
const char* catbal_last_kernel(const catbal_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catbal_last_kernel_ms(const catbal_ctx* ctx);

/* One pass over the state behind `view` (valid until the next pnp_set_batch / pnp_destroy of its handle).  The kernel and the copies
 * run on view->stream, behind whatever the handle enqueued there, and the call returns when the outputs are on the host.  The state
 * and the status flags of the handle are only read.
 * The tables must be the ones the state was solved with.  After pnp_scf_cycle that is n_wall = 0 and the loop's flux: its solves take
 * the wall reactions through the prescribed flux, not through the wall table, and with the table they would count twice.
 * CATBAL_EINVAL, before any device call: NULL argument, wrong struct_size (view or params), a view without a potential row (compat
 * handle), nx < 3 or > CATBAL_MAX_NX, more than CATBAL_MAX_SPECIES species, x not strictly increasing, a D that is not positive and
 * finite, a charge or velocity that is not finite, a beta that is not positive and finite, a negative or non-finite radius, nreactions or n_wall outside
 * their limits, n_lhs / n_rhs above PNP_MAX_REACTANTS, a species index of the reaction table outside [0, N) or of the wall table
 * outside [-1, N), n_wall > 0 without k, flux or phiM NULL.  Rate constants, fluxes and potentials are taken as they are: a NaN
 * among them shows in the rows of its operating point, as a NaN in the state does. */
int catbal_species(catbal_ctx* ctx, const pnp_device_view* view, const catbal_params* params, const catbal_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_BALANCE_H */
