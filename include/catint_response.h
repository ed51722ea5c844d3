/*
 * catint_response.h -- C-ABI of libcatint_response: the LINEAR RESPONSE of a stationary state of the physical mode (PNP_METHOD_NEWTON),
 * formed ON THE DEVICE from the state a pnp_handle holds there (pnp_get_device_view, catint_pnp.h): how surface potential, surface
 * concentrations, the charge on the metal and the wall fluxes answer a small change of the electrode potential (differential
 * capacitance, slope of the currents) or of a prescribed wall flux, at omega = 0 (the exact tangent) and for harmonic perturbations
 * exp(i omega t) (admittance / impedance spectrum).  One block-tridiagonal solve per (operating point, frequency).  The library shares
 * no code with the Newton kernels: the Jacobian is restated here from the definitions below.
 *
 * Conventions (those of catint_balance.h / catint_equil.h): plain C; every pointer is a HOST pointer to C-contiguous fp64 / int32 / int64
 * owned by the caller (the device pointers live in the pnp_device_view); every entry point returns 0 or a negative CATRESP_E* code and
 * catresp_last_error gives the message; a context is not thread-safe, distinct contexts are independent.  The library reads the view,
 * nothing else.  Complex results are interleaved (re, im) pairs of doubles: the layout of C99 double complex and numpy.complex128.
 *
 * Definitions (the symbols of the solver's discretisation: grid x[nx], reference length dx, edge e between points e and e+1 of length
 * h_e, edge weight w_e = dx / h_e, control volume v_i in units of dx -- (h_{i-1} + h_i) / (2 dx), half cells at both ends; species rows
 * scaled by dx^2 / D_k, the Poisson row by dx^2 / eps; unknowns (c_1 .. c_N, phi) per grid point; q_k = z_k F; psi_k = q_k beta phi + w,
 * w = -ln(1 - phi0), phi0 = N_A sum_k a_k^3 c_k; B(u) = u / (exp(u) - 1), by its series below |u| = 0.05):
 *   residual   F[k, i]  = Jhat_{i+1/2} - Jhat_{i-1/2} - (dx^2 / D_k) v_i R_k(c_i)                                     0 < i < nx-1
 *              F[k, 0]  = Jhat_{1/2} - (flux_k + sum_r nu[r][k] K_r g_r) dx / D_k - (dx^2 / D_k) v_0 R_k(c_0)
 *              Jhat_e   = -w_e ((B(u) + u) c_k[e+1] - B(u) c_k[e]),  u = psi_k[e+1] - psi_k[e] - velocity h_e / D_k
 *              F[phi,i] = w_i (phi_{i+1} - phi_i) - w_{i-1} (phi_i - phi_{i-1}) + (dx^2 / eps) v_i sum_k q_k c_k,i    0 < i < nx-1
 *              F[phi,0] = phi_0 - phiM                                                 (Dirichlet wall)
 *                         w_0 (phi_1 - phi_0) + (dx C_S / eps) (phiM - phi_PZC - phi_0)  (Stern wall)
 *              F[., nx-1] = u - u_bulk (identity rows)
 *              R_k: mass action in activities a = c / (1 - phi0), the table of pnp_set_reactions;
 *              g_r = c_s / (1 + saturation_r c_s) exp(alpha_r (phiM - phi_0)), c_s = c_species[r](0), 1 for species -1
 *   J          = (L, M, U), the block-tridiagonal Jacobian dF/du of this STATIONARY residual at the handle's state, with everything
 *                above: Scharfetter-Gummel fluxes with convection, steric coupling, reactions, Stern or Dirichlet wall, wall table
 *   S          diagonal: (dx^2 / D_k) v_i on the row of species k at points i < nx-1; 0 on every Poisson row and on the bulk rows
 *   system     (J + i omega_f S) du = r for every selected operating point and every omega_f of the list
 *   r, CATRESP_PHIM (d phiM = 1 V): r = -dF/dphiM: r[phi,0] = 1 (Dirichlet) or -dx C_S / eps (Stern);
 *              r[k,0] = sum_r nu[r][k] K_r alpha_r g_r dx / D_k; zero elsewhere
 *   r, CATRESP_WALL_FLUX of species j (d flux_j = 1 mol m^-2 s^-1): r[j,0] = dx / D_j, zero elsewhere (the transport Jacobian
 *              d c_surface / d flux a Newton-type loop around the solver would use)
 * Outputs per (operating point, frequency), complex:
 *   dphi_surface   du[phi, 0]
 *   dc_surface     du[k, 0]                                                                                              [N]
 *   dsigma         response of the charge on the metal.  Stern wall: sigma = C_S (phiM - phi_PZC - phi_0), so C_S (dphiM - du[phi,0]),
 *                  dphiM = 1 for CATRESP_PHIM and 0 for CATRESP_WALL_FLUX.  Dirichlet wall: the half cell of the wall point belongs to
 *                  the electrolyte: -eps (du[phi,1] - du[phi,0]) / h_0 - (h_0 / 2) sum_k q_k du[k,0] (without the second term the
 *                  capacitance is low by the half cell's share of the charge: 2.4 % at h_0 = lambda_D / 20)
 *   dwall_flux     response of the flux into the domain: [WALL_FLUX and k == j]
 *                  + sum_r nu[r][k] K_r (dg_r/dc_s du[s,0] + alpha_r g_r (dphiM - du[phi,0]))                             [N]
 *   admittance     i omega dsigma + sum_k q_k dwall_flux_k, A m^-2 per unit perturbation (the impedance is its reciprocal)
 *   status         0 ok; 1 a non-finite result, or a vanishing or too small pivot (see Solution below); 2 the operating point's solver status was non-zero: the state
 *                  is not a stationary solution, every output of the point is NaN
 *   dc, dphi       optional profiles du[k, i], du[phi, i]
 *
 * The response is defined for a STATIONARY state.  On a handle in the middle of a transient the library still linearises the stationary
 * operator about the state it finds, and the result has no physical meaning; the library cannot tell.
 * The tables must be the ones the state was solved with.  After pnp_scf_cycle the solves took the wall reactions through the prescribed
 * flux, not through the wall table: the response is then formed with n_wall = 0 (the rule of catint_balance.h).
 *
 * Solution: block elimination from the bulk row towards the wall without row exchanges inside a block (Gauss-Jordan on the diagonal
 * block).  Every elimination step is monitored for what partial pivoting would have checked: a pivot that is zero or not finite, or
 * an entry below the pivot whose magnitude exceeds CATRESP_PIVOT_GROWTH_LIMIT (1e8: eight digits lost) times the pivot's, gives
 * status 1 for that system -- the policy of the solver's lane kernels (PIVOT_GROWTH_LIMIT), never a silently wrong number.  The numbers
 * of such a system are returned as computed and must not be used.
 */
#ifndef CATINT_RESPONSE_H
#define CATINT_RESPONSE_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATRESP_OK 0
#define CATRESP_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATRESP_ENOMEM (-2)
#define CATRESP_EDEVICE (-3)  /* HIP runtime error */

#define CATRESP_MAX_SPECIES 8 /* = PNP_NEWTON_MAX_SPECIES */
#define CATRESP_MAX_NX 4098
#define CATRESP_MAX_FREQ 256
#define CATRESP_PIVOT_GROWTH_LIMIT 1e8 /* status 1 when an entry below a pivot exceeds this many times the pivot's magnitude */

#define CATRESP_WALL_DIRICHLET 0
#define CATRESP_WALL_STERN 1

#define CATRESP_PHIM 0        /* perturbation: the electrode potential, 1 V */
#define CATRESP_WALL_FLUX 1   /* perturbation: the prescribed wall flux of species `species`, 1 mol m^-2 s^-1 */

typedef struct catresp_ctx catresp_ctx;

typedef struct catresp_params {
  int32_t struct_size;       /* = sizeof(catresp_params) */
  int32_t max_waves;         /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t wall_bc;           /* CATRESP_WALL_* */
  int32_t perturbation;      /* CATRESP_PHIM / CATRESP_WALL_FLUX */
  int32_t species;           /* CATRESP_WALL_FLUX: the species whose flux is perturbed, in [0, N) */
  int32_t nfreq;             /* 1 .. CATRESP_MAX_FREQ */
  int32_t nreactions;        /* <= PNP_MAX_REACTIONS; the table of pnp_set_reactions: */
  int32_t n_wall;            /* <= PNP_MAX_WALL_REACTIONS; the table of pnp_set_wall_kinetics / pnp_set_wall_rate_law below */
  int64_t nlanes;            /* operating points to answer for; 0 is valid and makes no device call */
  const int64_t* lanes;      /* [nlanes] indices into the handle's batch, repeats allowed; NULL: lanes 0 .. nlanes-1 */
  const double* D;           /* [N] m^2/s */
  const double* charges;     /* [N] z F */
  const double* mpb_radius;  /* [N] m, NULL or all zero: point ions */
  const double* x;           /* [nx] strictly increasing */
  double beta;               /* 1/(R T) */
  double eps;                /* permittivity, F/m */
  double dx;                 /* the solver's reference length of the row scaling */
  double velocity;           /* convection velocity of pnp_set_convection */
  double stern_capacitance;  /* F/m^2, CATRESP_WALL_STERN */
  const int32_t* n_lhs;      /* [nreactions], each <= PNP_MAX_REACTANTS */
  const int32_t* lhs;        /* [nreactions][PNP_MAX_REACTANTS] species indices */
  const int32_t* n_rhs;      /* [nreactions] */
  const int32_t* rhs;        /* [nreactions][PNP_MAX_REACTANTS] */
  const double* kf;          /* [nreactions] */
  const double* kr;          /* [nreactions] */
  const int32_t* wall_species; /* [n_wall] species whose wall concentration drives the reaction, -1: zeroth order (catbal_params.species) */
  const double* nu;          /* [n_wall][N] stoichiometry of the flux into the domain */
  const double* k;           /* [B][n_wall] rate constants per operating point of the handle's batch; required when n_wall > 0 */
  const double* alpha;       /* [n_wall] 1/V, NULL: zeros */
  const double* saturation;  /* [n_wall] m^3/mol, NULL: zeros */
  const double* phiM;        /* [B] electrode potential (pb[b][0] of pnp_set_batch / pnp_set_pb) */
  const double* omega;       /* [nfreq] angular frequencies, rad/s, each >= 0 and finite; shared by all operating points */
} catresp_params;

/* n = nlanes, F = nfreq.  Any pointer may be NULL: that row is not copied, and not computed where nothing else needs it.  The complex
 * rows hold (re, im) pairs: 2 doubles per entry. */
typedef struct catresp_outputs {
  double* dphi_surface;      /* [n][F] complex */
  double* dc_surface;        /* [n][F][N] complex */
  double* dsigma;            /* [n][F] complex, C m^-2 per unit perturbation */
  double* dwall_flux;        /* [n][F][N] complex */
  double* admittance;        /* [n][F] complex */
  int32_t* status;           /* [n][F] */
  double* dc;                /* [n][F][N][nx] complex: with dc or dphi the elimination records go to a device workspace */
  double* dphi;              /* [n][F][nx] complex */
} catresp_outputs;

/* No device call is made before the first catresp_solve that passes validation with nlanes > 0. */
int catresp_create(int32_t device, catresp_ctx** out);
void catresp_destroy(catresp_ctx* ctx);
const char* catresp_last_error(const catresp_ctx* ctx); /* ctx may be NULL: last catresp_create error */
/* Census-form name of the kernel instance the last successful call launched, e.g. "catresp::response_kernel<9, true, false>"
 * (block size N + 1, complex arithmetic, elimination records for profiles); "" before the first one.  A call whose frequencies are
 * all 0 runs the real instance. */
const char* catresp_last_kernel(const catresp_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catresp_last_kernel_ms(const catresp_ctx* ctx);

/* One linear solve per (selected operating point, frequency) about the state behind `view` (valid until the next pnp_set_batch /
 * pnp_destroy of its handle).  The kernel and the copies run on view->stream, behind whatever the handle enqueued there, and the call
 * returns when the outputs are on the host.  The state and the status flags of the handle are only read.
 * Profiles (dc / dphi) keep N+1 x N+1 numbers per grid point and system in a device workspace of at most 2 GiB (the environment
 * variable CATRESP_WORKSPACE_BYTES overrides the cap; at least one wavefront's systems are always resident); a call with more systems
 * than fit walks them in turns.  The results do not depend on the cap or on max_waves.
 * CATRESP_EINVAL, before any device call: NULL argument, wrong struct_size (view or params), a view without a potential row (compat
 * handle), nx < 3 or > CATRESP_MAX_NX, more than CATRESP_MAX_SPECIES species, x not strictly increasing, a D that is not positive and
 * finite, a charge or velocity that is not finite, beta, eps or dx not positive and finite, a negative or non-finite radius, nreactions
 * or n_wall outside their limits, n_lhs / n_rhs above PNP_MAX_REACTANTS, a species index of the reaction table outside [0, N) or of the
 * wall table outside [-1, N), n_wall > 0 without k, phiM or omega NULL, an omega that is negative or not finite, nfreq outside
 * [1, CATRESP_MAX_FREQ], an unknown wall_bc or perturbation, `species` outside [0, N) for CATRESP_WALL_FLUX, a Stern wall without a
 * positive finite capacitance, negative max_waves or nlanes, a lane index outside the batch (or nlanes above it when lanes is NULL).
 * Rate constants and potentials are taken as they are: a NaN among them shows as status 1 of its operating point, as a NaN in the
 * state does. */
int catresp_solve(catresp_ctx* ctx, const pnp_device_view* view, const catresp_params* params, const catresp_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_RESPONSE_H */
