/*
 * catint_sens.h -- C-ABI of libcatint_sens: the PARAMETER SENSITIVITIES of a stationary state of the physical mode, formed ON THE DEVICE
 * from the state a pnp_handle holds there (pnp_get_device_view, catint_pnp.h): how the surface state, the charge on the metal and the
 * wall fluxes answer a small change of a MODEL PARAMETER -- a bulk concentration, a diffusion coefficient, a rate constant of a
 * homogeneous or of a wall reaction, the Stern capacitance, the convection velocity -- next to the two controls catint_response.h
 * answers for (the electrode potential, a prescribed wall flux).  The right-hand sides are non-zero at every grid row; they are carried
 * through ONE block elimination per chunk of parameters.  The library shares no code with the Newton kernels.
 *
 * Conventions (those of catint_couple.h): plain C; every pointer is a HOST pointer to C-contiguous fp64 / int32 / int64 owned by the
 * caller (the device pointers live in the pnp_device_view); every entry point returns 0 or a negative CATSENS_E* code and
 * catsens_last_error gives the message; a context is not thread-safe, distinct contexts are independent.  The library reads the view,
 * nothing else.
 *
 * Definitions.  F(u; p) = 0 is the stationary residual of catint_response.h (same symbols, same row scaling: Scharfetter-Gummel fluxes
 * with convection, steric coupling, mass-action reactions in activities, Stern or Dirichlet wall, wall table, identity rows at the bulk
 * point) and J = dF/du its block-tridiagonal Jacobian.  Per selected operating point and per parameter p_m of the call
 *   J du = r_m,   r_m = -dF/dp_m   at the handle's state.
 * r is zero wherever not listed; rows i < nx-1 unless said otherwise; h_e the length of edge e, Ju_e = dJhat_e/du; a_f,r and a_b,r the
 * unit-rate activity products gamma^m prod c of the two sides of reaction r, net[r][k] = n_rhs(k, r) - n_lhs(k, r); g_r as in
 * catint_response.h; R_k = sum_r net[r][k] (kf_r a_f,r - kr_r a_b,r).
 *   CATSENS_PHIM                as CATRESP_PHIM
 *   CATSENS_WALL_FLUX j         r[j,0] = dx / D_j (as CATRESP_WALL_FLUX)
 *   CATSENS_BULK_CONCENTRATION j  r[j,nx-1] = 1 (the identity row c - c_bulk)
 *   CATSENS_DIFFUSION j         rows of species j only.  Interior: -Ju_{i+1/2} s_i + Ju_{i-1/2} s_{i-1} - (dx^2 / D_j^2) v_i R_j(c_i),
 *                               s_e = velocity h_e / D_j^2.  Wall: -Ju_{1/2} s_0 - (flux_j + sum_r nu[r][j] K_r g_r) dx / D_j^2
 *                               - (dx^2 / D_j^2) v_0 R_j(c_0)
 *   CATSENS_RATE_FORWARD r      r[k,i] = +(dx^2 / D_k) v_i net[r][k] a_f,r(c_i): the derivative by the unit-rate product, so also
 *                               defined at kf = 0
 *   CATSENS_RATE_BACKWARD r     r[k,i] = -(dx^2 / D_k) v_i net[r][k] a_b,r(c_i)
 *   CATSENS_WALL_RATE r         r[k,0] = nu[r][k] g_r dx / D_k: with respect to the lane's own k[b][r]
 *   CATSENS_STERN_CAPACITANCE   r[phi,0] = -(dx / eps) (phiM - phi_PZC - phi_0); Stern wall only
 *   CATSENS_VELOCITY            r[k,i] = (Ju_{i+1/2} h_i - Ju_{i-1/2} h_{i-1}) / D_k; wall: Ju_{1/2} h_0 / D_k
 * Outputs per (selected point, parameter), real:
 *   dphi_surface   du[phi, 0]
 *   dc_surface     du[k, 0]                                                                                           [N]
 *   dsigma         the formula of catint_response.h for both walls (dphiM = 1 for CATSENS_PHIM, else 0); for
 *                  CATSENS_STERN_CAPACITANCE the explicit term (phiM - phi_PZC - phi_0) is added.  The Dirichlet form takes
 *                  du[phi, 1] from one step of back-substitution: T_1 and the reduced right-hand side of row 1 are kept, nothing else
 *   dwall_flux     total derivative of the flux into the domain: the explicit part ([k == j] for WALL_FLUX, nu[r][k] g_r for
 *                  WALL_RATE, the alpha g term for PHIM) and the wall table's answer to du[., 0]                     [N]
 *   dcurrent       sum_k q_k dwall_flux_k, A m^-2 per unit of the parameter
 *   status         per selected point: 0 ok; 1 a failed pivot check (that of catint_response.h, CATSENS_PIVOT_GROWTH_LIMIT) or a
 *                  non-finite number, in any chunk or column: the numbers are returned as computed and must not be used; 2 the
 *                  lane's solver status is non-zero or an input of the point (flux, k, phiM) is not finite: every output of the
 *                  point is NaN.  (2 goes before 1.)
 *
 * Solution: the block elimination of catint_couple.h from the bulk row towards the wall with the right-hand sides as extra columns
 * of the working block row: after the Gauss-Jordan of row i they hold y_i = D'_i^-1 g'_i, and g'_{i-1} = r_{i-1} - U_{i-1} y_i; the
 * walk starts from y_{nx-1} = r_{nx-1}, and at the wall the extra columns hold du_0.  Parameters are walked in chunks of
 * CATSENS_CHUNK columns, one elimination per chunk; the columns of a last partial chunk beyond nparams are zero right-hand sides.
 * Nothing is kept between block rows.  The numbers of a parameter do not depend, bit for bit, on which other parameters are in
 * the call, on its position in the list, on max_waves, on the selection of lanes or on which outputs are asked for.
 *
 * The tables must be the ones the state was solved with, `flux` the prescribed wall fluxes it was solved with.  After pnp_scf_cycle
 * the solves took the wall reactions through the prescribed flux: pass n_wall = 0 (the rule of catint_balance.h).
 */
#ifndef CATINT_SENS_H
#define CATINT_SENS_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATSENS_OK 0
#define CATSENS_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATSENS_ENOMEM (-2)
#define CATSENS_EDEVICE (-3)  /* HIP runtime error */

#define CATSENS_MAX_SPECIES 8 /* = CATRESP_MAX_SPECIES */
#define CATSENS_MAX_NX 4098
#define CATSENS_PIVOT_GROWTH_LIMIT 1e8 /* = CATRESP_PIVOT_GROWTH_LIMIT */
#define CATSENS_MAX_PARAMS 64
#define CATSENS_CHUNK 8       /* right-hand sides carried through one elimination */

#define CATSENS_WALL_DIRICHLET 0
#define CATSENS_WALL_STERN 1

/* kinds of parameter; `index` names the species, reaction or wall reaction where there is one */
#define CATSENS_PHIM 0
#define CATSENS_WALL_FLUX 1
#define CATSENS_BULK_CONCENTRATION 2
#define CATSENS_DIFFUSION 3
#define CATSENS_RATE_FORWARD 4
#define CATSENS_RATE_BACKWARD 5
#define CATSENS_WALL_RATE 6
#define CATSENS_STERN_CAPACITANCE 7
#define CATSENS_VELOCITY 8
#define CATSENS_NKINDS 9

typedef struct catsens_ctx catsens_ctx;

typedef struct catsens_params {
  int32_t struct_size;       /* = sizeof(catsens_params) */
  int32_t max_waves;         /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t wall_bc;           /* CATSENS_WALL_* */
  int32_t nreactions;        /* <= PNP_MAX_REACTIONS; the table of pnp_set_reactions: */
  int32_t n_wall;            /* <= PNP_MAX_WALL_REACTIONS; the table of pnp_set_wall_kinetics / pnp_set_wall_rate_law below */
  int32_t nparams;           /* P: 1 .. CATSENS_MAX_PARAMS */
  int64_t nlanes;            /* n: operating points to answer for; 0 is valid and makes no device call */
  const int64_t* lanes;      /* [n] indices into the handle's batch, repeats allowed; NULL: lanes 0 .. n-1 */
  const double* D;           /* [N] m^2/s */
  const double* charges;     /* [N] z F */
  const double* mpb_radius;  /* [N] m, NULL or all zero: point ions */
  const double* x;           /* [nx] strictly increasing */
  double beta;               /* 1/(R T) */
  double eps;                /* permittivity, F/m */
  double dx;                 /* the solver's reference length of the row scaling */
  double velocity;           /* convection velocity of pnp_set_convection */
  double stern_capacitance;  /* F/m^2, CATSENS_WALL_STERN */
  double phi_pzc;            /* V, finite */
  const int32_t* n_lhs;      /* [nreactions], each <= PNP_MAX_REACTANTS */
  const int32_t* lhs;        /* [nreactions][PNP_MAX_REACTANTS] species indices */
  const int32_t* n_rhs;      /* [nreactions] */
  const int32_t* rhs;        /* [nreactions][PNP_MAX_REACTANTS] */
  const double* kf;          /* [nreactions] */
  const double* kr;          /* [nreactions] */
  const int32_t* wall_species; /* [n_wall] species whose wall concentration drives the reaction, -1: zeroth order */
  const double* nu;          /* [n_wall][N] stoichiometry of the flux into the domain */
  const double* k;           /* [B][n_wall] rate constants per operating point of the handle's batch; required when n_wall > 0 */
  const double* alpha;       /* [n_wall] 1/V, NULL: zeros */
  const double* saturation;  /* [n_wall] m^3/mol, NULL: zeros */
  const double* phiM;        /* [B] electrode potential (pb[b][0] of pnp_set_batch / pnp_set_pb) */
  const double* flux;        /* [n][N] the prescribed wall fluxes the state was solved with, by the position in the call */
  const int32_t* kind;       /* [P] CATSENS_* kinds */
  const int32_t* index;      /* [P] species / reaction / wall reaction; ignored for kinds without one */
} catsens_params;

/* n = nlanes, P = nparams.  Any pointer may be NULL: that row is not copied.  Rows not asked for are not touched. */
typedef struct catsens_outputs {
  int32_t struct_size;       /* = sizeof(catsens_outputs) */
  int32_t reserved;          /* 0 */
  double* dphi_surface;      /* [n][P] */
  double* dc_surface;        /* [n][P][N] */
  double* dsigma;            /* [n][P] C m^-2 per unit of the parameter */
  double* dwall_flux;        /* [n][P][N] */
  double* dcurrent;          /* [n][P] */
  int32_t* status;           /* [n] */
} catsens_outputs;

/* No device call is made before the first catsens_solve that passes validation with nlanes > 0. */
int catsens_create(int32_t device, catsens_ctx** out);
void catsens_destroy(catsens_ctx* ctx);
const char* catsens_last_error(const catsens_ctx* ctx); /* ctx may be NULL: last catsens_create error */
/* Census-form name of the kernel instance the last successful call launched, e.g. "catsens::sens_kernel<9, 8>" (block size N + 1,
 * chunk width); "" before the first one. */
const char* catsens_last_kernel(const catsens_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catsens_last_kernel_ms(const catsens_ctx* ctx);

/* The sensitivities of every selected operating point to every parameter of the list, about the state behind `view` (valid until the
 * next pnp_set_batch / pnp_destroy of its handle).  The kernel and the copies run on view->stream, behind whatever the handle enqueued
 * there, and the call returns when the outputs are on the host.  The state, the status flags and the counters of the handle are only
 * read.  There is no workspace.
 * CATSENS_EINVAL, before any device call: everything catcpl_solve rejects for the arguments the two share (NULL argument, wrong
 * struct_size of view, params or outputs, a view without a potential row or without a status row, nx < 3 or > CATSENS_MAX_NX, more
 * than CATSENS_MAX_SPECIES species, x not strictly increasing, a D that is not positive and finite, a charge or velocity that is not
 * finite, beta, eps or dx not positive and finite, a negative or non-finite radius, nreactions outside its limits, n_lhs / n_rhs above
 * PNP_MAX_REACTANTS, a species index of the reaction table outside [0, N), an unknown wall_bc, a Stern wall without a positive finite
 * capacitance, negative max_waves or nlanes, a lane index outside the batch or nlanes above it when lanes is NULL); n_wall outside
 * its limits, n_wall > 0 without k, wall_species or nu, a species index of the wall table outside [-1, N), phiM NULL; nparams outside
 * [1, CATSENS_MAX_PARAMS], kind or index NULL, an unknown kind, an index outside its table (species outside [0, N), reaction outside
 * [0, nreactions), wall reaction outside [0, n_wall)), CATSENS_STERN_CAPACITANCE on a Dirichlet wall, flux NULL with nlanes > 0, a
 * phi_pzc that is not finite. */
int catsens_solve(catsens_ctx* ctx, const pnp_device_view* view, const catsens_params* params, const catsens_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_SENS_H */
