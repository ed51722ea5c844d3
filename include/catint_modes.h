/*
 * catint_modes.h -- C-ABI of libcatint_modes: the RELAXATION MODES of a stationary state of the physical mode, formed ON THE DEVICE from
 * the state a pnp_handle holds there (pnp_get_device_view, catint_pnp.h): the slowest rates at which a small perturbation of the state
 * decays, and with them whether the state is stable.  Per operating point a subspace iteration on A = J^-1 S -- every pass one block
 * elimination with the subspace as right-hand sides at every grid row, a substitution back to the bulk, and the Rayleigh-Ritz matrices
 * of the pass -- all passes inside one launch.  The library shares no code with the Newton kernels.
 *
 * Conventions (those of catint_sens.h): plain C; every pointer is a HOST pointer to C-contiguous fp64 / int32 / int64 owned by the
 * caller (the device pointers live in the pnp_device_view); every entry point returns 0 or a negative CATMODES_E* code and
 * catmodes_last_error gives the message; a context is not thread-safe, distinct contexts are independent.  The library reads the view,
 * nothing else.
 *
 * Definitions.  F, J = (L, M, U) and S are exactly those of catint_response.h: the stationary residual (same symbols, same row
 * scaling: Scharfetter-Gummel fluxes with convection, steric coupling, mass-action reactions in activities, Stern or Dirichlet wall,
 * wall table, identity rows at the bulk point, non-uniform x), its block-tridiagonal Jacobian at the handle's state, and the diagonal
 * storage matrix: (dx^2 / D_k) v_i on the row of species k at points i < nx-1, 0 on every Poisson row and on the bulk rows.  The
 * transient obeys S du/dt + F(u) = 0, so a perturbation decays as exp(-lambda t) with J v = lambda S v: the smallest |lambda| are the
 * relaxation rates, Re lambda < 0 marks an unstable state.  They are the largest eigenvalues theta = 1 / lambda of A = J^-1 S, which
 * is never formed.
 * With a subspace size m = `subspace`, a number of passes K = `iterations` and the start vectors start[m][N+1][nx] (unknown k at
 * grid point i of column j at start[(j (N+1) + k) nx + i]; row N is the potential), per selected operating point:
 *   Q = orth(start)
 *   repeat K times:
 *     solve J W = S Q          m real right-hand sides, non-zero on every species row i < nx-1, zero on Poisson and bulk rows
 *     B = Q^T W       [m][m]
 *     G = (W - Q B)^T (W - Q B)   [m][m]
 *     except after the last pass: Q = orth(W)
 * All inner products are Euclidean over the (N+1) nx entries of a column.  orth is modified Gram-Schmidt with the columns in order, in
 * its right-looking form: for k = 0 .. m-1, with d_kj = <v_k, v_j> taken once column k has been cleared of columns 0 .. k-1,
 * q_k = v_k / sqrt(d_kk) and v_j <- v_j - (d_kj / d_kk) v_k for every j > k.
 * Outputs per selected point:
 *   ritz     B of the last pass, row-major: ritz[a m + b] = <q_a, w_b>                                              [m][m]
 *   gram     G of the last pass (symmetric)                                                                       [m][m]
 *   basis    optional: the Q this B refers to, column j of unknown k at grid point i at [(j (N+1) + k) nx + i]     [m][N+1][nx]
 *   status   0 ok; 1 a failed pivot check (that of catint_response.h, CATMODES_PIVOT_GROWTH_LIMIT) or a non-finite number, in any
 *            pass: the numbers are returned as computed and must not be used; 2 the lane's solver status is non-zero or an input
 *            (phiM or k of the point, any start value) is not finite: every output of the point is NaN; 3 Gram-Schmidt breakdown: in
 *            some orth a column whose norm after projection is at most CATMODES_BREAKDOWN times its norm before (a zero column
 *            included).  Such a column is replaced by zeros and the passes go on with what is left, so every number stays finite;
 *            the outputs are returned as computed and must not be used.  2 goes before 1, and 1 before 3.
 * The small eigenproblem is the caller's: theta, s = eig(B), lambda = 1 / theta; the relative residual of Ritz pair j is
 * sqrt(s_j^H G s_j) / (|theta_j| |s_j|) (the norm of A x - theta x for x = Q s_j, over |theta| |x|); the mode profile is Q s_j.  J is
 * not symmetric: complex pairs are legitimate.
 *
 * Solution: the block elimination of catint_sens.h from the bulk row towards the wall with the m right-hand sides as extra columns
 * of the working block row (width CATMODES_MAX_SUBSPACE; columns beyond m are zero); T_i = D'_i^-1 L_i and the reduced right-hand
 * sides y_i go to a device workspace, and the same lanes substitute du_i = y_i - T_i du_{i-1} from the wall to the bulk.  The
 * elimination is repeated in every pass (nothing of the factorisation but the records of the pass in work is kept).  Inner products
 * and the Gram-Schmidt update are formed by the whole wavefront on one system at a time, each entry by a fixed lane, in a fixed order.
 * The outputs of a point do not depend, bit for bit, on max_waves, on the workspace cap, on the selection of lanes or its order, or on
 * which outputs are asked for.
 *
 * The tables must be the ones the state was solved with.  After pnp_scf_cycle the solves took the wall reactions through the prescribed
 * flux: pass n_wall = 0 (the rule of catint_balance.h).  The modes are defined for a STATIONARY state (catint_response.h).
 */
#ifndef CATINT_MODES_H
#define CATINT_MODES_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATMODES_OK 0
#define CATMODES_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATMODES_ENOMEM (-2)
#define CATMODES_EDEVICE (-3)  /* HIP runtime error */

#define CATMODES_MAX_SPECIES 8 /* = CATRESP_MAX_SPECIES */
#define CATMODES_MAX_NX 4098
#define CATMODES_PIVOT_GROWTH_LIMIT 1e8 /* = CATRESP_PIVOT_GROWTH_LIMIT */
#define CATMODES_MAX_SUBSPACE 8         /* = CATSENS_CHUNK: right-hand sides carried through one elimination */
#define CATMODES_MAX_ITERATIONS 64
#define CATMODES_BREAKDOWN 1e-10        /* status 3 when a column keeps no more than this share of its norm in a Gram-Schmidt */

#define CATMODES_WALL_DIRICHLET 0
#define CATMODES_WALL_STERN 1

typedef struct catmodes_ctx catmodes_ctx;

typedef struct catmodes_params {
  int32_t struct_size;       /* = sizeof(catmodes_params) */
  int32_t max_waves;         /* 0: the library's choice.  Otherwise the size of the persistent grid in wavefronts (tests) */
  int32_t wall_bc;           /* CATMODES_WALL_* */
  int32_t nreactions;        /* <= PNP_MAX_REACTIONS; the table of pnp_set_reactions: */
  int32_t n_wall;            /* <= PNP_MAX_WALL_REACTIONS; the table of pnp_set_wall_kinetics / pnp_set_wall_rate_law below */
  int32_t subspace;          /* m: 1 .. CATMODES_MAX_SUBSPACE, at most N (nx - 1), the rank of S */
  int32_t iterations;        /* K: 1 .. CATMODES_MAX_ITERATIONS */
  int32_t reserved;          /* 0 */
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
  double stern_capacitance;  /* F/m^2, CATMODES_WALL_STERN */
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
  const double* start;       /* [m][N+1][nx] start vectors, shared by all operating points */
} catmodes_params;

/* n = nlanes, m = subspace.  Any pointer may be NULL: that row is not copied.  Rows not asked for are not touched. */
typedef struct catmodes_outputs {
  int32_t struct_size;       /* = sizeof(catmodes_outputs) */
  int32_t reserved;          /* 0 */
  double* ritz;              /* [n][m][m] */
  double* gram;              /* [n][m][m] */
  double* basis;             /* [n][m][N+1][nx] */
  int32_t* status;           /* [n] */
} catmodes_outputs;

/* No device call is made before the first catmodes_solve that passes validation with nlanes > 0. */
int catmodes_create(int32_t device, catmodes_ctx** out);
void catmodes_destroy(catmodes_ctx* ctx);
const char* catmodes_last_error(const catmodes_ctx* ctx); /* ctx may be NULL: last catmodes_create error */
/* Census-form name of the kernel instance the last successful call launched, e.g. "catmodes::modes_kernel<9, 8>" (block size N + 1,
 * carried columns); "" before the first one. */
const char* catmodes_last_kernel(const catmodes_ctx* ctx);
/* Device time of that kernel alone (HIP events around its launch, without the copies), in milliseconds; -1 before the first one. */
float catmodes_last_kernel_ms(const catmodes_ctx* ctx);

/* The subspace iteration of every selected operating point about the state behind `view` (valid until the next pnp_set_batch /
 * pnp_destroy of its handle).  The kernel and the copies run on view->stream, behind whatever the handle enqueued there, and the call
 * returns when the outputs are on the host.  The state, the status flags and the counters of the handle are only read.
 * Per resident system (N+1) nx (N + 17) numbers are kept in a device workspace of at most 2 GiB (the environment variable
 * CATMODES_WORKSPACE_BYTES overrides the cap; at least one wavefront's systems are always resident); a call with more systems than fit
 * walks them in turns.  The results do not depend on the cap or on max_waves.
 * CATMODES_EINVAL, before any device call: everything catsens_solve rejects for the arguments the two share (NULL argument, wrong
 * struct_size of view, params or outputs, a view without a potential row or without a status row, nx < 3 or > CATMODES_MAX_NX, more
 * than CATMODES_MAX_SPECIES species, x not strictly increasing, a D that is not positive and finite, a charge or velocity that is not
 * finite, beta, eps or dx not positive and finite, a negative or non-finite radius, nreactions outside its limits, n_lhs / n_rhs above
 * PNP_MAX_REACTANTS, a species index of the reaction table outside [0, N), an unknown wall_bc, a Stern wall without a positive finite
 * capacitance, negative max_waves or nlanes, a lane index outside the batch or nlanes above it when lanes is NULL, n_wall outside its
 * limits, n_wall > 0 without k, wall_species or nu, a species index of the wall table outside [-1, N), phiM NULL); subspace outside
 * [1, CATMODES_MAX_SUBSPACE] or above N (nx - 1), iterations outside [1, CATMODES_MAX_ITERATIONS], start NULL with nlanes > 0. */
int catmodes_solve(catmodes_ctx* ctx, const pnp_device_view* view, const catmodes_params* params, const catmodes_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_MODES_H */
