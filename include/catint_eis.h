/*
 * catint_eis.h -- C-ABI of libcatint_eis: the SMALL-SIGNAL RESPONSE OF THE MICROKINETIC ELECTRODE at angular frequency omega, for a batch
 * of operating points and a list of frequencies, formed ON THE DEVICE.  It joins what the other libraries keep apart: the linearised
 * surface microkinetics with adsorbate storage i omega theta (the model of catint_kinetics.h), the transport transfer functions of the
 * electrolyte at the same omega (the operator of catint_response.h with n_wall = 0), and the Stern layer.  The result is the
 * admittance of the working electrode: charge-transfer resistance, adsorption pseudo-capacitance and the diffusion branch fed by the
 * reaction (Armstrong-Henderson, Harrington-Conway).  At omega = 0 it is the slope of the polarisation curve of the coupled
 * electrode.
 *
 * Conventions (those of catint_kinetics.h / catint_response.h): plain C; every pointer is a HOST pointer to C-contiguous fp64 / int32 /
 * int64 owned by the caller; every entry point returns 0 or a negative CATEIS_E* code and cateis_last_error gives the message; a
 * context is not thread-safe, distinct contexts are independent.  Complex numbers are interleaved (re, im) doubles.  The view is read,
 * never written.
 *
 * Assumptions.  Adsorbates carry no charge of their own, so the current is sum_k q_k flux_k at every frequency.  C_S is constant.  The
 * state must be STATIONARY and solved with PRESCRIBED wall fluxes (no wall table); the library cannot tell.
 *
 * The kinetic half (cateis_kinetic; the first stage of cateis_solve).  Per operating point, with y = ln theta, the rates rf, rb, the
 * orders, m, Jraw_st = sum_r m[r][s] (rf_r order_f[r][N+t] - rb_r order_b[r][N+t]), G_s = sum_r m[r][s] (rf_r - rb_r) and the row
 * scales D_s exactly as catint_kinetics.h defines them, at the GIVEN coverages theta[n][S+1] (clamped as a theta_guess is):
 *   A(omega)_st = (Jraw_st - i omega theta_s delta_st) / D_s for s = 1 .. S;  A_0t = n_t theta_t;  a row with D_s = 0 is the identity
 *   row with a zero right-hand side.
 *   parameters p in {c_j(0), j < N;  phi_M at fixed phi_0;  phi_0 at fixed phi_M}.  For each, A(omega) dy/dp = -(dG_s/dp) / D_s (row 0:
 *   0), then dflux_k/dp = dflux_k/dp|_y + site_density sum_r nu[r][k] sum_t (rf_r order_f[r][N+t] - rb_r order_b[r][N+t]) dy_t/dp.
 *   The derivative conventions are those of catkin_solve: sigma (when given), off and gamma are constants; d/dc_j is the product with
 *   one factor left out and is zero where c_j < 0 was clamped.
 *   A(omega) is factorised with partial row pivoting (the pivot chosen by |.|^2), once per (point, omega); the N + 2 right-hand sides
 *   go through one after another.
 *   Kc[n][F][N][N] = dflux_k/dc_j;  Kphi[n][F][N][2] = d/dphi_M, d/dphi_0;  dy[n][F][S+1][N+2];  residual[n] = max_s |G_s| / D_s.
 *
 * The coupled electrode (cateis_solve).  J, S: the Jacobian and the storage matrix of catint_response.h with n_wall = 0 (Stern wall).
 *   transport  block elimination of J + i omega S from the bulk to the wall, then Gauss-Jordan on [W(omega) | E | r_phi] with
 *              E = diag(dx / D_k) (the Poisson row zero) and r_phi the phi_M column (-dx C_S / eps in the Poisson row):
 *              T_c(omega)[k][j] = d c_k(0) / d flux_j, T_phi(omega)[j] = d phi_0 / d flux_j, t_c(omega)[k] = d c_k(0) / d phi_M and
 *              t_phi(omega) = d phi_0 / d phi_M, both at fixed fluxes
 *   closure    A = I - rf (Kc T_c + Kphi0 (x) T_phi),  b = rf (KphiM + Kc t_c + Kphi0 t_phi),  A dflux = b by Gauss-Jordan with partial
 *              row pivoting; a pivot that is zero, not finite or below CATEIS_SINGULAR times the largest magnitude among the entries
 *              of A and the two terms each is the difference of gives status 3 (the rule of catint_couple.h)
 *   results    dc_surface = T_c dflux + t_c;  dphi_surface = T_phi . dflux + t_phi;  dsigma = C_S (1 - dphi_surface);
 *              faradaic = sum_k q_k dflux_k;  double_layer = i omega dsigma;  admittance = double_layer + faradaic, in A m^-2 V^-1, the
 *              convention of catresp_outputs.admittance.  rf = 0 is the blocking electrode
 *   omega = 0 runs the same code; every imaginary part then is an exact zero.
 *
 * status[n][F]: 0 ok
 *               1 a non-finite number or a failed pivot check in the transport elimination (CATEIS_PIVOT_GROWTH_LIMIT, the check of
 *                 catint_response.h)
 *               2 the lane's solver status is non-zero or an input of the point is not finite: every output of the point is NaN, other
 *                 points are unaffected
 *               3 a zero or non-finite pivot of A(omega), kinetic or coupled (coupled: also the CATEIS_SINGULAR rule)
 *               4 residual > residual_tol: the coverages are not stationary; the numbers are returned as computed
 *               (2 goes before 1, 1 before 3, 3 before 4.)
 *
 * Work is done in turns of at most as many (point, omega) pairs as the workspace holds (2 GiB; the environment variable
 * CATEIS_WORKSPACE_BYTES overrides, never below one wavefront's 64 pairs).  The results do not depend on the cap, on max_waves, on the
 * position in the batch, on which outputs were asked for, or on the other frequencies of the list.
 */
#ifndef CATINT_EIS_H
#define CATINT_EIS_H

#include <stdint.h>

#include "catint_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CATEIS_OK 0
#define CATEIS_EINVAL (-1)   /* bad argument: reported before any device call */
#define CATEIS_ENOMEM (-2)
#define CATEIS_EDEVICE (-3)  /* HIP runtime error */

#define CATEIS_MAX_SPECIES 8
#define CATEIS_MAX_ADSORBATES 8
#define CATEIS_MAX_STEPS 16
#define CATEIS_MAX_NX 4098
#define CATEIS_MAX_FREQ 256
#define CATEIS_PIVOT_GROWTH_LIMIT 1e8
#define CATEIS_SINGULAR 1e-12

#define CATEIS_WALL_DIRICHLET 0  /* refused */
#define CATEIS_WALL_STERN 1

#define CATEIS_STATUS_OK 0
#define CATEIS_STATUS_PIVOT 1
#define CATEIS_STATUS_INPUT 2
#define CATEIS_STATUS_SINGULAR 3
#define CATEIS_STATUS_RESIDUAL 4

typedef struct cateis_ctx cateis_ctx;

typedef struct cateis_params {
  int32_t struct_size;        /* = sizeof(cateis_params) */
  int32_t max_waves;          /* 0: the library's choice.  Otherwise the size of the persistent grids in wavefronts (tests) */
  int32_t nspecies;           /* N; the view's on the view path */
  int32_t nadsorbates;        /* S, 1 .. CATEIS_MAX_ADSORBATES */
  int32_t nsteps;             /* R, 1 .. CATEIS_MAX_STEPS */
  int32_t potential_drop;     /* w of catkin_params */
  int32_t nfreq;              /* F, 1 .. CATEIS_MAX_FREQ */
  int32_t wall_bc;            /* cateis_solve: CATEIS_WALL_STERN */
  int32_t nreactions;         /* cateis_solve: the table of pnp_set_reactions */
  int32_t reserved;
  int64_t n;                  /* operating points; 0 is valid and makes no device call */
  const int64_t* lanes;       /* view path: [n] indices into the handle's batch, repeats allowed; NULL: 0 .. n-1 */
  /* the microkinetic model: catkin_params */
  const int32_t* order_f;     /* [R][N+S+1] */
  const int32_t* order_b;     /* [R][N+S+1] */
  const double* nu;           /* [R][N] */
  const double* cref;         /* [N] */
  const double* site_count;   /* [S+1] */
  const double* dG;           /* [R][4] */
  const double* Ea;           /* [R][4] */
  const double* lnA;          /* [R] */
  double site_density;        /* mol/m^2 */
  double stern_capacitance;   /* C_S, F/m^2: the surface charge when sigma is NULL, and the Stern wall of cateis_solve */
  double phi_pzc;             /* V */
  const double* phiM;         /* [n] */
  const double* sigma;        /* [n], or NULL */
  const double* off;          /* [n][R][2], or NULL */
  const double* gamma;        /* [n][N], or NULL */
  const double* theta;        /* [n][S+1]: the stationary coverages, required */
  const double* csurf;        /* cateis_kinetic: [n][N], or NULL: the view */
  const double* phi_surface;  /* cateis_kinetic: [n], or NULL: the view */
  const double* omega;        /* [F] rad/s, each finite and >= 0 */
  double residual_tol;        /* >= 0 and finite */
  /* the medium of cateis_solve: catcpl_params */
  const double* D;            /* [N] */
  const double* charges;      /* [N] */
  const double* mpb_radius;   /* [N], or NULL */
  const double* x;            /* [nx] */
  double beta, eps, dx, velocity;
  const int32_t* n_lhs;       /* [nreactions] */
  const int32_t* lhs;         /* [nreactions][PNP_MAX_REACTANTS] */
  const int32_t* n_rhs;
  const int32_t* rhs;
  const double* kf;
  const double* kr;
  double rf;                  /* roughness factor, >= 0 and finite; 0: the blocking electrode */
} cateis_params;

/* n points, F frequencies.  Complex rows hold (re, im) pairs.  Any pointer may be NULL: that row is not copied. */
typedef struct cateis_outputs {
  int32_t struct_size;        /* = sizeof(cateis_outputs) */
  int32_t reserved;
  double* Kc;                 /* [n][F][N][N] complex */
  double* Kphi;               /* [n][F][N][2] complex */
  double* dy;                 /* [n][F][S+1][N+2] complex */
  double* residual;           /* [n] real */
  int32_t* status;            /* [n][F] */
  /* cateis_solve only (cateis_kinetic ignores them): */
  double* admittance;         /* [n][F] complex */
  double* faradaic;           /* [n][F] */
  double* double_layer;       /* [n][F] */
  double* dflux;              /* [n][F][N] */
  double* dc_surface;         /* [n][F][N] */
  double* dphi_surface;       /* [n][F] */
  double* dsigma;             /* [n][F] */
  double* Tc;                 /* [n][F][N][N] */
  double* Tphi;               /* [n][F][N] */
  double* tc;                 /* [n][F][N] */
  double* tphi;               /* [n][F] */
} cateis_outputs;

/* No device call is made before the first solving call that passes validation with n > 0 and an output asked for. */
int cateis_create(int32_t device, cateis_ctx** out);
void cateis_destroy(cateis_ctx* ctx);
const char* cateis_last_error(const cateis_ctx* ctx); /* ctx may be NULL: last cateis_create error */
/* Census-form name of the last kernel the last successful call launched ("cateis::kinetic_kernel", "cateis::electrode_kernel<9>");
 * "" before the first one. */
const char* cateis_last_kernel(const cateis_ctx* ctx);
/* Device time of the kernels of that call alone (HIP events around the launches of every turn, without the copies), in milliseconds;
 * -1 before the first one. */
float cateis_last_kernel_ms(const cateis_ctx* ctx);

/* The intrinsic kinetic admittance at a fixed surface state.  view may be NULL when csurf and phi_surface are given.
 * CATEIS_EINVAL, before any device call: everything catkin_solve rejects for the same members, a missing theta or omega, nfreq outside
 * [1, CATEIS_MAX_FREQ], an omega that is negative or not finite, a residual_tol that is negative or not finite. */
int cateis_kinetic(cateis_ctx* ctx, const pnp_device_view* view, const cateis_params* params, const cateis_outputs* out);

/* The coupled electrode about the state behind `view`; both kernels run on view->stream, the second reads what the first wrote on the
 * device.  CATEIS_EINVAL, before any device call: everything above, everything catcpl_solve rejects for the medium, a host surface
 * state (csurf / phi_surface), a wall that is not CATEIS_WALL_STERN, an rf that is negative or not finite. */
int cateis_solve(cateis_ctx* ctx, const pnp_device_view* view, const cateis_params* params, const cateis_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* CATINT_EIS_H */
