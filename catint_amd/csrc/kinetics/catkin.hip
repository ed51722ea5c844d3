// libcatint_kinetics (include/catint_kinetics.h): the steady state of a mean-field surface microkinetic model per operating point --
// damped Newton in the log-coverages with row-scaled residuals -- and the wall fluxes and their sensitivities that follow from it.
// gfx950 / MI355X only.
//
// Mapping, working set, tables and arithmetic: ../pnp_kin.h, which also holds the rates, the rows, the LU and the host code this
// library shares with drc/catdrc.hip, and the Newton iteration and the flux sums it shares with scfkin/catscfkin.hip.  Here the only divergence besides the pivot row is the iteration count (a finished lane idles:
// its unknowns stop changing).  LDS slots: J[T][T] (or N slots, whichever is more), y[T], the right-hand side [T], the row scales D[T],
// the activities a[N] and N accumulators.  At S = 8, N = 8: 124 slots x 512 B = 62 KB per wave.
#include "../../../include/catint_kinetics.h"
#include "../pnp_kin.h"

#pragma clang fp contract(off)

namespace catkin {

using namespace pnp::kin;

struct KArgs {
  int32_t N, S, R, maxit, w, use_sigma, sens, from_view, ldx, pad_;
  int64_t n;
  const double* c;         // view: [B][N][ldx]
  const double* phi;       // view: [B][ldx]
  const int32_t* st;       // view: [B] solver status
  const int64_t* lanes;    // [n]
  const double *cs, *phis; // host surface state: [n][N], [n]
  const double *phiM, *sigma, *off, *gamma, *guess;   // [n], [n], [n][R][2], [n][N], [n][T]; null: absent
  double *theta, *rate, *gross, *flux, *fscale, *dfdc, *dfdphi;   // device rows; null: not wanted
  int32_t *status, *iters;
  double sd, tol, CS, pzc;
};

using Lane = SteadyLane;

__global__ __launch_bounds__(64) void steady_kernel(const KArgs A, const Table* __restrict__ tab) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1, R = A.R;
  const Table& tb = *tab;   // its own read-only argument: the uniform reads become scalar loads
  Lane ln;
  steady_slots(ln, lds, lane, N, T);
  double* L = ln.L;
  const double bad_number = __builtin_nan("");

  for (int64_t grp = blockIdx.x; grp * 64 < A.n; grp += gridDim.x) {
    const bool live = grp * 64 + lane < A.n;
    const int64_t i = live ? grp * 64 + lane : A.n - 1;
    const int64_t b = A.lanes[i];
    ln.pt = point_inputs(A, tb, i, b, ln.at(ln.oA));
    bool ok = ln.pt.ok;
    // ---- start ----
    double nsum = 0.0;
    for (int t = 0; t < T; ++t) nsum = nsum + tb.ns[t];
    const double y0 = log(1.0 / nsum);
    if (A.guess)
      for (int t = 0; t < T; ++t) ok = ok && finite_(A.guess[i * T + t]);
    for (int t = 0; t < T; ++t) L[(ln.oY + t) * 64] = A.guess && ok ? log_coverage(A.guess[i * T + t]) : y0;
    // ---- Newton ----
    int it;
    uint64_t pivs;
    int status = steady_newton(A, tb, ln, ok ? CATKIN_MAXIT : CATKIN_INPUT, ok && live, it, pivs);
    const bool nan = status == CATKIN_INPUT;

    // ---- coverages, rates, fluxes at the lane's y (the J slots are free: N of them hold flux_scale) ----
    if (A.theta && live)
      for (int t = 0; t < T; ++t) A.theta[i * T + t] = nan ? bad_number : exp(L[(ln.oY + t) * 64]);
    if (A.rate || A.gross || A.flux || A.fscale) {
      steady_fluxes(A, tb, ln, [&](int r, double net, double gross) {
        if (A.rate && live) A.rate[i * R + r] = nan ? bad_number : net;
        if (A.gross && live) A.gross[i * R + r] = nan ? bad_number : gross;
      });
      for (int k = 0; k < N; ++k) {
        if (A.flux && live) A.flux[i * N + k] = nan ? bad_number : A.sd * L[(ln.oC + k) * 64];
        if (A.fscale && live) A.fscale[i * N + k] = nan ? bad_number : A.sd * L[(ln.oJ + k) * 64];
      }
    }

    // ---- sensitivities: J at the lane's y factorised once, one right-hand side after another ----
    if (A.sens) {
      steady_assemble(A, tb, ln);
      const bool bad = factor(ln.at(ln.oJ), T, pivs);
      if (bad && status != CATKIN_INPUT) status = CATKIN_PIVOT;
      const int first = A.dfdc ? 0 : N, last = A.dfdphi ? N + 2 : N;
      for (int p = first; p < last; ++p) {
        // p < N: d/dc_p;  N: d/dphiM at fixed phi_0;  N + 1: d/dphi_0 at fixed phiM
        double dV = 0.0, ds = 0.0, dadc = 0.0;
        if (p == N) dV = 1.0, ds = A.use_sigma ? 0.0 : A.CS;
        else if (p == N + 1) dV = A.w ? -1.0 : 0.0, ds = A.use_sigma ? 0.0 : -A.CS;
        else {
          const double c = A.from_view ? A.c[((size_t)b * N + p) * A.ldx] : A.cs[i * N + p];
          const double g = A.gamma ? A.gamma[i * N + p] : 1.0;
          dadc = c >= 0.0 ? g / tb.cref[p] : 0.0;
        }
        for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0;
        for (int k = 0; k < N; ++k) L[(ln.oC + k) * 64] = 0.0;
        for (int r = 0; r < R; ++r) {
          double ef, eb, pf, pb, drf, drb;
          int br;
          if (p < N) {
            const int of = tb.of[r][p], ob = tb.ob[r][p];
            if (of == 0 && ob == 0) continue;
            steady_rates(A, tb, ln, r, p, br, ef, eb, pf, pb);
            drf = of ? ef * ((double)of * pf * dadc) : 0.0;
            drb = ob ? eb * ((double)ob * pb * dadc) : 0.0;
          } else {
            double dlf, dlb;
            steady_rates(A, tb, ln, r, -1, br, ef, eb, pf, pb);
            rate_constant_slopes(tb, ln.pt.sg, r, br, dV, ds, dlf, dlb);
            drf = (ef * pf) * dlf;
            drb = (eb * pb) * dlb;
          }
          const double dnet = drf - drb;
          for (int s = 1; s < T; ++s) {
            const int m = tb.ob[r][N + s] - tb.of[r][N + s];
            if (m) L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + (double)m * dnet;
          }
          for (int k = 0; k < N; ++k) {
            const double nu = tb.nu[r][k];
            if (nu != 0.0) L[(ln.oC + k) * 64] = L[(ln.oC + k) * 64] + nu * dnet;
          }
        }
        for (int s = 1; s < T; ++s) {
          const double D = L[(ln.oD + s) * 64];
          L[(ln.oB + s) * 64] = D == 0.0 ? 0.0 : -(L[(ln.oB + s) * 64] / D);
        }
        substitute(ln.at(ln.oJ), ln.at(ln.oB), T, pivs);
        for (int r = 0; r < R; ++r) {
          double ef, eb, pf, pb;
          int br;
          steady_rates(A, tb, ln, r, -1, br, ef, eb, pf, pb);
          const double rf = ef * pf, rb = eb * pb;
          double ws = 0.0;
          for (int t = 0; t < T; ++t) {
            const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
            if (of | ob) ws = ws + (rf * (double)of - rb * (double)ob) * L[(ln.oB + t) * 64];
          }
          for (int k = 0; k < N; ++k) {
            const double nu = tb.nu[r][k];
            if (nu != 0.0) L[(ln.oC + k) * 64] = L[(ln.oC + k) * 64] + nu * ws;
          }
        }
        if (live)
          for (int k = 0; k < N; ++k) {
            const double v = nan ? bad_number : A.sd * L[(ln.oC + k) * 64];
            if (p < N) A.dfdc[((size_t)i * N + k) * N + p] = v;
            else A.dfdphi[((size_t)i * N + k) * 2 + (p - N)] = v;
          }
      }
    }
    if (live) {
      if (A.status) A.status[i] = status;
      if (A.iters) A.iters[i] = it;
    }
  }
}

static size_t lds_bytes(int N, int S) {
  const int T = S + 1;
  return (size_t)(std::max(T * T, N) + 3 * T + 2 * N) * 64 * sizeof(double);
}

}  // namespace catkin

static_assert(CATKIN_OK == pnp::post::OK && CATKIN_EINVAL == pnp::post::ERR_INVAL && CATKIN_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATKIN_EDEVICE == pnp::post::ERR_DEVICE && CATKIN_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_kinetics.h and pnp_post.h disagree");
static_assert(CATKIN_CONVERGED == pnp::kin::STATUS_CONVERGED && CATKIN_MAXIT == pnp::kin::STATUS_MAXIT && CATKIN_INPUT == pnp::kin::STATUS_INPUT &&
                  CATKIN_PIVOT == pnp::kin::STATUS_PIVOT,
              "catint_kinetics.h and pnp_kin.h disagree");
static_assert(CATKIN_MAX_SPECIES == pnp::kin::MAXN && CATKIN_MAX_ADSORBATES == pnp::kin::MAXS && CATKIN_MAX_STEPS == pnp::kin::MAXR &&
                  CATKIN_MAX_ORDER == pnp::kin::MAX_ORDER && CATKIN_MIN_LOG == pnp::kin::MINLOG && CATKIN_DROP_FULL == pnp::kin::DROP_FULL &&
                  CATKIN_DROP_STERN == pnp::kin::DROP_STERN,
              "catint_kinetics.h and pnp_kin.h disagree");

struct catkin_ctx : pnp::post::Ctx {};

extern "C" {

int catkin_create(int32_t device, catkin_ctx** out) { return pnp::post::create("catkin_create", device, out); }
void catkin_destroy(catkin_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catkin_last_error(const catkin_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catkin_last_kernel(const catkin_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catkin_last_kernel_ms(const catkin_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catkin_solve(catkin_ctx* ctx, const pnp_device_view* view, const catkin_params* p, const catkin_outputs* out) {
  using namespace catkin;
  static const char entry[] = "catkin_solve";
  if (const int rc = check_sizes(ctx, entry, "catkin_params", "catkin_outputs", p, out)) return rc;
  if (p->maxit < 1) return fail(ctx, CATKIN_EINVAL, "catkin_solve: maxit < 1");
  if (const int rc = check_drop(ctx, entry, p)) return rc;
  if (!posfin(p->tol)) return fail(ctx, CATKIN_EINVAL, "catkin_solve: tol must be positive and finite");
  if (const int rc = check_tables(ctx, entry, p)) return rc;
  bool from_view = false;
  if (const int rc = check_points(ctx, entry, view, p, &from_view)) return rc;
  if (p->n == 0) return CATKIN_OK;

  const int N = p->nspecies, S = p->nadsorbates, R = p->nsteps, T = S + 1;
  const size_t sn = (size_t)p->n;
  KArgs a;
  set_args(a, view, p, from_view);
  Stage stage;
  if (const int rc = stage_inputs(ctx, entry, p, a, p->theta_guess, &a.guess, from_view, 2, &stage, [](Inputs&) {})) return rc;   // status and iterations
  a.maxit = p->maxit;
  a.tol = p->tol;
  const Row rows[] = {{out->theta, &a.theta, sn * T},       {out->rate, &a.rate, sn * R},           {out->rate_gross, &a.gross, sn * R},
                      {out->flux, &a.flux, sn * N},         {out->flux_scale, &a.fscale, sn * N},   {out->dflux_dc, &a.dfdc, sn * N * N},
                      {out->dflux_dphi, &a.dfdphi, sn * N * 2}};
  a.sens = (out->dflux_dc && N) || (out->dflux_dphi && N);
  if (!rows_doubles(rows) && !out->status && !out->iterations) return CATKIN_OK;
  const int rc = run(ctx, entry, "catkin::steady_kernel", steady_kernel, view, p, stage, a, rows, lds_bytes(N, S), 2, out->status || out->iterations,
                     [&](int32_t* flags) {
                       a.status = flags;
                       a.iters = flags + sn;
                     });
  if (rc) return rc;
  if (out->status) memcpy(out->status, ctx->flags.data(), sn * sizeof(int32_t));
  if (out->iterations) memcpy(out->iterations, ctx->flags.data() + sn, sn * sizeof(int32_t));
  return CATKIN_OK;
}

}  // extern "C"
