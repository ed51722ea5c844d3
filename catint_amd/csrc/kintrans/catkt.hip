// libcatint_kintrans (include/catint_kintrans.h): the transient of a mean-field surface microkinetic model per operating point --
// implicit Euler in the log-coverages with step doubling, every point with its own step size -- and the wall fluxes along it.
// gfx950 / MI355X only.
//
// Mapping, working set, tables and arithmetic: ../pnp_kin.h, which holds the rates, the unscaled rows, the LU, the flux sums and the
// host code this library shares with kinetics/catkin.hip.  Lanes differ in everything that is control flow on a CPU: whether a step is
// accepted, how many Newton iterations a solve takes, how many steps a point needs, whether a step is shortened to an output time.
// Here the step loop is ONE wave-uniform loop, every trip of which is one attempted step of every lane that still runs; it ends when
// __ballot(active) is 0.  What a lane decides is a predicated select on its scalars; a lane that has finished idles and the state it
// ended with (the y_n slots) stops changing.  The inner Newton loops end on a ballot in the same way.  The cost of the divergence is the
// ratio of the largest to the mean step count of a wave (tools/probe/kintrans_probe.py).
// LDS slots: those of the steady state (J[T][T] or N slots, y[T], the right-hand side [T], the row scales D[T], the activities a[N] and
// N accumulators) and y_n[T] (the accepted state), y_1[T] (the full step) and theta_old[T]; the first half step needs no slots of its
// own, the second starts from the y it left.  At S = 8, N = 8: 151 slots x 512 B = 75.5 KB per wave.
// Outputs are written by the lane that reaches an output time: a few scattered 8-byte stores per point and output time, not staged.
#include "../../../include/catint_kintrans.h"
#include "../pnp_kin.h"

#pragma clang fp contract(off)

namespace catkt {

using namespace pnp::kin;

constexpr int RUNNING = -1;   // a status no point ends with

struct KArgs {
  int32_t N, S, R, nmaxit, w, use_sigma, from_view, ldx, max_steps, pad_;
  int64_t n, n_out;
  const double* c;         // view: [B][N][ldx]
  const double* phi;       // view: [B][ldx]
  const int32_t* st;       // view: [B] solver status
  const int64_t* lanes;    // [n]
  const double *cs, *phis; // host surface state: [n][N], [n]
  const double *phiM, *sigma, *off, *gamma, *theta0, *tout;   // [n], [n], [n][R][2], [n][N], [n][T], [n_out]; null: absent
  double *theta, *flux, *fscale, *drift, *treached;           // device rows; null: not wanted
  int32_t *status, *steps;
  double sd, CS, pzc, rtol, atol, ntol, stol, h0;
};

struct Lane : SteadyLane {
  int oYn, oY1, oTo;   // first slots of the accepted state, of the full step and of theta_old
};

__device__ __forceinline__ void lane_slots(Lane& ln, double* lds, int lane, int N, int T) {
  steady_slots(ln, lds, lane, N, T);
  ln.oYn = ln.oC + N;
  ln.oY1 = ln.oYn + T;
  ln.oTo = ln.oY1 + T;
}

// G_s into the right-hand side slots and D_s into the row scales at the lane's y, without the Jacobian
__device__ __forceinline__ void net_rows(const KArgs& A, const Table& tb, const Lane& ln) {
#pragma clang fp contract(off)
  const int N = A.N, T = A.S + 1;
  double* L = ln.L;
  for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0, L[(ln.oD + s) * 64] = 0.0;
  for (int r = 0; r < A.R; ++r) {
    double ef, eb, pf, pb;
    int br;
    steady_rates(A, tb, ln, r, -1, br, ef, eb, pf, pb);
    const double rf = ef * pf, rb = eb * pb, net = rf - rb, gross = rf + rb;
    for (int s = 1; s < T; ++s) {
      const int m = tb.ob[r][N + s] - tb.of[r][N + s];
      if (m == 0) continue;
      const double dm = (double)m;
      L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + dm * net;
      L[(ln.oD + s) * 64] = L[(ln.oD + s) * 64] + fabs(dm) * gross;
    }
  }
}

// max over the rows with D_s > 0 of |G_s| / D_s after net_rows (a NaN stays one)
__device__ __forceinline__ double drift_of(const Lane& ln, int T) {
#pragma clang fp contract(off)
  double mx = 0.0;
  for (int s = 1; s < T; ++s) {
    const double D = ln.L[(ln.oD + s) * 64];
    const double d = D > 0.0 ? fabs(ln.L[(ln.oB + s) * 64]) / D : 0.0;
    mx = d > mx || d != d ? d : mx;
  }
  return mx;
}

// One implicit Euler solve of size h: Newton from the y in the lane's slots against the theta_old slots.  run: the lane takes part;
// it: the iterations whose update was applied are added.  Returns whether the lane converged; a lane that has converged or failed
// idles and its y stops changing
__device__ __forceinline__ bool be_solve(const KArgs& A, const Table& tb, const Lane& ln, double h, bool run, int& it) {
#pragma clang fp contract(off)
  const int N = A.N, T = A.S + 1;
  double* L = ln.L;
  bool active = run, ok = false;
  for (int iter = 0; iter < A.nmaxit; ++iter) {
    if (__ballot(active) == 0) break;
    for (int s = 0; s < T * T; ++s) L[(ln.oJ + s) * 64] = 0.0;
    for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0, L[(ln.oD + s) * 64] = 0.0;
    for (int r = 0; r < A.R; ++r) {
      double ef, eb, pf, pb;
      int br;
      steady_rates(A, tb, ln, r, -1, br, ef, eb, pf, pb);
      add_step_rows(tb, N, T, r, ef * pf, eb * pb, ln.at(ln.oJ), ln.at(ln.oB), ln.at(ln.oD));
    }
    for (int s = 1; s < T; ++s) {
      const double th = exp(L[(ln.oY + s) * 64]);
      const double w = th + h * L[(ln.oD + s) * 64];
      for (int t = 0; t < T; ++t) {
        double* e = &L[(ln.oJ + s * T + t) * 64];
        *e = ((t == s ? th : 0.0) - h * *e) / w;
      }
      L[(ln.oB + s) * 64] = -(((th - L[(ln.oTo + s) * 64]) - h * L[(ln.oB + s) * 64]) / w);
    }
    const double f0 = site_row(tb, ln.at(ln.oJ), ln.at(ln.oY), T);
    L[ln.oB * 64] = -(f0 - 1.0);
    uint64_t pivs;
    const bool bad = factor(ln.at(ln.oJ), T, pivs);
    substitute(ln.at(ln.oJ), ln.at(ln.oB), T, pivs);
    double mx = 0.0;
    for (int t = 0; t < T; ++t) {
      const double d = fabs(L[(ln.oB + t) * 64]);
      mx = d > mx || d != d ? d : mx;
    }
    const bool fin = finite_(mx);
    const double sc = mx > 3.0 ? 3.0 / mx : 1.0;
    const bool move = active && !bad && fin;
    for (int t = 0; t < T; ++t) {
      const double y = L[(ln.oY + t) * 64];
      const double v = y + sc * L[(ln.oB + t) * 64];
      L[(ln.oY + t) * 64] = move ? (v < MINLOG ? MINLOG : v) : y;
    }
    if (active) {
      if (!move) {
        active = false;
      } else {
        ++it;
        if (mx < A.ntol) {
          ok = true;
          active = false;
        }
      }
    }
  }
  return ok;
}

__global__ __launch_bounds__(64) void transient_kernel(const KArgs A, const Table* __restrict__ tab) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1;
  const int64_t n_out = A.n_out;
  const Table& tb = *tab;   // its own read-only argument: the uniform reads become scalar loads
  Lane ln;
  lane_slots(ln, lds, lane, N, T);
  double* L = ln.L;
  const double bad_number = __builtin_nan("");
  const bool want_flux = A.flux || A.fscale;

  for (int64_t grp = blockIdx.x; grp * 64 < A.n; grp += gridDim.x) {
    const bool live = grp * 64 + lane < A.n;
    const int64_t i = live ? grp * 64 + lane : A.n - 1;
    const int64_t b = A.lanes[i];
    ln.pt = point_inputs(A, tb, i, b, ln.at(ln.oA));
    bool ok = ln.pt.ok;
    // ---- start: the adsorbates as given, the free site from the balance ----
    double nsum = 0.0;
    for (int t = 0; t < T; ++t) nsum = nsum + tb.ns[t];
    const double y0 = log(1.0 / nsum);
    if (A.theta0) {
      double used = 0.0;
      for (int t = 1; t < T; ++t) {
        const double g = A.theta0[i * T + t];
        ok = ok && finite_(g);
        const double y = log_coverage(g);
        L[(ln.oYn + t) * 64] = y;
        used = used + tb.ns[t] * exp(y);
      }
      const double free_ = 1.0 - used;
      ok = ok && free_ > 0.0;
      L[ln.oYn * 64] = log_coverage(free_);
    }
    for (int t = 0; t < T; ++t) {
      const double y = A.theta0 && ok ? L[(ln.oYn + t) * 64] : y0;
      L[(ln.oYn + t) * 64] = y;
      L[(ln.oY + t) * 64] = y;
    }
    // ---- first step size ----
    net_rows(A, tb, ln);
    double fastest = 0.0;
    for (int s = 1; s < T; ++s) {
      const double D = L[(ln.oD + s) * 64];
      const double q = D > 0.0 ? D / exp(L[(ln.oY + s) * 64]) : 0.0;
      fastest = q > fastest ? q : fastest;
    }
    double h = A.h0 > 0.0 ? A.h0 : (fastest > 0.0 ? 0.01 / fastest : A.tout[0]);
    double t_now = 0.0, last_drift = bad_number;
    int64_t k = 0;   // output rows written
    int n_acc = 0, n_rej = 0, n_it = 0;
    int status = ok ? RUNNING : CATKT_INPUT;
    bool active = ok && live;

    // ---- the step loop: one attempted step of every running lane per trip ----
    for (;;) {
      if (active && (n_acc + n_rej >= A.max_steps || !(h >= CATKT_MIN_STEP))) {
        status = CATKT_STEPS;
        active = false;
      }
      if (__ballot(active) == 0) break;
      const double t_next = A.tout[k < n_out ? k : n_out - 1];
      const double rem = t_next - t_now;
      const bool lands = rem <= h, shortened = rem < h;
      const double hh = shortened ? rem : h, half = 0.5 * hh;
      // y1 = BE(y, hh)
      for (int t = 0; t < T; ++t) {
        const double v = L[(ln.oYn + t) * 64];
        L[(ln.oY + t) * 64] = v;
        L[(ln.oTo + t) * 64] = exp(v);
      }
      const bool ok1 = be_solve(A, tb, ln, hh, active, n_it);
      // ya = BE(y, hh / 2)
      for (int t = 0; t < T; ++t) {
        L[(ln.oY1 + t) * 64] = L[(ln.oY + t) * 64];
        L[(ln.oY + t) * 64] = L[(ln.oYn + t) * 64];
      }
      const bool oka = be_solve(A, tb, ln, half, active && ok1, n_it);
      // yb = BE(ya, hh / 2)
      for (int t = 0; t < T; ++t) L[(ln.oTo + t) * 64] = exp(L[(ln.oY + t) * 64]);
      const bool okb = be_solve(A, tb, ln, half, active && ok1 && oka, n_it);
      const bool solved = ok1 && oka && okb;
      double err = 0.0;
      for (int t = 0; t < T; ++t) {
        const double thb = exp(L[(ln.oY + t) * 64]), th1 = exp(L[(ln.oY1 + t) * 64]);
        const double d = fabs(thb - th1) / (A.atol + A.rtol * (thb > th1 ? thb : th1));
        err = d > err || d != d ? d : err;
      }
      const double f = 0.9 / sqrt(err);
      const double fac = f > 5.0 ? 5.0 : (f >= 0.2 ? f : 0.2);
      const bool accept = active && solved && err <= 1.0;
      if (active && !accept) {
        ++n_rej;
        h = solved ? fac * hh : 0.25 * hh;
      }
      if (accept) {
        ++n_acc;
        t_now = lands ? t_next : t_now + hh;
        const double hn = fac * hh;
        h = shortened && h > hn ? h : hn;
      }
      for (int t = 0; t < T; ++t) L[(ln.oYn + t) * 64] = accept ? L[(ln.oY + t) * 64] : L[(ln.oYn + t) * 64];
      if (__ballot(accept) == 0) continue;
      // ---- after an accepted step (the y slots of an accepting lane hold its new state): drift, steady stop, output ----
      net_rows(A, tb, ln);
      const double drift = drift_of(ln, T);
      if (accept) last_drift = drift;
      const bool steady = accept && A.stol > 0.0 && drift < A.stol;
      const bool write = accept && lands && !steady;
      if (steady) {
        status = CATKT_STEADY;
        active = false;
      }
      if (__ballot(write) == 0) continue;
      if (want_flux) steady_fluxes(A, tb, ln, [](int, double, double) {});
      if (write) {
        const size_t row = (size_t)i * n_out + k;
        if (A.theta)
          for (int t = 0; t < T; ++t) A.theta[row * T + t] = exp(L[(ln.oY + t) * 64]);
        for (int j = 0; j < N; ++j) {
          if (A.flux) A.flux[row * N + j] = A.sd * L[(ln.oC + j) * 64];
          if (A.fscale) A.fscale[row * N + j] = A.sd * L[(ln.oJ + j) * 64];
        }
        if (A.drift) A.drift[row] = drift;
        ++k;
        if (k == n_out) {
          status = CATKT_DONE;
          active = false;
        }
      }
    }

    // ---- the rows a lane did not reach: the state it stopped at (CATKT_STEADY) or NaN ----
    for (int t = 0; t < T; ++t) L[(ln.oY + t) * 64] = L[(ln.oYn + t) * 64];
    if (want_flux) steady_fluxes(A, tb, ln, [](int, double, double) {});
    const bool nan = status != CATKT_STEADY;
    for (int64_t kk = 0; kk < n_out; ++kk) {
      if (!live || kk < k) continue;
      const size_t row = (size_t)i * n_out + kk;
      if (A.theta)
        for (int t = 0; t < T; ++t) A.theta[row * T + t] = nan ? bad_number : exp(L[(ln.oY + t) * 64]);
      for (int j = 0; j < N; ++j) {
        if (A.flux) A.flux[row * N + j] = nan ? bad_number : A.sd * L[(ln.oC + j) * 64];
        if (A.fscale) A.fscale[row * N + j] = nan ? bad_number : A.sd * L[(ln.oJ + j) * 64];
      }
      if (A.drift) A.drift[row] = nan ? bad_number : last_drift;
    }
    if (live) {
      if (A.treached) A.treached[i] = status == CATKT_INPUT ? bad_number : t_now;
      if (A.status) A.status[i] = status;
      if (A.steps) A.steps[i * 3] = n_acc, A.steps[i * 3 + 1] = n_rej, A.steps[i * 3 + 2] = n_it;
    }
  }
}

static size_t lds_bytes(int N, int S) {
  const int T = S + 1;
  return (size_t)(std::max(T * T, N) + 6 * T + 2 * N) * 64 * sizeof(double);
}

}  // namespace catkt

static_assert(CATKT_OK == pnp::post::OK && CATKT_EINVAL == pnp::post::ERR_INVAL && CATKT_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATKT_EDEVICE == pnp::post::ERR_DEVICE,
              "catint_kintrans.h and pnp_post.h disagree");
static_assert(CATKT_INPUT == pnp::kin::STATUS_INPUT, "catint_kintrans.h and pnp_kin.h disagree");

struct catkt_ctx : pnp::post::Ctx {};

extern "C" {

int catkt_create(int32_t device, catkt_ctx** out) { return pnp::post::create("catkt_create", device, out); }
void catkt_destroy(catkt_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catkt_last_error(const catkt_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catkt_last_kernel(const catkt_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catkt_last_kernel_ms(const catkt_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catkt_solve(catkt_ctx* ctx, const pnp_device_view* view, const catkt_params* p, const catkt_outputs* out) {
  using namespace catkt;
  static const char entry[] = "catkt_solve";
  char msg[256];
  if (const int rc = check_sizes(ctx, entry, "catkt_params", "catkt_outputs", p, out)) return rc;
  if (p->newton_maxit < 1) return fail(ctx, CATKT_EINVAL, "catkt_solve: newton_maxit < 1");
  if (p->max_steps < 1 || p->max_steps > CATKT_MAX_STEPS) {
    snprintf(msg, sizeof msg, "catkt_solve: max_steps outside [1, %d]", CATKT_MAX_STEPS);
    return fail(ctx, CATKT_EINVAL, msg);
  }
  if (const int rc = check_drop(ctx, entry, p)) return rc;
  if (!posfin(p->rtol)) return fail(ctx, CATKT_EINVAL, "catkt_solve: rtol must be positive and finite");
  if (!posfin(p->newton_tol)) return fail(ctx, CATKT_EINVAL, "catkt_solve: newton_tol must be positive and finite");
  if (!(p->atol >= 0.0) || !std::isfinite(p->atol)) return fail(ctx, CATKT_EINVAL, "catkt_solve: atol must be finite and not negative");
  if (!(p->steady_tol >= 0.0) || !std::isfinite(p->steady_tol))
    return fail(ctx, CATKT_EINVAL, "catkt_solve: steady_tol must be finite and not negative");
  if (p->h0 != p->h0) return fail(ctx, CATKT_EINVAL, "catkt_solve: h0 is not a number");
  if (p->n_out < 1) return fail(ctx, CATKT_EINVAL, "catkt_solve: n_out < 1");
  if (!p->t_out) return fail(ctx, CATKT_EINVAL, "catkt_solve: t_out is required");
  for (int64_t k = 0; k < p->n_out; ++k) {
    const double t = p->t_out[k];
    if (!posfin(t)) {
      snprintf(msg, sizeof msg, "catkt_solve: t_out[%lld] must be positive and finite", (long long)k);
      return fail(ctx, CATKT_EINVAL, msg);
    }
    if (k > 0 && !(t > p->t_out[k - 1])) {
      snprintf(msg, sizeof msg, "catkt_solve: t_out is not strictly increasing at index %lld", (long long)k);
      return fail(ctx, CATKT_EINVAL, msg);
    }
  }
  if (const int rc = check_tables(ctx, entry, p)) return rc;
  bool from_view = false;
  if (const int rc = check_points(ctx, entry, view, p, &from_view)) return rc;
  if (p->n == 0) return CATKT_OK;

  const int N = p->nspecies, S = p->nadsorbates, T = S + 1;
  const size_t sn = (size_t)p->n, so = (size_t)p->n_out;
  KArgs a;
  set_args(a, view, p, from_view);
  // the output times behind the staged inputs of the shared layout: one copy still
  Stage stage;
  int i_tout = 0;
  if (const int rc = stage_inputs(ctx, entry, p, a, p->theta0, &a.theta0, from_view, 4, &stage, [&](Inputs& in) { i_tout = in.add(so, &a.tout); }))
    return rc;   // status and the three counters
  memcpy(stage.in.host(ctx->stage, i_tout), p->t_out, so * sizeof(double));
  a.nmaxit = p->newton_maxit;
  a.max_steps = p->max_steps;
  a.n_out = p->n_out;
  a.rtol = p->rtol;
  a.atol = p->atol;
  a.ntol = p->newton_tol;
  a.stol = p->steady_tol;
  a.h0 = p->h0;
  const Row rows[] = {{out->theta, &a.theta, sn * so * T}, {out->flux, &a.flux, sn * so * N}, {out->flux_scale, &a.fscale, sn * so * N},
                      {out->drift, &a.drift, sn * so},     {out->t_reached, &a.treached, sn}};
  if (!rows_doubles(rows) && !out->status && !out->steps) return CATKT_OK;
  const int rc = run(ctx, entry, "catkt::transient_kernel", transient_kernel, view, p, stage, a, rows, lds_bytes(N, S), 4, out->status || out->steps,
                     [&](int32_t* flags) {
                       a.status = flags;
                       a.steps = flags + sn;
                     });
  if (rc) return rc;
  if (out->status) memcpy(out->status, ctx->flags.data(), sn * sizeof(int32_t));
  if (out->steps) memcpy(out->steps, ctx->flags.data() + sn, 3 * sn * sizeof(int32_t));
  return CATKT_OK;
}

}  // extern "C"
