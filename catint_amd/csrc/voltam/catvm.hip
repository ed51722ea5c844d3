// libcatint_voltam (include/catint_voltam.h): the voltammogram of a mean-field surface microkinetic model per operating point --
// implicit Euler in the log-coverages along a linear potential program, step doubling with the turnover in the error norm and the
// Richardson-extrapolated state accepted, every point with its own program and step size -- with the current, the charge and the wall
// fluxes along it.  gfx950 / MI355X only.
//
// Mapping, working set, tables and arithmetic: ../pnp_kin.h, included as it is.  The step loop is that of kintrans/catkt.hip: ONE
// wave-uniform loop, every trip of which is one attempted step of every lane that still runs; it ends when __ballot(active) is 0.  What
// a lane decides (accept, extrapolate or not, landing, status) is a predicated select on its scalars; the inner Newton loops end on a
// ballot in the same way.  Before each implicit Euler solve a lane sets the potential and the charge of its point (ln.pt.V, ln.pt.sg) to
// the end time of that solve; the rate constants are recomputed from them at every rate evaluation, so nothing else knows that the
// potential moves.  The implicit Euler solve and the G / D rows are restated here: the bits of catkt.hip are pinned.
// LDS slots: those of kintrans (max(T T, N) + 6 T + 2 N: the steady state's, y_n[T], y_1[T], theta_old[T]); the turnovers of y1, ya and
// yb are scalars in registers, and the extrapolated coverages use the theta_old slots, which are free once the three solves are done.
// At S = 8, N = 8: 151 slots x 512 B = 75.5 KB per wave.  The cost of the divergence is the ratio of the largest to the mean step count
// of a wave (tools/probe/voltam_probe.py).
#include "../../../include/catint_voltam.h"
#include "../pnp_kin.h"

#pragma clang fp contract(off)

namespace catvm {

using namespace pnp::kin;

constexpr int RUNNING = -1;   // a status no point ends with

struct KArgs {
  int32_t N, S, R, nmaxit, w, use_sigma, from_view, ldx, max_steps, maxit, nseg, K;   // maxit, tol: the start (steady_newton reads them)
  int64_t n, n_out;
  const double* c;         // view: [B][N][ldx]
  const double* phi;       // view: [B][ldx]
  const int32_t* st;       // view: [B] solver status
  const int64_t* lanes;    // [n]
  const double *cs, *phis; // host surface state: [n][N], [n]
  const double *phiM, *sigma, *off, *gamma, *theta0;   // phiM: E_start [n]; [n], [n][R][2], [n][N], [n][T]; null: absent
  const double *Ev, *rate, *ne;                        // E_vertex [n], scan_rate [n], electrons [R]
  double *theta, *cur, *cscale, *charge, *eout, *flux, *fscale, *treached;   // device rows; null: not wanted
  int32_t *status, *steps;
  double sd, CS, pzc, rtol, atol, ntol, tol, h0, floor_, Fsd;
};

struct Lane : SteadyLane {
  int oYn, oY1, oTo;   // first slots of the accepted state, of the full step and of theta_old (after the solves: theta_e)
};

__device__ __forceinline__ void lane_slots(Lane& ln, double* lds, int lane, int N, int T) {
  steady_slots(ln, lds, lane, N, T);
  ln.oYn = ln.oC + N;
  ln.oY1 = ln.oYn + T;
  ln.oTo = ln.oY1 + T;
}

// the program of one lane
struct Program {
  double Es, Ev, tau, phi0;
};

// E(t) in segment k
__device__ __forceinline__ double potential_at(const Program& pg, int k, double t) {
#pragma clang fp contract(off)
  const bool back = k & 1;
  const double Ea = back ? pg.Ev : pg.Es, Ez = back ? pg.Es : pg.Ev;
  return Ea + (Ez - Ea) * ((t - (double)k * pg.tau) / pg.tau);
}

// output time of row j (0-based): (k + m / K) tau with k = j / K, m = j - k K + 1
__device__ __forceinline__ double output_time(const Program& pg, int K, int64_t j) {
#pragma clang fp contract(off)
  const int k = (int)(j / K), m = (int)(j - (int64_t)k * K) + 1;
  return ((double)k + (double)m / (double)K) * pg.tau;
}

// the lane's potential and charge at E
__device__ __forceinline__ void set_potential(const KArgs& A, Lane& ln, const Program& pg, int64_t i, double E) {
#pragma clang fp contract(off)
  ln.pt.V = E - (A.w ? pg.phi0 : 0.0);
  ln.pt.sg = A.use_sigma ? A.sigma[i] : A.CS * ((E - A.pzc) - pg.phi0);
}

// D_s into the row scales at the lane's y (and G_s into the right-hand side slots), without the Jacobian
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

// i = sum_r ne_r (rf_r - rb_r) and g = sum_r |ne_r| (rf_r + rb_r) at the lane's y and potential
__device__ __forceinline__ void turnover(const KArgs& A, const Table& tb, const Lane& ln, double& ti, double& tg) {
#pragma clang fp contract(off)
  ti = 0.0;
  tg = 0.0;
  for (int r = 0; r < A.R; ++r) {
    double ef, eb, pf, pb;
    int br;
    steady_rates(A, tb, ln, r, -1, br, ef, eb, pf, pb);
    const double rf = ef * pf, rb = eb * pb, ne = A.ne[r];
    ti = ti + ne * (rf - rb);
    tg = tg + fabs(ne) * (rf + rb);
  }
}

// One implicit Euler solve of size h at the lane's potential: Newton from the y in the lane's slots against the theta_old slots.  run:
// the lane takes part; it: the iterations whose update was applied are added.  Returns whether the lane converged; a lane that has
// converged or failed idles and its y stops changing
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

__global__ __launch_bounds__(64) void sweep_kernel(const KArgs A, const Table* __restrict__ tab) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1, K = A.K;
  const int64_t n_out = A.n_out;
  const Table& tb = *tab;   // its own read-only argument: the uniform reads become scalar loads
  Lane ln;
  lane_slots(ln, lds, lane, N, T);
  double* L = ln.L;
  const double bad_number = __builtin_nan("");

  for (int64_t grp = blockIdx.x; grp * 64 < A.n; grp += gridDim.x) {
    const bool live = grp * 64 + lane < A.n;
    const int64_t i = live ? grp * 64 + lane : A.n - 1;
    const int64_t b = A.lanes[i];
    ln.pt = point_inputs(A, tb, i, b, ln.at(ln.oA));   // phiM is E_start: the potential and the charge of the start
    bool ok = ln.pt.ok;
    // ---- the program ----
    Program pg;
    pg.Es = A.phiM[i];
    pg.Ev = A.Ev[i];
    pg.phi0 = A.from_view ? A.phi[(size_t)b * A.ldx] : A.phis[i];
    const double rate = A.rate[i];
    pg.tau = fabs(pg.Ev - pg.Es) / rate;
    ok = ok && finite_(pg.Ev) && pg.tau > 0.0 && finite_((double)A.nseg * pg.tau);
    const double i_floor = A.floor_ * rate;
    // ---- start: the adsorbates as given and the free site from the balance, or the steady state at E_start ----
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
      for (int t = 0; t < T; ++t) L[(ln.oY + t) * 64] = ok ? L[(ln.oYn + t) * 64] : y0;
    } else {
      for (int t = 0; t < T; ++t) L[(ln.oY + t) * 64] = y0;
      int it0;
      uint64_t pivs0;
      const int s0 = steady_newton(A, tb, ln, ok ? STATUS_MAXIT : STATUS_INPUT, ok && live, it0, pivs0);
      ok = ok && s0 == STATUS_CONVERGED;
    }
    for (int t = 0; t < T; ++t) {
      const double y = ok ? L[(ln.oY + t) * 64] : y0;
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
    double h = A.h0 > 0.0 ? A.h0 : (fastest > 0.0 ? 0.01 / fastest : output_time(pg, K, 0));
    double t_now = 0.0, q_sum = 0.0;
    int64_t k = 0;   // output rows written
    int n_acc = 0, n_rej = 0, n_it = 0, n_plain = 0;
    int status = ok ? RUNNING : CATVM_INPUT;
    bool active = ok && live;

    // ---- the step loop: one attempted step of every running lane per trip ----
    for (;;) {
      if (active && (n_acc + n_rej >= A.max_steps || !(h >= CATVM_MIN_STEP))) {
        status = CATVM_STEPS;
        active = false;
      }
      if (__ballot(active) == 0) break;
      const int64_t row_k = k < n_out ? k : n_out - 1;
      const int seg = (int)(row_k / K);
      const double t_next = output_time(pg, K, row_k);
      const double rem = t_next - t_now;
      const bool lands = rem <= h, shortened = rem < h;
      const double hh = shortened ? rem : h, half = 0.5 * hh;
      const double E_end = potential_at(pg, seg, lands ? t_next : t_now + hh), E_mid = potential_at(pg, seg, t_now + half);
      // y1 = BE(y, hh) at E_end
      for (int t = 0; t < T; ++t) {
        const double v = L[(ln.oYn + t) * 64];
        L[(ln.oY + t) * 64] = v;
        L[(ln.oTo + t) * 64] = exp(v);
      }
      set_potential(A, ln, pg, i, E_end);
      const bool ok1 = be_solve(A, tb, ln, hh, active, n_it);
      double i1, g1;
      turnover(A, tb, ln, i1, g1);
      // ya = BE(y, hh / 2) at E_mid
      for (int t = 0; t < T; ++t) {
        L[(ln.oY1 + t) * 64] = L[(ln.oY + t) * 64];
        L[(ln.oY + t) * 64] = L[(ln.oYn + t) * 64];
      }
      set_potential(A, ln, pg, i, E_mid);
      const bool oka = be_solve(A, tb, ln, half, active && ok1, n_it);
      double ia, ga;
      turnover(A, tb, ln, ia, ga);
      // yb = BE(ya, hh / 2) at E_end
      for (int t = 0; t < T; ++t) L[(ln.oTo + t) * 64] = exp(L[(ln.oY + t) * 64]);
      set_potential(A, ln, pg, i, E_end);
      const bool okb = be_solve(A, tb, ln, half, active && ok1 && oka, n_it);
      double ib, gb;
      turnover(A, tb, ln, ib, gb);
      const bool solved = ok1 && oka && okb;
      // the error of the coverages and of the turnover; the extrapolated coverages into the theta_old slots
      double err = 0.0, used = 0.0;
      bool positive = true;
      for (int t = T - 1; t >= 0; --t) {
        const double thb = exp(L[(ln.oY + t) * 64]), th1 = exp(L[(ln.oY1 + t) * 64]);
        const double d = fabs(thb - th1) / (A.atol + A.rtol * (thb > th1 ? thb : th1));
        err = d > err || d != d ? d : err;
        const double the = t ? 2.0 * thb - th1 : 1.0 - used;
        used = used + tb.ns[t] * the;
        positive = positive && the > 0.0;
        L[(ln.oTo + t) * 64] = the;
      }
      {
        const double ab = fabs(ib), a1 = fabs(i1);
        const double den = A.rtol * ((ab > a1 ? ab : a1) + i_floor) + A.ntol * (gb > g1 ? gb : g1);
        const double d = ib == i1 ? 0.0 : fabs(ib - i1) / den;
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
        n_plain += positive ? 0 : 1;
        t_now = lands ? t_next : t_now + hh;
        const double hn = fac * hh;
        h = shortened && h > hn ? h : hn;
        const double dq1 = hh * i1, dqb = half * (ia + ib);
        q_sum = q_sum + (positive ? 2.0 * dqb - dq1 : dqb);
      }
      for (int t = 0; t < T; ++t) {
        const double ye = log(L[(ln.oTo + t) * 64]);
        const double yn = positive ? (ye < MINLOG ? MINLOG : ye) : L[(ln.oY + t) * 64];
        const double v = accept ? yn : L[(ln.oYn + t) * 64];
        L[(ln.oYn + t) * 64] = v;
        L[(ln.oY + t) * 64] = v;   // the y slots hold the lane's state: what the outputs are formed at
      }
      const bool write = accept && lands;
      if (__ballot(write) == 0) continue;
      // ---- an output time (the lane's potential is that of the end of the step): turnover and fluxes at the accepted state ----
      double io = 0.0, go = 0.0;
      steady_fluxes(A, tb, ln, [&](int r, double net, double gross) {
        const double ne = A.ne[r];
        io = io + ne * net;
        go = go + fabs(ne) * gross;
      });
      if (write) {
        const size_t row = (size_t)i * n_out + k;
        if (A.theta)
          for (int t = 0; t < T; ++t) A.theta[row * T + t] = exp(L[(ln.oY + t) * 64]);
        for (int j = 0; j < N; ++j) {
          if (A.flux) A.flux[row * N + j] = A.sd * L[(ln.oC + j) * 64];
          if (A.fscale) A.fscale[row * N + j] = A.sd * L[(ln.oJ + j) * 64];
        }
        if (A.cur) A.cur[row] = -(A.Fsd * io);
        if (A.cscale) A.cscale[row] = A.Fsd * go;
        if (A.charge) A.charge[row] = -(A.Fsd * q_sum);
        if (A.eout) A.eout[row] = E_end;
        ++k;
        if (k == n_out) {
          status = CATVM_DONE;
          active = false;
        }
      }
    }

    // ---- the rows a lane did not reach: NaN ----
    for (int64_t kk = 0; kk < n_out; ++kk) {
      if (!live || kk < k) continue;
      const size_t row = (size_t)i * n_out + kk;
      if (A.theta)
        for (int t = 0; t < T; ++t) A.theta[row * T + t] = bad_number;
      for (int j = 0; j < N; ++j) {
        if (A.flux) A.flux[row * N + j] = bad_number;
        if (A.fscale) A.fscale[row * N + j] = bad_number;
      }
      if (A.cur) A.cur[row] = bad_number;
      if (A.cscale) A.cscale[row] = bad_number;
      if (A.charge) A.charge[row] = bad_number;
      if (A.eout) A.eout[row] = bad_number;
    }
    if (live) {
      if (A.treached) A.treached[i] = status == CATVM_INPUT ? bad_number : t_now;
      if (A.status) A.status[i] = status;
      if (A.steps) A.steps[i * 4] = n_acc, A.steps[i * 4 + 1] = n_rej, A.steps[i * 4 + 2] = n_it, A.steps[i * 4 + 3] = n_plain;
    }
  }
}

static size_t lds_bytes(int N, int S) {
  const int T = S + 1;
  return (size_t)(std::max(T * T, N) + 6 * T + 2 * N) * 64 * sizeof(double);
}

// catvm_params as the shared host code reads it: the start potentials under the name the other libraries give the potential
struct Params : catvm_params {
  const double* phiM;
};

}  // namespace catvm

static_assert(CATVM_OK == pnp::post::OK && CATVM_EINVAL == pnp::post::ERR_INVAL && CATVM_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATVM_EDEVICE == pnp::post::ERR_DEVICE,
              "catint_voltam.h and pnp_post.h disagree");
static_assert(CATVM_INPUT == pnp::kin::STATUS_INPUT, "catint_voltam.h and pnp_kin.h disagree");

struct catvm_ctx : pnp::post::Ctx {};

extern "C" {

int catvm_create(int32_t device, catvm_ctx** out) { return pnp::post::create("catvm_create", device, out); }
void catvm_destroy(catvm_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catvm_last_error(const catvm_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catvm_last_kernel(const catvm_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catvm_last_kernel_ms(const catvm_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catvm_solve(catvm_ctx* ctx, const pnp_device_view* view, const catvm_params* p, const catvm_outputs* out) {
  using namespace catvm;
  static const char entry[] = "catvm_solve";
  char msg[256];
  if (const int rc = check_sizes(ctx, entry, "catvm_params", "catvm_outputs", p, out)) return rc;
  if (p->newton_maxit < 1) return fail(ctx, CATVM_EINVAL, "catvm_solve: newton_maxit < 1");
  if (p->max_steps < 1 || p->max_steps > CATVM_MAX_STEPS) {
    snprintf(msg, sizeof msg, "catvm_solve: max_steps outside [1, %d]", CATVM_MAX_STEPS);
    return fail(ctx, CATVM_EINVAL, msg);
  }
  if (const int rc = check_drop(ctx, entry, p)) return rc;
  if (!posfin(p->rtol)) return fail(ctx, CATVM_EINVAL, "catvm_solve: rtol must be positive and finite");
  if (!posfin(p->newton_tol)) return fail(ctx, CATVM_EINVAL, "catvm_solve: newton_tol must be positive and finite");
  if (!(p->atol >= 0.0) || !std::isfinite(p->atol)) return fail(ctx, CATVM_EINVAL, "catvm_solve: atol must be finite and not negative");
  if (!(p->rate_floor >= 0.0) || !std::isfinite(p->rate_floor))
    return fail(ctx, CATVM_EINVAL, "catvm_solve: rate_floor must be finite and not negative");
  if (p->h0 != p->h0) return fail(ctx, CATVM_EINVAL, "catvm_solve: h0 is not a number");
  if (p->n_segments < 1 || p->n_segments > CATVM_MAX_SEGMENTS) {
    snprintf(msg, sizeof msg, "catvm_solve: n_segments outside [1, %d]", CATVM_MAX_SEGMENTS);
    return fail(ctx, CATVM_EINVAL, msg);
  }
  if (p->samples < 1 || p->samples > CATVM_MAX_SAMPLES) {
    snprintf(msg, sizeof msg, "catvm_solve: samples outside [1, %d]", CATVM_MAX_SAMPLES);
    return fail(ctx, CATVM_EINVAL, msg);
  }
  if (!p->E_start || !p->E_vertex || !p->scan_rate) return fail(ctx, CATVM_EINVAL, "catvm_solve: E_start, E_vertex and scan_rate are required");
  if (p->n < 0) return fail(ctx, CATVM_EINVAL, "catvm_solve: n < 0");
  for (int64_t i = 0; i < p->n; ++i)
    if (!posfin(p->scan_rate[i])) {
      snprintf(msg, sizeof msg, "catvm_solve: scan_rate[%lld] must be positive and finite", (long long)i);
      return fail(ctx, CATVM_EINVAL, msg);
    }
  Params q;
  static_cast<catvm_params&>(q) = *p;
  q.phiM = p->E_start;
  if (const int rc = check_tables(ctx, entry, &q)) return rc;
  if (!p->electrons) return fail(ctx, CATVM_EINVAL, "catvm_solve: electrons is required");
  for (int r = 0; r < p->nsteps; ++r)
    if (!std::isfinite(p->electrons[r])) {
      snprintf(msg, sizeof msg, "catvm_solve: electrons[%d] is not finite", r);
      return fail(ctx, CATVM_EINVAL, msg);
    }
  bool from_view = false;
  if (const int rc = check_points(ctx, entry, view, &q, &from_view)) return rc;
  if (p->n == 0) return CATVM_OK;

  const int N = p->nspecies, S = p->nadsorbates, R = p->nsteps, T = S + 1;
  const size_t sn = (size_t)p->n, so = (size_t)p->n_segments * (size_t)p->samples;
  KArgs a;
  set_args(a, view, &q, from_view);
  // the program arrays and the electrons behind the staged inputs of the shared layout: one copy still
  Stage stage;
  int i_ev = 0, i_rate = 0, i_ne = 0;
  if (const int rc = stage_inputs(ctx, entry, &q, a, p->theta0, &a.theta0, from_view, 5, &stage, [&](Inputs& in) {
        i_ev = in.add(sn, &a.Ev);
        i_rate = in.add(sn, &a.rate);
        i_ne = in.add((size_t)R, &a.ne);
      }))
    return rc;   // status and the four counters
  memcpy(stage.in.host(ctx->stage, i_ev), p->E_vertex, sn * sizeof(double));
  memcpy(stage.in.host(ctx->stage, i_rate), p->scan_rate, sn * sizeof(double));
  memcpy(stage.in.host(ctx->stage, i_ne), p->electrons, (size_t)R * sizeof(double));
  a.nmaxit = p->newton_maxit;
  a.max_steps = p->max_steps;
  a.maxit = CATVM_START_MAXIT;
  a.nseg = p->n_segments;
  a.K = p->samples;
  a.n_out = (int64_t)so;
  a.rtol = p->rtol;
  a.atol = p->atol;
  a.ntol = p->newton_tol;
  a.tol = p->newton_tol;
  a.h0 = p->h0;
  a.floor_ = p->rate_floor;
  a.Fsd = CATVM_FARADAY * p->site_density;
  const Row rows[] = {{out->theta, &a.theta, sn * so * T},      {out->current, &a.cur, sn * so},   {out->current_scale, &a.cscale, sn * so},
                      {out->charge, &a.charge, sn * so},        {out->E_out, &a.eout, sn * so},    {out->flux, &a.flux, sn * so * N},
                      {out->flux_scale, &a.fscale, sn * so * N}, {out->t_reached, &a.treached, sn}};
  if (!rows_doubles(rows) && !out->status && !out->steps) return CATVM_OK;
  const int rc = run(ctx, entry, "catvm::sweep_kernel", sweep_kernel, view, &q, stage, a, rows, lds_bytes(N, S), 5, out->status || out->steps,
                     [&](int32_t* flags) {
                       a.status = flags;
                       a.steps = flags + sn;
                     });
  if (rc) return rc;
  if (out->status) memcpy(out->status, ctx->flags.data(), sn * sizeof(int32_t));
  if (out->steps) memcpy(out->steps, ctx->flags.data() + sn, 4 * sn * sizeof(int32_t));
  return CATVM_OK;
}

}  // extern "C"
