// libcatint_iasweep (include/catint_iasweep.h): the voltammogram of a surface microkinetic model with lateral interactions and up to
// three site types per operating point -- the step loop of voltam/catvm.hip (implicit Euler in the log-coverages along a linear
// potential program, step doubling with the turnover in the error norm, the Richardson-extrapolated state accepted) over the rate
// constants, the effective orders and the site rows of interact/catia.hip, and a hold at constant potential.  gfx950 / MI355X only.
//
// Mapping, working set, tables and arithmetic: ../pnp_kin.h, included as it is.  ONE wave-uniform step loop, every trip of which is one
// attempted step of every lane that still runs; it ends when __ballot(active) is 0.  What a lane decides is a predicated select on its
// scalars; the inner Newton loops end on a ballot in the same way.  The coverage-dependent constants, the effective orders, the
// surface state and the unscaled rows are restated here from catia.hip, the step loop from catvm.hip: the bits of both are pinned, and
// with G = 1 and strength 0 every sum below is taken in catvm.hip's order, so the outputs have its bits.  The response factors f_g,
// f'_g and the per-type sums are scalars picked by compares on a wave-uniform type index, never an indexed register array.
// LDS slots: the steady state's of pnp_kin.h (max(T T, N) + 3 T + 2 N), theta[T], y_n[T], y_1[T], theta_old[T] (after the solves:
// theta_e): max(T T, N) + 7 T + 2 N.  catia.hip's w[T] = f theta is NOT kept: the one product is formed where it is read, with the same
// bits.  At T = 9, N = 8: 160 slots x 512 B = 80 KB per wave, two waves per CU (169 with w[T] kept: one).
#include "../../../include/catint_iasweep.h"
#include "../pnp_kin.h"

#pragma clang fp contract(off)

namespace catis {

using namespace pnp::kin;

constexpr int MAXG = CATIA_MAX_SITE_TYPES;
constexpr int RUNNING = -1;   // a status no point ends with

// what the call adds to kin::Table (T = G + S columns there), flattened and contracted on the host
struct Extra {
  int32_t G, mode;
  int32_t site_of[MAXT + 1];
  double x[MAXG], cutoff[MAXG], smooth[MAXG];
  double nx[MAXT];                               // n_t / x_g(t)
  double eps[MAXS][MAXS];                        // [adsorbate][adsorbate]
  double eg[MAXR][MAXS], ea[MAXR][MAXS];         // EG, EA: [step][adsorbate]
};
static_assert(sizeof(Extra) % 8 == 0, "the table is copied as doubles");

struct KArgs {
  int32_t N, S, R, nmaxit, w, use_sigma, from_view, ldx, max_steps, maxit, nseg, K, G, ramp;   // S: T - 1 (as pnp_kin.h reads it); maxit, tol: the start
  int64_t n, n_out;
  const double* c;         // view: [B][N][ldx]
  const double* phi;       // view: [B][ldx]
  const int32_t* st;       // view: [B] solver status
  const int64_t* lanes;    // [n]
  const double *cs, *phis; // host surface state: [n][N], [n]
  const double *phiM, *sigma, *off, *gamma, *theta0;   // phiM: E_start [n]; [n], [n][R][2], [n][N], [n][T]; null: absent
  const double *Ev, *rate, *ne, *hold;                 // E_vertex [n], scan_rate [n], electrons [R], hold_time [n] or null
  const Extra* ext;
  double *theta, *cur, *cscale, *charge, *eout, *flux, *fscale, *treached, *eshift;   // device rows; null: not wanted
  int32_t *status, *steps;
  double sd, CS, pzc, rtol, atol, ntol, tol, h0, floor_, Fsd, strength;
};

struct Lane : SteadyLane {
  int oTh, oYn, oY1, oTo;   // first slots of theta, of the accepted state, of the full step and of theta_old (after the solves: theta_e)
};

__device__ __forceinline__ void lane_slots(Lane& ln, double* lds, int lane, int N, int T) {
  steady_slots(ln, lds, lane, N, T);
  ln.oTh = ln.oC + N;
  ln.oYn = ln.oTh + T;
  ln.oY1 = ln.oYn + T;
  ln.oTo = ln.oY1 + T;
}

// f_g and f'_g of the three types
struct Resp {
  double f0, f1, f2, p0, p1, p2;
};

__device__ __forceinline__ double pick(int g, double a, double b, double c) { return g == 0 ? a : (g == 1 ? b : c); }

__device__ __forceinline__ void response(double crowd, double c, double s, double& f, double& fp) {
  const double d = crowd - c, u = d + s;
  const bool below = d <= -s, inside = d < s;
  f = below ? 0.0 : (inside ? (u * u) / (4.0 * s) : d);
  fp = below ? 0.0 : (inside ? u / (2.0 * s) : 1.0);
}

// theta_t = exp(y_t) into the lane's slots; the response of every type
__device__ __forceinline__ Resp surface_state(const Table& tb, const Extra& X, const Lane& ln, int T) {
  double* L = ln.L;
  const int G = X.G;
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;
  for (int t = 0; t < T; ++t) {
    const double th = exp(L[(ln.oY + t) * 64]);
    L[(ln.oTh + t) * 64] = th;
    if (t >= G) {
      const int g = X.site_of[t];
      const double v = tb.ns[t] * th;
      c0 = c0 + (g == 0 ? v : 0.0);
      c1 = c1 + (g == 1 ? v : 0.0);
      c2 = c2 + (g == 2 ? v : 0.0);
    }
  }
  Resp q{1.0, 1.0, 1.0, 0.0, 0.0, 0.0};
  if (X.mode == CATIA_PIECEWISE) {
    response(c0 / X.x[0], X.cutoff[0], X.smooth[0], q.f0, q.p0);
    if (G > 1) response(c1 / X.x[1], X.cutoff[1], X.smooth[1], q.f1, q.p1);
    if (G > 2) response(c2 / X.x[2], X.cutoff[2], X.smooth[2], q.f2, q.p2);
  }
  return q;
}

// w_t = f_g(t) theta_t of the adsorbate column t
__device__ __forceinline__ double weight(const Extra& X, const Lane& ln, const Resp& q, int t) {
  return pick(X.site_of[t], q.f0, q.f1, q.f2) * ln.L[(ln.oTh + t) * 64];
}

// what a step's rate constants are at the lane's coverages: ln kf, ln kb, the branch of Ga, and (piecewise mode, want_q) the per-type
// sums sum_{u on g} E[r][u] theta_u of the dG row (qg) and of the row of the branch (qs)
struct StepK {
  double lf, lb, qg0, qg1, qg2, qs0, qs1, qs2;
  int br;
};

__device__ __forceinline__ void step_constants(const KArgs& A, const Table& tb, const Extra& X, const Lane& ln, const Resp& q, int r, double lam, bool want_q,
                                               StepK& k) {
  const double* L = ln.L;
  const int G = X.G, S = A.S + 1 - G;
  const double V = ln.pt.V, sg = ln.pt.sg, s2 = sg * sg;
  const double dG0 = ((tb.dg[r][0] + tb.dg[r][1] * V) + tb.dg[r][2] * sg) + tb.dg[r][3] * s2;
  const double Ea0 = ((tb.ea[r][0] + tb.ea[r][1] * V) + tb.ea[r][2] * sg) + tb.ea[r][3] * s2;
  const bool ts = tb.ea[r][0] != -INFINITY;
  double sG = 0.0, sA = 0.0;
  for (int a = 0; a < S; ++a) {
    const double w = weight(X, ln, q, G + a);
    sG = sG + X.eg[r][a] * w;
    if (ts) sA = sA + X.ea[r][a] * w;
  }
  const double dG = dG0 + lam * sG;
  const double Ea = ts ? Ea0 + lam * sA : Ea0;
  const bool b0 = Ea >= dG && Ea >= 0.0, b1 = dG >= 0.0;
  k.br = b0 ? 0 : (b1 ? 1 : 2);
  const double Ga = b0 ? Ea : (b1 ? dG : 0.0);
  const double* off = ln.pt.off;
  const double o0 = off ? off[2 * r] : 0.0, o1 = off ? off[2 * r + 1] : 0.0;
  k.lf = (tb.lnA[r] - Ga) + o0;
  k.lb = (tb.lnA[r] - (Ga - dG)) + o1;
  k.qg0 = k.qg1 = k.qg2 = k.qs0 = k.qs1 = k.qs2 = 0.0;
  if (want_q && X.mode == CATIA_PIECEWISE)
    for (int a = 0; a < S; ++a) {
      const int g = X.site_of[G + a];
      const double th = L[(ln.oTh + G + a) * 64];
      const double eG = X.eg[r][a], eS = k.br == 0 ? X.ea[r][a] : (k.br == 1 ? eG : 0.0);
      const double vg = eG * th, vs = eS * th;
      k.qg0 = k.qg0 + (g == 0 ? vg : 0.0), k.qs0 = k.qs0 + (g == 0 ? vs : 0.0);
      k.qg1 = k.qg1 + (g == 1 ? vg : 0.0), k.qs1 = k.qs1 + (g == 1 ? vs : 0.0);
      k.qg2 = k.qg2 + (g == 2 ? vg : 0.0), k.qs2 = k.qs2 + (g == 2 ? vs : 0.0);
    }
}

// d ln rf / dy_t and d ln rb / dy_t of step r: the orders of column t, and for an adsorbate -theta_t dGa/dtheta_t and
// -theta_t (dGa/dtheta_t - ddG/dtheta_t) on top
__device__ __forceinline__ void effective_orders(const Extra& X, const Lane& ln, const Resp& q, const StepK& k, int r, double lam, int t, int of, int ob,
                                                 double& ofe, double& obe) {
  ofe = (double)of;
  obe = (double)ob;
  if (t < X.G) return;
  const int a = t - X.G, g = X.site_of[t];
  const double f = pick(g, q.f0, q.f1, q.f2), fp = pick(g, q.p0, q.p1, q.p2);
  const double eG = X.eg[r][a], eS = k.br == 0 ? X.ea[r][a] : (k.br == 1 ? eG : 0.0);
  const double gG = lam * (eG * f + (X.nx[t] * fp) * pick(g, k.qg0, k.qg1, k.qg2));
  const double gS = lam * (eS * f + (X.nx[t] * fp) * pick(g, k.qs0, k.qs1, k.qs2));
  const double th = ln.L[(ln.oTh + t) * 64];
  ofe = ofe - th * gS;
  obe = obe - th * (gS - gG);
}

// rf and rb of step r as their two factors; the theta slots hold the lane's coverages and q their response
__device__ __forceinline__ void step_rates(const KArgs& A, const Table& tb, const Extra& X, const Lane& ln, const Resp& q, int r, double lam, bool want_q,
                                           StepK& k, double& ef, double& eb, double& pf, double& pb) {
  step_constants(A, tb, X, ln, q, r, lam, want_q, k);
  rate_factors(tb, A.N, A.S + 1, ln.at(ln.oY), ln.at(ln.oA), r, k.lf, k.lb, -1, ef, eb, pf, pb);
}

// the unscaled rows at the lane's y and the strength lam: sum_r m[r][s] (rf - rb) into the right-hand side slots, the row scales D and,
// with jac, dG_s/dy_v into J (rows G .. T-1; J, B and D zeroed first).  Leaves theta of that y in its slots
__device__ __forceinline__ Resp raw_rows(const KArgs& A, const Table& tb, const Extra& X, const Lane& ln, double lam, bool jac) {
  const int N = A.N, T = A.S + 1, G = X.G;
  double* L = ln.L;
  const Resp q = surface_state(tb, X, ln, T);
  if (jac)
    for (int s = 0; s < T * T; ++s) L[(ln.oJ + s) * 64] = 0.0;
  for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0, L[(ln.oD + s) * 64] = 0.0;
  for (int r = 0; r < A.R; ++r) {
    StepK k;
    double ef, eb, pf, pb;
    step_rates(A, tb, X, ln, q, r, lam, jac, k, ef, eb, pf, pb);
    const double rf = ef * pf, rb = eb * pb, net = rf - rb, gross = rf + rb;
    for (int s = G; s < T; ++s) {
      const int m = tb.ob[r][N + s] - tb.of[r][N + s];
      if (m == 0) continue;
      L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + (double)m * net;
      L[(ln.oD + s) * 64] = L[(ln.oD + s) * 64] + fabs((double)m) * gross;
    }
    if (!jac) continue;
    for (int t = 0; t < T; ++t) {
      const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
      if (t < G && !(of | ob)) continue;
      double ofe, obe;
      effective_orders(X, ln, q, k, r, lam, t, of, ob, ofe, obe);
      const double c = rf * ofe - rb * obe;
      for (int s = G; s < T; ++s) {
        const int m = tb.ob[r][N + s] - tb.of[r][N + s];
        if (m) L[(ln.oJ + s * T + t) * 64] = L[(ln.oJ + s * T + t) * 64] + (double)m * c;
      }
    }
  }
  return q;
}

// one site row per type into rows 0 .. G-1 of J and of the right-hand side
__device__ __forceinline__ void site_rows(const Table& tb, const Extra& X, const Lane& ln, int T) {
  double* L = ln.L;
  for (int g = 0; g < X.G; ++g) {
    double f = 0.0;
    for (int t = 0; t < T; ++t) {
      const bool on = X.site_of[t] == g;
      const double th = tb.ns[t] * exp(L[(ln.oY + t) * 64]);
      L[(ln.oJ + g * T + t) * 64] = on ? th / X.x[g] : 0.0;
      f = f + (on ? th : 0.0);
    }
    L[(ln.oB + g) * 64] = -(f / X.x[g] - 1.0);
  }
}

// the damped update of catvm.hip's solve from the factorised J and the right-hand side; returns max|dy| and whether the lane moved
__device__ __forceinline__ bool damped_update(const Lane& ln, int T, bool active, bool need_finite, double& mx, bool& bad) {
  double* L = ln.L;
  uint64_t pivs;
  bad = factor(ln.at(ln.oJ), T, pivs);
  substitute(ln.at(ln.oJ), ln.at(ln.oB), T, pivs);
  mx = 0.0;
  for (int t = 0; t < T; ++t) {
    const double d = fabs(L[(ln.oB + t) * 64]);
    mx = d > mx || d != d ? d : mx;
  }
  const double sc = mx > 3.0 ? 3.0 / mx : 1.0;
  const bool move = active && !bad && (!need_finite || finite_(mx));
  for (int t = 0; t < T; ++t) {
    const double y = L[(ln.oY + t) * 64];
    const double v = y + sc * L[(ln.oB + t) * 64];
    L[(ln.oY + t) * 64] = move ? (v < MINLOG ? MINLOG : v) : y;
  }
  return move;
}

// One stage of the start: the damped Newton iteration of catia.hip at the strength lam from the y in the lane's slots
__device__ __forceinline__ int stage_newton(const KArgs& A, const Table& tb, const Extra& X, const Lane& ln, double lam, bool run) {
  const int T = A.S + 1, G = X.G;
  double* L = ln.L;
  int status = STATUS_MAXIT;
  bool active = run;
  for (int iter = 0; iter < A.maxit; ++iter) {
    if (__ballot(active) == 0) break;
    raw_rows(A, tb, X, ln, lam, true);
    for (int s = G; s < T; ++s) {
      const double D = L[(ln.oD + s) * 64];
      const bool dead = scale_row(ln.at(ln.oJ), ln.at(ln.oY), T, s, D);
      const double g = L[(ln.oB + s) * 64];
      L[(ln.oB + s) * 64] = dead ? 0.0 : -(g / D);
    }
    site_rows(tb, X, ln, T);
    double mx;
    bool bad;
    damped_update(ln, T, active, false, mx, bad);
    if (active) {
      if (bad) {
        status = STATUS_PIVOT;
        active = false;
      } else if (mx < A.tol) {
        status = STATUS_CONVERGED;
        active = false;
      }
    }
  }
  return status;
}

// One implicit Euler solve of size h at the lane's potential: Newton from the y in the lane's slots against the theta_old slots.  run:
// the lane takes part; it: the iterations whose update was applied are added.  Returns whether the lane converged
__device__ __forceinline__ bool be_solve(const KArgs& A, const Table& tb, const Extra& X, const Lane& ln, double h, bool run, int& it) {
  const int T = A.S + 1, G = X.G;
  double* L = ln.L;
  bool active = run, ok = false;
  for (int iter = 0; iter < A.nmaxit; ++iter) {
    if (__ballot(active) == 0) break;
    raw_rows(A, tb, X, ln, A.strength, true);
    for (int s = G; s < T; ++s) {
      const double th = L[(ln.oTh + s) * 64];
      const double w = th + h * L[(ln.oD + s) * 64];
      for (int t = 0; t < T; ++t) {
        double* e = &L[(ln.oJ + s * T + t) * 64];
        *e = ((t == s ? th : 0.0) - h * *e) / w;
      }
      L[(ln.oB + s) * 64] = -(((th - L[(ln.oTo + s) * 64]) - h * L[(ln.oB + s) * 64]) / w);
    }
    site_rows(tb, X, ln, T);
    double mx;
    bool bad;
    const bool move = damped_update(ln, T, active, true, mx, bad);
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

// i = sum_r ne_r (rf_r - rb_r) and g = sum_r |ne_r| (rf_r + rb_r) at the lane's y and potential
__device__ __forceinline__ void turnover(const KArgs& A, const Table& tb, const Extra& X, const Lane& ln, double& ti, double& tg) {
  const Resp q = surface_state(tb, X, ln, A.S + 1);
  ti = 0.0;
  tg = 0.0;
  for (int r = 0; r < A.R; ++r) {
    StepK k;
    double ef, eb, pf, pb;
    step_rates(A, tb, X, ln, q, r, A.strength, false, k, ef, eb, pf, pb);
    const double rf = ef * pf, rb = eb * pb, ne = A.ne[r];
    ti = ti + ne * (rf - rb);
    tg = tg + fabs(ne) * (rf + rb);
  }
}

// the program of one lane
struct Program {
  double Es, Ev, tau, phi0;
};

__device__ __forceinline__ double potential_at(const Program& pg, int k, double t) {
  const bool back = k & 1;
  const double Ea = back ? pg.Ev : pg.Es, Ez = back ? pg.Es : pg.Ev;
  return Ea + (Ez - Ea) * ((t - (double)k * pg.tau) / pg.tau);
}

__device__ __forceinline__ double output_time(const Program& pg, int K, int64_t j) {
  const int k = (int)(j / K), m = (int)(j - (int64_t)k * K) + 1;
  return ((double)k + (double)m / (double)K) * pg.tau;
}

__device__ __forceinline__ void set_potential(const KArgs& A, Lane& ln, const Program& pg, int64_t i, double E) {
  ln.pt.V = E - (A.w ? pg.phi0 : 0.0);
  ln.pt.sg = A.use_sigma ? A.sigma[i] : A.CS * ((E - A.pzc) - pg.phi0);
}

__global__ __launch_bounds__(64) void sweep_kernel(const KArgs A, const Table* __restrict__ tab) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1, K = A.K, G = A.G, S = T - G;
  const int64_t n_out = A.n_out;
  const Table& tb = *tab;   // its own read-only argument: the uniform reads become scalar loads
  const Extra& X = *A.ext;
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
    // ---- the program: a sweep, or a hold at E_start ----
    Program pg;
    pg.Es = A.phiM[i];
    pg.Ev = A.Ev[i];
    pg.phi0 = A.from_view ? A.phi[(size_t)b * A.ldx] : A.phis[i];
    const double rate = A.rate[i];
    const double hold = A.hold ? A.hold[i] : 0.0;
    const bool holds = pg.Ev == pg.Es && hold > 0.0 && finite_(hold);
    pg.tau = holds ? hold : fabs(pg.Ev - pg.Es) / rate;
    ok = ok && finite_(pg.Ev) && pg.tau > 0.0 && finite_((double)A.nseg * pg.tau);
    const double i_floor = A.floor_ * rate;
    // ---- start: the adsorbates as given and the free sites from the balances, or the ramped steady state at E_start ----
    if (A.theta0) {
      double u0 = 0.0, u1 = 0.0, u2 = 0.0;
      for (int t = G; t < T; ++t) {
        const double g = A.theta0[i * T + t];
        ok = ok && finite_(g);
        const double y = log_coverage(g);
        L[(ln.oYn + t) * 64] = y;
        const int gt = X.site_of[t];
        const double v = tb.ns[t] * exp(y);
        u0 = u0 + (gt == 0 ? v : 0.0);
        u1 = u1 + (gt == 1 ? v : 0.0);
        u2 = u2 + (gt == 2 ? v : 0.0);
      }
      for (int g = 0; g < G; ++g) {
        const double free_ = X.x[g] - pick(g, u0, u1, u2);
        ok = ok && free_ > 0.0;
        L[(ln.oYn + g) * 64] = log_coverage(free_);
      }
    }
    for (int t = 0; t < T; ++t) {
      const int g = X.site_of[t];
      double nsum = 0.0;
      for (int u = 0; u < T; ++u) nsum = nsum + (X.site_of[u] == g ? tb.ns[u] : 0.0);
      const double y0 = log(X.x[g] / nsum);
      L[(ln.oY + t) * 64] = A.theta0 && ok ? L[(ln.oYn + t) * 64] : y0;
      L[(ln.oY1 + t) * 64] = y0;   // kept for a lane whose start fails
    }
    if (!A.theta0) {
      bool go = ok && live;
      int s0 = STATUS_MAXIT;
      for (int k = 0; k < A.ramp; ++k) {
        if (__ballot(go) == 0) break;
        const double lam = k == A.ramp - 1 ? A.strength : (A.strength * (double)k) / (double)(A.ramp - 1);
        const int st = stage_newton(A, tb, X, ln, lam, go);
        if (go) {
          s0 = st;
          go = st == STATUS_CONVERGED;
        }
      }
      ok = ok && s0 == STATUS_CONVERGED;
    }
    for (int t = 0; t < T; ++t) {
      const double y = ok ? L[(ln.oY + t) * 64] : L[(ln.oY1 + t) * 64];
      L[(ln.oYn + t) * 64] = y;
      L[(ln.oY + t) * 64] = y;
    }
    // ---- first step size ----
    raw_rows(A, tb, X, ln, A.strength, false);
    double fastest = 0.0;
    for (int s = G; s < T; ++s) {
      const double D = L[(ln.oD + s) * 64];
      const double q = D > 0.0 ? D / exp(L[(ln.oY + s) * 64]) : 0.0;
      fastest = q > fastest ? q : fastest;
    }
    double h = A.h0 > 0.0 ? A.h0 : (fastest > 0.0 ? 0.01 / fastest : output_time(pg, K, 0));
    double t_now = 0.0, q_sum = 0.0;
    int64_t k = 0;   // output rows written
    int n_acc = 0, n_rej = 0, n_it = 0, n_plain = 0;
    int status = ok ? RUNNING : CATIS_INPUT;
    bool active = ok && live;

    // ---- the step loop: one attempted step of every running lane per trip ----
    for (;;) {
      if (active && (n_acc + n_rej >= A.max_steps || !(h >= CATIS_MIN_STEP))) {
        status = CATIS_STEPS;
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
      const bool ok1 = be_solve(A, tb, X, ln, hh, active, n_it);
      double i1, g1;
      turnover(A, tb, X, ln, i1, g1);
      // ya = BE(y, hh / 2) at E_mid
      for (int t = 0; t < T; ++t) {
        L[(ln.oY1 + t) * 64] = L[(ln.oY + t) * 64];
        L[(ln.oY + t) * 64] = L[(ln.oYn + t) * 64];
      }
      set_potential(A, ln, pg, i, E_mid);
      const bool oka = be_solve(A, tb, X, ln, half, active && ok1, n_it);
      double ia, ga;
      turnover(A, tb, X, ln, ia, ga);
      // yb = BE(ya, hh / 2) at E_end
      for (int t = 0; t < T; ++t) L[(ln.oTo + t) * 64] = exp(L[(ln.oY + t) * 64]);
      set_potential(A, ln, pg, i, E_end);
      const bool okb = be_solve(A, tb, X, ln, half, active && ok1 && oka, n_it);
      double ib, gb;
      turnover(A, tb, X, ln, ib, gb);
      const bool solved = ok1 && oka && okb;
      // the error of the coverages and of the turnover; the extrapolated coverages into the theta_old slots, the adsorbates from the
      // last one down, then the free site of every type from its balance
      double err = 0.0, u0 = 0.0, u1 = 0.0, u2 = 0.0;
      bool positive = true;
      for (int t = T - 1; t >= 0; --t) {
        const double thb = exp(L[(ln.oY + t) * 64]), th1 = exp(L[(ln.oY1 + t) * 64]);
        const double d = fabs(thb - th1) / (A.atol + A.rtol * (thb > th1 ? thb : th1));
        err = d > err || d != d ? d : err;
        const int gt = X.site_of[t];
        const double the = t >= G ? 2.0 * thb - th1 : X.x[t] - pick(t, u0, u1, u2);
        const double v = tb.ns[t] * the;
        u0 = u0 + (gt == 0 ? v : 0.0);
        u1 = u1 + (gt == 1 ? v : 0.0);
        u2 = u2 + (gt == 2 ? v : 0.0);
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
      // ---- an output time (the lane's potential is that of the end of the step): turnover, fluxes and shifts at the accepted state;
      // ---- the first N slots of J are free ----
      const Resp q = surface_state(tb, X, ln, T);
      double io = 0.0, go = 0.0;
      for (int j = 0; j < N; ++j) L[(ln.oC + j) * 64] = 0.0, L[(ln.oJ + j) * 64] = 0.0;
      for (int r = 0; r < A.R; ++r) {
        StepK sk;
        double ef, eb, pf, pb;
        step_rates(A, tb, X, ln, q, r, A.strength, false, sk, ef, eb, pf, pb);
        const double rf = ef * pf, rb = eb * pb, net = rf - rb, gross = rf + rb;
        const double ne = A.ne[r];
        io = io + ne * net;
        go = go + fabs(ne) * gross;
        for (int j = 0; j < N; ++j) {
          const double nu = tb.nu[r][j];
          if (nu != 0.0) {
            L[(ln.oC + j) * 64] = L[(ln.oC + j) * 64] + nu * net;
            L[(ln.oJ + j) * 64] = L[(ln.oJ + j) * 64] + fabs(nu) * gross;
          }
        }
      }
      if (write) {
        const size_t row = (size_t)i * n_out + k;
        if (A.theta)
          for (int t = 0; t < T; ++t) A.theta[row * T + t] = exp(L[(ln.oY + t) * 64]);
        for (int j = 0; j < N; ++j) {
          if (A.flux) A.flux[row * N + j] = A.sd * L[(ln.oC + j) * 64];
          if (A.fscale) A.fscale[row * N + j] = A.sd * L[(ln.oJ + j) * 64];
        }
        if (A.eshift)
          for (int a = 0; a < S; ++a) {
            double e = 0.0;
            for (int u = 0; u < S; ++u) e = e + X.eps[a][u] * weight(X, ln, q, G + u);
            A.eshift[row * S + a] = A.strength * e;
          }
        if (A.cur) A.cur[row] = -(A.Fsd * io);
        if (A.cscale) A.cscale[row] = A.Fsd * go;
        if (A.charge) A.charge[row] = -(A.Fsd * q_sum);
        if (A.eout) A.eout[row] = E_end;
        ++k;
        if (k == n_out) {
          status = CATIS_DONE;
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
      if (A.eshift)
        for (int a = 0; a < S; ++a) A.eshift[row * S + a] = bad_number;
      if (A.cur) A.cur[row] = bad_number;
      if (A.cscale) A.cscale[row] = bad_number;
      if (A.charge) A.charge[row] = bad_number;
      if (A.eout) A.eout[row] = bad_number;
    }
    if (live) {
      if (A.treached) A.treached[i] = status == CATIS_INPUT ? bad_number : t_now;
      if (A.status) A.status[i] = status;
      if (A.steps) A.steps[i * 4] = n_acc, A.steps[i * 4 + 1] = n_rej, A.steps[i * 4 + 2] = n_it, A.steps[i * 4 + 3] = n_plain;
    }
  }
}

static size_t lds_bytes(int N, int T) { return (size_t)(std::max(T * T, N) + 7 * T + 2 * N) * 64 * sizeof(double); }

// catis_params as the shared host code reads it: the start potentials under the name the other libraries give the potential
struct Params : catis_params {
  const double* phiM;
};

// the checks of catint_interact.h on the members it brings; 0 or the code.  T = G + S is known to be within the limits
static int check_interactions(Ctx* ctx, const catis_params* p) {
  char msg[256];
  const int G = p->nsitetypes, S = p->nadsorbates, R = p->nsteps, T = G + S;
  if (p->start_ramp < 1) return fail(ctx, ERR_INVAL, "catis_solve: start_ramp < 1");
  if (p->response != CATIA_LINEAR && p->response != CATIA_PIECEWISE) return fail(ctx, ERR_INVAL, "catis_solve: response is 0 (linear) or 1 (piecewise)");
  if (!std::isfinite(p->strength)) return fail(ctx, ERR_INVAL, "catis_solve: strength is not finite");
  if (!p->site_of || !p->site_fraction || !p->eps) return fail(ctx, ERR_INVAL, "catis_solve: site_of, site_fraction and eps are required");
  for (int g = 0; g < G; ++g)
    if (!posfin(p->site_fraction[g])) {
      snprintf(msg, sizeof msg, "catis_solve: site_fraction[%d] must be positive and finite", g);
      return fail(ctx, ERR_INVAL, msg);
    }
  for (int t = 0; t < T; ++t) {
    const int g = p->site_of[t];
    if (g < 0 || g >= G) {
      snprintf(msg, sizeof msg, "catis_solve: site_of[%d] = %d outside [0, %d)", t, g, G);
      return fail(ctx, ERR_INVAL, msg);
    }
    if (t < G && (g != t || (p->site_count && p->site_count[t] != 1.0))) {
      snprintf(msg, sizeof msg, "catis_solve: column %d is the free site of type %d: site_of must be %d and its site count 1", t, t, t);
      return fail(ctx, ERR_INVAL, msg);
    }
  }
  for (int e = 0; e < S * S; ++e)
    if (!std::isfinite(p->eps[e])) return fail(ctx, ERR_INVAL, "catis_solve: eps has a non-finite entry");
  if (p->eps_ts)
    for (int e = 0; e < R * S; ++e)
      if (!std::isfinite(p->eps_ts[e])) return fail(ctx, ERR_INVAL, "catis_solve: eps_ts has a non-finite entry");
  if (p->response == CATIA_PIECEWISE) {
    if (!p->cutoff || !p->smoothing) return fail(ctx, ERR_INVAL, "catis_solve: the piecewise response needs cutoff and smoothing");
    for (int g = 0; g < G; ++g)
      if (!std::isfinite(p->cutoff[g]) || !posfin(p->smoothing[g])) {
        snprintf(msg, sizeof msg, "catis_solve: type %d needs a finite cutoff and a positive, finite smoothing", g);
        return fail(ctx, ERR_INVAL, msg);
      }
  }
  return OK;
}

// every step conserves the sites of each type; after check_tables (the tables are there, the orders and site counts are in range)
static int check_type_balance(Ctx* ctx, const catis_params* p) {
  char msg[256];
  const int N = p->nspecies, G = p->nsitetypes, R = p->nsteps, T = G + p->nadsorbates, M = N + T;
  for (int r = 0; r < R; ++r)
    for (int g = 0; g < G; ++g) {
      double sites = 0.0;
      for (int t = 0; t < T; ++t)
        if (p->site_of[t] == g) sites += p->site_count[t] * (p->order_b[r * M + N + t] - p->order_f[r * M + N + t]);
      if (sites != 0.0) {
        snprintf(msg, sizeof msg, "catis_solve: step %d does not conserve the sites of type %d", r, g);
        return fail(ctx, ERR_INVAL, msg);
      }
    }
  return OK;
}

static void fill_extra(Extra* X, const catis_params* p) {
  const int N = p->nspecies, G = p->nsitetypes, S = p->nadsorbates, R = p->nsteps, T = G + S, M = N + T;
  memset(X, 0, sizeof *X);
  X->G = G;
  X->mode = p->response;
  for (int t = 0; t < T; ++t) X->site_of[t] = p->site_of[t], X->nx[t] = p->site_count[t] / p->site_fraction[p->site_of[t]];
  for (int g = 0; g < G; ++g) {
    X->x[g] = p->site_fraction[g];
    if (p->response == CATIA_PIECEWISE) X->cutoff[g] = p->cutoff[g], X->smooth[g] = p->smoothing[g];
  }
  for (int a = 0; a < S; ++a)
    for (int u = 0; u < S; ++u) X->eps[a][u] = p->eps[a * S + u];
  for (int r = 0; r < R; ++r)
    for (int u = 0; u < S; ++u) {
      double g = 0.0, f = 0.0;
      for (int a = 0; a < S; ++a) {
        const int of = p->order_f[r * M + N + G + a], ob = p->order_b[r * M + N + G + a];
        g = g + (double)(ob - of) * p->eps[a * S + u];
        f = f + (double)of * p->eps[a * S + u];
      }
      X->eg[r][u] = g;
      X->ea[r][u] = (p->eps_ts ? p->eps_ts[r * S + u] : 0.0) - f;
    }
}

}  // namespace catis

static_assert(CATIS_OK == pnp::post::OK && CATIS_EINVAL == pnp::post::ERR_INVAL && CATIS_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATIS_EDEVICE == pnp::post::ERR_DEVICE,
              "catint_iasweep.h and pnp_post.h disagree");
static_assert(CATIS_INPUT == pnp::kin::STATUS_INPUT && CATIS_DONE == CATVM_DONE && CATIS_INPUT == CATVM_INPUT && CATIS_STEPS == CATVM_STEPS &&
                  CATIS_MAX_STEPS == CATVM_MAX_STEPS && CATIS_MAX_SEGMENTS == CATVM_MAX_SEGMENTS && CATIS_MAX_SAMPLES == CATVM_MAX_SAMPLES &&
                  CATIS_START_MAXIT == CATVM_START_MAXIT,
              "catint_iasweep.h, catint_voltam.h and pnp_kin.h disagree");
static_assert(CATIA_MAX_SPECIES == pnp::kin::MAXN && CATIA_MAX_COLUMNS == pnp::kin::MAXT && CATIA_MAX_STEPS == pnp::kin::MAXR &&
                  CATIA_MAX_ORDER == pnp::kin::MAX_ORDER && CATIA_MIN_LOG == pnp::kin::MINLOG && CATIA_MAX_SITE_TYPES <= 3,
              "catint_interact.h and pnp_kin.h disagree");

struct catis_ctx : pnp::post::Ctx {};

extern "C" {

int catis_create(int32_t device, catis_ctx** out) { return pnp::post::create("catis_create", device, out); }
void catis_destroy(catis_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catis_last_error(const catis_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catis_last_kernel(const catis_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catis_last_kernel_ms(const catis_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catis_solve(catis_ctx* ctx, const pnp_device_view* view, const catis_params* p, const catis_outputs* out) {
  using namespace catis;
  static const char entry[] = "catis_solve";
  char msg[256];
  if (!ctx) return CATIS_EINVAL;
  if (!p || !out) return fail(ctx, CATIS_EINVAL, "catis_solve: null argument");
  if (p->struct_size != (int32_t)sizeof(catis_params)) return fail(ctx, CATIS_EINVAL, "catis_solve: catis_params.struct_size does not match this library");
  const int G = p->nsitetypes, S = p->nadsorbates;
  if (G < 1 || G > MAXG) {
    snprintf(msg, sizeof msg, "catis_solve: %d site types outside [1, %d]", G, MAXG);
    return fail(ctx, CATIS_EINVAL, msg);
  }
  if (S < 1 || G + S > MAXT) {
    snprintf(msg, sizeof msg, "catis_solve: %d adsorbates on %d site types: at least 1, and at most %d columns", S, G, MAXT);
    return fail(ctx, CATIS_EINVAL, msg);
  }
  // pnp_kin.h reads a model as one first column and S behind it: here T - 1 behind the free site of type 0
  catis_params q0 = *p;
  q0.nadsorbates = G + S - 1;
  if (const int rc = check_sizes(ctx, entry, "catis_params", "catis_outputs", &q0, out)) return rc;
  if (p->newton_maxit < 1) return fail(ctx, CATIS_EINVAL, "catis_solve: newton_maxit < 1");
  if (p->max_steps < 1 || p->max_steps > CATIS_MAX_STEPS) {
    snprintf(msg, sizeof msg, "catis_solve: max_steps outside [1, %d]", CATIS_MAX_STEPS);
    return fail(ctx, CATIS_EINVAL, msg);
  }
  if (const int rc = check_drop(ctx, entry, p)) return rc;
  if (!posfin(p->rtol)) return fail(ctx, CATIS_EINVAL, "catis_solve: rtol must be positive and finite");
  if (!posfin(p->newton_tol)) return fail(ctx, CATIS_EINVAL, "catis_solve: newton_tol must be positive and finite");
  if (!(p->atol >= 0.0) || !std::isfinite(p->atol)) return fail(ctx, CATIS_EINVAL, "catis_solve: atol must be finite and not negative");
  if (!(p->rate_floor >= 0.0) || !std::isfinite(p->rate_floor))
    return fail(ctx, CATIS_EINVAL, "catis_solve: rate_floor must be finite and not negative");
  if (p->h0 != p->h0) return fail(ctx, CATIS_EINVAL, "catis_solve: h0 is not a number");
  if (p->n_segments < 1 || p->n_segments > CATIS_MAX_SEGMENTS) {
    snprintf(msg, sizeof msg, "catis_solve: n_segments outside [1, %d]", CATIS_MAX_SEGMENTS);
    return fail(ctx, CATIS_EINVAL, msg);
  }
  if (p->samples < 1 || p->samples > CATIS_MAX_SAMPLES) {
    snprintf(msg, sizeof msg, "catis_solve: samples outside [1, %d]", CATIS_MAX_SAMPLES);
    return fail(ctx, CATIS_EINVAL, msg);
  }
  if (!p->E_start || !p->E_vertex || !p->scan_rate) return fail(ctx, CATIS_EINVAL, "catis_solve: E_start, E_vertex and scan_rate are required");
  if (p->n < 0) return fail(ctx, CATIS_EINVAL, "catis_solve: n < 0");
  for (int64_t i = 0; i < p->n; ++i)
    if (!posfin(p->scan_rate[i])) {
      snprintf(msg, sizeof msg, "catis_solve: scan_rate[%lld] must be positive and finite", (long long)i);
      return fail(ctx, CATIS_EINVAL, msg);
    }
  if (const int rc = check_interactions(ctx, p)) return rc;
  Params q;
  static_cast<catis_params&>(q) = q0;
  q.phiM = p->E_start;
  if (const int rc = check_tables(ctx, entry, &q)) return rc;
  if (const int rc = check_type_balance(ctx, p)) return rc;
  if (!p->electrons) return fail(ctx, CATIS_EINVAL, "catis_solve: electrons is required");
  for (int r = 0; r < p->nsteps; ++r)
    if (!std::isfinite(p->electrons[r])) {
      snprintf(msg, sizeof msg, "catis_solve: electrons[%d] is not finite", r);
      return fail(ctx, CATIS_EINVAL, msg);
    }
  bool from_view = false;
  if (const int rc = check_points(ctx, entry, view, &q, &from_view)) return rc;
  if (p->n == 0) return CATIS_OK;

  const int N = p->nspecies, R = p->nsteps, T = G + S;
  const size_t sn = (size_t)p->n, so = (size_t)p->n_segments * (size_t)p->samples;
  KArgs a;
  set_args(a, view, &q, from_view);
  a.G = G;
  a.ramp = p->start_ramp;
  a.strength = p->strength;
  // the program arrays, the electrons and the interaction table behind the staged inputs of the shared layout: one copy still
  Stage stage;
  int i_ev = 0, i_rate = 0, i_ne = 0, i_hold = -1, i_x = -1;
  if (const int rc = stage_inputs(ctx, entry, &q, a, p->theta0, &a.theta0, from_view, 5, &stage, [&](Inputs& in) {
        i_ev = in.add(sn, &a.Ev);
        i_rate = in.add(sn, &a.rate);
        i_ne = in.add((size_t)R, &a.ne);
        if (p->hold_time) i_hold = in.add(sn, &a.hold);
        i_x = in.add_unpadded(sizeof(Extra) / 8, &a.ext);
      }))
    return rc;   // status and the four counters
  memcpy(stage.in.host(ctx->stage, i_ev), p->E_vertex, sn * sizeof(double));
  memcpy(stage.in.host(ctx->stage, i_rate), p->scan_rate, sn * sizeof(double));
  memcpy(stage.in.host(ctx->stage, i_ne), p->electrons, (size_t)R * sizeof(double));
  if (p->hold_time) memcpy(stage.in.host(ctx->stage, i_hold), p->hold_time, sn * sizeof(double));
  fill_extra(reinterpret_cast<Extra*>(stage.in.host(ctx->stage, i_x)), p);
  a.nmaxit = p->newton_maxit;
  a.max_steps = p->max_steps;
  a.maxit = CATIS_START_MAXIT;
  a.nseg = p->n_segments;
  a.K = p->samples;
  a.n_out = (int64_t)so;
  a.rtol = p->rtol;
  a.atol = p->atol;
  a.ntol = p->newton_tol;
  a.tol = p->newton_tol;
  a.h0 = p->h0;
  a.floor_ = p->rate_floor;
  a.Fsd = CATIS_FARADAY * p->site_density;
  const Row rows[] = {{out->theta, &a.theta, sn * so * T},       {out->current, &a.cur, sn * so},    {out->current_scale, &a.cscale, sn * so},
                      {out->charge, &a.charge, sn * so},         {out->E_out, &a.eout, sn * so},     {out->flux, &a.flux, sn * so * N},
                      {out->flux_scale, &a.fscale, sn * so * N}, {out->t_reached, &a.treached, sn},  {out->energy_shift, &a.eshift, sn * so * S}};
  if (!rows_doubles(rows) && !out->status && !out->steps) return CATIS_OK;
  const int rc = run(ctx, entry, "catis::sweep_kernel", sweep_kernel, view, &q, stage, a, rows, lds_bytes(N, T), 5, out->status || out->steps,
                     [&](int32_t* flags) {
                       a.status = flags;
                       a.steps = flags + sn;
                     });
  if (rc) return rc;
  if (out->status) memcpy(out->status, ctx->flags.data(), sn * sizeof(int32_t));
  if (out->steps) memcpy(out->steps, ctx->flags.data() + sn, 4 * sn * sizeof(int32_t));
  return CATIS_OK;
}

}  // extern "C"
