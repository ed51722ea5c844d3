// libcatint_interact (include/catint_interact.h): the steady state of a surface microkinetic model with lateral interactions and up to
// three site types per operating point -- the damped Newton iteration of libcatint_kinetics with coverage-dependent rate constants and
// one site row per type, the interaction strength ramped in stages inside the launch -- and the wall fluxes and their sensitivities.
// gfx950 / MI355X only.
//
// Mapping, working set, tables and arithmetic: ../pnp_kin.h (one operating point per lane, everything indexed at run time in LDS as
// [slot][lane], tables read at wave-uniform addresses, contraction off).  From that header come the point's inputs, the factors of a
// rate, the row scaling with the dead-row rule and the per-lane LU; the rate constants, the rows and the iteration are this file's, since
// here ln k depends on the coverages.  The shifts dE_t enter the rate constants only through the per-step contractions EG[r][u] and
// EA[r][u] (the header), formed once on the host, so the kernel keeps neither dE nor d dE / d theta: what the Jacobian needs of them is
// one number per (step, column), formed where it is used.  The response factors f_g, f'_g and the per-type sums of a step are scalars
// picked by compares on a wave-uniform type index, never an indexed register array.
// LDS slots: those of the kinetics library (J[T][T] or N, y[T], right-hand side [T], D[T], a[N], N accumulators) plus theta[T] and
// w[T] = f theta.  At S = 8, G = 1, N = 8: 142 slots x 512 B = 71 KB per wave, two waves per CU.
#include "../../../include/catint_interact.h"
#include "../pnp_kin.h"

#pragma clang fp contract(off)

namespace catia {

using namespace pnp::kin;

constexpr int MAXG = CATIA_MAX_SITE_TYPES;

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
  int32_t N, S, R, maxit, w, use_sigma, sens, from_view, ldx, G, K, pad_;   // S: T - 1, the columns behind the first (as pnp_kin.h reads it)
  int64_t n;
  const double* c;
  const double* phi;
  const int32_t* st;
  const int64_t* lanes;
  const double *cs, *phis;
  const double *phiM, *sigma, *off, *gamma, *guess;
  const Extra* ext;
  double *theta, *rate, *gross, *flux, *fscale, *dfdc, *dfdphi, *eshift;
  int32_t *status, *iters, *reached;
  double sd, tol, CS, pzc, strength;
};

// a lane's slots: SteadyLane's, then theta[T] and w[T]
struct Lane : SteadyLane {
  int oTh, oW;
};

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

// theta_t = exp(y_t) and w_t = f_g(t) theta_t (0 for a free site) into the lane's slots; the response of every type
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
  for (int t = 0; t < T; ++t)
    L[(ln.oW + t) * 64] = t >= G ? pick(X.site_of[t], q.f0, q.f1, q.f2) * L[(ln.oTh + t) * 64] : 0.0;
  return q;
}

// what a step's rate constants are at the lane's coverages: ln kf, ln kb, the branch of Ga, and (piecewise mode, want_q) the per-type
// sums sum_{u on g} E[r][u] theta_u of the dG row (qg) and of the row of the branch (qs)
struct StepK {
  double lf, lb, qg0, qg1, qg2, qs0, qs1, qs2;
  int br;
};

template <class KA>
__device__ __forceinline__ void step_constants(const KA& A, const Table& tb, const Extra& X, const Lane& ln, int r, double lam, bool want_q, StepK& k) {
  const double* L = ln.L;
  const int G = X.G, S = A.S + 1 - G;
  const double V = ln.pt.V, sg = ln.pt.sg, s2 = sg * sg;
  const double dG0 = ((tb.dg[r][0] + tb.dg[r][1] * V) + tb.dg[r][2] * sg) + tb.dg[r][3] * s2;
  const double Ea0 = ((tb.ea[r][0] + tb.ea[r][1] * V) + tb.ea[r][2] * sg) + tb.ea[r][3] * s2;
  const bool ts = tb.ea[r][0] != -INFINITY;
  double sG = 0.0, sA = 0.0;
  for (int a = 0; a < S; ++a) {
    const double w = L[(ln.oW + G + a) * 64];
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

// rf and rb of step r as their two factors; the theta and w slots hold the lane's surface state
template <class KA>
__device__ __forceinline__ void step_rates(const KA& A, const Table& tb, const Extra& X, const Lane& ln, int r, double lam, int skip, bool want_q, StepK& k,
                                           double& ef, double& eb, double& pf, double& pb) {
  step_constants(A, tb, X, ln, r, lam, want_q, k);
  rate_factors(tb, A.N, A.S + 1, ln.at(ln.oY), ln.at(ln.oA), r, k.lf, k.lb, skip, ef, eb, pf, pb);
}

// J (scaled rows, one site row per type first), right-hand side -F and the row scales D at the lane's y and the strength lam; leaves
// theta and w of that y in their slots
template <class KA>
__device__ __forceinline__ Resp assemble(const KA& A, const Table& tb, const Extra& X, const Lane& ln, double lam) {
  const int N = A.N, T = A.S + 1, G = X.G;
  double* L = ln.L;
  const Resp q = surface_state(tb, X, ln, T);
  for (int s = 0; s < T * T; ++s) L[(ln.oJ + s) * 64] = 0.0;
  for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0, L[(ln.oD + s) * 64] = 0.0;
  for (int r = 0; r < A.R; ++r) {
    StepK k;
    double ef, eb, pf, pb;
    step_rates(A, tb, X, ln, r, lam, -1, true, k, ef, eb, pf, pb);
    const double rf = ef * pf, rb = eb * pb, net = rf - rb, gross = rf + rb;
    for (int s = G; s < T; ++s) {
      const int m = tb.ob[r][N + s] - tb.of[r][N + s];
      if (m == 0) continue;
      L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + (double)m * net;
      L[(ln.oD + s) * 64] = L[(ln.oD + s) * 64] + fabs((double)m) * gross;
    }
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
  for (int s = G; s < T; ++s) {
    const double D = L[(ln.oD + s) * 64];
    const bool dead = scale_row(ln.at(ln.oJ), ln.at(ln.oY), T, s, D);
    const double g = L[(ln.oB + s) * 64];
    L[(ln.oB + s) * 64] = dead ? 0.0 : -(g / D);
  }
  for (int g = 0; g < G; ++g) {
    double f = 0.0;
    for (int t = 0; t < T; ++t) {
      const bool on = X.site_of[t] == g;
      const double th = tb.ns[t] * exp(L[(ln.oY + t) * 64]);
      L[(ln.oJ + g * T + t) * 64] = on ? th / X.x[g] : 0.0;
      f = f + (on ? th : 0.0);
    }
    L[(ln.oB + g) * 64] = -(f / X.x[g] - 1.0);
  }
  return q;
}

// One stage: the damped Newton iteration of pnp_kin.h (steady_newton) at the strength lam from the y in the lane's slots.  Returns the
// stage's status for a lane that runs; it: its iterations
template <class KA>
__device__ __forceinline__ int stage_newton(const KA& A, const Table& tb, const Extra& X, const Lane& ln, double lam, bool run, int& it) {
  const int T = A.S + 1;
  double* L = ln.L;
  int status = STATUS_MAXIT;
  bool active = run;
  it = 0;
  for (int iter = 0; iter < A.maxit; ++iter) {
    if (__ballot(active) == 0) break;
    assemble(A, tb, X, ln, lam);
    uint64_t pivs;
    const bool bad = factor(ln.at(ln.oJ), T, pivs);
    substitute(ln.at(ln.oJ), ln.at(ln.oB), T, pivs);
    double mx = 0.0;
    for (int t = 0; t < T; ++t) {
      const double d = fabs(L[(ln.oB + t) * 64]);
      mx = d > mx || d != d ? d : mx;
    }
    const double sc = mx > 3.0 ? 3.0 / mx : 1.0;
    const bool move = active && !bad;
    for (int t = 0; t < T; ++t) {
      const double y = L[(ln.oY + t) * 64];
      const double v = y + sc * L[(ln.oB + t) * 64];
      L[(ln.oY + t) * 64] = move ? (v < MINLOG ? MINLOG : v) : y;
    }
    if (active) {
      if (bad) {
        status = STATUS_PIVOT;
        active = false;
      } else {
        ++it;
        if (mx < A.tol) {
          status = STATUS_CONVERGED;
          active = false;
        }
      }
    }
  }
  return status;
}

__global__ __launch_bounds__(64) void interact_kernel(const KArgs A, const Table* __restrict__ tab) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1, R = A.R, G = A.G, S = T - G;
  const Table& tb = *tab;
  const Extra& X = *A.ext;
  Lane ln;
  steady_slots(ln, lds, lane, N, T);
  ln.oTh = ln.oC + N;
  ln.oW = ln.oTh + T;
  double* L = ln.L;
  const double bad_number = __builtin_nan("");

  for (int64_t grp = blockIdx.x; grp * 64 < A.n; grp += gridDim.x) {
    const bool live = grp * 64 + lane < A.n;
    const int64_t i = live ? grp * 64 + lane : A.n - 1;
    const int64_t b = A.lanes[i];
    ln.pt = point_inputs(A, tb, i, b, ln.at(ln.oA));
    bool ok = ln.pt.ok;
    // ---- start ----
    if (A.guess)
      for (int t = 0; t < T; ++t) ok = ok && finite_(A.guess[i * T + t]);
    for (int t = 0; t < T; ++t) {
      const int g = X.site_of[t];
      double nsum = 0.0;
      for (int u = 0; u < T; ++u) nsum = nsum + (X.site_of[u] == g ? tb.ns[u] : 0.0);
      const double y0 = log(X.x[g] / nsum);
      L[(ln.oY + t) * 64] = A.guess && ok ? log_coverage(A.guess[i * T + t]) : y0;
    }
    // ---- the ramp: one Newton iteration per stage, each from the y of the stage before ----
    int status = ok ? CATIA_MAXIT : CATIA_INPUT, it = 0, reached = 0;
    bool go = ok && live;
    double lam_end = A.K == 1 ? A.strength : 0.0;
    for (int k = 0; k < A.K; ++k) {
      if (__ballot(go) == 0) break;
      const double lam = k == A.K - 1 ? A.strength : (A.strength * (double)k) / (double)(A.K - 1);
      int its;
      const int st = stage_newton(A, tb, X, ln, lam, go, its);
      if (go) {
        it += its;
        status = st;
        reached = k;
        lam_end = lam;
        go = st == CATIA_CONVERGED;
      }
    }
    const bool nan = status == CATIA_INPUT;

    // ---- coverages, rates, fluxes, shifts at the lane's y and the strength it ended with (the J slots are free) ----
    if (A.theta && live)
      for (int t = 0; t < T; ++t) A.theta[i * T + t] = nan ? bad_number : exp(L[(ln.oY + t) * 64]);
    if (A.rate || A.gross || A.flux || A.fscale || A.eshift) surface_state(tb, X, ln, T);
    if (A.rate || A.gross || A.flux || A.fscale) {
      for (int k = 0; k < N; ++k) L[(ln.oC + k) * 64] = 0.0, L[(ln.oJ + k) * 64] = 0.0;
      for (int r = 0; r < R; ++r) {
        StepK sk;
        double ef, eb, pf, pb;
        step_rates(A, tb, X, ln, r, lam_end, -1, false, sk, ef, eb, pf, pb);
        const double rf = ef * pf, rb = eb * pb, net = rf - rb, gross = rf + rb;
        if (A.rate && live) A.rate[i * R + r] = nan ? bad_number : net;
        if (A.gross && live) A.gross[i * R + r] = nan ? bad_number : gross;
        for (int k = 0; k < N; ++k) {
          const double nu = tb.nu[r][k];
          if (nu != 0.0) {
            L[(ln.oC + k) * 64] = L[(ln.oC + k) * 64] + nu * net;
            L[(ln.oJ + k) * 64] = L[(ln.oJ + k) * 64] + fabs(nu) * gross;
          }
        }
      }
      for (int k = 0; k < N; ++k) {
        if (A.flux && live) A.flux[i * N + k] = nan ? bad_number : A.sd * L[(ln.oC + k) * 64];
        if (A.fscale && live) A.fscale[i * N + k] = nan ? bad_number : A.sd * L[(ln.oJ + k) * 64];
      }
    }
    if (A.eshift && live)
      for (int a = 0; a < S; ++a) {
        double e = 0.0;
        for (int u = 0; u < S; ++u) e = e + X.eps[a][u] * L[(ln.oW + G + u) * 64];
        A.eshift[i * S + a] = nan ? bad_number : lam_end * e;
      }

    // ---- sensitivities: the full J at the lane's y factorised once, one right-hand side after another ----
    if (A.sens) {
      const Resp q = assemble(A, tb, X, ln, lam_end);
      uint64_t pivs;
      const bool bad = factor(ln.at(ln.oJ), T, pivs);
      if (bad && status != CATIA_INPUT) status = CATIA_PIVOT;
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
          StepK sk;
          double ef, eb, pf, pb, drf, drb;
          if (p < N) {
            const int of = tb.of[r][p], ob = tb.ob[r][p];
            if (of == 0 && ob == 0) continue;
            step_rates(A, tb, X, ln, r, lam_end, p, false, sk, ef, eb, pf, pb);
            drf = of ? ef * ((double)of * pf * dadc) : 0.0;
            drb = ob ? eb * ((double)ob * pb * dadc) : 0.0;
          } else {
            double dlf, dlb;
            step_rates(A, tb, X, ln, r, lam_end, -1, false, sk, ef, eb, pf, pb);
            rate_constant_slopes(tb, ln.pt.sg, r, sk.br, dV, ds, dlf, dlb);
            drf = (ef * pf) * dlf;
            drb = (eb * pb) * dlb;
          }
          const double dnet = drf - drb;
          for (int s = G; s < T; ++s) {
            const int m = tb.ob[r][N + s] - tb.of[r][N + s];
            if (m) L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + (double)m * dnet;
          }
          for (int k = 0; k < N; ++k) {
            const double nu = tb.nu[r][k];
            if (nu != 0.0) L[(ln.oC + k) * 64] = L[(ln.oC + k) * 64] + nu * dnet;
          }
        }
        for (int s = G; s < T; ++s) {
          const double D = L[(ln.oD + s) * 64];
          L[(ln.oB + s) * 64] = D == 0.0 ? 0.0 : -(L[(ln.oB + s) * 64] / D);
        }
        substitute(ln.at(ln.oJ), ln.at(ln.oB), T, pivs);
        for (int r = 0; r < R; ++r) {
          StepK sk;
          double ef, eb, pf, pb;
          step_rates(A, tb, X, ln, r, lam_end, -1, true, sk, ef, eb, pf, pb);
          const double rf = ef * pf, rb = eb * pb;
          double ws = 0.0;
          for (int t = 0; t < T; ++t) {
            const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
            if (t < G && !(of | ob)) continue;
            double ofe, obe;
            effective_orders(X, ln, q, sk, r, lam_end, t, of, ob, ofe, obe);
            ws = ws + (rf * ofe - rb * obe) * L[(ln.oB + t) * 64];
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
      if (A.reached) A.reached[i] = reached;
    }
  }
}

static size_t lds_bytes(int N, int T) { return (size_t)(std::max(T * T, N) + 5 * T + 2 * N) * 64 * sizeof(double); }

// the checks of the header that catkin_solve does not have; 0 or the code.  T = G + S is known to be within the limits
static int check_interactions(Ctx* ctx, const catia_params* p) {
  char msg[256];
  const int N = p->nspecies, G = p->nsitetypes, S = p->nadsorbates, R = p->nsteps, T = G + S, M = N + T;
  if (p->ramp < 1) return fail(ctx, ERR_INVAL, "catia_solve: ramp < 1");
  if (p->response != CATIA_LINEAR && p->response != CATIA_PIECEWISE) return fail(ctx, ERR_INVAL, "catia_solve: response is 0 (linear) or 1 (piecewise)");
  if (!std::isfinite(p->strength)) return fail(ctx, ERR_INVAL, "catia_solve: strength is not finite");
  if (!p->site_of || !p->site_fraction || !p->eps) return fail(ctx, ERR_INVAL, "catia_solve: site_of, site_fraction and eps are required");
  for (int g = 0; g < G; ++g)
    if (!posfin(p->site_fraction[g])) {
      snprintf(msg, sizeof msg, "catia_solve: site_fraction[%d] must be positive and finite", g);
      return fail(ctx, ERR_INVAL, msg);
    }
  for (int t = 0; t < T; ++t) {
    const int g = p->site_of[t];
    if (g < 0 || g >= G) {
      snprintf(msg, sizeof msg, "catia_solve: site_of[%d] = %d outside [0, %d)", t, g, G);
      return fail(ctx, ERR_INVAL, msg);
    }
    if (t < G && (g != t || (p->site_count && p->site_count[t] != 1.0))) {
      snprintf(msg, sizeof msg, "catia_solve: column %d is the free site of type %d: site_of must be %d and its site count 1", t, t, t);
      return fail(ctx, ERR_INVAL, msg);
    }
  }
  for (int e = 0; e < S * S; ++e)
    if (!std::isfinite(p->eps[e])) return fail(ctx, ERR_INVAL, "catia_solve: eps has a non-finite entry");
  if (p->eps_ts)
    for (int e = 0; e < R * S; ++e)
      if (!std::isfinite(p->eps_ts[e])) return fail(ctx, ERR_INVAL, "catia_solve: eps_ts has a non-finite entry");
  if (p->response == CATIA_PIECEWISE) {
    if (!p->cutoff || !p->smoothing) return fail(ctx, ERR_INVAL, "catia_solve: the piecewise response needs cutoff and smoothing");
    for (int g = 0; g < G; ++g)
      if (!std::isfinite(p->cutoff[g]) || !posfin(p->smoothing[g])) {
        snprintf(msg, sizeof msg, "catia_solve: type %d needs a finite cutoff and a positive, finite smoothing", g);
        return fail(ctx, ERR_INVAL, msg);
      }
  }
  return OK;
}

// every step conserves the sites of each type; after check_tables (the tables are there, the orders and site counts are in range)
static int check_type_balance(Ctx* ctx, const catia_params* p) {
  char msg[256];
  const int N = p->nspecies, G = p->nsitetypes, R = p->nsteps, T = G + p->nadsorbates, M = N + T;
  for (int r = 0; r < R; ++r)
      for (int g = 0; g < G; ++g) {
        double sites = 0.0;
        for (int t = 0; t < T; ++t)
          if (p->site_of[t] == g) sites += p->site_count[t] * (p->order_b[r * M + N + t] - p->order_f[r * M + N + t]);
        if (sites != 0.0) {
          snprintf(msg, sizeof msg, "catia_solve: step %d does not conserve the sites of type %d", r, g);
          return fail(ctx, ERR_INVAL, msg);
        }
      }
  return OK;
}

static void fill_extra(Extra* X, const catia_params* p) {
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

}  // namespace catia

static_assert(CATIA_OK == pnp::post::OK && CATIA_EINVAL == pnp::post::ERR_INVAL && CATIA_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATIA_EDEVICE == pnp::post::ERR_DEVICE && CATIA_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_interact.h and pnp_post.h disagree");
static_assert(CATIA_CONVERGED == pnp::kin::STATUS_CONVERGED && CATIA_MAXIT == pnp::kin::STATUS_MAXIT && CATIA_INPUT == pnp::kin::STATUS_INPUT &&
                  CATIA_PIVOT == pnp::kin::STATUS_PIVOT,
              "catint_interact.h and pnp_kin.h disagree");
static_assert(CATIA_MAX_SPECIES == pnp::kin::MAXN && CATIA_MAX_COLUMNS == pnp::kin::MAXT && CATIA_MAX_STEPS == pnp::kin::MAXR &&
                  CATIA_MAX_ORDER == pnp::kin::MAX_ORDER && CATIA_MIN_LOG == pnp::kin::MINLOG && CATIA_DROP_FULL == pnp::kin::DROP_FULL &&
                  CATIA_DROP_STERN == pnp::kin::DROP_STERN && CATIA_MAX_SITE_TYPES <= 3,
              "catint_interact.h and pnp_kin.h disagree");

struct catia_ctx : pnp::post::Ctx {};

extern "C" {

int catia_create(int32_t device, catia_ctx** out) { return pnp::post::create("catia_create", device, out); }
void catia_destroy(catia_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catia_last_error(const catia_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catia_last_kernel(const catia_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catia_last_kernel_ms(const catia_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catia_solve(catia_ctx* ctx, const pnp_device_view* view, const catia_params* p, const catia_outputs* out) {
  using namespace catia;
  static const char entry[] = "catia_solve";
  char msg[256];
  if (!ctx) return CATIA_EINVAL;
  if (!p || !out) return fail(ctx, CATIA_EINVAL, "catia_solve: null argument");
  if (p->struct_size != (int32_t)sizeof(catia_params)) return fail(ctx, CATIA_EINVAL, "catia_solve: catia_params.struct_size does not match this library");
  const int G = p->nsitetypes, S = p->nadsorbates;
  if (G < 1 || G > MAXG) {
    snprintf(msg, sizeof msg, "catia_solve: %d site types outside [1, %d]", G, MAXG);
    return fail(ctx, CATIA_EINVAL, msg);
  }
  if (S < 1 || G + S > MAXT) {
    snprintf(msg, sizeof msg, "catia_solve: %d adsorbates on %d site types: at least 1, and at most %d columns", S, G, MAXT);
    return fail(ctx, CATIA_EINVAL, msg);
  }
  // pnp_kin.h reads a model as one first column and S behind it: here T - 1 behind the free site of type 0
  catia_params q = *p;
  q.nadsorbates = G + S - 1;
  if (const int rc = check_sizes(ctx, entry, "catia_params", "catia_outputs", &q, out)) return rc;
  if (p->maxit < 1) return fail(ctx, CATIA_EINVAL, "catia_solve: maxit < 1");
  if (const int rc = check_drop(ctx, entry, p)) return rc;
  if (!posfin(p->tol)) return fail(ctx, CATIA_EINVAL, "catia_solve: tol must be positive and finite");
  if (const int rc = check_interactions(ctx, p)) return rc;
  if (const int rc = check_tables(ctx, entry, &q)) return rc;
  if (const int rc = check_type_balance(ctx, p)) return rc;
  bool from_view = false;
  if (const int rc = check_points(ctx, entry, view, &q, &from_view)) return rc;
  if (p->n == 0) return CATIA_OK;

  const int N = p->nspecies, R = p->nsteps, T = G + S;
  const size_t sn = (size_t)p->n;
  KArgs a;
  set_args(a, view, &q, from_view);
  a.G = G;
  a.K = p->ramp;
  a.strength = p->strength;
  Stage stage;
  int i_x = -1;
  if (const int rc = stage_inputs(ctx, entry, &q, a, p->theta_guess, &a.guess, from_view, 3, &stage,
                                  [&](Inputs& in) { i_x = in.add_unpadded(sizeof(Extra) / 8, &a.ext); }))   // status, iterations, ramp_reached
    return rc;
  fill_extra(reinterpret_cast<Extra*>(stage.in.host(ctx->stage, i_x)), p);
  a.maxit = p->maxit;
  a.tol = p->tol;
  const Row rows[] = {{out->theta, &a.theta, sn * T},       {out->rate, &a.rate, sn * R},           {out->rate_gross, &a.gross, sn * R},
                      {out->flux, &a.flux, sn * N},         {out->flux_scale, &a.fscale, sn * N},   {out->dflux_dc, &a.dfdc, sn * N * N},
                      {out->dflux_dphi, &a.dfdphi, sn * N * 2}, {out->energy_shift, &a.eshift, sn * S}};
  a.sens = (out->dflux_dc && N) || (out->dflux_dphi && N);
  const bool want_flags = out->status || out->iterations || out->ramp_reached;
  if (!rows_doubles(rows) && !want_flags) return CATIA_OK;
  const int rc = run(ctx, entry, "catia::interact_kernel", interact_kernel, view, &q, stage, a, rows, lds_bytes(N, T), 3, want_flags, [&](int32_t* flags) {
    a.status = flags;
    a.iters = flags + sn;
    a.reached = flags + 2 * sn;
  });
  if (rc) return rc;
  if (out->status) memcpy(out->status, ctx->flags.data(), sn * sizeof(int32_t));
  if (out->iterations) memcpy(out->iterations, ctx->flags.data() + sn, sn * sizeof(int32_t));
  if (out->ramp_reached) memcpy(out->ramp_reached, ctx->flags.data() + 2 * sn, sn * sizeof(int32_t));
  return CATIA_OK;
}

}  // extern "C"
