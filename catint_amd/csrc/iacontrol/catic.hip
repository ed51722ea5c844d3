// libcatint_iacontrol (include/catint_iacontrol.h): the degree of rate control of the steady state of the model of libcatint_interact
// (lateral interactions, up to three site types) per operating point -- the full Jacobian of the scaled rows at the given coverages,
// the shifts included, factorised once, then one right-hand side per rate constant, transition state and adsorbate energy, and one for
// the interaction strength itself.  gfx950 / MI355X only.
//
// Mapping, working set, tables and arithmetic: ../pnp_kin.h, included unchanged (point inputs, the factors of a rate, the row scaling
// with the dead-row rule, the per-lane LU, the host scaffold).  The columns, their refinement step and the order of every sum are those
// of drc/catdrc.hip; the response, the surface state, the rate constants at the lane's coverages and the effective orders are those of
// interact/catia.hip, restated here as iasweep/catis.hip restates them (a header shared by the three is a change of its own).
// LDS slots: catdrc's (J[T][T], the site rows' n_t theta_t [T], the right-hand side [T], D[T], N activities / accumulators, N fluxes,
// rf[R], rb[R], T refinement slots: 165 at T = 9, N = 8, R = 16) plus theta[T]: 174 slots x 512 B = 87 KB per wave.  w_u = f theta_u is
// formed where it is read.  The branches of Ga are 2-bit fields of one register; f_g, f'_g are scalars picked by compares.  In the
// piecewise mode the per-type sums qg, qs of a step are RECOMPUTED wherever W[r][t] is formed (the assembly and both passes of every
// column): 6 R slots more would be 48 KB, and would take the second wave of a CU away from every model with T <= 7; the sums cost S
// LDS reads per step next to the T reads of the column itself.  In the linear mode f' = 0 and they are not formed.
#include "../../../include/catint_iacontrol.h"
#include "../pnp_kin.h"

#pragma clang fp contract(off)

namespace catic {

using namespace pnp::kin;

constexpr int MAXG = CATIC_MAX_SITE_TYPES;

// what the call adds to kin::Table (T = G + S columns there), flattened and contracted on the host
struct Extra {
  int32_t G, mode;
  int32_t site_of[MAXT + 1];
  double x[MAXG], cutoff[MAXG], smooth[MAXG];
  double nx[MAXT];                               // n_t / x_g(t)
  double eg[MAXR][MAXS], ea[MAXR][MAXS];         // EG, EA: [step][adsorbate]
};
static_assert(sizeof(Extra) % 8 == 0, "the table is copied as doubles");

struct KArgs {
  int32_t N, S, R, w, use_sigma, from_view, ldx, G;   // S: T - 1, the columns behind the first (as pnp_kin.h reads it)
  int64_t n;
  const double* c;         // view: [B][N][ldx]
  const double* phi;       // view: [B][ldx]
  const int32_t* st;       // view: [B] solver status
  const int64_t* lanes;    // [n]
  const double *cs, *phis; // host surface state: [n][N], [n]
  const double *phiM, *sigma, *off, *gamma, *theta;   // [n], [n], [n][R][2], [n][N], [n][T]; null: absent (theta: never)
  const Extra* ext;
  double *dkf, *dkb, *dts, *dyts, *xrc, *dG, *xtrc, *dlam, *dylam, *xlam, *flux, *fscale, *resid;   // device rows; null: not wanted
  int32_t* status;
  double sd, rtol, CS, pzc, strength;
};

// what one lane carries in registers
struct Lane {
  double* L;       // lds + lane: slot s at L[s * 64]
  int oJ, oY, oB, oD, oA, oF, oRf, oRb, oX, oTh;   // first slots of J, y / n theta, right-hand side, D, activities / accumulators, fluxes, rf, rb, refinement, theta
  Point pt;        // potential, charge and off row of the point
  __device__ __forceinline__ double* at(int slot) const { return L + slot * 64; }
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
  if (X.mode == CATIC_PIECEWISE) {
    response(c0 / X.x[0], X.cutoff[0], X.smooth[0], q.f0, q.p0);
    if (G > 1) response(c1 / X.x[1], X.cutoff[1], X.smooth[1], q.f1, q.p1);
    if (G > 2) response(c2 / X.x[2], X.cutoff[2], X.smooth[2], q.f2, q.p2);
  }
  return q;
}

// sum_u EG[r][u] w_u and sum_u EA[r][u] w_u (0 without a transition state), w_u = f theta_u formed here, u ascending
__device__ __forceinline__ void step_shifts(const Table& tb, const Extra& X, const Lane& ln, const Resp& q, int T, int r, double& sG, double& sA) {
  const double* L = ln.L;
  const int G = X.G, S = T - G;
  const bool ts = tb.ea[r][0] != -INFINITY;
  sG = 0.0;
  sA = 0.0;
  for (int a = 0; a < S; ++a) {
    const double w = pick(X.site_of[G + a], q.f0, q.f1, q.f2) * L[(ln.oTh + G + a) * 64];
    sG = sG + X.eg[r][a] * w;
    if (ts) sA = sA + X.ea[r][a] * w;
  }
}

// ln kf, ln kb of step r at the lane's coverages and the strength lam, and the branch of Ga (0: Ea, 1: dG, 2: zero)
__device__ __forceinline__ void step_constants(const Table& tb, const Extra& X, const Lane& ln, const Resp& q, int T, int r, double lam, double& lf,
                                               double& lb, int& br) {
  const double V = ln.pt.V, sg = ln.pt.sg, s2 = sg * sg;
  const double dG0 = ((tb.dg[r][0] + tb.dg[r][1] * V) + tb.dg[r][2] * sg) + tb.dg[r][3] * s2;
  const double Ea0 = ((tb.ea[r][0] + tb.ea[r][1] * V) + tb.ea[r][2] * sg) + tb.ea[r][3] * s2;
  const bool ts = tb.ea[r][0] != -INFINITY;
  double sG, sA;
  step_shifts(tb, X, ln, q, T, r, sG, sA);
  const double dG = dG0 + lam * sG;
  const double Ea = ts ? Ea0 + lam * sA : Ea0;
  const bool b0 = Ea >= dG && Ea >= 0.0, b1 = dG >= 0.0;
  br = b0 ? 0 : (b1 ? 1 : 2);
  const double Ga = b0 ? Ea : (b1 ? dG : 0.0);
  const double* off = ln.pt.off;
  const double o0 = off ? off[2 * r] : 0.0, o1 = off ? off[2 * r + 1] : 0.0;
  lf = (tb.lnA[r] - Ga) + o0;
  lb = (tb.lnA[r] - (Ga - dG)) + o1;
}

// the per-type sums sum_{u on g} E[r][u] theta_u of the dG row (qg) and of the row of the branch (qs): the piecewise mode only
struct StepQ {
  double qg0, qg1, qg2, qs0, qs1, qs2;
  int br;
};

__device__ __forceinline__ void step_sums(const Extra& X, const Lane& ln, int T, int r, int br, StepQ& k) {
  const double* L = ln.L;
  const int G = X.G, S = T - G;
  k.br = br;
  k.qg0 = k.qg1 = k.qg2 = k.qs0 = k.qs1 = k.qs2 = 0.0;
  if (X.mode == CATIC_PIECEWISE)
    for (int a = 0; a < S; ++a) {
      const int g = X.site_of[G + a];
      const double th = L[(ln.oTh + G + a) * 64];
      const double eG = X.eg[r][a], eS = br == 0 ? X.ea[r][a] : (br == 1 ? eG : 0.0);
      const double vg = eG * th, vs = eS * th;
      k.qg0 = k.qg0 + (g == 0 ? vg : 0.0), k.qs0 = k.qs0 + (g == 0 ? vs : 0.0);
      k.qg1 = k.qg1 + (g == 1 ? vg : 0.0), k.qs1 = k.qs1 + (g == 1 ? vs : 0.0);
      k.qg2 = k.qg2 + (g == 2 ? vg : 0.0), k.qs2 = k.qs2 + (g == 2 ? vs : 0.0);
    }
}

// d ln rf / dy_t and d ln rb / dy_t of step r: the orders of column t, and for an adsorbate -theta_t dGa/dtheta_t and
// -theta_t (dGa/dtheta_t - ddG/dtheta_t) on top
__device__ __forceinline__ void effective_orders(const Extra& X, const Lane& ln, const Resp& q, const StepQ& k, int r, double lam, int t, int of, int ob,
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

// what every column reads of the point besides its slots
struct State {
  Resp q;
  uint32_t brs;    // the branch of Ga of step r in bits 2r, 2r+1
  double lam;
};

// dnet of step r into the column's right-hand side (unscaled) and flux accumulators
__device__ __forceinline__ void add_step(const Table& tb, const Lane& ln, int N, int G, int T, int r, double dnet) {
  double* L = ln.L;
  for (int s = G; s < T; ++s) {
    const int m = tb.ob[r][N + s] - tb.of[r][N + s];
    if (m) L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + (double)m * dnet;
  }
  for (int k = 0; k < N; ++k) {
    const double nu = tb.nu[r][k];
    if (nu != 0.0) L[(ln.oA + k) * 64] = L[(ln.oA + k) * 64] + nu * dnet;
  }
}

// d(rf_r - rb_r)/dp at fixed y of column q of family fam (0: ln kf_q, 1: ln kb_q, 2: the transition state of step q, 3: the energy of
// adsorbate q (column G + q), 4: the interaction strength); *in: whether step r is in the column's support at all (the same in every
// lane)
__device__ __forceinline__ double column_dnet(const Table& tb, const Extra& X, const Lane& ln, const State& st, int N, int T, int fam, int q, int r,
                                              bool* in) {
  const double rf = ln.L[(ln.oRf + r) * 64], rb = ln.L[(ln.oRb + r) * 64];
  if (fam < 3) {
    *in = r == q;
    return fam == 0 ? rf : (fam == 1 ? -rb : rf - rb);
  }
  const uint32_t br = (st.brs >> (2 * r)) & 3u;
  double ddG, dEa;
  if (fam == 3) {
    const int s = X.G + q;
    const int ofs = tb.of[r][N + s], ms = tb.ob[r][N + s] - ofs;
    *in = (ms | ofs) != 0;
    ddG = -(double)ms;
    dEa = (double)ofs;
  } else {
    *in = true;
    step_shifts(tb, X, ln, st.q, T, r, ddG, dEa);
  }
  const double dGa = br == 0 ? dEa : (br == 1 ? ddG : 0.0);
  const double alpha = -dGa, beta = -(dGa - ddG);
  return rf * alpha - rb * beta;
}

// sum_t W[r][t] v_t with v in the T slots from `at`
__device__ __forceinline__ double through_y(const Table& tb, const Extra& X, const Lane& ln, const State& st, int N, int T, int r, int at) {
  const double rf = ln.L[(ln.oRf + r) * 64], rb = ln.L[(ln.oRb + r) * 64];
  StepQ k;
  step_sums(X, ln, T, r, (int)((st.brs >> (2 * r)) & 3u), k);
  double ws = 0.0;
  for (int t = 0; t < T; ++t) {
    const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
    if (t < X.G && !(of | ob)) continue;
    double ofe, obe;
    effective_orders(X, ln, st.q, k, r, st.lam, t, of, ob, ofe, obe);
    ws = ws + (rf * ofe - rb * obe) * ln.L[(at + t) * 64];
  }
  return ws;
}

// The column's right-hand side scaled and solved, then one step of refinement against the rows themselves (catdrc.hip: close_column).
// dy is left in the B slots; the part of the fluxes that goes through dy is added to the accumulators.
__device__ __forceinline__ void close_column(const Table& tb, const Extra& X, const Lane& ln, const State& st, int N, int T, int R, uint64_t pivs, int fam,
                                             int q) {
  double* L = ln.L;
  const int G = X.G;
  for (int s = G; s < T; ++s) {
    const double D = L[(ln.oD + s) * 64];
    L[(ln.oB + s) * 64] = D == 0.0 ? 0.0 : -(L[(ln.oB + s) * 64] / D);
  }
  substitute(ln.at(ln.oJ), ln.at(ln.oB), T, pivs);
  for (int g = 0; g < G; ++g) {
    double r0 = 0.0;
    for (int t = 0; t < T; ++t) {
      const double v = L[(ln.oY + t) * 64] * L[(ln.oB + t) * 64];   // the y slots hold n_t theta_t by now
      r0 = r0 + (X.site_of[t] == g ? v : 0.0);
    }
    L[(ln.oX + g) * 64] = -(r0 / X.x[g]);
  }
  for (int s = G; s < T; ++s) L[(ln.oX + s) * 64] = 0.0;
  for (int r = 0; r < R; ++r) {
    bool in;
    const double dnet = column_dnet(tb, X, ln, st, N, T, fam, q, r, &in);
    const double ws = through_y(tb, X, ln, st, N, T, r, ln.oB);
    const double tot = in ? dnet + ws : ws;
    for (int s = G; s < T; ++s) {
      const int m = tb.ob[r][N + s] - tb.of[r][N + s];
      if (m) L[(ln.oX + s) * 64] = L[(ln.oX + s) * 64] + (double)m * tot;
    }
  }
  for (int s = G; s < T; ++s) {
    const double D = L[(ln.oD + s) * 64];
    L[(ln.oX + s) * 64] = D == 0.0 ? -L[(ln.oB + s) * 64] : -(L[(ln.oX + s) * 64] / D);
  }
  substitute(ln.at(ln.oJ), ln.at(ln.oX), T, pivs);
  for (int t = 0; t < T; ++t) L[(ln.oB + t) * 64] = L[(ln.oB + t) * 64] + L[(ln.oX + t) * 64];
  for (int r = 0; r < R; ++r) {
    const double ws = through_y(tb, X, ln, st, N, T, r, ln.oB);
    for (int k = 0; k < N; ++k) {
      const double nu = tb.nu[r][k];
      if (nu != 0.0) L[(ln.oA + k) * 64] = L[(ln.oA + k) * 64] + nu * ws;
    }
  }
}

__global__ __launch_bounds__(64) void control_kernel(const KArgs A, const Table* __restrict__ tab) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1, R = A.R, G = A.G;
  const Table& tb = *tab;   // its own read-only argument: the uniform reads become scalar loads
  const Extra& X = *A.ext;
  Lane ln;
  ln.L = lds + lane;
  ln.oJ = 0;
  ln.oY = T * T;
  ln.oB = ln.oY + T;
  ln.oD = ln.oB + T;
  ln.oA = ln.oD + T;
  ln.oF = ln.oA + N;
  ln.oRf = ln.oF + N;
  ln.oRb = ln.oRf + R;
  ln.oX = ln.oRb + R;
  ln.oTh = ln.oX + T;
  double* L = ln.L;
  const double bad_number = __builtin_nan("");
  // species that take no part in the mechanism (column k of nu all zero): their normalised entries are exactly 0
  uint32_t idle = 0;
  for (int k = 0; k < N; ++k) {
    bool any = false;
    for (int r = 0; r < R; ++r) any = any || tb.nu[r][k] != 0.0;
    idle |= any ? 0u : 1u << k;
  }

  for (int64_t grp = blockIdx.x; grp * 64 < A.n; grp += gridDim.x) {
    const bool live = grp * 64 + lane < A.n;
    const int64_t i = live ? grp * 64 + lane : A.n - 1;
    const int64_t b = A.lanes[i];
    ln.pt = point_inputs(A, tb, i, b, ln.at(ln.oA));
    bool ok = ln.pt.ok;
    // ---- the state: y = ln theta, clamped as catkin clamps its guess; theta = exp(y) and the response of every type ----
    for (int t = 0; t < T; ++t) {
      const double g = A.theta[i * T + t];
      ok = ok && finite_(g);
      L[(ln.oY + t) * 64] = log_coverage(g);
    }
    State st;
    st.lam = A.strength;
    st.q = surface_state(tb, X, ln, T);
    // ---- rf, rb once per point; the branch of Ga of step r in bits 2r, 2r+1 (0: Ea, 1: dG, 2: zero) ----
    st.brs = 0;
    for (int r = 0; r < R; ++r) {
      double lf, lb, ef, eb, pf, pb;
      int br;
      step_constants(tb, X, ln, st.q, T, r, st.lam, lf, lb, br);
      st.brs |= (uint32_t)br << (2 * r);
      rate_factors(tb, N, T, ln.at(ln.oY), ln.at(ln.oA), r, lf, lb, -1, ef, eb, pf, pb);
      L[(ln.oRf + r) * 64] = ef * pf;
      L[(ln.oRb + r) * 64] = eb * pb;
    }
    // ---- J (scaled rows), -F and the row scales D at this y; fluxes (the activities' slots now hold flux_scale) ----
    for (int s = 0; s < T * T; ++s) L[(ln.oJ + s) * 64] = 0.0;
    for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0, L[(ln.oD + s) * 64] = 0.0;
    for (int k = 0; k < N; ++k) L[(ln.oF + k) * 64] = 0.0, L[(ln.oA + k) * 64] = 0.0;
    for (int r = 0; r < R; ++r) {
      const double rf = L[(ln.oRf + r) * 64], rb = L[(ln.oRb + r) * 64], net = rf - rb, gross = rf + rb;
      for (int s = G; s < T; ++s) {
        const int m = tb.ob[r][N + s] - tb.of[r][N + s];
        if (m == 0) continue;
        L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + (double)m * net;
        L[(ln.oD + s) * 64] = L[(ln.oD + s) * 64] + fabs((double)m) * gross;
      }
      StepQ k;
      step_sums(X, ln, T, r, (int)((st.brs >> (2 * r)) & 3u), k);
      for (int t = 0; t < T; ++t) {
        const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
        if (t < G && !(of | ob)) continue;
        double ofe, obe;
        effective_orders(X, ln, st.q, k, r, st.lam, t, of, ob, ofe, obe);
        const double c = rf * ofe - rb * obe;
        for (int s = G; s < T; ++s) {
          const int m = tb.ob[r][N + s] - tb.of[r][N + s];
          if (m) L[(ln.oJ + s * T + t) * 64] = L[(ln.oJ + s * T + t) * 64] + (double)m * c;
        }
      }
      for (int j = 0; j < N; ++j) {
        const double nu = tb.nu[r][j];
        if (nu != 0.0) {
          L[(ln.oF + j) * 64] = L[(ln.oF + j) * 64] + nu * net;
          L[(ln.oA + j) * 64] = L[(ln.oA + j) * 64] + fabs(nu) * gross;
        }
      }
    }
    double res = 0.0;
    for (int s = G; s < T; ++s) {
      const double D = L[(ln.oD + s) * 64];
      const bool dead = scale_row(ln.at(ln.oJ), ln.at(ln.oY), T, s, D);
      const double f = dead ? 0.0 : fabs(L[(ln.oB + s) * 64] / D);
      res = f > res || f != f ? f : res;
    }
    // the site rows, one per type; n_t theta_t goes through the refinement slots into the y slots, which have done their work
    for (int t = 0; t < T; ++t) L[(ln.oX + t) * 64] = tb.ns[t] * exp(L[(ln.oY + t) * 64]);
    for (int g = 0; g < G; ++g) {
      double f0 = 0.0;
      for (int t = 0; t < T; ++t) {
        const bool on = X.site_of[t] == g;
        const double th = L[(ln.oX + t) * 64];
        L[(ln.oJ + g * T + t) * 64] = on ? th / X.x[g] : 0.0;
        f0 = f0 + (on ? th : 0.0);
      }
      const double f = fabs(f0 / X.x[g] - 1.0);
      res = f > res || f != f ? f : res;
    }
    for (int t = 0; t < T; ++t) L[(ln.oY + t) * 64] = L[(ln.oX + t) * 64];
    uint64_t pivs = 0;
    const bool bad = factor(ln.at(ln.oJ), T, pivs);
    const int status = !ok ? CATIC_INPUT : (bad ? CATIC_PIVOT : (res <= A.rtol ? CATIC_OK_POINT : CATIC_RESIDUAL));
    const bool nan = status == CATIC_INPUT;
    for (int k = 0; k < N; ++k) {
      const double fl = A.sd * L[(ln.oF + k) * 64];
      L[(ln.oF + k) * 64] = fl;          // as stored: the normalised entries divide by this number
      if (live) {
        if (A.flux) A.flux[i * N + k] = nan ? bad_number : fl;
        if (A.fscale) A.fscale[i * N + k] = nan ? bad_number : A.sd * L[(ln.oA + k) * 64];
      }
    }
    if (live) {
      if (A.resid) A.resid[i] = nan ? bad_number : res;
      if (A.status) A.status[i] = status;
    }

    // ---- the columns: family 0 d/d ln kf_r, 1 d/d ln kb_r, 2 the transition state of step r, 3 the energy of adsorbate q, 4 the strength ----
    for (int fam = 0; fam < 5; ++fam) {
      const bool wanted = fam == 0 ? A.dkf != nullptr
                                   : (fam == 1 ? A.dkb != nullptr
                                               : (fam == 2 ? (A.dts || A.dyts || A.xrc) : (fam == 3 ? (A.dG || A.xtrc) : (A.dlam || A.dylam || A.xlam))));
      if (!wanted) continue;
      const int ncol = fam == 3 ? T - G : (fam == 4 ? 1 : R);
      for (int q = 0; q < ncol; ++q) {
        for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0;
        for (int k = 0; k < N; ++k) L[(ln.oA + k) * 64] = 0.0;
        for (int r = fam < 3 ? q : 0; r < (fam < 3 ? q + 1 : R); ++r) {
          bool in;
          const double dnet = column_dnet(tb, X, ln, st, N, T, fam, q, r, &in);
          if (in) add_step(tb, ln, N, G, T, r, dnet);          // a step outside the column's support contributes nothing
        }
        close_column(tb, X, ln, st, N, T, R, pivs, fam, q);
        if (!live) continue;
        double* dy = fam == 2 ? A.dyts : (fam == 4 ? A.dylam : nullptr);
        if (dy)
          for (int t = 0; t < T; ++t) dy[((size_t)i * ncol + q) * T + t] = nan ? bad_number : L[(ln.oB + t) * 64];
        double* raw = fam == 0 ? A.dkf : (fam == 1 ? A.dkb : (fam == 2 ? A.dts : (fam == 3 ? A.dG : A.dlam)));
        double* norm = fam == 2 ? A.xrc : (fam == 3 ? A.xtrc : (fam == 4 ? A.xlam : nullptr));
        const size_t at = ((size_t)i * ncol + q) * N;
        for (int k = 0; k < N; ++k) {
          const double v = A.sd * L[(ln.oA + k) * 64];
          if (raw) raw[at + k] = nan ? bad_number : v;
          if (norm) {
            const double x = v / L[(ln.oF + k) * 64];
            norm[at + k] = nan ? bad_number : ((idle >> k) & 1u ? 0.0 : (fam == 4 ? A.strength * x : x));
          }
        }
      }
    }
  }
}

static size_t lds_bytes(int N, int T, int R) { return (size_t)(T * T + 5 * T + 2 * N + 2 * R) * 64 * sizeof(double); }

// the checks of catint_interact.h that catdrc_solve does not have; 0 or the code.  T = G + S is known to be within the limits
static int check_interactions(Ctx* ctx, const catic_params* p) {
  char msg[256];
  const int G = p->nsitetypes, S = p->nadsorbates, R = p->nsteps, T = G + S;
  if (p->response != CATIC_LINEAR && p->response != CATIC_PIECEWISE) return fail(ctx, ERR_INVAL, "catic_solve: response is 0 (linear) or 1 (piecewise)");
  if (!std::isfinite(p->strength)) return fail(ctx, ERR_INVAL, "catic_solve: strength is not finite");
  if (!p->site_of || !p->site_fraction || !p->eps) return fail(ctx, ERR_INVAL, "catic_solve: site_of, site_fraction and eps are required");
  for (int g = 0; g < G; ++g)
    if (!posfin(p->site_fraction[g])) {
      snprintf(msg, sizeof msg, "catic_solve: site_fraction[%d] must be positive and finite", g);
      return fail(ctx, ERR_INVAL, msg);
    }
  for (int t = 0; t < T; ++t) {
    const int g = p->site_of[t];
    if (g < 0 || g >= G) {
      snprintf(msg, sizeof msg, "catic_solve: site_of[%d] = %d outside [0, %d)", t, g, G);
      return fail(ctx, ERR_INVAL, msg);
    }
    if (t < G && (g != t || (p->site_count && p->site_count[t] != 1.0))) {
      snprintf(msg, sizeof msg, "catic_solve: column %d is the free site of type %d: site_of must be %d and its site count 1", t, t, t);
      return fail(ctx, ERR_INVAL, msg);
    }
  }
  for (int e = 0; e < S * S; ++e)
    if (!std::isfinite(p->eps[e])) return fail(ctx, ERR_INVAL, "catic_solve: eps has a non-finite entry");
  if (p->eps_ts)
    for (int e = 0; e < R * S; ++e)
      if (!std::isfinite(p->eps_ts[e])) return fail(ctx, ERR_INVAL, "catic_solve: eps_ts has a non-finite entry");
  if (p->response == CATIC_PIECEWISE) {
    if (!p->cutoff || !p->smoothing) return fail(ctx, ERR_INVAL, "catic_solve: the piecewise response needs cutoff and smoothing");
    for (int g = 0; g < G; ++g)
      if (!std::isfinite(p->cutoff[g]) || !posfin(p->smoothing[g])) {
        snprintf(msg, sizeof msg, "catic_solve: type %d needs a finite cutoff and a positive, finite smoothing", g);
        return fail(ctx, ERR_INVAL, msg);
      }
  }
  return OK;
}

// every step conserves the sites of each type; after check_tables (the tables are there, the orders and site counts are in range)
static int check_type_balance(Ctx* ctx, const catic_params* p) {
  char msg[256];
  const int N = p->nspecies, G = p->nsitetypes, R = p->nsteps, T = G + p->nadsorbates, M = N + T;
  for (int r = 0; r < R; ++r)
    for (int g = 0; g < G; ++g) {
      double sites = 0.0;
      for (int t = 0; t < T; ++t)
        if (p->site_of[t] == g) sites += p->site_count[t] * (p->order_b[r * M + N + t] - p->order_f[r * M + N + t]);
      if (sites != 0.0) {
        snprintf(msg, sizeof msg, "catic_solve: step %d does not conserve the sites of type %d", r, g);
        return fail(ctx, ERR_INVAL, msg);
      }
    }
  return OK;
}

static void fill_extra(Extra* X, const catic_params* p) {
  const int N = p->nspecies, G = p->nsitetypes, S = p->nadsorbates, R = p->nsteps, T = G + S, M = N + T;
  memset(X, 0, sizeof *X);
  X->G = G;
  X->mode = p->response;
  for (int t = 0; t < T; ++t) X->site_of[t] = p->site_of[t], X->nx[t] = p->site_count[t] / p->site_fraction[p->site_of[t]];
  for (int g = 0; g < G; ++g) {
    X->x[g] = p->site_fraction[g];
    if (p->response == CATIC_PIECEWISE) X->cutoff[g] = p->cutoff[g], X->smooth[g] = p->smoothing[g];
  }
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

}  // namespace catic

static_assert(CATIC_OK == pnp::post::OK && CATIC_EINVAL == pnp::post::ERR_INVAL && CATIC_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATIC_EDEVICE == pnp::post::ERR_DEVICE && CATIC_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_iacontrol.h and pnp_post.h disagree");
static_assert(CATIC_MAX_SPECIES == pnp::kin::MAXN && CATIC_MAX_COLUMNS == pnp::kin::MAXT && CATIC_MAX_STEPS == pnp::kin::MAXR &&
                  CATIC_MAX_ORDER == pnp::kin::MAX_ORDER && CATIC_MIN_LOG == pnp::kin::MINLOG && CATIC_DROP_FULL == pnp::kin::DROP_FULL &&
                  CATIC_DROP_STERN == pnp::kin::DROP_STERN && CATIC_MAX_SITE_TYPES <= 3,
              "catint_iacontrol.h and pnp_kin.h disagree");
static_assert(CATIC_MAX_STEPS <= 16 && CATIC_MAX_SPECIES <= 32, "a branch is a 2-bit field of 32 bits, an idle species one bit");

struct catic_ctx : pnp::post::Ctx {};

extern "C" {

int catic_create(int32_t device, catic_ctx** out) { return pnp::post::create("catic_create", device, out); }
void catic_destroy(catic_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catic_last_error(const catic_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catic_last_kernel(const catic_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catic_last_kernel_ms(const catic_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catic_solve(catic_ctx* ctx, const pnp_device_view* view, const catic_params* p, const catic_outputs* out) {
  using namespace catic;
  static const char entry[] = "catic_solve";
  char msg[256];
  if (!ctx) return CATIC_EINVAL;
  if (!p || !out) return fail(ctx, CATIC_EINVAL, "catic_solve: null argument");
  if (p->struct_size != (int32_t)sizeof(catic_params)) return fail(ctx, CATIC_EINVAL, "catic_solve: catic_params.struct_size does not match this library");
  const int G = p->nsitetypes, S = p->nadsorbates;
  if (G < 1 || G > MAXG) {
    snprintf(msg, sizeof msg, "catic_solve: %d site types outside [1, %d]", G, MAXG);
    return fail(ctx, CATIC_EINVAL, msg);
  }
  if (S < 1 || G + S > MAXT) {
    snprintf(msg, sizeof msg, "catic_solve: %d adsorbates on %d site types: at least 1, and at most %d columns", S, G, MAXT);
    return fail(ctx, CATIC_EINVAL, msg);
  }
  // pnp_kin.h reads a model as one first column and S behind it: here T - 1 behind the free site of type 0
  catic_params q = *p;
  q.nadsorbates = G + S - 1;
  if (const int rc = check_sizes(ctx, entry, "catic_params", "catic_outputs", &q, out)) return rc;
  if (const int rc = check_drop(ctx, entry, p)) return rc;
  if (!posfin(p->residual_tol)) return fail(ctx, CATIC_EINVAL, "catic_solve: residual_tol must be positive and finite");
  if (const int rc = check_interactions(ctx, p)) return rc;
  if (const int rc = check_tables(ctx, entry, &q)) return rc;
  if (const int rc = check_type_balance(ctx, p)) return rc;
  if (!p->theta) return fail(ctx, CATIC_EINVAL, "catic_solve: theta is required (the coverages catia_solve returned)");
  bool from_view = false;
  if (const int rc = check_points(ctx, entry, view, &q, &from_view)) return rc;
  if (p->n == 0) return CATIC_OK;

  const int N = p->nspecies, R = p->nsteps, T = G + S;
  const size_t sn = (size_t)p->n;
  KArgs a;
  set_args(a, view, &q, from_view);
  a.G = G;
  a.strength = p->strength;
  Stage stage;
  int i_x = -1;
  if (const int rc = stage_inputs(ctx, entry, &q, a, p->theta, &a.theta, from_view, 1, &stage,
                                  [&](Inputs& in) { i_x = in.add_unpadded(sizeof(Extra) / 8, &a.ext); }))   // the status
    return rc;
  fill_extra(reinterpret_cast<Extra*>(stage.in.host(ctx->stage, i_x)), p);
  a.rtol = p->residual_tol;
  const Row rows[] = {{out->dflux_dlnkf, &a.dkf, sn * R * N}, {out->dflux_dlnkb, &a.dkb, sn * R * N}, {out->dflux_drc, &a.dts, sn * R * N},
                      {out->dy_drc, &a.dyts, sn * R * T},     {out->drc, &a.xrc, sn * R * N},         {out->dflux_dG, &a.dG, sn * S * N},
                      {out->tdrc, &a.xtrc, sn * S * N},       {out->dflux_dstrength, &a.dlam, sn * N}, {out->dy_dstrength, &a.dylam, sn * T},
                      {out->strength_control, &a.xlam, sn * N}, {out->flux, &a.flux, sn * N},         {out->flux_scale, &a.fscale, sn * N},
                      {out->residual, &a.resid, sn}};
  if (!rows_doubles(rows) && !out->status) return CATIC_OK;
  const int rc = run(ctx, entry, "catic::control_kernel", control_kernel, view, &q, stage, a, rows, lds_bytes(N, T, R), 1, out->status != nullptr,
                     [&](int32_t* flags) { a.status = flags; });
  if (rc) return rc;
  if (out->status) memcpy(out->status, ctx->flags.data(), sn * sizeof(int32_t));
  return CATIC_OK;
}

}  // extern "C"
