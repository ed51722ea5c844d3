// libcatint_response (include/catint_response.h): the linear response of a stationary state of the physical mode -- one block-tridiagonal
// solve (J + i omega S) du = r per (operating point, frequency) -- formed on the device from the state a pnp_handle holds there.  It
// shares no code with the Newton kernels (pnp_newton.hip, pnp_lane*.hip): the Jacobian is restated here from the header's definitions.
// gfx950 / MI355X only.
//
// Mapping: a TEAM of NB = N + 1 adjacent lanes per system; lane r owns row r of the working block row [D' | L] (2 NB numbers, real or
// complex) in registers.  64 / NB teams per wave, one wave per workgroup, no workgroup barrier; persistent waves walk groups of systems.
// Lanes beyond the last full team form a partial team with an LDS area of its own and systems beyond the last one repeat a valid one:
// both run every step and only skip their stores.
// Algorithm: block Thomas from the bulk towards the wall.  r is zero away from the wall, so the eliminated right-hand sides are zero
// and only T_i = D'_i^-1 L_i is formed: row nx-1 is the identity (T = 0), for i = nx-2 .. 1 Gauss-Jordan without row exchanges on
// [D'_i | L_i] across the team, then D'_{i-1} = M_{i-1} - U_{i-1} T_i; at the wall du_0 = D'_0^-1 r_0, and du_i = -T_i du_{i-1}.
// Every elimination step is monitored as the lane kernels monitor theirs: a pivot that is zero or not finite, or an entry below it
// more than CATRESP_PIVOT_GROWTH_LIMIT times its size (what partial pivoting would have exchanged), marks the system: status 1.
// A system whose operating point is not solved (status 2) runs through the same steps -- the lanes of a wave move in lockstep, so
// skipping would save nothing -- and only its stores are replaced by NaN.
// A scalars-only call keeps nothing between rows (T_1 alone, for the Dirichlet charge).  With profiles the T_i go to a workspace area of
// the team's slot and the same lanes substitute from the wall to the bulk in the same launch (lane r reads back the row it wrote).
// Exchanges inside a team go through LDS (the pivot row and the rows of T_i are read as broadcasts); every lane of the wave takes
// part in every exchange.  State: lane r reads row r of the operating point (c_r, or phi for r = N) one point per block row, two
// block rows ahead of its use, so the load hides behind the O(NB^3) algebra of a block row.
// Arithmetic order is fixed in the source (no implicit contraction), so the two instances of a block size and number type that differ
// only in RECORDS return the same scalars bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../../include/catint_response.h"
#include "../pnp_post.h"

#pragma clang fp contract(off)

namespace catresp {

using namespace pnp::post;

constexpr int MAXS = CATRESP_MAX_SPECIES, MAXR = PNP_MAX_REACTIONS, MAXT = PNP_MAX_REACTANTS, MAXW = PNP_MAX_WALL_REACTIONS;
constexpr double GROWTH2 = CATRESP_PIVOT_GROWTH_LIMIT * CATRESP_PIVOT_GROWTH_LIMIT;
constexpr int SPF = 8;   // per-row constants: D, q beta, dx^2 / D, velocity dx, dx (row N: 1, 0, 0, 0, 0)

// the reaction and wall tables of one call, flattened on the host (every index validated there)
struct Table {
  int32_t n_side[2][MAXR];          // entries of the left / right side
  int32_t side[2][MAXR][MAXT];
  double kk[2][MAXR];               // kf, kr
  double net[MAXR][MAXS + 1];       // n_rhs(k, r) - n_lhs(k, r); column N: 0
  int32_t wspecies[MAXW], pad_[MAXW];
  double nu[MAXW][MAXS + 1];        // column N: 0
  double alpha[MAXW], sat[MAXW];
};
static_assert(sizeof(Table) % 8 == 0, "the table is copied as doubles");

struct KArgs {
  int32_t nx, ldx, nreact, nwall, stern, pert, pspecies, F, steric, slots_pad_;
  int64_t nsys;            // selected operating points x frequencies
  const double* c;         // [B][N][ldx]
  const double* phi;       // [B][ldx]
  const int32_t* st;       // [B] solver status
  const int64_t* lanes;    // [n]
  const double *wgt, *vol; // [nx-1] dx / h_e, [nx] v_i
  const double* sp;        // [NB][SPF]
  const double *kwall, *phiM, *omega;   // [B][nwall], [B], [F]
  const Table* tab;
  double *dphis, *dcs, *dsig, *dwf, *adm, *dc, *dphi;   // device rows of complex numbers; null: not wanted
  int32_t* status;
  void* ws;                // [grid x teams][nx][NB][NB] numbers: the records of the team slots
  double volk[MAXS], q[MAXS];   // N_A a_k^3, q_k
  double pe, sternc, CS, eps, h0;   // dx^2 / eps, dx C_S / eps, C_S, eps, x[1] - x[0]
};

// ---- real / complex numbers --------------------------------------------------------------------------------------------------------
struct cplx {
  double re, im;
};
template <bool CX>
struct Num {
  using T = double;
};
template <>
struct Num<true> {
  using T = cplx;
};

__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <class T>
__device__ __forceinline__ T make(double re, double im);
template <>
__device__ __forceinline__ double make<double>(double re, double) { return re; }
template <>
__device__ __forceinline__ cplx make<cplx>(double re, double im) { return cplx{re, im}; }

__device__ __forceinline__ double re_(double a) { return a; }
__device__ __forceinline__ double re_(cplx a) { return a.re; }
__device__ __forceinline__ double im_(double) { return 0.0; }
__device__ __forceinline__ double im_(cplx a) { return a.im; }
__device__ __forceinline__ double mul(double a, double b) { return a * b; }
__device__ __forceinline__ cplx mul(cplx a, cplx b) { return cplx{fma_(-a.im, b.im, a.re * b.re), fma_(a.im, b.re, a.re * b.im)}; }
// a - f b
__device__ __forceinline__ double fnma(double a, double f, double b) { return fma_(-f, b, a); }
__device__ __forceinline__ cplx fnma(cplx a, cplx f, cplx b) {
  return cplx{fma_(f.im, b.im, fma_(-f.re, b.re, a.re)), fma_(-f.im, b.re, fma_(-f.re, b.im, a.im))};
}
__device__ __forceinline__ cplx fnma(cplx a, double f, cplx b) { return cplx{fma_(-f, b.re, a.re), fma_(-f, b.im, a.im)}; }
__device__ __forceinline__ double add(double a, double b) { return a + b; }
__device__ __forceinline__ cplx add(cplx a, cplx b) { return cplx{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ double scale(double f, double a) { return f * a; }
__device__ __forceinline__ cplx scale(double f, cplx a) { return cplx{f * a.re, f * a.im}; }
__device__ __forceinline__ double inv(double a) { return 1.0 / a; }
__device__ __forceinline__ cplx inv(cplx a) {
  const double d = fma_(a.im, a.im, a.re * a.re);
  return cplx{a.re / d, -a.im / d};
}
__device__ __forceinline__ bool finite_(double a) { return fabs(a) < INFINITY; }
__device__ __forceinline__ bool finite_(cplx a) { return fabs(a.re) < INFINITY && fabs(a.im) < INFINITY; }
__device__ __forceinline__ double abs2(double a) { return a * a; }
__device__ __forceinline__ double abs2(cplx a) { return fma_(a.im, a.im, a.re * a.re); }
__device__ __forceinline__ bool nonzero(double a) { return a != 0.0; }
__device__ __forceinline__ bool nonzero(cplx a) { return a.re != 0.0 || a.im != 0.0; }
__device__ __forceinline__ double sel(bool c, double a, double b) { return c ? a : b; }
__device__ __forceinline__ cplx sel(bool c, cplx a, cplx b) { return cplx{c ? a.re : b.re, c ? a.im : b.im}; }
// i w a
__device__ __forceinline__ double times_iw(double, double) { return 0.0; }
__device__ __forceinline__ cplx times_iw(double w, cplx a) { return cplx{-w * a.im, w * a.re}; }

template <class T>
__device__ __forceinline__ void put(double* row, size_t at, T v, bool nan) {
  const double bad = __builtin_nan("");
  row[2 * at] = nan ? bad : re_(v);
  row[2 * at + 1] = nan ? bad : im_(v);
}

// B(u) = u / (exp(u) - 1) and dB/du, series below |u| = 0.05.  The entries of the Jacobian are formed with IEEE divisions and the
// library's expm1 / log1p / exp, operation by operation in the order of oracle/pnp_physical.py: an entry that is off by an ulp moves the
// solution by cond(J) ulp, which is what the solution methods themselves lose
__device__ __forceinline__ void bernoulli2(double u, double& B, double& dB) {
  if (fabs(u) < 0.05) {
    const double u2 = u * u;
    B = 1.0 - 0.5 * u + u2 * (1.0 / 12.0 + u2 * (-1.0 / 720.0 + u2 * (1.0 / 30240.0)));
    dB = -0.5 + u * (1.0 / 6.0 + u2 * (-1.0 / 180.0 + u2 * (1.0 / 5040.0)));
  } else {
    const double E = expm1(u);
    B = u / E;
    dB = (1.0 - B - u) / E;
  }
}

struct Edge {
  double Bp, Bm, Ju;   // w_e B(u), w_e (B(u) + u), dJhat/du
};

// g and dg/dc_s of wall reaction r at the wall state (cs: the driving concentration, 1 for species -1)
__device__ __forceinline__ void wall_law(const Table& tb, int r, double cs, double dphi, double& g, double& dg) {
  const double al = tb.alpha[r];
  const double den = 1.0 / (1.0 + tb.sat[r] * cs);
  const double E = al != 0.0 ? exp(al * dphi) : 1.0;
  g = cs * den * E;
  dg = den * den * E;
}

template <int NB, bool CX, bool REC>
__global__ __launch_bounds__(64) void response_kernel(const KArgs A) {
  using T = typename Num<CX>::T;
  constexpr int N = NB - 1, TPW = 64 / NB, RW = (TPW + 1) * NB;
  const int lane = threadIdx.x;
  const int team = lane / NB, r0 = lane - team * NB, base = team * NB;   // team TPW: the partial team of the lanes left over
  const bool isP = r0 == N;
  const int nx = A.nx;
  const Table& tb = *A.tab;

  __shared__ double ring[3][RW];          // the unknowns of the last three grid points, one column per lane
  __shared__ T prow[2][TPW + 1][2 * NB];  // the pivot row of an elimination step (two buffers: one wave-level sync per step)
  __shared__ T tmat[TPW + 1][NB][NB];     // T_i
  __shared__ T t1row[TPW + 1][NB];        // row N of T_1

  const double Dk = A.sp[r0 * SPF], qb = A.sp[r0 * SPF + 1], rs = A.sp[r0 * SPF + 2], vdx = A.sp[r0 * SPF + 3];
  const double dx = A.sp[r0 * SPF + 4];   // 0 on row N

  for (int64_t grp = blockIdx.x; grp * TPW < A.nsys; grp += gridDim.x) {
    const int64_t sys = grp * TPW + team;
    const bool live = team < TPW && sys < A.nsys;
    const int64_t sy = live ? sys : grp * TPW;
    const int64_t li = sy / A.F;
    const int f = (int)(sy - li * A.F);
    const int64_t b = A.lanes[li];
    const double* urow = isP ? A.phi + (size_t)b * A.ldx : A.c + ((size_t)b * N + r0) * A.ldx;
    const double omega = CX ? A.omega[f] : 0.0;
    const double phiM = A.phiM[b];
    bool bad = false;

    // a grid point enters: the lane's own unknown goes to the ring, phi and the steric terms of the point come back
    const auto point = [&](int i, double own, double& ph, double& w, double& gf) {
      double* slot = ring[i % 3];
      slot[base + r0] = own;
      pnp::lds_sync();
      ph = slot[base + N];
      w = 0.0;
      gf = 1.0;
      if (A.steric) {
        double p0 = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) p0 = p0 + A.volk[j] * slot[base + j];
        w = -log1p(-p0);
        gf = 1.0 - p0;   // the free volume fraction: g_j = vol_j / gf, gamma = 1 / gf
      }
    };
    // edge e between a left and a right point, for the species of this lane
    const auto edge = [&](int e, double cl, double cr, double phl, double phr, double wl, double wr) {
      const double wg = A.wgt[e];
      double u = qb * (phr - phl) + (wr - wl);
      if (vdx != 0.0) u = u - vdx / (Dk * wg);
      double B, dB;
      bernoulli2(u, B, dB);
      Edge E;
      E.Bp = wg * B;
      E.Bm = wg * (B + u);
      E.Ju = -wg * ((dB + 1.0) * cr - dB * cl);
      return E;
    };

    // points in registers: R, C, L = i+1, i, i-1 of the block row i in work, LL = i-2 (entered one block row ahead)
    double cR, cC, cL, cLL = 0.0, phR, phC, phL, phLL = 0.0, wR, wC, wL, wLL = 0.0, gR, gC, gL, gLL = 1.0;
    cR = urow[nx - 1];
    cC = urow[nx - 2];
    cL = urow[nx - 3];
    const double c4 = nx >= 4 ? urow[nx - 4] : 0.0;
    point(nx - 1, cR, phR, wR, gR);
    point(nx - 2, cC, phC, wC, gC);
    point(nx - 3, cL, phL, wL, gL);
    Edge eR = edge(nx - 2, cC, cR, phC, phR, wC, wR), eL = edge(nx - 3, cL, cC, phL, phC, wL, wC);

    T Aw[2 * NB];     // [D'_i | L_i], row r0
    double Ur[NB];    // U_i, row r0
    double rhs0 = 0.0;

    // rows r0 of M_i, L_i, U_i from the three points and two edges in registers (centre C = point i); the wall terms at i = 0
    const auto assemble = [&](int i, T (&Mr)[NB], double (&Lr)[NB], const double (&wallM)[NB]) {
      const double vi = A.vol[i];
      double mN = eR.Ju * (-qb) - eL.Ju * qb + wallM[N];
      double dR[N > 0 ? N : 1];
#pragma unroll
      for (int j = 0; j < N; ++j) dR[j] = 0.0;
      if (A.nreact > 0) {
        const double* cc = ring[i % 3] + base;
        for (int r = 0; r < A.nreact; ++r) {
          const double net = tb.net[r][r0];
#pragma unroll 1
          for (int sd = 0; sd < 2; ++sd) {
            const double kk = tb.kk[sd][r];
            if (kk == 0.0) continue;   // a side whose rate constant is 0 contributes nothing
            const int m = tb.n_side[sd][r];
            const double gam = 1.0 / gC;
            double gp = 1.0;
            for (int e = 0; e < m; ++e) gp *= gam;
            const double gm = kk * gp;
            double prod = gm;
            double vals[MAXT];
            int ids[MAXT];
#pragma unroll
            for (int e = 0; e < MAXT; ++e) {
              ids[e] = e < m ? tb.side[sd][r][e] : -1;
              vals[e] = e < m ? cc[ids[e]] : 1.0;
              prod *= vals[e];
            }
            const double sgn = sd == 0 ? net : -net;
#pragma unroll
            for (int j = 0; j < N; ++j) {
              double rest = gm;
              int cnt = 0;
#pragma unroll
              for (int e = 0; e < MAXT; ++e) {
                const bool hit = ids[e] == j;
                rest *= (hit && cnt == 0) ? 1.0 : vals[e];
                cnt += hit ? 1 : 0;
              }
              double d = cnt ? (double)cnt * rest : 0.0;
              if (A.steric) d += prod * (double)m * (A.volk[j] * (gam * gam)) / gam;   // d gamma^m / d c_j = m gamma^m vol_j gamma
              dR[j] = fma_(sgn, d, dR[j]);
            }
          }
        }
      }
      const double wl = i > 0 ? A.wgt[i - 1] : 0.0, wr = A.wgt[i];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const bool dg = j == r0;
        // diagonal, (wall table), steric coupling, reactions: the oracle's order of accumulation
        double sm = dg ? eR.Bp + eL.Bm : 0.0, su = dg ? -eR.Bm : 0.0, sl = dg ? -eL.Bp : 0.0;
        sm += wallM[j];
        if (A.steric) {
          sm += -eR.Ju * (A.volk[j] / gC) - eL.Ju * (A.volk[j] / gC);
          su += eR.Ju * (A.volk[j] / gR);
          sl += eL.Ju * (A.volk[j] / gL);
        }
        sm += -rs * vi * dR[j];
        const double pm = i > 0 ? A.pe * vi * A.q[j] : 0.0;
        Mr[j] = make<T>(isP ? pm : sm, (CX && dg) ? omega * rs * vi : 0.0);
        Ur[j] = isP ? 0.0 : su;
        Lr[j] = isP ? 0.0 : sl;
      }
      double pmm = -(wr + wl), puu = wr;
      if (i == 0) {
        pmm = A.stern ? -wr - A.sternc : 1.0;
        puu = A.stern ? wr : 0.0;
      }
      mN = isP ? pmm : mN;
      Ur[N] = isP ? puu : eR.Ju * qb;
      Lr[N] = isP ? wl : eL.Ju * qb;
      Mr[N] = make<T>(mN, 0.0);
    };
    // the wall terms of row 0, formed before the row: the right-hand side and the wall table's part of M_0
    const auto wall_terms = [&](double (&wallM)[NB]) {
      {
        // right-hand side and wall table
        rhs0 = 0.0;
        if (A.pert == CATRESP_PHIM) rhs0 = isP ? (A.stern ? -A.sternc : 1.0) : 0.0;
        else rhs0 = r0 == A.pspecies ? dx / Dk : 0.0;
        const double* cc = ring[0] + base;
        for (int r = 0; r < A.nwall; ++r) {
          const int s = tb.wspecies[r];
          double g, dg;
          wall_law(tb, r, s >= 0 ? cc[s] : 1.0, phiM - phC, g, dg);
          const double nk = tb.nu[r][r0] * A.kwall[b * A.nwall + r];
#pragma unroll
          for (int j = 0; j < N; ++j) wallM[j] += j == s ? -nk * dg * dx / Dk : 0.0;
          const double t = nk * tb.alpha[r] * g * dx / Dk;
          wallM[N] += t;
          if (A.pert == CATRESP_PHIM) rhs0 += t;
        }
      }
    };

    {
      // row nx-2: T_{nx-1} = 0, so D' = M
      T Mr[NB];
      double Lr[NB], wallM[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) wallM[j] = 0.0;
      assemble(nx - 2, Mr, Lr, wallM);
#pragma unroll
      for (int j = 0; j < NB; ++j) Aw[j] = Mr[j], Aw[NB + j] = make<T>(Lr[j], 0.0);
      if (nx >= 4) {
        cLL = c4;
        point(nx - 4, cLL, phLL, wLL, gLL);
      }
    }
    T* wsT = nullptr;
    if constexpr (REC) wsT = static_cast<T*>(A.ws) + ((size_t)blockIdx.x * TPW + (team < TPW ? team : 0)) * (size_t)nx * NB * NB;

#pragma unroll 1
    for (int i = nx - 2; i >= 0; --i) {
      const double nxt = i >= 3 ? urow[i - 3] : 0.0;   // the point the row after next needs: used at the end of this block row
      if (i == 0) {
        Aw[NB] = make<T>(rhs0, 0.0);
#pragma unroll
        for (int j = 1; j < NB; ++j) Aw[NB + j] = make<T>(0.0, 0.0);
      }
      // ---- Gauss-Jordan on [D' | L] across the team, no row exchanges ----
#pragma unroll
      for (int p = 0; p < NB; ++p) {
        const bool mine = r0 == p;
        const T piv = Aw[p];
        bad = bad || (mine && !(nonzero(piv) && finite_(piv)));
        const T ip = inv(piv);
        T* pr = prow[p & 1][team];
#pragma unroll
        for (int j = p + 1; j < 2 * NB; ++j) Aw[j] = sel(mine, mul(Aw[j], ip), Aw[j]);
        if (mine) {
          pr[p] = piv;
#pragma unroll
          for (int j = p + 1; j < 2 * NB; ++j) pr[j] = Aw[j];
        }
        pnp::lds_sync();
        // the pivot monitor: what partial pivoting would have checked -- an entry below the pivot beyond the growth limit times the pivot
        bad = bad || (r0 > p && abs2(piv) > GROWTH2 * abs2(pr[p]));
#pragma unroll
        for (int j = p + 1; j < 2 * NB; ++j) Aw[j] = sel(mine, Aw[j], fnma(Aw[j], piv, pr[j]));
      }
      if (i == 0) break;
      // ---- T_i = Aw[NB ..]: to the team, to the records ----
#pragma unroll
      for (int j = 0; j < NB; ++j) tmat[team][r0][j] = Aw[NB + j];
      if (i == 1 && isP) {
#pragma unroll
        for (int j = 0; j < NB; ++j) t1row[team][j] = Aw[NB + j];
      }
      if constexpr (REC) {
        if (live) {
          T* rec = wsT + ((size_t)i * NB + r0) * NB;
#pragma unroll
          for (int j = 0; j < NB; ++j) rec[j] = Aw[NB + j];
        }
      }
      // ---- row i-1 ----
      cR = cC, phR = phC, wR = wC, gR = gC;
      cC = cL, phC = phL, wC = wL, gC = gL;
      cL = cLL, phL = phLL, wL = wLL, gL = gLL;
      eR = eL;
      if (i >= 2) eL = edge(i - 2, cL, cC, phL, phC, wL, wC);
      else eL = {0.0, 0.0, 0.0};   // the wall row has no left edge
      T Mr[NB];
      double Lr[NB], wallM[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) wallM[j] = 0.0;
      if (i == 1) wall_terms(wallM);
      assemble(i - 1, Mr, Lr, wallM);
      pnp::lds_sync();
      if (A.steric) {
#pragma unroll
        for (int s = 0; s < NB; ++s) {
#pragma unroll
          for (int j = 0; j < NB; ++j) Mr[j] = fnma(Mr[j], Ur[s], tmat[team][s][j]);
        }
      } else {
        // point ions: U has its diagonal and the phi column
        double ud = 0.0;
#pragma unroll
        for (int s = 0; s < NB; ++s) ud = s == r0 ? Ur[s] : ud;
        const double uN = isP ? 0.0 : Ur[N];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          Mr[j] = fnma(Mr[j], ud, Aw[NB + j]);
          Mr[j] = fnma(Mr[j], uN, tmat[team][N][j]);
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) Aw[j] = Mr[j], Aw[NB + j] = make<T>(Lr[j], 0.0);
      // the point the row after next needs on its left (its ring slot held point i, which no row needs any more)
      if (i >= 3) {
        cLL = nxt;
        point(i - 3, cLL, phLL, wLL, gLL);
      }
    }

    // ---- the wall: du_0[r0] = Aw[NB] ----
    const T du0 = Aw[NB];
    T* x0 = prow[0][team];
    pnp::lds_sync();   // the last elimination step has read its pivot row
    x0[r0] = du0;
    pnp::lds_sync();
    const T dph0 = x0[N];
    const double dphiM = A.pert == CATRESP_PHIM ? 1.0 : 0.0;
    const T drive = fnma(make<T>(dphiM, 0.0), make<T>(1.0, 0.0), dph0);   // dphiM - du[phi, 0]
    // flux response of this lane's species
    T dwf = make<T>((A.pert == CATRESP_WALL_FLUX && r0 == A.pspecies) ? 1.0 : 0.0, 0.0);
    {
      const double* cc = ring[0] + base;
      const double ph0 = cc[N];
      for (int r = 0; r < A.nwall; ++r) {
        const int s = tb.wspecies[r];
        double g, dg;
        wall_law(tb, r, s >= 0 ? cc[s] : 1.0, phiM - ph0, g, dg);
        const double nk = tb.nu[r][r0] * A.kwall[b * A.nwall + r];
        const T dcs = s >= 0 ? x0[s] : make<T>(0.0, 0.0);
        dwf = add(dwf, scale(nk, add(scale(dg, dcs), scale(tb.alpha[r] * g, drive))));
      }
    }
    x0[NB + r0] = dwf;
    pnp::lds_sync();
    T dsig, adm = make<T>(0.0, 0.0);
    if (A.stern) {
      dsig = scale(A.CS, drive);
    } else {
      // du[phi, 1] = -(row N of T_1) du_0
      T d1 = make<T>(0.0, 0.0), qs = make<T>(0.0, 0.0);
#pragma unroll
      for (int j = 0; j < NB; ++j) d1 = fnma(d1, t1row[team][j], x0[j]);
#pragma unroll
      for (int j = 0; j < N; ++j) qs = add(qs, scale(A.q[j], x0[j]));
      dsig = add(scale(-A.eps / A.h0, fnma(d1, make<T>(1.0, 0.0), dph0)), scale(-0.5 * A.h0, qs));
    }
#pragma unroll
    for (int j = 0; j < N; ++j) adm = add(adm, scale(A.q[j], x0[NB + j]));
    adm = add(adm, times_iw(omega, dsig));
    bad = bad || !finite_(du0) || !finite_(dwf) || !finite_(dsig) || !finite_(adm);
    const bool unsolved = A.st[b] != 0;

    // ---- profiles: du_i = -T_i du_{i-1}, the records read back by the lane that wrote them ----
    if constexpr (REC) {
      double* prof = nullptr;
      if (live) prof = isP ? (A.dphi ? A.dphi + 2 * (size_t)sys * nx : nullptr) : (A.dc ? A.dc + 2 * ((size_t)sys * N + r0) * nx : nullptr);
      if (prof) put<T>(prof, 0, du0, unsolved);
      T* xa = prow[1][team];
      // x0 holds du_0 in its first NB entries; the two buffers alternate
#pragma unroll 1
      for (int i = 1; i <= nx - 2; ++i) {
        const T* xp = (i & 1) ? x0 : xa;
        T* xn = (i & 1) ? xa : x0;
        const T* rec = wsT + ((size_t)i * NB + r0) * NB;
        T v = make<T>(0.0, 0.0);
        if (live) {
#pragma unroll
          for (int j = 0; j < NB; ++j) v = fnma(v, rec[j], xp[j]);
        }
        bad = bad || !finite_(v);
        xn[r0] = v;
        pnp::lds_sync();
        if (prof) put<T>(prof, i, v, unsolved);
      }
      if (prof) put<T>(prof, nx - 1, make<T>(0.0, 0.0), unsolved);
    }

    // ---- status of the system: any lane of the team ----
    pnp::lds_sync();
    ring[0][base + r0] = bad ? 1.0 : 0.0;
    pnp::lds_sync();
    double anybad = 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) anybad += ring[0][base + j];
    if (live) {
      if (isP) {
        if (A.dphis) put<T>(A.dphis, sys, dph0, unsolved);
        if (A.dsig) put<T>(A.dsig, sys, dsig, unsolved);
        if (A.adm) put<T>(A.adm, sys, adm, unsolved);
        if (A.status) A.status[sys] = unsolved ? 2 : (anybad != 0.0 ? 1 : 0);
      } else {
        if (A.dcs) put<T>(A.dcs, (size_t)sys * N + r0, du0, unsolved);
        if (A.dwf) put<T>(A.dwf, (size_t)sys * N + r0, dwf, unsolved);
      }
    }
    pnp::lds_sync();   // the ring and the exchange buffers are free for the next group
  }
}

template <int NB, bool CX, bool REC>
static hipError_t launch(const KArgs& a, int64_t blocks, hipStream_t st) {
  hipLaunchKernelGGL((response_kernel<NB, CX, REC>), dim3((int)blocks), dim3(64), 0, st, a);
  return hipSuccess;
}

template <int NB, bool CX, bool REC>
static hipError_t resident(int* per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, response_kernel<NB, CX, REC>, 64, 0);
}

// the compiled instances: NB = 2 .. 9, real / complex, scalars only / records.  f(ic<NB>, bool_constant<CX>, bool_constant<REC>)
template <class Fn>
static void dispatch(int NB, bool cx, bool rec, Fn&& f) {
  const auto with_nb = [&](auto nb) {
    if (cx && rec) f(nb, std::true_type(), std::true_type());
    else if (cx) f(nb, std::true_type(), std::false_type());
    else if (rec) f(nb, std::false_type(), std::true_type());
    else f(nb, std::false_type(), std::false_type());
  };
  switch (NB) {
    case 2: with_nb(ic<2>()); break;
    case 3: with_nb(ic<3>()); break;
    case 4: with_nb(ic<4>()); break;
    case 5: with_nb(ic<5>()); break;
    case 6: with_nb(ic<6>()); break;
    case 7: with_nb(ic<7>()); break;
    case 8: with_nb(ic<8>()); break;
    default: with_nb(ic<9>()); break;
  }
}

}  // namespace catresp

static_assert(CATRESP_OK == pnp::post::OK && CATRESP_EINVAL == pnp::post::ERR_INVAL && CATRESP_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATRESP_EDEVICE == pnp::post::ERR_DEVICE && CATRESP_MAX_NX == pnp::post::MAX_NX && CATRESP_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_response.h and pnp_post.h disagree");

struct catresp_ctx : pnp::post::Ctx {
  std::vector<double> stage;    // host: the inputs of the call in flight, one copy
  std::vector<int32_t> flags;   // host: status as the kernel wrote it
};

extern "C" {

int catresp_create(int32_t device, catresp_ctx** out) { return pnp::post::create("catresp_create", device, out); }
void catresp_destroy(catresp_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catresp_last_error(const catresp_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catresp_last_kernel(const catresp_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catresp_last_kernel_ms(const catresp_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catresp_solve(catresp_ctx* ctx, const pnp_device_view* view, const catresp_params* p, const catresp_outputs* out) {
  using namespace catresp;
  static const char entry[] = "catresp_solve";
  if (const int rc = check_view(ctx, entry, "catresp_params", view, p, out)) return rc;
  const int N = view->nspecies, nx = view->nx, NB = N + 1;
  const int64_t B = view->batch;
  char msg[256];
  const auto posfin = [](double v) { return v > 0.0 && std::isfinite(v); };
  if (p->max_waves < 0) return fail(ctx, CATRESP_EINVAL, "catresp_solve: negative max_waves");
  if (!view->status_dev) return fail(ctx, CATRESP_EINVAL, "catresp_solve: the view has no status row");
  if (!posfin(p->beta) || !posfin(p->eps) || !posfin(p->dx) || !std::isfinite(p->velocity))
    return fail(ctx, CATRESP_EINVAL, "catresp_solve: beta, eps and dx must be positive and finite, velocity finite");
  if (p->wall_bc != CATRESP_WALL_DIRICHLET && p->wall_bc != CATRESP_WALL_STERN) return fail(ctx, CATRESP_EINVAL, "catresp_solve: unknown wall_bc");
  if (p->wall_bc == CATRESP_WALL_STERN && !posfin(p->stern_capacitance))
    return fail(ctx, CATRESP_EINVAL, "catresp_solve: a Stern wall needs a positive, finite capacitance");
  if (p->perturbation != CATRESP_PHIM && p->perturbation != CATRESP_WALL_FLUX) return fail(ctx, CATRESP_EINVAL, "catresp_solve: unknown perturbation");
  if (p->perturbation == CATRESP_WALL_FLUX && (p->species < 0 || p->species >= N)) {
    snprintf(msg, sizeof msg, "catresp_solve: perturbed species %d outside [0, %d)", p->species, N);
    return fail(ctx, CATRESP_EINVAL, msg);
  }
  for (int k = 0; k < N; ++k) {
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    if (!posfin(p->D[k]) || !std::isfinite(p->charges[k]) || !(r >= 0.0) || !std::isfinite(r)) {
      snprintf(msg, sizeof msg, "catresp_solve: species %d needs D > 0, a finite charge and a radius >= 0 (all finite)", k);
      return fail(ctx, CATRESP_EINVAL, msg);
    }
  }
  const int R = p->nreactions, W = p->n_wall, F = p->nfreq;
  if (R < 0 || R > PNP_MAX_REACTIONS) {
    snprintf(msg, sizeof msg, "catresp_solve: nreactions = %d outside [0, %d]", R, PNP_MAX_REACTIONS);
    return fail(ctx, CATRESP_EINVAL, msg);
  }
  if (W < 0 || W > PNP_MAX_WALL_REACTIONS) {
    snprintf(msg, sizeof msg, "catresp_solve: n_wall = %d outside [0, %d]", W, PNP_MAX_WALL_REACTIONS);
    return fail(ctx, CATRESP_EINVAL, msg);
  }
  if (R > 0 && (!p->n_lhs || !p->lhs || !p->n_rhs || !p->rhs || !p->kf || !p->kr))
    return fail(ctx, CATRESP_EINVAL, "catresp_solve: nreactions > 0 needs n_lhs, lhs, n_rhs, rhs, kf and kr");
  for (int r = 0; r < R; ++r) {
    if (p->n_lhs[r] < 0 || p->n_lhs[r] > PNP_MAX_REACTANTS || p->n_rhs[r] < 0 || p->n_rhs[r] > PNP_MAX_REACTANTS) {
      snprintf(msg, sizeof msg, "catresp_solve: reaction %d has n_lhs / n_rhs outside [0, %d]", r, PNP_MAX_REACTANTS);
      return fail(ctx, CATRESP_EINVAL, msg);
    }
    for (int side = 0; side < 2; ++side)
      for (int j = 0; j < (side ? p->n_rhs[r] : p->n_lhs[r]); ++j) {
        const int s = (side ? p->rhs : p->lhs)[r * PNP_MAX_REACTANTS + j];
        if (s < 0 || s >= N) {
          snprintf(msg, sizeof msg, "catresp_solve: reaction %d names species index %d outside [0, %d)", r, s, N);
          return fail(ctx, CATRESP_EINVAL, msg);
        }
      }
  }
  if (W > 0 && !p->k) return fail(ctx, CATRESP_EINVAL, "catresp_solve: n_wall > 0 needs the rate constants k");
  if (W > 0 && (!p->wall_species || !p->nu)) return fail(ctx, CATRESP_EINVAL, "catresp_solve: n_wall > 0 needs wall_species and nu");
  for (int r = 0; r < W; ++r)
    if (p->wall_species[r] < -1 || p->wall_species[r] >= N) {
      snprintf(msg, sizeof msg, "catresp_solve: wall reaction %d names species index %d outside [-1, %d)", r, p->wall_species[r], N);
      return fail(ctx, CATRESP_EINVAL, msg);
    }
  if (F < 1 || F > CATRESP_MAX_FREQ) {
    snprintf(msg, sizeof msg, "catresp_solve: nfreq = %d outside [1, %d]", F, CATRESP_MAX_FREQ);
    return fail(ctx, CATRESP_EINVAL, msg);
  }
  if (!p->phiM || !p->omega) return fail(ctx, CATRESP_EINVAL, "catresp_solve: phiM and omega are required");
  bool complex_call = false;
  for (int f = 0; f < F; ++f) {
    if (!(p->omega[f] >= 0.0) || !std::isfinite(p->omega[f])) {
      snprintf(msg, sizeof msg, "catresp_solve: omega[%d] must be >= 0 and finite", f);
      return fail(ctx, CATRESP_EINVAL, msg);
    }
    complex_call = complex_call || p->omega[f] != 0.0;
  }
  if (p->nlanes < 0) return fail(ctx, CATRESP_EINVAL, "catresp_solve: nlanes < 0");
  const int64_t n = p->nlanes;
  if (!p->lanes && n > B) return fail(ctx, CATRESP_EINVAL, "catresp_solve: nlanes above the batch (lanes is NULL)");
  if (p->lanes)
    for (int64_t i = 0; i < n; ++i)
      if (p->lanes[i] < 0 || p->lanes[i] >= B) {
        snprintf(msg, sizeof msg, "catresp_solve: lane index %lld outside [0, %lld)", (long long)p->lanes[i], (long long)B);
        return fail(ctx, CATRESP_EINVAL, msg);
      }
  if (n == 0) return CATRESP_OK;

  KArgs a;
  memset(&a, 0, sizeof a);
  a.nx = nx; a.ldx = view->row_pitch; a.nreact = R; a.nwall = W; a.stern = p->wall_bc == CATRESP_WALL_STERN;
  a.pert = p->perturbation; a.pspecies = p->species; a.F = F; a.nsys = n * F;
  a.c = view->c_dev; a.phi = view->phi_dev; a.st = view->status_dev;
  a.pe = p->dx * p->dx / p->eps;
  a.sternc = a.stern ? p->dx * p->stern_capacitance / p->eps : 0.0;
  a.CS = a.stern ? p->stern_capacitance : 0.0;
  a.eps = p->eps;
  a.h0 = p->x[1] - p->x[0];
  for (int k = 0; k < N; ++k) {
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    a.volk[k] = pnp::N_AVOGADRO * r * r * r;
    a.q[k] = p->charges[k];
    a.steric = a.steric || a.volk[k] != 0.0;
  }
  const bool rec = out->dc || out->dphi;
  const int TPW = 64 / NB;

  // the inputs, staged on the host for one copy: edge weights, control volumes, row constants, potentials, rate constants,
  // frequencies, lanes (int64 in the place of doubles), tables
  const size_t o_w = 0, o_v = o_w + even((size_t)nx - 1), o_sp = o_v + even(nx), o_p = o_sp + (size_t)(MAXS + 1) * SPF, o_k = o_p + even(B),
               o_f = o_k + even((size_t)B * W), o_l = o_f + even(F), o_t = o_l + (size_t)n, n_in = o_t + sizeof(Table) / 8;
  const size_t nsys = (size_t)n * F;
  try {
    ctx->stage.assign(n_in, 0.0);
    ctx->flags.assign(nsys, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATRESP_ENOMEM, "catresp_solve: out of host memory");
  }
  double* sg = ctx->stage.data();
  for (int e = 0; e < nx - 1; ++e) sg[o_w + e] = p->dx / (p->x[e + 1] - p->x[e]);
  for (int i = 0; i < nx; ++i) {
    const double hl = i > 0 ? p->x[i] - p->x[i - 1] : 0.0, hr = i < nx - 1 ? p->x[i + 1] - p->x[i] : 0.0;
    sg[o_v + i] = 0.5 * (hr + hl) / p->dx;
  }
  for (int k = 0; k <= N; ++k) {
    double* s = sg + o_sp + k * SPF;
    s[0] = 1.0;
    if (k < N) {
      s[0] = p->D[k];
      s[1] = p->charges[k] * p->beta;
      s[2] = p->dx * p->dx / p->D[k];
      s[3] = p->velocity * p->dx;
      s[4] = p->dx;
    }
  }
  memcpy(sg + o_p, p->phiM, (size_t)B * 8);
  if (W) memcpy(sg + o_k, p->k, (size_t)B * W * 8);
  memcpy(sg + o_f, p->omega, (size_t)F * 8);
  {
    int64_t* l = reinterpret_cast<int64_t*>(sg + o_l);
    for (int64_t i = 0; i < n; ++i) l[i] = p->lanes ? p->lanes[i] : i;
  }
  Table* tb = reinterpret_cast<Table*>(sg + o_t);
  for (int r = 0; r < R; ++r) {
    tb->n_side[0][r] = p->n_lhs[r];
    tb->n_side[1][r] = p->n_rhs[r];
    tb->kk[0][r] = p->kf[r];
    tb->kk[1][r] = p->kr[r];
    for (int j = 0; j < p->n_lhs[r]; ++j) tb->net[r][tb->side[0][r][j] = p->lhs[r * PNP_MAX_REACTANTS + j]] -= 1.0;
    for (int j = 0; j < p->n_rhs[r]; ++j) tb->net[r][tb->side[1][r][j] = p->rhs[r * PNP_MAX_REACTANTS + j]] += 1.0;
  }
  for (int r = 0; r < W; ++r) {
    tb->wspecies[r] = p->wall_species[r];
    tb->alpha[r] = p->alpha ? p->alpha[r] : 0.0;
    tb->sat[r] = p->saturation ? p->saturation[r] : 0.0;
    for (int k = 0; k < N; ++k) tb->nu[r][k] = p->nu[r * N + k];
  }

  // the rows that were asked for (complex: two doubles per entry)
  const Row rows[] = {{out->dphi_surface, &a.dphis, 2 * nsys}, {out->dc_surface, &a.dcs, 2 * nsys * N}, {out->dsigma, &a.dsig, 2 * nsys},
                      {out->dwall_flux, &a.dwf, 2 * nsys * N}, {out->admittance, &a.adm, 2 * nsys}, {out->dc, &a.dc, 2 * nsys * N * nx},
                      {out->dphi, &a.dphi, 2 * nsys * nx}};
  const size_t need_out = rows_doubles(rows), n_flags = even((nsys + 1) / 2);
  if (!need_out && !out->status) return CATRESP_OK;

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  // persistent grid: as many waves as the device holds at once unless the caller sizes it, no more than there are groups of systems;
  // with records, no more than the workspace cap admits (at least one)
  const int64_t groups = ((int64_t)nsys + TPW - 1) / TPW;
  int64_t blocks = p->max_waves;
  if (blocks == 0) {
    int cus = 0, per_cu = 0;
    PNP_POST_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    hipError_t oe = hipSuccess;
    dispatch(NB, complex_call, rec, [&](auto nb, auto cx, auto rc_) { oe = resident<decltype(nb)::value, decltype(cx)::value, decltype(rc_)::value>(&per_cu); });
    PNP_POST_HIP(oe);
    blocks = (int64_t)std::max(per_cu, 1) * std::max(cus, 1);
  }
  blocks = std::min(std::max<int64_t>(blocks, 1), groups);
  size_t ws_doubles = 0;
  if (rec) {
    size_t cap = (size_t)2 << 30;
    if (const char* e = getenv("CATRESP_WORKSPACE_BYTES")) {
      char* end = nullptr;
      const unsigned long long v = strtoull(e, &end, 10);
      if (end && end != e && *end == 0) cap = (size_t)v;
    }
    const size_t per_wave = (size_t)TPW * nx * NB * NB * (complex_call ? 2 : 1);   // doubles
    blocks = std::min<int64_t>(blocks, std::max<int64_t>(1, (int64_t)(cap / 8 / per_wave)));
    ws_doubles = (size_t)blocks * per_wave;
  }
  if (const int rc = reserve(ctx, entry, n_in + need_out + n_flags + ws_doubles)) return rc;
  a.wgt = ctx->buf + o_w;
  a.vol = ctx->buf + o_v;
  a.sp = ctx->buf + o_sp;
  a.phiM = ctx->buf + o_p;
  a.kwall = ctx->buf + o_k;
  a.omega = ctx->buf + o_f;
  a.lanes = reinterpret_cast<const int64_t*>(ctx->buf + o_l);
  a.tab = reinterpret_cast<const Table*>(ctx->buf + o_t);
  double* cur = place_rows(rows, ctx->buf + n_in);
  a.status = reinterpret_cast<int32_t*>(cur);
  a.ws = cur + n_flags;
  PNP_POST_HIP(hipMemcpyAsync(ctx->buf, sg, n_in * sizeof(double), hipMemcpyHostToDevice, st));
  if (!ctx->ev0) PNP_POST_HIP(hipEventCreate(&ctx->ev0));
  if (!ctx->ev1) PNP_POST_HIP(hipEventCreate(&ctx->ev1));
  ctx->kernel_ms = -1.0f;
  PNP_POST_HIP(hipEventRecord(ctx->ev0, st));
  hipError_t le = hipSuccess;
  dispatch(NB, complex_call, rec, [&](auto nb, auto cx, auto rc_) { le = launch<decltype(nb)::value, decltype(cx)::value, decltype(rc_)::value>(a, blocks, st); });
  PNP_POST_HIP(le);
  PNP_POST_HIP(hipGetLastError());
  PNP_POST_HIP(hipEventRecord(ctx->ev1, st));
  for (const Row& r : rows)
    if (r.wanted()) PNP_POST_HIP(hipMemcpyAsync(r.host, *r.dev, r.n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (out->status) PNP_POST_HIP(hipMemcpyAsync(ctx->flags.data(), a.status, nsys * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PNP_POST_HIP(hipStreamSynchronize(st));
  PNP_POST_HIP(hipEventElapsedTime(&ctx->kernel_ms, ctx->ev0, ctx->ev1));
  if (out->status) memcpy(out->status, ctx->flags.data(), nsys * sizeof(int32_t));
  snprintf(msg, sizeof msg, "catresp::response_kernel<%d, %s, %s>", NB, complex_call ? "true" : "false", rec ? "true" : "false");
  ctx->last_kernel = msg;
  return CATRESP_OK;
}

}  // extern "C"
