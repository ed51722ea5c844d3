// libcatint_couple (include/catint_couple.h): one Newton step of the self-consistency between kinetics and transport per operating
// point, formed on the device from the state a pnp_handle holds there.  It shares no code with the Newton kernels or with
// response/catresp.hip: the row assembly of the stationary Jacobian is restated here from the definitions of catint_response.h (with
// n_wall = 0), real arithmetic only.  gfx950 / MI355X only.
//
// Mapping (that of catresp::response_kernel<NB, false, false>): a TEAM of NB = N + 1 adjacent lanes per system;
// lane r owns row r of the working block row [D' | L] (2 NB numbers) in registers.  64 / NB teams per wave, one wave per workgroup, no
// workgroup barrier; persistent waves walk groups of systems.  Lanes beyond the last full team form a partial team with an LDS area of
// its own and systems beyond the last one repeat a valid one: both run every step and only skip their stores.
// Elimination: block Thomas from the bulk towards the wall, T_i = D'_i^-1 L_i by Gauss-Jordan without row exchanges across the team,
// D'_{i-1} = M_{i-1} - U_{i-1} T_i, every step monitored as in catresp.hip (status 1).  Nothing is kept between block rows.
// The wall: Gauss-Jordan on [W | E], E = diag(dx / D_k) with a zero Poisson row, leaves row r of the transport tangent T = W^-1 E in
// lane r (rows 0 .. N-1: T_c, row N: T_phi) -- all N columns from the one elimination.  Lane k < N then forms row k of
// A = I - rf (Kc T_c + Kphi (x) T_phi) and the entry -G_k of the right-hand side, the team eliminates A by Gauss-Jordan WITH partial
// row pivoting (the pivot lane is found through LDS, rows stay where they are), applies the damping rule and stores.  O(N^3) per
// system on top of an elimination that is O(nx N^3).
// Arithmetic order is fixed in the source (no implicit contraction); the elimination of a column of E performs the operations
// catresp.hip performs on its single right-hand side, in the same order.  Results leave through plain vector stores.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../../include/catint_couple.h"
#include "../pnp_post.h"

#pragma clang fp contract(off)

namespace catcpl {

using namespace pnp::post;

constexpr int MAXS = CATCPL_MAX_SPECIES, MAXR = PNP_MAX_REACTIONS, MAXT = PNP_MAX_REACTANTS;
constexpr double GROWTH2 = CATCPL_PIVOT_GROWTH_LIMIT * CATCPL_PIVOT_GROWTH_LIMIT;
constexpr int SPF = 8;   // per-row constants: D, q beta, dx^2 / D, velocity dx, dx (row N: 1, 0, 0, 0, 0)

// the reaction table of one call, flattened on the host (every index validated there)
struct Table {
  int32_t n_side[2][MAXR];          // entries of the left / right side
  int32_t side[2][MAXR][MAXT];
  double kk[2][MAXR];               // kf, kr
  double net[MAXR][MAXS + 1];       // n_rhs(k, r) - n_lhs(k, r); column N: 0
};
static_assert(sizeof(Table) % 8 == 0, "the table is copied as doubles");

struct KArgs {
  int32_t nx, ldx, nreact, stern, steric, pad_;
  int64_t nsys;            // selected operating points
  const double* c;         // [B][N][ldx]
  const double* phi;       // [B][ldx]
  const int32_t* st;       // [B] solver status
  const int64_t* lanes;    // [n]
  const int32_t* badin;    // [n] 1: an input of the point is not finite
  const double *wgt, *vol; // [nx-1] dx / h_e, [nx] v_i
  const double* sp;        // [NB][SPF]
  const Table* tab;
  const double *g, *K, *Kc, *Kphi;   // [n][N], [n][N], [n][N][N], [n][N]
  double *Tc, *Tphi, *dflux, *lam, *fnew, *dcs, *dphis;   // device rows; null: not wanted
  int32_t* status;
  double volk[MAXS], q[MAXS];   // N_A a_k^3, q_k
  double pe, sternc, rf, dphi_max;   // dx^2 / eps, dx C_S / eps
};

__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
// a - f b
__device__ __forceinline__ double fnma(double a, double f, double b) { return fma_(-f, b, a); }
__device__ __forceinline__ bool finite_(double a) { return fabs(a) < INFINITY; }
// both operands are evaluated before the choice: a select, never a branch around the arithmetic of one side
__device__ __forceinline__ double sel(bool c, double a, double b) { return c ? a : b; }

// B(u) = u / (exp(u) - 1) and dB/du, series below |u| = 0.05.  The entries of the Jacobian are formed with IEEE divisions and the
// library's expm1 / log1p, operation by operation in the order of oracle/pnp_physical.py
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

template <int NB>
__global__ __launch_bounds__(64) void couple_kernel(const KArgs A) {
  constexpr int N = NB - 1, TPW = 64 / NB, RW = (TPW + 1) * NB;
  const int lane = threadIdx.x;
  const int team = lane / NB, r0 = lane - team * NB, base = team * NB;   // team TPW: the partial team of the lanes left over
  const bool isP = r0 == N;
  const int nx = A.nx;
  const Table& tb = *A.tab;

  __shared__ double ring[3][RW];               // the unknowns of the last three grid points, one column per lane
  __shared__ double prow[2][TPW + 1][2 * NB];  // the pivot row of an elimination step (two buffers: one wave-level sync per step)
  __shared__ double tmat[TPW + 1][NB][NB];     // T_i; at the wall the transport tangent
  __shared__ double xch[2][RW];                // the wall stage: pivot search, solution, flags

  const double Dk = A.sp[r0 * SPF], qb = A.sp[r0 * SPF + 1], rs = A.sp[r0 * SPF + 2], vdx = A.sp[r0 * SPF + 3];
  const double dx = A.sp[r0 * SPF + 4];   // 0 on row N

  for (int64_t grp = blockIdx.x; grp * TPW < A.nsys; grp += gridDim.x) {
    const int64_t sys = grp * TPW + team;
    const bool live = team < TPW && sys < A.nsys;
    const int64_t sy = live ? sys : grp * TPW;
    const int64_t b = A.lanes[sy];
    const double* urow = isP ? A.phi + (size_t)b * A.ldx : A.c + ((size_t)b * N + r0) * A.ldx;
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

    double Aw[2 * NB];   // [D'_i | L_i], row r0; at the wall [W | E]
    double Ur[NB];       // U_i, row r0

    // rows r0 of M_i, L_i, U_i from the three points and two edges in registers (centre C = point i)
    const auto assemble = [&](int i, double (&Mr)[NB], double (&Lr)[NB]) {
      const double vi = A.vol[i];
      double mN = eR.Ju * (-qb) - eL.Ju * qb + 0.0;
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
        // diagonal, (no wall table), steric coupling, reactions: the oracle's order of accumulation
        double sm = dg ? eR.Bp + eL.Bm : 0.0, su = dg ? -eR.Bm : 0.0, sl = dg ? -eL.Bp : 0.0;
        sm += 0.0;
        if (A.steric) {
          sm += -eR.Ju * (A.volk[j] / gC) - eL.Ju * (A.volk[j] / gC);
          su += eR.Ju * (A.volk[j] / gR);
          sl += eL.Ju * (A.volk[j] / gL);
        }
        sm += -rs * vi * dR[j];
        const double pm = i > 0 ? A.pe * vi * A.q[j] : 0.0;
        Mr[j] = isP ? pm : sm;
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
      Mr[N] = mN;
    };

    {
      // row nx-2: T_{nx-1} = 0, so D' = M
      double Mr[NB], Lr[NB];
      assemble(nx - 2, Mr, Lr);
#pragma unroll
      for (int j = 0; j < NB; ++j) Aw[j] = Mr[j], Aw[NB + j] = Lr[j];
      if (nx >= 4) {
        cLL = c4;
        point(nx - 4, cLL, phLL, wLL, gLL);
      }
    }

#pragma unroll 1
    for (int i = nx - 2; i >= 0; --i) {
      const double nxt = i >= 3 ? urow[i - 3] : 0.0;   // the point the row after next needs: used at the end of this block row
      if (i == 0) {
        // the wall: the N columns of E in the place of L (column N, the Poisson unknown, is zero)
        const double e0 = dx / Dk;
#pragma unroll
        for (int j = 0; j < NB; ++j) Aw[NB + j] = (j == r0 && !isP) ? e0 : 0.0;
      }
      // ---- Gauss-Jordan on [D' | L] across the team, no row exchanges ----
#pragma unroll
      for (int p = 0; p < NB; ++p) {
        const bool mine = r0 == p;
        const double piv = Aw[p];
        bad = bad || (mine && !(piv != 0.0 && finite_(piv)));
        const double ip = 1.0 / piv;
        double* pr = prow[p & 1][team];
#pragma unroll
        for (int j = p + 1; j < 2 * NB; ++j) Aw[j] = sel(mine, Aw[j] * ip, Aw[j]);
        if (mine) {
          pr[p] = piv;
#pragma unroll
          for (int j = p + 1; j < 2 * NB; ++j) pr[j] = Aw[j];
        }
        pnp::lds_sync();
        // the pivot monitor: what partial pivoting would have checked -- an entry below the pivot beyond the growth limit times the pivot
        bad = bad || (r0 > p && piv * piv > GROWTH2 * (pr[p] * pr[p]));
#pragma unroll
        for (int j = p + 1; j < 2 * NB; ++j) Aw[j] = sel(mine, Aw[j], fnma(Aw[j], piv, pr[j]));
      }
      if (i == 0) break;
      // ---- T_i = Aw[NB ..]: to the team ----
#pragma unroll
      for (int j = 0; j < NB; ++j) tmat[team][r0][j] = Aw[NB + j];
      // ---- row i-1 ----
      cR = cC, phR = phC, wR = wC, gR = gC;
      cC = cL, phC = phL, wC = wL, gC = gL;
      cL = cLL, phL = phLL, wL = wLL, gL = gLL;
      eR = eL;
      if (i >= 2) eL = edge(i - 2, cL, cC, phL, phC, wL, wC);
      else eL = {0.0, 0.0, 0.0};   // the wall row has no left edge
      double Mr[NB], Lr[NB];
      assemble(i - 1, Mr, Lr);
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
      for (int j = 0; j < NB; ++j) Aw[j] = Mr[j], Aw[NB + j] = Lr[j];
      // the point the row after next needs on its left (its ring slot held point i, which no row needs any more)
      if (i >= 3) {
        cLL = nxt;
        point(i - 3, cLL, phLL, wLL, gLL);
      }
    }

    // ---- the wall: row r0 of T = W^-1 E is Aw[NB .. NB + N); cC is the lane's own unknown at the wall point ----
    double Tr[N > 0 ? N : 1];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      Tr[j] = Aw[NB + j];
      bad = bad || !finite_(Tr[j]);
    }
    pnp::lds_sync();   // the last elimination step has read its pivot row; T_1 has been read
#pragma unroll
    for (int j = 0; j < N; ++j) tmat[team][r0][j] = Tr[j];
    pnp::lds_sync();

    // row k = r0 of [A | -G] (lane N: a zero row that never pivots)
    const int kq = isP ? N - 1 : r0;   // the Poisson lane reads a valid address and drops the value
    const size_t at = (size_t)sy * N + kq;
    const double gk = A.g[at], Kk = A.K[at], Kp = A.Kphi[at];
    double Ar[NB];   // columns 0 .. N-1, then the right-hand side
    double amax = 0.0;
    {
      double kc[N > 0 ? N : 1];
#pragma unroll
      for (int m = 0; m < N; ++m) kc[m] = A.Kc[at * N + m];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < N; ++m) s = fma_(kc[m], tmat[team][m][j], s);
        s = fma_(Kp, tmat[team][N][j], s);
        const double x = A.rf * s;
        const double a = (j == r0 ? 1.0 : 0.0) - x;
        Ar[j] = isP ? 0.0 : a;
        // the scale of the singularity check: the entry and the two terms it is the difference of (where they cancel, the entry
        // itself is rounding noise and measures nothing)
        amax = isP ? amax : fmax(fmax(amax, fabs(a)), fmax(j == r0 ? 1.0 : 0.0, fabs(x)));
      }
      Ar[N] = isP ? 0.0 : -(gk - A.rf * Kk);
    }
    xch[0][base + r0] = amax;
    pnp::lds_sync();
#pragma unroll
    for (int j = 0; j < N; ++j) amax = fmax(amax, xch[0][base + j]);
    pnp::lds_sync();

    // ---- Gauss-Jordan on [A | -G] with partial row pivoting: the pivot lane of column p is the unused lane with the largest entry ----
    bool used = isP, sing = false;
    int mycol = 0;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      double* xb = xch[p & 1];
      xb[base + r0] = used ? -1.0 : (finite_(Ar[p]) ? fabs(Ar[p]) : INFINITY);   // a non-finite entry is chosen, and reported
      pnp::lds_sync();
      double best = -1.0;
      int bi = 0;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const double v = xb[base + j];
        const bool gt = v > best;   // the first of equal candidates
        best = gt ? v : best;
        bi = gt ? j : bi;
      }
      const bool mine = r0 == bi;
      const double piv = Ar[p];
      sing = sing || (mine && (!(piv != 0.0 && finite_(piv)) || fabs(piv) < CATCPL_SINGULAR * amax));
      const double ip = 1.0 / piv;
      double* pr = prow[p & 1][team];
#pragma unroll
      for (int j = p + 1; j < NB; ++j) Ar[j] = sel(mine, Ar[j] * ip, Ar[j]);
      if (mine) {
#pragma unroll
        for (int j = p + 1; j < NB; ++j) pr[j] = Ar[j];
        used = true;
        mycol = p;
      }
      pnp::lds_sync();
#pragma unroll
      for (int j = p + 1; j < NB; ++j) Ar[j] = sel(mine, Ar[j], fnma(Ar[j], piv, pr[j]));
    }
    // the lane that pivoted column p holds dflux_p
    double* xs = xch[N & 1];
    pnp::lds_sync();
    if (!isP) xs[base + mycol] = Ar[N];
    pnp::lds_sync();
    double dstate = 0.0;   // dc_surface of the lane's species; lane N: dphi_surface
#pragma unroll
    for (int j = 0; j < N; ++j) dstate = fma_(Tr[j], xs[base + j], dstate);
    const double dg = xs[base + kq];
    sing = sing || (!isP && !finite_(dg)) || !finite_(dstate);

    // ---- damping ----
    double lc = 1.0;
    if (isP) {
      if (A.dphi_max > 0.0 && fabs(dstate) > A.dphi_max) lc = A.dphi_max / fabs(dstate);
    } else if (cC > 0.0 && dstate < 0.0) {
      lc = fmin(1.0, 0.9 * cC / (-dstate));
    }
    double* xl = xch[(N + 1) & 1];
    xl[base + r0] = lc;
    pnp::lds_sync();
    double lam = 1.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) lam = fmin(lam, xl[base + j]);
    const double fnew = gk + lam * dg;

    // ---- status of the system: any lane of the team ----
    pnp::lds_sync();
    xch[0][base + r0] = bad ? 1.0 : 0.0;
    xch[1][base + r0] = sing ? 1.0 : 0.0;
    pnp::lds_sync();
    double anybad = 0.0, anysing = 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) anybad += xch[0][base + j], anysing += xch[1][base + j];
    if (live) {
      const bool unsolved = A.st[b] != 0 || A.badin[sys] != 0;
      const double nan = __builtin_nan("");
      if (isP) {
        if (A.Tphi) {
#pragma unroll
          for (int j = 0; j < N; ++j) A.Tphi[(size_t)sys * N + j] = unsolved ? nan : Tr[j];
        }
        if (A.lam) A.lam[sys] = unsolved ? nan : lam;
        if (A.dphis) A.dphis[sys] = unsolved ? nan : dstate;
        if (A.status) A.status[sys] = unsolved ? 2 : (anybad != 0.0 ? 1 : (anysing != 0.0 ? 3 : 0));
      } else {
        const size_t o = (size_t)sys * N + r0;
        if (A.Tc) {
#pragma unroll
          for (int j = 0; j < N; ++j) A.Tc[o * N + j] = unsolved ? nan : Tr[j];
        }
        if (A.dflux) A.dflux[o] = unsolved ? nan : dg;
        if (A.fnew) A.fnew[o] = unsolved ? nan : fnew;
        if (A.dcs) A.dcs[o] = unsolved ? nan : dstate;
      }
    }
    pnp::lds_sync();   // the ring and the exchange buffers are free for the next group
  }
}

template <int NB>
static hipError_t launch(const KArgs& a, int64_t blocks, hipStream_t st) {
  hipLaunchKernelGGL((couple_kernel<NB>), dim3((int)blocks), dim3(64), 0, st, a);
  return hipSuccess;
}

template <int NB>
static hipError_t resident(int* per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, couple_kernel<NB>, 64, 0);
}

// the compiled instances: NB = 2 .. 9.  f(ic<NB>)
template <class Fn>
static void dispatch(int NB, Fn&& f) {
  switch (NB) {
    case 2: f(ic<2>()); break;
    case 3: f(ic<3>()); break;
    case 4: f(ic<4>()); break;
    case 5: f(ic<5>()); break;
    case 6: f(ic<6>()); break;
    case 7: f(ic<7>()); break;
    case 8: f(ic<8>()); break;
    default: f(ic<9>()); break;
  }
}

}  // namespace catcpl

static_assert(CATCPL_OK == pnp::post::OK && CATCPL_EINVAL == pnp::post::ERR_INVAL && CATCPL_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATCPL_EDEVICE == pnp::post::ERR_DEVICE && CATCPL_MAX_NX == pnp::post::MAX_NX && CATCPL_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_couple.h and pnp_post.h disagree");

struct catcpl_ctx : pnp::post::Ctx {
  std::vector<double> stage;    // host: the inputs of the call in flight, one copy
  std::vector<int32_t> flags;   // host: status as the kernel wrote it
};

extern "C" {

int catcpl_create(int32_t device, catcpl_ctx** out) { return pnp::post::create("catcpl_create", device, out); }
void catcpl_destroy(catcpl_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catcpl_last_error(const catcpl_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catcpl_last_kernel(const catcpl_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catcpl_last_kernel_ms(const catcpl_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catcpl_solve(catcpl_ctx* ctx, const pnp_device_view* view, const catcpl_params* p, const catcpl_outputs* out) {
  using namespace catcpl;
  static const char entry[] = "catcpl_solve";
  if (const int rc = check_view(ctx, entry, "catcpl_params", view, p, out)) return rc;
  if (out->struct_size != (int32_t)sizeof(catcpl_outputs))
    return fail(ctx, CATCPL_EINVAL, "catcpl_solve: catcpl_outputs.struct_size does not match this library");
  const int N = view->nspecies, nx = view->nx, NB = N + 1;
  const int64_t B = view->batch;
  char msg[256];
  const auto posfin = [](double v) { return v > 0.0 && std::isfinite(v); };
  if (p->max_waves < 0) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: negative max_waves");
  if (!view->status_dev) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: the view has no status row");
  if (!posfin(p->beta) || !posfin(p->eps) || !posfin(p->dx) || !std::isfinite(p->velocity))
    return fail(ctx, CATCPL_EINVAL, "catcpl_solve: beta, eps and dx must be positive and finite, velocity finite");
  if (p->wall_bc != CATCPL_WALL_DIRICHLET && p->wall_bc != CATCPL_WALL_STERN) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: unknown wall_bc");
  if (p->wall_bc == CATCPL_WALL_STERN && !posfin(p->stern_capacitance))
    return fail(ctx, CATCPL_EINVAL, "catcpl_solve: a Stern wall needs a positive, finite capacitance");
  if (!posfin(p->rf)) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: the roughness factor rf must be positive and finite");
  if (!std::isfinite(p->dphi_max)) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: dphi_max must be finite (<= 0: no limit)");
  for (int k = 0; k < N; ++k) {
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    if (!posfin(p->D[k]) || !std::isfinite(p->charges[k]) || !(r >= 0.0) || !std::isfinite(r)) {
      snprintf(msg, sizeof msg, "catcpl_solve: species %d needs D > 0, a finite charge and a radius >= 0 (all finite)", k);
      return fail(ctx, CATCPL_EINVAL, msg);
    }
  }
  const int R = p->nreactions;
  if (R < 0 || R > PNP_MAX_REACTIONS) {
    snprintf(msg, sizeof msg, "catcpl_solve: nreactions = %d outside [0, %d]", R, PNP_MAX_REACTIONS);
    return fail(ctx, CATCPL_EINVAL, msg);
  }
  if (R > 0 && (!p->n_lhs || !p->lhs || !p->n_rhs || !p->rhs || !p->kf || !p->kr))
    return fail(ctx, CATCPL_EINVAL, "catcpl_solve: nreactions > 0 needs n_lhs, lhs, n_rhs, rhs, kf and kr");
  for (int r = 0; r < R; ++r) {
    if (p->n_lhs[r] < 0 || p->n_lhs[r] > PNP_MAX_REACTANTS || p->n_rhs[r] < 0 || p->n_rhs[r] > PNP_MAX_REACTANTS) {
      snprintf(msg, sizeof msg, "catcpl_solve: reaction %d has n_lhs / n_rhs outside [0, %d]", r, PNP_MAX_REACTANTS);
      return fail(ctx, CATCPL_EINVAL, msg);
    }
    for (int side = 0; side < 2; ++side)
      for (int j = 0; j < (side ? p->n_rhs[r] : p->n_lhs[r]); ++j) {
        const int s = (side ? p->rhs : p->lhs)[r * PNP_MAX_REACTANTS + j];
        if (s < 0 || s >= N) {
          snprintf(msg, sizeof msg, "catcpl_solve: reaction %d names species index %d outside [0, %d)", r, s, N);
          return fail(ctx, CATCPL_EINVAL, msg);
        }
      }
  }
  if (p->nlanes < 0) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: nlanes < 0");
  const int64_t n = p->nlanes;
  if (!p->lanes && n > B) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: nlanes above the batch (lanes is NULL)");
  if (p->lanes)
    for (int64_t i = 0; i < n; ++i)
      if (p->lanes[i] < 0 || p->lanes[i] >= B) {
        snprintf(msg, sizeof msg, "catcpl_solve: lane index %lld outside [0, %lld)", (long long)p->lanes[i], (long long)B);
        return fail(ctx, CATCPL_EINVAL, msg);
      }
  if (n > 0 && (!p->flux || !p->K || !p->Kc || !p->Kphi)) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: flux, K, Kc and Kphi are required");
  if (n == 0) return CATCPL_OK;

  KArgs a;
  memset(&a, 0, sizeof a);
  a.nx = nx; a.ldx = view->row_pitch; a.nreact = R; a.stern = p->wall_bc == CATCPL_WALL_STERN;
  a.nsys = n;
  a.c = view->c_dev; a.phi = view->phi_dev; a.st = view->status_dev;
  a.pe = p->dx * p->dx / p->eps;
  a.sternc = a.stern ? p->dx * p->stern_capacitance / p->eps : 0.0;
  a.rf = p->rf;
  a.dphi_max = p->dphi_max;
  for (int k = 0; k < N; ++k) {
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    a.volk[k] = pnp::N_AVOGADRO * r * r * r;
    a.q[k] = p->charges[k];
    a.steric = a.steric || a.volk[k] != 0.0;
  }
  const int TPW = 64 / NB;
  const size_t nn = (size_t)n;

  // the inputs, staged on the host for one copy: edge weights, control volumes, row constants, the kinetic inputs, lanes (int64 in the
  // place of doubles), the flags of non-finite inputs (int32 pairs), the table
  const size_t o_w = 0, o_v = o_w + even((size_t)nx - 1), o_sp = o_v + even(nx), o_g = o_sp + (size_t)(MAXS + 1) * SPF, o_K = o_g + even(nn * N),
               o_Kc = o_K + even(nn * N), o_Kp = o_Kc + even(nn * N * N), o_l = o_Kp + even(nn * N), o_b = o_l + nn, o_t = o_b + even((nn + 1) / 2),
               n_in = o_t + sizeof(Table) / 8;
  try {
    ctx->stage.assign(n_in, 0.0);
    ctx->flags.assign(nn, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATCPL_ENOMEM, "catcpl_solve: out of host memory");
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
  memcpy(sg + o_g, p->flux, nn * N * 8);
  memcpy(sg + o_K, p->K, nn * N * 8);
  memcpy(sg + o_Kc, p->Kc, nn * N * N * 8);
  memcpy(sg + o_Kp, p->Kphi, nn * N * 8);
  {
    int64_t* l = reinterpret_cast<int64_t*>(sg + o_l);
    int32_t* bi = reinterpret_cast<int32_t*>(sg + o_b);
    for (size_t i = 0; i < nn; ++i) {
      l[i] = p->lanes ? p->lanes[i] : (int64_t)i;
      bool fin = true;
      for (int k = 0; k < N; ++k) fin = fin && std::isfinite(p->flux[i * N + k]) && std::isfinite(p->K[i * N + k]) && std::isfinite(p->Kphi[i * N + k]);
      for (int k = 0; k < N * N; ++k) fin = fin && std::isfinite(p->Kc[i * N * N + k]);
      bi[i] = fin ? 0 : 1;
    }
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

  // the rows that were asked for
  const Row rows[] = {{out->T_c, &a.Tc, nn * N * N}, {out->T_phi, &a.Tphi, nn * N}, {out->dflux, &a.dflux, nn * N}, {out->lambda, &a.lam, nn},
                      {out->flux_new, &a.fnew, nn * N}, {out->dc_surface, &a.dcs, nn * N}, {out->dphi_surface, &a.dphis, nn}};
  const size_t need_out = rows_doubles(rows), n_flags = even((nn + 1) / 2);
  if (!need_out && !out->status) return CATCPL_OK;

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  // persistent grid: as many waves as the device holds at once unless the caller sizes it, no more than there are groups of systems
  const int64_t groups = ((int64_t)n + TPW - 1) / TPW;
  int64_t blocks = p->max_waves;
  if (blocks == 0) {
    int cus = 0, per_cu = 0;
    PNP_POST_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    hipError_t oe = hipSuccess;
    dispatch(NB, [&](auto nb) { oe = resident<decltype(nb)::value>(&per_cu); });
    PNP_POST_HIP(oe);
    blocks = (int64_t)std::max(per_cu, 1) * std::max(cus, 1);
  }
  blocks = std::min(std::max<int64_t>(blocks, 1), groups);
  if (const int rc = reserve(ctx, entry, n_in + need_out + n_flags)) return rc;
  a.wgt = ctx->buf + o_w;
  a.vol = ctx->buf + o_v;
  a.sp = ctx->buf + o_sp;
  a.g = ctx->buf + o_g;
  a.K = ctx->buf + o_K;
  a.Kc = ctx->buf + o_Kc;
  a.Kphi = ctx->buf + o_Kp;
  a.lanes = reinterpret_cast<const int64_t*>(ctx->buf + o_l);
  a.badin = reinterpret_cast<const int32_t*>(ctx->buf + o_b);
  a.tab = reinterpret_cast<const Table*>(ctx->buf + o_t);
  double* cur = place_rows(rows, ctx->buf + n_in);
  a.status = reinterpret_cast<int32_t*>(cur);
  PNP_POST_HIP(hipMemcpyAsync(ctx->buf, sg, n_in * sizeof(double), hipMemcpyHostToDevice, st));
  if (!ctx->ev0) PNP_POST_HIP(hipEventCreate(&ctx->ev0));
  if (!ctx->ev1) PNP_POST_HIP(hipEventCreate(&ctx->ev1));
  ctx->kernel_ms = -1.0f;
  PNP_POST_HIP(hipEventRecord(ctx->ev0, st));
  hipError_t le = hipSuccess;
  dispatch(NB, [&](auto nb) { le = launch<decltype(nb)::value>(a, blocks, st); });
  PNP_POST_HIP(le);
  PNP_POST_HIP(hipGetLastError());
  PNP_POST_HIP(hipEventRecord(ctx->ev1, st));
  for (const Row& r : rows)
    if (r.wanted()) PNP_POST_HIP(hipMemcpyAsync(r.host, *r.dev, r.n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (out->status) PNP_POST_HIP(hipMemcpyAsync(ctx->flags.data(), a.status, nn * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PNP_POST_HIP(hipStreamSynchronize(st));
  PNP_POST_HIP(hipEventElapsedTime(&ctx->kernel_ms, ctx->ev0, ctx->ev1));
  if (out->status) memcpy(out->status, ctx->flags.data(), nn * sizeof(int32_t));
  snprintf(msg, sizeof msg, "catcpl::couple_kernel<%d>", NB);
  ctx->last_kernel = msg;
  return CATCPL_OK;
}

}  // extern "C"
