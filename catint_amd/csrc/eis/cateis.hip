// libcatint_eis (include/catint_eis.h): the small-signal response of the microkinetic electrode at frequency omega -- the linearised
// surface kinetics with adsorbate storage, the transport transfer functions at the same omega and the Stern layer, closed at the wall.
// Two kernels on one stream, no host round trip between them.  gfx950 / MI355X only.
//
// kinetic_kernel: one (operating point, omega) pair per lane, persistent waves (the mapping of ../pnp_kin.h, whose point_inputs,
// rate_constants, rate_constant_slopes, rate_factors, add_step_rows, scale_row and site_row it calls).  The complex matrix A(omega) --
// at most 9 x 9 x 2 = 162 doubles per lane -- lives in per-lane LDS slots (slot s at L[s * 64], the layout of drc/catdrc.hip) as a real
// and an imaginary plane; it is factorised once with partial row pivoting by |.|^2 and the N + 2 right-hand sides go through one at a
// time: matrix plus all right-hand sides would exceed the 2.5 KB of LDS a lane has.  Slots: 2 T T + 4 T + 3 N, at S = N = 8 222 of
// them, 111 KB per wave.  Registers hold scalars only.  Kc, Kphi (and dy) go to rows of the device buffer that electrode_kernel reads.
//
// electrode_kernel<NB>: a team of NB = N + 1 lanes per (system, omega) (../pnp_team.h with T = cplx: Window, first_row / shift /
// next_row).  The Gauss-Jordan step with its pivot monitor stands in the row loop in the words of response/catresp.hip and
// couple/catcpl.hip, for the reason pnp_team.h gives.  The wall stage is that of couple/catcpl.hip with the phi_M column in the place
// that kernel leaves zero (the working row keeps its width of 2 NB), the pivoted closure is its Gauss-Jordan restated for complex
// numbers.  Nothing is kept between block rows.  Results leave through plain vector stores.  omega = 0 runs the same instance: every
// imaginary part is then a sum of products with a zero factor.
// Arithmetic order is fixed in the source (no implicit contraction).
#include <cstdlib>

#include "../../../include/catint_eis.h"
#include "../pnp_kin.h"
#include "../pnp_team.h"

#pragma clang fp contract(off)

namespace cateis {

using pnp::team::cplx;

// ---- the kinetic kernel ------------------------------------------------------------------------------------------------------------
struct KinArgs {
  int32_t N, S, R, w, use_sigma, from_view, ldx, F;
  int64_t n;               // operating points of the call
  int64_t s0, ns;          // the (point, omega) pairs of this turn: s0 .. s0 + ns - 1
  const double* c;         // view: [B][N][ldx]
  const double* phi;       // view: [B][ldx]
  const int32_t* st;       // view: [B] solver status
  const int64_t* lanes;    // [n]
  const double *cs, *phis; // host surface state: [n][N], [n]
  const double *phiM, *sigma, *off, *gamma, *theta, *omega;   // [n], [n], [n][R][2], [n][N], [n][T], [F]
  double *Kc, *Kphi, *dy, *resid;   // device rows of this turn, indexed by the pair's place in the turn; null: not wanted
  int32_t* kstat;          // [ns]
  double sd, rtol, CS, pzc;
};

// LU of the complex matrix (planes Jr, Ji) with partial row pivoting by |.|^2 in place: rows exchanged whole, multipliers below the
// diagonal, the pivot row of step k in bits 4k .. 4k+3 (the first of equal magnitudes wins).  Returns whether a pivot was zero or not
// finite
__device__ __forceinline__ bool factor(double* Jr, double* Ji, int T, uint64_t& pivs) {
  bool bad = false;
  pivs = 0;
  for (int k = 0; k < T; ++k) {
    int p = k;
    double best = Ji[(k * T + k) * 64] * Ji[(k * T + k) * 64] + Jr[(k * T + k) * 64] * Jr[(k * T + k) * 64];
    for (int i = k + 1; i < T; ++i) {
      const double v = Ji[(i * T + k) * 64] * Ji[(i * T + k) * 64] + Jr[(i * T + k) * 64] * Jr[(i * T + k) * 64];
      const bool up = v > best;
      best = up ? v : best;
      p = up ? i : p;
    }
    pivs |= (uint64_t)p << (4 * k);
    for (int c = 0; c < T; ++c) {
      const double ar = Jr[(k * T + c) * 64], br = Jr[(p * T + c) * 64], ai = Ji[(k * T + c) * 64], bi = Ji[(p * T + c) * 64];
      Jr[(p * T + c) * 64] = ar;
      Jr[(k * T + c) * 64] = br;
      Ji[(p * T + c) * 64] = ai;
      Ji[(k * T + c) * 64] = bi;
    }
    const double pr = Jr[(k * T + k) * 64], pi = Ji[(k * T + k) * 64];
    const double d = pi * pi + pr * pr;
    bad = bad || !(d != 0.0 && pnp::kin::finite_(d));
    const double qr = pr / d, qi = -pi / d;   // 1 / pivot
    for (int i = k + 1; i < T; ++i) {
      const double ar = Jr[(i * T + k) * 64], ai = Ji[(i * T + k) * 64];
      const double fr = ar * qr - ai * qi, fi = ar * qi + ai * qr;
      Jr[(i * T + k) * 64] = fr;
      Ji[(i * T + k) * 64] = fi;
      for (int c = k + 1; c < T; ++c) {
        const double ur = Jr[(k * T + c) * 64], ui = Ji[(k * T + c) * 64];
        Jr[(i * T + c) * 64] = Jr[(i * T + c) * 64] - (fr * ur - fi * ui);
        Ji[(i * T + c) * 64] = Ji[(i * T + c) * 64] - (fr * ui + fi * ur);
      }
    }
  }
  return bad;
}

// the right-hand side (planes br, bi) against the stored factors, in place
__device__ __forceinline__ void substitute(const double* Jr, const double* Ji, double* br, double* bi, int T, uint64_t pivs) {
  for (int k = 0; k < T; ++k) {
    const int p = (int)((pivs >> (4 * k)) & 15);
    const double ur = br[k * 64], vr = br[p * 64], ui = bi[k * 64], vi = bi[p * 64];
    br[p * 64] = ur;
    br[k * 64] = vr;
    bi[p * 64] = ui;
    bi[k * 64] = vi;
  }
  for (int k = 0; k < T; ++k) {
    const double vr = br[k * 64], vi = bi[k * 64];
    for (int i = k + 1; i < T; ++i) {
      const double fr = Jr[(i * T + k) * 64], fi = Ji[(i * T + k) * 64];
      br[i * 64] = br[i * 64] - (fr * vr - fi * vi);
      bi[i * 64] = bi[i * 64] - (fr * vi + fi * vr);
    }
  }
  for (int k = T - 1; k >= 0; --k) {
    double sr = br[k * 64], si = bi[k * 64];
    for (int c = k + 1; c < T; ++c) {
      const double ur = Jr[(k * T + c) * 64], ui = Ji[(k * T + c) * 64], xr = br[c * 64], xi = bi[c * 64];
      sr = sr - (ur * xr - ui * xi);
      si = si - (ur * xi + ui * xr);
    }
    const double pr = Jr[(k * T + k) * 64], pi = Ji[(k * T + k) * 64];
    const double d = pi * pi + pr * pr;
    const double qr = pr / d, qi = -pi / d;
    br[k * 64] = sr * qr - si * qi;
    bi[k * 64] = sr * qi + si * qr;
  }
}

__global__ __launch_bounds__(64) void kinetic_kernel(const KinArgs A, const pnp::kin::Table* __restrict__ tab) {
  using namespace pnp::kin;
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1, R = A.R;
  const Table& tb = *tab;   // its own read-only argument: the uniform reads become scalar loads
  double* L = lds + lane;   // slot s at L[s * 64]
  const int oJr = 0, oJi = T * T, oY = 2 * T * T, oBr = oY + T, oBi = oBr + T, oD = oBi + T, oA = oD + T, oCr = oA + N, oCi = oCr + N;
  const double bad_number = __builtin_nan("");

  for (int64_t grp = blockIdx.x; grp * 64 < A.ns; grp += gridDim.x) {
    const bool live = grp * 64 + lane < A.ns;
    const int64_t q = live ? grp * 64 + lane : A.ns - 1;   // the pair's place in the turn
    const int64_t sys = A.s0 + q;
    const int64_t i = sys / A.F;
    const int f = (int)(sys - i * A.F);
    const int64_t b = A.lanes[i];
    const double omega = A.omega[f];
    const Point pt = point_inputs(A, tb, i, b, L + oA * 64);
    bool ok = pt.ok;
    // ---- the state: y = ln theta, clamped as catkin clamps its guess ----
    for (int t = 0; t < T; ++t) {
      const double g = A.theta[i * T + t];
      ok = ok && finite_(g);
      L[(oY + t) * 64] = log_coverage(g);
    }
    // ---- Jraw, G and the row scales D at this y ----
    for (int s = 0; s < 2 * T * T; ++s) L[(oJr + s) * 64] = 0.0;
    for (int s = 0; s < T; ++s) L[(oBr + s) * 64] = 0.0, L[(oD + s) * 64] = 0.0;
    for (int r = 0; r < R; ++r) {
      double lf, lb, ef, eb, pf, pb;
      int br;
      rate_constants(tb, pt.V, pt.sg, pt.off, r, lf, lb, br);
      rate_factors(tb, N, T, L + oY * 64, L + oA * 64, r, lf, lb, -1, ef, eb, pf, pb);
      add_step_rows(tb, N, T, r, ef * pf, eb * pb, L + oJr * 64, L + oBr * 64, L + oD * 64);
    }
    // ---- A(omega): the scaled rows, the storage term on the diagonal, the site row ----
    double res = 0.0;
    for (int s = 1; s < T; ++s) {
      const double D = L[(oD + s) * 64];
      const bool dead = scale_row(L + oJr * 64, L + oY * 64, T, s, D);
      const double g = dead ? 0.0 : fabs(L[(oBr + s) * 64] / D);
      res = g > res || g != g ? g : res;
      const double th = exp(L[(oY + s) * 64]);
      L[(oJi + s * T + s) * 64] = dead ? 0.0 : -(omega * th) / D;
    }
    site_row(tb, L + oJr * 64, L + oY * 64, T);
    uint64_t pivs = 0;
    const bool bad = factor(L + oJr * 64, L + oJi * 64, T, pivs);
    const int status = !ok ? CATEIS_STATUS_INPUT : (bad ? CATEIS_STATUS_SINGULAR : (res <= A.rtol ? CATEIS_STATUS_OK : CATEIS_STATUS_RESIDUAL));
    const bool nan = status == CATEIS_STATUS_INPUT;
    if (live) {
      A.kstat[q] = status;
      if (A.resid) A.resid[q] = nan ? bad_number : res;
    }

    // ---- one right-hand side after another.  p < N: d/dc_p;  N: d/dphiM at fixed phi_0;  N + 1: d/dphi_0 at fixed phiM ----
    for (int p = 0; p < N + 2; ++p) {
      double dV = 0.0, ds = 0.0, dadc = 0.0;
      if (p == N) dV = 1.0, ds = A.use_sigma ? 0.0 : A.CS;
      else if (p == N + 1) dV = A.w ? -1.0 : 0.0, ds = A.use_sigma ? 0.0 : -A.CS;
      else {
        const double c = A.from_view ? A.c[((size_t)b * N + p) * A.ldx] : A.cs[i * N + p];
        const double g = A.gamma ? A.gamma[i * N + p] : 1.0;
        dadc = c >= 0.0 ? g / tb.cref[p] : 0.0;
      }
      for (int s = 0; s < T; ++s) L[(oBr + s) * 64] = 0.0, L[(oBi + s) * 64] = 0.0;
      for (int k = 0; k < N; ++k) L[(oCr + k) * 64] = 0.0, L[(oCi + k) * 64] = 0.0;
      for (int r = 0; r < R; ++r) {
        double lf, lb, ef, eb, pf, pb, drf, drb;
        int br;
        rate_constants(tb, pt.V, pt.sg, pt.off, r, lf, lb, br);
        if (p < N) {
          const int of = tb.of[r][p], ob = tb.ob[r][p];
          if (of == 0 && ob == 0) continue;
          rate_factors(tb, N, T, L + oY * 64, L + oA * 64, r, lf, lb, p, ef, eb, pf, pb);
          drf = of ? ef * ((double)of * pf * dadc) : 0.0;
          drb = ob ? eb * ((double)ob * pb * dadc) : 0.0;
        } else {
          double dlf, dlb;
          rate_factors(tb, N, T, L + oY * 64, L + oA * 64, r, lf, lb, -1, ef, eb, pf, pb);
          rate_constant_slopes(tb, pt.sg, r, br, dV, ds, dlf, dlb);
          drf = (ef * pf) * dlf;
          drb = (eb * pb) * dlb;
        }
        const double dnet = drf - drb;
        for (int s = 1; s < T; ++s) {
          const int m = tb.ob[r][N + s] - tb.of[r][N + s];
          if (m) L[(oBr + s) * 64] = L[(oBr + s) * 64] + (double)m * dnet;
        }
        for (int k = 0; k < N; ++k) {
          const double nu = tb.nu[r][k];
          if (nu != 0.0) L[(oCr + k) * 64] = L[(oCr + k) * 64] + nu * dnet;
        }
      }
      for (int s = 1; s < T; ++s) {
        const double D = L[(oD + s) * 64];
        L[(oBr + s) * 64] = D == 0.0 ? 0.0 : -(L[(oBr + s) * 64] / D);
      }
      substitute(L + oJr * 64, L + oJi * 64, L + oBr * 64, L + oBi * 64, T, pivs);
      for (int r = 0; r < R; ++r) {
        double lf, lb, ef, eb, pf, pb;
        int br;
        rate_constants(tb, pt.V, pt.sg, pt.off, r, lf, lb, br);
        rate_factors(tb, N, T, L + oY * 64, L + oA * 64, r, lf, lb, -1, ef, eb, pf, pb);
        const double rf = ef * pf, rb = eb * pb;
        double wr = 0.0, wi = 0.0;
        for (int t = 0; t < T; ++t) {
          const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
          if (of | ob) {
            const double wgt = rf * (double)of - rb * (double)ob;
            wr = wr + wgt * L[(oBr + t) * 64];
            wi = wi + wgt * L[(oBi + t) * 64];
          }
        }
        for (int k = 0; k < N; ++k) {
          const double nu = tb.nu[r][k];
          if (nu != 0.0) {
            L[(oCr + k) * 64] = L[(oCr + k) * 64] + nu * wr;
            L[(oCi + k) * 64] = L[(oCi + k) * 64] + nu * wi;
          }
        }
      }
      if (live) {
        for (int k = 0; k < N; ++k) {
          const double vr = nan ? bad_number : A.sd * L[(oCr + k) * 64], vi = nan ? bad_number : A.sd * L[(oCi + k) * 64];
          double* at = p < N ? A.Kc + 2 * (((size_t)q * N + k) * N + p) : A.Kphi + 2 * (((size_t)q * N + k) * 2 + (p - N));
          at[0] = vr;
          at[1] = vi;
        }
        if (A.dy)
          for (int t = 0; t < T; ++t) {
            double* at = A.dy + 2 * (((size_t)q * T + t) * (N + 2) + p);
            at[0] = nan ? bad_number : L[(oBr + t) * 64];
            at[1] = nan ? bad_number : L[(oBi + t) * 64];
          }
      }
    }
  }
}

static size_t kinetic_lds_bytes(int N, int S) {
  const int T = S + 1;
  return (size_t)(2 * T * T + 4 * T + 3 * N) * 64 * sizeof(double);
}

// ---- the electrode kernel ----------------------------------------------------------------------------------------------------------
struct ElArgs {
  int32_t nx, ldx, nreact, stern, steric, F;
  int64_t s0, nsys;        // the (point, omega) pairs of this turn: s0 .. s0 + nsys - 1
  const double* c;         // [B][N][ldx]
  const double* phi;       // [B][ldx]
  const int32_t* st;       // [B] solver status
  const int64_t* lanes;    // [n]
  const double *wgt, *vol; // [nx-1] dx / h_e, [nx] v_i
  const double* sp;        // [NB][SPF]
  const double* omega;     // [F]
  const pnp::team::ReactionTable* tab;
  const double *Kc, *Kphi; // what kinetic_kernel wrote: [nsys][N][N], [nsys][N][2] complex
  const int32_t* kstat;    // [nsys] its status
  double *adm, *far, *ydl, *dflux, *dcs, *dphis, *dsig, *Tc, *Tphi, *tc, *tphi;   // device rows of this turn; null: not wanted
  int32_t* status;
  pnp::team::Consts k;
  double rf, CS;
};

__device__ __forceinline__ void put(double* row, size_t at, cplx v, bool nan) {
  const double bad = __builtin_nan("");
  row[2 * at] = nan ? bad : v.re;
  row[2 * at + 1] = nan ? bad : v.im;
}

template <int NB>
__global__ __launch_bounds__(64) void electrode_kernel(const ElArgs A) {
  using namespace pnp::team;
  using T = cplx;
  constexpr int N = NB - 1, TPW = 64 / NB, RW = (TPW + 1) * NB;
  const Lane ln = lane_of<NB>(A.sp);
  const int team = ln.team, r0 = ln.r0, base = ln.base;
  const bool isP = ln.isP;
  const int nx = A.nx;
  const ReactionTable& tb = *A.tab;

  __shared__ Ring<NB> ring;
  __shared__ T prow[2][TPW + 1][2 * NB];   // the pivot row of an elimination step (two buffers: one wave-level sync per step)
  __shared__ T tmat[TPW + 1][NB][NB];      // T_i; at the wall the transfer functions [T | t]
  __shared__ double xch[2][RW];            // the wall stage: pivot search, flags
  __shared__ T xsol[RW];                   // the wall stage: the solution

  for (int64_t grp = blockIdx.x; grp * TPW < A.nsys; grp += gridDim.x) {
    const int64_t qs = grp * TPW + team;   // the pair's place in the turn
    const bool live = team < TPW && qs < A.nsys;
    const int64_t q = live ? qs : grp * TPW;
    const int64_t sys = A.s0 + q;
    const int64_t li = sys / A.F;
    const int f = (int)(sys - li * A.F);
    const int64_t b = A.lanes[li];
    const double* urow = isP ? A.phi + (size_t)b * A.ldx : A.c + ((size_t)b * N + r0) * A.ldx;
    const double omega = A.omega[f];
    bool bad = false;

    Window w;
    double c4;
    open<NB>(A, ring, ln, urow, w, c4);

    T Aw[2 * NB];     // [D'_i | L_i], row r0; at the wall [W | E | r_phi]
    double Ur[NB];    // U_i, row r0

    first_row<NB, T>(A, tb, ring, ln, w, c4, omega, Aw, Ur);

#pragma unroll 1
    for (int i = nx - 2; i >= 0; --i) {
      const double nxt = i >= 3 ? urow[i - 3] : 0.0;   // the point the row after next needs: used at the end of this block row
      if (i == 0) {
        // the wall: the N columns of E in the place of L, and the phi_M column in the column of the Poisson unknown
        const double e0 = ln.dx / ln.Dk;
#pragma unroll
        for (int j = 0; j < N; ++j) Aw[NB + j] = make<T>((j == r0 && !isP) ? e0 : 0.0, 0.0);
        Aw[NB + N] = make<T>(isP ? -A.k.sternc : 0.0, 0.0);
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
      // ---- T_i = Aw[NB ..]: to the team ----
#pragma unroll
      for (int j = 0; j < NB; ++j) tmat[team][r0][j] = Aw[NB + j];
      // ---- row i-1 ----
      shift(A, ln, i, w);
      double wallM[NB];   // no wall table
#pragma unroll
      for (int j = 0; j < NB; ++j) wallM[j] = 0.0;
      next_row<NB, T>(A, tb, ring, tmat[team], ln, w, i, nxt, omega, wallM, Aw, Ur);
    }

    // ---- the wall: row r0 of [T | t] = W^-1 [E | r_phi] is Aw[NB .. 2 NB) ----
    T Tr[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      Tr[j] = Aw[NB + j];
      bad = bad || !finite_(Tr[j]);
    }
    pnp::lds_sync();   // the last elimination step has read its pivot row; T_1 has been read
#pragma unroll
    for (int j = 0; j < NB; ++j) tmat[team][r0][j] = Tr[j];
    pnp::lds_sync();

    // row k = r0 of [A | b] (lane N: a zero row that never pivots)
    const int kq = isP ? N - 1 : r0;   // the Poisson lane reads a valid address and drops the value
    const size_t at = (size_t)q * N + kq;
    const T KpM = T{A.Kphi[4 * at], A.Kphi[4 * at + 1]}, Kp0 = T{A.Kphi[4 * at + 2], A.Kphi[4 * at + 3]};
    T Ar[NB];   // columns 0 .. N-1, then the right-hand side
    double amax = 0.0;   // squared
    {
      T kc[N > 0 ? N : 1];
#pragma unroll
      for (int m = 0; m < N; ++m) kc[m] = T{A.Kc[2 * (at * N + m)], A.Kc[2 * (at * N + m) + 1]};
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        T s = make<T>(0.0, 0.0);
#pragma unroll
        for (int m = 0; m < N; ++m) s = add(s, mul(kc[m], tmat[team][m][j]));
        s = add(s, mul(Kp0, tmat[team][N][j]));
        if (j < N) {
          const T x = scale(A.rf, s);
          const double d = j == r0 ? 1.0 : 0.0;
          const T a = T{d - x.re, -x.im};
          Ar[j] = isP ? make<T>(0.0, 0.0) : a;
          // the scale of the singularity check: the entry and the two terms it is the difference of
          amax = isP ? amax : fmax(fmax(amax, abs2(a)), fmax(d, abs2(x)));
        } else {
          Ar[N] = isP ? make<T>(0.0, 0.0) : scale(A.rf, add(KpM, s));
        }
      }
    }
    xch[0][base + r0] = amax;
    pnp::lds_sync();
#pragma unroll
    for (int j = 0; j < N; ++j) amax = fmax(amax, xch[0][base + j]);
    pnp::lds_sync();

    // ---- Gauss-Jordan on [A | b] with partial row pivoting: the pivot lane of column p is the unused lane with the largest entry ----
    bool used = isP, sing = false;
    int mycol = 0;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      double* xb = xch[p & 1];
      xb[base + r0] = used ? -1.0 : (finite_(Ar[p]) ? abs2(Ar[p]) : INFINITY);   // a non-finite entry is chosen, and reported
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
      const T piv = Ar[p];
      sing = sing || (mine && (!(nonzero(piv) && finite_(piv)) || abs2(piv) < (CATEIS_SINGULAR * CATEIS_SINGULAR) * amax));
      const T ip = inv(piv);
      T* pr = prow[p & 1][team];
#pragma unroll
      for (int j = p + 1; j < NB; ++j) Ar[j] = sel(mine, mul(Ar[j], ip), Ar[j]);
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
    pnp::lds_sync();
    if (!isP) xsol[base + mycol] = Ar[N];
    pnp::lds_sync();
    T dstate = Tr[N];   // dc_surface of the lane's species; lane N: dphi_surface
    T yf = make<T>(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      dstate = add(dstate, mul(Tr[j], xsol[base + j]));
      yf = add(yf, scale(A.k.q[j], xsol[base + j]));
    }
    const T dg = xsol[base + kq];
    const T dsig = scale(A.CS, T{1.0 - dstate.re, -dstate.im});
    const T ydl = times_iw(omega, dsig);
    const T adm = add(ydl, yf);
    sing = sing || (!isP && !finite_(dg)) || !finite_(dstate) || (isP && !finite_(adm));

    // ---- status of the system: any lane of the team ----
    pnp::lds_sync();
    xch[0][base + r0] = bad ? 1.0 : 0.0;
    xch[1][base + r0] = sing ? 1.0 : 0.0;
    pnp::lds_sync();
    const double anybad = team_sum<NB>(xch[0], ln), anysing = team_sum<NB>(xch[1], ln);
    if (live) {
      const int ks = A.kstat[q];
      const bool unsolved = A.st[b] != 0 || ks == CATEIS_STATUS_INPUT;
      if (isP) {
        if (A.Tphi) {
#pragma unroll
          for (int j = 0; j < N; ++j) put(A.Tphi, (size_t)q * N + j, Tr[j], unsolved);
        }
        if (A.tphi) put(A.tphi, q, Tr[N], unsolved);
        if (A.dphis) put(A.dphis, q, dstate, unsolved);
        if (A.dsig) put(A.dsig, q, dsig, unsolved);
        if (A.far) put(A.far, q, yf, unsolved);
        if (A.ydl) put(A.ydl, q, ydl, unsolved);
        if (A.adm) put(A.adm, q, adm, unsolved);
        A.status[q] = unsolved ? CATEIS_STATUS_INPUT
                               : (anybad != 0.0 ? CATEIS_STATUS_PIVOT
                                                : ((anysing != 0.0 || ks == CATEIS_STATUS_SINGULAR) ? CATEIS_STATUS_SINGULAR : ks));
      } else {
        const size_t o = (size_t)q * N + r0;
        if (A.Tc) {
#pragma unroll
          for (int j = 0; j < N; ++j) put(A.Tc, o * N + j, Tr[j], unsolved);
        }
        if (A.tc) put(A.tc, o, Tr[N], unsolved);
        if (A.dflux) put(A.dflux, o, dg, unsolved);
        if (A.dcs) put(A.dcs, o, dstate, unsolved);
      }
    }
    pnp::lds_sync();   // the ring and the exchange buffers are free for the next group
  }
}

template <int NB>
static hipError_t launch(const ElArgs& a, int64_t blocks, hipStream_t st) {
  hipLaunchKernelGGL((electrode_kernel<NB>), dim3((int)blocks), dim3(64), 0, st, a);
  return hipSuccess;
}

template <int NB>
static hipError_t resident(int* per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, electrode_kernel<NB>, 64, 0);
}

// an output of a call: `per` doubles per (point, omega) pair, copied turn by turn; keep: the row exists on the device whether the caller
// wants it or not (electrode_kernel reads it)
struct Out {
  double* host;
  double** dev;
  size_t per;
  bool keep;
  bool placed() const { return (host || keep) && per; }
};

}  // namespace cateis

static_assert(CATEIS_OK == pnp::post::OK && CATEIS_EINVAL == pnp::post::ERR_INVAL && CATEIS_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATEIS_EDEVICE == pnp::post::ERR_DEVICE && CATEIS_MAX_NX == pnp::post::MAX_NX && CATEIS_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_eis.h and pnp_post.h disagree");
static_assert(CATEIS_WALL_DIRICHLET == pnp::team::WALL_DIRICHLET && CATEIS_WALL_STERN == pnp::team::WALL_STERN &&
                  CATEIS_PIVOT_GROWTH_LIMIT == pnp::team::PIVOT_GROWTH_LIMIT,
              "catint_eis.h and pnp_team.h disagree");
static_assert(CATEIS_MAX_SPECIES == pnp::kin::MAXN && CATEIS_MAX_ADSORBATES == pnp::kin::MAXS && CATEIS_MAX_STEPS == pnp::kin::MAXR &&
                  CATEIS_STATUS_INPUT == pnp::kin::STATUS_INPUT,
              "catint_eis.h and pnp_kin.h disagree");

struct cateis_ctx : pnp::post::Ctx {
  std::vector<double> turn;   // host: the per-pair residuals of a turn
};

namespace cateis {

// what both entry points check of the kinetic half, in catkin_solve's order; then the frequencies
static int check_kinetic(cateis_ctx* ctx, const char* entry, const pnp_device_view* view, const cateis_params* p, const cateis_outputs* out,
                         bool* from_view) {
  using namespace pnp::kin;
  const std::string e(entry);
  char msg[256];
  if (const int rc = check_sizes(ctx, entry, "cateis_params", "cateis_outputs", p, out)) return rc;
  if (const int rc = check_drop(ctx, entry, p)) return rc;
  if (!(p->residual_tol >= 0.0) || !std::isfinite(p->residual_tol)) return fail(ctx, ERR_INVAL, e + ": residual_tol must be >= 0 and finite");
  if (const int rc = check_tables(ctx, entry, p)) return rc;
  if (!p->theta) return fail(ctx, ERR_INVAL, e + ": theta is required (the stationary coverages)");
  if (p->nfreq < 1 || p->nfreq > CATEIS_MAX_FREQ) {
    snprintf(msg, sizeof msg, "%s: nfreq = %d outside [1, %d]", entry, p->nfreq, CATEIS_MAX_FREQ);
    return fail(ctx, ERR_INVAL, msg);
  }
  if (!p->omega) return fail(ctx, ERR_INVAL, e + ": omega is required");
  for (int f = 0; f < p->nfreq; ++f)
    if (!(p->omega[f] >= 0.0) || !std::isfinite(p->omega[f])) {
      snprintf(msg, sizeof msg, "%s: omega[%d] must be >= 0 and finite", entry, f);
      return fail(ctx, ERR_INVAL, msg);
    }
  return check_points(ctx, entry, view, p, from_view);
}

// Both entry points behind their checks.  electrode: cateis_solve
static int run(cateis_ctx* ctx, const char* entry, const pnp_device_view* view, const cateis_params* p, const cateis_outputs* out, bool from_view,
               bool electrode) {
  using namespace pnp::post;
  namespace knh = pnp::kin;
  namespace tmh = pnp::team;
  const int N = p->nspecies, S = p->nadsorbates, Tn = S + 1, F = p->nfreq, NB = N + 1;
  const int nx = electrode ? view->nx : 0;
  const size_t sn = (size_t)p->n, nsys = sn * F;
  KinArgs ka;
  ElArgs ea;
  memset(&ea, 0, sizeof ea);
  knh::set_args(ka, view, p, from_view);
  ka.F = F;
  ka.rtol = p->residual_tol;

  // the outputs, per pair in doubles
  const size_t cN = 2 * (size_t)N;
  const Out outs[] = {{out->Kc, &ka.Kc, cN * N, true},
                      {out->Kphi, &ka.Kphi, cN * 2, true},
                      {out->dy, &ka.dy, 2 * (size_t)Tn * (N + 2), false},
                      {nullptr, &ka.resid, 1, out->residual != nullptr},
                      {electrode ? out->admittance : nullptr, &ea.adm, 2, false},
                      {electrode ? out->faradaic : nullptr, &ea.far, 2, false},
                      {electrode ? out->double_layer : nullptr, &ea.ydl, 2, false},
                      {electrode ? out->dflux : nullptr, &ea.dflux, cN, false},
                      {electrode ? out->dc_surface : nullptr, &ea.dcs, cN, false},
                      {electrode ? out->dphi_surface : nullptr, &ea.dphis, 2, false},
                      {electrode ? out->dsigma : nullptr, &ea.dsig, 2, false},
                      {electrode ? out->Tc : nullptr, &ea.Tc, cN * N, false},
                      {electrode ? out->Tphi : nullptr, &ea.Tphi, cN, false},
                      {electrode ? out->tc : nullptr, &ea.tc, cN, false},
                      {electrode ? out->tphi : nullptr, &ea.tphi, 2, false}};
  bool any = out->status != nullptr || out->residual != nullptr;
  for (const Out& o : outs) any = any || (o.host && o.per);
  if (!any) return OK;

  // ---- the inputs, staged on the host for one copy: those of pnp_kin.h (the coverages, lanes and table included), the frequencies, and
  // ---- for the electrode the grid, the row constants and the reaction table of pnp_team.h
  knh::Stage stage;
  int i_f = 0, i_grid = 0, i_t = 0;
  if (const int rc = knh::stage_inputs(ctx, entry, p, ka, p->theta, &ka.theta, from_view, 0, &stage, [&](Inputs& in) {
        i_f = in.add((size_t)F, &ka.omega);
        if (electrode) i_grid = tmh::declare_grid(in, ea, nx), i_t = in.add_unpadded(sizeof(tmh::ReactionTable) / 8, &ea.tab);
      }))
    return rc;
  const Inputs& in = stage.in;
  const size_t n_in = in.total;
  memcpy(in.host(ctx->stage, i_f), p->omega, (size_t)F * 8);
  if (electrode) {
    tmh::stage_grid(in, ctx->stage, i_grid, p, nx, N);
    tmh::fill_reactions(reinterpret_cast<tmh::ReactionTable*>(in.host(ctx->stage, i_t)), p);
    ea.nx = nx; ea.ldx = view->row_pitch; ea.nreact = p->nreactions; ea.stern = 1; ea.F = F;
    ea.c = view->c_dev; ea.phi = view->phi_dev; ea.st = view->status_dev;
    ea.steric = tmh::fill_consts(ea.k, p, N, true);
    ea.rf = p->rf;
    ea.CS = p->stern_capacitance;
  }

  // ---- turns: as many pairs as the workspace cap admits, at least one wavefront's worth ----
  size_t per_pair = 2;   // the two int32 rows
  for (const Out& o : outs)
    if (o.placed()) per_pair += even(o.per);
  size_t cap = (size_t)2 << 30;
  if (const char* e = getenv("CATEIS_WORKSPACE_BYTES")) {
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end && end != e && *end == 0) cap = (size_t)v;
  }
  const size_t chunk = std::min(nsys, std::max<size_t>(64, cap / 8 / per_pair));
  size_t need_out = 2 * even((chunk + 1) / 2);
  for (const Out& o : outs)
    if (o.placed()) need_out += even(chunk * o.per);
  try {
    ctx->flags.assign(chunk, 0);
    ctx->turn.assign(chunk, 0.0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, ERR_NOMEM, std::string(entry) + ": out of host memory");
  }

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = from_view ? (hipStream_t)view->stream : (hipStream_t) nullptr;
  const size_t lds = kinetic_lds_bytes(N, S);
  if (lds > 48 * 1024) PNP_POST_HIP(hipFuncSetAttribute((const void*)kinetic_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // persistent grids, sized for the longest turn; a shorter last turn launches no more waves than it has groups
  const int TPW = 64 / NB;
  int64_t kin_waves = 0, el_waves = 0;
  if (const int rc = persistent_waves(ctx, entry, p->max_waves, [&](int* per_cu) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kinetic_kernel, 64, lds);
      }, ((int64_t)chunk + 63) / 64, &kin_waves))
    return rc;
  if (electrode)
    if (const int rc = persistent_waves(ctx, entry, p->max_waves, [&](int* per_cu) {
          return tmh::dispatch_nb(NB, [&](auto nb) { return resident<decltype(nb)::value>(per_cu); });
        }, ((int64_t)chunk + TPW - 1) / TPW, &el_waves))
      return rc;
  if (const int rc = reserve(ctx, entry, n_in + need_out)) return rc;
  in.place(ctx->buf);
  double* cur = ctx->buf + n_in;
  for (const Out& o : outs)
    if (o.placed()) {
      *o.dev = cur;
      cur += even(chunk * o.per);
    }
  ka.kstat = reinterpret_cast<int32_t*>(cur);
  cur += even((chunk + 1) / 2);
  if (electrode) {
    ea.lanes = ka.lanes;
    ea.omega = ka.omega;
    ea.Kc = ka.Kc;
    ea.Kphi = ka.Kphi;
    ea.kstat = ka.kstat;
    ea.status = reinterpret_cast<int32_t*>(cur);
  }
  const int32_t* status_dev = electrode ? ea.status : ka.kstat;

  // ---- the turns: the staged inputs go up with the first ----
  float total_ms = 0.0f;
  for (size_t s0 = 0; s0 < nsys; s0 += chunk) {
    const size_t ns = std::min(chunk, nsys - s0);
    ka.s0 = (int64_t)s0;
    ka.ns = (int64_t)ns;
    ea.s0 = (int64_t)s0;
    ea.nsys = (int64_t)ns;
    Row rows[sizeof outs / sizeof outs[0] + 1];
    size_t nr = 0;
    for (const Out& o : outs) rows[nr++] = Row{o.host ? o.host + s0 * o.per : nullptr, o.dev, ns * o.per};
    rows[nr] = Row{out->residual ? ctx->turn.data() : nullptr, &ka.resid, ns};
    float ms = 0.0f;
    if (const int rc = launch_and_fetch(ctx, entry, st, s0 == 0 ? n_in : 0, rows, Flags{status_dev, ns, out->status != nullptr}, &ms, [&] {
          const int64_t kb = std::min<int64_t>(kin_waves, ((int64_t)ns + 63) / 64);
          hipLaunchKernelGGL(kinetic_kernel, dim3((int)kb), dim3(64), lds, st, ka, stage.tab);
          if (!electrode) return hipSuccess;
          const hipError_t ke = hipGetLastError();
          if (ke != hipSuccess) return ke;
          const int64_t eb = std::min<int64_t>(el_waves, ((int64_t)ns + TPW - 1) / TPW);
          return tmh::dispatch_nb(NB, [&](auto nb) { return launch<decltype(nb)::value>(ea, eb, st); });
        }))
      return rc;
    total_ms += ms;
    if (out->status) memcpy(out->status + s0, ctx->flags.data(), ns * sizeof(int32_t));
    if (out->residual)
      for (size_t q = 0; q < ns; ++q)
        if ((s0 + q) % F == 0) out->residual[(s0 + q) / F] = ctx->turn[q];
  }
  ctx->kernel_ms = total_ms;
  if (electrode) {
    char msg[64];
    snprintf(msg, sizeof msg, "cateis::electrode_kernel<%d>", NB);
    ctx->last_kernel = msg;
  } else {
    ctx->last_kernel = "cateis::kinetic_kernel";
  }
  return OK;
}

}  // namespace cateis

extern "C" {

int cateis_create(int32_t device, cateis_ctx** out) { return pnp::post::create("cateis_create", device, out); }
void cateis_destroy(cateis_ctx* ctx) { pnp::post::destroy(ctx); }
const char* cateis_last_error(const cateis_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* cateis_last_kernel(const cateis_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float cateis_last_kernel_ms(const cateis_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int cateis_kinetic(cateis_ctx* ctx, const pnp_device_view* view, const cateis_params* p, const cateis_outputs* out) {
  using namespace cateis;
  static const char entry[] = "cateis_kinetic";
  if (!ctx) return CATEIS_EINVAL;
  bool from_view = false;
  if (const int rc = check_kinetic(ctx, entry, view, p, out, &from_view)) return rc;
  if (p->n == 0) return CATEIS_OK;
  return run(ctx, entry, view, p, out, from_view, false);
}

int cateis_solve(cateis_ctx* ctx, const pnp_device_view* view, const cateis_params* p, const cateis_outputs* out) {
  using namespace cateis;
  namespace tmh = pnp::team;
  static const char entry[] = "cateis_solve";
  if (!ctx) return CATEIS_EINVAL;
  if (const int rc = pnp::post::check_view(ctx, entry, "cateis_params", view, p, out)) return rc;
  if (const int rc = tmh::check_medium(ctx, entry, view, p)) return rc;
  if (p->wall_bc != CATEIS_WALL_STERN) return pnp::post::fail(ctx, CATEIS_EINVAL, "cateis_solve: the electrode needs a Stern wall (wall_bc = CATEIS_WALL_STERN)");
  if (!(p->rf >= 0.0) || !std::isfinite(p->rf)) return pnp::post::fail(ctx, CATEIS_EINVAL, "cateis_solve: the roughness factor rf must be >= 0 and finite");
  if (const int rc = tmh::check_species(ctx, entry, p, view->nspecies)) return rc;
  if (const int rc = tmh::check_nreactions(ctx, entry, p->nreactions)) return rc;
  if (const int rc = tmh::check_reactions(ctx, entry, p, view->nspecies)) return rc;
  if (p->csurf || p->phi_surface) return pnp::post::fail(ctx, CATEIS_EINVAL, "cateis_solve: the surface state is the view's (csurf and phi_surface must be NULL)");
  bool from_view = false;
  if (const int rc = check_kinetic(ctx, entry, view, p, out, &from_view)) return rc;
  if (p->n == 0) return CATEIS_OK;
  return run(ctx, entry, view, p, out, true, true);
}

}  // extern "C"
