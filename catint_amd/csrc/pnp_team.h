// What the libraries that eliminate the stationary Jacobian of the physical mode with a TEAM of lanes per system have in common
// (response/catresp.hip, couple/catcpl.hip, sens/catsens.hip, modes/catmodes.hip, eis/cateis.hip): the rows of the Jacobian, the block
// Thomas walk from the bulk to the wall, the reaction and wall tables, and the host code around a launch.  Each library is one
// translation unit and compiles its own copy: nothing here is exported.  The frame of an entry point (context, check_view, staged
// inputs, rows, reserve, the tail) is that of pnp_post.h and pnp_stage.h.  gfx950 / MI355X only.
//
// Mapping: a team of NB = N + 1 adjacent lanes per system; lane r owns row r of the working block row [D' | L] (2 NB numbers, real or
// complex) in registers.  64 / NB teams per wave, one wave per workgroup, no workgroup barrier.  The lanes beyond the last full team form
// a partial team with an LDS area of its own: every LDS array of a kernel has 64 / NB + 1 team areas, declared in the kernel and passed
// in by reference.
// Walk: row nx-1 is the identity (T = 0); for i = nx-2 .. 1 Gauss-Jordan without row exchanges on [D'_i | L_i] across the team leaves
// T_i = D'_i^-1 L_i, then D'_{i-1} = M_{i-1} - U_{i-1} T_i (`next_row`); what is eliminated at the wall row is the kernel's own.  Lane r
// reads row r of the operating point (c_r, or phi for r = N) one point per block row, two block rows ahead of its use (`Window`), so
// the load hides behind the O(NB^3) algebra of a block row.
// The Gauss-Jordan step itself, with its pivot monitor, is NOT here: it stands in the row loop of each kernel, in the same words.  As a
// function (by reference, by value, one call per pivot, inlined early or late) it computes the same bits, but the compiler turns the
// short-circuit branches of the monitor into selects and schedules the longer blocks differently: the complex instances of block size
// 7 to 9 ran 5 to 12 % slower on the MI355X (profiles/team_header.md).
// Code generation: every function here is inlined into the one row loop of its kernel, register state comes in as references to
// scalars, small structs of scalars and fixed arrays (all scalar-replaced: no instance has scratch), every loop over NB, 2 NB and MAXT is
// unrolled, and every update is a `sel` of two computed values -- written as `mine ? a : b` with the arithmetic inside the branch is
// correct as well, but the compiler then branches around the arithmetic of one side: three times the branches in the row loop and
// 1.48 x the time on the point-ion handle.
// Arithmetic order is fixed in the source (no implicit contraction: the pragma below governs every definition of this header whatever
// the including source sets), in the order of oracle/pnp_physical.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "pnp_post.h"

#pragma clang fp contract(off)

namespace pnp {
namespace team {

using namespace pnp::post;

constexpr int MAXS = MAX_SPECIES, MAXR = PNP_MAX_REACTIONS, MAXT = PNP_MAX_REACTANTS;
constexpr int WALL_DIRICHLET = 0, WALL_STERN = 1;   // the CATRESP_WALL_* / CATCPL_WALL_* values
constexpr double PIVOT_GROWTH_LIMIT = 1e8;          // CATRESP_PIVOT_GROWTH_LIMIT, CATCPL_PIVOT_GROWTH_LIMIT
constexpr double GROWTH2 = PIVOT_GROWTH_LIMIT * PIVOT_GROWTH_LIMIT;
constexpr int SPF = 8;   // per-row constants: D, q beta, dx^2 / D, velocity dx, dx (row N: 1, 0, 0, 0, 0)

// the reaction table of one call, flattened on the host (every index validated there)
struct ReactionTable {
  int32_t n_side[2][MAXR];          // entries of the left / right side
  int32_t side[2][MAXR][MAXT];
  double kk[2][MAXR];               // kf, kr
  double net[MAXR][MAXS + 1];       // n_rhs(k, r) - n_lhs(k, r); column N: 0
};
static_assert(sizeof(ReactionTable) % 8 == 0, "the table is copied as doubles");

// ... and the wall table behind it, in the libraries that take one
struct WallTable : ReactionTable {
  int32_t wspecies[PNP_MAX_WALL_REACTIONS], pad_[PNP_MAX_WALL_REACTIONS];
  double nu[PNP_MAX_WALL_REACTIONS][MAXS + 1];   // column N: 0
  double alpha[PNP_MAX_WALL_REACTIONS], sat[PNP_MAX_WALL_REACTIONS];
};
static_assert(sizeof(WallTable) % 8 == 0, "the table is copied as doubles");

// The constants of the medium, member `k` of a kernel's arguments.  The shared functions read these further members of the arguments
// (type KA) by name, so each kernel keeps the layout of its own: int32 nx, nreact, stern, steric; const double *wgt, *vol ([nx-1]
// dx / h_e, [nx] v_i) and *sp ([NB][SPF]).
struct Consts {
  double volk[MAXS], q[MAXS];   // N_A a_k^3, q_k
  double pe, sternc;            // dx^2 / eps, dx C_S / eps
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
// both operands are evaluated before the choice: a select, never a branch around the arithmetic of one side
__device__ __forceinline__ double sel(bool c, double a, double b) { return c ? a : b; }
__device__ __forceinline__ cplx sel(bool c, cplx a, cplx b) { return cplx{c ? a.re : b.re, c ? a.im : b.im}; }
// i w a
__device__ __forceinline__ double times_iw(double, double) { return 0.0; }
__device__ __forceinline__ cplx times_iw(double w, cplx a) { return cplx{-w * a.im, w * a.re}; }

// ---- device: the rows of the Jacobian ----------------------------------------------------------------------------------------------
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

// a grid point as a lane holds it: its own unknown, and phi and the steric terms of the point
struct Point {
  double c, ph, w, gf;   // gf: the free volume fraction, g_j = vol_j / gf, gamma = 1 / gf
};

// points in registers: R, C, L = i+1, i, i-1 of the block row i in work, LL = i-2 (entered one block row ahead); the edges C-R and L-C
struct Window {
  Point R, C, L, LL;
  Edge eR, eL;
};

// a lane's place in its team (team 64 / NB: the partial team of the lanes left over) and the constants of its row
struct Lane {
  int team, r0, base;
  bool isP;   // row N: the Poisson row
  double Dk, qb, rs, vdx, dx;   // dx: 0 on row N
};

template <int NB>
__device__ __forceinline__ Lane lane_of(const double* sp) {
  Lane ln;
  const int lane = threadIdx.x;
  ln.team = lane / NB, ln.r0 = lane - ln.team * NB, ln.base = ln.team * NB;
  ln.isP = ln.r0 == NB - 1;
  ln.Dk = sp[ln.r0 * SPF], ln.qb = sp[ln.r0 * SPF + 1], ln.rs = sp[ln.r0 * SPF + 2], ln.vdx = sp[ln.r0 * SPF + 3];
  ln.dx = sp[ln.r0 * SPF + 4];
  return ln;
}

template <int NB>
using Ring = double[3][(64 / NB + 1) * NB];   // the unknowns of the last three grid points, one column per lane

// grid point i enters: the lane's own unknown p.c goes to the ring, phi and the steric terms of the point come back
template <int NB, class KA>
__device__ __forceinline__ void enter(const KA& A, Ring<NB>& ring, const Lane& ln, int i, Point& p) {
  constexpr int N = NB - 1;
  double* slot = ring[i % 3];
  slot[ln.base + ln.r0] = p.c;
  pnp::lds_sync();
  p.ph = slot[ln.base + N];
  p.w = 0.0;
  p.gf = 1.0;
  if (A.steric) {
    double p0 = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) p0 = p0 + A.k.volk[j] * slot[ln.base + j];
    p.w = -log1p(-p0);
    p.gf = 1.0 - p0;
  }
}

// edge e between a left and a right point, for the species of this lane
template <class KA>
__device__ __forceinline__ Edge edge(const KA& A, const Lane& ln, int e, const Point& l, const Point& r) {
  const double wg = A.wgt[e];
  double u = ln.qb * (r.ph - l.ph) + (r.w - l.w);
  if (ln.vdx != 0.0) u = u - ln.vdx / (ln.Dk * wg);
  double B, dB;
  bernoulli2(u, B, dB);
  Edge E;
  E.Bp = wg * B;
  E.Bm = wg * (B + u);
  E.Ju = -wg * ((dB + 1.0) * r.c - dB * l.c);
  return E;
}

// the window of block row nx-2; c4: point nx-4, which first_row enters
template <int NB, class KA>
__device__ __forceinline__ void open(const KA& A, Ring<NB>& ring, const Lane& ln, const double* urow, Window& w, double& c4) {
  const int nx = A.nx;
  w.LL = Point{0.0, 0.0, 0.0, 1.0};
  w.R.c = urow[nx - 1];
  w.C.c = urow[nx - 2];
  w.L.c = urow[nx - 3];
  c4 = nx >= 4 ? urow[nx - 4] : 0.0;
  enter<NB>(A, ring, ln, nx - 1, w.R);
  enter<NB>(A, ring, ln, nx - 2, w.C);
  enter<NB>(A, ring, ln, nx - 3, w.L);
  w.eR = edge(A, ln, nx - 2, w.C, w.R), w.eL = edge(A, ln, nx - 3, w.L, w.C);
}

// Rows r0 of M_i, L_i, U_i from the three points and two edges of the window (centre C = point i).  wallM: the wall table's part of
// M_0 (zeros where there is none: they vanish as a literal + 0.0 does); omega enters the complex rows only.
template <int NB, class T, class KA>
__device__ __forceinline__ void assemble(const KA& A, const ReactionTable& tb, const Ring<NB>& ring, const Lane& ln, const Window& w, int i,
                                         double omega, const double (&wallM)[NB], T (&Mr)[NB], double (&Lr)[NB], double (&Ur)[NB]) {
  constexpr int N = NB - 1;
  constexpr bool CX = !std::is_same<T, double>::value;
  const int r0 = ln.r0;
  const bool isP = ln.isP;
  const double qb = ln.qb, rs = ln.rs, gR = w.R.gf, gC = w.C.gf, gL = w.L.gf;
  const Edge &eR = w.eR, &eL = w.eL;
  const double vi = A.vol[i];
  double mN = eR.Ju * (-qb) - eL.Ju * qb + wallM[N];
  double dR[N > 0 ? N : 1];
#pragma unroll
  for (int j = 0; j < N; ++j) dR[j] = 0.0;
  if (A.nreact > 0) {
    const double* cc = ring[i % 3] + ln.base;
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
          if (A.steric) d += prod * (double)m * (A.k.volk[j] * (gam * gam)) / gam;   // d gamma^m / d c_j = m gamma^m vol_j gamma
          dR[j] = fma_(sgn, d, dR[j]);
        }
      }
    }
  }
  const double wl = i > 0 ? A.wgt[i - 1] : 0.0, wr = A.wgt[i];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool dg = j == r0;
    // diagonal, wall table, steric coupling, reactions: the oracle's order of accumulation
    double sm = dg ? eR.Bp + eL.Bm : 0.0, su = dg ? -eR.Bm : 0.0, sl = dg ? -eL.Bp : 0.0;
    sm += wallM[j];
    if (A.steric) {
      sm += -eR.Ju * (A.k.volk[j] / gC) - eL.Ju * (A.k.volk[j] / gC);
      su += eR.Ju * (A.k.volk[j] / gR);
      sl += eL.Ju * (A.k.volk[j] / gL);
    }
    sm += -rs * vi * dR[j];
    const double pm = i > 0 ? A.k.pe * vi * A.k.q[j] : 0.0;
    Mr[j] = make<T>(isP ? pm : sm, (CX && dg) ? omega * rs * vi : 0.0);
    Ur[j] = isP ? 0.0 : su;
    Lr[j] = isP ? 0.0 : sl;
  }
  double pmm = -(wr + wl), puu = wr;
  if (i == 0) {
    pmm = A.stern ? -wr - A.k.sternc : 1.0;
    puu = A.stern ? wr : 0.0;
  }
  mN = isP ? pmm : mN;
  Ur[N] = isP ? puu : eR.Ju * qb;
  Lr[N] = isP ? wl : eL.Ju * qb;
  Mr[N] = make<T>(mN, 0.0);
}

// row nx-2: T_{nx-1} = 0, so D' = M.  Point nx-4 enters as LL
template <int NB, class T, class KA>
__device__ __forceinline__ void first_row(const KA& A, const ReactionTable& tb, Ring<NB>& ring, const Lane& ln, Window& w, double c4, double omega,
                                          T (&Aw)[2 * NB], double (&Ur)[NB]) {
  const int nx = A.nx;
  T Mr[NB];
  double Lr[NB], wallM[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) wallM[j] = 0.0;
  assemble<NB, T>(A, tb, ring, ln, w, nx - 2, omega, wallM, Mr, Lr, Ur);
#pragma unroll
  for (int j = 0; j < NB; ++j) Aw[j] = Mr[j], Aw[NB + j] = make<T>(Lr[j], 0.0);
  if (nx >= 4) {
    w.LL.c = c4;
    enter<NB>(A, ring, ln, nx - 4, w.LL);
  }
}

// the window moves to block row i-1
template <class KA>
__device__ __forceinline__ void shift(const KA& A, const Lane& ln, int i, Window& w) {
  w.R = w.C;
  w.C = w.L;
  w.L = w.LL;
  w.eR = w.eL;
  if (i >= 2) w.eL = edge(A, ln, i - 2, w.L, w.C);
  else w.eL = {0.0, 0.0, 0.0};   // the wall row has no left edge
}

// Mr = D'_{i-1} = M_{i-1} - U_{i-1} T_i, row r0; tm: T_i of the team, whose row r0 the lane still holds in Aw[NB ..]
template <int NB, class T>
__device__ __forceinline__ void subtract_UT(bool steric, const Lane& ln, const T (&tm)[NB][NB], const double (&Ur)[NB], const T (&Aw)[2 * NB],
                                            T (&Mr)[NB]) {
  constexpr int N = NB - 1;
  if (steric) {
#pragma unroll
    for (int s = 0; s < NB; ++s) {
#pragma unroll
      for (int j = 0; j < NB; ++j) Mr[j] = fnma(Mr[j], Ur[s], tm[s][j]);
    }
  } else {
    // point ions: U has its diagonal and the phi column
    double ud = 0.0;
#pragma unroll
    for (int s = 0; s < NB; ++s) ud = s == ln.r0 ? Ur[s] : ud;
    const double uN = ln.isP ? 0.0 : Ur[N];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      Mr[j] = fnma(Mr[j], ud, Aw[NB + j]);
      Mr[j] = fnma(Mr[j], uN, tm[N][j]);
    }
  }
}

// Block row i-1 after `shift`: Aw = [D'_{i-1} | L_{i-1}] from the window and T_i (tm: of the team, stored by the caller).  nxt: point
// i-3, which the row after next needs on its left (its ring slot held point i, which no row needs any more)
template <int NB, class T, class KA>
__device__ __forceinline__ void next_row(const KA& A, const ReactionTable& tb, Ring<NB>& ring, const T (&tm)[NB][NB], const Lane& ln, Window& w, int i,
                                         double nxt, double omega, const double (&wallM)[NB], T (&Aw)[2 * NB], double (&Ur)[NB]) {
  T Mr[NB];
  double Lr[NB];
  assemble<NB, T>(A, tb, ring, ln, w, i - 1, omega, wallM, Mr, Lr, Ur);
  pnp::lds_sync();
  subtract_UT<NB, T>(A.steric, ln, tm, Ur, Aw, Mr);
#pragma unroll
  for (int j = 0; j < NB; ++j) Aw[j] = Mr[j], Aw[NB + j] = make<T>(Lr[j], 0.0);
  if (i >= 3) {
    w.LL.c = nxt;
    enter<NB>(A, ring, ln, i - 3, w.LL);
  }
}

// how many lanes of the team raised their flag (1.0 / 0.0 in `row`, one column per lane, stored before the caller's lds_sync)
template <int NB>
__device__ __forceinline__ double team_sum(const double* row, const Lane& ln) {
  double any = 0.0;
#pragma unroll
  for (int j = 0; j < NB; ++j) any += row[ln.base + j];
  return any;
}

// ---- host: the context and the checks of an entry point ----------------------------------------------------------------------------
// (the context is pnp::post::Ctx)
static bool posfin(double v) { return v > 0.0 && std::isfinite(v); }

// The checks come in pieces so that an entry point can keep its own between them; each returns 0 or the code.  Params: catresp_params /
// catcpl_params; entry: the name of the exported function, the head of every message.
template <class Params>
static int check_medium(Ctx* ctx, const char* entry, const pnp_device_view* view, const Params* p) {
  const std::string e(entry);
  if (p->max_waves < 0) return fail(ctx, ERR_INVAL, e + ": negative max_waves");
  if (!view->status_dev) return fail(ctx, ERR_INVAL, e + ": the view has no status row");
  if (!posfin(p->beta) || !posfin(p->eps) || !posfin(p->dx) || !std::isfinite(p->velocity))
    return fail(ctx, ERR_INVAL, e + ": beta, eps and dx must be positive and finite, velocity finite");
  if (p->wall_bc != WALL_DIRICHLET && p->wall_bc != WALL_STERN) return fail(ctx, ERR_INVAL, e + ": unknown wall_bc");
  if (p->wall_bc == WALL_STERN && !posfin(p->stern_capacitance))
    return fail(ctx, ERR_INVAL, e + ": a Stern wall needs a positive, finite capacitance");
  return OK;
}

template <class Params>
static int check_species(Ctx* ctx, const char* entry, const Params* p, int N) {
  char msg[256];
  for (int k = 0; k < N; ++k) {
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    if (!posfin(p->D[k]) || !std::isfinite(p->charges[k]) || !(r >= 0.0) || !std::isfinite(r)) {
      snprintf(msg, sizeof msg, "%s: species %d needs D > 0, a finite charge and a radius >= 0 (all finite)", entry, k);
      return fail(ctx, ERR_INVAL, msg);
    }
  }
  return OK;
}

static int check_nreactions(Ctx* ctx, const char* entry, int R) {
  char msg[256];
  if (R < 0 || R > PNP_MAX_REACTIONS) {
    snprintf(msg, sizeof msg, "%s: nreactions = %d outside [0, %d]", entry, R, PNP_MAX_REACTIONS);
    return fail(ctx, ERR_INVAL, msg);
  }
  return OK;
}

// after check_nreactions
template <class Params>
static int check_reactions(Ctx* ctx, const char* entry, const Params* p, int N) {
  char msg[256];
  const int R = p->nreactions;
  if (R > 0 && (!p->n_lhs || !p->lhs || !p->n_rhs || !p->rhs || !p->kf || !p->kr))
    return fail(ctx, ERR_INVAL, std::string(entry) + ": nreactions > 0 needs n_lhs, lhs, n_rhs, rhs, kf and kr");
  for (int r = 0; r < R; ++r) {
    if (p->n_lhs[r] < 0 || p->n_lhs[r] > PNP_MAX_REACTANTS || p->n_rhs[r] < 0 || p->n_rhs[r] > PNP_MAX_REACTANTS) {
      snprintf(msg, sizeof msg, "%s: reaction %d has n_lhs / n_rhs outside [0, %d]", entry, r, PNP_MAX_REACTANTS);
      return fail(ctx, ERR_INVAL, msg);
    }
    for (int side = 0; side < 2; ++side)
      for (int j = 0; j < (side ? p->n_rhs[r] : p->n_lhs[r]); ++j) {
        const int s = (side ? p->rhs : p->lhs)[r * PNP_MAX_REACTANTS + j];
        if (s < 0 || s >= N) {
          snprintf(msg, sizeof msg, "%s: reaction %d names species index %d outside [0, %d)", entry, r, s, N);
          return fail(ctx, ERR_INVAL, msg);
        }
      }
  }
  return OK;
}

// the wall table: its size (which the libraries check before check_reactions) ...
static int check_nwall(Ctx* ctx, const char* entry, int W) {
  char msg[256];
  if (W < 0 || W > PNP_MAX_WALL_REACTIONS) {
    snprintf(msg, sizeof msg, "%s: n_wall = %d outside [0, %d]", entry, W, PNP_MAX_WALL_REACTIONS);
    return fail(ctx, ERR_INVAL, msg);
  }
  return OK;
}

// ... and its entries (after check_reactions)
template <class Params>
static int check_wall(Ctx* ctx, const char* entry, const Params* p, int N) {
  char msg[256];
  const std::string e(entry);
  const int W = p->n_wall;
  if (W > 0 && !p->k) return fail(ctx, ERR_INVAL, e + ": n_wall > 0 needs the rate constants k");
  if (W > 0 && (!p->wall_species || !p->nu)) return fail(ctx, ERR_INVAL, e + ": n_wall > 0 needs wall_species and nu");
  for (int r = 0; r < W; ++r)
    if (p->wall_species[r] < -1 || p->wall_species[r] >= N) {
      snprintf(msg, sizeof msg, "%s: wall reaction %d names species index %d outside [-1, %d)", entry, r, p->wall_species[r], N);
      return fail(ctx, ERR_INVAL, msg);
    }
  return OK;
}

template <class Params>
static int check_lanes(Ctx* ctx, const char* entry, const Params* p, int64_t B) {
  char msg[256];
  const std::string e(entry);
  if (p->nlanes < 0) return fail(ctx, ERR_INVAL, e + ": nlanes < 0");
  const int64_t n = p->nlanes;
  if (!p->lanes && n > B) return fail(ctx, ERR_INVAL, e + ": nlanes above the batch (lanes is NULL)");
  if (p->lanes)
    for (int64_t i = 0; i < n; ++i)
      if (p->lanes[i] < 0 || p->lanes[i] >= B) {
        snprintf(msg, sizeof msg, "%s: lane index %lld outside [0, %lld)", entry, (long long)p->lanes[i], (long long)B);
        return fail(ctx, ERR_INVAL, msg);
      }
  return OK;
}

// ---- host: the inputs of a call ----------------------------------------------------------------------------------------------------
// the constants of the medium; true when any species has a volume (the steric rows)
template <class Params>
static bool fill_consts(Consts& k, const Params* p, int N, bool stern) {
  bool steric = false;
  k.pe = p->dx * p->dx / p->eps;
  k.sternc = stern ? p->dx * p->stern_capacitance / p->eps : 0.0;
  for (int j = 0; j < N; ++j) {
    const double r = p->mpb_radius ? p->mpb_radius[j] : 0.0;
    k.volk[j] = pnp::N_AVOGADRO * r * r * r;
    k.q[j] = p->charges[j];
    steric = steric || k.volk[j] != 0.0;
  }
  return steric;
}

// The grid as every kernel here reads it, three staged inputs in a row: edge weights dx / h_e -> a.wgt, control volumes v_i -> a.vol,
// row constants -> a.sp.  Returns the first of the three slots for stage_grid.
template <class KA>
static int declare_grid(Inputs& in, KA& a, int nx) {
  const int first = in.add((size_t)nx - 1, &a.wgt);
  in.add((size_t)nx, &a.vol);
  in.add((size_t)(MAXS + 1) * SPF, &a.sp);
  return first;
}

template <class Params>
static void stage_grid(const Inputs& in, std::vector<double>& stage, int first, const Params* p, int nx, int N) {
  double *wgt = in.host(stage, first), *vol = in.host(stage, first + 1), *sp = in.host(stage, first + 2);
  for (int e = 0; e < nx - 1; ++e) wgt[e] = p->dx / (p->x[e + 1] - p->x[e]);
  for (int i = 0; i < nx; ++i) {
    const double hl = i > 0 ? p->x[i] - p->x[i - 1] : 0.0, hr = i < nx - 1 ? p->x[i + 1] - p->x[i] : 0.0;
    vol[i] = 0.5 * (hr + hl) / p->dx;
  }
  for (int k = 0; k <= N; ++k) {
    double* s = sp + k * SPF;
    s[0] = 1.0;
    if (k < N) {
      s[0] = p->D[k];
      s[1] = p->charges[k] * p->beta;
      s[2] = p->dx * p->dx / p->D[k];
      s[3] = p->velocity * p->dx;
      s[4] = p->dx;
    }
  }
}

// the selected operating points (int64 in the place of doubles, one unpadded input: what follows has always started right behind
// them); lanes NULL: the first n
template <class Params>
static void stage_lanes(double* at, const Params* p) {
  int64_t* l = reinterpret_cast<int64_t*>(at);
  for (int64_t i = 0; i < p->nlanes; ++i) l[i] = p->lanes ? p->lanes[i] : i;
}

// into a zeroed table (after check_reactions)
template <class Params>
static void fill_reactions(ReactionTable* tb, const Params* p) {
  for (int r = 0; r < p->nreactions; ++r) {
    tb->n_side[0][r] = p->n_lhs[r];
    tb->n_side[1][r] = p->n_rhs[r];
    tb->kk[0][r] = p->kf[r];
    tb->kk[1][r] = p->kr[r];
    for (int j = 0; j < p->n_lhs[r]; ++j) tb->net[r][tb->side[0][r][j] = p->lhs[r * PNP_MAX_REACTANTS + j]] -= 1.0;
    for (int j = 0; j < p->n_rhs[r]; ++j) tb->net[r][tb->side[1][r][j] = p->rhs[r * PNP_MAX_REACTANTS + j]] += 1.0;
  }
}

// the wall part of a zeroed table (after check_wall)
template <class Params>
static void fill_wall(WallTable* tb, const Params* p, int N) {
  for (int r = 0; r < p->n_wall; ++r) {
    tb->wspecies[r] = p->wall_species[r];
    tb->alpha[r] = p->alpha ? p->alpha[r] : 0.0;
    tb->sat[r] = p->saturation ? p->saturation[r] : 0.0;
    for (int k = 0; k < N; ++k) tb->nu[r][k] = p->nu[r * N + k];
  }
}

// ---- host: the launch --------------------------------------------------------------------------------------------------------------
// the compiled block sizes: NB = 2 .. 9.  What f(ic<NB>) returns
template <class Fn>
static auto dispatch_nb(int NB, Fn&& f) {
  switch (NB) {
    case 2: return f(ic<2>());
    case 3: return f(ic<3>());
    case 4: return f(ic<4>());
    case 5: return f(ic<5>());
    case 6: return f(ic<6>());
    case 7: return f(ic<7>());
    case 8: return f(ic<8>());
    default: return f(ic<9>());
  }
}

// The tail of an entry point whose kernel writes one status row: pnp::post::launch_and_fetch, and the nsys int32 of the row handed to
// the caller (status: the caller's row or NULL; status_dev: the kernel's).
template <size_t NR, class L>
static int run_with_status(Ctx* ctx, const char* entry, hipStream_t st, size_t n_in, const Row (&rows)[NR], int32_t* status,
                           const int32_t* status_dev, size_t nsys, L&& launch) {
  if (const int rc = launch_and_fetch(ctx, entry, st, n_in, rows, Flags{status_dev, nsys, status != nullptr}, &ctx->kernel_ms, launch)) return rc;
  if (status) memcpy(status, ctx->flags.data(), nsys * sizeof(int32_t));
  return OK;
}

}  // namespace team
}  // namespace pnp
