// libcatint_drc (include/catint_drc.h): the degree of rate control of a microkinetic steady state per operating point -- the Jacobian of
// the scaled steady-state rows at the given coverages factorised once, then one right-hand side per rate constant, transition state
// and adsorbate energy.  gfx950 / MI355X only.
//
// Mapping (that of kinetics/catkin.hip): one operating point per lane, one wave per workgroup, persistent waves walking groups of 64
// points.  No lane ever reads what another lane wrote, so there is no barrier and no cross-lane exchange; the only per-lane control is
// the row a lane chooses as its pivot, which is an address, and the branch of Ga, which is a select.
// Working set: everything indexed by a run-time step, column or row number lives in LDS as [slot][lane], the lane fastest (a wave's
// 8-byte accesses are conflict-free): J[T][T] (T = S + 1), y[T], the right-hand side [T], the row scales D[T], N slots that hold the
// activities until the rates are formed and the column's accumulators afterwards, the fluxes [N], the gross rates rf[R], rb[R] --
// formed once per point (two exp per step) and read by every one of the up to 3 R + S columns -- and the T slots of the refinement
// step.  At S = N = 8, R = 16: 165 slots x 512 B = 82.5 KB per wave, sized per call (dynamic LDS, the attribute raised above the
// default).  Registers hold scalars only; the pivot rows are 4-bit fields of one 64-bit register, the branches of Ga 2-bit fields of
// one 32-bit register.
// Tables are the same for every lane and are read at wave-uniform addresses through a read-only pointer: every loop over steps and
// columns has a uniform trip count, and a step outside a column's support is skipped by a uniform test.
// Arithmetic: IEEE divisions and the compiler's exp / log; implicit contraction is off, so a point's numbers do not depend on where
// in the batch it stands.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../../include/catint_drc.h"
#include "../pnp_post.h"

#pragma clang fp contract(off)

namespace catdrc {

using namespace pnp::post;

constexpr int MAXN = CATDRC_MAX_SPECIES, MAXS = CATDRC_MAX_ADSORBATES, MAXT = MAXS + 1, MAXR = CATDRC_MAX_STEPS, MAXM = MAXN + MAXT;
constexpr double MINLOG = CATDRC_MIN_LOG;

// the tables of one call, flattened on the host (everything validated there)
struct Table {
  int32_t of[MAXR][MAXM + 1], ob[MAXR][MAXM + 1];   // columns 0 .. N-1: species, N .. N+S: coverages
  double nu[MAXR][MAXN];
  double cref[MAXN];
  double ns[MAXT + 1];
  double dg[MAXR][4], ea[MAXR][4], lnA[MAXR];
};
static_assert(sizeof(Table) % 8 == 0, "the table is copied as doubles");

struct KArgs {
  int32_t N, S, R, w, use_sigma, from_view, ldx, pad_;
  int64_t n;
  const double* c;         // view: [B][N][ldx]
  const double* phi;       // view: [B][ldx]
  const int32_t* st;       // view: [B] solver status
  const int64_t* lanes;    // [n]
  const double *cs, *phis; // host surface state: [n][N], [n]
  const double *phiM, *sigma, *off, *gamma, *theta;   // [n], [n], [n][R][2], [n][N], [n][T]; null: absent (theta: never)
  double *dkf, *dkb, *dts, *dyts, *xrc, *dG, *xtrc, *flux, *fscale, *resid;   // device rows; null: not wanted
  int32_t* status;
  double sd, rtol, CS, pzc;
};

__device__ __forceinline__ bool finite_(double a) { return fabs(a) < INFINITY; }

// what one lane carries in registers
struct Lane {
  double* L;       // lds + lane: slot s at L[s * 64]
  int oJ, oY, oB, oD, oA, oF, oRf, oRb, oX;   // first slots of J, y / theta, right-hand side, D, activities / accumulators, fluxes, rf, rb, refinement
};

// LU with partial row pivoting in place: rows exchanged whole, multipliers below the diagonal, the pivot row of step k in bits 4k .. 4k+3
__device__ __forceinline__ bool factor(const Lane& ln, int T, uint64_t& pivs) {
  double* J = ln.L + ln.oJ * 64;
  bool bad = false;
  pivs = 0;
  for (int k = 0; k < T; ++k) {
    int p = k;
    double best = fabs(J[(k * T + k) * 64]);
    for (int i = k + 1; i < T; ++i) {
      const double v = fabs(J[(i * T + k) * 64]);
      const bool up = v > best;
      best = up ? v : best;
      p = up ? i : p;
    }
    pivs |= (uint64_t)p << (4 * k);
    for (int c = 0; c < T; ++c) {
      const double a = J[(k * T + c) * 64], b = J[(p * T + c) * 64];
      J[(p * T + c) * 64] = a;
      J[(k * T + c) * 64] = b;
    }
    const double piv = J[(k * T + k) * 64];
    bad = bad || !(piv != 0.0 && finite_(piv));
    for (int i = k + 1; i < T; ++i) {
      const double f = J[(i * T + k) * 64] / piv;
      J[(i * T + k) * 64] = f;
      for (int c = k + 1; c < T; ++c) J[(i * T + c) * 64] = J[(i * T + c) * 64] - f * J[(k * T + c) * 64];
    }
  }
  return bad;
}

// the right-hand side in the T slots from `at` against the stored factors, in place
__device__ __forceinline__ void substitute(const Lane& ln, int at, int T, uint64_t pivs) {
  const double* J = ln.L + ln.oJ * 64;
  double* b = ln.L + at * 64;
  // the rows were exchanged whole, multipliers included: every exchange is applied to the right-hand side before the first elimination
  for (int k = 0; k < T; ++k) {
    const int p = (int)((pivs >> (4 * k)) & 15);
    const double u = b[k * 64], v = b[p * 64];
    b[p * 64] = u;
    b[k * 64] = v;
  }
  for (int k = 0; k < T; ++k) {
    const double v = b[k * 64];
    for (int i = k + 1; i < T; ++i) b[i * 64] = b[i * 64] - J[(i * T + k) * 64] * v;
  }
  for (int k = T - 1; k >= 0; --k) {
    double s = b[k * 64];
    for (int c = k + 1; c < T; ++c) s = s - J[(k * T + c) * 64] * b[c * 64];
    b[k * 64] = s / J[(k * T + k) * 64];
  }
}

// dnet of step r into the column's right-hand side (unscaled) and flux accumulators
__device__ __forceinline__ void add_step(const Table& tb, const Lane& ln, int N, int T, int r, double dnet) {
  double* L = ln.L;
  for (int s = 1; s < T; ++s) {
    const int m = tb.ob[r][N + s] - tb.of[r][N + s];
    if (m) L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + (double)m * dnet;
  }
  for (int k = 0; k < N; ++k) {
    const double nu = tb.nu[r][k];
    if (nu != 0.0) L[(ln.oA + k) * 64] = L[(ln.oA + k) * 64] + nu * dnet;
  }
}

// d(rf_r - rb_r)/dp at fixed y of column q of family fam (0: ln kf_q, 1: ln kb_q, 2: the transition state of step q, 3: the energy of
// adsorbate q + 1); *in: whether step r is in the column's support at all (the same in every lane)
__device__ __forceinline__ double column_dnet(const Table& tb, const Lane& ln, int N, int fam, int q, int r, uint32_t brs, bool* in) {
  const double rf = ln.L[(ln.oRf + r) * 64], rb = ln.L[(ln.oRb + r) * 64];
  if (fam < 3) {
    *in = r == q;
    return fam == 0 ? rf : (fam == 1 ? -rb : rf - rb);
  }
  const int s = q + 1;
  const int ofs = tb.of[r][N + s], ms = tb.ob[r][N + s] - ofs;
  *in = (ms | ofs) != 0;
  const uint32_t br = (brs >> (2 * r)) & 3u;
  const double ddG = -(double)ms, dEa = (double)ofs;
  const double dGa = br == 0 ? dEa : (br == 1 ? ddG : 0.0);
  const double alpha = -dGa, beta = -(dGa - ddG);
  return rf * alpha - rb * beta;
}

// sum_t W[r][t] v_t with v in the T slots from `at`
__device__ __forceinline__ double through_y(const Table& tb, const Lane& ln, int N, int T, int r, int at) {
  const double rf = ln.L[(ln.oRf + r) * 64], rb = ln.L[(ln.oRb + r) * 64];
  double ws = 0.0;
  for (int t = 0; t < T; ++t) {
    const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
    if (of | ob) ws = ws + (rf * (double)of - rb * (double)ob) * ln.L[(at + t) * 64];
  }
  return ws;
}

// The column's right-hand side scaled and solved, then one step of refinement against the rows themselves: the stored J is a sum
// that cancels, the total derivative of a row formed from the rates is not.  dy is left in the B slots; the part of the fluxes that
// goes through dy is added to the accumulators.
__device__ __forceinline__ void close_column(const Table& tb, const Lane& ln, int N, int T, int R, uint64_t pivs, int fam, int q, uint32_t brs) {
  double* L = ln.L;
  for (int s = 1; s < T; ++s) {
    const double D = L[(ln.oD + s) * 64];
    L[(ln.oB + s) * 64] = D == 0.0 ? 0.0 : -(L[(ln.oB + s) * 64] / D);
  }
  substitute(ln, ln.oB, T, pivs);
  double r0 = 0.0;
  for (int t = 0; t < T; ++t) r0 = r0 + L[(ln.oY + t) * 64] * L[(ln.oB + t) * 64];   // the y slots hold n_t theta_t by now
  L[ln.oX * 64] = -r0;
  for (int s = 1; s < T; ++s) L[(ln.oX + s) * 64] = 0.0;
  for (int r = 0; r < R; ++r) {
    bool in;
    const double dnet = column_dnet(tb, ln, N, fam, q, r, brs, &in);
    const double ws = through_y(tb, ln, N, T, r, ln.oB);
    const double tot = in ? dnet + ws : ws;
    for (int s = 1; s < T; ++s) {
      const int m = tb.ob[r][N + s] - tb.of[r][N + s];
      if (m) L[(ln.oX + s) * 64] = L[(ln.oX + s) * 64] + (double)m * tot;
    }
  }
  for (int s = 1; s < T; ++s) {
    const double D = L[(ln.oD + s) * 64];
    L[(ln.oX + s) * 64] = D == 0.0 ? -L[(ln.oB + s) * 64] : -(L[(ln.oX + s) * 64] / D);
  }
  substitute(ln, ln.oX, T, pivs);
  for (int t = 0; t < T; ++t) L[(ln.oB + t) * 64] = L[(ln.oB + t) * 64] + L[(ln.oX + t) * 64];
  for (int r = 0; r < R; ++r) {
    const double ws = through_y(tb, ln, N, T, r, ln.oB);
    for (int k = 0; k < N; ++k) {
      const double nu = tb.nu[r][k];
      if (nu != 0.0) L[(ln.oA + k) * 64] = L[(ln.oA + k) * 64] + nu * ws;
    }
  }
}

__global__ __launch_bounds__(64) void control_kernel(const KArgs A, const Table* __restrict__ tab) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1, R = A.R;
  const Table& tb = *tab;   // its own read-only argument: the uniform reads become scalar loads
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
    // ---- the point's inputs ----
    const double phiM = A.phiM[i];
    const double phi0 = A.from_view ? A.phi[(size_t)b * A.ldx] : A.phis[i];
    bool ok = finite_(phiM) && finite_(phi0);
    if (A.from_view) ok = ok && A.st[b] == 0;
    for (int j = 0; j < N; ++j) {
      const double c = A.from_view ? A.c[((size_t)b * N + j) * A.ldx] : A.cs[i * N + j];
      const double g = A.gamma ? A.gamma[i * N + j] : 1.0;
      ok = ok && finite_(c) && finite_(g);
      L[(ln.oA + j) * 64] = g * (c > 0.0 ? c : 0.0) / tb.cref[j];
    }
    const double V = phiM - (A.w ? phi0 : 0.0);
    const double sg = A.use_sigma ? A.sigma[i] : A.CS * ((phiM - A.pzc) - phi0);
    ok = ok && finite_(sg);
    const double* off = A.off ? A.off + (size_t)i * R * 2 : nullptr;
    if (off)
      for (int r = 0; r < 2 * R; ++r) ok = ok && finite_(off[r]);
    // ---- the state: y = ln theta, clamped as catkin clamps its guess ----
    for (int t = 0; t < T; ++t) {
      const double g = A.theta[i * T + t];
      ok = ok && finite_(g);
      double y = g >= 1.0 ? 0.0 : (g > 0.0 ? log(g) : MINLOG);
      y = y < MINLOG ? MINLOG : y;
      L[(ln.oY + t) * 64] = y;
    }
    // ---- rf, rb once per point; the branch of Ga of step r in bits 2r, 2r+1 (0: Ea, 1: dG, 2: zero) ----
    uint32_t brs = 0;
    for (int r = 0; r < R; ++r) {
      const double s2 = sg * sg;
      const double dG = ((tb.dg[r][0] + tb.dg[r][1] * V) + tb.dg[r][2] * sg) + tb.dg[r][3] * s2;
      const double Ea = ((tb.ea[r][0] + tb.ea[r][1] * V) + tb.ea[r][2] * sg) + tb.ea[r][3] * s2;
      const bool b0 = Ea >= dG && Ea >= 0.0, b1 = dG >= 0.0;
      brs |= (b0 ? 0u : (b1 ? 1u : 2u)) << (2 * r);
      const double Ga = b0 ? Ea : (b1 ? dG : 0.0);
      const double o0 = off ? off[2 * r] : 0.0, o1 = off ? off[2 * r + 1] : 0.0;
      double sf = (tb.lnA[r] - Ga) + o0, sb = (tb.lnA[r] - (Ga - dG)) + o1;
      for (int t = 0; t < T; ++t) {
        const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
        if (of | ob) {
          const double y = L[(ln.oY + t) * 64];
          if (of) sf = sf + (double)of * y;
          if (ob) sb = sb + (double)ob * y;
        }
      }
      double pf = 1.0, pb = 1.0;
      for (int j = 0; j < N; ++j) {
        const int of = tb.of[r][j], ob = tb.ob[r][j];
        if (of | ob) {
          const double a = L[(ln.oA + j) * 64];
          for (int e = 0; e < of; ++e) pf = pf * a;
          for (int e = 0; e < ob; ++e) pb = pb * a;
        }
      }
      L[(ln.oRf + r) * 64] = exp(sf) * pf;
      L[(ln.oRb + r) * 64] = exp(sb) * pb;
    }
    // ---- J (scaled rows), -F and the row scales D at this y; fluxes (the activities' slots now hold flux_scale) ----
    for (int s = 0; s < T * T; ++s) L[(ln.oJ + s) * 64] = 0.0;
    for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0, L[(ln.oD + s) * 64] = 0.0;
    for (int k = 0; k < N; ++k) L[(ln.oF + k) * 64] = 0.0, L[(ln.oA + k) * 64] = 0.0;
    for (int r = 0; r < R; ++r) {
      const double rf = L[(ln.oRf + r) * 64], rb = L[(ln.oRb + r) * 64], net = rf - rb, gross = rf + rb;
      for (int s = 1; s < T; ++s) {
        const int m = tb.ob[r][N + s] - tb.of[r][N + s];
        if (m == 0) continue;
        const double dm = (double)m;
        L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + dm * net;
        L[(ln.oD + s) * 64] = L[(ln.oD + s) * 64] + fabs(dm) * gross;
        for (int t = 0; t < T; ++t) {
          const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
          if (of | ob) {
            double* e = &L[(ln.oJ + s * T + t) * 64];
            *e = *e + dm * (rf * (double)of - rb * (double)ob);
          }
        }
      }
      for (int k = 0; k < N; ++k) {
        const double nu = tb.nu[r][k];
        if (nu != 0.0) {
          L[(ln.oF + k) * 64] = L[(ln.oF + k) * 64] + nu * net;
          L[(ln.oA + k) * 64] = L[(ln.oA + k) * 64] + fabs(nu) * gross;
        }
      }
    }
    double res = 0.0;
    for (int s = 1; s < T; ++s) {
      const double D = L[(ln.oD + s) * 64];
      const bool dead = D == 0.0;
      for (int t = 0; t < T; ++t) {
        double* e = &L[(ln.oJ + s * T + t) * 64];
        *e = dead ? (t == s ? 1.0 : 0.0) : *e / D;
      }
      const double f = dead ? 0.0 : fabs(L[(ln.oB + s) * 64] / D);
      res = f > res || f != f ? f : res;
      if (dead) L[(ln.oY + s) * 64] = MINLOG;
    }
    {
      double f0 = 0.0;
      for (int t = 0; t < T; ++t) {
        const double th = tb.ns[t] * exp(L[(ln.oY + t) * 64]);
        L[(ln.oJ + t) * 64] = th;
        L[(ln.oY + t) * 64] = th;          // y has done its work: the site row stays here for the refinement
        f0 = f0 + th;
      }
      const double f = fabs(f0 - 1.0);
      res = f > res || f != f ? f : res;
    }
    uint64_t pivs = 0;
    const bool bad = factor(ln, T, pivs);
    const int status = !ok ? CATDRC_INPUT : (bad ? CATDRC_PIVOT : (res <= A.rtol ? CATDRC_OK_POINT : CATDRC_RESIDUAL));
    const bool nan = status == CATDRC_INPUT;
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

    // ---- the columns: family 0 d/d ln kf_r, 1 d/d ln kb_r, 2 the transition state of step r, 3 the energy of adsorbate q + 1 ----
    for (int fam = 0; fam < 4; ++fam) {
      const bool wanted = fam == 0 ? A.dkf != nullptr : (fam == 1 ? A.dkb != nullptr : (fam == 2 ? (A.dts || A.dyts || A.xrc) : (A.dG || A.xtrc)));
      if (!wanted) continue;
      const int ncol = fam == 3 ? A.S : R;
      for (int q = 0; q < ncol; ++q) {
        for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0;
        for (int k = 0; k < N; ++k) L[(ln.oA + k) * 64] = 0.0;
        for (int r = fam < 3 ? q : 0; r < (fam < 3 ? q + 1 : R); ++r) {
          bool in;
          const double dnet = column_dnet(tb, ln, N, fam, q, r, brs, &in);
          if (in) add_step(tb, ln, N, T, r, dnet);          // a step outside the column's support contributes nothing
        }
        close_column(tb, ln, N, T, R, pivs, fam, q, brs);
        if (!live) continue;
        if (fam == 2 && A.dyts)
          for (int t = 0; t < T; ++t) A.dyts[((size_t)i * R + q) * T + t] = nan ? bad_number : L[(ln.oB + t) * 64];
        double* raw = fam == 0 ? A.dkf : (fam == 1 ? A.dkb : (fam == 2 ? A.dts : A.dG));
        double* norm = fam == 2 ? A.xrc : (fam == 3 ? A.xtrc : nullptr);
        const size_t at = ((size_t)i * ncol + q) * N;
        for (int k = 0; k < N; ++k) {
          const double v = A.sd * L[(ln.oA + k) * 64];
          if (raw) raw[at + k] = nan ? bad_number : v;
          if (norm) norm[at + k] = nan ? bad_number : ((idle >> k) & 1u ? 0.0 : v / L[(ln.oF + k) * 64]);
        }
      }
    }
  }
}

static size_t lds_bytes(int N, int S, int R) {
  const int T = S + 1;
  return (size_t)(T * T + 4 * T + 2 * N + 2 * R) * 64 * sizeof(double);
}

}  // namespace catdrc

static_assert(CATDRC_OK == pnp::post::OK && CATDRC_EINVAL == pnp::post::ERR_INVAL && CATDRC_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATDRC_EDEVICE == pnp::post::ERR_DEVICE && CATDRC_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_drc.h and pnp_post.h disagree");
static_assert(CATDRC_MAX_ADSORBATES + 1 <= 15, "a pivot row is a 4-bit field");
static_assert(CATDRC_MAX_STEPS <= 16 && CATDRC_MAX_SPECIES <= 32, "a branch is a 2-bit field of 32 bits, an idle species one bit");

struct catdrc_ctx : pnp::post::Ctx {
  std::vector<double> stage;    // host: the inputs of the call in flight, one copy
  std::vector<int32_t> flags;   // host: the status as the kernel wrote it
};

extern "C" {

int catdrc_create(int32_t device, catdrc_ctx** out) { return pnp::post::create("catdrc_create", device, out); }
void catdrc_destroy(catdrc_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catdrc_last_error(const catdrc_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catdrc_last_kernel(const catdrc_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catdrc_last_kernel_ms(const catdrc_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catdrc_solve(catdrc_ctx* ctx, const pnp_device_view* view, const catdrc_params* p, const catdrc_outputs* out) {
  using namespace catdrc;
  static const char entry[] = "catdrc_solve";
  if (!ctx) return CATDRC_EINVAL;
  char msg[256];
  const auto posfin = [](double v) { return v > 0.0 && std::isfinite(v); };
  if (!p || !out) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: null argument");
  if (p->struct_size != (int32_t)sizeof(catdrc_params)) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: catdrc_params.struct_size does not match this library");
  if (out->struct_size != (int32_t)sizeof(catdrc_outputs))
    return fail(ctx, CATDRC_EINVAL, "catdrc_solve: catdrc_outputs.struct_size does not match this library");
  const int N = p->nspecies, S = p->nadsorbates, R = p->nsteps, T = S + 1, M = N + T;
  if (N < 0 || N > CATDRC_MAX_SPECIES) {
    snprintf(msg, sizeof msg, "catdrc_solve: %d species outside [0, %d]", N, CATDRC_MAX_SPECIES);
    return fail(ctx, CATDRC_EINVAL, msg);
  }
  if (S < 1 || S > CATDRC_MAX_ADSORBATES) {
    snprintf(msg, sizeof msg, "catdrc_solve: %d adsorbates outside [1, %d]", S, CATDRC_MAX_ADSORBATES);
    return fail(ctx, CATDRC_EINVAL, msg);
  }
  if (R < 1 || R > CATDRC_MAX_STEPS) {
    snprintf(msg, sizeof msg, "catdrc_solve: %d steps outside [1, %d]", R, CATDRC_MAX_STEPS);
    return fail(ctx, CATDRC_EINVAL, msg);
  }
  if (p->max_waves < 0) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: negative max_waves");
  if (p->potential_drop != CATDRC_DROP_FULL && p->potential_drop != CATDRC_DROP_STERN)
    return fail(ctx, CATDRC_EINVAL, "catdrc_solve: potential_drop is 0 (full) or 1 (Stern)");
  if (!posfin(p->residual_tol)) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: residual_tol must be positive and finite");
  if (!posfin(p->site_density)) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: site_density must be positive and finite");
  if (!p->order_f || !p->order_b || !p->site_count || !p->dG || !p->Ea || !p->lnA || (N > 0 && (!p->nu || !p->cref)))
    return fail(ctx, CATDRC_EINVAL, "catdrc_solve: order_f, order_b, nu, cref, site_count, dG, Ea and lnA are required");
  for (int j = 0; j < N; ++j)
    if (!posfin(p->cref[j])) {
      snprintf(msg, sizeof msg, "catdrc_solve: cref[%d] must be positive and finite", j);
      return fail(ctx, CATDRC_EINVAL, msg);
    }
  for (int t = 0; t < T; ++t) {
    const double v = p->site_count[t];
    if (!(t == 0 ? v == 1.0 : (v == 1.0 || v == 2.0 || v == 3.0))) {
      snprintf(msg, sizeof msg, "catdrc_solve: site count %d must be 1, 2 or 3 (1 for the free site)", t);
      return fail(ctx, CATDRC_EINVAL, msg);
    }
  }
  for (int r = 0; r < R; ++r) {
    double sites = 0.0;
    bool any_f = false, any_b = false, any_nu = false;
    for (int c = 0; c < M; ++c) {
      const int of = p->order_f[r * M + c], ob = p->order_b[r * M + c];
      if (of < 0 || of > CATDRC_MAX_ORDER || ob < 0 || ob > CATDRC_MAX_ORDER) {
        snprintf(msg, sizeof msg, "catdrc_solve: step %d has an order outside [0, %d]", r, CATDRC_MAX_ORDER);
        return fail(ctx, CATDRC_EINVAL, msg);
      }
      any_f = any_f || of;
      any_b = any_b || ob;
      if (c >= N) sites += p->site_count[c - N] * (ob - of);
    }
    if (sites != 0.0) {
      snprintf(msg, sizeof msg, "catdrc_solve: step %d does not conserve sites", r);
      return fail(ctx, CATDRC_EINVAL, msg);
    }
    for (int k = 0; k < N; ++k) {
      if (!std::isfinite(p->nu[r * N + k])) {
        snprintf(msg, sizeof msg, "catdrc_solve: nu of step %d is not finite", r);
        return fail(ctx, CATDRC_EINVAL, msg);
      }
      any_nu = any_nu || p->nu[r * N + k] != 0.0;
    }
    if ((!any_f || !any_b) && !any_nu) {
      snprintf(msg, sizeof msg, "catdrc_solve: step %d is an empty step (no orders on a side and no stoichiometry)", r);
      return fail(ctx, CATDRC_EINVAL, msg);
    }
    bool fin = std::isfinite(p->lnA[r]);
    for (int q = 0; q < 4; ++q) {
      fin = fin && std::isfinite(p->dG[r * 4 + q]);
      const double e = p->Ea[r * 4 + q];
      fin = fin && (std::isfinite(e) || (q == 0 && e == -INFINITY));
    }
    if (!fin) {
      snprintf(msg, sizeof msg, "catdrc_solve: step %d has a non-finite table entry (only e0 may be -INFINITY)", r);
      return fail(ctx, CATDRC_EINVAL, msg);
    }
  }
  if (!p->phiM) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: phiM is required");
  if (!p->theta) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: theta is required (the coverages catkin_solve returned)");
  if (!p->sigma && !(std::isfinite(p->stern_capacitance) && std::isfinite(p->phi_pzc)))
    return fail(ctx, CATDRC_EINVAL, "catdrc_solve: the surface charge needs sigma or a finite stern_capacitance and phi_pzc");
  if (p->n < 0) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: n < 0");
  const int64_t n = p->n;
  if ((p->csurf == nullptr) != (p->phi_surface == nullptr))
    return fail(ctx, CATDRC_EINVAL, "catdrc_solve: csurf and phi_surface come together (or both NULL: the view)");
  const bool from_view = !p->csurf;
  if (from_view) {
    if (!view) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: null view without csurf and phi_surface");
    if (view->struct_size != (int32_t)sizeof(pnp_device_view))
      return fail(ctx, CATDRC_EINVAL, "catdrc_solve: pnp_device_view.struct_size does not match this library");
    if (!view->phi_dev || !view->c_dev)
      return fail(ctx, CATDRC_EINVAL, "catdrc_solve: the view has no potential row (only the physical mode keeps the potential in its state)");
    if (!view->status_dev) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: the view has no status row");
    if (view->nspecies != N) {
      snprintf(msg, sizeof msg, "catdrc_solve: %d species, the view has %d", N, view->nspecies);
      return fail(ctx, CATDRC_EINVAL, msg);
    }
    if (view->batch < 1 || view->nx < 1 || view->row_pitch < view->nx) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: empty batch or a row pitch below nx");
    if (!p->lanes && n > view->batch) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: n above the batch (lanes is NULL)");
    if (p->lanes)
      for (int64_t i = 0; i < n; ++i)
        if (p->lanes[i] < 0 || p->lanes[i] >= view->batch) {
          snprintf(msg, sizeof msg, "catdrc_solve: lane index %lld outside [0, %lld)", (long long)p->lanes[i], (long long)view->batch);
          return fail(ctx, CATDRC_EINVAL, msg);
        }
  } else if (view && view->struct_size != (int32_t)sizeof(pnp_device_view)) {
    return fail(ctx, CATDRC_EINVAL, "catdrc_solve: pnp_device_view.struct_size does not match this library");
  }
  if (n == 0) return CATDRC_OK;

  KArgs a;
  memset(&a, 0, sizeof a);
  a.N = N; a.S = S; a.R = R; a.w = p->potential_drop; a.use_sigma = p->sigma != nullptr;
  a.from_view = from_view; a.n = n;
  a.sd = p->site_density; a.rtol = p->residual_tol; a.CS = p->stern_capacitance; a.pzc = p->phi_pzc;
  if (from_view) {
    a.ldx = view->row_pitch;
    a.c = view->c_dev; a.phi = view->phi_dev; a.st = view->status_dev;
  }

  // the inputs, staged on the host for one copy
  const size_t sn = (size_t)n;
  const size_t o_pm = 0, o_cs = o_pm + even(sn), o_ps = o_cs + (from_view ? 0 : even(sn * N)), o_sg = o_ps + (from_view ? 0 : even(sn)),
               o_off = o_sg + (p->sigma ? even(sn) : 0), o_gm = o_off + (p->off ? sn * R * 2 : 0), o_th = o_gm + (p->gamma ? even(sn * N) : 0),
               o_l = o_th + even(sn * T), o_t = o_l + sn, n_in = o_t + sizeof(Table) / 8;
  try {
    ctx->stage.assign(n_in, 0.0);
    ctx->flags.assign(sn, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATDRC_ENOMEM, "catdrc_solve: out of host memory");
  }
  double* sg = ctx->stage.data();
  memcpy(sg + o_pm, p->phiM, sn * 8);
  if (!from_view) {
    if (N) memcpy(sg + o_cs, p->csurf, sn * N * 8);
    memcpy(sg + o_ps, p->phi_surface, sn * 8);
  }
  if (p->sigma) memcpy(sg + o_sg, p->sigma, sn * 8);
  if (p->off) memcpy(sg + o_off, p->off, sn * R * 2 * 8);
  if (p->gamma && N) memcpy(sg + o_gm, p->gamma, sn * N * 8);
  memcpy(sg + o_th, p->theta, sn * T * 8);
  {
    int64_t* l = reinterpret_cast<int64_t*>(sg + o_l);
    for (int64_t i = 0; i < n; ++i) l[i] = (from_view && p->lanes) ? p->lanes[i] : i;
  }
  Table* tb = reinterpret_cast<Table*>(sg + o_t);
  for (int r = 0; r < R; ++r) {
    for (int c = 0; c < M; ++c) tb->of[r][c] = p->order_f[r * M + c], tb->ob[r][c] = p->order_b[r * M + c];
    for (int k = 0; k < N; ++k) tb->nu[r][k] = p->nu[r * N + k];
    for (int q = 0; q < 4; ++q) tb->dg[r][q] = p->dG[r * 4 + q], tb->ea[r][q] = p->Ea[r * 4 + q];
    tb->lnA[r] = p->lnA[r];
  }
  for (int j = 0; j < N; ++j) tb->cref[j] = p->cref[j];
  for (int t = 0; t < T; ++t) tb->ns[t] = p->site_count[t];

  const Row rows[] = {{out->dflux_dlnkf, &a.dkf, sn * R * N}, {out->dflux_dlnkb, &a.dkb, sn * R * N}, {out->dflux_drc, &a.dts, sn * R * N},
                      {out->dy_drc, &a.dyts, sn * R * T},     {out->drc, &a.xrc, sn * R * N},         {out->dflux_dG, &a.dG, sn * S * N},
                      {out->tdrc, &a.xtrc, sn * S * N},       {out->flux, &a.flux, sn * N},           {out->flux_scale, &a.fscale, sn * N},
                      {out->residual, &a.resid, sn}};
  const size_t need_out = rows_doubles(rows), n_flags = even(sn) / 2;   // the status: n int32
  if (!need_out && !out->status) return CATDRC_OK;

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = from_view ? (hipStream_t)view->stream : (hipStream_t) nullptr;
  const size_t lds = lds_bytes(N, S, R);
  if (lds > 48 * 1024) PNP_POST_HIP(hipFuncSetAttribute((const void*)control_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t groups = (n + 63) / 64;
  int64_t blocks = p->max_waves;
  if (blocks == 0) {
    int cus = 0, per_cu = 0;
    PNP_POST_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    PNP_POST_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, control_kernel, 64, lds));
    blocks = (int64_t)std::max(per_cu, 1) * std::max(cus, 1);
  }
  blocks = std::min(std::max<int64_t>(blocks, 1), groups);
  if (const int rc = reserve(ctx, entry, n_in + need_out + n_flags)) return rc;
  a.phiM = ctx->buf + o_pm;
  if (!from_view) a.cs = ctx->buf + o_cs, a.phis = ctx->buf + o_ps;
  if (p->sigma) a.sigma = ctx->buf + o_sg;
  if (p->off) a.off = ctx->buf + o_off;
  if (p->gamma && N) a.gamma = ctx->buf + o_gm;
  a.theta = ctx->buf + o_th;
  a.lanes = reinterpret_cast<const int64_t*>(ctx->buf + o_l);
  const Table* tab = reinterpret_cast<const Table*>(ctx->buf + o_t);   // a kernel argument of its own (read-only: scalar loads)
  double* cur = place_rows(rows, ctx->buf + n_in);
  a.status = reinterpret_cast<int32_t*>(cur);
  PNP_POST_HIP(hipMemcpyAsync(ctx->buf, sg, n_in * sizeof(double), hipMemcpyHostToDevice, st));
  if (!ctx->ev0) PNP_POST_HIP(hipEventCreate(&ctx->ev0));
  if (!ctx->ev1) PNP_POST_HIP(hipEventCreate(&ctx->ev1));
  ctx->kernel_ms = -1.0f;
  PNP_POST_HIP(hipEventRecord(ctx->ev0, st));
  hipLaunchKernelGGL(control_kernel, dim3((int)blocks), dim3(64), lds, st, a, tab);
  PNP_POST_HIP(hipGetLastError());
  PNP_POST_HIP(hipEventRecord(ctx->ev1, st));
  for (const Row& r : rows)
    if (r.wanted()) PNP_POST_HIP(hipMemcpyAsync(r.host, *r.dev, r.n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (out->status) PNP_POST_HIP(hipMemcpyAsync(ctx->flags.data(), a.status, sn * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PNP_POST_HIP(hipStreamSynchronize(st));
  PNP_POST_HIP(hipEventElapsedTime(&ctx->kernel_ms, ctx->ev0, ctx->ev1));
  if (out->status) memcpy(out->status, ctx->flags.data(), sn * sizeof(int32_t));
  ctx->last_kernel = "catdrc::control_kernel";
  return CATDRC_OK;
}

}  // extern "C"
