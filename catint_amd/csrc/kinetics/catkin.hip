// libcatint_kinetics (include/catint_kinetics.h): the steady state of a mean-field surface microkinetic model per operating point --
// damped Newton in the log-coverages with row-scaled residuals -- and the wall fluxes and their sensitivities that follow from it.
// gfx950 / MI355X only.
//
// Mapping: one operating point per lane, one wave per workgroup, persistent waves walking groups of 64 points.  No lane ever reads what
// another lane wrote, so there is no barrier and no cross-lane exchange; the only divergence is the iteration count (a finished lane
// idles: its unknowns stop changing) and the row a lane chooses as its pivot.
// Working set: everything that is indexed by a run-time step, column or row number lives in LDS as [slot][lane], the lane fastest (a
// wave's 8-byte accesses are conflict-free, and a per-lane row number is only an address): the matrix J[T][T] (T = S + 1), y[T], the
// right-hand side [T], the row scales D[T], the activities a[N] and N accumulators.  At S = 8, N = 8: 124 slots x 512 B = 62 KB per
// wave, sized per call (dynamic LDS).  Registers hold scalars only, so nothing goes to scratch.  The pivot rows of the factorisation
// are kept as 4-bit fields of one 64-bit register.
// Tables (orders, stoichiometry, polynomial coefficients) are the same for every lane and are read at wave-uniform addresses through a
// read-only pointer: every loop over steps and columns has a uniform trip count.
// Arithmetic: IEEE divisions and the compiler's exp / log (pnp_math.h has exp(u) - 1 away from 0 and log(1 + x) on (-1, 0] only);
// implicit contraction is off, so a point's numbers do not depend on where in the batch it stands.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../../include/catint_kinetics.h"
#include "../pnp_post.h"

#pragma clang fp contract(off)

namespace catkin {

using namespace pnp::post;

constexpr int MAXN = CATKIN_MAX_SPECIES, MAXS = CATKIN_MAX_ADSORBATES, MAXT = MAXS + 1, MAXR = CATKIN_MAX_STEPS, MAXM = MAXN + MAXT;
constexpr double MINLOG = CATKIN_MIN_LOG;

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
  int32_t N, S, R, maxit, w, use_sigma, sens, from_view, ldx, pad_;
  int64_t n;
  const double* c;         // view: [B][N][ldx]
  const double* phi;       // view: [B][ldx]
  const int32_t* st;       // view: [B] solver status
  const int64_t* lanes;    // [n]
  const double *cs, *phis; // host surface state: [n][N], [n]
  const double *phiM, *sigma, *off, *gamma, *guess;   // [n], [n], [n][R][2], [n][N], [n][T]; null: absent
  double *theta, *rate, *gross, *flux, *fscale, *dfdc, *dfdphi;   // device rows; null: not wanted
  int32_t *status, *iters;
  double sd, tol, CS, pzc;
};

__device__ __forceinline__ bool finite_(double a) { return fabs(a) < INFINITY; }

// what one lane carries in registers
struct Lane {
  double* L;       // lds + lane: slot s at L[s * 64]
  int oJ, oY, oB, oD, oA, oC;   // first slots of J, y, right-hand side, D, activities, accumulators
  double V, sg;    // potential and charge of the point
  const double* off;   // [R][2] of the point, or null
};

// ln kf, ln kb of step r and the branch of Ga (0: Ea, 1: dG, 2: zero)
__device__ __forceinline__ void rate_constants(const Table& tb, const Lane& ln, int r, double& lf, double& lb, int& br) {
  const double s2 = ln.sg * ln.sg;
  const double dG = ((tb.dg[r][0] + tb.dg[r][1] * ln.V) + tb.dg[r][2] * ln.sg) + tb.dg[r][3] * s2;
  const double Ea = ((tb.ea[r][0] + tb.ea[r][1] * ln.V) + tb.ea[r][2] * ln.sg) + tb.ea[r][3] * s2;
  const bool b0 = Ea >= dG && Ea >= 0.0, b1 = dG >= 0.0;
  br = b0 ? 0 : (b1 ? 1 : 2);
  const double Ga = b0 ? Ea : (b1 ? dG : 0.0);
  const double o0 = ln.off ? ln.off[2 * r] : 0.0, o1 = ln.off ? ln.off[2 * r + 1] : 0.0;
  lf = (tb.lnA[r] - Ga) + o0;
  lb = (tb.lnA[r] - (Ga - dG)) + o1;
}

// d ln kf / dp and d ln kb / dp of step r for dV/dp = dV, dsigma/dp = ds
__device__ __forceinline__ void rate_constant_slopes(const Table& tb, const Lane& ln, int r, int br, double dV, double ds, double& dlf, double& dlb) {
  const double ddG = tb.dg[r][1] * dV + (tb.dg[r][2] + 2.0 * tb.dg[r][3] * ln.sg) * ds;
  const double dEa = tb.ea[r][1] * dV + (tb.ea[r][2] + 2.0 * tb.ea[r][3] * ln.sg) * ds;
  const double dGa = br == 0 ? dEa : (br == 1 ? ddG : 0.0);
  dlf = -dGa;
  dlb = -(dGa - ddG);
}

// the two factors of rf and rb: exp(ln k + sum_t order y_t) and prod_j a_j^order.  skip: a species whose order counts one less (the
// product with one factor left out), -1: none
__device__ __forceinline__ void rate_factors(const KArgs& A, const Table& tb, const Lane& ln, int r, double lf, double lb, int skip, double& ef, double& eb,
                                             double& pf, double& pb) {
  const int N = A.N, T = A.S + 1;
  double sf = lf, sb = lb;
  for (int t = 0; t < T; ++t) {
    const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
    if (of | ob) {
      const double y = ln.L[(ln.oY + t) * 64];
      if (of) sf = sf + (double)of * y;
      if (ob) sb = sb + (double)ob * y;
    }
  }
  pf = 1.0;
  pb = 1.0;
  for (int j = 0; j < N; ++j) {
    const int of = tb.of[r][j] - (j == skip ? 1 : 0), ob = tb.ob[r][j] - (j == skip ? 1 : 0);
    if (of > 0 || ob > 0) {
      const double a = ln.L[(ln.oA + j) * 64];
      for (int e = 0; e < of; ++e) pf = pf * a;
      for (int e = 0; e < ob; ++e) pb = pb * a;
    }
  }
  ef = exp(sf);
  eb = exp(sb);
}

// J (scaled rows), right-hand side -F and the row scales D at the lane's y
__device__ __forceinline__ void assemble(const KArgs& A, const Table& tb, const Lane& ln) {
  const int N = A.N, T = A.S + 1;
  double* L = ln.L;
  for (int s = 0; s < T * T; ++s) L[(ln.oJ + s) * 64] = 0.0;
  for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0, L[(ln.oD + s) * 64] = 0.0;
  for (int r = 0; r < A.R; ++r) {
    double lf, lb, ef, eb, pf, pb;
    int br;
    rate_constants(tb, ln, r, lf, lb, br);
    rate_factors(A, tb, ln, r, lf, lb, -1, ef, eb, pf, pb);
    const double rf = ef * pf, rb = eb * pb, net = rf - rb, gross = rf + rb;
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
  }
  // the scaling of the rows; an adsorbate that nothing produces or consumes is set to CATKIN_MIN_LOG and its row keeps it there
  for (int s = 1; s < T; ++s) {
    const double D = L[(ln.oD + s) * 64];
    const bool dead = D == 0.0;
    for (int t = 0; t < T; ++t) {
      double* e = &L[(ln.oJ + s * T + t) * 64];
      *e = dead ? (t == s ? 1.0 : 0.0) : *e / D;
    }
    const double g = L[(ln.oB + s) * 64];
    L[(ln.oB + s) * 64] = dead ? 0.0 : -(g / D);
    if (dead) L[(ln.oY + s) * 64] = MINLOG;
  }
  // the site row
  double f0 = 0.0;
  for (int t = 0; t < T; ++t) {
    const double th = tb.ns[t] * exp(L[(ln.oY + t) * 64]);
    L[(ln.oJ + t) * 64] = th;
    f0 = f0 + th;
  }
  L[ln.oB * 64] = -(f0 - 1.0);
}

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

// the right-hand side against the stored factors, in place
__device__ __forceinline__ void substitute(const Lane& ln, int T, uint64_t pivs) {
  const double* J = ln.L + ln.oJ * 64;
  double* b = ln.L + ln.oB * 64;
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

__global__ __launch_bounds__(64) void steady_kernel(const KArgs A, const Table* __restrict__ tab) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1, R = A.R;
  const Table& tb = *tab;   // its own read-only argument: the uniform reads become scalar loads
  Lane ln;
  ln.L = lds + lane;
  ln.oJ = 0;
  ln.oY = T * T > N ? T * T : N;
  ln.oB = ln.oY + T;
  ln.oD = ln.oB + T;
  ln.oA = ln.oD + T;
  ln.oC = ln.oA + N;
  double* L = ln.L;
  const double bad_number = __builtin_nan("");

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
    ln.V = phiM - (A.w ? phi0 : 0.0);
    ln.sg = A.use_sigma ? A.sigma[i] : A.CS * ((phiM - A.pzc) - phi0);
    ok = ok && finite_(ln.sg);
    ln.off = A.off ? A.off + (size_t)i * R * 2 : nullptr;
    if (ln.off)
      for (int r = 0; r < 2 * R; ++r) ok = ok && finite_(ln.off[r]);
    // ---- start ----
    double nsum = 0.0;
    for (int t = 0; t < T; ++t) nsum = nsum + tb.ns[t];
    const double y0 = log(1.0 / nsum);
    if (A.guess)
      for (int t = 0; t < T; ++t) ok = ok && finite_(A.guess[i * T + t]);
    for (int t = 0; t < T; ++t) {
      double y = y0;
      if (A.guess && ok) {
        const double g = A.guess[i * T + t];
        y = g >= 1.0 ? 0.0 : (g > 0.0 ? log(g) : MINLOG);
        y = y < MINLOG ? MINLOG : y;
      }
      L[(ln.oY + t) * 64] = y;
    }
    // ---- Newton ----
    int status = ok ? CATKIN_MAXIT : CATKIN_INPUT, it = 0;
    bool active = ok && live;
    uint64_t pivs = 0;
    for (int iter = 0; iter < A.maxit; ++iter) {
      if (__ballot(active) == 0) break;
      assemble(A, tb, ln);
      const bool bad = factor(ln, T, pivs);
      substitute(ln, T, pivs);
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
          status = CATKIN_PIVOT;
          active = false;
        } else {
          ++it;
          if (mx < A.tol) {
            status = CATKIN_CONVERGED;
            active = false;
          }
        }
      }
    }
    const bool nan = status == CATKIN_INPUT;

    // ---- coverages, rates, fluxes at the lane's y (the J slots are free: N of them hold flux_scale) ----
    if (A.theta && live)
      for (int t = 0; t < T; ++t) A.theta[i * T + t] = nan ? bad_number : exp(L[(ln.oY + t) * 64]);
    if (A.rate || A.gross || A.flux || A.fscale) {
      for (int k = 0; k < N; ++k) L[(ln.oC + k) * 64] = 0.0, L[(ln.oJ + k) * 64] = 0.0;
      for (int r = 0; r < R; ++r) {
        double lf, lb, ef, eb, pf, pb;
        int br;
        rate_constants(tb, ln, r, lf, lb, br);
        rate_factors(A, tb, ln, r, lf, lb, -1, ef, eb, pf, pb);
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

    // ---- sensitivities: J at the lane's y factorised once, one right-hand side after another ----
    if (A.sens) {
      assemble(A, tb, ln);
      const bool bad = factor(ln, T, pivs);
      if (bad && status != CATKIN_INPUT) status = CATKIN_PIVOT;
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
          double lf, lb, ef, eb, pf, pb, drf, drb;
          int br;
          rate_constants(tb, ln, r, lf, lb, br);
          if (p < N) {
            const int of = tb.of[r][p], ob = tb.ob[r][p];
            if (of == 0 && ob == 0) continue;
            rate_factors(A, tb, ln, r, lf, lb, p, ef, eb, pf, pb);
            drf = of ? ef * ((double)of * pf * dadc) : 0.0;
            drb = ob ? eb * ((double)ob * pb * dadc) : 0.0;
          } else {
            double dlf, dlb;
            rate_constant_slopes(tb, ln, r, br, dV, ds, dlf, dlb);
            rate_factors(A, tb, ln, r, lf, lb, -1, ef, eb, pf, pb);
            drf = (ef * pf) * dlf;
            drb = (eb * pb) * dlb;
          }
          const double dnet = drf - drb;
          for (int s = 1; s < T; ++s) {
            const int m = tb.ob[r][N + s] - tb.of[r][N + s];
            if (m) L[(ln.oB + s) * 64] = L[(ln.oB + s) * 64] + (double)m * dnet;
          }
          for (int k = 0; k < N; ++k) {
            const double nu = tb.nu[r][k];
            if (nu != 0.0) L[(ln.oC + k) * 64] = L[(ln.oC + k) * 64] + nu * dnet;
          }
        }
        for (int s = 1; s < T; ++s) {
          const double D = L[(ln.oD + s) * 64];
          L[(ln.oB + s) * 64] = D == 0.0 ? 0.0 : -(L[(ln.oB + s) * 64] / D);
        }
        substitute(ln, T, pivs);
        for (int r = 0; r < R; ++r) {
          double lf, lb, ef, eb, pf, pb;
          int br;
          rate_constants(tb, ln, r, lf, lb, br);
          rate_factors(A, tb, ln, r, lf, lb, -1, ef, eb, pf, pb);
          const double rf = ef * pf, rb = eb * pb;
          double ws = 0.0;
          for (int t = 0; t < T; ++t) {
            const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
            if (of | ob) ws = ws + (rf * (double)of - rb * (double)ob) * L[(ln.oB + t) * 64];
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
    }
  }
}

static size_t lds_bytes(int N, int S) {
  const int T = S + 1;
  return (size_t)(std::max(T * T, N) + 3 * T + 2 * N) * 64 * sizeof(double);
}

}  // namespace catkin

static_assert(CATKIN_OK == pnp::post::OK && CATKIN_EINVAL == pnp::post::ERR_INVAL && CATKIN_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATKIN_EDEVICE == pnp::post::ERR_DEVICE && CATKIN_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_kinetics.h and pnp_post.h disagree");
static_assert(CATKIN_MAX_ADSORBATES + 1 <= 15, "a pivot row is a 4-bit field");

struct catkin_ctx : pnp::post::Ctx {
  std::vector<double> stage;    // host: the inputs of the call in flight, one copy
  std::vector<int32_t> flags;   // host: status and iterations as the kernel wrote them
};

extern "C" {

int catkin_create(int32_t device, catkin_ctx** out) { return pnp::post::create("catkin_create", device, out); }
void catkin_destroy(catkin_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catkin_last_error(const catkin_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catkin_last_kernel(const catkin_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catkin_last_kernel_ms(const catkin_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catkin_solve(catkin_ctx* ctx, const pnp_device_view* view, const catkin_params* p, const catkin_outputs* out) {
  using namespace catkin;
  static const char entry[] = "catkin_solve";
  if (!ctx) return CATKIN_EINVAL;
  char msg[256];
  const auto posfin = [](double v) { return v > 0.0 && std::isfinite(v); };
  if (!p || !out) return fail(ctx, CATKIN_EINVAL, "catkin_solve: null argument");
  if (p->struct_size != (int32_t)sizeof(catkin_params)) return fail(ctx, CATKIN_EINVAL, "catkin_solve: catkin_params.struct_size does not match this library");
  if (out->struct_size != (int32_t)sizeof(catkin_outputs))
    return fail(ctx, CATKIN_EINVAL, "catkin_solve: catkin_outputs.struct_size does not match this library");
  const int N = p->nspecies, S = p->nadsorbates, R = p->nsteps, T = S + 1, M = N + T;
  if (N < 0 || N > CATKIN_MAX_SPECIES) {
    snprintf(msg, sizeof msg, "catkin_solve: %d species outside [0, %d]", N, CATKIN_MAX_SPECIES);
    return fail(ctx, CATKIN_EINVAL, msg);
  }
  if (S < 1 || S > CATKIN_MAX_ADSORBATES) {
    snprintf(msg, sizeof msg, "catkin_solve: %d adsorbates outside [1, %d]", S, CATKIN_MAX_ADSORBATES);
    return fail(ctx, CATKIN_EINVAL, msg);
  }
  if (R < 1 || R > CATKIN_MAX_STEPS) {
    snprintf(msg, sizeof msg, "catkin_solve: %d steps outside [1, %d]", R, CATKIN_MAX_STEPS);
    return fail(ctx, CATKIN_EINVAL, msg);
  }
  if (p->max_waves < 0) return fail(ctx, CATKIN_EINVAL, "catkin_solve: negative max_waves");
  if (p->maxit < 1) return fail(ctx, CATKIN_EINVAL, "catkin_solve: maxit < 1");
  if (p->potential_drop != CATKIN_DROP_FULL && p->potential_drop != CATKIN_DROP_STERN)
    return fail(ctx, CATKIN_EINVAL, "catkin_solve: potential_drop is 0 (full) or 1 (Stern)");
  if (!posfin(p->tol)) return fail(ctx, CATKIN_EINVAL, "catkin_solve: tol must be positive and finite");
  if (!posfin(p->site_density)) return fail(ctx, CATKIN_EINVAL, "catkin_solve: site_density must be positive and finite");
  if (!p->order_f || !p->order_b || !p->site_count || !p->dG || !p->Ea || !p->lnA || (N > 0 && (!p->nu || !p->cref)))
    return fail(ctx, CATKIN_EINVAL, "catkin_solve: order_f, order_b, nu, cref, site_count, dG, Ea and lnA are required");
  for (int j = 0; j < N; ++j)
    if (!posfin(p->cref[j])) {
      snprintf(msg, sizeof msg, "catkin_solve: cref[%d] must be positive and finite", j);
      return fail(ctx, CATKIN_EINVAL, msg);
    }
  for (int t = 0; t < T; ++t) {
    const double v = p->site_count[t];
    if (!(t == 0 ? v == 1.0 : (v == 1.0 || v == 2.0 || v == 3.0))) {
      snprintf(msg, sizeof msg, "catkin_solve: site count %d must be 1, 2 or 3 (1 for the free site)", t);
      return fail(ctx, CATKIN_EINVAL, msg);
    }
  }
  for (int r = 0; r < R; ++r) {
    double sites = 0.0;
    bool any_f = false, any_b = false, any_nu = false;
    for (int c = 0; c < M; ++c) {
      const int of = p->order_f[r * M + c], ob = p->order_b[r * M + c];
      if (of < 0 || of > CATKIN_MAX_ORDER || ob < 0 || ob > CATKIN_MAX_ORDER) {
        snprintf(msg, sizeof msg, "catkin_solve: step %d has an order outside [0, %d]", r, CATKIN_MAX_ORDER);
        return fail(ctx, CATKIN_EINVAL, msg);
      }
      any_f = any_f || of;
      any_b = any_b || ob;
      if (c >= N) sites += p->site_count[c - N] * (ob - of);
    }
    if (sites != 0.0) {
      snprintf(msg, sizeof msg, "catkin_solve: step %d does not conserve sites", r);
      return fail(ctx, CATKIN_EINVAL, msg);
    }
    for (int k = 0; k < N; ++k) {
      if (!std::isfinite(p->nu[r * N + k])) {
        snprintf(msg, sizeof msg, "catkin_solve: nu of step %d is not finite", r);
        return fail(ctx, CATKIN_EINVAL, msg);
      }
      any_nu = any_nu || p->nu[r * N + k] != 0.0;
    }
    if ((!any_f || !any_b) && !any_nu) {
      snprintf(msg, sizeof msg, "catkin_solve: step %d is an empty step (no orders on a side and no stoichiometry)", r);
      return fail(ctx, CATKIN_EINVAL, msg);
    }
    bool fin = std::isfinite(p->lnA[r]);
    for (int q = 0; q < 4; ++q) {
      fin = fin && std::isfinite(p->dG[r * 4 + q]);
      const double e = p->Ea[r * 4 + q];
      fin = fin && (std::isfinite(e) || (q == 0 && e == -INFINITY));
    }
    if (!fin) {
      snprintf(msg, sizeof msg, "catkin_solve: step %d has a non-finite table entry (only e0 may be -INFINITY)", r);
      return fail(ctx, CATKIN_EINVAL, msg);
    }
  }
  if (!p->phiM) return fail(ctx, CATKIN_EINVAL, "catkin_solve: phiM is required");
  if (!p->sigma && !(std::isfinite(p->stern_capacitance) && std::isfinite(p->phi_pzc)))
    return fail(ctx, CATKIN_EINVAL, "catkin_solve: the surface charge needs sigma or a finite stern_capacitance and phi_pzc");
  if (p->n < 0) return fail(ctx, CATKIN_EINVAL, "catkin_solve: n < 0");
  const int64_t n = p->n;
  if ((p->csurf == nullptr) != (p->phi_surface == nullptr))
    return fail(ctx, CATKIN_EINVAL, "catkin_solve: csurf and phi_surface come together (or both NULL: the view)");
  const bool from_view = !p->csurf;
  if (from_view) {
    if (!view) return fail(ctx, CATKIN_EINVAL, "catkin_solve: null view without csurf and phi_surface");
    if (view->struct_size != (int32_t)sizeof(pnp_device_view))
      return fail(ctx, CATKIN_EINVAL, "catkin_solve: pnp_device_view.struct_size does not match this library");
    if (!view->phi_dev || !view->c_dev)
      return fail(ctx, CATKIN_EINVAL, "catkin_solve: the view has no potential row (only the physical mode keeps the potential in its state)");
    if (!view->status_dev) return fail(ctx, CATKIN_EINVAL, "catkin_solve: the view has no status row");
    if (view->nspecies != N) {
      snprintf(msg, sizeof msg, "catkin_solve: %d species, the view has %d", N, view->nspecies);
      return fail(ctx, CATKIN_EINVAL, msg);
    }
    if (view->batch < 1 || view->nx < 1 || view->row_pitch < view->nx) return fail(ctx, CATKIN_EINVAL, "catkin_solve: empty batch or a row pitch below nx");
    if (!p->lanes && n > view->batch) return fail(ctx, CATKIN_EINVAL, "catkin_solve: n above the batch (lanes is NULL)");
    if (p->lanes)
      for (int64_t i = 0; i < n; ++i)
        if (p->lanes[i] < 0 || p->lanes[i] >= view->batch) {
          snprintf(msg, sizeof msg, "catkin_solve: lane index %lld outside [0, %lld)", (long long)p->lanes[i], (long long)view->batch);
          return fail(ctx, CATKIN_EINVAL, msg);
        }
  } else if (view && view->struct_size != (int32_t)sizeof(pnp_device_view)) {
    return fail(ctx, CATKIN_EINVAL, "catkin_solve: pnp_device_view.struct_size does not match this library");
  }
  if (n == 0) return CATKIN_OK;

  KArgs a;
  memset(&a, 0, sizeof a);
  a.N = N; a.S = S; a.R = R; a.maxit = p->maxit; a.w = p->potential_drop; a.use_sigma = p->sigma != nullptr;
  a.from_view = from_view; a.n = n;
  a.sd = p->site_density; a.tol = p->tol; a.CS = p->stern_capacitance; a.pzc = p->phi_pzc;
  if (from_view) {
    a.ldx = view->row_pitch;
    a.c = view->c_dev; a.phi = view->phi_dev; a.st = view->status_dev;
  }

  // the inputs, staged on the host for one copy
  const size_t sn = (size_t)n;
  const size_t o_pm = 0, o_cs = o_pm + even(sn), o_ps = o_cs + (from_view ? 0 : even(sn * N)), o_sg = o_ps + (from_view ? 0 : even(sn)),
               o_off = o_sg + (p->sigma ? even(sn) : 0), o_gm = o_off + (p->off ? sn * R * 2 : 0), o_gs = o_gm + (p->gamma ? even(sn * N) : 0),
               o_l = o_gs + (p->theta_guess ? even(sn * T) : 0), o_t = o_l + sn, n_in = o_t + sizeof(Table) / 8;
  try {
    ctx->stage.assign(n_in, 0.0);
    ctx->flags.assign(2 * sn, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATKIN_ENOMEM, "catkin_solve: out of host memory");
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
  if (p->theta_guess) memcpy(sg + o_gs, p->theta_guess, sn * T * 8);
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

  const Row rows[] = {{out->theta, &a.theta, sn * T},       {out->rate, &a.rate, sn * R},           {out->rate_gross, &a.gross, sn * R},
                      {out->flux, &a.flux, sn * N},         {out->flux_scale, &a.fscale, sn * N},   {out->dflux_dc, &a.dfdc, sn * N * N},
                      {out->dflux_dphi, &a.dfdphi, sn * N * 2}};
  a.sens = (out->dflux_dc && N) || (out->dflux_dphi && N);
  const size_t need_out = rows_doubles(rows), n_flags = even(sn);   // status and iterations: 2 n int32
  if (!need_out && !out->status && !out->iterations) return CATKIN_OK;

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = from_view ? (hipStream_t)view->stream : (hipStream_t) nullptr;
  const size_t lds = lds_bytes(N, S);
  const int64_t groups = (n + 63) / 64;
  int64_t blocks = p->max_waves;
  if (blocks == 0) {
    int cus = 0, per_cu = 0;
    PNP_POST_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    PNP_POST_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, steady_kernel, 64, lds));
    blocks = (int64_t)std::max(per_cu, 1) * std::max(cus, 1);
  }
  blocks = std::min(std::max<int64_t>(blocks, 1), groups);
  if (const int rc = reserve(ctx, entry, n_in + need_out + n_flags)) return rc;
  a.phiM = ctx->buf + o_pm;
  if (!from_view) a.cs = ctx->buf + o_cs, a.phis = ctx->buf + o_ps;
  if (p->sigma) a.sigma = ctx->buf + o_sg;
  if (p->off) a.off = ctx->buf + o_off;
  if (p->gamma && N) a.gamma = ctx->buf + o_gm;
  if (p->theta_guess) a.guess = ctx->buf + o_gs;
  a.lanes = reinterpret_cast<const int64_t*>(ctx->buf + o_l);
  const Table* tab = reinterpret_cast<const Table*>(ctx->buf + o_t);   // a kernel argument of its own (read-only: scalar loads)
  double* cur = place_rows(rows, ctx->buf + n_in);
  a.status = reinterpret_cast<int32_t*>(cur);
  a.iters = a.status + sn;
  PNP_POST_HIP(hipMemcpyAsync(ctx->buf, sg, n_in * sizeof(double), hipMemcpyHostToDevice, st));
  if (!ctx->ev0) PNP_POST_HIP(hipEventCreate(&ctx->ev0));
  if (!ctx->ev1) PNP_POST_HIP(hipEventCreate(&ctx->ev1));
  ctx->kernel_ms = -1.0f;
  PNP_POST_HIP(hipEventRecord(ctx->ev0, st));
  hipLaunchKernelGGL(steady_kernel, dim3((int)blocks), dim3(64), lds, st, a, tab);
  PNP_POST_HIP(hipGetLastError());
  PNP_POST_HIP(hipEventRecord(ctx->ev1, st));
  for (const Row& r : rows)
    if (r.wanted()) PNP_POST_HIP(hipMemcpyAsync(r.host, *r.dev, r.n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (out->status || out->iterations)
    PNP_POST_HIP(hipMemcpyAsync(ctx->flags.data(), a.status, 2 * sn * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PNP_POST_HIP(hipStreamSynchronize(st));
  PNP_POST_HIP(hipEventElapsedTime(&ctx->kernel_ms, ctx->ev0, ctx->ev1));
  if (out->status) memcpy(out->status, ctx->flags.data(), sn * sizeof(int32_t));
  if (out->iterations) memcpy(out->iterations, ctx->flags.data() + sn, sn * sizeof(int32_t));
  ctx->last_kernel = "catkin::steady_kernel";
  return CATKIN_OK;
}

}  // extern "C"
