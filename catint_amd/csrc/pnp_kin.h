// What the libraries that work on a mean-field surface microkinetic model with ONE OPERATING POINT PER LANE have in common
// (kinetics/catkin.hip, drc/catdrc.hip, kintrans/catkt.hip, scfkin/catscfkin.hip, eis/cateis.hip): the tables of a call, the rate constants
// and rates, the scaled rows of the steady state, the per-lane LU, and the host code around a launch.  Each library is one translation
// unit and compiles its own copy: nothing here is exported.  The frame of an entry point (context, staged inputs, rows, reserve, the
// tail) is that of pnp_post.h and pnp_stage.h.  gfx950 / MI355X only.
//
// Mapping: one operating point per lane, one wave per workgroup, persistent waves walking groups of 64 points.  No lane ever reads what
// another lane wrote, so there is no barrier and no cross-lane exchange; the only per-lane control is the row a lane chooses as its
// pivot, which is an address, and the branch of Ga, which is a select.
// Working set: everything that is indexed by a run-time step, column or row number lives in LDS as [slot][lane], the lane fastest (a
// wave's 8-byte accesses are conflict-free, and a per-lane row number is only an address): the matrix J[T][T] (T = S + 1), y[T], the
// right-hand side [T], the row scales D[T], the activities a[N] and what else the kernel keeps, sized per call (dynamic LDS).  The
// functions here take the lane's pointer to the first slot of an array (lds + lane + 64 slot): element e is p[64 e].  Registers hold
// scalars only, so nothing goes to scratch.  The pivot rows of the factorisation are kept as 4-bit fields of one 64-bit register.
// Tables (orders, stoichiometry, polynomial coefficients) are the same for every lane and are read at wave-uniform addresses through a
// read-only pointer: every loop over steps and columns has a uniform trip count.
// Arithmetic: IEEE divisions and the compiler's exp / log (pnp_math.h has exp(u) - 1 away from 0 and log(1 + x) on (-1, 0] only);
// implicit contraction is off, so a point's numbers do not depend on where in the batch it stands.  Every device function here switches
// it off in its own body: whatever the including source sets, and wherever it sets it, governs that source's code alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "pnp_post.h"

namespace pnp {
namespace kin {

using namespace pnp::post;

// the CATKIN_* / CATDRC_* limits and values
constexpr int MAXN = MAX_SPECIES, MAXS = 8, MAXT = MAXS + 1, MAXR = 16, MAXM = MAXN + MAXT, MAX_ORDER = 3;
constexpr int DROP_FULL = 0, DROP_STERN = 1;
constexpr double MINLOG = -700.0;
static_assert(MAXT <= 15, "a pivot row is a 4-bit field");

// the tables of one call, flattened on the host (everything validated there)
struct Table {
  int32_t of[MAXR][MAXM + 1], ob[MAXR][MAXM + 1];   // columns 0 .. N-1: species, N .. N+S: coverages
  double nu[MAXR][MAXN];
  double cref[MAXN];
  double ns[MAXT + 1];
  double dg[MAXR][4], ea[MAXR][4], lnA[MAXR];
};
static_assert(sizeof(Table) % 8 == 0, "the table is copied as doubles");

// ---- device ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite_(double a) { return fabs(a) < INFINITY; }

// y = ln of a given coverage g, clamped to [MINLOG, 0]
__device__ __forceinline__ double log_coverage(double g) {
  double y = g >= 1.0 ? 0.0 : (g > 0.0 ? log(g) : MINLOG);
  y = y < MINLOG ? MINLOG : y;
  return y;
}

// what the head of the loop over groups leaves of a point's inputs
struct Point {
  bool ok;             // every input finite, and on the view path the solver's lane converged
  double V, sg;        // potential and charge
  const double* off;   // [R][2] of the point, or null
};

// The inputs of point i (lane b of the view).  The activities go to the N slots from `a`.  A: the kernel's arguments, read by name
// (int32 N, R, w, use_sigma, from_view, ldx; c, phi, st of the view; cs, phis, phiM, sigma, off, gamma; CS, pzc)
template <class KA>
__device__ __forceinline__ Point point_inputs(const KA& A, const Table& tb, int64_t i, int64_t b, double* a) {
#pragma clang fp contract(off)
  const int N = A.N, R = A.R;
  Point pt;
  const double phiM = A.phiM[i];
  const double phi0 = A.from_view ? A.phi[(size_t)b * A.ldx] : A.phis[i];
  bool ok = finite_(phiM) && finite_(phi0);
  if (A.from_view) ok = ok && A.st[b] == 0;
  for (int j = 0; j < N; ++j) {
    const double c = A.from_view ? A.c[((size_t)b * N + j) * A.ldx] : A.cs[i * N + j];
    const double g = A.gamma ? A.gamma[i * N + j] : 1.0;
    ok = ok && finite_(c) && finite_(g);
    a[j * 64] = g * (c > 0.0 ? c : 0.0) / tb.cref[j];
  }
  pt.V = phiM - (A.w ? phi0 : 0.0);
  pt.sg = A.use_sigma ? A.sigma[i] : A.CS * ((phiM - A.pzc) - phi0);
  ok = ok && finite_(pt.sg);
  pt.off = A.off ? A.off + (size_t)i * R * 2 : nullptr;
  if (pt.off)
    for (int r = 0; r < 2 * R; ++r) ok = ok && finite_(pt.off[r]);
  pt.ok = ok;
  return pt;
}

// ln kf, ln kb of step r and the branch of Ga (0: Ea, 1: dG, 2: zero)
__device__ __forceinline__ void rate_constants(const Table& tb, double V, double sg, const double* off, int r, double& lf, double& lb, int& br) {
#pragma clang fp contract(off)
  const double s2 = sg * sg;
  const double dG = ((tb.dg[r][0] + tb.dg[r][1] * V) + tb.dg[r][2] * sg) + tb.dg[r][3] * s2;
  const double Ea = ((tb.ea[r][0] + tb.ea[r][1] * V) + tb.ea[r][2] * sg) + tb.ea[r][3] * s2;
  const bool b0 = Ea >= dG && Ea >= 0.0, b1 = dG >= 0.0;
  br = b0 ? 0 : (b1 ? 1 : 2);
  const double Ga = b0 ? Ea : (b1 ? dG : 0.0);
  const double o0 = off ? off[2 * r] : 0.0, o1 = off ? off[2 * r + 1] : 0.0;
  lf = (tb.lnA[r] - Ga) + o0;
  lb = (tb.lnA[r] - (Ga - dG)) + o1;
}

// d ln kf / dp and d ln kb / dp of step r for dV/dp = dV, dsigma/dp = ds
__device__ __forceinline__ void rate_constant_slopes(const Table& tb, double sg, int r, int br, double dV, double ds, double& dlf, double& dlb) {
#pragma clang fp contract(off)
  const double ddG = tb.dg[r][1] * dV + (tb.dg[r][2] + 2.0 * tb.dg[r][3] * sg) * ds;
  const double dEa = tb.ea[r][1] * dV + (tb.ea[r][2] + 2.0 * tb.ea[r][3] * sg) * ds;
  const double dGa = br == 0 ? dEa : (br == 1 ? ddG : 0.0);
  dlf = -dGa;
  dlb = -(dGa - ddG);
}

// the two factors of rf and rb: exp(ln k + sum_t order y_t) and prod_j a_j^order, y in the T slots from `y`, the activities in the N
// slots from `a`.  skip: a species whose order counts one less (the product with one factor left out), -1: none
__device__ __forceinline__ void rate_factors(const Table& tb, int N, int T, const double* y, const double* a, int r, double lf, double lb, int skip,
                                             double& ef, double& eb, double& pf, double& pb) {
#pragma clang fp contract(off)
  double sf = lf, sb = lb;
  for (int t = 0; t < T; ++t) {
    const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
    if (of | ob) {
      const double v = y[t * 64];
      if (of) sf = sf + (double)of * v;
      if (ob) sb = sb + (double)ob * v;
    }
  }
  pf = 1.0;
  pb = 1.0;
  for (int j = 0; j < N; ++j) {
    const int of = tb.of[r][j] - (j == skip ? 1 : 0), ob = tb.ob[r][j] - (j == skip ? 1 : 0);
    if (of > 0 || ob > 0) {
      const double v = a[j * 64];
      for (int e = 0; e < of; ++e) pf = pf * v;
      for (int e = 0; e < ob; ++e) pb = pb * v;
    }
  }
  ef = exp(sf);
  eb = exp(sb);
}

// step r at the rates rf, rb into the unscaled rows: its net rate into B, its gross rate into the row scales D, its derivative into J
__device__ __forceinline__ void add_step_rows(const Table& tb, int N, int T, int r, double rf, double rb, double* J, double* B, double* D) {
#pragma clang fp contract(off)
  const double net = rf - rb, gross = rf + rb;
  for (int s = 1; s < T; ++s) {
    const int m = tb.ob[r][N + s] - tb.of[r][N + s];
    if (m == 0) continue;
    const double dm = (double)m;
    B[s * 64] = B[s * 64] + dm * net;
    D[s * 64] = D[s * 64] + fabs(dm) * gross;
    for (int t = 0; t < T; ++t) {
      const int of = tb.of[r][N + t], ob = tb.ob[r][N + t];
      if (of | ob) {
        double* e = &J[(s * T + t) * 64];
        *e = *e + dm * (rf * (double)of - rb * (double)ob);
      }
    }
  }
}

// Row s of J divided by its scale d.  An adsorbate that nothing produces or consumes (d == 0: a dead row) gets the identity row and is
// set to MINLOG, where the row keeps it.  Returns whether the row is dead
__device__ __forceinline__ bool scale_row(double* J, double* y, int T, int s, double d) {
#pragma clang fp contract(off)
  const bool dead = d == 0.0;
  for (int t = 0; t < T; ++t) {
    double* e = &J[(s * T + t) * 64];
    *e = dead ? (t == s ? 1.0 : 0.0) : *e / d;
  }
  if (dead) y[s * 64] = MINLOG;
  return dead;
}

// the site row: n_t theta_t into row 0 of J; their sum
__device__ __forceinline__ double site_row(const Table& tb, double* J, const double* y, int T) {
#pragma clang fp contract(off)
  double f0 = 0.0;
  for (int t = 0; t < T; ++t) {
    const double th = tb.ns[t] * exp(y[t * 64]);
    J[t * 64] = th;
    f0 = f0 + th;
  }
  return f0;
}

// LU with partial row pivoting in place: rows exchanged whole, multipliers below the diagonal, the pivot row of step k in bits
// 4k .. 4k+3 (the first of equal magnitudes wins).  Returns whether a pivot was zero or not finite
__device__ __forceinline__ bool factor(double* J, int T, uint64_t& pivs) {
#pragma clang fp contract(off)
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

// the right-hand side in the T slots from `b` against the stored factors, in place
__device__ __forceinline__ void substitute(const double* J, double* b, int T, uint64_t pivs) {
#pragma clang fp contract(off)
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

// ---- device: the steady state of one lane (kinetics/catkin.hip and scfkin/catscfkin.hip compile it from this one text) -------------
// what one lane of a steady-state kernel carries in registers
struct SteadyLane {
  double* L;       // lds + lane: slot s at L[s * 64]
  int oJ, oY, oB, oD, oA, oC;   // first slots of J, y, right-hand side, D, activities, accumulators
  Point pt;        // potential, charge and off row of the point
  __device__ __forceinline__ double* at(int slot) const { return L + slot * 64; }
};

// the slots of a lane for N species and T = S + 1 coverages: (max(T T, N) + 3 T + 2 N) of them
__device__ __forceinline__ void steady_slots(SteadyLane& ln, double* lds, int lane, int N, int T) {
  ln.L = lds + lane;
  ln.oJ = 0;
  ln.oY = T * T > N ? T * T : N;
  ln.oB = ln.oY + T;
  ln.oD = ln.oB + T;
  ln.oA = ln.oD + T;
  ln.oC = ln.oA + N;
}

// rf and rb of step r at the lane's y; skip: see rate_factors.  A: the kernel's arguments, read by name (int32 N, S, R here; maxit and
// tol in steady_newton)
template <class KA>
__device__ __forceinline__ void steady_rates(const KA& A, const Table& tb, const SteadyLane& ln, int r, int skip, int& br, double& ef, double& eb,
                                             double& pf, double& pb) {
#pragma clang fp contract(off)
  double lf, lb;
  rate_constants(tb, ln.pt.V, ln.pt.sg, ln.pt.off, r, lf, lb, br);
  rate_factors(tb, A.N, A.S + 1, ln.at(ln.oY), ln.at(ln.oA), r, lf, lb, skip, ef, eb, pf, pb);
}

// J (scaled rows), right-hand side -F and the row scales D at the lane's y
template <class KA>
__device__ __forceinline__ void steady_assemble(const KA& A, const Table& tb, const SteadyLane& ln) {
#pragma clang fp contract(off)
  const int N = A.N, T = A.S + 1;
  double* L = ln.L;
  for (int s = 0; s < T * T; ++s) L[(ln.oJ + s) * 64] = 0.0;
  for (int s = 0; s < T; ++s) L[(ln.oB + s) * 64] = 0.0, L[(ln.oD + s) * 64] = 0.0;
  for (int r = 0; r < A.R; ++r) {
    double ef, eb, pf, pb;
    int br;
    steady_rates(A, tb, ln, r, -1, br, ef, eb, pf, pb);
    add_step_rows(tb, N, T, r, ef * pf, eb * pb, ln.at(ln.oJ), ln.at(ln.oB), ln.at(ln.oD));
  }
  for (int s = 1; s < T; ++s) {
    const double D = L[(ln.oD + s) * 64];
    const bool dead = scale_row(ln.at(ln.oJ), ln.at(ln.oY), T, s, D);
    const double g = L[(ln.oB + s) * 64];
    L[(ln.oB + s) * 64] = dead ? 0.0 : -(g / D);
  }
  const double f0 = site_row(tb, ln.at(ln.oJ), ln.at(ln.oY), T);
  L[ln.oB * 64] = -(f0 - 1.0);
}

// The damped Newton iteration from the y in the lane's slots: the update scaled by min(1, 3 / max|dy|), y clamped to >= MINLOG, stopped
// when max|dy| < A.tol (the update still applied) or after A.maxit iterations.  A finished lane idles: its unknowns stop changing.
// start: what the status is before the first iteration (STATUS_MAXIT for a lane that iterates, STATUS_INPUT for one whose inputs are
// bad); run: the lane iterates.  Returns the status; it: the iterations taken; pivs: the pivot rows of the last factorisation
constexpr int STATUS_CONVERGED = 0, STATUS_MAXIT = 1, STATUS_INPUT = 2, STATUS_PIVOT = 3;   // the CATKIN_* values
template <class KA>
__device__ __forceinline__ int steady_newton(const KA& A, const Table& tb, const SteadyLane& ln, int start, bool run, int& it, uint64_t& pivs) {
#pragma clang fp contract(off)
  const int T = A.S + 1;
  double* L = ln.L;
  int status = start;
  bool active = run;
  it = 0;
  pivs = 0;
  for (int iter = 0; iter < A.maxit; ++iter) {
    if (__ballot(active) == 0) break;
    steady_assemble(A, tb, ln);
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

// The rates at the lane's y summed into the fluxes: sum_r nu_rk (rf_r - rb_r) into the N accumulator slots, sum_r |nu_rk| (rf_r + rb_r)
// (flux_scale without the site density) into the first N slots of J, which are free by now.  per_step(r, net, gross) sees every step
template <class KA, class F>
__device__ __forceinline__ void steady_fluxes(const KA& A, const Table& tb, const SteadyLane& ln, F&& per_step) {
#pragma clang fp contract(off)
  const int N = A.N, R = A.R;
  double* L = ln.L;
  for (int k = 0; k < N; ++k) L[(ln.oC + k) * 64] = 0.0, L[(ln.oJ + k) * 64] = 0.0;
  for (int r = 0; r < R; ++r) {
    double ef, eb, pf, pb;
    int br;
    steady_rates(A, tb, ln, r, -1, br, ef, eb, pf, pb);
    const double rf = ef * pf, rb = eb * pb, net = rf - rb, gross = rf + rb;
    per_step(r, net, gross);
    for (int k = 0; k < N; ++k) {
      const double nu = tb.nu[r][k];
      if (nu != 0.0) {
        L[(ln.oC + k) * 64] = L[(ln.oC + k) * 64] + nu * net;
        L[(ln.oJ + k) * 64] = L[(ln.oJ + k) * 64] + fabs(nu) * gross;
      }
    }
  }
}

// (the context is pnp::post::Ctx)
// ---- host: what an entry point checks, in three parts; the library's own checks stand between them.  0 or the code.  Params:
// ---- catkin_params / catdrc_params, read by the member names the two share; entry: the exported function, the head of every message --
static bool posfin(double v) { return v > 0.0 && std::isfinite(v); }

// the arguments themselves and the sizes of the model
template <class Params, class Outputs>
static int check_sizes(Ctx* ctx, const char* entry, const char* params_name, const char* outputs_name, const Params* p, const Outputs* out) {
  if (!ctx) return ERR_INVAL;
  const std::string e(entry);
  char msg[256];
  if (!p || !out) return fail(ctx, ERR_INVAL, e + ": null argument");
  if (p->struct_size != (int32_t)sizeof(Params)) return fail(ctx, ERR_INVAL, e + ": " + params_name + ".struct_size does not match this library");
  if (out->struct_size != (int32_t)sizeof(Outputs)) return fail(ctx, ERR_INVAL, e + ": " + outputs_name + ".struct_size does not match this library");
  const int N = p->nspecies, S = p->nadsorbates, R = p->nsteps;
  if (N < 0 || N > MAXN) {
    snprintf(msg, sizeof msg, "%s: %d species outside [0, %d]", entry, N, MAXN);
    return fail(ctx, ERR_INVAL, msg);
  }
  if (S < 1 || S > MAXS) {
    snprintf(msg, sizeof msg, "%s: %d adsorbates outside [1, %d]", entry, S, MAXS);
    return fail(ctx, ERR_INVAL, msg);
  }
  if (R < 1 || R > MAXR) {
    snprintf(msg, sizeof msg, "%s: %d steps outside [1, %d]", entry, R, MAXR);
    return fail(ctx, ERR_INVAL, msg);
  }
  if (p->max_waves < 0) return fail(ctx, ERR_INVAL, e + ": negative max_waves");
  return OK;
}

template <class Params>
static int check_drop(Ctx* ctx, const char* entry, const Params* p) {
  if (p->potential_drop != DROP_FULL && p->potential_drop != DROP_STERN)
    return fail(ctx, ERR_INVAL, std::string(entry) + ": potential_drop is 0 (full) or 1 (Stern)");
  return OK;
}

// the tables
template <class Params>
static int check_tables(Ctx* ctx, const char* entry, const Params* p) {
  const std::string e(entry);
  char msg[256];
  const int N = p->nspecies, R = p->nsteps, T = p->nadsorbates + 1, M = N + T;
  if (!posfin(p->site_density)) return fail(ctx, ERR_INVAL, e + ": site_density must be positive and finite");
  if (!p->order_f || !p->order_b || !p->site_count || !p->dG || !p->Ea || !p->lnA || (N > 0 && (!p->nu || !p->cref)))
    return fail(ctx, ERR_INVAL, e + ": order_f, order_b, nu, cref, site_count, dG, Ea and lnA are required");
  for (int j = 0; j < N; ++j)
    if (!posfin(p->cref[j])) {
      snprintf(msg, sizeof msg, "%s: cref[%d] must be positive and finite", entry, j);
      return fail(ctx, ERR_INVAL, msg);
    }
  for (int t = 0; t < T; ++t) {
    const double v = p->site_count[t];
    if (!(t == 0 ? v == 1.0 : (v == 1.0 || v == 2.0 || v == 3.0))) {
      snprintf(msg, sizeof msg, "%s: site count %d must be 1, 2 or 3 (1 for the free site)", entry, t);
      return fail(ctx, ERR_INVAL, msg);
    }
  }
  for (int r = 0; r < R; ++r) {
    double sites = 0.0;
    bool any_f = false, any_b = false, any_nu = false;
    for (int c = 0; c < M; ++c) {
      const int of = p->order_f[r * M + c], ob = p->order_b[r * M + c];
      if (of < 0 || of > MAX_ORDER || ob < 0 || ob > MAX_ORDER) {
        snprintf(msg, sizeof msg, "%s: step %d has an order outside [0, %d]", entry, r, MAX_ORDER);
        return fail(ctx, ERR_INVAL, msg);
      }
      any_f = any_f || of;
      any_b = any_b || ob;
      if (c >= N) sites += p->site_count[c - N] * (ob - of);
    }
    if (sites != 0.0) {
      snprintf(msg, sizeof msg, "%s: step %d does not conserve sites", entry, r);
      return fail(ctx, ERR_INVAL, msg);
    }
    for (int k = 0; k < N; ++k) {
      if (!std::isfinite(p->nu[r * N + k])) {
        snprintf(msg, sizeof msg, "%s: nu of step %d is not finite", entry, r);
        return fail(ctx, ERR_INVAL, msg);
      }
      any_nu = any_nu || p->nu[r * N + k] != 0.0;
    }
    if ((!any_f || !any_b) && !any_nu) {
      snprintf(msg, sizeof msg, "%s: step %d is an empty step (no orders on a side and no stoichiometry)", entry, r);
      return fail(ctx, ERR_INVAL, msg);
    }
    bool fin = std::isfinite(p->lnA[r]);
    for (int q = 0; q < 4; ++q) {
      fin = fin && std::isfinite(p->dG[r * 4 + q]);
      const double v = p->Ea[r * 4 + q];
      fin = fin && (std::isfinite(v) || (q == 0 && v == -INFINITY));
    }
    if (!fin) {
      snprintf(msg, sizeof msg, "%s: step %d has a non-finite table entry (only e0 may be -INFINITY)", entry, r);
      return fail(ctx, ERR_INVAL, msg);
    }
  }
  if (!p->phiM) return fail(ctx, ERR_INVAL, e + ": phiM is required");
  return OK;
}

// the surface charge, the points and where their surface state comes from (*from_view: the view)
template <class Params>
static int check_points(Ctx* ctx, const char* entry, const pnp_device_view* view, const Params* p, bool* from_view) {
  const std::string e(entry);
  char msg[256];
  if (!p->sigma && !(std::isfinite(p->stern_capacitance) && std::isfinite(p->phi_pzc)))
    return fail(ctx, ERR_INVAL, e + ": the surface charge needs sigma or a finite stern_capacitance and phi_pzc");
  if (p->n < 0) return fail(ctx, ERR_INVAL, e + ": n < 0");
  const int64_t n = p->n;
  if ((p->csurf == nullptr) != (p->phi_surface == nullptr))
    return fail(ctx, ERR_INVAL, e + ": csurf and phi_surface come together (or both NULL: the view)");
  *from_view = !p->csurf;
  if (*from_view) {
    if (!view) return fail(ctx, ERR_INVAL, e + ": null view without csurf and phi_surface");
    if (view->struct_size != (int32_t)sizeof(pnp_device_view)) return fail(ctx, ERR_INVAL, e + ": pnp_device_view.struct_size does not match this library");
    if (!view->phi_dev || !view->c_dev)
      return fail(ctx, ERR_INVAL, e + ": the view has no potential row (only the physical mode keeps the potential in its state)");
    if (!view->status_dev) return fail(ctx, ERR_INVAL, e + ": the view has no status row");
    if (view->nspecies != p->nspecies) {
      snprintf(msg, sizeof msg, "%s: %d species, the view has %d", entry, p->nspecies, view->nspecies);
      return fail(ctx, ERR_INVAL, msg);
    }
    if (view->batch < 1 || view->nx < 1 || view->row_pitch < view->nx) return fail(ctx, ERR_INVAL, e + ": empty batch or a row pitch below nx");
    if (!p->lanes && n > view->batch) return fail(ctx, ERR_INVAL, e + ": n above the batch (lanes is NULL)");
    if (p->lanes)
      for (int64_t i = 0; i < n; ++i)
        if (p->lanes[i] < 0 || p->lanes[i] >= view->batch) {
          snprintf(msg, sizeof msg, "%s: lane index %lld outside [0, %lld)", entry, (long long)p->lanes[i], (long long)view->batch);
          return fail(ctx, ERR_INVAL, msg);
        }
  } else if (view && view->struct_size != (int32_t)sizeof(pnp_device_view)) {
    return fail(ctx, ERR_INVAL, e + ": pnp_device_view.struct_size does not match this library");
  }
  return OK;
}

// ---- host: the inputs of a call, staged for one copy -----------------------------------------------------------------------------------
struct Stage {
  bool from_view;     // the surface state comes from the view, not from csurf and phi_surface
  Inputs in;          // the inputs every kernel here reads, then what the library declared behind them
  const Table* tab;   // device: the table, a kernel argument of its own (read-only: scalar loads)
  Stage() = default;
  Stage(const Stage&) = delete;   // `in` holds the address of `tab`
};

template <class Params>
static void fill_table(Table* tb, const Params* p) {
  const int N = p->nspecies, R = p->nsteps, T = p->nadsorbates + 1, M = N + T;
  for (int r = 0; r < R; ++r) {
    for (int c = 0; c < M; ++c) tb->of[r][c] = p->order_f[r * M + c], tb->ob[r][c] = p->order_b[r * M + c];
    for (int k = 0; k < N; ++k) tb->nu[r][k] = p->nu[r * N + k];
    for (int q = 0; q < 4; ++q) tb->dg[r][q] = p->dG[r * 4 + q], tb->ea[r][q] = p->Ea[r * 4 + q];
    tb->lnA[r] = p->lnA[r];
  }
  for (int j = 0; j < N; ++j) tb->cref[j] = p->cref[j];
  for (int t = 0; t < T; ++t) tb->ns[t] = p->site_count[t];
}

// Declares the inputs every kernel here reads, in this order, with the members of the arguments `a` that take their device addresses:
// phiM; csurf and phi_surface (not from the view); sigma, off, gamma (where given); the coverages [n][T] the library takes (theta:
// catkin's optional guess, catdrc's state, or null; their address goes to *theta_dev); the lanes; the Table (s->tab).  more(s->in)
// declares what the library stages behind them.  Then sizes ctx->stage for all of it, fills what was declared here, and sizes
// ctx->flags to `flag_rows` int32 rows of n.
template <class KA, class Params, class More>
static int stage_inputs(Ctx* ctx, const char* entry, const Params* p, KA& a, const double* theta, const double** theta_dev, bool from_view,
                        int flag_rows, Stage* s, More&& more) {
  const int N = p->nspecies, R = p->nsteps, T = p->nadsorbates + 1;
  const int64_t n = p->n;
  const size_t sn = (size_t)n;
  s->from_view = from_view;
  Inputs& in = s->in;
  const int i_pm = in.add(sn, &a.phiM);
  const int i_cs = from_view ? -1 : in.add(sn * N, &a.cs), i_ps = from_view ? -1 : in.add(sn, &a.phis);
  const int i_sg = p->sigma ? in.add(sn, &a.sigma) : -1, i_off = p->off ? in.add(sn * R * 2, &a.off) : -1;
  const int i_gm = (p->gamma && N) ? in.add(sn * N, &a.gamma) : -1, i_th = theta ? in.add(sn * T, theta_dev) : -1;
  const int i_l = in.add_unpadded(sn, &a.lanes), i_t = in.add_unpadded(sizeof(Table) / 8, &s->tab);
  more(in);
  try {
    ctx->stage.assign(in.total, 0.0);
    ctx->flags.assign(flag_rows * sn, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, ERR_NOMEM, std::string(entry) + ": out of host memory");
  }
  std::vector<double>& sg = ctx->stage;
  memcpy(in.host(sg, i_pm), p->phiM, sn * 8);
  if (!from_view) {
    if (N) memcpy(in.host(sg, i_cs), p->csurf, sn * N * 8);
    memcpy(in.host(sg, i_ps), p->phi_surface, sn * 8);
  }
  if (p->sigma) memcpy(in.host(sg, i_sg), p->sigma, sn * 8);
  if (p->off) memcpy(in.host(sg, i_off), p->off, sn * R * 2 * 8);
  if (p->gamma && N) memcpy(in.host(sg, i_gm), p->gamma, sn * N * 8);
  if (theta) memcpy(in.host(sg, i_th), theta, sn * T * 8);
  int64_t* l = reinterpret_cast<int64_t*>(in.host(sg, i_l));
  for (int64_t i = 0; i < n; ++i) l[i] = (from_view && p->lanes) ? p->lanes[i] : i;
  fill_table(reinterpret_cast<Table*>(in.host(sg, i_t)), p);
  return OK;
}

// the members of the kernel's arguments that both kernels have, but for the device addresses (KA: see point_inputs; n, S, sd on top)
template <class KA, class Params>
static void set_args(KA& a, const pnp_device_view* view, const Params* p, bool from_view) {
  memset(&a, 0, sizeof a);
  a.N = p->nspecies; a.S = p->nadsorbates; a.R = p->nsteps; a.w = p->potential_drop; a.use_sigma = p->sigma != nullptr;
  a.from_view = from_view; a.n = p->n;
  a.sd = p->site_density; a.CS = p->stern_capacitance; a.pzc = p->phi_pzc;
  if (from_view) {
    a.ldx = view->row_pitch;
    a.c = view->c_dev; a.phi = view->phi_dev; a.st = view->status_dev;
  }
}

// The tail of an entry point.  One wave per block: max_waves of them, or (0) what the device holds at `lds` bytes each; the output
// rows and `flag_rows` int32 rows of n behind the staged inputs; own(int32_t* flags) puts the device address of the int32 rows into
// the arguments `a` under the library's own names; then pnp::post::launch_and_fetch with `kernel`, whose name `kernel_name` is
// recorded (the int32 rows come back to ctx->flags when want_flags).
template <class KA, class Params, size_t NR, class F>
static int run(Ctx* ctx, const char* entry, const char* kernel_name, void (*kernel)(const KA, const Table*), const pnp_device_view* view, const Params* p,
               const Stage& s, KA& a, const Row (&rows)[NR], size_t lds, int flag_rows, bool want_flags, F&& own) {
  const int64_t n = p->n;
  const size_t sn = (size_t)n, n_in = s.in.total;
  const size_t need_out = rows_doubles(rows), n_flags = even(sn) * flag_rows / 2;
  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = s.from_view ? (hipStream_t)view->stream : (hipStream_t) nullptr;
  if (lds > 48 * 1024) PNP_POST_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int64_t blocks = 0;
  if (const int rc = persistent_waves(ctx, entry, p->max_waves, [&](int* per_cu) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kernel, 64, lds);
      }, (n + 63) / 64, &blocks))
    return rc;
  if (const int rc = reserve(ctx, entry, n_in + need_out + n_flags)) return rc;
  s.in.place(ctx->buf);
  int32_t* flags_dev = reinterpret_cast<int32_t*>(place_rows(rows, ctx->buf + n_in));
  own(flags_dev);
  if (const int rc = launch_and_fetch(ctx, entry, st, n_in, rows, Flags{flags_dev, flag_rows * sn, want_flags}, &ctx->kernel_ms, [&] {
        hipLaunchKernelGGL(kernel, dim3((int)blocks), dim3(64), lds, st, a, s.tab);
        return hipSuccess;
      }))
    return rc;
  ctx->last_kernel = kernel_name;
  return OK;
}

}  // namespace kin
}  // namespace pnp
