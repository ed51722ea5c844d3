// libcatint_drc (include/catint_drc.h): the degree of rate control of a microkinetic steady state per operating point -- the Jacobian of
// the scaled steady-state rows at the given coverages factorised once, then one right-hand side per rate constant, transition state
// and adsorbate energy.  gfx950 / MI355X only.
//
// Mapping, working set, tables and arithmetic: ../pnp_kin.h, which also holds the rates, the rows, the LU and the host code this
// library shares with kinetics/catkin.hip.  LDS slots: J[T][T], y[T], the right-hand side [T], the row scales D[T], N slots that hold
// the activities until the rates are formed and the column's accumulators afterwards, the fluxes [N], the gross rates rf[R], rb[R] --
// formed once per point (two exp per step) and read by every one of the up to 3 R + S columns -- and the T slots of the refinement
// step.  At S = N = 8, R = 16: 165 slots x 512 B = 82.5 KB per wave (the attribute raised above the default).  The branches of Ga are
// 2-bit fields of one 32-bit register; a step outside a column's support is skipped by a uniform test.
#include "../../../include/catint_drc.h"
#include "../pnp_kin.h"

#pragma clang fp contract(off)

namespace catdrc {

using namespace pnp::kin;

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

// what one lane carries in registers
struct Lane {
  double* L;       // lds + lane: slot s at L[s * 64]
  int oJ, oY, oB, oD, oA, oF, oRf, oRb, oX;   // first slots of J, y / theta, right-hand side, D, activities / accumulators, fluxes, rf, rb, refinement
  __device__ __forceinline__ double* at(int slot) const { return L + slot * 64; }
};

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
  substitute(ln.at(ln.oJ), ln.at(ln.oB), T, pivs);
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
  substitute(ln.at(ln.oJ), ln.at(ln.oX), T, pivs);
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
    const Point pt = point_inputs(A, tb, i, b, ln.at(ln.oA));
    bool ok = pt.ok;
    // ---- the state: y = ln theta, clamped as catkin clamps its guess ----
    for (int t = 0; t < T; ++t) {
      const double g = A.theta[i * T + t];
      ok = ok && finite_(g);
      L[(ln.oY + t) * 64] = log_coverage(g);
    }
    // ---- rf, rb once per point; the branch of Ga of step r in bits 2r, 2r+1 (0: Ea, 1: dG, 2: zero) ----
    uint32_t brs = 0;
    for (int r = 0; r < R; ++r) {
      double lf, lb, ef, eb, pf, pb;
      int br;
      rate_constants(tb, pt.V, pt.sg, pt.off, r, lf, lb, br);
      brs |= (uint32_t)br << (2 * r);
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
      add_step_rows(tb, N, T, r, rf, rb, ln.at(ln.oJ), ln.at(ln.oB), ln.at(ln.oD));
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
      const bool dead = scale_row(ln.at(ln.oJ), ln.at(ln.oY), T, s, D);
      const double f = dead ? 0.0 : fabs(L[(ln.oB + s) * 64] / D);
      res = f > res || f != f ? f : res;
    }
    {
      const double f = fabs(site_row(tb, ln.at(ln.oJ), ln.at(ln.oY), T) - 1.0);
      res = f > res || f != f ? f : res;
      // y has done its work: the site row stays in its slots for the refinement
      for (int t = 0; t < T; ++t) L[(ln.oY + t) * 64] = L[(ln.oJ + t) * 64];
    }
    uint64_t pivs = 0;
    const bool bad = factor(ln.at(ln.oJ), T, pivs);
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
static_assert(CATDRC_MAX_SPECIES == pnp::kin::MAXN && CATDRC_MAX_ADSORBATES == pnp::kin::MAXS && CATDRC_MAX_STEPS == pnp::kin::MAXR &&
                  CATDRC_MAX_ORDER == pnp::kin::MAX_ORDER && CATDRC_MIN_LOG == pnp::kin::MINLOG && CATDRC_DROP_FULL == pnp::kin::DROP_FULL &&
                  CATDRC_DROP_STERN == pnp::kin::DROP_STERN,
              "catint_drc.h and pnp_kin.h disagree");
static_assert(CATDRC_MAX_STEPS <= 16 && CATDRC_MAX_SPECIES <= 32, "a branch is a 2-bit field of 32 bits, an idle species one bit");

struct catdrc_ctx : pnp::post::Ctx {};

extern "C" {

int catdrc_create(int32_t device, catdrc_ctx** out) { return pnp::post::create("catdrc_create", device, out); }
void catdrc_destroy(catdrc_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catdrc_last_error(const catdrc_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catdrc_last_kernel(const catdrc_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catdrc_last_kernel_ms(const catdrc_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catdrc_solve(catdrc_ctx* ctx, const pnp_device_view* view, const catdrc_params* p, const catdrc_outputs* out) {
  using namespace catdrc;
  static const char entry[] = "catdrc_solve";
  if (const int rc = check_sizes(ctx, entry, "catdrc_params", "catdrc_outputs", p, out)) return rc;
  if (const int rc = check_drop(ctx, entry, p)) return rc;
  if (!posfin(p->residual_tol)) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: residual_tol must be positive and finite");
  if (const int rc = check_tables(ctx, entry, p)) return rc;
  if (!p->theta) return fail(ctx, CATDRC_EINVAL, "catdrc_solve: theta is required (the coverages catkin_solve returned)");
  bool from_view = false;
  if (const int rc = check_points(ctx, entry, view, p, &from_view)) return rc;
  if (p->n == 0) return CATDRC_OK;

  const int N = p->nspecies, S = p->nadsorbates, R = p->nsteps, T = S + 1;
  const size_t sn = (size_t)p->n;
  KArgs a;
  set_args(a, view, p, from_view);
  Stage stage;
  if (const int rc = stage_inputs(ctx, entry, p, a, p->theta, &a.theta, from_view, 1, &stage, [](Inputs&) {})) return rc;   // the status
  a.rtol = p->residual_tol;
  const Row rows[] = {{out->dflux_dlnkf, &a.dkf, sn * R * N}, {out->dflux_dlnkb, &a.dkb, sn * R * N}, {out->dflux_drc, &a.dts, sn * R * N},
                      {out->dy_drc, &a.dyts, sn * R * T},     {out->drc, &a.xrc, sn * R * N},         {out->dflux_dG, &a.dG, sn * S * N},
                      {out->tdrc, &a.xtrc, sn * S * N},       {out->flux, &a.flux, sn * N},           {out->flux_scale, &a.fscale, sn * N},
                      {out->residual, &a.resid, sn}};
  if (!rows_doubles(rows) && !out->status) return CATDRC_OK;
  const int rc = run(ctx, entry, "catdrc::control_kernel", control_kernel, view, p, stage, a, rows, lds_bytes(N, S, R), 1, out->status != nullptr,
                     [&](int32_t* flags) { a.status = flags; });
  if (rc) return rc;
  if (out->status) memcpy(out->status, ctx->flags.data(), sn * sizeof(int32_t));
  return CATDRC_OK;
}

}  // extern "C"
