// libcatint_response (include/catint_response.h): the linear response of a stationary state of the physical mode -- one block-tridiagonal
// solve (J + i omega S) du = r per (operating point, frequency) -- formed on the device from the state a pnp_handle holds there.  It
// shares no code with the Newton kernels (pnp_newton.hip, pnp_lane*.hip).  The rows of the Jacobian, the team mapping, the walk
// from block row to block row and the host code around the launch are defined once, in ../pnp_team.h, for this library and
// couple/catcpl.hip (the Gauss-Jordan step stands in both kernels: see there); here are the wall table, the right-hand side, the
// records and the substitution, and the scalars at the wall.
// gfx950 / MI355X only.
//
// Mapping: a TEAM of NB = N + 1 adjacent lanes per system (pnp_team.h); persistent waves walk groups of systems.  Systems beyond the
// last one repeat a valid one: like the partial team they run every step and only skip their stores.
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
// part in every exchange.
// Arithmetic order is fixed in the source (no implicit contraction), so the two instances of a block size and number type that differ
// only in RECORDS return the same scalars bit for bit.
#include <cstdlib>

#include "../../../include/catint_response.h"
#include "../pnp_team.h"

#pragma clang fp contract(off)

namespace catresp {

using namespace pnp::team;

using Table = pnp::team::WallTable;   // the reaction and wall tables of one call

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
  Consts k;
  double CS, eps, h0;   // C_S, eps, x[1] - x[0]
};

template <class T>
__device__ __forceinline__ void put(double* row, size_t at, T v, bool nan) {
  const double bad = __builtin_nan("");
  row[2 * at] = nan ? bad : re_(v);
  row[2 * at + 1] = nan ? bad : im_(v);
}

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
  constexpr int N = NB - 1, TPW = 64 / NB;
  const Lane ln = lane_of<NB>(A.sp);
  const int team = ln.team, r0 = ln.r0, base = ln.base;
  const bool isP = ln.isP;
  const int nx = A.nx;
  const Table& tb = *A.tab;

  __shared__ Ring<NB> ring;
  __shared__ T prow[2][TPW + 1][2 * NB];  // the pivot row of an elimination step (two buffers: one wave-level sync per step)
  __shared__ T tmat[TPW + 1][NB][NB];     // T_i
  __shared__ T t1row[TPW + 1][NB];        // row N of T_1

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

    Window w;
    double c4;
    open<NB>(A, ring, ln, urow, w, c4);

    T Aw[2 * NB];     // [D'_i | L_i], row r0
    double Ur[NB];    // U_i, row r0
    double rhs0 = 0.0;

    // the wall terms of row 0, formed before the row: the right-hand side and the wall table's part of M_0
    const auto wall_terms = [&](double (&wallM)[NB]) {
      rhs0 = 0.0;
      if (A.pert == CATRESP_PHIM) rhs0 = isP ? (A.stern ? -A.k.sternc : 1.0) : 0.0;
      else rhs0 = r0 == A.pspecies ? ln.dx / ln.Dk : 0.0;
      const double* cc = ring[0] + base;
      for (int r = 0; r < A.nwall; ++r) {
        const int s = tb.wspecies[r];
        double g, dg;
        wall_law(tb, r, s >= 0 ? cc[s] : 1.0, phiM - w.C.ph, g, dg);
        const double nk = tb.nu[r][r0] * A.kwall[b * A.nwall + r];
#pragma unroll
        for (int j = 0; j < N; ++j) wallM[j] += j == s ? -nk * dg * ln.dx / ln.Dk : 0.0;
        const double t = nk * tb.alpha[r] * g * ln.dx / ln.Dk;
        wallM[N] += t;
        if (A.pert == CATRESP_PHIM) rhs0 += t;
      }
    };

    first_row<NB, T>(A, tb, ring, ln, w, c4, omega, Aw, Ur);
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
      shift(A, ln, i, w);
      double wallM[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) wallM[j] = 0.0;
      if (i == 1) wall_terms(wallM);
      next_row<NB, T>(A, tb, ring, tmat[team], ln, w, i, nxt, omega, wallM, Aw, Ur);
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
      for (int j = 0; j < N; ++j) qs = add(qs, scale(A.k.q[j], x0[j]));
      dsig = add(scale(-A.eps / A.h0, fnma(d1, make<T>(1.0, 0.0), dph0)), scale(-0.5 * A.h0, qs));
    }
#pragma unroll
    for (int j = 0; j < N; ++j) adm = add(adm, scale(A.k.q[j], x0[NB + j]));
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
    const double anybad = team_sum<NB>(ring[0], ln);
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
static hipError_t dispatch(int NB, bool cx, bool rec, Fn&& f) {
  const auto with_nb = [&](auto nb) {
    if (cx && rec) return f(nb, std::true_type(), std::true_type());
    if (cx) return f(nb, std::true_type(), std::false_type());
    if (rec) return f(nb, std::false_type(), std::true_type());
    return f(nb, std::false_type(), std::false_type());
  };
  return dispatch_nb(NB, with_nb);
}

}  // namespace catresp

static_assert(CATRESP_OK == pnp::post::OK && CATRESP_EINVAL == pnp::post::ERR_INVAL && CATRESP_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATRESP_EDEVICE == pnp::post::ERR_DEVICE && CATRESP_MAX_NX == pnp::post::MAX_NX && CATRESP_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_response.h and pnp_post.h disagree");
static_assert(CATRESP_WALL_DIRICHLET == pnp::team::WALL_DIRICHLET && CATRESP_WALL_STERN == pnp::team::WALL_STERN &&
                  CATRESP_PIVOT_GROWTH_LIMIT == pnp::team::PIVOT_GROWTH_LIMIT,
              "catint_response.h and pnp_team.h disagree");

struct catresp_ctx : pnp::post::Ctx {};

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
  if (const int rc = check_medium(ctx, entry, view, p)) return rc;
  if (p->perturbation != CATRESP_PHIM && p->perturbation != CATRESP_WALL_FLUX) return fail(ctx, CATRESP_EINVAL, "catresp_solve: unknown perturbation");
  if (p->perturbation == CATRESP_WALL_FLUX && (p->species < 0 || p->species >= N)) {
    snprintf(msg, sizeof msg, "catresp_solve: perturbed species %d outside [0, %d)", p->species, N);
    return fail(ctx, CATRESP_EINVAL, msg);
  }
  if (const int rc = check_species(ctx, entry, p, N)) return rc;
  const int R = p->nreactions, W = p->n_wall, F = p->nfreq;
  if (const int rc = check_nreactions(ctx, entry, R)) return rc;
  if (const int rc = check_nwall(ctx, entry, W)) return rc;
  if (const int rc = check_reactions(ctx, entry, p, N)) return rc;
  if (const int rc = check_wall(ctx, entry, p, N)) return rc;
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
  if (const int rc = check_lanes(ctx, entry, p, B)) return rc;
  const int64_t n = p->nlanes;
  if (n == 0) return CATRESP_OK;

  KArgs a;
  memset(&a, 0, sizeof a);
  a.nx = nx; a.ldx = view->row_pitch; a.nreact = R; a.nwall = W; a.stern = p->wall_bc == CATRESP_WALL_STERN;
  a.pert = p->perturbation; a.pspecies = p->species; a.F = F; a.nsys = n * F;
  a.c = view->c_dev; a.phi = view->phi_dev; a.st = view->status_dev;
  a.steric = fill_consts(a.k, p, N, a.stern);
  a.CS = a.stern ? p->stern_capacitance : 0.0;
  a.eps = p->eps;
  a.h0 = p->x[1] - p->x[0];
  const bool rec = out->dc || out->dphi;
  const int TPW = 64 / NB;

  // the inputs, staged on the host for one copy: edge weights, control volumes, row constants, potentials, rate constants,
  // frequencies, lanes (int64 in the place of doubles), tables
  Inputs in;
  const int i_grid = declare_grid(in, a, nx), i_p = in.add((size_t)B, &a.phiM), i_k = in.add((size_t)B * W, &a.kwall),
            i_f = in.add((size_t)F, &a.omega), i_l = in.add_unpadded((size_t)n, &a.lanes), i_t = in.add_unpadded(sizeof(Table) / 8, &a.tab);
  const size_t n_in = in.total, nsys = (size_t)n * F;
  try {
    ctx->stage.assign(n_in, 0.0);
    ctx->flags.assign(nsys, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATRESP_ENOMEM, "catresp_solve: out of host memory");
  }
  stage_grid(in, ctx->stage, i_grid, p, nx, N);
  memcpy(in.host(ctx->stage, i_p), p->phiM, (size_t)B * 8);
  if (W) memcpy(in.host(ctx->stage, i_k), p->k, (size_t)B * W * 8);
  memcpy(in.host(ctx->stage, i_f), p->omega, (size_t)F * 8);
  stage_lanes(in.host(ctx->stage, i_l), p);
  Table* tb = reinterpret_cast<Table*>(in.host(ctx->stage, i_t));
  fill_reactions(tb, p);
  fill_wall(tb, p, N);

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
  int64_t blocks = 0;
  if (const int rc = persistent_waves(ctx, entry, p->max_waves, [&](int* per_cu) {
        return dispatch(NB, complex_call, rec, [&](auto nb, auto cx, auto rc_) { return resident<decltype(nb)::value, decltype(cx)::value, decltype(rc_)::value>(per_cu); });
      }, groups, &blocks))
    return rc;
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
  in.place(ctx->buf);
  double* cur = place_rows(rows, ctx->buf + n_in);
  a.status = reinterpret_cast<int32_t*>(cur);
  a.ws = cur + n_flags;
  if (const int rc = run_with_status(ctx, entry, st, n_in, rows, out->status, a.status, nsys, [&] {
        return dispatch(NB, complex_call, rec, [&](auto nb, auto cx, auto rc_) { return launch<decltype(nb)::value, decltype(cx)::value, decltype(rc_)::value>(a, blocks, st); });
      }))
    return rc;
  snprintf(msg, sizeof msg, "catresp::response_kernel<%d, %s, %s>", NB, complex_call ? "true" : "false", rec ? "true" : "false");
  ctx->last_kernel = msg;
  return CATRESP_OK;
}

}  // extern "C"
