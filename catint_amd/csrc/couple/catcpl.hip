// libcatint_couple (include/catint_couple.h): one Newton step of the self-consistency between kinetics and transport per operating
// point, formed on the device from the state a pnp_handle holds there.  It shares no code with the Newton kernels.  The rows of the
// stationary Jacobian (that of catint_response.h with n_wall = 0), the team mapping, the walk from block row to block row and
// the host code around the launch are defined once, in ../pnp_team.h, for this library and response/catresp.hip (the Gauss-Jordan
// step stands in both kernels: see there); here are the columns [W | E] at the wall, the pivoted elimination of [A | -G] and the
// damping.  Real arithmetic only.  gfx950 / MI355X only.
//
// Mapping (pnp_team.h): a TEAM of NB = N + 1 adjacent lanes per system; persistent waves walk groups of systems.
// Systems beyond the last one repeat a valid one: like the partial team they run every step and only skip their stores.
// Elimination: block Thomas from the bulk towards the wall, T_i = D'_i^-1 L_i by Gauss-Jordan without row exchanges across the team,
// D'_{i-1} = M_{i-1} - U_{i-1} T_i, every step monitored (status 1).  Nothing is kept between block rows.
// The wall: Gauss-Jordan on [W | E], E = diag(dx / D_k) with a zero Poisson row, leaves row r of the transport tangent T = W^-1 E in
// lane r (rows 0 .. N-1: T_c, row N: T_phi) -- all N columns from the one elimination.  Lane k < N then forms row k of
// A = I - rf (Kc T_c + Kphi (x) T_phi) and the entry -G_k of the right-hand side, the team eliminates A by Gauss-Jordan WITH partial
// row pivoting (the pivot lane is found through LDS, rows stay where they are), applies the damping rule and stores.  O(N^3) per
// system on top of an elimination that is O(nx N^3).
// Arithmetic order is fixed in the source (no implicit contraction); the elimination of a column of E performs the operations
// catresp.hip performs on its single right-hand side, in the same order.  Results leave through plain vector
// stores.
#include "../../../include/catint_couple.h"
#include "../pnp_team.h"

#pragma clang fp contract(off)

namespace catcpl {

using namespace pnp::team;

using Table = ReactionTable;

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
  Consts k;
  double rf, dphi_max;
};

template <int NB>
__global__ __launch_bounds__(64) void couple_kernel(const KArgs A) {
  constexpr int N = NB - 1, TPW = 64 / NB, RW = (TPW + 1) * NB;
  const Lane ln = lane_of<NB>(A.sp);
  const int team = ln.team, r0 = ln.r0, base = ln.base;
  const bool isP = ln.isP;
  const int nx = A.nx;
  const Table& tb = *A.tab;

  __shared__ Ring<NB> ring;
  __shared__ double prow[2][TPW + 1][2 * NB];  // the pivot row of an elimination step (two buffers: one wave-level sync per step)
  __shared__ double tmat[TPW + 1][NB][NB];     // T_i; at the wall the transport tangent
  __shared__ double xch[2][RW];                // the wall stage: pivot search, solution, flags

  for (int64_t grp = blockIdx.x; grp * TPW < A.nsys; grp += gridDim.x) {
    const int64_t sys = grp * TPW + team;
    const bool live = team < TPW && sys < A.nsys;
    const int64_t sy = live ? sys : grp * TPW;
    const int64_t b = A.lanes[sy];
    const double* urow = isP ? A.phi + (size_t)b * A.ldx : A.c + ((size_t)b * N + r0) * A.ldx;
    bool bad = false;

    Window w;
    double c4;
    open<NB>(A, ring, ln, urow, w, c4);

    double Aw[2 * NB];   // [D'_i | L_i], row r0; at the wall [W | E]
    double Ur[NB];       // U_i, row r0

    first_row<NB, double>(A, tb, ring, ln, w, c4, 0.0, Aw, Ur);

#pragma unroll 1
    for (int i = nx - 2; i >= 0; --i) {
      const double nxt = i >= 3 ? urow[i - 3] : 0.0;   // the point the row after next needs: used at the end of this block row
      if (i == 0) {
        // the wall: the N columns of E in the place of L (column N, the Poisson unknown, is zero)
        const double e0 = ln.dx / ln.Dk;
#pragma unroll
        for (int j = 0; j < NB; ++j) Aw[NB + j] = (j == r0 && !isP) ? e0 : 0.0;
      }
      // ---- Gauss-Jordan on [D' | L] across the team, no row exchanges ----
#pragma unroll
      for (int p = 0; p < NB; ++p) {
        const bool mine = r0 == p;
        const double piv = Aw[p];
        bad = bad || (mine && !(nonzero(piv) && finite_(piv)));
        const double ip = inv(piv);
        double* pr = prow[p & 1][team];
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
      next_row<NB, double>(A, tb, ring, tmat[team], ln, w, i, nxt, 0.0, wallM, Aw, Ur);
    }

    // ---- the wall: row r0 of T = W^-1 E is Aw[NB .. NB + N); w.C.c is the lane's own unknown at the wall point ----
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
    } else if (w.C.c > 0.0 && dstate < 0.0) {
      lc = fmin(1.0, 0.9 * w.C.c / (-dstate));
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
    const double anybad = team_sum<NB>(xch[0], ln), anysing = team_sum<NB>(xch[1], ln);
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

}  // namespace catcpl

static_assert(CATCPL_OK == pnp::post::OK && CATCPL_EINVAL == pnp::post::ERR_INVAL && CATCPL_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATCPL_EDEVICE == pnp::post::ERR_DEVICE && CATCPL_MAX_NX == pnp::post::MAX_NX && CATCPL_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_couple.h and pnp_post.h disagree");
static_assert(CATCPL_WALL_DIRICHLET == pnp::team::WALL_DIRICHLET && CATCPL_WALL_STERN == pnp::team::WALL_STERN &&
                  CATCPL_PIVOT_GROWTH_LIMIT == pnp::team::PIVOT_GROWTH_LIMIT,
              "catint_couple.h and pnp_team.h disagree");

struct catcpl_ctx : pnp::post::Ctx {};

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
  if (const int rc = check_medium(ctx, entry, view, p)) return rc;
  if (!posfin(p->rf)) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: the roughness factor rf must be positive and finite");
  if (!std::isfinite(p->dphi_max)) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: dphi_max must be finite (<= 0: no limit)");
  if (const int rc = check_species(ctx, entry, p, N)) return rc;
  const int R = p->nreactions;
  if (const int rc = check_nreactions(ctx, entry, R)) return rc;
  if (const int rc = check_reactions(ctx, entry, p, N)) return rc;
  if (const int rc = check_lanes(ctx, entry, p, B)) return rc;
  const int64_t n = p->nlanes;
  if (n > 0 && (!p->flux || !p->K || !p->Kc || !p->Kphi)) return fail(ctx, CATCPL_EINVAL, "catcpl_solve: flux, K, Kc and Kphi are required");
  if (n == 0) return CATCPL_OK;

  KArgs a;
  memset(&a, 0, sizeof a);
  a.nx = nx; a.ldx = view->row_pitch; a.nreact = R; a.stern = p->wall_bc == CATCPL_WALL_STERN;
  a.nsys = n;
  a.c = view->c_dev; a.phi = view->phi_dev; a.st = view->status_dev;
  a.steric = fill_consts(a.k, p, N, a.stern);
  a.rf = p->rf;
  a.dphi_max = p->dphi_max;
  const int TPW = 64 / NB;
  const size_t nn = (size_t)n;

  // the inputs, staged on the host for one copy: edge weights, control volumes, row constants, the kinetic inputs, lanes (int64 in the
  // place of doubles), the flags of non-finite inputs (int32 pairs), the table
  Inputs in;
  const int i_grid = declare_grid(in, a, nx), i_g = in.add(nn * N, &a.g), i_K = in.add(nn * N, &a.K), i_Kc = in.add(nn * N * N, &a.Kc),
            i_Kp = in.add(nn * N, &a.Kphi), i_l = in.add_unpadded(nn, &a.lanes), i_b = in.add((nn + 1) / 2, &a.badin),
            i_t = in.add_unpadded(sizeof(Table) / 8, &a.tab);
  const size_t n_in = in.total;
  try {
    ctx->stage.assign(n_in, 0.0);
    ctx->flags.assign(nn, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATCPL_ENOMEM, "catcpl_solve: out of host memory");
  }
  stage_grid(in, ctx->stage, i_grid, p, nx, N);
  memcpy(in.host(ctx->stage, i_g), p->flux, nn * N * 8);
  memcpy(in.host(ctx->stage, i_K), p->K, nn * N * 8);
  memcpy(in.host(ctx->stage, i_Kc), p->Kc, nn * N * N * 8);
  memcpy(in.host(ctx->stage, i_Kp), p->Kphi, nn * N * 8);
  stage_lanes(in.host(ctx->stage, i_l), p);
  {
    int32_t* bi = reinterpret_cast<int32_t*>(in.host(ctx->stage, i_b));
    for (size_t i = 0; i < nn; ++i) {
      bool fin = true;
      for (int k = 0; k < N; ++k) fin = fin && std::isfinite(p->flux[i * N + k]) && std::isfinite(p->K[i * N + k]) && std::isfinite(p->Kphi[i * N + k]);
      for (int k = 0; k < N * N; ++k) fin = fin && std::isfinite(p->Kc[i * N * N + k]);
      bi[i] = fin ? 0 : 1;
    }
  }
  fill_reactions(reinterpret_cast<Table*>(in.host(ctx->stage, i_t)), p);

  // the rows that were asked for
  const Row rows[] = {{out->T_c, &a.Tc, nn * N * N}, {out->T_phi, &a.Tphi, nn * N}, {out->dflux, &a.dflux, nn * N}, {out->lambda, &a.lam, nn},
                      {out->flux_new, &a.fnew, nn * N}, {out->dc_surface, &a.dcs, nn * N}, {out->dphi_surface, &a.dphis, nn}};
  const size_t need_out = rows_doubles(rows), n_flags = even((nn + 1) / 2);
  if (!need_out && !out->status) return CATCPL_OK;

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  // persistent grid: as many waves as the device holds at once unless the caller sizes it, no more than there are groups of systems
  const int64_t groups = ((int64_t)n + TPW - 1) / TPW;
  int64_t blocks = 0;
  if (const int rc = persistent_waves(ctx, entry, p->max_waves, [&](int* per_cu) {
        return dispatch_nb(NB, [&](auto nb) { return resident<decltype(nb)::value>(per_cu); });
      }, groups, &blocks))
    return rc;
  if (const int rc = reserve(ctx, entry, n_in + need_out + n_flags)) return rc;
  in.place(ctx->buf);
  a.status = reinterpret_cast<int32_t*>(place_rows(rows, ctx->buf + n_in));
  if (const int rc = run_with_status(ctx, entry, st, n_in, rows, out->status, a.status, nn, [&] {
        return dispatch_nb(NB, [&](auto nb) { return launch<decltype(nb)::value>(a, blocks, st); });
      }))
    return rc;
  char msg[64];
  snprintf(msg, sizeof msg, "catcpl::couple_kernel<%d>", NB);
  ctx->last_kernel = msg;
  return CATCPL_OK;
}

}  // extern "C"
