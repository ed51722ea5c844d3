// libcatint_sens (include/catint_sens.h): the sensitivities of a stationary state of the physical mode to its model parameters -- per
// operating point one block-tridiagonal solve J du = -dF/dp with as many right-hand sides as there are parameters -- formed on the
// device from the state a pnp_handle holds there.  It shares no code with the Newton kernels.  The rows of the stationary Jacobian,
// the team mapping, the walk from block row to block row and the host code around the launch are those of ../pnp_team.h (as for
// response/catresp.hip and couple/catcpl.hip; the Gauss-Jordan step stands in the row loop in the same words as there); here are the
// right-hand sides at every grid row, their carriage through the walk, the wall table and the scalars at the wall.
// gfx950 / MI355X only.
//
// Mapping (pnp_team.h): a TEAM of NB = N + 1 adjacent lanes per system; a system is one (operating point, chunk of PC parameters);
// persistent waves walk groups of systems.  Systems beyond the last one repeat a valid one: like the partial team they run every step
// and only skip their stores.
// Elimination: lane r owns row r of [D'_i | L_i | G_i], G_i the PC carried columns.  After the Gauss-Jordan of row i the carried columns
// hold y_i = D'_i^-1 g'_i; they go to the team through LDS next to T_i, and row i-1 forms g'_{i-1} = r_{i-1} - U_{i-1} y_i (point ions:
// the diagonal and the phi column of U, as subtract_UT).  The walk starts from y_{nx-1} = r_{nx-1}; at the wall the carried columns
// hold du_0.  Nothing is kept between block rows but row N of T_1 and of y_1 (the Dirichlet charge).
// A column's numbers are formed by operations on that column alone, in an order fixed in the source (no implicit contraction): they do
// not depend on its neighbours in the chunk, on its place, or on what else the call asks for.  The PHIM and WALL_FLUX columns undergo
// the operations catresp.hip performs on its single right-hand side.  Results leave through plain vector stores.
#include "../../../include/catint_sens.h"
#include "../pnp_team.h"

#pragma clang fp contract(off)

namespace catsens {

using namespace pnp::team;


using Table = pnp::team::WallTable;   // the reaction and wall tables of one call

struct KArgs {
  int32_t nx, ldx, nreact, nwall, stern, steric, P, nchunk;
  int64_t nsys;            // selected operating points x chunks
  const double* c;         // [B][N][ldx]
  const double* phi;       // [B][ldx]
  const int32_t* st;       // [B] solver status
  const int64_t* lanes;    // [n]
  const int32_t* badin;    // [n] 1: an input of the point is not finite
  const double *wgt, *vol; // [nx-1] dx / h_e, [nx] v_i
  const double* sp;        // [NB][SPF]
  const double* h;         // [nx-1] h_e
  const double *kwall, *phiM, *flux;   // [B][nwall], [B], [n][N]
  const int32_t* key;      // [nchunk][PC] key_of(kind, index) of every column; -1: a padding column
  const Table* tab;
  double *dphis, *dcs, *dsig, *dwf, *dcur;   // device rows; null: not wanted
  int32_t* flags;          // [nsys] status of every (point, chunk)
  Consts k;
  double CS, eps, h0, velocity, dx_eps, phi_pzc;   // C_S, eps, x[1] - x[0], velocity, dx / eps, phi_PZC
};

// a column's parameter in one number: the kind, and the index where the kind has one (species, reaction, wall reaction; else -1)
__host__ __device__ constexpr int key_of(int kind, int index) { return kind + 16 * (index + 1); }
static_assert(CATSENS_NKINDS <= 16, "key_of keeps the kind in four bits");

// g and dg/dc_s of wall reaction r at the wall state (cs: the driving concentration, 1 for species -1)
__device__ __forceinline__ void wall_law(const Table& tb, int r, double cs, double dphi, double& g, double& dg) {
  const double al = tb.alpha[r];
  const double den = 1.0 / (1.0 + tb.sat[r] * cs);
  const double E = al != 0.0 ? exp(al * dphi) : 1.0;
  g = cs * den * E;
  dg = den * den * E;
}

// Row r0 of r_i = -dF/dp at grid row i < nx-1 for the PC parameters of the chunk, from the window (centre C = point i) and the
// concentrations cc of the point: what the transport and the homogeneous reactions contribute.  The wall row's own terms are the
// caller's.  Operation by operation the order of tests/sens_ref.py.
template <int NB, int PC>
__device__ __forceinline__ void row_rhs(const KArgs& A, const Table& tb, const double* cc, const Lane& ln, const Window& w, int i,
                                        const int (&ky)[PC], double (&rv)[PC]) {
  const int r0 = ln.r0;
  const double vi = A.vol[i], hR = A.h[i], hL = i > 0 ? A.h[i - 1] : 0.0;
  const double D2 = ln.Dk * ln.Dk, rsv = ln.rs * vi;
#pragma unroll
  for (int m = 0; m < PC; ++m) rv[m] = 0.0;
  double Rk = 0.0;
  if (A.nreact > 0) {
    const double gam = 1.0 / w.C.gf;
    for (int r = 0; r < A.nreact; ++r) {
      const double net = tb.net[r][r0];
      double a[2];
#pragma unroll
      for (int sd = 0; sd < 2; ++sd) {
        const int ms = tb.n_side[sd][r];
        double prod = 1.0;
        for (int e = 0; e < ms; ++e) prod *= gam;
#pragma unroll
        for (int e = 0; e < MAXT; ++e) prod *= e < ms ? cc[tb.side[sd][r][e]] : 1.0;
        a[sd] = prod;
      }
      Rk = Rk + net * (tb.kk[0][r] * a[0] - tb.kk[1][r] * a[1]);
      const double rf = rsv * net * a[0], rb = -(rsv * net * a[1]);
#pragma unroll
      for (int m = 0; m < PC; ++m) {
        rv[m] = ky[m] == key_of(CATSENS_RATE_FORWARD, r) ? rf : rv[m];
        rv[m] = ky[m] == key_of(CATSENS_RATE_BACKWARD, r) ? rb : rv[m];
      }
    }
  }
  const double sR = A.velocity * hR / D2, sL = A.velocity * hL / D2;
  const double dterm = (-(w.eR.Ju * sR) + w.eL.Ju * sL) - ln.rs / ln.Dk * vi * Rk;
  const double vterm = (w.eR.Ju * hR - w.eL.Ju * hL) / ln.Dk;
#pragma unroll
  for (int m = 0; m < PC; ++m) {
    rv[m] = (!ln.isP && ky[m] == key_of(CATSENS_DIFFUSION, r0)) ? dterm : rv[m];
    rv[m] = (!ln.isP && ky[m] == key_of(CATSENS_VELOCITY, -1)) ? vterm : rv[m];
  }
}

// g'_{i-1} = r_{i-1} - U_{i-1} y_i, row r0, into G; ym: y_i of the team, whose row r0 the lane still holds in G
template <int NB, int PC>
__device__ __forceinline__ void carry(bool steric, const Lane& ln, const double (&ym)[NB][PC], const double (&Ur)[NB], const double (&rv)[PC],
                                      double (&G)[PC]) {
  constexpr int N = NB - 1;
  if (steric) {
#pragma unroll
    for (int m = 0; m < PC; ++m) {
      double g = rv[m];
#pragma unroll
      for (int s = 0; s < NB; ++s) g = fnma(g, Ur[s], ym[s][m]);
      G[m] = g;
    }
  } else {
    // point ions: U has its diagonal and the phi column
    double ud = 0.0;
#pragma unroll
    for (int s = 0; s < NB; ++s) ud = s == ln.r0 ? Ur[s] : ud;
    const double uN = ln.isP ? 0.0 : Ur[N];
#pragma unroll
    for (int m = 0; m < PC; ++m) {
      double g = fnma(rv[m], ud, G[m]);
      G[m] = fnma(g, uN, ym[N][m]);
    }
  }
}

template <int NB, int PC>
__global__ __launch_bounds__(64) void sens_kernel(const KArgs A) {
  constexpr int N = NB - 1, TPW = 64 / NB, W = 2 * NB + PC;
  const Lane ln = lane_of<NB>(A.sp);
  const int team = ln.team, r0 = ln.r0, base = ln.base;
  const bool isP = ln.isP;
  const int nx = A.nx;
  const Table& tb = *A.tab;

  __shared__ Ring<NB> ring;
  __shared__ double prow[2][TPW + 1][W];      // the pivot row of an elimination step (two buffers: one wave-level sync per step)
  __shared__ double tmat[TPW + 1][NB][NB];    // T_i
  __shared__ double ymat[TPW + 1][NB][PC];    // y_i; at the wall du_0
  __shared__ double wq[TPW + 1][NB][PC];      // the wall stage: dwall_flux of the team
  __shared__ double t1row[TPW + 1][NB];       // row N of T_1
  __shared__ double y1row[TPW + 1][PC];       // row N of y_1

  for (int64_t grp = blockIdx.x; grp * TPW < A.nsys; grp += gridDim.x) {
    const int64_t sys = grp * TPW + team;
    const bool live = team < TPW && sys < A.nsys;
    const int64_t sy = live ? sys : grp * TPW;
    const int64_t li = sy / A.nchunk;
    const int ch = (int)(sy - li * A.nchunk);
    const int64_t b = A.lanes[li];
    const double* urow = isP ? A.phi + (size_t)b * A.ldx : A.c + ((size_t)b * N + r0) * A.ldx;
    const double phiM = A.phiM[b];
    bool bad = false;

    int ky[PC];
#pragma unroll
    for (int m = 0; m < PC; ++m) ky[m] = A.key[ch * PC + m];

    Window w;
    double c4;
    open<NB>(A, ring, ln, urow, w, c4);

    double Aw[2 * NB];   // [D'_i | L_i], row r0
    double G[PC];        // the carried columns, row r0
    double Ur[NB];       // U_i, row r0
    double rv[PC];

    // the wall terms of row 0: the wall table's part of M_0, formed before the row ...
    const auto wall_matrix = [&](double (&wallM)[NB]) {
      const double* cc = ring[0] + base;
      for (int r = 0; r < A.nwall; ++r) {
        const int s = tb.wspecies[r];
        double g, dg;
        wall_law(tb, r, s >= 0 ? cc[s] : 1.0, phiM - w.C.ph, g, dg);
        const double nk = tb.nu[r][r0] * A.kwall[b * A.nwall + r];
#pragma unroll
        for (int j = 0; j < N; ++j) wallM[j] += j == s ? -nk * dg * ln.dx / ln.Dk : 0.0;
        wallM[N] += nk * tb.alpha[r] * g * ln.dx / ln.Dk;
      }
    };
    // ... and the wall row's own part of the right-hand sides, added to rv once the row stands
    const auto wall_rhs = [&]() {
      const int kq = isP ? N - 1 : r0;   // the Poisson lane reads a valid address and drops the value
      double wallj = A.flux[(size_t)li * N + kq];   // flux_k + sum_r nu[r][k] K_r g_r
      const double e0 = ln.dx / ln.Dk;
      double rphim = isP ? (A.stern ? -A.k.sternc : 1.0) : 0.0;
      double wr[PC];
#pragma unroll
      for (int m = 0; m < PC; ++m) wr[m] = 0.0;
      const double* cc = ring[0] + base;
      for (int r = 0; r < A.nwall; ++r) {
        const int s = tb.wspecies[r];
        double g, dg;
        wall_law(tb, r, s >= 0 ? cc[s] : 1.0, phiM - w.C.ph, g, dg);
        const double nk = tb.nu[r][r0] * A.kwall[b * A.nwall + r];
        rphim += nk * tb.alpha[r] * g * ln.dx / ln.Dk;
        wallj = wallj + nk * g;
        const double ng = tb.nu[r][r0] * g;
#pragma unroll
        for (int m = 0; m < PC; ++m) wr[m] = ky[m] == key_of(CATSENS_WALL_RATE, r) ? ng * ln.dx / ln.Dk : wr[m];
      }
      const double dwall = -(wallj * ln.dx / (ln.Dk * ln.Dk));
      const double rcs = -A.dx_eps * (phiM - A.phi_pzc - w.C.ph);
#pragma unroll
      for (int m = 0; m < PC; ++m) {
        wr[m] = ky[m] == key_of(CATSENS_PHIM, -1) ? rphim : wr[m];
        wr[m] = (!isP && ky[m] == key_of(CATSENS_WALL_FLUX, r0)) ? e0 : wr[m];
        wr[m] = (!isP && ky[m] == key_of(CATSENS_DIFFUSION, r0)) ? dwall : wr[m];
        wr[m] = (isP && ky[m] == key_of(CATSENS_STERN_CAPACITANCE, -1)) ? rcs : wr[m];
        // (CATSENS_DIFFUSION has a part from both; elsewhere one of the two is zero)
        rv[m] = rv[m] + wr[m];
      }
    };

    first_row<NB, double>(A, tb, ring, ln, w, c4, 0.0, Aw, Ur);
    // y_{nx-1} = r_{nx-1}: the identity rows of the bulk point
#pragma unroll
    for (int m = 0; m < PC; ++m) {
      G[m] = (!isP && ky[m] == key_of(CATSENS_BULK_CONCENTRATION, r0)) ? 1.0 : 0.0;
      ymat[team][r0][m] = G[m];
    }
    pnp::lds_sync();
    row_rhs<NB, PC>(A, tb, ring[(nx - 2) % 3] + base, ln, w, nx - 2, ky, rv);
    carry<NB, PC>(A.steric, ln, ymat[team], Ur, rv, G);

#pragma unroll 1
    for (int i = nx - 2; i >= 0; --i) {
      const double nxt = i >= 3 ? urow[i - 3] : 0.0;   // the point the row after next needs: used at the end of this block row
      // ---- Gauss-Jordan on [D' | L | G] across the team, no row exchanges ----
#pragma unroll
      for (int p = 0; p < NB; ++p) {
        const bool mine = r0 == p;
        const double piv = Aw[p];
        bad = bad || (mine && !(nonzero(piv) && finite_(piv)));
        const double ip = inv(piv);
        double* pr = prow[p & 1][team];
#pragma unroll
        for (int j = p + 1; j < 2 * NB; ++j) Aw[j] = sel(mine, mul(Aw[j], ip), Aw[j]);
#pragma unroll
        for (int m = 0; m < PC; ++m) G[m] = sel(mine, mul(G[m], ip), G[m]);
        if (mine) {
          pr[p] = piv;
#pragma unroll
          for (int j = p + 1; j < 2 * NB; ++j) pr[j] = Aw[j];
#pragma unroll
          for (int m = 0; m < PC; ++m) pr[2 * NB + m] = G[m];
        }
        pnp::lds_sync();
        // the pivot monitor: what partial pivoting would have checked -- an entry below the pivot beyond the growth limit times the pivot
        bad = bad || (r0 > p && abs2(piv) > GROWTH2 * abs2(pr[p]));
#pragma unroll
        for (int j = p + 1; j < 2 * NB; ++j) Aw[j] = sel(mine, Aw[j], fnma(Aw[j], piv, pr[j]));
#pragma unroll
        for (int m = 0; m < PC; ++m) G[m] = sel(mine, G[m], fnma(G[m], piv, pr[2 * NB + m]));
      }
      if (i == 0) break;
      // ---- T_i = Aw[NB ..], y_i = G: to the team ----
#pragma unroll
      for (int j = 0; j < NB; ++j) tmat[team][r0][j] = Aw[NB + j];
#pragma unroll
      for (int m = 0; m < PC; ++m) ymat[team][r0][m] = G[m];
      if (i == 1 && isP) {
#pragma unroll
        for (int j = 0; j < NB; ++j) t1row[team][j] = Aw[NB + j];
#pragma unroll
        for (int m = 0; m < PC; ++m) y1row[team][m] = G[m];
      }
      // ---- row i-1 ----
      shift(A, ln, i, w);
      double wallM[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) wallM[j] = 0.0;
      if (i == 1) wall_matrix(wallM);
      next_row<NB, double>(A, tb, ring, tmat[team], ln, w, i, nxt, 0.0, wallM, Aw, Ur);
      row_rhs<NB, PC>(A, tb, ring[(i - 1) % 3] + base, ln, w, i - 1, ky, rv);
      if (i == 1) wall_rhs();
      carry<NB, PC>(A.steric, ln, ymat[team], Ur, rv, G);
    }

    // ---- the wall: du_0[r0] of column m is G[m] ----
    pnp::lds_sync();   // the last elimination step has read its pivot row; y_1 has been read
#pragma unroll
    for (int m = 0; m < PC; ++m) {
      ymat[team][r0][m] = G[m];
      bad = bad || !finite_(G[m]);
    }
    pnp::lds_sync();
    const double* cc = ring[0] + base;
    const double ph0 = cc[N];
    double dph0[PC], drive[PC], dwf[PC];
#pragma unroll
    for (int m = 0; m < PC; ++m) {
      dph0[m] = ymat[team][N][m];
      drive[m] = (ky[m] == key_of(CATSENS_PHIM, -1) ? 1.0 : 0.0) - dph0[m];   // dphiM - du[phi, 0]
      dwf[m] = (!isP && ky[m] == key_of(CATSENS_WALL_FLUX, r0)) ? 1.0 : 0.0;   // the explicit part
    }
    for (int r = 0; r < A.nwall; ++r) {   // ... of a wall rate constant: nu[r][k] g_r
      const int s = tb.wspecies[r];
      double g, dg;
      wall_law(tb, r, s >= 0 ? cc[s] : 1.0, phiM - ph0, g, dg);
      const double ng = tb.nu[r][r0] * g;
#pragma unroll
      for (int m = 0; m < PC; ++m) dwf[m] = ky[m] == key_of(CATSENS_WALL_RATE, r) ? ng : dwf[m];
    }
    for (int r = 0; r < A.nwall; ++r) {
      const int s = tb.wspecies[r];
      double g, dg;
      wall_law(tb, r, s >= 0 ? cc[s] : 1.0, phiM - ph0, g, dg);
      const double nk = tb.nu[r][r0] * A.kwall[b * A.nwall + r];
      const double ag = tb.alpha[r] * g;
#pragma unroll
      for (int m = 0; m < PC; ++m) {
        const double dcs = s >= 0 ? ymat[team][s][m] : 0.0;
        dwf[m] = dwf[m] + nk * (dg * dcs + ag * drive[m]);
      }
    }
#pragma unroll
    for (int m = 0; m < PC; ++m) wq[team][r0][m] = dwf[m];
    pnp::lds_sync();
    double dsig[PC], dcur[PC];
#pragma unroll
    for (int m = 0; m < PC; ++m) {
      if (A.stern) {
        dsig[m] = A.CS * drive[m];
        if (ky[m] == key_of(CATSENS_STERN_CAPACITANCE, -1)) dsig[m] = dsig[m] + (phiM - A.phi_pzc - ph0);
      } else {
        // du[phi, 1] = y_1[phi] - (row N of T_1) du_0
        double d1 = y1row[team][m], qs = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) d1 = fnma(d1, t1row[team][j], ymat[team][j][m]);
#pragma unroll
        for (int j = 0; j < N; ++j) qs = qs + A.k.q[j] * ymat[team][j][m];
        dsig[m] = -A.eps / A.h0 * (d1 - dph0[m]) + -0.5 * A.h0 * qs;
      }
      double cur = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) cur = cur + A.k.q[j] * wq[team][j][m];
      dcur[m] = cur;
      bad = bad || !finite_(dwf[m]) || !finite_(dsig[m]) || !finite_(cur);
    }

    // ---- status of the system: any lane of the team ----
    pnp::lds_sync();
    ring[0][base + r0] = bad ? 1.0 : 0.0;
    pnp::lds_sync();
    const double anybad = team_sum<NB>(ring[0], ln);
    if (live) {
      const bool unsolved = A.st[b] != 0 || A.badin[li] != 0;
      const double nan = __builtin_nan("");
#pragma unroll
      for (int m = 0; m < PC; ++m) {
        const int pm = ch * PC + m;
        if (pm >= A.P) continue;
        const size_t o = (size_t)li * A.P + pm;
        if (isP) {
          if (A.dphis) A.dphis[o] = unsolved ? nan : dph0[m];
          if (A.dsig) A.dsig[o] = unsolved ? nan : dsig[m];
          if (A.dcur) A.dcur[o] = unsolved ? nan : dcur[m];
        } else {
          if (A.dcs) A.dcs[o * N + r0] = unsolved ? nan : G[m];
          if (A.dwf) A.dwf[o * N + r0] = unsolved ? nan : dwf[m];
        }
      }
      if (isP) A.flags[sys] = unsolved ? 2 : (anybad != 0.0 ? 1 : 0);
    }
    pnp::lds_sync();   // the ring and the exchange buffers are free for the next group
  }
}

template <int NB>
static hipError_t launch(const KArgs& a, int64_t blocks, hipStream_t st) {
  hipLaunchKernelGGL((sens_kernel<NB, CATSENS_CHUNK>), dim3((int)blocks), dim3(64), 0, st, a);
  return hipSuccess;
}

template <int NB>
static hipError_t resident(int* per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, sens_kernel<NB, CATSENS_CHUNK>, 64, 0);
}

}  // namespace catsens

static_assert(CATSENS_OK == pnp::post::OK && CATSENS_EINVAL == pnp::post::ERR_INVAL && CATSENS_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATSENS_EDEVICE == pnp::post::ERR_DEVICE && CATSENS_MAX_NX == pnp::post::MAX_NX && CATSENS_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_sens.h and pnp_post.h disagree");
static_assert(CATSENS_WALL_DIRICHLET == pnp::team::WALL_DIRICHLET && CATSENS_WALL_STERN == pnp::team::WALL_STERN &&
                  CATSENS_PIVOT_GROWTH_LIMIT == pnp::team::PIVOT_GROWTH_LIMIT,
              "catint_sens.h and pnp_team.h disagree");

struct catsens_ctx : pnp::post::Ctx {
  std::vector<int32_t> chunk_flags;   // host: status of every (point, chunk)
};

extern "C" {

int catsens_create(int32_t device, catsens_ctx** out) { return pnp::post::create("catsens_create", device, out); }
void catsens_destroy(catsens_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catsens_last_error(const catsens_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catsens_last_kernel(const catsens_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catsens_last_kernel_ms(const catsens_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catsens_solve(catsens_ctx* ctx, const pnp_device_view* view, const catsens_params* p, const catsens_outputs* out) {
  using namespace catsens;
  static const char entry[] = "catsens_solve";
  constexpr int PC = CATSENS_CHUNK;
  if (const int rc = check_view(ctx, entry, "catsens_params", view, p, out)) return rc;
  if (out->struct_size != (int32_t)sizeof(catsens_outputs))
    return fail(ctx, CATSENS_EINVAL, "catsens_solve: catsens_outputs.struct_size does not match this library");
  const int N = view->nspecies, nx = view->nx, NB = N + 1;
  const int64_t B = view->batch;
  char msg[256];
  if (const int rc = check_medium(ctx, entry, view, p)) return rc;
  if (!std::isfinite(p->phi_pzc)) return fail(ctx, CATSENS_EINVAL, "catsens_solve: phi_pzc must be finite");
  if (const int rc = check_species(ctx, entry, p, N)) return rc;
  const int R = p->nreactions, W = p->n_wall, P = p->nparams;
  if (const int rc = check_nreactions(ctx, entry, R)) return rc;
  if (const int rc = check_nwall(ctx, entry, W)) return rc;
  if (const int rc = check_reactions(ctx, entry, p, N)) return rc;
  if (const int rc = check_wall(ctx, entry, p, N)) return rc;
  if (!p->phiM) return fail(ctx, CATSENS_EINVAL, "catsens_solve: phiM is required");
  if (P < 1 || P > CATSENS_MAX_PARAMS) {
    snprintf(msg, sizeof msg, "catsens_solve: nparams = %d outside [1, %d]", P, CATSENS_MAX_PARAMS);
    return fail(ctx, CATSENS_EINVAL, msg);
  }
  if (!p->kind || !p->index) return fail(ctx, CATSENS_EINVAL, "catsens_solve: kind and index are required");
  for (int m = 0; m < P; ++m) {
    const int kd = p->kind[m], ix = p->index[m];
    int lim = -1;   // -1: the kind has no index
    const char* what = "";
    switch (kd) {
      case CATSENS_PHIM: case CATSENS_VELOCITY: break;
      case CATSENS_STERN_CAPACITANCE:
        if (p->wall_bc != CATSENS_WALL_STERN) {
          snprintf(msg, sizeof msg, "catsens_solve: parameter %d is the Stern capacitance, but the wall is a Dirichlet wall", m);
          return fail(ctx, CATSENS_EINVAL, msg);
        }
        break;
      case CATSENS_WALL_FLUX: case CATSENS_BULK_CONCENTRATION: case CATSENS_DIFFUSION: lim = N, what = "species"; break;
      case CATSENS_RATE_FORWARD: case CATSENS_RATE_BACKWARD: lim = R, what = "reaction"; break;
      case CATSENS_WALL_RATE: lim = W, what = "wall reaction"; break;
      default:
        snprintf(msg, sizeof msg, "catsens_solve: parameter %d has the unknown kind %d", m, kd);
        return fail(ctx, CATSENS_EINVAL, msg);
    }
    if (lim >= 0 && (ix < 0 || ix >= lim)) {
      snprintf(msg, sizeof msg, "catsens_solve: parameter %d names %s index %d outside [0, %d)", m, what, ix, lim);
      return fail(ctx, CATSENS_EINVAL, msg);
    }
  }
  if (const int rc = check_lanes(ctx, entry, p, B)) return rc;
  const int64_t n = p->nlanes;
  if (n > 0 && !p->flux) return fail(ctx, CATSENS_EINVAL, "catsens_solve: flux is required");
  if (n == 0) return CATSENS_OK;

  const int nchunk = (P + PC - 1) / PC;
  KArgs a;
  memset(&a, 0, sizeof a);
  a.nx = nx; a.ldx = view->row_pitch; a.nreact = R; a.nwall = W; a.stern = p->wall_bc == CATSENS_WALL_STERN;
  a.P = P; a.nchunk = nchunk; a.nsys = n * nchunk;
  a.c = view->c_dev; a.phi = view->phi_dev; a.st = view->status_dev;
  a.steric = fill_consts(a.k, p, N, a.stern);
  a.CS = a.stern ? p->stern_capacitance : 0.0;
  a.eps = p->eps;
  a.h0 = p->x[1] - p->x[0];
  a.velocity = p->velocity;
  a.dx_eps = p->dx / p->eps;
  a.phi_pzc = p->phi_pzc;
  const int TPW = 64 / NB;
  const size_t nn = (size_t)n, nsys = nn * nchunk, ncol = (size_t)nchunk * PC;

  // the inputs, staged on the host for one copy: edge weights, control volumes, row constants, edge lengths, potentials, rate
  // constants, fluxes, lanes (int64 in the place of doubles), the flags of non-finite inputs and the columns' keys (int32 pairs), tables
  Inputs in;
  const int i_grid = declare_grid(in, a, nx), i_h = in.add((size_t)nx - 1, &a.h), i_p = in.add((size_t)B, &a.phiM),
            i_k = in.add((size_t)B * W, &a.kwall), i_g = in.add(nn * N, &a.flux), i_l = in.add_unpadded(nn, &a.lanes),
            i_b = in.add((nn + 1) / 2, &a.badin), i_ky = in.add_unpadded(ncol / 2, &a.key), i_t = in.add_unpadded(sizeof(Table) / 8, &a.tab);
  const size_t n_in = in.total;
  try {
    ctx->stage.assign(n_in, 0.0);
    ctx->flags.assign(nsys, 0);
    ctx->chunk_flags.assign(nsys, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATSENS_ENOMEM, "catsens_solve: out of host memory");
  }
  stage_grid(in, ctx->stage, i_grid, p, nx, N);
  double* h = in.host(ctx->stage, i_h);
  for (int e = 0; e < nx - 1; ++e) h[e] = p->x[e + 1] - p->x[e];
  memcpy(in.host(ctx->stage, i_p), p->phiM, (size_t)B * 8);
  if (W) memcpy(in.host(ctx->stage, i_k), p->k, (size_t)B * W * 8);
  memcpy(in.host(ctx->stage, i_g), p->flux, nn * N * 8);
  stage_lanes(in.host(ctx->stage, i_l), p);
  {
    int32_t* bi = reinterpret_cast<int32_t*>(in.host(ctx->stage, i_b));
    for (size_t i = 0; i < nn; ++i) {
      const int64_t b = p->lanes ? p->lanes[i] : (int64_t)i;
      bool fin = std::isfinite(p->phiM[b]);
      for (int k = 0; k < N; ++k) fin = fin && std::isfinite(p->flux[i * N + k]);
      for (int r = 0; r < W; ++r) fin = fin && std::isfinite(p->k[b * W + r]);
      bi[i] = fin ? 0 : 1;
    }
    int32_t* ky = reinterpret_cast<int32_t*>(in.host(ctx->stage, i_ky));
    for (size_t m = 0; m < ncol; ++m) {
      const int kd = m < (size_t)P ? p->kind[m] : -1;
      const bool indexed = kd != CATSENS_PHIM && kd != CATSENS_VELOCITY && kd != CATSENS_STERN_CAPACITANCE;
      ky[m] = kd < 0 ? -1 : key_of(kd, indexed ? p->index[m] : -1);
    }
  }
  Table* tb = reinterpret_cast<Table*>(in.host(ctx->stage, i_t));
  fill_reactions(tb, p);
  fill_wall(tb, p, N);

  // the rows that were asked for
  const size_t np = nn * P;
  const Row rows[] = {{out->dphi_surface, &a.dphis, np}, {out->dc_surface, &a.dcs, np * N}, {out->dsigma, &a.dsig, np},
                      {out->dwall_flux, &a.dwf, np * N}, {out->dcurrent, &a.dcur, np}};
  const size_t need_out = rows_doubles(rows), n_flags = even((nsys + 1) / 2);
  if (!need_out && !out->status) return CATSENS_OK;

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  // persistent grid: as many waves as the device holds at once unless the caller sizes it, no more than there are groups of systems
  const int64_t groups = ((int64_t)nsys + TPW - 1) / TPW;
  int64_t blocks = 0;
  if (const int rc = persistent_waves(ctx, entry, p->max_waves, [&](int* per_cu) {
        return dispatch_nb(NB, [&](auto nb) { return resident<decltype(nb)::value>(per_cu); });
      }, groups, &blocks))
    return rc;
  if (const int rc = reserve(ctx, entry, n_in + need_out + n_flags)) return rc;
  in.place(ctx->buf);
  a.flags = reinterpret_cast<int32_t*>(place_rows(rows, ctx->buf + n_in));
  if (const int rc = run_with_status(ctx, entry, st, n_in, rows, out->status ? ctx->chunk_flags.data() : nullptr, a.flags, nsys, [&] {
        return dispatch_nb(NB, [&](auto nb) { return launch<decltype(nb)::value>(a, blocks, st); });
      }))
    return rc;
  if (out->status)
    for (size_t i = 0; i < nn; ++i) {
      int32_t s = 0;   // 2 goes before 1
      for (int c = 0; c < nchunk; ++c) s = std::max(s, ctx->chunk_flags[i * nchunk + c]);
      out->status[i] = s;
    }
  snprintf(msg, sizeof msg, "catsens::sens_kernel<%d, %d>", NB, PC);
  ctx->last_kernel = msg;
  return CATSENS_OK;
}

}  // extern "C"
