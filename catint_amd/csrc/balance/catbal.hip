// libcatint_balance (include/catint_balance.h): species fluxes, reaction rates, wall terms and the discrete mass balance of the physical
// mode derived on the device from the state a pnp_handle holds there.  It shares no code with the Newton kernels (pnp_newton.hip,
// pnp_lane*.hip): the formulas are restated here from the header's definitions.  gfx950 / MI355X only.
//
// Layout and memory access: csrc/pnp_post.h, shared with observe/catobs.hip.  Persistent workgroups walk operating points b, b + grid,
// ...  Here every thread evaluates all P + 1 edges of its window (the balance of its last own point needs the edge to its right), and
// stores the P edges left of its points; when the grid is `tight` the last thread also stores the bulk point and the last edge.
// Passes per operating point: (0, steric ions only) phi0 -> w, gamma over the window; (A) one reaction at a time: the participants'
// windows are multiplied and the rate row is written -- to the output row when it was asked for, else to a workspace row of this
// workgroup -- with the sum of the absolute forward and backward terms next to it when the scalars are wanted; (B) one species at a
// time: edge fluxes from the windows of c_k and phi, the source from the rate rows the species takes part in, the imbalance, and the
// per-thread partial sums that wave scans (pnp_wave.h) and, with several waves, a few doubles of LDS turn into the scalars.
// A thread reads back from the rate rows only the positions it stored itself (its own points; the wall for thread 0; the bulk point
// for the last thread when tight), so pass B needs no barrier behind pass A.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../../include/catint_balance.h"
#include "../pnp_post.h"

namespace catbal {

using namespace pnp::post;

constexpr int MAXS = CATBAL_MAX_SPECIES, MAXR = PNP_MAX_REACTIONS, MAXT = PNP_MAX_REACTANTS, MAXW = PNP_MAX_WALL_REACTIONS;

// the reaction and wall tables of one call, flattened on the host (every index validated there)
struct Table {
  int32_t n_lhs[MAXR], n_rhs[MAXR];
  int32_t lhs[MAXR][MAXT], rhs[MAXR][MAXT];
  double kf[MAXR], kr[MAXR];
  int32_t nsp[MAXS];            // species k takes part in nsp[k] reactions: sp_r[k][e], with
  int32_t sp_r[MAXS][MAXR];
  double sp_net[MAXS][MAXR];    // n_rhs(k, r) - n_lhs(k, r)
  double sp_abs[MAXS][MAXR];    // n_rhs(k, r) + n_lhs(k, r)
  int32_t wspecies[MAXW], pad_[MAXW];
  double nu[MAXW][MAXS], alpha[MAXW], sat[MAXW];
};
static_assert(sizeof(Table) % 8 == 0, "the table is copied as doubles");

struct KArgs {
  int32_t N, nx, ldx, tight, nreact, nwall;
  int64_t B;
  const double* c;       // [B][N][ldx]
  const double* phi;     // [B][ldx]
  const double* x;       // [nx]
  const Table* tab;
  const double *kwall, *jpre, *phiM;   // [B][nwall], [B][N], [B]
  double *flux, *rate, *source, *wall_rate, *wall_flux, *imb, *scal;   // device rows; null: not wanted
  double* ws;            // [blocks][2][nreact][nx]: rate rows (unless `rate` takes them) and the rows of |forward| + |backward|
  double D[MAXS], qb[MAXS], pe[MAXS], vol[MAXS];   // D_k, q_k beta, velocity / D_k, N_A a_k^3
};

// the larger of two values that are >= 0 or NaN; a NaN wins
__device__ __forceinline__ double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

// sum / maximum (of values >= 0) over the 64 lanes, the same in every lane: the scan sequence of pnp::wave_scan_incl, read at lane 63
__device__ __forceinline__ double wave_sum(double v) { return pnp::read_lane(pnp::wave_scan_incl(v), 63); }
__device__ __forceinline__ double wave_max(double v) {
  v = max_nan(v, pnp::dpp_f64<0x111>(0.0, v));
  v = max_nan(v, pnp::dpp_f64<0x112>(0.0, v));
  v = max_nan(v, pnp::dpp_f64<0x114>(0.0, v));
  v = max_nan(v, pnp::dpp_f64<0x118>(0.0, v));
  v = max_nan(v, pnp::dpp_f64<0x142, 0xa>(0.0, v));
  v = max_nan(v, pnp::dpp_f64<0x143, 0xc>(0.0, v));
  return pnp::read_lane(v, 63);
}

// rate of wall reaction r at operating point b (wave-uniform: every lane evaluates it)
__device__ __forceinline__ double wall_rate_of(const KArgs& A, const Table& tb, int r, int64_t b, const double* crow, const double* prow) {
  const int s = tb.wspecies[r];
  const double cs = s >= 0 ? crow[(size_t)s * A.ldx] : 1.0;
  const double al = tb.alpha[r];
  const double E = al != 0.0 ? exp(al * (A.phiM[b] - prow[0])) : 1.0;
  return A.kwall[b * A.nwall + r] * (cs / (1.0 + tb.sat[r] * cs) * E);
}

template <int P, int WY, bool STERIC>
__global__ __launch_bounds__(64 * WY) void species_kernel(const KArgs A) {
  constexpr int T = 64 * WY;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nx = A.nx, N = A.N, R = A.nreact;
  const bool tight = A.tight != 0;
  const Table& tb = *A.tab;
  const bool want_src = A.source || A.imb || A.scal;
  const bool pass_b = A.flux || want_src;
  const bool pass_a = R > 0 && (A.rate || want_src);
  __shared__ double red[2][4][4];   // [parity of the species step][quantity][wave]: the waves' parts of the scalars

  // edge lengths of the window, formed once per wave: in registers, or (P >= 8) in a column of LDS per thread (conflict-free, read
  // back by this thread only: no barrier)
  constexpr bool HLDS = P >= 8;
  __shared__ double hl[HLDS ? (P + 1) * T : 1];
  double hr[P + 1];
  {
    double xw[P + 2];
    load_win<P>(pnp::row_rsrc(A.x, nx), xw, t);
#pragma unroll
    for (int j = 0; j <= P; ++j) {
      hr[j] = xw[j + 1] - xw[j];
      if constexpr (HLDS) hl[j * T + t] = hr[j];
    }
  }
  const auto h = [&](int j) { return HLDS ? hl[j * T + t] : hr[j]; };
  // the last edge nx - 2: edge je of thread te (an own edge, or edge P of the last thread when tight)
  const int te = min((nx - 2) / P, T - 1), je = nx - 2 - te * P;

  int par = 0;
  for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
    const double* crow = A.c + (size_t)b * N * A.ldx;
    const double* prow = A.phi + (size_t)b * A.ldx;
    double* rrow = A.rate ? A.rate + (size_t)b * R * nx : A.ws + (size_t)blockIdx.x * 2 * R * nx;
    double* arow = A.ws + ((size_t)blockIdx.x * 2 + 1) * R * nx;

    if (A.wall_rate) {
      for (int r = 0; r < A.nwall; ++r) {
        const double v = wall_rate_of(A, tb, r, b, crow, prow);
        if (t == 0) A.wall_rate[b * A.nwall + r] = v;
      }
    }

    // ---- pass 0: w = -ln(1 - phi0) and gamma = 1 / (1 - phi0) at the window positions (point ions: 0 and 1) ----------------------
    double w[P + 2], gam[P + 2];
#pragma unroll
    for (int jw = 0; jw < P + 2; ++jw) w[jw] = 0.0, gam[jw] = 1.0;
    if constexpr (STERIC) {
      if (pass_a || pass_b) {
        double vs[P + 2];
#pragma unroll
        for (int jw = 0; jw < P + 2; ++jw) vs[jw] = 0.0;
        for (int k = 0; k < N; ++k) {
          double cw[P + 2];
          load_win<P>(pnp::row_rsrc(crow + (size_t)k * A.ldx, nx), cw, t);
          const double vol = A.vol[k];
#pragma unroll
          for (int jw = 0; jw < P + 2; ++jw) vs[jw] = __builtin_fma(vol, cw[jw], vs[jw]);
        }
#pragma unroll
        for (int jw = 0; jw < P + 2; ++jw) {
          w[jw] = -pnp::log1p_sc(-vs[jw]);
          gam[jw] = 1.0 / (1.0 - vs[jw]);
        }
      }
    }

    // ---- pass A: one reaction at a time -------------------------------------------------------------------------------------------
    if (pass_a) {
      for (int r = 0; r < R; ++r) {
        double f[2][P + 2];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
          const double kk = side ? tb.kr[r] : tb.kf[r];
          const int m = side ? tb.n_rhs[r] : tb.n_lhs[r];
#pragma unroll
          for (int jw = 0; jw < P + 2; ++jw) f[side][jw] = kk;
          if (kk != 0.0) {   // a side whose rate constant is 0 contributes nothing, whatever its species hold
            for (int j = 0; j < m; ++j) {
              const int s = side ? tb.rhs[r][j] : tb.lhs[r][j];
              double cw[P + 2];
              load_win<P>(pnp::row_rsrc(crow + (size_t)s * A.ldx, nx), cw, t);
#pragma unroll
              for (int jw = 0; jw < P + 2; ++jw) f[side][jw] *= STERIC ? gam[jw] * cw[jw] : cw[jw];
            }
          }
        }
        double v[P + 2];
#pragma unroll
        for (int jw = 0; jw < P + 2; ++jw) v[jw] = f[0][jw] - f[1][jw];
        store_point_row<P, T>(rrow + (size_t)r * nx, v, nx, t, tight);
        if (A.scal) {
#pragma unroll
          for (int jw = 0; jw < P + 2; ++jw) v[jw] = fabs(f[0][jw]) + fabs(f[1][jw]);
          store_point_row<P, T>(arow + (size_t)r * nx, v, nx, t, tight);
        }
      }
    }

    // ---- pass B: one species at a time --------------------------------------------------------------------------------------------
    if (!pass_b && !A.wall_flux) continue;
    double pw[P + 2];
    load_win<P>(pnp::row_rsrc(prow, pass_b ? nx : 0), pw, t);
    for (int k = 0; k < N; ++k) {
      // the wall: prescribed flux and every wall reaction (wave-uniform)
      double wf = A.jpre[b * N + k], wfa = fabs(wf);
      for (int r = 0; r < A.nwall; ++r) {
        const double nu = tb.nu[r][k];
        if (nu != 0.0) {
          const double j = nu * wall_rate_of(A, tb, r, b, crow, prow);
          wf += j;
          wfa += fabs(j);
        }
      }
      if (A.wall_flux && t == 0) A.wall_flux[b * N + k] = wf;
      if (!pass_b) continue;

      double cw[P + 2];
      load_win<P>(pnp::row_rsrc(crow + (size_t)k * A.ldx, nx), cw, t);
      const double Dk = A.D[k], qbk = A.qb[k], pek = A.pe[k];
      double J[P + 1], Ja[P + 1];   // the edge flux and the sum of the absolute values of its two terms
#pragma unroll
      for (int j = 0; j <= P; ++j) {
        const double hj = h(j);
        const double u = __builtin_fma(qbk, pw[j + 1] - pw[j], w[j + 1] - w[j]) - pek * hj;
        const double Bp = bernoulli(u), Bm = Bp + u;
        const double dh = Dk * pnp::nrcp(hj), a = Bm * cw[j + 1], c = Bp * cw[j];
        J[j] = -dh * (a - c);
        Ja[j] = dh * (fabs(a) + fabs(c));
        // (keeps the scheduler from interleaving all P + 1 exponentials: their temporaries would not fit the register file)
        if constexpr (P >= 8) if (j % 2 == 1) __builtin_amdgcn_sched_barrier(0);
      }
      if (A.flux) store_edge_row<P, T>(A.flux + ((size_t)b * N + k) * (nx - 1), J, nx, t, tight);
      if (!want_src) continue;

      // the source at the window positions (valid where this thread stored the rate rows: see above) and its absolute terms
      double src[P + 2], sab[P + 2];
#pragma unroll
      for (int jw = 0; jw < P + 2; ++jw) src[jw] = 0.0, sab[jw] = 0.0;
      if (R > 0) {
        const int ne = tb.nsp[k];
        for (int e = 0; e < ne; ++e) {
          const int r = tb.sp_r[k][e];
          const double net = tb.sp_net[k][e], mult = tb.sp_abs[k][e];
          double rw[P + 2];
          load_win<P>(pnp::row_rsrc(rrow + (size_t)r * nx, nx), rw, t);
#pragma unroll
          for (int jw = 0; jw < P + 2; ++jw) src[jw] = __builtin_fma(net, rw[jw], src[jw]);
          if (A.scal) {
            load_win<P>(pnp::row_rsrc(arow + (size_t)r * nx, nx), rw, t);
#pragma unroll
            for (int jw = 0; jw < P + 2; ++jw) sab[jw] = __builtin_fma(mult, rw[jw], sab[jw]);
          }
        }
      }
      if (A.source) store_point_row<P, T>(A.source + ((size_t)b * N + k) * nx, src, nx, t, tight);

      // the imbalance, and this thread's part of the scalars: own points i = t P + jw, the wall (thread 0), the bulk point (its
      // owner, or the last thread when tight)
      double imb[P + 2];
      double s_src = 0.0, s_def = 0.0, s_inv = 0.0, s_max = 0.0;
      {
        const double V0 = 0.5 * h(0), rV = pnp::nrcp(V0);
        imb[0] = (wf - J[0]) * rV + src[0];
        if (t == 0) {
          const double scl = (wfa + Ja[0]) * rV + sab[0], a = fabs(imb[0]);
          s_src = V0 * src[0];
          s_def = V0 * imb[0];
          s_inv = V0 * cw[0];
          s_max = scl > 0.0 ? a * pnp::nrcp(scl) : (a != a ? a : 0.0);
        }
      }
#pragma unroll
      for (int jw = 1; jw <= P; ++jw) {
        const int i = t * P + jw;
        const bool inner = i < nx - 1, bulk = i == nx - 1;
        const double V = 0.5 * (h(jw - 1) + h(jw)), rV = pnp::nrcp(V);
        const double v = (J[jw - 1] - J[jw]) * rV + src[jw];
        const double scl = (Ja[jw - 1] + Ja[jw]) * rV + sab[jw], a = fabs(v);
        imb[jw] = inner ? v : 0.0;
        s_src += inner ? V * src[jw] : 0.0;
        s_def += inner ? V * v : 0.0;
        s_inv += inner ? V * cw[jw] : (bulk ? 0.5 * h(jw - 1) * cw[jw] : 0.0);
        s_max = inner ? max_nan(s_max, scl > 0.0 ? a * pnp::nrcp(scl) : (a != a ? a : 0.0)) : s_max;
      }
      imb[P + 1] = 0.0;
      if (tight && t == T - 1) s_inv += 0.5 * h(P) * cw[P + 1];
      if (A.imb) store_point_row<P, T>(A.imb + ((size_t)b * N + k) * nx, imb, nx, t, tight);

      if (A.scal) {
        double* sc = A.scal + ((size_t)b * N + k) * CATBAL_NSCALARS;
        double q0 = wave_sum(s_src), q1 = wave_sum(s_def), q2 = wave_sum(s_inv), q3 = wave_max(s_max);
        if constexpr (WY > 1) {
          if (lane == 0) {
            red[par][0][wave] = q0;
            red[par][1][wave] = q1;
            red[par][2][wave] = q2;
            red[par][3][wave] = q3;
          }
          pnp::wg_sync<WY>();
          q0 = red[par][0][0], q1 = red[par][1][0], q2 = red[par][2][0], q3 = red[par][3][0];
#pragma unroll
          for (int v = 1; v < WY; ++v) {
            q0 += red[par][0][v];
            q1 += red[par][1][v];
            q2 += red[par][2][v];
            q3 = max_nan(q3, red[par][3][v]);
          }
          par ^= 1;
        }
        if (t == 0) {
          sc[CATBAL_WALL_FLUX] = wf;
          sc[CATBAL_SOURCE_INTEGRAL] = q0;
          sc[CATBAL_DEFECT] = q1;
          sc[CATBAL_MAX_IMBALANCE_REL] = q3;
          sc[CATBAL_INVENTORY] = q2;
        }
        if (t == te) sc[CATBAL_BULK_FLUX] = pick(J, je);
      }
    }
  }
}

}  // namespace catbal

static_assert(CATBAL_OK == pnp::post::OK && CATBAL_EINVAL == pnp::post::ERR_INVAL && CATBAL_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATBAL_EDEVICE == pnp::post::ERR_DEVICE && CATBAL_MAX_NX == pnp::post::MAX_NX && CATBAL_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_balance.h and pnp_post.h disagree");

struct catbal_ctx : pnp::post::Ctx {};

extern "C" {

int catbal_create(int32_t device, catbal_ctx** out) { return pnp::post::create("catbal_create", device, out); }
void catbal_destroy(catbal_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catbal_last_error(const catbal_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catbal_last_kernel(const catbal_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catbal_last_kernel_ms(const catbal_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catbal_species(catbal_ctx* ctx, const pnp_device_view* view, const catbal_params* p, const catbal_outputs* out) {
  using namespace catbal;
  static const char entry[] = "catbal_species";
  if (const int rc = check_view(ctx, entry, "catbal_params", view, p, out)) return rc;
  const int N = view->nspecies, nx = view->nx;
  const int64_t B = view->batch;
  char msg[256];
  if (p->max_waves < 0) return fail(ctx, CATBAL_EINVAL, "catbal_species: negative max_waves");
  // what the kernel divides by or exponentiates: a zero, negative or non-finite value would fill rows with inf / NaN without an error
  // (catobs_electrolyte has no such checks)
  if (!(p->beta > 0.0) || !std::isfinite(p->beta) || !std::isfinite(p->velocity))
    return fail(ctx, CATBAL_EINVAL, "catbal_species: beta must be positive and finite, velocity finite");
  for (int k = 0; k < N; ++k) {
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    if (!(p->D[k] > 0.0) || !std::isfinite(p->D[k]) || !std::isfinite(p->charges[k]) || !(r >= 0.0) || !std::isfinite(r)) {
      snprintf(msg, sizeof msg, "catbal_species: species %d needs D > 0, a finite charge and a radius >= 0 (all finite)", k);
      return fail(ctx, CATBAL_EINVAL, msg);
    }
  }
  const int R = p->nreactions, W = p->n_wall;
  if (R < 0 || R > PNP_MAX_REACTIONS) {
    snprintf(msg, sizeof msg, "catbal_species: nreactions = %d outside [0, %d]", R, PNP_MAX_REACTIONS);
    return fail(ctx, CATBAL_EINVAL, msg);
  }
  if (W < 0 || W > PNP_MAX_WALL_REACTIONS) {
    snprintf(msg, sizeof msg, "catbal_species: n_wall = %d outside [0, %d]", W, PNP_MAX_WALL_REACTIONS);
    return fail(ctx, CATBAL_EINVAL, msg);
  }
  if (R > 0 && (!p->n_lhs || !p->lhs || !p->n_rhs || !p->rhs || !p->kf || !p->kr))
    return fail(ctx, CATBAL_EINVAL, "catbal_species: nreactions > 0 needs n_lhs, lhs, n_rhs, rhs, kf and kr");
  for (int r = 0; r < R; ++r) {
    if (p->n_lhs[r] < 0 || p->n_lhs[r] > PNP_MAX_REACTANTS || p->n_rhs[r] < 0 || p->n_rhs[r] > PNP_MAX_REACTANTS) {
      snprintf(msg, sizeof msg, "catbal_species: reaction %d has n_lhs / n_rhs outside [0, %d]", r, PNP_MAX_REACTANTS);
      return fail(ctx, CATBAL_EINVAL, msg);
    }
    for (int side = 0; side < 2; ++side)
      for (int j = 0; j < (side ? p->n_rhs[r] : p->n_lhs[r]); ++j) {
        const int s = (side ? p->rhs : p->lhs)[r * PNP_MAX_REACTANTS + j];
        if (s < 0 || s >= N) {
          snprintf(msg, sizeof msg, "catbal_species: reaction %d names species index %d outside [0, %d)", r, s, N);
          return fail(ctx, CATBAL_EINVAL, msg);
        }
      }
  }
  if (W > 0 && !p->k) return fail(ctx, CATBAL_EINVAL, "catbal_species: n_wall > 0 needs the rate constants k");
  if (W > 0 && (!p->species || !p->nu)) return fail(ctx, CATBAL_EINVAL, "catbal_species: n_wall > 0 needs species and nu");
  for (int r = 0; r < W; ++r)
    if (p->species[r] < -1 || p->species[r] >= N) {
      snprintf(msg, sizeof msg, "catbal_species: wall reaction %d names species index %d outside [-1, %d)", r, p->species[r], N);
      return fail(ctx, CATBAL_EINVAL, msg);
    }
  if (!p->flux || !p->phiM) return fail(ctx, CATBAL_EINVAL, "catbal_species: flux and phiM are required");

  KArgs a;
  memset(&a, 0, sizeof a);
  a.N = N; a.nx = nx; a.ldx = view->row_pitch; a.B = B; a.nreact = R; a.nwall = W;
  a.c = view->c_dev; a.phi = view->phi_dev;
  bool steric = false;
  for (int k = 0; k < N; ++k) {
    a.D[k] = p->D[k];
    a.qb[k] = p->charges[k] * p->beta;
    a.pe[k] = p->velocity / p->D[k];
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    a.vol[k] = pnp::N_AVOGADRO * r * r * r;
    steric = steric || a.vol[k] != 0.0;
  }
  int P = 1, WY = 1;
  choose_shape(nx, &P, &WY);
  a.tight = (nx - 2 == 64 * P * WY) ? 1 : 0;

  // the rows that were asked for (an empty row counts as not asked for)
  const size_t np = (size_t)B * N * nx, ne = (size_t)B * N * (nx - 1);
  const Row rows[] = {{out->flux, &a.flux, ne}, {out->reaction_rate, &a.rate, (size_t)B * R * nx}, {out->source, &a.source, np},
                      {out->wall_rate, &a.wall_rate, (size_t)B * W}, {out->wall_flux, &a.wall_flux, (size_t)B * N}, {out->imbalance, &a.imb, np},
                      {out->scalars, &a.scal, (size_t)B * N * CATBAL_NSCALARS}};
  const size_t need_out = rows_doubles(rows);
  if (!need_out) return CATBAL_OK;

  // persistent grid: 8 waves per CU on 256 CUs unless the caller sizes it; every workgroup walks b, b + grid, ...  A workgroup's rate
  // rows take 2 R nx doubles: the grid shrinks before that workspace passes 128 MiB
  const int waves = p->max_waves > 0 ? p->max_waves : 2048;
  int64_t blocks = waves / WY;
  if (blocks < 1) blocks = 1;
  if (blocks > B) blocks = B;
  const size_t ws_block = (size_t)2 * R * nx;
  while (blocks > 1 && (size_t)blocks * ws_block > ((size_t)16 << 20)) blocks /= 2;

  // the inputs, staged on the host for one copy: grid, prescribed flux, electrode potential, wall rate constants, tables
  Inputs in;
  const int i_x = in.add((size_t)nx, &a.x), i_j = in.add((size_t)B * N, &a.jpre), i_p = in.add((size_t)B, &a.phiM),
            i_k = in.add((size_t)B * W, &a.kwall), i_t = in.add_unpadded(sizeof(Table) / 8, &a.tab);
  const size_t n_in = in.total;
  try {
    ctx->stage.assign(n_in, 0.0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATBAL_ENOMEM, "catbal_species: out of host memory");
  }
  memcpy(in.host(ctx->stage, i_x), p->x, (size_t)nx * 8);
  memcpy(in.host(ctx->stage, i_j), p->flux, (size_t)B * N * 8);
  memcpy(in.host(ctx->stage, i_p), p->phiM, (size_t)B * 8);
  if (W) memcpy(in.host(ctx->stage, i_k), p->k, (size_t)B * W * 8);
  Table* tb = reinterpret_cast<Table*>(in.host(ctx->stage, i_t));
  for (int r = 0; r < R; ++r) {
    tb->n_lhs[r] = p->n_lhs[r];
    tb->n_rhs[r] = p->n_rhs[r];
    tb->kf[r] = p->kf[r];
    tb->kr[r] = p->kr[r];
    int cl[CATBAL_MAX_SPECIES] = {0}, cr[CATBAL_MAX_SPECIES] = {0};
    for (int j = 0; j < p->n_lhs[r]; ++j) ++cl[tb->lhs[r][j] = p->lhs[r * PNP_MAX_REACTANTS + j]];
    for (int j = 0; j < p->n_rhs[r]; ++j) ++cr[tb->rhs[r][j] = p->rhs[r * PNP_MAX_REACTANTS + j]];
    for (int k = 0; k < N; ++k)
      if (cl[k] + cr[k]) {
        const int e = tb->nsp[k]++;
        tb->sp_r[k][e] = r;
        tb->sp_net[k][e] = cr[k] - cl[k];
        tb->sp_abs[k][e] = cr[k] + cl[k];
      }
  }
  for (int r = 0; r < W; ++r) {
    tb->wspecies[r] = p->species[r];
    tb->alpha[r] = p->alpha ? p->alpha[r] : 0.0;
    tb->sat[r] = p->saturation ? p->saturation[r] : 0.0;
    for (int k = 0; k < N; ++k) tb->nu[r][k] = p->nu[r * N + k];
  }

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  if (const int rc = reserve(ctx, entry, n_in + need_out + even((size_t)blocks * ws_block))) return rc;
  in.place(ctx->buf);
  a.ws = place_rows(rows, ctx->buf + n_in);
  PNP_POST_HIP(hipMemcpyAsync(ctx->buf, ctx->stage.data(), n_in * sizeof(double), hipMemcpyHostToDevice, st));
  return run(ctx, entry, st, rows, "catbal::species_kernel", P, WY, steric, [&](auto p_, auto wy_, auto steric_) {
    hipLaunchKernelGGL((species_kernel<p_(), wy_(), steric_()>), dim3((int)blocks), dim3(64 * wy_()), 0, st, a);
  });
}

}  // extern "C"
