// libcatint_observe (include/catint_observe.h): electrolyte observables of the physical mode derived on the device from the state a
// pnp_handle holds there.  One pass over the state: every operating point is one workgroup iteration, the species rows are summed
// in registers, the two potential drops are prefix sums over the edges.  gfx950 / MI355X only.
//
// Layout and memory access: csrc/pnp_post.h.  Here, when the grid is `tight`, every thread also evaluates window position P + 1 and
// edge P, and the last thread stores them.  Point ions: every input row is read once.  Steric ions: w = -ln(1 - phi0) is needed at
// both ends of an edge before any species flux, so the species rows are read twice (the second time from L2).
#include <cstring>

#include "../../../include/catint_observe.h"
#include "../pnp_post.h"

namespace catobs {

using namespace pnp::post;

struct KArgs {
  int32_t N, nx, ldx, sH, sOH, tight;
  int64_t B;
  const double* c;     // [B][N][ldx]
  const double* phi;   // [B][ldx]
  const double* x;     // [nx]
  double *efield, *rho, *gamma, *pH, *kappa, *iel, *diR, *ddf, *scal;   // device rows, [B][nx] / [B][nx-1] / [B][NSCALARS]; null: not wanted
  double D[CATOBS_MAX_SPECIES], q[CATOBS_MAX_SPECIES], qb[CATOBS_MAX_SPECIES];   // D_k, q_k, q_k beta
  double pe[CATOBS_MAX_SPECIES], kz[CATOBS_MAX_SPECIES], vol[CATOBS_MAX_SPECIES];   // velocity / D_k, beta q_k^2 D_k, N_A a_k^3
};

template <int P, int WY, bool STERIC>
__global__ __launch_bounds__(64 * WY) void electrolyte_kernel(const KArgs A) {
  constexpr int T = 64 * WY;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nx = A.nx, N = A.N;
  const bool tight = A.tight != 0;
  const bool want_edges = A.kappa || A.iel || A.diR || A.ddf || A.scal;
  const bool want_pH = A.pH || A.scal;
  __shared__ double tot[2][2][4];   // [parity of the iteration][scan][wave]: inclusive totals of the waves of one operating point

  // the grid is the same for every operating point: the edge lengths are formed once per wave and kept for its life -- in registers,
  // or (P >= 8, where the accumulators alone fill the register file) in a column of LDS per thread, which is conflict-free.  Their
  // reciprocals are formed where they are used: v_rcp_f64 and two Newton steps cost less than the registers would.
  constexpr bool HLDS = P >= 8;
  __shared__ double hl[HLDS ? (P + 1) * T : 1];
  double hr[P + 1];
  {
    double xw[P + 2];
    load_win<P>(pnp::row_rsrc(A.x, nx), xw, t);
#pragma unroll
    for (int j = 0; j <= P; ++j) {
      hr[j] = xw[j + 1] - xw[j];
      if constexpr (HLDS) hl[j * T + t] = hr[j];   // read back by this thread only: no barrier
    }
  }
  const auto h = [&](int j) { return HLDS ? hl[j * T + t] : hr[j]; };
  // the species whose concentration gives the pH is summed last, so that its window is still in registers when the pH is formed
  const int sPH = A.sH >= 0 ? A.sH : A.sOH;
  // the bulk point: window position posb of thread tb (an own position, or P + 1 of the last thread when tight)
  const int tb = min((nx - 2) / P, T - 1), posb = nx - 1 - tb * P;

  int par = 0;
  for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x, par ^= 1) {
    const double* crow = A.c + (size_t)b * N * A.ldx;
    const double* prow = A.phi + (size_t)b * A.ldx;
    double pw[P + 2];
    load_win<P>(pnp::row_rsrc(prow, nx), pw, t);
    double cw[P + 2];
    // w = -ln(1 - phi0) at the window positions (point ions: 0); gamma = 1 / (1 - phi0) goes out as soon as it is known, and
    // log10 gamma = w / ln 10 serves the pH
    double w[P + 2], gam0 = 1.0;
#pragma unroll
    for (int jw = 0; jw < P + 2; ++jw) w[jw] = 0.0;
    if constexpr (STERIC) {
      double vs[P + 2];
#pragma unroll
      for (int jw = 0; jw < P + 2; ++jw) vs[jw] = 0.0;
      load_win<P>(pnp::row_rsrc(crow, nx), cw, t);
      for (int k = 0; k < N; ++k) {
        double nw[P + 2];
        load_win<P>(pnp::row_rsrc(crow + (size_t)(k + 1) * A.ldx, k + 1 < N ? nx : 0), nw, t);
        const double vol = A.vol[k];
#pragma unroll
        for (int jw = 0; jw < P + 2; ++jw) {
          vs[jw] = __builtin_fma(vol, cw[jw], vs[jw]);
          cw[jw] = nw[jw];
        }
      }
      double gam[P + 2];
#pragma unroll
      for (int jw = 0; jw < P + 2; ++jw) {
        w[jw] = -pnp::log1p_sc(-vs[jw]);
        gam[jw] = 1.0 / (1.0 - vs[jw]);
      }
      gam0 = gam[0];
      if (A.gamma) store_point_row<P, T>(A.gamma + (size_t)b * nx, gam, nx, t, tight);
    } else if (A.gamma) {
      double gam[P + 2];
#pragma unroll
      for (int jw = 0; jw < P + 2; ++jw) gam[jw] = 1.0;
      store_point_row<P, T>(A.gamma + (size_t)b * nx, gam, nx, t, tight);
    }

    // iel / idf hold sum_k q_k D_k (...) until the loop is over: the factor -1 / h_e is common to the species
    double rho[P + 2], kap[P + 1], iel[P + 1], idf[P + 1];
#pragma unroll
    for (int jw = 0; jw < P + 2; ++jw) rho[jw] = 0.0;
#pragma unroll
    for (int j = 0; j <= P; ++j) kap[j] = 0.0, iel[j] = 0.0, idf[j] = 0.0;

    // step s of the loop takes species s, except that species sPH changes places with the last one
    const auto species_of = [&](int s) { return sPH < 0 ? s : (s < sPH ? s : (s < N - 1 ? s + 1 : sPH)); };
    load_win<P>(pnp::row_rsrc(crow + (size_t)species_of(0) * A.ldx, nx), cw, t);
    for (int s = 0; s < N; ++s) {
      const int k = species_of(s);
      double nw[P + 2];   // the next species' window is on its way while this one is summed (after the last: an empty resource, zeros)
      load_win<P>(pnp::row_rsrc(crow + (size_t)species_of(s + 1 < N ? s + 1 : s) * A.ldx, s + 1 < N ? nx : 0), nw, t);
      const double qk = A.q[k], qDk = A.q[k] * A.D[k], qbk = A.qb[k], pek = A.pe[k], kzk = A.kz[k];
#pragma unroll
      for (int jw = 0; jw < P + 2; ++jw) rho[jw] = __builtin_fma(qk, cw[jw], rho[jw]);
      if (want_edges) {
#pragma unroll
        for (int j = 0; j <= P; ++j) {
          if (j < P || tight) {
            const double cl = cw[j], cr = cw[j + 1];
            const double u = __builtin_fma(qbk, pw[j + 1] - pw[j], w[j + 1] - w[j]) - pek * h(j);
            const double Bp = bernoulli(u), Bm = Bp + u;
            iel[j] = __builtin_fma(qDk, Bm * cr - Bp * cl, iel[j]);
            idf[j] = __builtin_fma(qDk, cr - cl, idf[j]);
            kap[j] = __builtin_fma(kzk, 0.5 * (cl + cr), kap[j]);
          }
          // (keeps the scheduler from interleaving all P + 1 exponentials: their temporaries would not fit the register file)
          if constexpr (P >= 8) if (j % 2 == 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (s + 1 < N) {
#pragma unroll
        for (int jw = 0; jw < P + 2; ++jw) cw[jw] = nw[jw];
      }
    }
    if (want_edges) {
#pragma unroll
      for (int j = 0; j <= P; ++j) {
        const double mrh = -pnp::nrcp(h(j));
        iel[j] *= mrh;
        idf[j] *= mrh;
      }
    }

    // ---- point rows ----------------------------------------------------------------------------------------------------------
    double ef[P + 2];
    ef[0] = -(pw[1] - pw[0]) * pnp::nrcp(h(0));               // one-sided at the wall (thread 0 stores it)
    ef[P + 1] = -(pw[P + 1] - pw[P]) * pnp::nrcp(h(P));       // ... and at the bulk point without an owner (tight)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const bool bulk = (t * P + 1 + j == nx - 1);
      const double num = bulk ? pw[j + 1] - pw[j] : pw[j + 2] - pw[j];
      const double den = bulk ? h(j) : h(j) + h(j + 1);
      ef[j + 1] = -num * pnp::nrcp(den);
    }
    double pH[P + 2];
    if (want_pH) {
#pragma unroll
      for (int jw = 0; jw < P + 2; ++jw) {
        const double l = log10(cw[jw] * 1e-3);      // cw: the window of species sPH
        pH[jw] = (A.sH >= 0 ? -l : (A.sOH >= 0 ? 14.0 + l : __builtin_nan("")));
        if constexpr (STERIC) pH[jw] -= w[jw] * 0.43429448190325182765;   // log10 gamma = w / ln 10
      }
    }
    if (A.efield) store_point_row<P, T>(A.efield + (size_t)b * nx, ef, nx, t, tight);
    if (A.rho) store_point_row<P, T>(A.rho + (size_t)b * nx, rho, nx, t, tight);
    if (A.pH) store_point_row<P, T>(A.pH + (size_t)b * nx, pH, nx, t, tight);

    if (want_edges) {
      // ---- the two prefix sums over the edges, together: in the thread, across the wave (DPP), across the waves (LDS) ----------
      double s1[P + 2], s2[P + 2];   // values at the window positions: s[jw] = sum over the edges left of position jw
      double a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int j = 0; j <= P; ++j) {
        const bool on = kap[j] > 0.0 && (t * P + j <= nx - 2) && (j < P || tight);
        const double rk = pnp::nrcp(kap[j]);
        const double hj = h(j);
        a1 += on ? -(iel[j] * rk) * hj : 0.0;
        a2 += on ? (idf[j] * rk) * hj : 0.0;
        s1[j + 1] = a1;
        s2[j + 1] = a2;
      }
      const double in1 = pnp::wave_scan_incl(s1[P]), in2 = pnp::wave_scan_incl(s2[P]);   // own edges 0 .. P - 1 of every thread
      double base1 = pnp::from_prev_lane(0.0, in1), base2 = pnp::from_prev_lane(0.0, in2);
      if constexpr (WY > 1) {
        if (lane == 63) {
          tot[par][0][wave] = in1;
          tot[par][1][wave] = in2;
        }
        pnp::wg_sync<WY>();
#pragma unroll
        for (int w = 0; w < WY - 1; ++w) {
          base1 += (w < wave) ? tot[par][0][w] : 0.0;
          base2 += (w < wave) ? tot[par][1][w] : 0.0;
        }
      }
      s1[0] = base1;
      s2[0] = base2;
#pragma unroll
      for (int jw = 1; jw < P + 2; ++jw) {
        s1[jw] += base1;
        s2[jw] += base2;
      }
      if (A.kappa) store_edge_row<P, T>(A.kappa + (size_t)b * (nx - 1), kap, nx, t, tight);
      if (A.iel) store_edge_row<P, T>(A.iel + (size_t)b * (nx - 1), iel, nx, t, tight);
      if (A.diR) store_point_row<P, T>(A.diR + (size_t)b * nx, s1, nx, t, tight);
      if (A.ddf) store_point_row<P, T>(A.ddf + (size_t)b * nx, s2, nx, t, tight);
      if (A.scal) {
        double* sc = A.scal + (size_t)b * CATOBS_NSCALARS;
        if (t == 0) {
          sc[CATOBS_SURFACE_POTENTIAL] = pw[0];
          sc[CATOBS_SURFACE_EFIELD] = ef[0];
          sc[CATOBS_SURFACE_GAMMA] = gam0;
          sc[CATOBS_SURFACE_PH] = pH[0];
          sc[CATOBS_WALL_CURRENT_DENSITY] = iel[0];
        }
        if (t == tb) {
          const double iR = pick(s1, posb), dphi_inf = pick(pw, posb) - prow[0];
          sc[CATOBS_DELTA_PHI_IR_INF] = iR;
          sc[CATOBS_DELTA_PHI_DIFF_INF] = pick(s2, posb);
          sc[CATOBS_DELTA_PHI_INF] = dphi_inf;
          sc[CATOBS_DELTA_PHI_INF_MIN_IR] = dphi_inf - iR;
          sc[CATOBS_BULK_CONDUCTIVITY] = pick(kap, posb - 1);
        }
      }
    }
  }
}

}  // namespace catobs

static_assert(CATOBS_OK == pnp::post::OK && CATOBS_EINVAL == pnp::post::ERR_INVAL && CATOBS_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATOBS_EDEVICE == pnp::post::ERR_DEVICE && CATOBS_MAX_NX == pnp::post::MAX_NX && CATOBS_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_observe.h and pnp_post.h disagree");

struct catobs_ctx : pnp::post::Ctx {};

extern "C" {

int catobs_create(int32_t device, catobs_ctx** out) { return pnp::post::create("catobs_create", device, out); }
void catobs_destroy(catobs_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catobs_last_error(const catobs_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catobs_last_kernel(const catobs_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catobs_last_kernel_ms(const catobs_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catobs_electrolyte(catobs_ctx* ctx, const pnp_device_view* view, const catobs_params* p, const catobs_outputs* out) {
  using namespace catobs;
  static const char entry[] = "catobs_electrolyte";
  if (const int rc = check_view(ctx, entry, "catobs_params", view, p, out)) return rc;
  const int N = view->nspecies, nx = view->nx;
  const int64_t B = view->batch;
  // (catbal_species goes on to check that beta, D, the charges and the radii are finite and in range; this entry point does not)
  if (p->species_H < -1 || p->species_H >= N || p->species_OH < -1 || p->species_OH >= N)
    return fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: species_H / species_OH outside [-1, N)");
  if (p->max_waves < 0) return fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: negative max_waves");

  KArgs a;
  memset(&a, 0, sizeof a);
  a.N = N; a.nx = nx; a.ldx = view->row_pitch; a.sH = p->species_H; a.sOH = p->species_OH; a.B = B;
  a.c = view->c_dev; a.phi = view->phi_dev;
  bool steric = false;
  for (int k = 0; k < N; ++k) {
    a.D[k] = p->D[k];
    a.q[k] = p->charges[k];
    a.qb[k] = p->charges[k] * p->beta;
    a.pe[k] = p->velocity / p->D[k];
    a.kz[k] = p->beta * p->charges[k] * p->charges[k] * p->D[k];
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    a.vol[k] = pnp::N_AVOGADRO * r * r * r;
    steric = steric || a.vol[k] != 0.0;
  }
  int P = 1, WY = 1;
  choose_shape(nx, &P, &WY);
  a.tight = (nx - 2 == 64 * P * WY) ? 1 : 0;

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  // one device buffer: the grid (padded to an even count), then the rows that were asked for (none of them is empty for a valid view)
  const size_t np = (size_t)B * nx, ne = (size_t)B * (nx - 1);
  const Row rows[] = {{out->efield, &a.efield, np}, {out->charge_density, &a.rho, np}, {out->gamma, &a.gamma, np}, {out->pH, &a.pH, np},
                      {out->conductivity, &a.kappa, ne}, {out->current_density, &a.iel, ne}, {out->dphi_iR, &a.diR, np},
                      {out->dphi_diff, &a.ddf, np}, {out->scalars, &a.scal, (size_t)B * CATOBS_NSCALARS}};
  const size_t need_out = rows_doubles(rows);
  if (!need_out) return CATOBS_OK;
  if (const int rc = reserve(ctx, entry, even(nx) + need_out)) return rc;
  a.x = ctx->buf;
  place_rows(rows, ctx->buf + even(nx));
  PNP_POST_HIP(hipMemcpyAsync(ctx->buf, p->x, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, st));
  // persistent grid: 8 waves per CU on 256 CUs unless the caller sizes it; every workgroup walks b, b + grid, ...
  const int waves = p->max_waves > 0 ? p->max_waves : 2048;
  int64_t blocks = waves / WY;
  if (blocks < 1) blocks = 1;
  if (blocks > B) blocks = B;
  return run(ctx, entry, st, rows, "catobs::electrolyte_kernel", P, WY, steric, [&](auto p_, auto wy_, auto steric_) {
    hipLaunchKernelGGL((electrolyte_kernel<p_(), wy_(), steric_()>), dim3((int)blocks), dim3(64 * wy_()), 0, st, a);
  });
}

}  // extern "C"
