// libcatint_observe (include/catint_observe.h): electrolyte observables of the physical mode derived on the device from the state a
// pnp_handle holds there.  One pass over the state: every operating point is one workgroup iteration, the species rows are summed
// in registers, the two potential drops are prefix sums over the edges.  gfx950 / MI355X only.
//
// Layout (that of the compat kernels): thread t of the WY waves of an operating point owns the P consecutive grid points
// t P + 1 .. t P + P; its window of P + 2 values starts at point t P, so it holds both neighbours of every own point and both ends of
// the P edges to the left of its points (edge e lies between points e and e + 1; the thread owns edges t P .. t P + P - 1).  The wall
// point is window position 0 of thread 0.  When the nx - 2 interior points fill the waves exactly (nx = 64 P WY + 2: 66, 130, ...,
// 1026, 2050, 4098 -- `tight`) the bulk point and the last edge have no owner: every thread then also evaluates window position P + 1
// and edge P, and the last thread stores them.
// Memory: rows come in as 16-byte buffer loads whose resource ends at the row's nx-th value (beyond it the hardware returns 0, so
// neither the pad of the row pitch nor a neighbouring row is ever read); results go out as 16-byte buffer stores of the P own values
// (a wave writes 64 P consecutive doubles; the resource ends at the row's end, stores beyond it are dropped) plus single stores of the
// wall value and, when tight, the bulk value.  Point ions: every input row is read once.  Steric ions: w = -ln(1 - phi0) is needed at
// both ends of an edge before any species flux, so the species rows are read twice (the second time from L2).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/catint_observe.h"
#include "../pnp_math.h"
#include "../pnp_wave.h"

namespace catobs {

using pnp::d2;
using pnp::u4;
typedef unsigned int u2 __attribute__((ext_vector_type(2)));

constexpr double N_AVOGADRO = 6.022140857e23;   // catint/units.py (unit_NA), as in oracle/pnp_physical.py

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

// window of P + 2 doubles starting at element t P of a row
template <int P>
__device__ __forceinline__ void load_win(__amdgpu_buffer_rsrc_t r, double (&w)[P + 2], int t) {
  if constexpr (P == 1) {
#pragma unroll
    for (int q = 0; q < 3; ++q) w[q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, t * 8 + q * 8, 0, 0));
  } else {
    pnp::load_window<P>(r, w, t);
  }
}

// v[OFF .. OFF + P) to consecutive doubles at byte offset `at`
template <int P, int OFF, int LEN>
__device__ __forceinline__ void store_blocked(__amdgpu_buffer_rsrc_t r, const double (&v)[LEN], int at) {
  if constexpr (P == 1) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v[OFF]), r, at, 0, 0);
  } else {
#pragma unroll
    for (int q = 0; q < P / 2; ++q) {
      d2 t;
      t.x = v[OFF + 2 * q];
      t.y = v[OFF + 2 * q + 1];
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, t), r, at + q * 16, 0, 0);
    }
  }
}

// element `pos` (thread-dependent) of a register array: compares, not an indexed access (which would go to scratch)
template <int LEN>
__device__ __forceinline__ double pick(const double (&a)[LEN], int pos) {
  double v = 0.0;
#pragma unroll
  for (int j = 0; j < LEN; ++j) v = (j == pos) ? a[j] : v;
  return v;
}

// Row of point values, v[jw] = value at window position jw: own positions 1 .. P by vector stores, the wall by thread 0, the bulk
// point by the last thread when it has no owner.
template <int P, int T>
__device__ __forceinline__ void store_point_row(double* row, const double (&v)[P + 2], int nx, int t, bool tight) {
  store_blocked<P, 1, P + 2>(pnp::row_rsrc(row, nx), v, (t * P + 1) * 8);
  if (t == 0) row[0] = v[0];
  if (tight && t == T - 1) row[nx - 1] = v[P + 1];
}

// Row of edge values, v[j] = value on edge t P + j
template <int P, int T>
__device__ __forceinline__ void store_edge_row(double* row, const double (&v)[P + 1], int nx, int t, bool tight) {
  store_blocked<P, 0, P + 1>(pnp::row_rsrc(row, nx - 1), v, t * P * 8);
  if (tight && t == T - 1) row[nx - 2] = v[P];
}

// B(u) = u / (exp(u) - 1): the solver's evaluation (edge_flux in pnp_newton.hip, oracle/pnp_physical.py: bernoulli, SERIES_U)
__device__ __forceinline__ double bernoulli(double u) {
  if (fabs(u) < 0.05) {
    const double u2 = u * u;
    return 1.0 - 0.5 * u + u2 * (1.0 / 12.0 + u2 * (-1.0 / 720.0 + u2 * (1.0 / 30240.0)));
  }
  return u * pnp::nrcp(pnp::expm1_sc(u));
}

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

// (P, WY) of a grid: the compat kernels' rule -- nx - 2 <= 64 P in one wave up to 1026 points, then 16 points per lane in 2 / 4 waves
static void choose_shape(int nx, int* P, int* WY) {
  const int m = nx - 2;
  *WY = 1;
  if (m > 2048) *P = 16, *WY = 4;
  else if (m > 1024) *P = 16, *WY = 2;
  else
    for (int p : {1, 2, 4, 8, 16})
      if (m <= 64 * p) {
        *P = p;
        break;
      }
}

template <int P, int WY, bool STERIC>
static void launch_one(const KArgs& a, int blocks, hipStream_t st) {
  hipLaunchKernelGGL((electrolyte_kernel<P, WY, STERIC>), dim3(blocks), dim3(64 * WY), 0, st, a);
}
template <bool STERIC>
static void launch_shape(int P, int WY, const KArgs& a, int blocks, hipStream_t st) {
  if (WY == 4) launch_one<16, 4, STERIC>(a, blocks, st);
  else if (WY == 2) launch_one<16, 2, STERIC>(a, blocks, st);
  else if (P == 1) launch_one<1, 1, STERIC>(a, blocks, st);
  else if (P == 2) launch_one<2, 1, STERIC>(a, blocks, st);
  else if (P == 4) launch_one<4, 1, STERIC>(a, blocks, st);
  else if (P == 8) launch_one<8, 1, STERIC>(a, blocks, st);
  else launch_one<16, 1, STERIC>(a, blocks, st);
}

}  // namespace catobs

struct catobs_ctx {
  int device = 0;
  double* buf = nullptr;     // device: the grid, then the requested output rows
  size_t buf_doubles = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the kernel of the last call (catobs_last_kernel_ms)
  float kernel_ms = -1.0f;
  std::string err, last_kernel;
};

static thread_local std::string g_catobs_create_error;

static int catobs_fail(catobs_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  else g_catobs_create_error = msg;
  return code;
}

extern "C" {

int catobs_create(int32_t device, catobs_ctx** out) {
  if (!out) return catobs_fail(nullptr, CATOBS_EINVAL, "catobs_create: null argument");
  if (device < 0) return catobs_fail(nullptr, CATOBS_EINVAL, "catobs_create: negative device ordinal");
  catobs_ctx* ctx = new (std::nothrow) catobs_ctx;
  if (!ctx) return catobs_fail(nullptr, CATOBS_ENOMEM, "catobs_create: out of host memory");
  ctx->device = device;
  *out = ctx;
  return CATOBS_OK;
}

void catobs_destroy(catobs_ctx* ctx) {
  if (!ctx) return;
  if ((ctx->buf || ctx->ev0) && hipSetDevice(ctx->device) == hipSuccess) {
    if (ctx->buf) (void)hipFree(ctx->buf);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  }
  delete ctx;
}

const char* catobs_last_error(const catobs_ctx* ctx) { return ctx ? ctx->err.c_str() : g_catobs_create_error.c_str(); }
const char* catobs_last_kernel(const catobs_ctx* ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }
float catobs_last_kernel_ms(const catobs_ctx* ctx) { return ctx ? ctx->kernel_ms : -1.0f; }

int catobs_electrolyte(catobs_ctx* ctx, const pnp_device_view* view, const catobs_params* p, const catobs_outputs* out) {
  using namespace catobs;
  if (!ctx) return CATOBS_EINVAL;
  if (!view || !p || !out) return catobs_fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: null argument");
  if (view->struct_size != (int32_t)sizeof(pnp_device_view))
    return catobs_fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: pnp_device_view.struct_size does not match this library");
  if (p->struct_size != (int32_t)sizeof(catobs_params))
    return catobs_fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: catobs_params.struct_size does not match this library");
  if (!view->phi_dev || !view->c_dev)
    return catobs_fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: the view has no potential row (only the physical mode keeps the potential in its state)");
  const int N = view->nspecies, nx = view->nx;
  const int64_t B = view->batch;
  char msg[256];
  if (nx < 3 || nx > CATOBS_MAX_NX) {
    snprintf(msg, sizeof msg, "catobs_electrolyte: nx = %d outside [3, %d]", nx, CATOBS_MAX_NX);
    return catobs_fail(ctx, CATOBS_EINVAL, msg);
  }
  if (N < 1 || N > CATOBS_MAX_SPECIES) {
    snprintf(msg, sizeof msg, "catobs_electrolyte: %d species outside [1, %d]", N, CATOBS_MAX_SPECIES);
    return catobs_fail(ctx, CATOBS_EINVAL, msg);
  }
  if (B < 1 || view->row_pitch < nx) return catobs_fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: empty batch or a row pitch below nx");
  if (!p->D || !p->charges || !p->x) return catobs_fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: D, charges and x are required");
  for (int i = 1; i < nx; ++i)
    if (!(p->x[i] > p->x[i - 1])) {
      snprintf(msg, sizeof msg, "catobs_electrolyte: x is not strictly increasing at index %d", i);
      return catobs_fail(ctx, CATOBS_EINVAL, msg);
    }
  if (p->species_H < -1 || p->species_H >= N || p->species_OH < -1 || p->species_OH >= N)
    return catobs_fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: species_H / species_OH outside [-1, N)");
  if (p->max_waves < 0) return catobs_fail(ctx, CATOBS_EINVAL, "catobs_electrolyte: negative max_waves");

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
    a.vol[k] = N_AVOGADRO * r * r * r;
    steric = steric || a.vol[k] != 0.0;
  }
  int P = 1, WY = 1;
  choose_shape(nx, &P, &WY);
  a.tight = (nx - 2 == 64 * P * WY) ? 1 : 0;

#define CATOBS_HIP(call)                                                                                            \
  do {                                                                                                              \
    hipError_t e_ = (call);                                                                                         \
    if (e_ != hipSuccess)                                                                                           \
      return catobs_fail(ctx, e_ == hipErrorOutOfMemory ? CATOBS_ENOMEM : CATOBS_EDEVICE,                           \
                         std::string("catobs_electrolyte: " #call ": ") + hipGetErrorString(e_));                   \
  } while (0)
  CATOBS_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  // one device buffer: the grid (padded to an even count), then the rows that were asked for
  struct Row { double* host; double** dev; size_t n; };
  const size_t np = (size_t)B * nx, ne = (size_t)B * (nx - 1);
  Row rows[] = {{out->efield, &a.efield, np}, {out->charge_density, &a.rho, np}, {out->gamma, &a.gamma, np}, {out->pH, &a.pH, np},
                {out->conductivity, &a.kappa, ne}, {out->current_density, &a.iel, ne}, {out->dphi_iR, &a.diR, np},
                {out->dphi_diff, &a.ddf, np}, {out->scalars, &a.scal, (size_t)B * CATOBS_NSCALARS}};
  size_t need = ((size_t)nx + 1) & ~(size_t)1;
  bool any = false;
  for (const Row& r : rows)
    if (r.host) need += (r.n + 1) & ~(size_t)1, any = true;
  if (!any) return CATOBS_OK;
  if (need > ctx->buf_doubles) {
    if (ctx->buf) CATOBS_HIP(hipFree(ctx->buf));
    ctx->buf = nullptr;
    ctx->buf_doubles = 0;
    CATOBS_HIP(hipMalloc((void**)&ctx->buf, need * sizeof(double)));
    ctx->buf_doubles = need;
  }
  double* cur = ctx->buf;
  a.x = cur;
  cur += ((size_t)nx + 1) & ~(size_t)1;
  for (const Row& r : rows)
    if (r.host) {
      *r.dev = cur;
      cur += (r.n + 1) & ~(size_t)1;
    }
  CATOBS_HIP(hipMemcpyAsync(ctx->buf, p->x, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, st));
  // persistent grid: 8 waves per CU on 256 CUs unless the caller sizes it; every workgroup walks b, b + grid, ...
  const int waves = p->max_waves > 0 ? p->max_waves : 2048;
  int64_t blocks = waves / WY;
  if (blocks < 1) blocks = 1;
  if (blocks > B) blocks = B;
  if (!ctx->ev0) CATOBS_HIP(hipEventCreate(&ctx->ev0));
  if (!ctx->ev1) CATOBS_HIP(hipEventCreate(&ctx->ev1));
  ctx->kernel_ms = -1.0f;
  CATOBS_HIP(hipEventRecord(ctx->ev0, st));
  if (steric) launch_shape<true>(P, WY, a, (int)blocks, st);
  else launch_shape<false>(P, WY, a, (int)blocks, st);
  CATOBS_HIP(hipGetLastError());
  CATOBS_HIP(hipEventRecord(ctx->ev1, st));
  for (const Row& r : rows)
    if (r.host) CATOBS_HIP(hipMemcpyAsync(r.host, *r.dev, r.n * sizeof(double), hipMemcpyDeviceToHost, st));
  CATOBS_HIP(hipStreamSynchronize(st));
  CATOBS_HIP(hipEventElapsedTime(&ctx->kernel_ms, ctx->ev0, ctx->ev1));
#undef CATOBS_HIP
  snprintf(msg, sizeof msg, "catobs::electrolyte_kernel<%d, %d, %s>", P, WY, steric ? "true" : "false");
  ctx->last_kernel = msg;
  return CATOBS_OK;
}

}  // extern "C"
