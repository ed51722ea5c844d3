// libcatint_regrid (include/catint_regrid.h): the state a pnp_handle of the physical mode holds on the device resampled onto another
// grid with the Scharfetter-Gummel interpolant of the header's definition.  It shares no code with the Newton kernels: the formulas
// are restated here from the header.  Context, validation frame and Bernoulli function: csrc/pnp_post.h.  gfx950 / MI355X only.
//
// Layout: WY waves (1 / 2 / 4 by max(nx, nx_target) <= 1026 / 2050 / 4098) per operating point, persistent workgroups walk the
// requested lanes i, i + grid, ...  Per operating point the source potential row is staged in LDS by 16-byte buffer loads (the
// resource ends with the pair that holds the row's nx-th value: neither the rest of the pitch nor a neighbouring row is read); with
// steric ions a first pass over the species rows sums phi0 into a second LDS row, which becomes w = -ln(1 - phi0) (every thread
// works on the slots it staged itself: no barrier in between); then one species row at a time is staged in a third LDS row.  The
// rows are dynamic LDS of the source grid's length: 3 x 32.8 KB at 4098 points with steric ions (one workgroup per CU), 6 KB at 384
// points without (the CU's 32 waves); the grid is what the device holds at once.
// Threads take target points in pairs, strided over the workgroup (pair j = 2 t + 2 T m), read the cell index e, the cell coordinate
// s and the cell length h of the pair from the table the host built (16 + 16 + 8 bytes per lane, consecutive over the wave; the same
// for every operating point and species: L2), gather both cell ends from LDS and store 16 bytes per lane: a wave's store instruction
// writes 1 KiB of consecutive bytes.  The loops run to the row pitch, so the pads of the result are written as zeros.  No index read
// on the device can point outside a row: the host validates every e in [0, nx-1], and the right end is min(e + 1, nx - 1) (e = nx-1
// only with s = 0, the last node, which copies).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../../include/catint_regrid.h"
#include "../pnp_post.h"

namespace catgrid {

using namespace pnp::post;
using pnp::d2;

constexpr int MAXS = CATGRID_MAX_SPECIES;
typedef int i2 __attribute__((ext_vector_type(2)));

struct KArgs {
  int32_t N, nx, ldx, nxt, pitch, pad_;
  int64_t n;               // operating points to resample
  const double* c;         // [B][N][ldx]
  const double* phi;       // [B][ldx]
  const double* s;         // [pitch] cell coordinate of every target point (pads: 0)
  const double* h;         // [pitch] length of its cell (pads: 1)
  const int32_t* e;        // [pitch] its cell (pads: 0)
  const int64_t* lanes;    // [n] source operating points
  double* oc;              // [n][N][pitch]
  double* ophi;            // [n][pitch]
  double qb[MAXS], pe[MAXS], vol[MAXS];   // q_k beta, velocity / D_k, N_A a_k^3
};

// source row -> LDS: thread t stages the pairs 2 t + 2 T m; the resource ends behind the pair that holds the row's last value
template <int T>
__device__ __forceinline__ void stage_row(const double* row, int nx, double* dst, int t) {
  const __amdgpu_buffer_rsrc_t r = pnp::row_rsrc(row, (nx + 1) & ~1);
  for (int off = 2 * t; off < nx; off += 2 * T)
    *reinterpret_cast<d2*>(dst + off) = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, off * 8, 0, 0));
}

// c(X) between the node values ce, ce1 of a cell with the solver's u, at cell coordinate s
__device__ __forceinline__ double sg_value(double ce, double ce1, double u, double s) {
  u = u > CATGRID_MAX_U ? CATGRID_MAX_U : (u < -CATGRID_MAX_U ? -CATGRID_MAX_U : u);   // (a NaN stays a NaN)
  const double r = 1.0 - s;
  const double G = s * bernoulli(-u) * pnp::nrcp(bernoulli(-u * s));
  const double H = r * bernoulli(u) * pnp::nrcp(bernoulli(u * r));
  const double v = __builtin_fma(H, ce, G * ce1);
  return s == 0.0 ? ce : v;
}

template <int WY, bool STERIC>
__global__ __launch_bounds__(64 * WY) void regrid_kernel(const KArgs A) {
  constexpr int T = 64 * WY;
  extern __shared__ __attribute__((aligned(16))) double smem[];   // lds_bytes(): 2 or 3 rows of nx doubles, rounded up to a pair
  const int t = threadIdx.x;
  const int nx = A.nx, N = A.N, nxt = A.nxt, pitch = A.pitch, last = nx - 1;
  double* const sphi = smem;
  double* const sc = smem + ((nx + 1) & ~1);
  double* const sw = sc + ((nx + 1) & ~1);   // steric only

  for (int64_t i = blockIdx.x; i < A.n; i += gridDim.x) {
    const int64_t b = A.lanes[i];
    const double* crow = A.c + (size_t)b * N * A.ldx;
    pnp::wg_sync<WY>();          // the previous operating point's reads of the LDS rows are done
    stage_row<T>(A.phi + (size_t)b * A.ldx, nx, sphi, t);
    if constexpr (STERIC) {
      for (int k = 0; k < N; ++k) {
        const __amdgpu_buffer_rsrc_t r = pnp::row_rsrc(crow + (size_t)k * A.ldx, (nx + 1) & ~1);
        const double vol = A.vol[k];
        for (int off = 2 * t; off < nx; off += 2 * T) {
          const d2 v = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, off * 8, 0, 0));
          d2 a = *reinterpret_cast<d2*>(sw + off);
          a.x = k == 0 ? vol * v.x : __builtin_fma(vol, v.x, a.x);
          a.y = k == 0 ? vol * v.y : __builtin_fma(vol, v.y, a.y);
          *reinterpret_cast<d2*>(sw + off) = a;
        }
      }
      for (int off = 2 * t; off < nx; off += 2 * T) {
        d2 a = *reinterpret_cast<d2*>(sw + off);
        a.x = -pnp::log1p_sc(-a.x);
        a.y = -pnp::log1p_sc(-a.y);
        *reinterpret_cast<d2*>(sw + off) = a;
      }
    }
    pnp::wg_sync<WY>();

    // the potential: linear inside the cell
    {
      double* orow = A.ophi + (size_t)i * pitch;
      for (int j = 2 * t; j < pitch; j += 2 * T) {
        const d2 s = *reinterpret_cast<const d2*>(A.s + j);
        const i2 e = *reinterpret_cast<const i2*>(A.e + j);
        const double p0 = sphi[e.x], p1 = sphi[e.y];
        const double v0 = __builtin_fma(s.x, sphi[min(e.x + 1, last)] - p0, p0);
        const double v1 = __builtin_fma(s.y, sphi[min(e.y + 1, last)] - p1, p1);
        d2 o;
        o.x = j < nxt ? (s.x == 0.0 ? p0 : v0) : 0.0;
        o.y = j + 1 < nxt ? (s.y == 0.0 ? p1 : v1) : 0.0;
        *reinterpret_cast<d2*>(orow + j) = o;
      }
    }

    // one species at a time
    for (int k = 0; k < N; ++k) {
      if (k > 0) pnp::wg_sync<WY>();   // the previous species' reads of sc are done
      stage_row<T>(crow + (size_t)k * A.ldx, nx, sc, t);
      pnp::wg_sync<WY>();
      const double qbk = A.qb[k], pek = A.pe[k];
      double* orow = A.oc + ((size_t)i * N + k) * pitch;
      for (int j = 2 * t; j < pitch; j += 2 * T) {
        const d2 s = *reinterpret_cast<const d2*>(A.s + j);
        const d2 h = *reinterpret_cast<const d2*>(A.h + j);
        const i2 e = *reinterpret_cast<const i2*>(A.e + j);
        const int f0 = min(e.x + 1, last), f1 = min(e.y + 1, last);
        double dw0 = 0.0, dw1 = 0.0;
        if constexpr (STERIC) {
          dw0 = sw[f0] - sw[e.x];
          dw1 = sw[f1] - sw[e.y];
        }
        const double u0 = __builtin_fma(qbk, sphi[f0] - sphi[e.x], dw0) - pek * h.x;
        const double u1 = __builtin_fma(qbk, sphi[f1] - sphi[e.y], dw1) - pek * h.y;
        d2 o;
        o.x = j < nxt ? sg_value(sc[e.x], sc[f0], u0, s.x) : 0.0;
        o.y = j + 1 < nxt ? sg_value(sc[e.y], sc[f1], u1, s.y) : 0.0;
        *reinterpret_cast<d2*>(orow + j) = o;
      }
    }
  }
}

// LDS of a launch: the potential row, the species row and, with steric ions, w
static size_t lds_bytes(int nx, bool steric) { return (size_t)(steric ? 3 : 2) * ((nx + 1) & ~1) * sizeof(double); }

// The instance on stream st between the two events.  max_waves == 0: as many workgroups as the device holds at once (persistent:
// each walks i, i + grid, ...), no more than there are operating points.
template <int WY, bool STERIC>
static hipError_t launch(const KArgs& a, int max_waves, int cus, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  const auto kernel = regrid_kernel<WY, STERIC>;
  const size_t lds = lds_bytes(a.nx, STERIC);
  hipError_t e;
  if (lds > 48 * 1024 && (e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess)
    return e;
  int64_t blocks = max_waves / WY;
  if (max_waves == 0) {
    int per_cu = 0;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64 * WY, lds)) != hipSuccess) return e;
    blocks = (int64_t)std::max(per_cu, 1) * cus;
  }
  blocks = std::min(std::max<int64_t>(blocks, 1), a.n);
  if ((e = hipEventRecord(ev0, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3((int)blocks), dim3(64 * WY), lds, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipEventRecord(ev1, st);
}

}  // namespace catgrid

static_assert(CATGRID_OK == pnp::post::OK && CATGRID_EINVAL == pnp::post::ERR_INVAL && CATGRID_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATGRID_EDEVICE == pnp::post::ERR_DEVICE && CATGRID_MAX_NX == pnp::post::MAX_NX && CATGRID_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_regrid.h and pnp_post.h disagree");

struct catgrid_ctx : pnp::post::Ctx {};

extern "C" {

int catgrid_create(int32_t device, catgrid_ctx** out) { return pnp::post::create("catgrid_create", device, out); }
void catgrid_destroy(catgrid_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catgrid_last_error(const catgrid_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catgrid_last_kernel(const catgrid_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catgrid_last_kernel_ms(const catgrid_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catgrid_resample(catgrid_ctx* ctx, const pnp_device_view* view, const catgrid_params* p, const catgrid_outputs* out) {
  using namespace catgrid;
  static const char entry[] = "catgrid_resample";
  if (const int rc = check_view(ctx, entry, "catgrid_params", view, p, out)) return rc;
  const int N = view->nspecies, nx = view->nx;
  const int64_t B = view->batch;
  char msg[256];
  if (p->max_waves < 0) return fail(ctx, CATGRID_EINVAL, "catgrid_resample: negative max_waves");
  if (!(p->beta > 0.0) || !std::isfinite(p->beta) || !std::isfinite(p->velocity))
    return fail(ctx, CATGRID_EINVAL, "catgrid_resample: beta must be positive and finite, velocity finite");
  for (int k = 0; k < N; ++k) {
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    if (!(p->D[k] > 0.0) || !std::isfinite(p->D[k]) || !std::isfinite(p->charges[k]) || !(r >= 0.0) || !std::isfinite(r)) {
      snprintf(msg, sizeof msg, "catgrid_resample: species %d needs D > 0, a finite charge and a radius >= 0 (all finite)", k);
      return fail(ctx, CATGRID_EINVAL, msg);
    }
  }
  const int nxt = p->nx_target;
  if (nxt < 3 || nxt > CATGRID_MAX_NX) {
    snprintf(msg, sizeof msg, "catgrid_resample: nx_target = %d outside [3, %d]", nxt, CATGRID_MAX_NX);
    return fail(ctx, CATGRID_EINVAL, msg);
  }
  if (!p->x_target) return fail(ctx, CATGRID_EINVAL, "catgrid_resample: x_target is required");
  for (int j = 0; j < nxt; ++j) {
    const double X = p->x_target[j];
    if (j > 0 && !(X > p->x_target[j - 1])) {
      snprintf(msg, sizeof msg, "catgrid_resample: x_target is not strictly increasing at index %d", j);
      return fail(ctx, CATGRID_EINVAL, msg);
    }
    if (!(X >= p->x[0] && X <= p->x[nx - 1])) {
      snprintf(msg, sizeof msg, "catgrid_resample: target point %d lies outside the source grid (no extrapolation)", j);
      return fail(ctx, CATGRID_EINVAL, msg);
    }
  }
  if (p->lanes && p->nlanes < 0) return fail(ctx, CATGRID_EINVAL, "catgrid_resample: nlanes < 0");
  const int64_t n = p->lanes ? p->nlanes : B;
  for (int64_t i = 0; p->lanes && i < n; ++i)
    if (p->lanes[i] < 0 || p->lanes[i] >= B) {
      snprintf(msg, sizeof msg, "catgrid_resample: lane index %lld outside [0, %lld)", (long long)p->lanes[i], (long long)B);
      return fail(ctx, CATGRID_EINVAL, msg);
    }
  if (n == 0) return CATGRID_OK;

  KArgs a;
  memset(&a, 0, sizeof a);
  const int pitch = (nxt + 15) / 16 * 16;
  a.N = N; a.nx = nx; a.ldx = view->row_pitch; a.nxt = nxt; a.pitch = pitch; a.n = n;
  a.c = view->c_dev; a.phi = view->phi_dev;
  bool steric = false;
  for (int k = 0; k < N; ++k) {
    a.qb[k] = p->charges[k] * p->beta;
    a.pe[k] = p->velocity / p->D[k];
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    a.vol[k] = pnp::N_AVOGADRO * r * r * r;
    steric = steric || a.vol[k] != 0.0;
  }
  const int big = std::max(nx, nxt), WY = big <= 1026 ? 1 : (big <= 2050 ? 2 : 4);

  // the table of the target points (cell, cell coordinate, cell length) and the lane list, staged on the host for one copy
  Inputs in;
  const int i_s = in.add((size_t)pitch, &a.s), i_h = in.add((size_t)pitch, &a.h), i_e = in.add((size_t)pitch / 2, &a.e), i_l = in.add((size_t)n, &a.lanes);
  const size_t n_in = in.total;
  try {
    ctx->stage.assign(n_in, 0.0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATGRID_ENOMEM, "catgrid_resample: out of host memory");
  }
  double *ss = in.host(ctx->stage, i_s), *sh = in.host(ctx->stage, i_h);
  int32_t* se = reinterpret_cast<int32_t*>(in.host(ctx->stage, i_e));
  int64_t* sl = reinterpret_cast<int64_t*>(in.host(ctx->stage, i_l));
  for (int j = 0; j < pitch; ++j) sh[j] = 1.0;
  for (int j = 0; j < nxt; ++j) {
    const double X = p->x_target[j];
    int e = (int)(std::upper_bound(p->x, p->x + nx, X) - p->x) - 1;   // the largest e with x[e] <= X
    if (e > nx - 2) e = nx - 2;
    const double he = p->x[e + 1] - p->x[e];
    if (X == p->x[nx - 1]) {     // the last node: a copy
      se[j] = nx - 1;
      ss[j] = 0.0;
    } else {
      se[j] = e;
      ss[j] = (X - p->x[e]) / he;
    }
    sh[j] = he;
  }
  for (int64_t i = 0; i < n; ++i) sl[i] = p->lanes ? p->lanes[i] : i;

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  const size_t n_c = (size_t)n * N * pitch, n_phi = (size_t)n * pitch;
  if (const int rc = reserve(ctx, entry, n_in + n_c + n_phi)) return rc;
  in.place(ctx->buf);
  a.oc = ctx->buf + n_in;
  a.ophi = a.oc + n_c;
  PNP_POST_HIP(hipMemcpyAsync(ctx->buf, ctx->stage.data(), n_in * sizeof(double), hipMemcpyHostToDevice, st));
  if (!ctx->ev0) PNP_POST_HIP(hipEventCreate(&ctx->ev0));
  if (!ctx->ev1) PNP_POST_HIP(hipEventCreate(&ctx->ev1));
  ctx->kernel_ms = -1.0f;
  int cus = 0;
  PNP_POST_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const auto by_waves = [&](auto steric_) {
    constexpr bool S = decltype(steric_)::value;
    return WY == 4 ? launch<4, S>(a, p->max_waves, cus, st, ctx->ev0, ctx->ev1)
                   : WY == 2 ? launch<2, S>(a, p->max_waves, cus, st, ctx->ev0, ctx->ev1) : launch<1, S>(a, p->max_waves, cus, st, ctx->ev0, ctx->ev1);
  };
  const hipError_t le = steric ? by_waves(std::true_type()) : by_waves(std::false_type());
  PNP_POST_HIP(le);
  const size_t w = (size_t)nxt * sizeof(double), dp = (size_t)pitch * sizeof(double);
  if (out->c) PNP_POST_HIP(hipMemcpy2DAsync(out->c, w, a.oc, dp, w, (size_t)n * N, hipMemcpyDeviceToHost, st));
  if (out->phi) PNP_POST_HIP(hipMemcpy2DAsync(out->phi, w, a.ophi, dp, w, (size_t)n, hipMemcpyDeviceToHost, st));
  PNP_POST_HIP(hipStreamSynchronize(st));
  PNP_POST_HIP(hipEventElapsedTime(&ctx->kernel_ms, ctx->ev0, ctx->ev1));
  snprintf(msg, sizeof msg, "catgrid::regrid_kernel<%d, %s>", WY, steric ? "true" : "false");
  ctx->last_kernel = msg;
  if (out->c_dev) *out->c_dev = a.oc;
  if (out->phi_dev) *out->phi_dev = a.ophi;
  return CATGRID_OK;
}

}  // extern "C"
