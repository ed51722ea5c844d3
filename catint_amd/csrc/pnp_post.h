// What the libraries that derive quantities from a device-resident state (observe/catobs.hip, balance/catbal.hip) have in common.
// Each library is one translation unit and compiles its own copy: nothing here is exported.  gfx950 / MI355X only.
//
// Layout (that of the compat kernels): thread t of the WY waves of an operating point owns the P consecutive grid points
// t P + 1 .. t P + P; its window of P + 2 values starts at point t P, so it holds both neighbours of every own point and both ends of
// the P edges to the left of its points (edge e lies between points e and e + 1; the thread owns edges t P .. t P + P - 1).  The wall
// point is window position 0 of thread 0.  When the nx - 2 interior points fill the waves exactly (nx = 64 P WY + 2: 66, 130, ...,
// 1026, 2050, 4098 -- `tight`) the bulk point and the last edge have no owner: the last thread stores them.
// Memory: rows come in as 16-byte buffer loads whose resource ends at the row's nx-th value (beyond it the hardware returns 0, so
// neither the pad of the row pitch nor a neighbouring row is ever read); results go out as 16-byte buffer stores of the P own values
// (a wave writes 64 P consecutive doubles; the resource ends at the row's end, stores beyond it are dropped) plus single stores of the
// wall value and, when tight, the bulk value.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "pnp_math.h"
#include "pnp_stage.h"
#include "pnp_wave.h"

namespace pnp {
namespace post {

// ---- device: windows and rows ----------------------------------------------------------------------------------------------------
typedef unsigned int u2 __attribute__((ext_vector_type(2)));

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

// B(u) = u / (exp(u) - 1): the solver's evaluation (edge_flux in pnp_newton.hip, oracle/pnp_physical.py: bernoulli, SERIES_U).
// Domain |u| <= 709: beyond it expm1_sc is +inf and nrcp(+inf) is NaN, not 0; every caller bounds u far below that.  Within 8 ulp on both
// sides of the switch (tests/test_gpu_primitives.py, profiles/primitives_unit.md).
__device__ __forceinline__ double bernoulli(double u) {
  if (fabs(u) < 0.05) {
    const double u2 = u * u;
    return 1.0 - 0.5 * u + u2 * (1.0 / 12.0 + u2 * (-1.0 / 720.0 + u2 * (1.0 / 30240.0)));
  }
  return u * pnp::nrcp(pnp::expm1_sc(u));
}

// ---- host: the launch shape ------------------------------------------------------------------------------------------------------
constexpr int MAX_NX = 4098, MAX_SPECIES = 8;   // 4 waves x 64 lanes x 16 points + the two boundary points; PNP_NEWTON_MAX_SPECIES

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

template <int V>
using ic = std::integral_constant<int, V>;

// the compiled (P, WY, steric) instances of a kernel: f(ic<P>, ic<WY>, std::bool_constant<STERIC>) launches the one that was chosen
template <bool STERIC, class F>
static void launch_shape(int P, int WY, F&& f) {
  constexpr std::bool_constant<STERIC> s{};
  if (WY == 4) f(ic<16>(), ic<4>(), s);
  else if (WY == 2) f(ic<16>(), ic<2>(), s);
  else if (P == 1) f(ic<1>(), ic<1>(), s);
  else if (P == 2) f(ic<2>(), ic<1>(), s);
  else if (P == 4) f(ic<4>(), ic<1>(), s);
  else if (P == 8) f(ic<8>(), ic<1>(), s);
  else f(ic<16>(), ic<1>(), s);
}

// ---- host: the context and the frame of an entry point ---------------------------------------------------------------------------
constexpr int OK = 0, ERR_INVAL = -1, ERR_NOMEM = -2, ERR_DEVICE = -3;   // the CATOBS_* / CATBAL_* codes

struct Ctx {
  int device = 0;
  double* buf = nullptr;     // device: the call's inputs, then the requested output rows (and what else the library lays behind them)
  size_t buf_doubles = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the kernel of the last call (last_kernel_ms)
  float kernel_ms = -1.0f;
  std::string err, last_kernel;
  std::vector<double> stage;    // host: the inputs of the call in flight, one copy (pnp_stage.h: Inputs)
  std::vector<int32_t> flags;   // host: the int32 rows (status, counters) as the kernel wrote them
};

static thread_local std::string g_create_error;

static int fail(Ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  else g_create_error = msg;
  return code;
}

// C: the library's context type (Ctx or derived from it); entry: the name of the exported function, the head of every message
template <class C>
static int create(const char* entry, int32_t device, C** out) {
  const std::string e(entry);
  if (!out) return fail(nullptr, ERR_INVAL, e + ": null argument");
  if (device < 0) return fail(nullptr, ERR_INVAL, e + ": negative device ordinal");
  C* ctx = new (std::nothrow) C;
  if (!ctx) return fail(nullptr, ERR_NOMEM, e + ": out of host memory");
  ctx->device = device;
  *out = ctx;
  return OK;
}

template <class C>
static void destroy(C* ctx) {
  if (!ctx) return;
  if ((ctx->buf || ctx->ev0) && hipSetDevice(ctx->device) == hipSuccess) {
    if (ctx->buf) (void)hipFree(ctx->buf);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  }
  delete ctx;
}

static const char* last_error(const Ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }
static const char* last_kernel(const Ctx* ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }
static float last_kernel_ms(const Ctx* ctx) { return ctx ? ctx->kernel_ms : -1.0f; }

static int hip_fail(Ctx* ctx, const char* entry, const char* call, hipError_t e) {
  return fail(ctx, e == hipErrorOutOfMemory ? ERR_NOMEM : ERR_DEVICE, std::string(entry) + ": " + call + ": " + hipGetErrorString(e));
}
// returns from a function that has `ctx` and `entry` in scope with "<entry>: <call>: <hip string>"
#define PNP_POST_HIP(call)                                                        \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) return pnp::post::hip_fail(ctx, entry, #call, e_);      \
  } while (0)

// What every entry point checks first, in this order (Params: catobs_params / catbal_params, params_name its name): 0 or the code.
template <class Params>
static int check_view(Ctx* ctx, const char* entry, const char* params_name, const pnp_device_view* view, const Params* p, const void* out) {
  if (!ctx) return ERR_INVAL;
  const std::string e(entry);
  if (!view || !p || !out) return fail(ctx, ERR_INVAL, e + ": null argument");
  if (view->struct_size != (int32_t)sizeof(pnp_device_view))
    return fail(ctx, ERR_INVAL, e + ": pnp_device_view.struct_size does not match this library");
  if (p->struct_size != (int32_t)sizeof(Params)) return fail(ctx, ERR_INVAL, e + ": " + params_name + ".struct_size does not match this library");
  if (!view->phi_dev || !view->c_dev)
    return fail(ctx, ERR_INVAL, e + ": the view has no potential row (only the physical mode keeps the potential in its state)");
  const int N = view->nspecies, nx = view->nx;
  char msg[256];
  if (nx < 3 || nx > MAX_NX) {
    snprintf(msg, sizeof msg, "%s: nx = %d outside [3, %d]", entry, nx, MAX_NX);
    return fail(ctx, ERR_INVAL, msg);
  }
  if (N < 1 || N > MAX_SPECIES) {
    snprintf(msg, sizeof msg, "%s: %d species outside [1, %d]", entry, N, MAX_SPECIES);
    return fail(ctx, ERR_INVAL, msg);
  }
  if (view->batch < 1 || view->row_pitch < nx) return fail(ctx, ERR_INVAL, e + ": empty batch or a row pitch below nx");
  if (!p->D || !p->charges || !p->x) return fail(ctx, ERR_INVAL, e + ": D, charges and x are required");
  for (int i = 1; i < nx; ++i)
    if (!(p->x[i] > p->x[i - 1])) {
      snprintf(msg, sizeof msg, "%s: x is not strictly increasing at index %d", entry, i);
      return fail(ctx, ERR_INVAL, msg);
    }
  return OK;
}

// the context's device buffer only grows
static int reserve(Ctx* ctx, const char* entry, size_t need) {
  if (need > ctx->buf_doubles) {
    if (ctx->buf) PNP_POST_HIP(hipFree(ctx->buf));
    ctx->buf = nullptr;
    ctx->buf_doubles = 0;
    PNP_POST_HIP(hipMalloc((void**)&ctx->buf, need * sizeof(double)));
    ctx->buf_doubles = need;
  }
  return OK;
}

// Persistent grid: as many waves as the device holds at once (occupancy(&per_cu): the occupancy query of the chosen instance, made only
// when the caller does not size the grid with max_waves), no more than there are groups of systems.
template <class Occ>
static int persistent_waves(Ctx* ctx, const char* entry, int64_t max_waves, Occ&& occupancy, int64_t groups, int64_t* out) {
  int64_t blocks = max_waves;
  if (blocks == 0) {
    int cus = 0, per_cu = 0;
    PNP_POST_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const hipError_t oe = occupancy(&per_cu);
    PNP_POST_HIP(oe);
    blocks = (int64_t)std::max(per_cu, 1) * std::max(cus, 1);
  }
  *out = std::min(std::max<int64_t>(blocks, 1), groups);
  return OK;
}

// the int32 rows a kernel writes behind its output rows: n of them at dev, copied to ctx->flags when wanted
struct Flags {
  const int32_t* dev;
  size_t n;
  bool wanted;
};

// The tail of every entry point, on stream st: the first n_in doubles of ctx->stage copied to the device buffer (0: nothing), launch()
// (the chosen instance; its hipError_t) between the context's two events, the wanted rows and the wanted flags copied back, the stream
// drained, and the time between the events in *ms.
template <size_t NR, class L>
static int launch_and_fetch(Ctx* ctx, const char* entry, hipStream_t st, size_t n_in, const Row (&rows)[NR], const Flags& fl, float* ms, L&& launch) {
  if (n_in) PNP_POST_HIP(hipMemcpyAsync(ctx->buf, ctx->stage.data(), n_in * sizeof(double), hipMemcpyHostToDevice, st));
  if (!ctx->ev0) PNP_POST_HIP(hipEventCreate(&ctx->ev0));
  if (!ctx->ev1) PNP_POST_HIP(hipEventCreate(&ctx->ev1));
  ctx->kernel_ms = -1.0f;
  PNP_POST_HIP(hipEventRecord(ctx->ev0, st));
  const hipError_t le = launch();
  PNP_POST_HIP(le);
  PNP_POST_HIP(hipGetLastError());
  PNP_POST_HIP(hipEventRecord(ctx->ev1, st));
  for (const Row& r : rows)
    if (r.wanted()) PNP_POST_HIP(hipMemcpyAsync(r.host, *r.dev, r.n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (fl.wanted) PNP_POST_HIP(hipMemcpyAsync(ctx->flags.data(), fl.dev, fl.n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PNP_POST_HIP(hipStreamSynchronize(st));
  PNP_POST_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
  return OK;
}

// The tail of the libraries whose kernel comes in (P, WY, steric) instances (f: see launch_shape) and writes no flags
template <size_t NR, class F>
static int run(Ctx* ctx, const char* entry, hipStream_t st, const Row (&rows)[NR], const char* kernel, int P, int WY, bool steric, F&& f) {
  if (const int rc = launch_and_fetch(ctx, entry, st, 0, rows, Flags{nullptr, 0, false}, &ctx->kernel_ms, [&] {
        if (steric) launch_shape<true>(P, WY, f);
        else launch_shape<false>(P, WY, f);
        return hipSuccess;
      }))
    return rc;
  char msg[128];
  snprintf(msg, sizeof msg, "%s<%d, %d, %s>", kernel, P, WY, steric ? "true" : "false");
  ctx->last_kernel = msg;
  return OK;
}

}  // namespace post
}  // namespace pnp
