// Test-only harness (libcatint_unittest.so): every shared device primitive of the libraries behind a kernel of its own, so that
// tests/test_gpu_primitives.py can hold each one to its own accuracy claim instead of seeing it through solver output.  Nothing of the
// product links against this library.  gfx950 / MI355X only.
//
// The exported catunit_* functions take HOST pointers, do their own hipMalloc / copy / launch / synchronise / free and return 0 or the
// HIP error code (hipErrorInvalidValue for an argument that would break a launch rule below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../catint_amd/csrc/pnp_kin.h"
#include "../../catint_amd/csrc/pnp_lane_cols.h"
#include "../../catint_amd/csrc/pnp_lane_common.h"
#include "../../catint_amd/csrc/pnp_math.h"
#include "../../catint_amd/csrc/pnp_post.h"
#include "../../catint_amd/csrc/pnp_wave.h"

namespace catunit {

using namespace pnp;

// ---- scalar functions: 256 threads per block, one argument per thread -------------------------------------------------------------------
enum { FN_FAST_RCP = 0, FN_FAST_RCP2 = 1, FN_NRCP = 2, FN_EXPM1 = 3, FN_LOG1P = 4, FN_BERNOULLI = 5, FN_COUNT = 6 };

template <int FN>
__global__ __launch_bounds__(256) void scalar_kernel(const double* __restrict__ x, double* __restrict__ y, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  double r;
  if constexpr (FN == FN_FAST_RCP) r = fast_rcp(v);
  else if constexpr (FN == FN_FAST_RCP2) r = fast_rcp2(v);
  else if constexpr (FN == FN_NRCP) r = nrcp(v);
  else if constexpr (FN == FN_EXPM1) r = expm1_sc(v);
  else if constexpr (FN == FN_LOG1P) r = log1p_sc(v);
  else r = post::bernoulli(v);
  y[i] = r;
}

// lane_edge_flux(u, cl = 1, cr = 0, w = 1): Bp is B(u) and Ju is B'(u)
__global__ __launch_bounds__(256) void edge_flux_kernel(const double* __restrict__ u, double* __restrict__ B, double* __restrict__ dB, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const lane::LEdge e = lane::lane_edge_flux(u[i], 1.0, 0.0, 1.0);
  B[i] = e.Bp;
  dB[i] = e.Ju;
}

// ---- wave primitives: exactly ONE wave per workgroup (blockDim = 64: the DPP moves, readlane and the wave-private LDS hand-offs of
// ---- lds_sync all assume that the 64 lanes of the workgroup are one wave); one workgroup is one test case ------------------------------
__global__ __launch_bounds__(64) void wave_moves_kernel(const double* __restrict__ v, double old, double* __restrict__ prev, double* __restrict__ next) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const double x = v[i];
  prev[i] = from_prev_lane(old, x);
  next[i] = from_next_lane(old, x);
}

// out[l][lane] = read_lane(v, l) for every l (wave-uniform: the loop counter)
__global__ __launch_bounds__(64) void read_lane_kernel(const double* __restrict__ v, double* __restrict__ out) {
  const int lane = threadIdx.x;
  const double x = v[lane];
  for (int l = 0; l < 64; ++l) out[l * 64 + lane] = read_lane(x, l);
}

// out[q][lane] = pick_blocked<P>(a, lane P, q) for every interior index q (wave-uniform)
template <int P>
__global__ __launch_bounds__(64) void pick_blocked_kernel(const double* __restrict__ a, double* __restrict__ out) {
  const int lane = threadIdx.x;
  double r[P];
#pragma unroll
  for (int j = 0; j < P; ++j) r[j] = a[lane * P + j];
  for (int q = 0; q < 64 * P; ++q) out[q * 64 + lane] = pick_blocked<P>(r, lane * P, q);
}

// The exchanges of the column-lane Newton kernels (pnp_lane_cols.h; lane = 2 W point + W direction + column lane).  bcast[Q][lane]: the
// value of column lane Q of the lane's own point and direction; other[lane]: the same column lane of the other direction; sum[lane]: the
// sum over the column lanes of the lane's direction
template <int W>
__global__ __launch_bounds__(64) void col_lanes_kernel(const double* __restrict__ v, double* __restrict__ bcast, double* __restrict__ other,
                                                       double* __restrict__ sum) {
  const int lane = threadIdx.x;
  const double x = v[lane];
#pragma unroll
  for (int Q = 0; Q < W; ++Q) bcast[Q * 64 + lane] = lane::col_bcast_sel<W>(Q, x);
  other[lane] = lane::other_dir<W>(x);
  sum[lane] = lane::col_sum<W>(x);
}

template <bool BC>
__global__ __launch_bounds__(64) void wave_scan_kernel(const double* __restrict__ v, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  out[i] = BC ? wave_scan_incl_bc(v[i]) : wave_scan_incl(v[i]);
}

// LDS: the 128-double strip of blocked_scan (the scan sets its own guards; the strip is zeroed all the same)
template <int P, bool REV>
__global__ __launch_bounds__(64) void blocked_scan_kernel(const double* __restrict__ x, double* __restrict__ xo, double* __restrict__ total,
                                                          double* __restrict__ base) {
  __shared__ double X[128];
  const int lane = threadIdx.x;
  X[lane] = 0.0;
  X[lane + 64] = 0.0;
  __syncthreads();
  const int64_t o = (int64_t)blockIdx.x * 64 * P + lane * P;
  double r[P];
#pragma unroll
  for (int j = 0; j < P; ++j) r[j] = x[o + j];
  double t, b;
  blocked_scan<P, REV>(r, X, lane, t, b);
#pragma unroll
  for (int j = 0; j < P; ++j) xo[o + j] = r[j];
  total[blockIdx.x * 64 + lane] = t;
  base[blockIdx.x * 64 + lane] = b;
}

// LDS: the 256 doubles of blocked_scan_sum, zeroed (it sets only the left guards and reads only those)
template <int P>
__global__ __launch_bounds__(64) void blocked_scan_sum_kernel(const double* __restrict__ x, const double* __restrict__ w, double* __restrict__ xo,
                                                              double* __restrict__ total, double* __restrict__ base, double* __restrict__ wtotal) {
  __shared__ double X[256];
  const int lane = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) X[lane + 64 * q] = 0.0;
  __syncthreads();
  const int64_t o = (int64_t)blockIdx.x * 64 * P + lane * P;
  double r[P];
#pragma unroll
  for (int j = 0; j < P; ++j) r[j] = x[o + j];
  double t, b, wt;
  blocked_scan_sum<P>(r, w[blockIdx.x * 64 + lane], X, lane, t, b, wt);
#pragma unroll
  for (int j = 0; j < P; ++j) xo[o + j] = r[j];
  total[blockIdx.x * 64 + lane] = t;
  base[blockIdx.x * 64 + lane] = b;
  wtotal[blockIdx.x * 64 + lane] = wt;
}

// G systems of 64 P rows per workgroup, a / c / d laid out [case][g][row].  LDS: G strips of XSTRIDE = 384 doubles (three arrays of 128:
// 32 guard slots on either side of the 64 lanes), zeroed before use -- the contract of tridiag_wave is that the guards read zero.
constexpr int XSTRIDE = 384;
template <int P, int G, bool DPP1>
__global__ __launch_bounds__(64) void tridiag_kernel(const double* __restrict__ A, const double* __restrict__ C, const double* __restrict__ D,
                                                     double* __restrict__ Xo) {
  __shared__ double X[G * XSTRIDE];
  const int lane = threadIdx.x;
  for (int i = lane; i < G * XSTRIDE; i += 64) X[i] = 0.0;
  __syncthreads();
  double a[G][P], c[G][P], d[G][P];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t o = ((int64_t)blockIdx.x * G + g) * 64 * P + lane * P;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      a[g][j] = A[o + j];
      c[g][j] = C[o + j];
      d[g][j] = D[o + j];
    }
  }
  tridiag_wave<P, G, DPP1>(a, c, d, X, XSTRIDE, lane);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t o = ((int64_t)blockIdx.x * G + g) * 64 * P + lane * P;
#pragma unroll
    for (int j = 0; j < P; ++j) Xo[o + j] = d[g][j];
  }
}

// ---- rows and windows: one wave, one workgroup.  Every device buffer a load or store helper touches here holds at least row_alloc<P>()
// ---- (rows) or win_alloc<P>() (windows) doubles: the largest byte offset a lane can form -- 63*16 + (IT-1)*1024 + 16 for the row
// ---- helpers, lane*P*8 + 8 + (P/2)*16 (stores) and lane*P*8 + (P/2+1)*16 (loads) for the windows -- lies inside the allocation, so the
// ---- hardware range check of the buffer resource is what decides the result and a failure of it is a wrong value, never an access
// ---- outside the allocation.  The host side fills the slack behind the resource's end with canaries. ------------------------------------
template <int P>
constexpr int row_alloc() {
  return 128 * RowRegs<P>::IT;
}
template <int P>
constexpr int win_alloc() {
  return 64 * P + 2;
}
constexpr double LDS_FILL = -777.0;   // what the staged row holds before load_row: a slot the load did not write shows it

// LDS: rowbuf_doubles<P>() per staged row.  out[i] = slot pidx<P>(i) of the staged row, i < row_alloc<P>()
template <int P>
__global__ __launch_bounds__(64) void load_row_kernel(const double* __restrict__ src, int ldx, double* __restrict__ out) {
  __shared__ double buf[rowbuf_doubles<P>()];
  const int lane = threadIdx.x;
  for (int i = lane; i < rowbuf_doubles<P>(); i += 64) buf[i] = LDS_FILL;
  __syncthreads();
  load_row<P>(src, buf, ldx, lane);
  __syncthreads();
  for (int i = lane; i < row_alloc<P>(); i += 64) out[i] = buf[pidx<P>(i)];
}

template <int P, int AUX>
__global__ __launch_bounds__(64) void store_row_kernel(const double* __restrict__ vals, double* __restrict__ dst, int ldx) {
  __shared__ double buf[rowbuf_doubles<P>()];
  const int lane = threadIdx.x;
  for (int i = lane; i < rowbuf_doubles<P>(); i += 64) buf[i] = LDS_FILL;
  __syncthreads();
  for (int i = lane; i < row_alloc<P>(); i += 64) buf[pidx<P>(i)] = vals[i];
  __syncthreads();
  store_row<P, AUX>(dst, buf, ldx, lane);
}

// w[lane][0 .. P+2) = the window of lane `lane` through a resource of nrec doubles.  POST: post::load_win (P = 1 too), else
// pnp::load_window<P, AUX> (P even)
template <int P, int AUX, bool POST>
__global__ __launch_bounds__(64) void load_window_kernel(const double* __restrict__ row, int nrec, double* __restrict__ w) {
  const int lane = threadIdx.x;
  const __amdgpu_buffer_rsrc_t r = row_rsrc(row, nrec);
  double win[P + 2];
  if constexpr (POST) post::load_win<P>(r, win, lane);
  else load_window<P, AUX>(r, win, lane);
#pragma unroll
  for (int q = 0; q < P + 2; ++q) w[lane * (P + 2) + q] = win[q];
}

// MODE 0: pnp::store_rows<P> of the own values v[lane][1 .. P];  MODE 1: post::store_blocked as store_point_row calls it (the same values at
// byte (lane P + 1) 8);  MODE 2: as store_edge_row calls it (v[lane][0 .. P-1] at byte lane P 8).  v: [64][P + 2]
template <int P, int MODE>
__global__ __launch_bounds__(64) void store_window_kernel(const double* __restrict__ v, double* __restrict__ dst, int nrec) {
  const int lane = threadIdx.x;
  const __amdgpu_buffer_rsrc_t r = row_rsrc(dst, nrec);
  double win[P + 2];
#pragma unroll
  for (int q = 0; q < P + 2; ++q) win[q] = v[lane * (P + 2) + q];
  if constexpr (MODE == 0) {
    double own[P];
#pragma unroll
    for (int j = 0; j < P; ++j) own[j] = win[j + 1];
    store_rows<P>(r, own, lane);
  } else if constexpr (MODE == 1) {
    post::store_blocked<P, 1, P + 2>(r, win, (lane * P + 1) * 8);
  } else {
    double e[P + 1];
#pragma unroll
    for (int j = 0; j < P + 1; ++j) e[j] = win[j];
    post::store_blocked<P, 0, P + 1>(r, e, lane * P * 8);
  }
}

// ---- the damped Newton update of the physical mode (pnp_math.h), one row of N species and the potential per thread ------------------------
// in: c, du, cb, vol [n][N]; lam, dphi, dphi_max [n].  out: cf = the floored steps and cn = the row after both clips [n][N]; per row
// row [n][4]: backtrack taken (0 / 1), theta (0 where it is not taken), the largest scaled update of the row's species and the change of its
// potential (infinite for a NaN); damp [n] = newton_damping(that change, dphi_max)
template <int N>
__global__ __launch_bounds__(256) void newton_rule_kernel(const double* __restrict__ c, const double* __restrict__ du, const double* __restrict__ cb,
                                                          const double* __restrict__ vol, const double* __restrict__ lam, const double* __restrict__ dphi,
                                                          const double* __restrict__ dphi_max, double* __restrict__ cf, double* __restrict__ cn,
                                                          double* __restrict__ row, double* __restrict__ damp, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double cc[N], dd[N], out[N];
  double f_old = 0.0, f_new = 0.0, upd = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    cc[k] = c[i * N + k];
    dd[k] = du[i * N + k];
    const double f = newton_floor_step(lam[i], dd[k], cc[k]);
    cf[i * N + k] = f;
    f_old = __builtin_fma(vol[i * N + k], cc[k], f_old);
    f_new = __builtin_fma(vol[i * N + k], f, f_new);
    upd = newton_norm_species(upd, dd[k], cc[k], cb[i * N + k]);
  }
  double theta = 0.0;
  const bool back = newton_free_volume(f_old, f_new, theta);
  newton_clip_row<N, true>(lam[i], dd, cc, vol + i * N, out);
#pragma unroll
  for (int k = 0; k < N; ++k) cn[i * N + k] = out[k];
  const double mphi = newton_norm_phi(0.0, dphi[i]);
  row[i * 4 + 0] = back ? 1.0 : 0.0;
  row[i * 4 + 1] = back ? theta : 0.0;
  row[i * 4 + 2] = upd;
  row[i * 4 + 3] = mphi;
  damp[i] = newton_damping(mphi, dphi_max[i]);
}

// in [n]: lam, upd, upd_prev, tol, estimate (0 / 1).  out [n]: accepted (0 / 1) and upd_prev after the call
__global__ __launch_bounds__(256) void newton_accept_kernel(const double* __restrict__ lam, const double* __restrict__ upd, const double* __restrict__ upd_prev,
                                                            const double* __restrict__ tol, const double* __restrict__ estimate,
                                                            double* __restrict__ accept, double* __restrict__ prev_out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double prev = upd_prev[i];
  accept[i] = newton_accept(lam[i], upd[i], prev, tol[i], estimate[i] != 0.0) ? 1.0 : 0.0;
  prev_out[i] = prev;
}

// ---- the per-lane LU of pnp_kin.h: one wave, one system of order T with two right-hand sides per lane ------------------------------------
// A: [64][T][T], b: [64][2][T].  LDS as the libraries lay it out, [slot][lane]: J in slots 0 .. T T - 1, the right-hand sides in the 2 T slots
// behind (dynamic, lu_lds_bytes(T)).  lu: [64][T][T] the factors; meta: [64][2] the packed pivot rows and the bad-pivot flag; x: [64][2][T].
// This source sets no contraction pragma: the header's functions carry their own
__global__ __launch_bounds__(64) void lu_kernel(const double* __restrict__ A, const double* __restrict__ b, int T, double* __restrict__ lu,
                                                uint64_t* __restrict__ meta, double* __restrict__ x) {
  extern __shared__ double lu_lds[];
  const int lane = threadIdx.x;
  double* J = lu_lds + lane;
  double* rhs = J + T * T * 64;
  for (int e = 0; e < T * T; ++e) J[e * 64] = A[lane * T * T + e];
  for (int e = 0; e < 2 * T; ++e) rhs[e * 64] = b[lane * 2 * T + e];
  uint64_t pivs = 0;
  const bool bad = kin::factor(J, T, pivs);
  kin::substitute(J, rhs, T, pivs);
  kin::substitute(J, rhs + T * 64, T, pivs);
  for (int e = 0; e < T * T; ++e) lu[lane * T * T + e] = J[e * 64];
  for (int e = 0; e < 2 * T; ++e) x[lane * 2 * T + e] = rhs[e * 64];
  meta[lane * 2] = pivs;
  meta[lane * 2 + 1] = bad ? 1 : 0;
}
static size_t lu_lds_bytes(int T) { return (size_t)(T * T + 2 * T) * 64 * sizeof(double); }

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct Buf {
  void* p = nullptr;
  ~Buf() {
    if (p) (void)hipFree(p);
  }
  double* d() const { return (double*)p; }
};

#define CATUNIT_HIP(call)                        \
  do {                                           \
    hipError_t e_ = (call);                      \
    if (e_ != hipSuccess) return (int)e_;        \
  } while (0)

static int dev_alloc(Buf& b, size_t doubles) {
  CATUNIT_HIP(hipMalloc(&b.p, (doubles ? doubles : 1) * sizeof(double)));
  return 0;
}
static int dev_upload(Buf& b, const double* host, size_t doubles) {
  if (int e = dev_alloc(b, doubles)) return e;
  if (doubles) CATUNIT_HIP(hipMemcpy(b.p, host, doubles * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}
static int dev_download(double* host, const Buf& b, size_t doubles) {
  if (doubles) CATUNIT_HIP(hipMemcpy(host, b.p, doubles * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
static int finish() {
  CATUNIT_HIP(hipGetLastError());
  CATUNIT_HIP(hipDeviceSynchronize());
  return 0;
}
#define CATUNIT_TRY(expr)      \
  do {                         \
    if (int e_ = (expr)) return e_; \
  } while (0)

constexpr int EINVAL_ = (int)hipErrorInvalidValue;

// f(ic<P>) for the P of the five shapes; false for any other P
template <class F>
static bool with_p(int P, F&& f) {
  switch (P) {
    case 1: f(post::ic<1>()); return true;
    case 2: f(post::ic<2>()); return true;
    case 4: f(post::ic<4>()); return true;
    case 8: f(post::ic<8>()); return true;
    case 16: f(post::ic<16>()); return true;
  }
  return false;
}

template <int P, int G>
static void launch_tridiag(bool dpp1, int ncase, const double* a, const double* c, const double* d, double* x) {
  if (dpp1) tridiag_kernel<P, G, true><<<ncase, 64>>>(a, c, d, x);
  else tridiag_kernel<P, G, false><<<ncase, 64>>>(a, c, d, x);
}

}  // namespace catunit

using namespace catunit;

extern "C" {

// y[i] = fn(x[i]): fn 0 fast_rcp, 1 fast_rcp2, 2 nrcp, 3 expm1_sc, 4 log1p_sc, 5 post::bernoulli
__attribute__((visibility("default"))) int catunit_scalar(int fn, const double* x, double* y, int n) {
  if (!x || !y || n < 0 || fn < 0 || fn >= FN_COUNT) return EINVAL_;
  if (n == 0) return 0;
  Buf dx, dy;
  CATUNIT_TRY(dev_upload(dx, x, n));
  CATUNIT_TRY(dev_alloc(dy, n));
  const int blocks = (n + 255) / 256;
  switch (fn) {
    case FN_FAST_RCP: scalar_kernel<FN_FAST_RCP><<<blocks, 256>>>(dx.d(), dy.d(), n); break;
    case FN_FAST_RCP2: scalar_kernel<FN_FAST_RCP2><<<blocks, 256>>>(dx.d(), dy.d(), n); break;
    case FN_NRCP: scalar_kernel<FN_NRCP><<<blocks, 256>>>(dx.d(), dy.d(), n); break;
    case FN_EXPM1: scalar_kernel<FN_EXPM1><<<blocks, 256>>>(dx.d(), dy.d(), n); break;
    case FN_LOG1P: scalar_kernel<FN_LOG1P><<<blocks, 256>>>(dx.d(), dy.d(), n); break;
    default: scalar_kernel<FN_BERNOULLI><<<blocks, 256>>>(dx.d(), dy.d(), n); break;
  }
  CATUNIT_TRY(finish());
  return dev_download(y, dy, n);
}

// B[i], dB[i] from lane_edge_flux(u[i], 1, 0, 1)
__attribute__((visibility("default"))) int catunit_edge_flux(const double* u, double* B, double* dB, int n) {
  if (!u || !B || !dB || n < 0) return EINVAL_;
  if (n == 0) return 0;
  Buf du, db, dd;
  CATUNIT_TRY(dev_upload(du, u, n));
  CATUNIT_TRY(dev_alloc(db, n));
  CATUNIT_TRY(dev_alloc(dd, n));
  edge_flux_kernel<<<(n + 255) / 256, 256>>>(du.d(), db.d(), dd.d(), n);
  CATUNIT_TRY(finish());
  CATUNIT_TRY(dev_download(B, db, n));
  return dev_download(dB, dd, n);
}

// v, prev, next: [ncase][64]
__attribute__((visibility("default"))) int catunit_wave_moves(const double* v, double old, double* prev, double* next, int ncase) {
  if (!v || !prev || !next || ncase < 1) return EINVAL_;
  const size_t n = (size_t)ncase * 64;
  Buf dv, dp, dn;
  CATUNIT_TRY(dev_upload(dv, v, n));
  CATUNIT_TRY(dev_alloc(dp, n));
  CATUNIT_TRY(dev_alloc(dn, n));
  wave_moves_kernel<<<ncase, 64>>>(dv.d(), old, dp.d(), dn.d());
  CATUNIT_TRY(finish());
  CATUNIT_TRY(dev_download(prev, dp, n));
  return dev_download(next, dn, n);
}

// v: [64]; out: [64 (l)][64 (lane)]
__attribute__((visibility("default"))) int catunit_read_lane(const double* v, double* out) {
  if (!v || !out) return EINVAL_;
  Buf dv, dout;
  CATUNIT_TRY(dev_upload(dv, v, 64));
  CATUNIT_TRY(dev_alloc(dout, 64 * 64));
  read_lane_kernel<<<1, 64>>>(dv.d(), dout.d());
  CATUNIT_TRY(finish());
  return dev_download(out, dout, 64 * 64);
}

// v, other, sum: [64]; bcast: [W][64]; W 2 or 4
__attribute__((visibility("default"))) int catunit_col_lanes(int W, const double* v, double* bcast, double* other, double* sum) {
  if (!v || !bcast || !other || !sum || (W != 2 && W != 4)) return EINVAL_;
  Buf dv, db, dO, ds;
  CATUNIT_TRY(dev_upload(dv, v, 64));
  CATUNIT_TRY(dev_alloc(db, (size_t)W * 64));
  CATUNIT_TRY(dev_alloc(dO, 64));
  CATUNIT_TRY(dev_alloc(ds, 64));
  if (W == 2) col_lanes_kernel<2><<<1, 64>>>(dv.d(), db.d(), dO.d(), ds.d());
  else col_lanes_kernel<4><<<1, 64>>>(dv.d(), db.d(), dO.d(), ds.d());
  CATUNIT_TRY(finish());
  CATUNIT_TRY(dev_download(bcast, db, (size_t)W * 64));
  CATUNIT_TRY(dev_download(other, dO, 64));
  return dev_download(sum, ds, 64);
}

// a: [64 P]; out: [64 P (q)][64 (lane)]
__attribute__((visibility("default"))) int catunit_pick_blocked(int P, const double* a, double* out) {
  if (!a || !out) return EINVAL_;
  Buf da, dout;
  int rc = 0;
  const bool ok = with_p(P, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    if ((rc = dev_upload(da, a, 64 * PP)) || (rc = dev_alloc(dout, (size_t)64 * PP * 64))) return;
    pick_blocked_kernel<PP><<<1, 64>>>(da.d(), dout.d());
    if ((rc = finish())) return;
    rc = dev_download(out, dout, (size_t)64 * PP * 64);
  });
  return ok ? rc : EINVAL_;
}

// v, out: [ncase][64]; bc: wave_scan_incl_bc instead of wave_scan_incl
__attribute__((visibility("default"))) int catunit_wave_scan(int bc, const double* v, double* out, int ncase) {
  if (!v || !out || ncase < 1) return EINVAL_;
  const size_t n = (size_t)ncase * 64;
  Buf dv, dout;
  CATUNIT_TRY(dev_upload(dv, v, n));
  CATUNIT_TRY(dev_alloc(dout, n));
  if (bc) wave_scan_kernel<true><<<ncase, 64>>>(dv.d(), dout.d());
  else wave_scan_kernel<false><<<ncase, 64>>>(dv.d(), dout.d());
  CATUNIT_TRY(finish());
  return dev_download(out, dout, n);
}

// x, xo: [ncase][64 P]; total, base: [ncase][64] (one value per lane)
__attribute__((visibility("default"))) int catunit_blocked_scan(int P, int rev, const double* x, double* xo, double* total, double* base, int ncase) {
  if (!x || !xo || !total || !base || ncase < 1) return EINVAL_;
  Buf dx, dxo, dt, db;
  int rc = 0;
  const bool ok = with_p(P, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    const size_t n = (size_t)ncase * 64 * PP, nl = (size_t)ncase * 64;
    if ((rc = dev_upload(dx, x, n)) || (rc = dev_alloc(dxo, n)) || (rc = dev_alloc(dt, nl)) || (rc = dev_alloc(db, nl))) return;
    if (rev) blocked_scan_kernel<PP, true><<<ncase, 64>>>(dx.d(), dxo.d(), dt.d(), db.d());
    else blocked_scan_kernel<PP, false><<<ncase, 64>>>(dx.d(), dxo.d(), dt.d(), db.d());
    if ((rc = finish())) return;
    if ((rc = dev_download(xo, dxo, n)) || (rc = dev_download(total, dt, nl))) return;
    rc = dev_download(base, db, nl);
  });
  return ok ? rc : EINVAL_;
}

// x, xo: [ncase][64 P]; w, total, base, wtotal: [ncase][64]
__attribute__((visibility("default"))) int catunit_blocked_scan_sum(int P, const double* x, const double* w, double* xo, double* total, double* base,
                                                                    double* wtotal, int ncase) {
  if (!x || !w || !xo || !total || !base || !wtotal || ncase < 1) return EINVAL_;
  Buf dx, dw, dxo, dt, db, dwt;
  int rc = 0;
  const bool ok = with_p(P, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    const size_t n = (size_t)ncase * 64 * PP, nl = (size_t)ncase * 64;
    if ((rc = dev_upload(dx, x, n)) || (rc = dev_upload(dw, w, nl)) || (rc = dev_alloc(dxo, n)) || (rc = dev_alloc(dt, nl)) ||
        (rc = dev_alloc(db, nl)) || (rc = dev_alloc(dwt, nl)))
      return;
    blocked_scan_sum_kernel<PP><<<ncase, 64>>>(dx.d(), dw.d(), dxo.d(), dt.d(), db.d(), dwt.d());
    if ((rc = finish())) return;
    if ((rc = dev_download(xo, dxo, n)) || (rc = dev_download(total, dt, nl)) || (rc = dev_download(base, db, nl))) return;
    rc = dev_download(wtotal, dwt, nl);
  });
  return ok ? rc : EINVAL_;
}

// a, c, d, x: [ncase][G][64 P]; G in 1 .. 3
__attribute__((visibility("default"))) int catunit_tridiag(int P, int G, int dpp1, const double* a, const double* c, const double* d, double* x,
                                                           int ncase) {
  if (!a || !c || !d || !x || ncase < 1 || G < 1 || G > 3) return EINVAL_;
  Buf da, dc, dd, dx;
  int rc = 0;
  const bool ok = with_p(P, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    const size_t n = (size_t)ncase * G * 64 * PP;
    if ((rc = dev_upload(da, a, n)) || (rc = dev_upload(dc, c, n)) || (rc = dev_upload(dd, d, n)) || (rc = dev_alloc(dx, n))) return;
    if (G == 1) launch_tridiag<PP, 1>(dpp1 != 0, ncase, da.d(), dc.d(), dd.d(), dx.d());
    else if (G == 2) launch_tridiag<PP, 2>(dpp1 != 0, ncase, da.d(), dc.d(), dd.d(), dx.d());
    else launch_tridiag<PP, 3>(dpp1 != 0, ncase, da.d(), dc.d(), dd.d(), dx.d());
    if ((rc = finish())) return;
    rc = dev_download(x, dx, n);
  });
  return ok ? rc : EINVAL_;
}

// c, du, cb, vol, cf, cn: [n][N]; lam, dphi, dphi_max, damp: [n]; row: [n][4] (newton_rule_kernel); N 1, 2, 7 or 8
__attribute__((visibility("default"))) int catunit_newton_rule(int N, int n, const double* c, const double* du, const double* cb, const double* vol,
                                                               const double* lam, const double* dphi, const double* dphi_max, double* cf, double* cn,
                                                               double* row, double* damp) {
  if (!c || !du || !cb || !vol || !lam || !dphi || !dphi_max || !cf || !cn || !row || !damp || n < 1 || (N != 1 && N != 2 && N != 7 && N != 8)) return EINVAL_;
  Buf dc, ddu, dcb, dvol, dlam, dph, dmx, dcf, dcn, drow, ddamp;
  const size_t nn = (size_t)n * N;
  CATUNIT_TRY(dev_upload(dc, c, nn));
  CATUNIT_TRY(dev_upload(ddu, du, nn));
  CATUNIT_TRY(dev_upload(dcb, cb, nn));
  CATUNIT_TRY(dev_upload(dvol, vol, nn));
  CATUNIT_TRY(dev_upload(dlam, lam, n));
  CATUNIT_TRY(dev_upload(dph, dphi, n));
  CATUNIT_TRY(dev_upload(dmx, dphi_max, n));
  CATUNIT_TRY(dev_alloc(dcf, nn));
  CATUNIT_TRY(dev_alloc(dcn, nn));
  CATUNIT_TRY(dev_alloc(drow, (size_t)n * 4));
  CATUNIT_TRY(dev_alloc(ddamp, n));
  const int blocks = (n + 255) / 256;
  switch (N) {
#define CATUNIT_RULE(NN)                                                                                                                   \
  case NN:                                                                                                                                 \
    newton_rule_kernel<NN><<<blocks, 256>>>(dc.d(), ddu.d(), dcb.d(), dvol.d(), dlam.d(), dph.d(), dmx.d(), dcf.d(), dcn.d(), drow.d(), \
                                            ddamp.d(), n);                                                                                 \
    break;
    CATUNIT_RULE(1)
    CATUNIT_RULE(2)
    CATUNIT_RULE(7)
    CATUNIT_RULE(8)
#undef CATUNIT_RULE
    default: return EINVAL_;
  }
  CATUNIT_TRY(finish());
  CATUNIT_TRY(dev_download(cf, dcf, nn));
  CATUNIT_TRY(dev_download(cn, dcn, nn));
  CATUNIT_TRY(dev_download(row, drow, (size_t)n * 4));
  return dev_download(damp, ddamp, n);
}

// lam, upd, upd_prev, tol, estimate, accept, prev_out: [n] (newton_accept_kernel)
__attribute__((visibility("default"))) int catunit_newton_accept(int n, const double* lam, const double* upd, const double* upd_prev, const double* tol,
                                                                 const double* estimate, double* accept, double* prev_out) {
  if (!lam || !upd || !upd_prev || !tol || !estimate || !accept || !prev_out || n < 1) return EINVAL_;
  Buf dl, du, dp, dt, de, da, dpo;
  CATUNIT_TRY(dev_upload(dl, lam, n));
  CATUNIT_TRY(dev_upload(du, upd, n));
  CATUNIT_TRY(dev_upload(dp, upd_prev, n));
  CATUNIT_TRY(dev_upload(dt, tol, n));
  CATUNIT_TRY(dev_upload(de, estimate, n));
  CATUNIT_TRY(dev_alloc(da, n));
  CATUNIT_TRY(dev_alloc(dpo, n));
  newton_accept_kernel<<<(n + 255) / 256, 256>>>(dl.d(), du.d(), dp.d(), dt.d(), de.d(), da.d(), dpo.d(), n);
  CATUNIT_TRY(finish());
  CATUNIT_TRY(dev_download(accept, da, n));
  return dev_download(prev_out, dpo, n);
}

// A: [64][T][T]; b, x: [64][2][T]; lu: [64][T][T]; meta: [64][2] (lu_kernel); T in 1 .. 9
__attribute__((visibility("default"))) int catunit_lu(int T, const double* A, const double* b, double* lu, uint64_t* meta, double* x) {
  if (!A || !b || !lu || !meta || !x || T < 1 || T > kin::MAXT) return EINVAL_;
  static_assert(sizeof(uint64_t) == sizeof(double), "meta travels in a buffer of doubles");
  Buf dA, db, dlu, dmeta, dx;
  const size_t nA = (size_t)64 * T * T, nb = (size_t)64 * 2 * T;
  CATUNIT_TRY(dev_upload(dA, A, nA));
  CATUNIT_TRY(dev_upload(db, b, nb));
  CATUNIT_TRY(dev_alloc(dlu, nA));
  CATUNIT_TRY(dev_alloc(dmeta, 128));
  CATUNIT_TRY(dev_alloc(dx, nb));
  const size_t lds = lu_lds_bytes(T);
  if (lds > 48 * 1024) CATUNIT_HIP(hipFuncSetAttribute((const void*)lu_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  lu_kernel<<<1, 64, lds>>>(dA.d(), db.d(), T, dlu.d(), (uint64_t*)dmeta.p, dx.d());
  CATUNIT_TRY(finish());
  CATUNIT_TRY(dev_download(lu, dlu, nA));
  CATUNIT_HIP(hipMemcpy(meta, dmeta.p, 128 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return dev_download(x, dx, nb);
}

// doubles every row buffer (catunit_load_row, catunit_store_row) resp. window buffer (catunit_load_window, catunit_store_window) must hold
__attribute__((visibility("default"))) int catunit_row_alloc(int P) {
  int n = -1;
  with_p(P, [&](auto p) { n = row_alloc<decltype(p)::value>(); });
  return n;
}
__attribute__((visibility("default"))) int catunit_win_alloc(int P) {
  int n = -1;
  with_p(P, [&](auto p) { n = win_alloc<decltype(p)::value>(); });
  return n;
}

// src: [alloc] (the row, canaries behind it); out: [row_alloc(P)] = the staged LDS row read back through pidx<P>
__attribute__((visibility("default"))) int catunit_load_row(int P, const double* src, int alloc, int ldx, double* out) {
  if (!src || !out || ldx < 0) return EINVAL_;
  Buf ds, dout;
  int rc = 0;
  const bool ok = with_p(P, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    if (alloc < row_alloc<PP>() || ldx > alloc) {
      rc = EINVAL_;
      return;
    }
    if ((rc = dev_upload(ds, src, alloc)) || (rc = dev_alloc(dout, row_alloc<PP>()))) return;
    load_row_kernel<PP><<<1, 64>>>(ds.d(), ldx, dout.d());
    if ((rc = finish())) return;
    rc = dev_download(out, dout, row_alloc<PP>());
  });
  return ok ? rc : EINVAL_;
}

// vals: [row_alloc(P)] (the staged row); dst: [alloc], canaries on entry, the device buffer after the store on return; aux 0 or 2
__attribute__((visibility("default"))) int catunit_store_row(int P, int aux, const double* vals, double* dst, int alloc, int ldx) {
  if (!vals || !dst || ldx < 0 || (aux != 0 && aux != 2)) return EINVAL_;
  Buf dv, dd;
  int rc = 0;
  const bool ok = with_p(P, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    if (alloc < row_alloc<PP>() || ldx > alloc) {
      rc = EINVAL_;
      return;
    }
    if ((rc = dev_upload(dv, vals, row_alloc<PP>())) || (rc = dev_upload(dd, dst, alloc))) return;
    if (aux == 0) store_row_kernel<PP, 0><<<1, 64>>>(dv.d(), dd.d(), ldx);
    else store_row_kernel<PP, 2><<<1, 64>>>(dv.d(), dd.d(), ldx);
    if ((rc = finish())) return;
    rc = dev_download(dst, dd, alloc);
  });
  return ok ? rc : EINVAL_;
}

// row: [alloc]; the resource covers its first nrec doubles; w: [64][P + 2].  which 0: pnp::load_window<P, 0>, 1: pnp::load_window<P, 2>
// (both P even), 2: post::load_win<P>
__attribute__((visibility("default"))) int catunit_load_window(int P, int which, const double* row, int alloc, int nrec, double* w) {
  if (!row || !w || nrec < 0 || which < 0 || which > 2 || (which < 2 && P == 1)) return EINVAL_;
  Buf dr, dw;
  int rc = 0;
  const bool ok = with_p(P, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    if (alloc < win_alloc<PP>() || nrec > alloc) {
      rc = EINVAL_;
      return;
    }
    if ((rc = dev_upload(dr, row, alloc)) || (rc = dev_alloc(dw, 64 * (PP + 2)))) return;
    if (which == 2) load_window_kernel<PP, 0, true><<<1, 64>>>(dr.d(), nrec, dw.d());
    else if constexpr (PP > 1) {
      if (which == 0) load_window_kernel<PP, 0, false><<<1, 64>>>(dr.d(), nrec, dw.d());
      else load_window_kernel<PP, 2, false><<<1, 64>>>(dr.d(), nrec, dw.d());
    }
    if ((rc = finish())) return;
    rc = dev_download(w, dw, 64 * (PP + 2));
  });
  return ok ? rc : EINVAL_;
}

// v: [64][P + 2]; dst: [alloc], canaries on entry, the device buffer after the store on return; the resource covers nrec doubles.
// mode 0: pnp::store_rows<P> (P even), 1: post::store_blocked as for a point row, 2: as for an edge row
__attribute__((visibility("default"))) int catunit_store_window(int P, int mode, const double* v, double* dst, int alloc, int nrec) {
  if (!v || !dst || nrec < 0 || mode < 0 || mode > 2 || (mode == 0 && P == 1)) return EINVAL_;
  Buf dv, dd;
  int rc = 0;
  const bool ok = with_p(P, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    if (alloc < win_alloc<PP>() || nrec > alloc) {
      rc = EINVAL_;
      return;
    }
    if ((rc = dev_upload(dv, v, 64 * (PP + 2))) || (rc = dev_upload(dd, dst, alloc))) return;
    if (mode == 1) store_window_kernel<PP, 1><<<1, 64>>>(dv.d(), dd.d(), nrec);
    else if (mode == 2) store_window_kernel<PP, 2><<<1, 64>>>(dv.d(), dd.d(), nrec);
    else if constexpr (PP > 1) store_window_kernel<PP, 0><<<1, 64>>>(dv.d(), dd.d(), nrec);
    if ((rc = finish())) return;
    rc = dev_download(dst, dd, alloc);
  });
  return ok ? rc : EINVAL_;
}

}  // extern "C"
