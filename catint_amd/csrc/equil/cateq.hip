// libcatint_equil (include/catint_equil.h): the zero-flux state of the physical mode as a discrete size-modified Poisson-Boltzmann
// problem, solved on the device.  It shares no code with the Newton kernels: the formulas are restated here from the header.
// Context, validation frame, windows and row stores: csrc/pnp_post.h.  gfx950 / MI355X only.
//
// Layout (that of pnp_post.h): WY waves per operating point, thread t owns the P points t P + 1 .. t P + P and keeps the potential
// of its window t P .. t P + P + 1, the weights w_e of the P + 1 edges between them and pe v_i of its points in registers for the
// whole solve.  Persistent workgroups walk the operating points i, i + grid, ...  The grid rows are read once per workgroup (the
// same rows for every workgroup: L2); per operating point the kernel reads 2 + N doubles of parameters (uniform addresses: scalar
// loads) and writes the result once.  Nothing goes to memory between the iterations.
// One Newton iteration: every thread evaluates rho and d rho / d phi at its points (N exponentials per point, four points at a
// time for instruction-level parallelism), forms its P rows scaled to a unit diagonal, and the rows are solved by
// pnp::tridiag_wave (one wave) or by tridiag_wg below (2 / 4 waves: the same per-lane elimination, then parallel cyclic reduction
// over the workgroup's 128 / 256 interface rows through LDS).  The wall row is eliminated into the row of point 1 by thread 0; the
// bulk row is the identity and its update is 0.  Own points behind the bulk point (grids that do not fill the waves) are identity
// rows with a zero right-hand side.  No pivoting: the matrix is diagonally dominant (d rho / d phi <= 0 is enforced).
// The loop: max |dphi| goes through LDS (one value per wave) and every thread reads the same WY values, so the exit decision is
// workgroup-uniform and no wave can wait at a barrier another has left; the trip count is bounded by maxit whatever the data (a
// NaN never compares below tol).  Every row access goes through a buffer resource that ends at the row's end.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../../include/catint_equil.h"
#include "../pnp_post.h"

namespace cateq {

using namespace pnp::post;

constexpr int MAXS = CATEQ_MAX_SPECIES;
constexpr int LP = 2 + MAXS;   // doubles of parameters per operating point: phiM, phi_bulk, a0[MAXS] = c_bulk / (1 - phi0_bulk)

struct KArgs {
  int32_t N, nx, pitch, stern, maxit, pad_;
  int64_t n;              // operating points to solve
  const double* w;        // [nx - 1] dx / h_e
  const double* pv;       // [nx] pe v_i
  const double* lp;       // [n][LP]
  const double* sp;       // [MAXS][SPF] per species: q_k beta, q_k, q_k q_k beta, N_A a_k^3, vol_k q_k beta, 0
  double* oc;             // [n][N][pitch]
  double* ophi;           // [n][pitch]
  int32_t* oflag;         // [n][2] status, iterations
  double g, phi_pzc, tol, qbmax;   // dx C_S / eps
};
constexpr int SPF = 6;   // doubles per species of the table the kernel keeps in LDS; the last is a0 of the operating point at hand

__device__ __forceinline__ double boltzmann(double qb, double dphi) {
  const double u = -qb * dphi;
  return exp(fmin(fmax(u, -CATEQ_MAX_EXPONENT), CATEQ_MAX_EXPONENT));   // (a NaN becomes the lower clamp: the update stays NaN-free)
}

// a value every lane of the wave holds, moved to scalar registers: what depends on it (the exit of the Newton loop) is uniform for
// the compiler as well
__device__ __forceinline__ double uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// rho and min(d rho / d phi, 0) at C potentials (dphi = phi - phi_bulk)
template <int C, bool STERIC>
__device__ __forceinline__ void charge(int N, const double* sp, const double (&dphi)[C], double (&rho)[C], double (&drho)[C]) {
  double r1[C], r2[C], s[C], r3[C];
#pragma unroll
  for (int j = 0; j < C; ++j) r1[j] = r2[j] = s[j] = r3[j] = 0.0;
#pragma unroll 1
  for (int k = 0; k < N; ++k) {   // (uniform LDS addresses: broadcast reads)
    const double qb = sp[k * SPF], q = sp[k * SPF + 1], qqb = sp[k * SPF + 2], a0k = sp[k * SPF + 5];
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const double a = a0k * boltzmann(qb, dphi[j]);
      r1[j] = __builtin_fma(q, a, r1[j]);
      r2[j] = __builtin_fma(qqb, a, r2[j]);
      if constexpr (STERIC) {
        s[j] = __builtin_fma(sp[k * SPF + 3], a, s[j]);
        r3[j] = __builtin_fma(sp[k * SPF + 4], a, r3[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < C; ++j) {
    if constexpr (STERIC) {
      const double r = pnp::nrcp(1.0 + s[j]);
      rho[j] = r1[j] * r;
      drho[j] = fmin(__builtin_fma(rho[j], r3[j] * r, -r2[j] * r), 0.0);
    } else {
      rho[j] = r1[j];
      drho[j] = -r2[j];   // <= 0 always
    }
  }
}

// LDS doubles of the tridiagonal solve: the strips of pnp::tridiag_wave, or two sets (ping-pong: one barrier per exchange) of three
// arrays of T slots between two guards of T / 2 zeros
template <int WY>
constexpr int tri_doubles() { return WY == 1 ? 384 : 2 * 3 * 2 * 64 * WY; }

// pnp::tridiag_wave<P, 1> over the 64 WY lanes of a workgroup, WY > 1 (P > 1).  The guards of X are zero (the kernel sets them once;
// nothing here writes them).
template <int P, int WY>
__device__ __forceinline__ void tridiag_wg(double (&a)[1][P], double (&c)[1][P], double (&d)[1][P], double* X, int t) {
  constexpr int T = 64 * WY, ARR = 2 * T, SET = 3 * ARR;
  double* const X0 = X + T / 2 + t;
  int set = 0;
  const auto strip = [&]() {   // the next set's slot of this thread
    double* p = X0 + set * SET;
    set ^= 1;
    return p;
  };
#pragma unroll
  for (int i = 1; i < P - 1; ++i) {
    const double ai = a[0][i];
    const double bb = __builtin_fma(-ai, c[0][i - 1], 1.0);
    const double dd = __builtin_fma(-ai, d[0][i - 1], d[0][i]);
    const double vv = -ai * a[0][i - 1];
    const double r = pnp::fast_rcp(bb);
    a[0][i] = vv * r;
    d[0][i] = dd * r;
    c[0][i] = c[0][i] * r;
  }
#pragma unroll
  for (int i = P - 3; i >= 0; --i) {
    const double cs = c[0][i];
    d[0][i] = __builtin_fma(-cs, d[0][i + 1], d[0][i]);
    a[0][i] = __builtin_fma(-cs, a[0][i + 1], a[0][i]);
    c[0][i] = -cs * c[0][i + 1];
  }
  double ra, rc, rd;
  {   // the first interior row of the next lane closes this lane's interface row (the last lane reads the zero guard)
    double* p = strip();
    p[0] = a[0][0];
    p[ARR] = c[0][0];
    p[2 * ARR] = d[0][0];
    pnp::wg_sync<WY>();
    const double Vn0 = p[1], Wn0 = p[ARR + 1], dn0 = p[2 * ARR + 1];
    const double aL = a[0][P - 1], cL = c[0][P - 1];
    double rb = __builtin_fma(-aL, c[0][P - 2], 1.0);
    rb = __builtin_fma(-cL, Vn0, rb);
    const double rr = pnp::fast_rcp(rb);
    double tt = __builtin_fma(-aL, d[0][P - 2], d[0][P - 1]);
    tt = __builtin_fma(-cL, dn0, tt);
    ra = (-aL * a[0][P - 2]) * rr;
    rc = (-cL * Wn0) * rr;
    rd = tt * rr;
  }
#pragma unroll
  for (int s = 1; s < T; s <<= 1) {
    double* p = strip();
    p[0] = ra;
    p[ARR] = rc;
    p[2 * ARR] = rd;
    pnp::wg_sync<WY>();
    const double aL = p[-s], aR = p[s], cL = p[ARR - s], cR = p[ARR + s], dL = p[2 * ARR - s], dR = p[2 * ARR + s];
    double nb = __builtin_fma(-ra, cL, 1.0);
    nb = __builtin_fma(-rc, aR, nb);
    double nd = __builtin_fma(-ra, dL, rd);
    nd = __builtin_fma(-rc, dR, nd);
    const double na = -ra * aL, nc = -rc * cR;
    const double rr = pnp::fast_rcp(nb);
    ra = na * rr;
    rc = nc * rr;
    rd = nd * rr;
  }
  {
    double* p = strip();
    p[0] = rd;
    pnp::wg_sync<WY>();
    const double yL = p[-1];   // thread 0 reads the zero guard
#pragma unroll
    for (int i = 0; i < P - 1; ++i) {
      const double tt = __builtin_fma(-a[0][i], yL, d[0][i]);
      d[0][i] = __builtin_fma(-c[0][i], rd, tt);
    }
  }
  d[0][P - 1] = rd;
}

template <int P, int WY, bool STERIC>
__global__ __launch_bounds__(64 * WY) void pb_kernel(const KArgs A) {
  constexpr int T = 64 * WY, C = P < 4 ? P : 4;
  __shared__ __attribute__((aligned(16))) double tri[tri_doubles<WY>()];
  __shared__ __attribute__((aligned(16))) double sp[MAXS * SPF];   // the species table
  __shared__ double exl[T + 2], exf[T + 2], red[WY];   // last / first update of every thread between two zeros; max |dphi| per wave
  const int t = threadIdx.x;
  const int nx = A.nx, N = A.N, pitch = A.pitch;
  const bool tight = nx == T * P + 2;

  // the grid, once: edges t P .. t P + P and pe v of the own points; beyond the row the loads return 0
  double we[P + 2], pv[P + 2];
  load_win<P>(pnp::row_rsrc(A.w, nx - 1), we, t);
  load_win<P>(pnp::row_rsrc(A.pv, nx), pv, t);
  if constexpr (WY > 1) {   // the guards of tridiag_wg
#pragma unroll
    for (int q = 0; q < 6; ++q) tri[q * 2 * T + (t < T / 2 ? t : T + t)] = 0.0;
  }
  if (t == 0) exl[0] = exf[0] = exl[T + 1] = exf[T + 1] = 0.0;
  if (t < N * SPF) sp[t] = A.sp[t];

  for (int64_t i = blockIdx.x; i < A.n; i += gridDim.x) {
    const double* __restrict__ lp = A.lp + i * LP;
    const double phiM = uniform(lp[0]), phib = uniform(lp[1]);
    pnp::wg_sync<WY>();   // the previous operating point's reads of the table are done
    if (t < N) sp[t * SPF + 5] = lp[2 + t];
    pnp::wg_sync<WY>();
    double ph[P + 2];
#pragma unroll
    for (int j = 0; j < P + 2; ++j) ph[j] = phib;
    int it = 0, status = 1;
    while (it < A.maxit) {
      double a[1][P], c[1][P], d[1][P];
#pragma unroll
      for (int j0 = 0; j0 < P; j0 += C) {
        double dp[C], rho[C], drho[C];
#pragma unroll
        for (int jj = 0; jj < C; ++jj) dp[jj] = ph[j0 + jj + 1] - phib;
        charge<C, STERIC>(N, sp, dp, rho, drho);
#pragma unroll
        for (int jj = 0; jj < C; ++jj) {
          const int j = j0 + jj + 1;                 // window position; point t P + j
          const double sub = we[j - 1], sup = we[j];
          a[0][j - 1] = sub;
          c[0][j - 1] = sup;
          d[0][j - 1] = -(sup * (ph[j + 1] - ph[j]) - sub * (ph[j] - ph[j - 1]) + pv[j] * rho[jj]);   // -F
          rho[jj] = -(sup + sub) + pv[j] * drho[jj];                                                  // the diagonal
        }
#pragma unroll
        for (int jj = 0; jj < C; ++jj) {
          const int j = j0 + jj + 1;
          double diag = rho[jj];
          if (j == 1) {   // thread 0: the wall row d0 x0 + u0 x1 = r0 eliminated from the row of point 1
            const double d0 = A.stern ? -(we[0] + A.g) : 1.0, u0 = A.stern ? we[0] : 0.0;
            const double r0 = A.stern ? -(we[0] * (ph[1] - ph[0]) + A.g * (phiM - A.phi_pzc - ph[0])) : phiM - ph[0];
            const double m = a[0][0] * pnp::nrcp(d0);
            if (t == 0) {
              diag = __builtin_fma(-m, u0, diag);
              d[0][0] = __builtin_fma(-m, r0, d[0][0]);
              a[0][0] = 0.0;
            }
          }
          const int p = t * P + j;
          const bool inside = p <= nx - 2;
          const double r = pnp::nrcp(inside ? diag : 1.0);
          a[0][j - 1] = inside ? a[0][j - 1] * r : 0.0;
          c[0][j - 1] = p < nx - 2 ? c[0][j - 1] * r : 0.0;   // the bulk point's update is 0
          d[0][j - 1] = inside ? d[0][j - 1] * r : 0.0;
        }
      }
      if constexpr (WY == 1) pnp::tridiag_wave<P, 1>(a, c, d, tri, 0, t);
      else tridiag_wg<P, WY>(a, c, d, tri, t);

      // the wall's update (thread 0), the neighbours' updates and max |dphi|
      double dw[P + 2];
#pragma unroll
      for (int j = 0; j < P; ++j) dw[j + 1] = d[0][j];
      double m = 0.0;
#pragma unroll
      for (int j = 1; j <= P; ++j) m = fmax(m, fabs(dw[j]));
      double d0w;
      {
        const double d0 = A.stern ? -(we[0] + A.g) : 1.0, u0 = A.stern ? we[0] : 0.0;
        const double r0 = A.stern ? -(we[0] * (ph[1] - ph[0]) + A.g * (phiM - A.phi_pzc - ph[0])) : phiM - ph[0];
        d0w = (r0 - u0 * dw[1]) * pnp::nrcp(d0);
      }
      if (t == 0) m = fmax(m, fabs(d0w));
      m = isnan(m) ? INFINITY : m;   // fmax drops a NaN: keep the iteration from ending on one
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) m = fmax(m, __shfl_xor(m, s));
      exl[t + 1] = dw[P];
      exf[t + 1] = dw[1];
      if ((t & 63) == 0) red[t >> 6] = m;
      pnp::wg_sync<WY>();
      dw[0] = t == 0 ? d0w : exl[t];
      dw[P + 1] = exf[t + 2];
      double mm = red[0];
#pragma unroll
      for (int wv = 1; wv < WY; ++wv) mm = fmax(mm, red[wv]);
      const double upd = uniform(A.qbmax * mm);
      const double lam = upd > 2.0 ? 2.0 / upd : 1.0;
#pragma unroll
      for (int j = 0; j < P + 2; ++j) ph[j] = __builtin_fma(lam, dw[j], ph[j]);
      ++it;
      if (upd < A.tol) {   // workgroup-uniform: every thread read the same red[]
        status = 0;
        break;
      }
      if constexpr (WY == 1) pnp::lds_sync();   // (with more waves the barriers of the next solve separate the reads from the next writes)
    }

    // the result: phi, then one species row at a time
    double* prow = A.ophi + (size_t)i * pitch;
    store_point_row<P, T>(prow, ph, nx, t, tight);
    if (t < pitch - nx) prow[nx + t] = 0.0;
    double rs[P + 2];
#pragma unroll
    for (int j = 0; j < P + 2; ++j) rs[j] = 1.0;
    if constexpr (STERIC) {
#pragma unroll
      for (int j = 0; j < P + 2; ++j) rs[j] = 0.0;
#pragma unroll 1
      for (int k = 0; k < N; ++k) {
        const double va = sp[k * SPF + 3] * sp[k * SPF + 5], qb = sp[k * SPF];
#pragma unroll
        for (int j = 0; j < P + 2; ++j) rs[j] = __builtin_fma(va, boltzmann(qb, ph[j] - phib), rs[j]);
      }
#pragma unroll
      for (int j = 0; j < P + 2; ++j) rs[j] = pnp::nrcp(1.0 + rs[j]);
    }
#pragma unroll 1
    for (int k = 0; k < N; ++k) {
      const double a0k = sp[k * SPF + 5], qb = sp[k * SPF];
      double ck[P + 2];
#pragma unroll
      for (int j = 0; j < P + 2; ++j) ck[j] = a0k * boltzmann(qb, ph[j] - phib) * rs[j];
      double* crow = A.oc + ((size_t)i * N + k) * pitch;
      store_point_row<P, T>(crow, ck, nx, t, tight);
      if (t < pitch - nx) crow[nx + t] = 0.0;
    }
    if (t == 0) {
      A.oflag[2 * i] = status;
      A.oflag[2 * i + 1] = it;
    }
  }
}

// The instance on stream st.  max_waves == 0: as many workgroups as the device holds at once (persistent: each walks i, i + grid,
// ...), no more than there are operating points.
template <int P, int WY, bool STERIC>
static hipError_t launch(const KArgs& a, int max_waves, int cus, hipStream_t st) {
  const auto kernel = pb_kernel<P, WY, STERIC>;
  int64_t blocks = max_waves / WY;
  if (max_waves == 0) {
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64 * WY, 0);
    if (e != hipSuccess) return e;
    blocks = (int64_t)std::max(per_cu, 1) * cus;
  }
  blocks = std::min(std::max<int64_t>(blocks, 1), a.n);
  hipLaunchKernelGGL(kernel, dim3((int)blocks), dim3(64 * WY), 0, st, a);
  return hipSuccess;
}

}  // namespace cateq

static_assert(CATEQ_OK == pnp::post::OK && CATEQ_EINVAL == pnp::post::ERR_INVAL && CATEQ_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATEQ_EDEVICE == pnp::post::ERR_DEVICE && CATEQ_MAX_NX == pnp::post::MAX_NX && CATEQ_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_equil.h and pnp_post.h disagree");

struct cateq_ctx : pnp::post::Ctx {};

extern "C" {

int cateq_create(int32_t device, cateq_ctx** out) { return pnp::post::create("cateq_create", device, out); }
void cateq_destroy(cateq_ctx* ctx) { pnp::post::destroy(ctx); }
const char* cateq_last_error(const cateq_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* cateq_last_kernel(const cateq_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float cateq_last_kernel_ms(const cateq_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int cateq_solve(cateq_ctx* ctx, const pnp_device_view* view, const cateq_params* p, const cateq_outputs* out) {
  using namespace cateq;
  static const char entry[] = "cateq_solve";
  if (!ctx) return CATEQ_EINVAL;
  if (!view || !p || !out) return fail(ctx, CATEQ_EINVAL, "cateq_solve: null argument");
  {
    // check_view's frame wants the three pointers every library of this family requires; this one has no diffusion coefficients
    // (the equilibrium does not depend on them), so the charges stand in for them there
    struct Frame {
      int32_t struct_size;
      const double *D, *charges, *x;
    } f = {p->struct_size == (int32_t)sizeof(cateq_params) ? (int32_t)sizeof(Frame) : -1, p->charges, p->charges, p->x};
    if (const int rc = check_view(ctx, entry, "cateq_params", view, &f, out)) {
      if (!p->charges || !p->x) return fail(ctx, CATEQ_EINVAL, "cateq_solve: charges and x are required");
      return rc;
    }
  }
  const int N = view->nspecies, nx = view->nx;
  char msg[256];
  if (p->max_waves < 0) return fail(ctx, CATEQ_EINVAL, "cateq_solve: negative max_waves");
  const auto posfin = [](double v) { return v > 0.0 && std::isfinite(v); };
  if (!posfin(p->beta) || !posfin(p->eps) || !posfin(p->dx) || !posfin(p->tol))
    return fail(ctx, CATEQ_EINVAL, "cateq_solve: beta, eps, dx and tol must be positive and finite");
  if (p->maxit < 1) return fail(ctx, CATEQ_EINVAL, "cateq_solve: maxit < 1");
  if (p->wall_bc != CATEQ_WALL_DIRICHLET && p->wall_bc != CATEQ_WALL_STERN) return fail(ctx, CATEQ_EINVAL, "cateq_solve: unknown wall_bc");
  if (p->wall_bc == CATEQ_WALL_STERN && (!posfin(p->stern_capacitance) || !std::isfinite(p->phi_pzc)))
    return fail(ctx, CATEQ_EINVAL, "cateq_solve: a Stern wall needs a positive, finite capacitance and a finite phi_pzc");
  double vol[MAXS];
  bool steric = false;
  for (int k = 0; k < N; ++k) {
    const double r = p->mpb_radius ? p->mpb_radius[k] : 0.0;
    if (!std::isfinite(p->charges[k]) || !(r >= 0.0) || !std::isfinite(r)) {
      snprintf(msg, sizeof msg, "cateq_solve: species %d needs a finite charge and a radius >= 0 (finite)", k);
      return fail(ctx, CATEQ_EINVAL, msg);
    }
    vol[k] = pnp::N_AVOGADRO * r * r * r;
    steric = steric || vol[k] != 0.0;
  }
  if (p->nlanes < 0) return fail(ctx, CATEQ_EINVAL, "cateq_solve: nlanes < 0");
  const int64_t n = p->nlanes;
  if (n > 0 && (!p->phiM || !p->phi_bulk || !p->c_bulk)) return fail(ctx, CATEQ_EINVAL, "cateq_solve: phiM, phi_bulk and c_bulk are required");
  for (int64_t i = 0; i < n; ++i) {
    double phi0 = 0.0;
    bool ok = std::isfinite(p->phiM[i]) && std::isfinite(p->phi_bulk[i]);
    for (int k = 0; k < N; ++k) {
      const double cb = p->c_bulk[i * N + k];
      ok = ok && cb >= 0.0 && std::isfinite(cb);
      phi0 += vol[k] * cb;
    }
    if (!ok || !(phi0 < 1.0)) {
      snprintf(msg, sizeof msg, "cateq_solve: operating point %lld needs finite potentials, finite c_bulk >= 0 and a bulk volume fraction < 1",
               (long long)i);
      return fail(ctx, CATEQ_EINVAL, msg);
    }
  }
  if (n == 0) return CATEQ_OK;

  KArgs a;
  memset(&a, 0, sizeof a);
  const int pitch = view->row_pitch;
  a.N = N; a.nx = nx; a.pitch = pitch; a.stern = p->wall_bc == CATEQ_WALL_STERN; a.n = n;
  a.maxit = std::min<int>(p->maxit, CATEQ_MAX_ITERATIONS);
  a.g = a.stern ? p->dx * p->stern_capacitance / p->eps : 0.0;
  a.phi_pzc = a.stern ? p->phi_pzc : 0.0;
  a.tol = p->tol;
  for (int k = 0; k < N; ++k) a.qbmax = std::max(a.qbmax, std::fabs(p->charges[k] * p->beta));
  int P = 1, WY = 1;
  choose_shape(nx, &P, &WY);

  // the grid weights and the per-lane parameters, staged on the host for one copy
  Inputs in;
  const int i_w = in.add((size_t)nx - 1, &a.w), i_pv = in.add((size_t)nx, &a.pv), i_sp = in.add((size_t)MAXS * SPF, &a.sp),
            i_lp = in.add_unpadded((size_t)n * LP, &a.lp);
  const size_t n_in = in.total;
  try {
    ctx->stage.assign(n_in, 0.0);
    ctx->flags.assign((size_t)2 * n, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATEQ_ENOMEM, "cateq_solve: out of host memory");
  }
  double *sw = in.host(ctx->stage, i_w), *spv = in.host(ctx->stage, i_pv), *ssp = in.host(ctx->stage, i_sp), *slp = in.host(ctx->stage, i_lp);
  const double pe = p->dx * p->dx / p->eps;
  for (int e = 0; e < nx - 1; ++e) sw[e] = p->dx / (p->x[e + 1] - p->x[e]);
  for (int i = 0; i < nx; ++i) {
    const double hl = i > 0 ? p->x[i] - p->x[i - 1] : 0.0, hr = i < nx - 1 ? p->x[i + 1] - p->x[i] : 0.0;
    spv[i] = pe * (0.5 * (hr + hl) / p->dx);
  }
  for (int k = 0; k < N; ++k) {
    double* f = ssp + k * SPF;
    f[0] = p->charges[k] * p->beta;
    f[1] = p->charges[k];
    f[2] = f[1] * f[0];
    f[3] = vol[k];
    f[4] = vol[k] * f[0];
  }
  for (int64_t i = 0; i < n; ++i) {
    double* l = slp + i * LP;
    double phi0 = 0.0;
    for (int k = 0; k < N; ++k) phi0 += vol[k] * p->c_bulk[i * N + k];
    l[0] = p->phiM[i];
    l[1] = p->phi_bulk[i];
    for (int k = 0; k < N; ++k) l[2 + k] = p->c_bulk[i * N + k] / (1.0 - phi0);
  }

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  const size_t n_c = (size_t)n * N * pitch, n_phi = (size_t)n * pitch;
  if (const int rc = reserve(ctx, entry, n_in + n_c + n_phi + even((size_t)n))) return rc;   // 2 n int32 = n doubles
  in.place(ctx->buf);
  a.oc = ctx->buf + n_in;
  a.ophi = a.oc + n_c;
  a.oflag = reinterpret_cast<int32_t*>(a.ophi + n_phi);
  PNP_POST_HIP(hipMemcpyAsync(ctx->buf, ctx->stage.data(), n_in * sizeof(double), hipMemcpyHostToDevice, st));
  int cus = 0;
  PNP_POST_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  if (!ctx->ev0) PNP_POST_HIP(hipEventCreate(&ctx->ev0));
  if (!ctx->ev1) PNP_POST_HIP(hipEventCreate(&ctx->ev1));
  ctx->kernel_ms = -1.0f;
  PNP_POST_HIP(hipEventRecord(ctx->ev0, st));
  hipError_t le = hipSuccess;
  const auto instance = [&](auto P_, auto WY_, auto S_) {
    le = launch<decltype(P_)::value, decltype(WY_)::value, decltype(S_)::value>(a, p->max_waves, cus, st);
  };
  if (steric) launch_shape<true>(P, WY, instance);
  else launch_shape<false>(P, WY, instance);
  PNP_POST_HIP(le);
  PNP_POST_HIP(hipGetLastError());
  PNP_POST_HIP(hipEventRecord(ctx->ev1, st));
  const size_t w = (size_t)nx * sizeof(double), dp = (size_t)pitch * sizeof(double);
  if (out->c) PNP_POST_HIP(hipMemcpy2DAsync(out->c, w, a.oc, dp, w, (size_t)n * N, hipMemcpyDeviceToHost, st));
  if (out->phi) PNP_POST_HIP(hipMemcpy2DAsync(out->phi, w, a.ophi, dp, w, (size_t)n, hipMemcpyDeviceToHost, st));
  if (out->status || out->iterations)
    PNP_POST_HIP(hipMemcpyAsync(ctx->flags.data(), a.oflag, (size_t)2 * n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PNP_POST_HIP(hipStreamSynchronize(st));
  PNP_POST_HIP(hipEventElapsedTime(&ctx->kernel_ms, ctx->ev0, ctx->ev1));
  snprintf(msg, sizeof msg, "cateq::pb_kernel<%d, %d, %s>", P, WY, steric ? "true" : "false");
  ctx->last_kernel = msg;
  for (int64_t i = 0; i < n; ++i) {
    if (out->status) out->status[i] = ctx->flags[2 * i];
    if (out->iterations) out->iterations[i] = ctx->flags[2 * i + 1];
  }
  if (out->c_dev) *out->c_dev = a.oc;
  if (out->phi_dev) *out->phi_dev = a.ophi;
  return CATEQ_OK;
}

}  // extern "C"
