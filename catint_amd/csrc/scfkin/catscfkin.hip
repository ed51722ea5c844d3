// libcatint_scfkin (include/catint_scfkin.h): the wall fluxes of a mean-field surface microkinetic model inside the device SCF loop --
// the function pnp_scf_cycle_fn calls between its bookkeeping and its transport solve, one launch per iteration, the coverages of
// every lane kept on the device as the next iteration's start.  gfx950 / MI355X only.
//
// Mapping, working set, tables and arithmetic: ../pnp_kin.h, which also holds the Newton iteration and the flux sums this kernel
// shares with kinetics/catkin.hip (one text, the same bits).  A point is a lane of the batch: group g of the persistent grid holds
// lanes 64 g .. 64 g + 63.  A lane that is not active reads and writes no global memory and idles through the iteration; a group
// without an active lane is skipped, so the lanes that left the loop cost a flag read.  LDS slots as in catkin::steady_kernel: J[T][T]
// (or N slots, whichever is more), y[T], the right-hand side [T], the row scales D[T], the activities a[N] and N accumulators.  At
// S = 8, N = 8: 124 slots x 512 B = 62 KB per wave.
#include "../../../include/catint_scfkin.h"
#include "../pnp_kin.h"

#pragma clang fp contract(off)

namespace catsk {

using namespace pnp::kin;

struct KArgs {
  int32_t N, S, R, maxit, w, use_sigma, from_view, ldx;   // use_sigma, from_view: 0 (point_inputs reads them by name)
  int64_t n;               // B
  const double* c;         // never: the view path of point_inputs
  const double* phi;
  const int32_t* st;
  const double *cs, *phis; // the loop's mixed surface concentrations [B][N] and the surface potential of its last solve [B]
  const double *phiM, *sigma, *off, *gamma;   // [B], null, null, [B][N] or null
  const int32_t* active;   // [B]
  double *theta, *fscale, *flast, *flux;   // [B][T], [B][N], [B][N] of the context; [B][N] of the loop
  int32_t *status, *iters, *total, *calls; // [B] of the context
  double sd, tol, CS, pzc;
};

__global__ __launch_bounds__(64) void flux_kernel(const KArgs A, const Table* __restrict__ tab) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = A.N, T = A.S + 1;
  const Table& tb = *tab;   // its own read-only argument: the uniform reads become scalar loads
  SteadyLane ln;
  steady_slots(ln, lds, lane, N, T);
  double* L = ln.L;
  const double bad_number = __builtin_nan("");

  for (int64_t grp = blockIdx.x; grp * 64 < A.n; grp += gridDim.x) {
    const int64_t b = grp * 64 + lane;
    const bool live = b < A.n && A.active[b < A.n ? b : 0] != 0;
    if (__ballot(live) == 0) continue;
    bool ok = false;
    if (live) {
      ln.pt = point_inputs(A, tb, b, b, ln.at(ln.oA));
      ok = ln.pt.ok;
    } else {   // an idle lane: numbers of its own that no one reads
      ln.pt.ok = false;
      ln.pt.V = 0.0;
      ln.pt.sg = 0.0;
      ln.pt.off = nullptr;
      for (int j = 0; j < N; ++j) L[(ln.oA + j) * 64] = 0.0;
    }
    // ---- start: the lane's stored coverages when all are finite, else the uniform one ----
    double nsum = 0.0;
    for (int t = 0; t < T; ++t) nsum = nsum + tb.ns[t];
    const double y0 = log(1.0 / nsum);
    bool warm = live;
    if (live)
      for (int t = 0; t < T; ++t) warm = warm && finite_(A.theta[b * T + t]);
    for (int t = 0; t < T; ++t) L[(ln.oY + t) * 64] = warm ? log_coverage(A.theta[b * T + t]) : y0;
    // ---- Newton ----
    int it;
    uint64_t pivs;
    const int status = steady_newton(A, tb, ln, ok ? CATSK_MAXIT : CATSK_INPUT, ok && live, it, pivs);
    const bool nan = status == CATSK_INPUT;

    // ---- coverages and fluxes at the lane's y (the J slots are free: N of them hold flux_scale) ----
    if (live)
      for (int t = 0; t < T; ++t) A.theta[b * T + t] = nan ? bad_number : exp(L[(ln.oY + t) * 64]);
    steady_fluxes(A, tb, ln, [](int, double, double) {});
    if (live) {
      for (int k = 0; k < N; ++k) {
        const double f = A.sd * L[(ln.oC + k) * 64];
        A.fscale[b * N + k] = nan ? bad_number : A.sd * L[(ln.oJ + k) * 64];
        if (status == CATSK_CONVERGED) A.flast[b * N + k] = f;
        A.flux[b * N + k] = status == CATSK_CONVERGED ? f : bad_number;
      }
      A.status[b] = status;
      A.iters[b] = it;
      A.total[b] = A.total[b] + it;
      A.calls[b] = A.calls[b] + 1;
    }
  }
}

static size_t lds_bytes(int N, int S) {
  const int T = S + 1;
  return (size_t)(std::max(T * T, N) + 3 * T + 2 * N) * 64 * sizeof(double);
}

}  // namespace catsk

static_assert(CATSK_OK == pnp::post::OK && CATSK_EINVAL == pnp::post::ERR_INVAL && CATSK_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATSK_EDEVICE == pnp::post::ERR_DEVICE && CATSK_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_scfkin.h and pnp_post.h disagree");
static_assert(CATSK_MAX_SPECIES == pnp::kin::MAXN && CATSK_MAX_ADSORBATES == pnp::kin::MAXS && CATSK_MAX_STEPS == pnp::kin::MAXR &&
                  CATSK_MIN_LOG == pnp::kin::MINLOG && CATSK_DROP_FULL == pnp::kin::DROP_FULL && CATSK_DROP_STERN == pnp::kin::DROP_STERN &&
                  CATSK_CONVERGED == pnp::kin::STATUS_CONVERGED && CATSK_MAXIT == pnp::kin::STATUS_MAXIT &&
                  CATSK_INPUT == pnp::kin::STATUS_INPUT && CATSK_PIVOT == pnp::kin::STATUS_PIVOT,
              "catint_scfkin.h and pnp_kin.h disagree");

// From catsk_begin on the context's device buffer holds, in doubles from its start: the Table, phiM [B], gamma [B][N]
// (when given), theta [B][T], flux_scale [B][N], flux_last [B][N], the four int32 rows [4][B], and the buffers of catsk_step_host:
// csurf [B][N], phi_surface [B], flux [B][N], active [B] int32
struct catsk_ctx : pnp::post::Ctx {
  bool begun = false;
  int N = 0, S = 0, R = 0;
  int64_t B = 0;
  int blocks = 0;
  size_t lds = 0;
  size_t o_th = 0, o_fs = 0, o_fl = 0, o_int = 0, o_cs = 0, o_ps = 0, o_fx = 0, o_act = 0;
  catsk::KArgs a;
  const pnp::kin::Table* tab = nullptr;
};

static int catsk_flux(void* user, const pnp_scf_device* d) {
  using namespace catsk;
  catsk_ctx* ctx = static_cast<catsk_ctx*>(user);
  if (!ctx) return 1;
  if (!ctx->begun) return fail(ctx, 1, "catsk_flux_fn: call catsk_begin first");
  char msg[256];
  if (!d || d->struct_size != (int32_t)sizeof(pnp_scf_device)) return fail(ctx, 2, "catsk_flux_fn: pnp_scf_device.struct_size does not match this library");
  if (d->batch != ctx->B) {
    snprintf(msg, sizeof msg, "catsk_flux_fn: the loop has %lld lanes, catsk_begin was given %lld", (long long)d->batch, (long long)ctx->B);
    return fail(ctx, 3, msg);
  }
  if (d->nspecies != ctx->N) {
    snprintf(msg, sizeof msg, "catsk_flux_fn: the loop has %d species, catsk_begin was given %d", d->nspecies, ctx->N);
    return fail(ctx, 4, msg);
  }
  if (!d->surface_concentration || !d->surface_potential || !d->active || !d->flux) return fail(ctx, 2, "catsk_flux_fn: null array in pnp_scf_device");
  KArgs a = ctx->a;
  a.cs = d->surface_concentration;
  a.phis = d->surface_potential;
  a.active = d->active;
  a.flux = d->flux;
  hipLaunchKernelGGL(flux_kernel, dim3(ctx->blocks), dim3(64), ctx->lds, (hipStream_t)d->stream, a, ctx->tab);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, 5, std::string("catsk_flux_fn: ") + hipGetErrorString(e));
  ctx->last_kernel = "catsk::flux_kernel";
  return 0;
}

extern "C" {

int catsk_create(int32_t device, catsk_ctx** out) { return pnp::post::create("catsk_create", device, out); }
void catsk_destroy(catsk_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catsk_last_error(const catsk_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catsk_last_kernel(const catsk_ctx* ctx) { return pnp::post::last_kernel(ctx); }

int catsk_begin(catsk_ctx* ctx, const catsk_params* p) {
  using namespace catsk;
  static const char entry[] = "catsk_begin";
  // (the parameters stand in for the outputs check_sizes also looks at: this entry point has none)
  if (const int rc = check_sizes(ctx, entry, "catsk_params", "catsk_params", p, p)) return rc;
  if (p->maxit < 1) return fail(ctx, CATSK_EINVAL, "catsk_begin: maxit < 1");
  if (const int rc = check_drop(ctx, entry, p)) return rc;
  if (!posfin(p->tol)) return fail(ctx, CATSK_EINVAL, "catsk_begin: tol must be positive and finite");
  if (const int rc = check_tables(ctx, entry, p)) return rc;
  if (!(std::isfinite(p->stern_capacitance) && std::isfinite(p->phi_pzc)))
    return fail(ctx, CATSK_EINVAL, "catsk_begin: the surface charge needs a finite stern_capacitance and phi_pzc");
  if (p->batch < 1) return fail(ctx, CATSK_EINVAL, "catsk_begin: batch < 1");

  ctx->begun = false;
  const int N = p->nspecies, S = p->nadsorbates, R = p->nsteps, T = S + 1;
  const size_t B = (size_t)p->batch;
  const bool gm = p->gamma && N;
  const size_t o_t = 0, o_pm = o_t + sizeof(Table) / 8, o_gm = o_pm + even(B);
  ctx->o_th = o_gm + (gm ? even(B * N) : 0);
  ctx->o_fs = ctx->o_th + even(B * T);
  ctx->o_fl = ctx->o_fs + even(B * N);
  ctx->o_int = ctx->o_fl + even(B * N);
  ctx->o_cs = ctx->o_int + 2 * B;
  ctx->o_ps = ctx->o_cs + even(B * N);
  ctx->o_fx = ctx->o_ps + even(B);
  ctx->o_act = ctx->o_fx + even(B * N);
  const size_t total = ctx->o_act + even(B) / 2;
  try {
    ctx->stage.assign(total, 0.0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATSK_ENOMEM, "catsk_begin: out of host memory");
  }
  double* sg = ctx->stage.data();
  fill_table(reinterpret_cast<Table*>(sg + o_t), p);
  memcpy(sg + o_pm, p->phiM, B * 8);
  if (gm) memcpy(sg + o_gm, p->gamma, B * N * 8);
  if (p->theta_guess) memcpy(sg + ctx->o_th, p->theta_guess, B * T * 8);
  else std::fill(sg + ctx->o_th, sg + ctx->o_th + B * T, std::nan(""));

  PNP_POST_HIP(hipSetDevice(ctx->device));
  ctx->lds = lds_bytes(N, S);
  if (ctx->lds > 48 * 1024) PNP_POST_HIP(hipFuncSetAttribute((const void*)flux_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->lds));
  const int64_t groups = ((int64_t)B + 63) / 64;
  int64_t blocks = p->max_waves;
  if (blocks == 0) {
    int cus = 0, per_cu = 0;
    PNP_POST_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    PNP_POST_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, flux_kernel, 64, ctx->lds));
    blocks = (int64_t)std::max(per_cu, 1) * std::max(cus, 1);
  }
  ctx->blocks = (int)std::min(std::max<int64_t>(blocks, 1), groups);
  if (const int rc = reserve(ctx, entry, total)) return rc;
  PNP_POST_HIP(hipMemcpy(ctx->buf, sg, total * sizeof(double), hipMemcpyHostToDevice));

  KArgs& a = ctx->a;
  memset(&a, 0, sizeof a);
  a.N = N; a.S = S; a.R = R; a.maxit = p->maxit; a.w = p->potential_drop;
  a.n = p->batch;
  a.sd = p->site_density; a.tol = p->tol; a.CS = p->stern_capacitance; a.pzc = p->phi_pzc;
  a.phiM = ctx->buf + o_pm;
  if (gm) a.gamma = ctx->buf + o_gm;
  a.theta = ctx->buf + ctx->o_th;
  a.fscale = ctx->buf + ctx->o_fs;
  a.flast = ctx->buf + ctx->o_fl;
  int32_t* ints = reinterpret_cast<int32_t*>(ctx->buf + ctx->o_int);
  a.status = ints;
  a.iters = ints + B;
  a.total = ints + 2 * B;
  a.calls = ints + 3 * B;
  ctx->tab = reinterpret_cast<const Table*>(ctx->buf + o_t);
  ctx->N = N; ctx->S = S; ctx->R = R; ctx->B = p->batch;
  ctx->begun = true;
  return CATSK_OK;
}

pnp_scf_flux_fn catsk_flux_fn(void) { return catsk_flux; }

int catsk_step_host(catsk_ctx* ctx, const double* csurf, const double* phi_surface, const int32_t* active, double* flux) {
  static const char entry[] = "catsk_step_host";
  if (!ctx) return CATSK_EINVAL;
  if (!ctx->begun) return fail(ctx, CATSK_EINVAL, "catsk_step_host: call catsk_begin first");
  if (!phi_surface || !active || (ctx->N > 0 && (!csurf || !flux))) return fail(ctx, CATSK_EINVAL, "catsk_step_host: null argument");
  const size_t B = (size_t)ctx->B, N = (size_t)ctx->N;
  PNP_POST_HIP(hipSetDevice(ctx->device));
  double* buf = ctx->buf;
  if (N) PNP_POST_HIP(hipMemcpy(buf + ctx->o_cs, csurf, B * N * 8, hipMemcpyHostToDevice));
  PNP_POST_HIP(hipMemcpy(buf + ctx->o_ps, phi_surface, B * 8, hipMemcpyHostToDevice));
  if (N) PNP_POST_HIP(hipMemcpy(buf + ctx->o_fx, flux, B * N * 8, hipMemcpyHostToDevice));
  PNP_POST_HIP(hipMemcpy(buf + ctx->o_act, active, B * sizeof(int32_t), hipMemcpyHostToDevice));
  pnp_scf_device d;
  memset(&d, 0, sizeof d);
  d.struct_size = (int32_t)sizeof d;
  d.nspecies = ctx->N;
  d.batch = ctx->B;
  d.surface_concentration = buf + ctx->o_cs;
  d.surface_potential = buf + ctx->o_ps;
  d.active = reinterpret_cast<const int32_t*>(buf + ctx->o_act);
  d.flux = buf + ctx->o_fx;
  d.stream = nullptr;
  if (catsk_flux(ctx, &d) != 0) return CATSK_EDEVICE;   // (the message is the function's)
  if (N) PNP_POST_HIP(hipMemcpy(flux, buf + ctx->o_fx, B * N * 8, hipMemcpyDeviceToHost));
  PNP_POST_HIP(hipDeviceSynchronize());
  return CATSK_OK;
}

int catsk_end(catsk_ctx* ctx, const catsk_outputs* out) {
  static const char entry[] = "catsk_end";
  if (!ctx) return CATSK_EINVAL;
  if (!out) return fail(ctx, CATSK_EINVAL, "catsk_end: null argument");
  if (out->struct_size != (int32_t)sizeof(catsk_outputs)) return fail(ctx, CATSK_EINVAL, "catsk_end: catsk_outputs.struct_size does not match this library");
  if (!ctx->begun) return fail(ctx, CATSK_EINVAL, "catsk_end: call catsk_begin first");
  const size_t B = (size_t)ctx->B, N = (size_t)ctx->N, T = (size_t)ctx->S + 1;
  PNP_POST_HIP(hipSetDevice(ctx->device));
  PNP_POST_HIP(hipDeviceSynchronize());   // the loop's stream included
  const int32_t* ints = reinterpret_cast<const int32_t*>(ctx->buf + ctx->o_int);
  if (out->theta) PNP_POST_HIP(hipMemcpy(out->theta, ctx->buf + ctx->o_th, B * T * 8, hipMemcpyDeviceToHost));
  if (out->flux_scale && N) PNP_POST_HIP(hipMemcpy(out->flux_scale, ctx->buf + ctx->o_fs, B * N * 8, hipMemcpyDeviceToHost));
  if (out->flux_last && N) PNP_POST_HIP(hipMemcpy(out->flux_last, ctx->buf + ctx->o_fl, B * N * 8, hipMemcpyDeviceToHost));
  if (out->status) PNP_POST_HIP(hipMemcpy(out->status, ints, B * 4, hipMemcpyDeviceToHost));
  if (out->iterations_last) PNP_POST_HIP(hipMemcpy(out->iterations_last, ints + B, B * 4, hipMemcpyDeviceToHost));
  if (out->iterations_total) PNP_POST_HIP(hipMemcpy(out->iterations_total, ints + 2 * B, B * 4, hipMemcpyDeviceToHost));
  if (out->calls) PNP_POST_HIP(hipMemcpy(out->calls, ints + 3 * B, B * 4, hipMemcpyDeviceToHost));
  return CATSK_OK;
}

}  // extern "C"
