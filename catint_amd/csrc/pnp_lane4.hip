// Physical mode, batches of a few thousand operating points and long grids: the LANE-QUAD kernel -- the column-lane scheme of
// pnp_lane_cols.h at W = 4: every block row shared by FOUR lanes (eight lanes per operating point: two sweep directions x four column
// lanes).  Lane = 8 * point + 4 * direction + column lane.
//
// Why (round 3 measurements): a lone wave runs at the SIMD's full instruction rate (one vector instruction per
// ~4 cycles), so at a given batch the only way to go faster is more waves.  The lane kernel holds 32 operating points per wave (256
// waves for 8192 points: three SIMDs of every CU idle), the lane-pair kernel 16 (512 waves) at 1.28 x the instructions per row and
// wave.  Here a wave holds 8 points: 8192 points give every SIMD of the chip a wave, and a wave's row costs about half the pair
// kernel's instructions because a lane carries a quarter of the columns.  On top of the shared scheme the quad requests its records
// and update rows four rows ahead and staggers the start of its waves (pnp_lane_cols.h: PREFETCH_ROWS, START_STAGGER).
#include "pnp_lane_cols.h"

namespace pnp {

using namespace lane;

// per group of 8 operating points
size_t newton_lane4_rec_doubles(int nb, int nx) { return ColLanes<4>::rec_doubles(nb, nx); }
size_t newton_lane4_state_doubles(int nb, int nx) { return ColLanes<4>::state_doubles(nb, nx); }

template <int NB, int MODE, bool BDF>
__global__ __launch_bounds__(64) void newton_lane4_kernel(const NewtonArgs G) {
  newton_lane_cols_body<4, NB, MODE, BDF>(G);
}

namespace {
struct Lane4Kernels {
  template <int NB, int MODE, bool BDF>
  static auto kernel() { return &newton_lane4_kernel<NB, MODE, BDF>; }
};
}  // namespace

hipError_t launch_newton_lane4(const NewtonArgs& a, hipStream_t stream) {
  NewtonArgs as = a;
  as.lane_stagger = (as.opt && as.opt->lane_stagger >= 0) ? as.opt->lane_stagger : 0;
  return launch_lane_cols<4, Lane4Kernels>(as, stream);
}

bool newton_lane4_supported(int nb, int nx, int mode) { return nb >= 6 && nb <= 9 && nx >= 5 && mode <= 2; }

bool newton_lane4_preferred(int nb, int nx, int64_t B) {
  // Measured on one device in one process (tools/probe/lane4_probe.py -> profiles/r04_lane4_probe.jsonl; N = 8 steric, nx = 512,
  // timesteps/s, lane quad / lane pair / lane / lane teams): B = 1024 1.66e5 / 1.19e5 / 1.00e5 / 1.38e5, 2048 3.24e5 / 2.32e5 / 1.97e5 /
  // 1.41e5, 4096 5.61e5 / 4.46e5 / 3.86e5 / 1.45e5, 8192 9.09e5 / 7.43e5 / 7.18e5, 12 288 7.78e5 / 9.96e5 / 9.55e5, 16 384 0.87e6 /
  // 1.05e6 / 1.10e6; nx = 4096: B = 2048 3.97e4 / 2.86e4 / 2.49e4, 8192 1.10e5 / 0.97e5 / 0.92e5; N = 6, nx = 1024: 8192 6.50e5 / 5.53e5 /
  // 5.26e5, 16 384 6.98e5 / 8.28e5 / 8.15e5.  Eight points per wave: the chip is full at 8192 points (one wave per SIMD) and the
  // kernel saturates there; beyond, a second round of waves per SIMD costs more than the lane pair's and the lane kernel's larger
  // waves (a wave's row: ~2000 vector instructions for 8 points against ~4200 for the lane kernel's 32).
  return B >= 896 && B < 10240;
}

}  // namespace pnp
