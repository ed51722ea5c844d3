// Physical mode, mid-size batches: the LANE-PAIR kernel -- the column-lane scheme of pnp_lane_cols.h at W = 2: every block row shared
// by TWO lanes (four lanes per operating point: two sweep directions x two halves of the block row).
// Lane = 4 * point + 2 * direction + half.
//
// Why: a lane of pnp_lane.hip advances its operating point at a fixed pace whatever the batch (N = 8, nx = 512: 3.4 ms per Newton
// iteration; 67 % of it the forward pass at ~4 200 instructions per grid row), and a batch of 8192 operating points puts one wave on a
// quarter of the SIMDs.  Here four lanes work on one operating point, so a wave holds 16 points, a batch gives twice the waves, and a
// wave's critical path per row is about half as long.  Same restrictions as the lane kernel (see there and DESIGN.md section 7a).
#include "pnp_lane_cols.h"

namespace pnp {

using namespace lane;

// per group of 16 operating points
size_t newton_lane2_rec_doubles(int nb, int nx) { return ColLanes<2>::rec_doubles(nb, nx); }
size_t newton_lane2_state_doubles(int nb, int nx) { return ColLanes<2>::state_doubles(nb, nx); }

template <int NB, int MODE, bool BDF>
__global__ __launch_bounds__(64) void newton_lane2_kernel(const NewtonArgs G) {
  newton_lane_cols_body<2, NB, MODE, BDF>(G);
}

namespace {
struct Lane2Kernels {
  template <int NB, int MODE, bool BDF>
  static auto kernel() { return &newton_lane2_kernel<NB, MODE, BDF>; }
};
}  // namespace

hipError_t launch_newton_lane2(const NewtonArgs& a, hipStream_t stream) { return launch_lane_cols<2, Lane2Kernels>(a, stream); }

bool newton_lane2_supported(int nb, int nx, int mode) { return nb >= 6 && nb <= 9 && nx >= 5 && mode <= 2; }

bool newton_lane2_preferred(int nb, int nx, int64_t B) {
  // Measured on one device in one call (tools/probe/lane2_probe.sh; N = 8, nx = 512, timesteps/s, lane pair / lane / lane teams):
  // B = 1024 1.16e5 / 1.00e5 / 1.40e5, 2048 2.40e5 / 1.96e5 / 1.43e5, 4096 4.51e5 / 3.85e5 / 1.44e5, 8192 7.31e5 / 7.07e5 / 1.51e5,
  // 16 384 0.99e6 / 1.03e6.  Twice the waves for the same batch, but the distribution overhead (selects, DPP moves, duplicated
  // assembly) leaves a wave's pace only 1.28 x the lane kernel's and two waves on a CU cost each other ~20 %.
  // Round 4: below 10 240 points the lane-quad kernel (pnp_lane4.hip) is ahead of both; the pair keeps the window up to the lane
  // kernel's crossover (profiles/r04_lane4_probe.jsonl: B = 12 288 lane pair 9.96e5 / lane 9.55e5 / lane quad 7.78e5; 16 384 1.05e6 /
  // 1.10e6 / 0.87e6).
  // End of the window, measured again with the fused lane kernel as the alternative (profiles/r04_family_rates.jsonl; lane pair /
  // lane fused): N = 8, nx = 512: B = 14 336 1.17e6 / 1.05e6, 16 384 (1024 waves of 16 points: the last batch in one round) 1.25e6 /
  // 1.19e6, 18 432 0.97e6 / 1.20e6; N = 8, nx = 1024: 16 384 5.6e5 / 5.4e5; N = 6, nx = 1024: 12 288 7.6e5 / 7.4e5, 14 336 7.8e5 / 8.1e5;
  // N = 6, nx = 512: 12 288 1.62e6 / 1.58e6, 16 384 1.90e6 / 2.04e6.
  // N = 7, nx = 512 (profiles/r04_family_rates_n5_n7.jsonl): 12 288 1.39e6 / 1.28e6, 14 336 1.44e6 / 1.47e6;  N = 5: 10 240 1.79e6 / 1.86e6,
  // 12 288 2.12e6 / 2.26e6 -- no window above the lane quad's.
  return B >= 1280 && B <= (nb >= 9 ? 16384 : (nb >= 7 ? 13311 : 10239));
}

}  // namespace pnp
