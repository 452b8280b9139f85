// The recomputed record of one slot (point-major observation), and B = Jp L^-T of it: ONE copy for every pass that forms them — the
// point-side passes (kernels_point.hip, point_sweep.hpp) and the points' covariance blocks (kernels_selinv.hip) —, so that the passes
// give the same bits because they run the same text.
#pragma once
#include "lm_record.hpp"
#include "solver_state.hpp"

namespace rsba {

namespace {   // (internal linkage, as in a kernel file of its own: what a pass leaves unread the compiler may drop)

// the record of slot s (clamped by the caller): pose and scales straight from L2 (F x 192 B: resident)
// slot_xy: the observations in slot order (the solve's: sv.slot_xy)
// (GEN: the general-loss instantiation, lm_record.hpp — chosen by the launchers from dp.loss_general, like every GEN of the passes)
template <bool CAL, int P, bool GEN = false>
__device__ __forceinline__ void slot_record(const DeviceProblem& dp, const SolverDev& sv, const double2* slot_xy, int64_t s, ObsOut<CAL, P>& o, int& frame, int& point) {
  constexpr int CD = 6 * P;
  frame = sv.slot_frame[s]; point = sv.slot_point[s];
  const double2 xy = slot_xy[s];
  double pose[CD], psc[CD];
#pragma unroll
  for (int k = 0; k < CD; ++k) { pose[k] = dp.poses[(size_t)frame * CD + k]; psc[k] = dp.scale_pose[(size_t)frame * CD + k]; }
  double half_rho; bool dropped;
  lm_observation<CAL, P, GEN>(dp, frame, point, xy.x, xy.y, pose, psc, o, half_rho, dropped);
}

// B = Jp L^-T (2 x 3): jp = the point's three columns of the first residual row (of an ObsOut or of a stored record), the second row's
// row_stride doubles behind them; li = the six entries of the point's L^-1 (sv.Linv: i00 i10 i11 i20 i21 i22)
__device__ __forceinline__ void jp_linv(const double* jp, int row_stride, const double* li, double B[2][3]) {
  const double i00 = li[0], i10 = li[1], i11 = li[2], i20 = li[3], i21 = li[4], i22 = li[5];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double p0 = jp[r * row_stride], p1 = jp[r * row_stride + 1], p2 = jp[r * row_stride + 2];
    B[r][0] = p0 * i00; B[r][1] = p0 * i10 + p1 * i11; B[r][2] = p0 * i20 + p1 * i21 + p2 * i22;
  }
}

}  // namespace

}  // namespace rsba
