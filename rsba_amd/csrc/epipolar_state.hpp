// Arguments of the two-view kernels (kernels_epipolar.hip, kernels_five_point.hip); all pointers are device pointers.  The loop of the batched
// call around them is pair_loop_state.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pair_loop_state.hpp"   // PairRange

namespace rsba {

// epipolar_eight_point_kernel
struct EpiEightArgs {
  int n, m, num_tasks;
  const double* na;              // [n][2] undistorted, normalised image points of frame A (pnp_normalise_kernel)
  const double* nb;              // [n][2] ... of frame B
  const int32_t* subsets;        // [num_tasks][m]; with sub_start: the ragged lists, task t's at subsets[sub_start[t] .. + sub_count[t])
  const int32_t* sub_start;      // [num_tasks] or null (task t's list starts at t * m)
  const int32_t* sub_count;      // [num_tasks], with sub_start: the length of each list in m's place (below 8: declined)
  double* E_out;                 // [num_tasks][9]; declined slots are not written
  uint8_t* status;               // [num_tasks] 0 declined, 1 solved
};

// epipolar_score_kernel
struct EpiScoreArgs {
  int n, num_tasks;
  double f2, thr2;               // (mean focal length)^2, threshold_px^2
  const PairRange* pairs;        // null: every task counts over [0, n) with f2.  Else task t belongs to pairs[t / tasks_per_pair] and counts over
  int tasks_per_pair;            //   that pair's range with that pair's f2 (n and f2 above are not read)
  const double* na;              // [n][2]
  const double* nb;              // [n][2]
  const double* E;               // [num_tasks][9]
  const uint8_t* status_in;      // [num_tasks] or null: tasks with 0 here are declined without being read
  int32_t* num_inliers;          // [num_tasks]
  int32_t* num_front;            // [num_tasks][4]
  double* poses_out;             // [num_tasks][6]; declined slots are not written
  uint8_t* status;               // [num_tasks] 0 declined, 1 scored (may alias status_in)
};

// epipolar_five_point_kernel
struct EpiFiveArgs {
  int n, num_tasks;
  const double* na;              // [n][2]
  const double* nb;              // [n][2]
  const int32_t* subsets;        // [num_tasks][5]
  double* E_out;                 // [num_tasks][10][9]; only the slots below num_solutions are written
  int32_t* num_solutions;        // [num_tasks] 0 (declined) .. 10
  uint8_t* slot_status;          // [num_tasks][10] 1 for a written slot: the score kernel's status_in over the 10 num_tasks slots
  uint8_t* status;               // [num_tasks] 0 declined, 1 solved
};

// epipolar_pick_kernel: per task the best of its ten scored slots
struct EpiPickArgs {
  int num_tasks;
  const uint8_t* slot_status;    // [num_tasks][10] the score kernel's status
  const int32_t* slot_inliers;   // [num_tasks][10]
  const int32_t* slot_front;     // [num_tasks][10][4]
  const double* slot_E;          // [num_tasks][10][9]
  const double* slot_poses;      // [num_tasks][10][6]
  double* E_out;                 // [num_tasks][9]; declined tasks are not written
  double* poses_out;             // [num_tasks][6]; declined tasks are not written
  int32_t* num_inliers;          // [num_tasks]
  int32_t* num_front;            // [num_tasks][4]
  uint8_t* status;               // [num_tasks] 0: no slot that the score accepted
};

hipError_t launch_epipolar_five_point(const EpiFiveArgs& args, hipStream_t st);
hipError_t launch_epipolar_pick(const EpiPickArgs& args, hipStream_t st);
hipError_t launch_epipolar_eight_point(const EpiEightArgs& args, hipStream_t st);
hipError_t launch_epipolar_score(const EpiScoreArgs& args, hipStream_t st);
// mask[i] = correspondence i is an inlier of E [9]
hipError_t launch_epipolar_inliers(const EpiScoreArgs& args, uint8_t* mask, hipStream_t st);

}  // namespace rsba
