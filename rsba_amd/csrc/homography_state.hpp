// Arguments of the homography and parallax kernels (kernels_homography.hip); all pointers are device pointers.  The loop of the batched call
// around them is pair_loop_state.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pair_loop_state.hpp"   // PairRange

namespace rsba {

// homography_dlt_kernel
struct HomoDltArgs {
  int n, m, num_tasks;
  const double* na;              // [n][2] undistorted, normalised image points of frame A (pnp_normalise_kernel)
  const double* nb;              // [n][2] ... of frame B
  const int32_t* subsets;        // [num_tasks][m]; with sub_start: the ragged lists, task t's at subsets[sub_start[t] .. + sub_count[t])
  const int32_t* sub_start;      // [num_tasks] or null (task t's list starts at t * m)
  const int32_t* sub_count;      // [num_tasks], with sub_start: the length of each list in m's place (below 4: declined)
  double* H_out;                 // [num_tasks][9]; declined slots are not written
  uint8_t* status;               // [num_tasks] 0 declined, 1 solved
};

// homography_score_kernel
struct HomoScoreArgs {
  int n, num_tasks;
  double f2, thr2;               // (mean focal length)^2, threshold_px^2
  const PairRange* pairs;        // null: every task counts over [0, n) with f2.  Else task t belongs to pairs[t / tasks_per_pair] and counts over
  int tasks_per_pair;            //   that pair's range with that pair's f2 (n and f2 above are not read)
  const double* na;              // [n][2]
  const double* nb;              // [n][2]
  const double* H;               // [num_tasks][9]
  const uint8_t* status_in;      // [num_tasks] or null: tasks with 0 here are declined without being read
  int32_t* num_inliers;          // [num_tasks]
  uint8_t* status;               // [num_tasks] 0 declined, 1 scored (may alias status_in)
};

// two_view_parallax_kernel: per pair the two counts of the parallax rule
struct ParallaxArgs {
  int num_pairs;
  const PairRange* pairs;        // [num_pairs]
  const double* na;              // [points][2]
  const double* nb;              // [points][2]
  const double* E;               // [num_pairs][9]
  const double* poses;           // [num_pairs][6] camera B in A's frame
  const uint8_t* pair_status;    // [num_pairs] 0: the pair has no essential matrix — zero counts, E and the pose are not read
  double thr2, cos_min;          // threshold_px^2, the cosine of the threshold angle
  int32_t* num_front;            // [num_pairs]
  int32_t* num_parallax;         // [num_pairs]
};

hipError_t launch_homography_dlt(const HomoDltArgs& args, hipStream_t st);
hipError_t launch_homography_score(const HomoScoreArgs& args, hipStream_t st);
// mask[i] = correspondence i is an inlier of H [9]
hipError_t launch_homography_inliers(const HomoScoreArgs& args, uint8_t* mask, hipStream_t st);
hipError_t launch_two_view_parallax(const ParallaxArgs& args, hipStream_t st);

}  // namespace rsba
