// Arguments of the two-view kernels (kernels_epipolar.hip, kernels_five_point.hip); all pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

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
struct EpiPair { int32_t start, n; double f2; };   // one frame pair of a batched call: its range of the concatenated points, its (mean focal length)^2
struct EpiScoreArgs {
  int n, num_tasks;
  double f2, thr2;               // (mean focal length)^2, threshold_px^2
  const EpiPair* pairs;          // null: every task counts over [0, n) with f2.  Else task t belongs to pairs[t / tasks_per_pair] and counts over
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

// ---- the batched RANSAC of many frame pairs (rsba_epipolar_ransac_pairs): the state of the loop per pair, and the kernels around the
// hypothesis kernels above that keep the loop on the device
struct EpiPairState {
  int num_pairs;                 // of this launch (a chunk); every array below is indexed by the chunk's pair, every range by EpiPair::start
  const EpiPair* pairs;          // [num_pairs]
  double* E;                     // [num_pairs][9] the current matrix
  double* pose;                  // [num_pairs][6]
  int32_t* num_inliers;          // [num_pairs]
  int32_t* num_front;            // [num_pairs][4]
  int32_t* winner_task;          // [num_pairs] -1: no accepted hypothesis
  int32_t* refits_adopted;       // [num_pairs]
  uint8_t* status;               // [num_pairs] 1: the pair has a winner
  uint8_t* done;                 // [num_pairs] 1: no (further) refit — no winner, fewer than 8 inliers, or a refit that was not adopted
  uint8_t* mask;                 // [points] inlier flags of the current matrix (zero for a pair without a winner)
  int32_t* inlier_idx;           // [points] per pair, from its start: the ascending (global) indices of its inliers
  int32_t* inlier_count;         // [num_pairs] their number; 0 for a pair that is done
};
// epipolar_winner_kernel: per pair the best of its tasks_per_pair scored hypotheses — most inliers, with front_breaks_ties the most in front
// (over the four candidates) next, then the lowest task
struct EpiWinnerArgs {
  EpiPairState S;
  int tasks_per_pair, front_breaks_ties;
  const uint8_t* status;         // [num_pairs][tasks_per_pair]
  const int32_t* num_inliers;    // [num_pairs][tasks_per_pair]
  const int32_t* num_front;      // [num_pairs][tasks_per_pair][4]
  const double* E;               // [num_pairs][tasks_per_pair][9]
  const double* poses;           // [num_pairs][tasks_per_pair][6]
};
// epipolar_adopt_kernel: the refit of each pair (one task per pair), adopted iff accepted and its count is not lower
struct EpiAdoptArgs {
  EpiPairState S;
  const uint8_t* status;         // [num_pairs] the score kernel's
  const int32_t* num_inliers;    // [num_pairs]
  const int32_t* num_front;      // [num_pairs][4]
  const double* E;               // [num_pairs][9]
  const double* poses;           // [num_pairs][6]
};
hipError_t launch_epipolar_winner(const EpiWinnerArgs& args, hipStream_t st);
// mask[i] of every correspondence of the pairs that are not done, from its pair's current E; first_point / num_points: the chunk's range,
// point_pair [points]: the chunk's pair of each correspondence
hipError_t launch_epipolar_pair_masks(const EpiPairState& S, const int32_t* point_pair, int first_point, int num_points, double thr2, const double* na, const double* nb, hipStream_t st);
// inlier_idx / inlier_count from mask, in ascending order; a pair with fewer than 8 inliers becomes done
hipError_t launch_epipolar_compact(const EpiPairState& S, hipStream_t st);
hipError_t launch_epipolar_adopt(const EpiAdoptArgs& args, hipStream_t st);

hipError_t launch_epipolar_five_point(const EpiFiveArgs& args, hipStream_t st);
hipError_t launch_epipolar_pick(const EpiPickArgs& args, hipStream_t st);
hipError_t launch_epipolar_eight_point(const EpiEightArgs& args, hipStream_t st);
hipError_t launch_epipolar_score(const EpiScoreArgs& args, hipStream_t st);
// mask[i] = correspondence i is an inlier of E [9]
hipError_t launch_epipolar_inliers(const EpiScoreArgs& args, uint8_t* mask, hipStream_t st);

}  // namespace rsba
