// Arguments of the homography and parallax kernels (kernels_homography.hip); all pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

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
struct HomoPair { int32_t start, n; double f2; };   // one frame pair of a batched call: its range of the concatenated points, its (mean focal length)^2
struct HomoScoreArgs {
  int n, num_tasks;
  double f2, thr2;               // (mean focal length)^2, threshold_px^2
  const HomoPair* pairs;         // null: every task counts over [0, n) with f2.  Else task t belongs to pairs[t / tasks_per_pair] and counts over
  int tasks_per_pair;            //   that pair's range with that pair's f2 (n and f2 above are not read)
  const double* na;              // [n][2]
  const double* nb;              // [n][2]
  const double* H;               // [num_tasks][9]
  const uint8_t* status_in;      // [num_tasks] or null: tasks with 0 here are declined without being read
  int32_t* num_inliers;          // [num_tasks]
  uint8_t* status;               // [num_tasks] 0 declined, 1 scored (may alias status_in)
};

// ---- the batched homography RANSAC of many frame pairs (rsba_two_view_classify_pairs): the state of the loop per pair
struct HomoPairState {
  int num_pairs;                 // of this launch (a chunk); every array below is indexed by the chunk's pair, every range by HomoPair::start
  const HomoPair* pairs;         // [num_pairs]
  double* H;                     // [num_pairs][9] the current matrix
  int32_t* num_inliers;          // [num_pairs]
  int32_t* winner_task;          // [num_pairs] -1: no accepted hypothesis
  int32_t* refits_adopted;       // [num_pairs]
  uint8_t* status;               // [num_pairs] 1: the pair has a winner
  uint8_t* done;                 // [num_pairs] 1: no (further) refit — no winner, fewer than 5 inliers, or a refit that was not adopted
  uint8_t* mask;                 // [points] inlier flags of the current matrix (zero for a pair without a winner)
  int32_t* inlier_idx;           // [points] per pair, from its start: the ascending (global) indices of its inliers
  int32_t* inlier_count;         // [num_pairs] their number; 0 for a pair that is done
};
// homography_winner_kernel: per pair the best of its tasks_per_pair scored hypotheses — most inliers, then the lowest task
struct HomoWinnerArgs {
  HomoPairState S;
  int tasks_per_pair;
  const uint8_t* status;         // [num_pairs][tasks_per_pair]
  const int32_t* num_inliers;    // [num_pairs][tasks_per_pair]
  const double* H;               // [num_pairs][tasks_per_pair][9]
};
// homography_adopt_kernel: the refit of each pair (one task per pair), adopted iff accepted and its count is not lower
struct HomoAdoptArgs {
  HomoPairState S;
  const uint8_t* status;         // [num_pairs] the score kernel's
  const int32_t* num_inliers;    // [num_pairs]
  const double* H;               // [num_pairs][9]
};
// two_view_parallax_kernel: per pair the two counts of the parallax rule
struct ParallaxArgs {
  int num_pairs;
  const HomoPair* pairs;         // [num_pairs]
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
hipError_t launch_homography_winner(const HomoWinnerArgs& args, hipStream_t st);
// mask[i] of every correspondence of the pairs that are not done, from its pair's current H; first_point / num_points: the chunk's range,
// point_pair [points]: the chunk's pair of each correspondence
hipError_t launch_homography_pair_masks(const HomoPairState& S, const int32_t* point_pair, int first_point, int num_points, double thr2, const double* na, const double* nb,
                                        hipStream_t st);
// inlier_idx / inlier_count from mask, in ascending order; a pair with fewer than 5 inliers becomes done
hipError_t launch_homography_compact(const HomoPairState& S, hipStream_t st);
hipError_t launch_homography_adopt(const HomoAdoptArgs& args, hipStream_t st);
hipError_t launch_two_view_parallax(const ParallaxArgs& args, hipStream_t st);

}  // namespace rsba
