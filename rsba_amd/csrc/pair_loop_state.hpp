// The RANSAC loop of many frame pairs in one call, kept on the device (kernels_pair_loop.hip): the state per pair and the arguments of the
// kernels around a model's hypothesis kernels.  One loop for both models — the essential matrix (rsba_epipolar_ransac_pairs: E, its pose and
// the four front counts) and the homography (rsba_two_view_classify_pairs: H alone, the pose and front pointers null).  All pointers are
// device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rsba {

// one frame pair of a batched call: its range of the concatenated points, its (mean focal length)^2
struct PairRange { int32_t start, n; double f2; };

struct PairLoopState {
  int num_pairs;                 // of this launch (a chunk); every array below is indexed by the chunk's pair, every range by PairRange::start
  const PairRange* pairs;        // [num_pairs]
  double* model;                 // [num_pairs][9] the current matrix (E or H)
  double* pose;                  // [num_pairs][6], or null (homography)
  int32_t* num_inliers;          // [num_pairs]
  int32_t* num_front;            // [num_pairs][4], or null (homography)
  int32_t* winner_task;          // [num_pairs] -1: no accepted hypothesis
  int32_t* refits_adopted;       // [num_pairs]
  uint8_t* status;               // [num_pairs] 1: the pair has a winner
  uint8_t* done;                 // [num_pairs] 1: no (further) refit — no winner, too few inliers for a refit, or a refit that was not adopted
  uint8_t* mask;                 // [points] inlier flags of the current matrix (zero for a pair without a winner)
  int32_t* inlier_idx;           // [points] per pair, from its start: the ascending (global) indices of its inliers
  int32_t* inlier_count;         // [num_pairs] their number; 0 for a pair that is done
};
// pair_winner_kernel: per pair the best of its tasks_per_pair scored hypotheses — most inliers, with front_breaks_ties (and num_front given)
// the most in front over the four candidates next, then the lowest task
struct WinnerArgs {
  PairLoopState S;
  int tasks_per_pair, front_breaks_ties;
  const uint8_t* status;         // [num_pairs][tasks_per_pair]
  const int32_t* num_inliers;    // [num_pairs][tasks_per_pair]
  const int32_t* num_front;      // [num_pairs][tasks_per_pair][4], or null
  const double* models;          // [num_pairs][tasks_per_pair][9]
  const double* poses;           // [num_pairs][tasks_per_pair][6], or null
};
// pair_adopt_kernel: the refit of each pair (one task per pair), adopted iff accepted and its count is not lower
struct AdoptArgs {
  PairLoopState S;
  const uint8_t* status;         // [num_pairs] the score kernel's
  const int32_t* num_inliers;    // [num_pairs]
  const int32_t* num_front;      // [num_pairs][4], or null
  const double* models;          // [num_pairs][9]
  const double* poses;           // [num_pairs][6], or null
};
// the inlier rule of the model: Sampson distance to E, or both transfer errors of H and its inverse
enum class PairRule { Sampson, Transfer };

hipError_t launch_pair_winner(const WinnerArgs& args, hipStream_t st);
// mask[i] of every correspondence of the pairs that are not done, from its pair's current matrix; first_point / num_points: the chunk's range,
// point_pair [points]: the chunk's pair of each correspondence
hipError_t launch_pair_masks(PairRule rule, const PairLoopState& S, const int32_t* point_pair, int first_point, int num_points, double thr2, const double* na,
                             const double* nb, hipStream_t st);
// inlier_idx / inlier_count from mask, in ascending order; a pair with fewer than min_refit inliers becomes done
hipError_t launch_pair_compact(const PairLoopState& S, int min_refit, hipStream_t st);
hipError_t launch_pair_adopt(const AdoptArgs& args, hipStream_t st);

}  // namespace rsba
