// What the C-ABI entry points of the two-view models share on the host (epipolar_capi.hip, homography_capi.hip): the argument checks and the
// normalisation of a single pair, and the staging of a batched call (rsba_epipolar_ransac_pairs, rsba_two_view_classify_pairs) — the pair
// table, the one upload, the state of the loop, the sequence of launches per chunk and the one download.  What differs between the two models
// is an argument here: the least sizes, the messages, the inlier rule, the model's own launches.  Host-side glue only; private to the library.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "capi_util.hpp"
#include "pair_loop_state.hpp"
#include "pnp_state.hpp"

#pragma GCC visibility push(hidden)

namespace rsba {

// ---- a single pair ----
inline int32_t check_points(const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n, int32_t min_n, const char* message) {
  if (!cam_a || !cam_b || !xy_a || !xy_b) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (n < min_n) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, message);
  return RSBA_OK;
}
inline int32_t check_subsets(int32_t n, const int32_t* subsets, int32_t m, int32_t num_tasks, int32_t min_m, const char* message) {
  if (!subsets) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (m < min_m || n < m || num_tasks <= 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, message);
  for (size_t k = 0; k < (size_t)num_tasks * m; ++k)
    if (subsets[k] < 0 || subsets[k] >= n) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "subset index out of range");
  return RSBA_OK;
}

// both frames' points uploaded, undistorted and normalised (pnp_normalise_kernel, once per side)
struct Normalised { double* na = nullptr; double* nb = nullptr; };
inline int32_t normalise_both(DeviceBuffers& B, Normalised& N, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n) {
  const double* cams[2] = {cam_a, cam_b};
  const float* xy[2] = {xy_a, xy_b};
  double** out[2] = {&N.na, &N.nb};
  for (int side = 0; side < 2; ++side) {
    PnpDltArgs D{};
    for (int k = 0; k < 9; ++k) D.cam[k] = cams[side][k];
    D.n = n;
    RSBA_HIP_TRY(B.upload(&D.image_points, xy[side], (size_t)n * 2));
    RSBA_HIP_TRY(B.alloc(&D.normalised, (size_t)n * 2));
    RSBA_HIP_TRY(launch_pnp_normalise(D, nullptr));
    *out[side] = D.normalised;
  }
  return RSBA_OK;
}

inline double mean_focal2(const double* cam_a, const double* cam_b) {
  const double f = (cam_a[0] + cam_a[1] + cam_b[0] + cam_b[1]) / 4.0;
  return f * f;
}

// ---- many pairs in one call ----
constexpr int32_t kDefaultTasksPerLaunch = 65536;   // five-point scratch is about 1.5 KB per task: 100 MB at this budget

// one side of every pair normalised by its own camera: pnp_normalise_kernel itself (the kernel the single-pair calls run, so the same
// bytes), once per run of consecutive pairs that share the camera — a session with one camera takes one launch per side
inline int32_t normalise_pairs(const double* cams, const int32_t* pair_cam, const int32_t* pair_offset, int32_t num_pairs, const float* d_xy, double* d_out) {
  for (int32_t p = 0; p < num_pairs;) {
    int32_t q = p + 1;
    while (q < num_pairs && pair_cam[q] == pair_cam[p]) ++q;
    const int32_t first = pair_offset[p], count = pair_offset[q] - first;
    if (count > 0) {
      PnpDltArgs D{};
      for (int k = 0; k < 9; ++k) D.cam[k] = cams[(size_t)pair_cam[p] * 9 + k];
      D.n = count; D.image_points = d_xy + 2 * (size_t)first; D.normalised = d_out + 2 * (size_t)first;
      RSBA_HIP_TRY(launch_pnp_normalise(D, nullptr));
    }
    p = q;
  }
  return RSBA_OK;
}

inline int32_t check_pair_table(int32_t num_cams, const int32_t* pair_cam_a, const int32_t* pair_cam_b, const int32_t* pair_offset, int32_t num_pairs) {
  if (pair_offset[0] != 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "pair_offset[0] is not 0");
  for (int32_t p = 0; p < num_pairs; ++p) {
    if (pair_offset[p + 1] < pair_offset[p]) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "pair_offset decreases");
    if (pair_cam_a[p] < 0 || pair_cam_a[p] >= num_cams || pair_cam_b[p] < 0 || pair_cam_b[p] >= num_cams)
      return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "camera index out of range");
  }
  return RSBA_OK;
}

// whole pairs per launch; a pair above the budget is a chunk of its own
inline int32_t pairs_per_launch(int32_t num_pairs, int32_t tasks_per_pair, int32_t max_tasks_per_launch) {
  const int32_t budget = max_tasks_per_launch ? max_tasks_per_launch : kDefaultTasksPerLaunch;
  return (int32_t)std::min<int64_t>(num_pairs, std::max<int64_t>(1, budget / tasks_per_pair));
}

// what a batched call holds on the device for all its pairs
struct PairStaging {
  DeviceBuffers B;
  int32_t num_pairs = 0, chunk_pairs = 0;
  size_t per_pair = 0, points = 0;         // subset indices per pair, correspondences of all pairs
  const int32_t* pair_offset = nullptr;    // (the caller's, on the host)
  double* na = nullptr;                    // [points][2] normalised
  double* nb = nullptr;
  const int32_t* subsets = nullptr;        // [num_pairs][per_pair] indices of the concatenated points
  const int32_t* starts = nullptr;         // [num_pairs] PairRange::start, the refit lists' sub_start
  const int32_t* point_pair = nullptr;     // [points] the pair's index within its chunk
  const PairRange* table = nullptr;        // [num_pairs]
  PairLoopState all{};                     // the state of the loop, every pair's; a chunk works on its slice
};
struct PairChunk {
  int32_t p0, np, first_point, num_points;
  PairLoopState S;
};

// Pair-local subset indices to indices of the concatenated points — a pair under min_n correspondences gets the repeated index 0, which
// every hypothesis kernel declines before it reads a point, and its part of the caller's array is not read — the pair table, then the one
// upload and the normalisation of both sides.
inline int32_t stage_pairs(PairStaging& G, int32_t device, const double* cams, const int32_t* pair_cam_a, const int32_t* pair_cam_b, const int32_t* pair_offset,
                           int32_t num_pairs, const float* xy_a, const float* xy_b, const int32_t* subsets, int32_t m, int32_t tasks_per_pair, int32_t chunk_pairs, int32_t min_n) {
  G.num_pairs = num_pairs; G.chunk_pairs = chunk_pairs; G.pair_offset = pair_offset;
  G.per_pair = (size_t)tasks_per_pair * m; G.points = (size_t)pair_offset[num_pairs];
  const size_t per_pair = G.per_pair, points = G.points;
  std::vector<int32_t> global((size_t)num_pairs * per_pair, 0);
  std::vector<PairRange> table((size_t)num_pairs);
  std::vector<int32_t> starts((size_t)num_pairs), point_pair(points);
  for (int32_t p = 0; p < num_pairs; ++p) {
    const int32_t first = pair_offset[p], n = pair_offset[p + 1] - first;
    table[(size_t)p] = PairRange{first, n, mean_focal2(cams + 9 * (size_t)pair_cam_a[p], cams + 9 * (size_t)pair_cam_b[p])};
    starts[(size_t)p] = first;
    for (int32_t i = 0; i < n; ++i) point_pair[(size_t)first + i] = p % chunk_pairs;
    if (n < min_n) continue;
    for (size_t k = 0; k < per_pair; ++k) {
      const int32_t s = subsets[(size_t)p * per_pair + k];
      if (s < 0 || s >= n) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "subset index out of range");
      global[(size_t)p * per_pair + k] = first + s;
    }
  }
  int32_t rc = rsba_select_device(device);
  if (rc) return rc;
  DeviceBuffers& B = G.B;
  const float* d_xy[2] = {nullptr, nullptr};
  RSBA_HIP_TRY(B.upload(&d_xy[0], xy_a, points * 2));
  RSBA_HIP_TRY(B.upload(&d_xy[1], xy_b, points * 2));
  RSBA_HIP_TRY(B.alloc(&G.na, points * 2));
  RSBA_HIP_TRY(B.alloc(&G.nb, points * 2));
  RSBA_HIP_TRY(B.upload(&G.subsets, global.data(), global.size()));
  RSBA_HIP_TRY(B.upload(&G.starts, starts.data(), starts.size()));
  RSBA_HIP_TRY(B.upload(&G.point_pair, point_pair.data(), point_pair.size()));
  RSBA_HIP_TRY(B.upload(&G.table, table.data(), table.size()));
  if ((rc = normalise_pairs(cams, pair_cam_a, pair_offset, num_pairs, d_xy[0], G.na))) return rc;
  return normalise_pairs(cams, pair_cam_b, pair_offset, num_pairs, d_xy[1], G.nb);
}

// the state of the loop allocated, the matrices (and poses) and the flags zeroed; with_pose: the pose and the four front counts as well
inline int32_t alloc_pair_loop(PairStaging& G, bool with_pose) {
  DeviceBuffers& B = G.B;
  PairLoopState& all = G.all;
  const size_t P = (size_t)G.num_pairs, points = G.points;
  RSBA_HIP_TRY(B.alloc(&all.model, P * 9));
  if (with_pose) RSBA_HIP_TRY(B.alloc(&all.pose, P * 6));
  RSBA_HIP_TRY(B.alloc(&all.num_inliers, P));
  if (with_pose) RSBA_HIP_TRY(B.alloc(&all.num_front, P * 4));
  RSBA_HIP_TRY(B.alloc(&all.winner_task, P));
  RSBA_HIP_TRY(B.alloc(&all.refits_adopted, P));
  RSBA_HIP_TRY(B.alloc(&all.status, P));
  RSBA_HIP_TRY(B.alloc(&all.done, P));
  RSBA_HIP_TRY(B.alloc(&all.inlier_count, P));
  RSBA_HIP_TRY(B.alloc(&all.mask, points));
  RSBA_HIP_TRY(B.alloc(&all.inlier_idx, points));
  RSBA_HIP_TRY(hipMemset(all.model, 0, P * 9 * sizeof(double)));
  if (with_pose) RSBA_HIP_TRY(hipMemset(all.pose, 0, P * 6 * sizeof(double)));
  RSBA_HIP_TRY(hipMemset(all.mask, 0, points ? points : 1));
  return RSBA_OK;
}

// the chunk that starts at pair p0: its pairs, its range of the points, its slice of the state
inline PairChunk pair_chunk(const PairStaging& G, int32_t p0) {
  PairChunk K{};
  K.p0 = p0; K.np = std::min(G.chunk_pairs, G.num_pairs - p0);
  K.first_point = G.pair_offset[p0]; K.num_points = G.pair_offset[p0 + K.np] - K.first_point;
  PairLoopState& C = K.S;
  C = G.all;
  C.num_pairs = K.np; C.pairs = G.table + p0;
  C.model += (size_t)p0 * 9; C.num_inliers += p0; C.winner_task += p0; C.refits_adopted += p0; C.status += p0; C.done += p0; C.inlier_count += p0;
  if (C.pose) { C.pose += (size_t)p0 * 6; C.num_front += (size_t)p0 * 4; }
  return K;
}

// The loop of a chunk after its hypotheses are scored, a fixed sequence of launches with nothing read back between them: the winner and its
// flags, then `refits` rounds of compact, fit over the inlier lists, score, adopt, flags.  W and D name the scored hypotheses and the scored
// refits (their S is set here); refit() launches the model's fit kernel over the lists and its score kernel, one task per pair.  Every round
// is launched: a pair that is done is skipped by the kernels.
template <class Refit>
inline int32_t run_pair_loop(const PairStaging& G, const PairChunk& K, WinnerArgs W, AdoptArgs D, PairRule rule, int min_refit, int32_t refits, double thr2, Refit&& refit) {
  W.S = D.S = K.S;
  RSBA_HIP_TRY(launch_pair_winner(W, nullptr));
  RSBA_HIP_TRY(launch_pair_masks(rule, K.S, G.point_pair, K.first_point, K.num_points, thr2, G.na, G.nb, nullptr));
  for (int32_t round = 0; round < refits; ++round) {
    RSBA_HIP_TRY(launch_pair_compact(K.S, min_refit, nullptr));
    const int32_t rc = refit();
    if (rc) return rc;
    RSBA_HIP_TRY(launch_pair_adopt(D, nullptr));
    RSBA_HIP_TRY(launch_pair_masks(rule, K.S, G.point_pair, K.first_point, K.num_points, thr2, G.na, G.nb, nullptr));
  }
  return RSBA_OK;
}

// The one download of what both calls return; the matrix of a pair without a winner stays the caller's.  A call fetches its own device arrays
// into host memory before this, so that nothing of the caller's is written before every copy has succeeded; st: the status bytes, for the
// call's own outputs.
inline int32_t download_pairs(const PairStaging& G, uint8_t* status, int32_t* winner_task, int32_t* refits_adopted, int32_t* num_inliers, uint8_t* inlier_mask,
                              double* model_out, std::vector<uint8_t>& st) {
  const size_t P = (size_t)G.num_pairs, points = G.points;
  const PairLoopState& all = G.all;
  std::vector<double> model(P * 9);
  std::vector<uint8_t> mask(points);
  std::vector<int32_t> win(P), adopted(P), inl(P);
  st.resize(P);
  RSBA_HIP_TRY(hipMemcpy(model.data(), all.model, model.size() * sizeof(double), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(st.data(), all.status, st.size(), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(win.data(), all.winner_task, win.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(adopted.data(), all.refits_adopted, adopted.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(inl.data(), all.num_inliers, inl.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (points) RSBA_HIP_TRY(hipMemcpy(mask.data(), all.mask, points, hipMemcpyDeviceToHost));
  for (size_t p = 0; p < P; ++p) {
    status[p] = st[p]; winner_task[p] = win[p]; refits_adopted[p] = adopted[p]; num_inliers[p] = inl[p];
    if (st[p]) for (int k = 0; k < 9; ++k) model_out[p * 9 + k] = model[p * 9 + k];
  }
  for (size_t i = 0; i < points; ++i) inlier_mask[i] = mask[i];
  return RSBA_OK;
}

}  // namespace rsba

#pragma GCC visibility pop
