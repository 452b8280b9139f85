// C-ABI of the two-view degeneracy test (include/rsba_amd.h: rsba_homography_dlt, rsba_homography_score, rsba_homography_inliers,
// rsba_homography_hypotheses, rsba_two_view_classify_pairs).  Host-side glue only: argument checks (the codes rsba_epipolar_* return for the
// same mistakes), staging of the caller's arrays and the launches; every number comes from kernels_homography.hip and pnp_normalise_kernel
// (kernels_pnp_dlt.hip).
#include "../../include/rsba_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "capi_util.hpp"
#include "homography_state.hpp"
#include "pnp_state.hpp"

using namespace rsba;

namespace {

int32_t check_points(const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n) {
  if (!cam_a || !cam_b || !xy_a || !xy_b) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 4) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (a homography takes at least 4 correspondences)");
  return RSBA_OK;
}
int32_t check_subsets(int32_t n, const int32_t* subsets, int32_t m, int32_t num_tasks) {
  if (!subsets) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (m < 4 || n < m || num_tasks <= 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (a homography subset has at least 4 correspondences, n >= m)");
  for (size_t k = 0; k < (size_t)num_tasks * m; ++k)
    if (subsets[k] < 0 || subsets[k] >= n) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "subset index out of range");
  return RSBA_OK;
}

// both frames' points uploaded, undistorted and normalised (pnp_normalise_kernel, once per side)
struct Normalised { double* na = nullptr; double* nb = nullptr; };
int32_t normalise_both(DeviceBuffers& B, Normalised& N, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n) {
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

double mean_focal2(const double* cam_a, const double* cam_b) {
  const double f = (cam_a[0] + cam_a[1] + cam_b[0] + cam_b[1]) / 4.0;
  return f * f;
}

int32_t run_dlt(DeviceBuffers& B, HomoDltArgs& A, const Normalised& N, int32_t n, const int32_t* subsets, int32_t m, int32_t num_tasks) {
  A.n = n; A.m = m; A.num_tasks = num_tasks; A.na = N.na; A.nb = N.nb;
  RSBA_HIP_TRY(B.upload(&A.subsets, subsets, (size_t)num_tasks * m));
  RSBA_HIP_TRY(B.alloc(&A.H_out, (size_t)num_tasks * 9));
  RSBA_HIP_TRY(B.alloc(&A.status, (size_t)num_tasks));
  RSBA_HIP_TRY(hipMemset(A.H_out, 0, (size_t)num_tasks * 9 * sizeof(double)));
  RSBA_HIP_TRY(launch_homography_dlt(A, nullptr));
  return RSBA_OK;
}

// S.H / S.status_in set by the caller; the outputs are allocated here and stay on the device
int32_t run_score(DeviceBuffers& B, HomoScoreArgs& S, const Normalised& N, const double* cam_a, const double* cam_b, int32_t n, int32_t num_tasks, double threshold_px) {
  S.n = n; S.num_tasks = num_tasks; S.na = N.na; S.nb = N.nb;
  S.f2 = mean_focal2(cam_a, cam_b); S.thr2 = threshold_px * threshold_px;
  RSBA_HIP_TRY(B.alloc(&S.num_inliers, (size_t)num_tasks));
  RSBA_HIP_TRY(B.alloc(&S.status, (size_t)num_tasks));
  RSBA_HIP_TRY(launch_homography_score(S, nullptr));
  return RSBA_OK;
}

int32_t download_score(const HomoScoreArgs& S, int32_t num_tasks, int32_t* num_inliers, uint8_t* status) {
  RSBA_HIP_TRY(hipMemcpy(num_inliers, S.num_inliers, (size_t)num_tasks * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(status, S.status, (size_t)num_tasks, hipMemcpyDeviceToHost));
  return RSBA_OK;
}

}  // namespace

extern "C" int32_t rsba_homography_dlt(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                       const int32_t* subsets, int32_t m, int32_t num_tasks, double* H_out, uint8_t* status) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n);
  if (rc) return rc;
  if (!H_out || !status) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets(n, subsets, m, num_tasks))) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  HomoDltArgs A{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  if ((rc = run_dlt(B, A, N, n, subsets, m, num_tasks))) return rc;
  std::vector<uint8_t> st;
  return download_accepted(A.status, A.H_out, 9, num_tasks, status, H_out, st);
}

extern "C" int32_t rsba_homography_score(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                         const double* H, int32_t num_tasks, double threshold_px, int32_t* num_inliers, uint8_t* status) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n);
  if (rc) return rc;
  if (!H || !num_inliers || !status) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (num_tasks <= 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (num_tasks <= 0)");
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  HomoScoreArgs S{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  RSBA_HIP_TRY(B.upload(&S.H, H, (size_t)num_tasks * 9));
  if ((rc = run_score(B, S, N, cam_a, cam_b, n, num_tasks, threshold_px))) return rc;
  return download_score(S, num_tasks, num_inliers, status);
}

extern "C" int32_t rsba_homography_hypotheses(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                              const int32_t* subsets, int32_t m, int32_t num_tasks, double threshold_px, double* H_out, uint8_t* status,
                                              int32_t* num_inliers) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n);
  if (rc) return rc;
  if (!H_out || !status || !num_inliers) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets(n, subsets, m, num_tasks))) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  HomoDltArgs A{};
  HomoScoreArgs S{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  if ((rc = run_dlt(B, A, N, n, subsets, m, num_tasks))) return rc;
  S.H = A.H_out; S.status_in = A.status;   // H stays on the device between the two kernels
  if ((rc = run_score(B, S, N, cam_a, cam_b, n, num_tasks, threshold_px))) return rc;
  RSBA_HIP_TRY(hipMemcpy(num_inliers, S.num_inliers, (size_t)num_tasks * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<uint8_t> st;
  return download_accepted(S.status, A.H_out, 9, num_tasks, status, H_out, st);
}

extern "C" int32_t rsba_homography_inliers(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                           const double* H, double threshold_px, uint8_t* inlier_mask) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n);
  if (rc) return rc;
  if (!H || !inlier_mask) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  HomoScoreArgs S{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  S.n = n; S.num_tasks = 1; S.na = N.na; S.nb = N.nb; S.f2 = mean_focal2(cam_a, cam_b); S.thr2 = threshold_px * threshold_px;
  RSBA_HIP_TRY(B.upload(&S.H, H, 9));
  uint8_t* d_mask = nullptr;
  RSBA_HIP_TRY(B.alloc(&d_mask, (size_t)n));
  RSBA_HIP_TRY(launch_homography_inliers(S, d_mask, nullptr));
  RSBA_HIP_TRY(hipMemcpy(inlier_mask, d_mask, (size_t)n, hipMemcpyDeviceToHost));
  return RSBA_OK;
}

// ---- the homography RANSAC and the parallax counts of many frame pairs in one call: the kernels above over the concatenated points, the
// loop of homo_detail::ransac per pair kept on the device (winner, masks, ordered compaction, adopt) ----
namespace {

constexpr int32_t kDefaultTasksPerLaunch = 65536;

// one side of every pair normalised by its own camera: pnp_normalise_kernel itself (the kernel the single-pair calls run, so the same
// bytes), once per run of consecutive pairs that share the camera
int32_t normalise_pairs(const double* cams, const int32_t* pair_cam, const int32_t* pair_offset, int32_t num_pairs, const float* d_xy, double* d_out) {
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

}  // namespace

extern "C" int32_t rsba_two_view_classify_pairs(int32_t device, const double* cams, int32_t num_cams, const int32_t* pair_cam_a, const int32_t* pair_cam_b,
                                                const int32_t* pair_offset, int32_t num_pairs, const float* xy_a, const float* xy_b, const double* E, const double* poses,
                                                const uint8_t* pair_status, const int32_t* subsets, int32_t tasks_per_pair, double threshold_px, int32_t refits,
                                                double cos_min_parallax, int32_t max_tasks_per_launch, double* H_out, uint8_t* h_status, int32_t* h_winner_task,
                                                int32_t* h_refits_adopted, int32_t* num_h_inliers, uint8_t* h_inlier_mask, int32_t* num_front, int32_t* num_parallax) {
  if (!cams || !pair_cam_a || !pair_cam_b || !pair_offset || !xy_a || !xy_b || !E || !poses || !pair_status || !subsets || !H_out || !h_status || !h_winner_task ||
      !h_refits_adopted || !num_h_inliers || !h_inlier_mask || !num_front || !num_parallax)
    return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (num_cams <= 0 || num_pairs <= 0 || tasks_per_pair <= 0 || refits < 0 || max_tasks_per_launch < 0)
    return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (num_cams, num_pairs, tasks_per_pair > 0; refits, max_tasks_per_launch >= 0)");
  if (!(cos_min_parallax >= -1.0 && cos_min_parallax <= 1.0)) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "cos_min_parallax is not a cosine");
  if (pair_offset[0] != 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "pair_offset[0] is not 0");
  for (int32_t p = 0; p < num_pairs; ++p) {
    if (pair_offset[p + 1] < pair_offset[p]) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "pair_offset decreases");
    if (pair_cam_a[p] < 0 || pair_cam_a[p] >= num_cams || pair_cam_b[p] < 0 || pair_cam_b[p] >= num_cams)
      return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "camera index out of range");
  }
  const int32_t budget = max_tasks_per_launch ? max_tasks_per_launch : kDefaultTasksPerLaunch;
  const int32_t chunk_pairs = std::min<int64_t>(num_pairs, std::max<int64_t>(1, budget / tasks_per_pair));   // whole pairs; a pair above the budget is a chunk of its own
  if ((int64_t)chunk_pairs * tasks_per_pair > INT32_MAX / 16) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (tasks per launch)");
  const size_t per_pair = (size_t)tasks_per_pair * 4, points = (size_t)pair_offset[num_pairs];
  // pair-local indices to indices of the concatenated points; a pair under 4 correspondences gets the repeated index 0, which the DLT
  // kernel declines before it reads a point, and its part of the caller's array is not read
  std::vector<int32_t> global((size_t)num_pairs * per_pair, 0);
  std::vector<HomoPair> table((size_t)num_pairs);
  std::vector<int32_t> starts((size_t)num_pairs), point_pair(points);
  for (int32_t p = 0; p < num_pairs; ++p) {
    const int32_t first = pair_offset[p], n = pair_offset[p + 1] - first;
    table[(size_t)p] = HomoPair{first, n, mean_focal2(cams + 9 * (size_t)pair_cam_a[p], cams + 9 * (size_t)pair_cam_b[p])};
    starts[(size_t)p] = first;
    for (int32_t i = 0; i < n; ++i) point_pair[(size_t)first + i] = p % chunk_pairs;   // the pair's index within its chunk
    if (n < 4) continue;
    for (size_t k = 0; k < per_pair; ++k) {
      const int32_t s = subsets[(size_t)p * per_pair + k];
      if (s < 0 || s >= n) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "subset index out of range");
      global[(size_t)p * per_pair + k] = first + s;
    }
  }
  int32_t rc = rsba_select_device(device);
  if (rc) return rc;

  // ---- one upload ----
  DeviceBuffers B;
  const float* d_xy[2] = {nullptr, nullptr};
  double* d_n[2] = {nullptr, nullptr};
  const int32_t* d_subsets = nullptr; const int32_t* d_starts = nullptr; const int32_t* d_point_pair = nullptr;
  const HomoPair* d_table = nullptr;
  ParallaxArgs X{};
  RSBA_HIP_TRY(B.upload(&d_xy[0], xy_a, points * 2));
  RSBA_HIP_TRY(B.upload(&d_xy[1], xy_b, points * 2));
  RSBA_HIP_TRY(B.alloc(&d_n[0], points * 2));
  RSBA_HIP_TRY(B.alloc(&d_n[1], points * 2));
  RSBA_HIP_TRY(B.upload(&d_subsets, global.data(), global.size()));
  RSBA_HIP_TRY(B.upload(&d_starts, starts.data(), starts.size()));
  RSBA_HIP_TRY(B.upload(&d_point_pair, point_pair.data(), point_pair.size()));
  RSBA_HIP_TRY(B.upload(&d_table, table.data(), table.size()));
  RSBA_HIP_TRY(B.upload(&X.E, E, (size_t)num_pairs * 9));
  RSBA_HIP_TRY(B.upload(&X.poses, poses, (size_t)num_pairs * 6));
  RSBA_HIP_TRY(B.upload(&X.pair_status, pair_status, (size_t)num_pairs));
  if ((rc = normalise_pairs(cams, pair_cam_a, pair_offset, num_pairs, d_xy[0], d_n[0]))) return rc;
  if ((rc = normalise_pairs(cams, pair_cam_b, pair_offset, num_pairs, d_xy[1], d_n[1]))) return rc;

  // the state of the loop, every pair's; a chunk works on its slice
  HomoPairState all{};
  RSBA_HIP_TRY(B.alloc(&all.H, (size_t)num_pairs * 9));
  RSBA_HIP_TRY(B.alloc(&all.num_inliers, (size_t)num_pairs));
  RSBA_HIP_TRY(B.alloc(&all.winner_task, (size_t)num_pairs));
  RSBA_HIP_TRY(B.alloc(&all.refits_adopted, (size_t)num_pairs));
  RSBA_HIP_TRY(B.alloc(&all.status, (size_t)num_pairs));
  RSBA_HIP_TRY(B.alloc(&all.done, (size_t)num_pairs));
  RSBA_HIP_TRY(B.alloc(&all.inlier_count, (size_t)num_pairs));
  RSBA_HIP_TRY(B.alloc(&all.mask, points));
  RSBA_HIP_TRY(B.alloc(&all.inlier_idx, points));
  RSBA_HIP_TRY(hipMemset(all.H, 0, (size_t)num_pairs * 9 * sizeof(double)));
  RSBA_HIP_TRY(hipMemset(all.mask, 0, points ? points : 1));

  // scratch of the largest chunk: the hypotheses of its tasks, the refit of its pairs
  const size_t T = (size_t)chunk_pairs * tasks_per_pair;
  HomoDltArgs A{}, RA{};
  HomoScoreArgs S{}, RS{};
  A.na = S.na = RA.na = RS.na = d_n[0];
  A.nb = S.nb = RA.nb = RS.nb = d_n[1];
  A.n = RA.n = (int)points;
  A.m = 4;
  S.thr2 = RS.thr2 = threshold_px * threshold_px;
  RSBA_HIP_TRY(B.alloc(&A.H_out, T * 9));
  RSBA_HIP_TRY(B.alloc(&A.status, T));
  S.H = A.H_out; S.status_in = A.status; S.tasks_per_pair = tasks_per_pair;
  RSBA_HIP_TRY(B.alloc(&S.num_inliers, T));
  RSBA_HIP_TRY(B.alloc(&S.status, T));
  RSBA_HIP_TRY(B.alloc(&RA.H_out, (size_t)chunk_pairs * 9));
  RSBA_HIP_TRY(B.alloc(&RA.status, (size_t)chunk_pairs));
  RS.H = RA.H_out; RS.status_in = RA.status; RS.tasks_per_pair = 1;
  RSBA_HIP_TRY(B.alloc(&RS.num_inliers, (size_t)chunk_pairs));
  RSBA_HIP_TRY(B.alloc(&RS.status, (size_t)chunk_pairs));

  // ---- per chunk a fixed sequence of launches, nothing read back between them ----
  for (int32_t p0 = 0; p0 < num_pairs; p0 += chunk_pairs) {
    const int32_t np = std::min(chunk_pairs, num_pairs - p0), tasks = np * tasks_per_pair;
    const int32_t first_point = pair_offset[p0], num_points = pair_offset[p0 + np] - first_point;
    HomoPairState C = all;
    C.num_pairs = np; C.pairs = d_table + p0;
    C.H += (size_t)p0 * 9; C.num_inliers += p0; C.winner_task += p0; C.refits_adopted += p0; C.status += p0; C.done += p0; C.inlier_count += p0;
    S.pairs = RS.pairs = C.pairs;
    A.num_tasks = S.num_tasks = tasks; A.subsets = d_subsets + (size_t)p0 * per_pair;
    RSBA_HIP_TRY(launch_homography_dlt(A, nullptr));
    RSBA_HIP_TRY(launch_homography_score(S, nullptr));
    HomoWinnerArgs W{};
    W.S = C; W.tasks_per_pair = tasks_per_pair; W.status = S.status; W.num_inliers = S.num_inliers; W.H = A.H_out;
    RSBA_HIP_TRY(launch_homography_winner(W, nullptr));
    RSBA_HIP_TRY(launch_homography_pair_masks(C, d_point_pair, first_point, num_points, S.thr2, d_n[0], d_n[1], nullptr));
    RA.num_tasks = RS.num_tasks = np; RA.subsets = C.inlier_idx; RA.sub_start = d_starts + p0; RA.sub_count = C.inlier_count;
    HomoAdoptArgs D{};
    D.S = C; D.status = RS.status; D.num_inliers = RS.num_inliers; D.H = RA.H_out;
    for (int32_t round = 0; round < refits; ++round) {   // every round is launched: a pair that is done is skipped by the kernels
      RSBA_HIP_TRY(launch_homography_compact(C, nullptr));
      RSBA_HIP_TRY(launch_homography_dlt(RA, nullptr));
      RSBA_HIP_TRY(launch_homography_score(RS, nullptr));
      RSBA_HIP_TRY(launch_homography_adopt(D, nullptr));
      RSBA_HIP_TRY(launch_homography_pair_masks(C, d_point_pair, first_point, num_points, S.thr2, d_n[0], d_n[1], nullptr));
    }
  }
  // the parallax counts: one wave per pair over the given E and pose, all pairs in one launch (a pair's counts are its own)
  X.num_pairs = num_pairs; X.pairs = d_table; X.na = d_n[0]; X.nb = d_n[1]; X.thr2 = S.thr2; X.cos_min = cos_min_parallax;
  RSBA_HIP_TRY(B.alloc(&X.num_front, (size_t)num_pairs));
  RSBA_HIP_TRY(B.alloc(&X.num_parallax, (size_t)num_pairs));
  RSBA_HIP_TRY(launch_two_view_parallax(X, nullptr));

  // ---- one download; H of a pair without a winner stays the caller's ----
  std::vector<double> h((size_t)num_pairs * 9);
  std::vector<uint8_t> st((size_t)num_pairs), mask(points);
  std::vector<int32_t> win((size_t)num_pairs), adopted((size_t)num_pairs), inl((size_t)num_pairs), front((size_t)num_pairs), par((size_t)num_pairs);
  RSBA_HIP_TRY(hipMemcpy(h.data(), all.H, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(st.data(), all.status, st.size(), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(win.data(), all.winner_task, win.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(adopted.data(), all.refits_adopted, adopted.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(inl.data(), all.num_inliers, inl.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(front.data(), X.num_front, front.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(par.data(), X.num_parallax, par.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (points) RSBA_HIP_TRY(hipMemcpy(mask.data(), all.mask, points, hipMemcpyDeviceToHost));
  for (size_t p = 0; p < (size_t)num_pairs; ++p) {
    h_status[p] = st[p]; h_winner_task[p] = win[p]; h_refits_adopted[p] = adopted[p]; num_h_inliers[p] = inl[p];
    num_front[p] = front[p]; num_parallax[p] = par[p];
    if (!st[p]) continue;
    for (int k = 0; k < 9; ++k) H_out[p * 9 + k] = h[p * 9 + k];
  }
  for (size_t i = 0; i < points; ++i) h_inlier_mask[i] = mask[i];
  return RSBA_OK;
}
