// C-ABI of the two-view bootstrap (include/rsba_amd.h: rsba_epipolar_eight_point, rsba_epipolar_score, rsba_epipolar_hypotheses,
// rsba_epipolar_inliers, rsba_epipolar_five_point, rsba_epipolar_hypotheses_five_point, rsba_epipolar_ransac_pairs).  Host-side glue only:
// argument checks (the codes rsba_pnp_dlt returns for the same mistakes), staging of the caller's arrays and the launches; what it shares with
// homography_capi.hip is pair_capi_util.hpp.  Every number comes from kernels_epipolar.hip, kernels_five_point.hip and pnp_normalise_kernel
// (kernels_pnp_dlt.hip).
#include "../../include/rsba_amd.h"

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "epipolar_state.hpp"
#include "pair_capi_util.hpp"

using namespace rsba;

namespace {

constexpr const char* kTooFewPoints = "bad sizes (an essential matrix takes at least 8 correspondences)";
constexpr const char* kBadSubsets = "bad sizes (an eight-point subset has at least 8 correspondences, n >= m)";
constexpr const char* kTooFewPointsFive = "bad sizes (the five-point solver takes at least 5 correspondences)";

int32_t run_eight_point(DeviceBuffers& B, EpiEightArgs& A, const Normalised& N, int32_t n, const int32_t* subsets, int32_t m, int32_t num_tasks) {
  A.n = n; A.m = m; A.num_tasks = num_tasks; A.na = N.na; A.nb = N.nb;
  RSBA_HIP_TRY(B.upload(&A.subsets, subsets, (size_t)num_tasks * m));
  RSBA_HIP_TRY(B.alloc(&A.E_out, (size_t)num_tasks * 9));
  RSBA_HIP_TRY(B.alloc(&A.status, (size_t)num_tasks));
  RSBA_HIP_TRY(hipMemset(A.E_out, 0, (size_t)num_tasks * 9 * sizeof(double)));
  RSBA_HIP_TRY(launch_epipolar_eight_point(A, nullptr));
  return RSBA_OK;
}

// S.E / S.status_in set by the caller; the outputs are allocated here and stay on the device
int32_t run_score(DeviceBuffers& B, EpiScoreArgs& S, const Normalised& N, const double* cam_a, const double* cam_b, int32_t n, int32_t num_tasks, double threshold_px) {
  S.n = n; S.num_tasks = num_tasks; S.na = N.na; S.nb = N.nb;
  S.f2 = mean_focal2(cam_a, cam_b); S.thr2 = threshold_px * threshold_px;
  RSBA_HIP_TRY(B.alloc(&S.num_inliers, (size_t)num_tasks));
  RSBA_HIP_TRY(B.alloc(&S.num_front, (size_t)num_tasks * 4));
  RSBA_HIP_TRY(B.alloc(&S.poses_out, (size_t)num_tasks * 6));
  RSBA_HIP_TRY(B.alloc(&S.status, (size_t)num_tasks));
  RSBA_HIP_TRY(hipMemset(S.poses_out, 0, (size_t)num_tasks * 6 * sizeof(double)));
  RSBA_HIP_TRY(launch_epipolar_score(S, nullptr));
  return RSBA_OK;
}

// counts, status and the accepted tasks' poses to the caller's arrays (declined pose slots are left as they are)
int32_t download_score(const EpiScoreArgs& S, int32_t num_tasks, int32_t* num_inliers, int32_t* num_front, double* poses_out, uint8_t* status, std::vector<uint8_t>& st) {
  RSBA_HIP_TRY(hipMemcpy(num_inliers, S.num_inliers, (size_t)num_tasks * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(num_front, S.num_front, (size_t)num_tasks * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return download_accepted(S.status, S.poses_out, 6, num_tasks, status, poses_out, st);
}

}  // namespace

extern "C" int32_t rsba_epipolar_eight_point(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                             const int32_t* subsets, int32_t m, int32_t num_tasks, double* E_out, uint8_t* status) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 8, kTooFewPoints);
  if (rc) return rc;
  if (!E_out || !status) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets(n, subsets, m, num_tasks, 8, kBadSubsets))) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  EpiEightArgs A{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  if ((rc = run_eight_point(B, A, N, n, subsets, m, num_tasks))) return rc;
  std::vector<uint8_t> st;
  return download_accepted(A.status, A.E_out, 9, num_tasks, status, E_out, st);
}

extern "C" int32_t rsba_epipolar_score(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                       const double* E, int32_t num_tasks, double threshold_px, int32_t* num_inliers, int32_t* num_front,
                                       double* poses_out, uint8_t* status) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 8, kTooFewPoints);
  if (rc) return rc;
  if (!E || !num_inliers || !num_front || !poses_out || !status) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (num_tasks <= 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (num_tasks <= 0)");
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  EpiScoreArgs S{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  RSBA_HIP_TRY(B.upload(&S.E, E, (size_t)num_tasks * 9));
  if ((rc = run_score(B, S, N, cam_a, cam_b, n, num_tasks, threshold_px))) return rc;
  std::vector<uint8_t> st;
  return download_score(S, num_tasks, num_inliers, num_front, poses_out, status, st);
}

extern "C" int32_t rsba_epipolar_hypotheses(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                            const int32_t* subsets, int32_t m, int32_t num_tasks, double threshold_px, double* E_out, double* poses_out,
                                            uint8_t* status, int32_t* num_inliers, int32_t* num_front) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 8, kTooFewPoints);
  if (rc) return rc;
  if (!E_out || !poses_out || !status || !num_inliers || !num_front) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets(n, subsets, m, num_tasks, 8, kBadSubsets))) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  EpiEightArgs A{};
  EpiScoreArgs S{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  if ((rc = run_eight_point(B, A, N, n, subsets, m, num_tasks))) return rc;
  S.E = A.E_out; S.status_in = A.status;   // E stays on the device between the two kernels
  if ((rc = run_score(B, S, N, cam_a, cam_b, n, num_tasks, threshold_px))) return rc;
  std::vector<uint8_t> st;
  if ((rc = download_score(S, num_tasks, num_inliers, num_front, poses_out, status, st))) return rc;
  return download_accepted(nullptr, A.E_out, 9, num_tasks, status, E_out, st);   // (st: the score kernel's, downloaded above)
}

extern "C" int32_t rsba_epipolar_inliers(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                         const double* E, double threshold_px, uint8_t* inlier_mask) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 8, kTooFewPoints);
  if (rc) return rc;
  if (!E || !inlier_mask) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  EpiScoreArgs S{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  S.n = n; S.num_tasks = 1; S.na = N.na; S.nb = N.nb; S.f2 = mean_focal2(cam_a, cam_b); S.thr2 = threshold_px * threshold_px;
  RSBA_HIP_TRY(B.upload(&S.E, E, 9));
  uint8_t* d_mask = nullptr;
  RSBA_HIP_TRY(B.alloc(&d_mask, (size_t)n));
  RSBA_HIP_TRY(launch_epipolar_inliers(S, d_mask, nullptr));
  RSBA_HIP_TRY(hipMemcpy(inlier_mask, d_mask, (size_t)n, hipMemcpyDeviceToHost));
  return RSBA_OK;
}

// ---- the five-point solver beside the eight-point: the same order of argument checks, n >= 5, exactly five indices per subset ----
namespace {

int32_t check_subsets_five(int32_t n, const int32_t* subsets, int32_t num_tasks) {
  if (!subsets) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (num_tasks <= 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (num_tasks <= 0)");
  for (size_t k = 0; k < (size_t)num_tasks * 5; ++k)
    if (subsets[k] < 0 || subsets[k] >= n) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "subset index out of range");
  return RSBA_OK;
}

int32_t run_five_point(DeviceBuffers& B, EpiFiveArgs& F, const Normalised& N, int32_t n, const int32_t* subsets, int32_t num_tasks) {
  F.n = n; F.num_tasks = num_tasks; F.na = N.na; F.nb = N.nb;
  RSBA_HIP_TRY(B.upload(&F.subsets, subsets, (size_t)num_tasks * 5));
  RSBA_HIP_TRY(B.alloc(&F.E_out, (size_t)num_tasks * 90));
  RSBA_HIP_TRY(B.alloc(&F.num_solutions, (size_t)num_tasks));
  RSBA_HIP_TRY(B.alloc(&F.slot_status, (size_t)num_tasks * 10));
  RSBA_HIP_TRY(B.alloc(&F.status, (size_t)num_tasks));
  RSBA_HIP_TRY(hipMemset(F.E_out, 0, (size_t)num_tasks * 90 * sizeof(double)));
  RSBA_HIP_TRY(launch_epipolar_five_point(F, nullptr));
  return RSBA_OK;
}

}  // namespace

extern "C" int32_t rsba_epipolar_five_point(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                            const int32_t* subsets, int32_t num_tasks, double* E_out, int32_t* num_solutions, uint8_t* status) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 5, kTooFewPointsFive);
  if (rc) return rc;
  if (!E_out || !num_solutions || !status) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets_five(n, subsets, num_tasks))) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  EpiFiveArgs F{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  if ((rc = run_five_point(B, F, N, n, subsets, num_tasks))) return rc;
  std::vector<double> values((size_t)num_tasks * 90);
  std::vector<int32_t> counts((size_t)num_tasks);
  RSBA_HIP_TRY(hipMemcpy(values.data(), F.E_out, values.size() * sizeof(double), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(counts.data(), F.num_solutions, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(status, F.status, (size_t)num_tasks, hipMemcpyDeviceToHost));
  for (size_t t = 0; t < (size_t)num_tasks; ++t) {   // the written slots only: the rest of E_out stays the caller's
    num_solutions[t] = counts[t];
    for (size_t k = 0; k < (size_t)counts[t] * 9; ++k) E_out[t * 90 + k] = values[t * 90 + k];
  }
  return RSBA_OK;
}

extern "C" int32_t rsba_epipolar_hypotheses_five_point(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                                       const int32_t* subsets, int32_t num_tasks, double threshold_px, double* E_out, double* poses_out,
                                                       uint8_t* status, int32_t* num_inliers, int32_t* num_front, int32_t* num_solutions) {
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 5, kTooFewPointsFive);
  if (rc) return rc;
  if (!E_out || !poses_out || !status || !num_inliers || !num_front) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets_five(n, subsets, num_tasks))) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  Normalised N;
  EpiFiveArgs F{};
  EpiScoreArgs S{};
  EpiPickArgs P{};
  if ((rc = normalise_both(B, N, cam_a, cam_b, xy_a, xy_b, n))) return rc;
  if ((rc = run_five_point(B, F, N, n, subsets, num_tasks))) return rc;
  S.E = F.E_out; S.status_in = F.slot_status;   // every slot is a task of the score kernel; the solutions stay on the device
  if ((rc = run_score(B, S, N, cam_a, cam_b, n, num_tasks * 10, threshold_px))) return rc;
  P.num_tasks = num_tasks; P.slot_status = S.status; P.slot_inliers = S.num_inliers; P.slot_front = S.num_front; P.slot_E = F.E_out; P.slot_poses = S.poses_out;
  RSBA_HIP_TRY(B.alloc(&P.E_out, (size_t)num_tasks * 9));
  RSBA_HIP_TRY(B.alloc(&P.poses_out, (size_t)num_tasks * 6));
  RSBA_HIP_TRY(B.alloc(&P.num_inliers, (size_t)num_tasks));
  RSBA_HIP_TRY(B.alloc(&P.num_front, (size_t)num_tasks * 4));
  RSBA_HIP_TRY(B.alloc(&P.status, (size_t)num_tasks));
  RSBA_HIP_TRY(hipMemset(P.E_out, 0, (size_t)num_tasks * 9 * sizeof(double)));
  RSBA_HIP_TRY(hipMemset(P.poses_out, 0, (size_t)num_tasks * 6 * sizeof(double)));
  RSBA_HIP_TRY(launch_epipolar_pick(P, nullptr));
  RSBA_HIP_TRY(hipMemcpy(num_inliers, P.num_inliers, (size_t)num_tasks * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(num_front, P.num_front, (size_t)num_tasks * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (num_solutions) RSBA_HIP_TRY(hipMemcpy(num_solutions, F.num_solutions, (size_t)num_tasks * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<uint8_t> st;
  if ((rc = download_accepted(P.status, P.poses_out, 6, num_tasks, status, poses_out, st))) return rc;
  return download_accepted(nullptr, P.E_out, 9, num_tasks, status, E_out, st);
}

// ---- the RANSAC of many frame pairs in one call: the hypothesis kernels above over the concatenated points, the loop of
// epi_detail::ransac per pair kept on the device.  The staging and the loop are pair_capi_util.hpp's and kernels_pair_loop.hip's, shared with
// the homography; here, what is the essential matrix's own: the two hypothesis stages, the pose and the front counts ----
extern "C" int32_t rsba_epipolar_ransac_pairs(int32_t device, const double* cams, int32_t num_cams, const int32_t* pair_cam_a, const int32_t* pair_cam_b,
                                              const int32_t* pair_offset, int32_t num_pairs, const float* xy_a, const float* xy_b, const int32_t* subsets, int32_t m,
                                              int32_t tasks_per_pair, double threshold_px, int32_t refits, int32_t max_tasks_per_launch, double* E_out, double* poses_out,
                                              uint8_t* status, int32_t* winner_task, int32_t* refits_adopted, int32_t* num_inliers, int32_t* num_front, uint8_t* inlier_mask) {
  if (!cams || !pair_cam_a || !pair_cam_b || !pair_offset || !xy_a || !xy_b || !subsets || !E_out || !poses_out || !status || !winner_task || !refits_adopted ||
      !num_inliers || !num_front || !inlier_mask)
    return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (num_cams <= 0 || num_pairs <= 0 || tasks_per_pair <= 0 || refits < 0 || max_tasks_per_launch < 0)
    return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (num_cams, num_pairs, tasks_per_pair > 0; refits, max_tasks_per_launch >= 0)");
  if (m != 5 && m != 8) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (m is 5, five-point subsets, or 8, eight-point subsets)");
  int32_t rc = check_pair_table(num_cams, pair_cam_a, pair_cam_b, pair_offset, num_pairs);
  if (rc) return rc;
  const int32_t chunk_pairs = pairs_per_launch(num_pairs, tasks_per_pair, max_tasks_per_launch);
  if ((int64_t)chunk_pairs * tasks_per_pair * 10 > INT32_MAX) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (tasks per launch)");
  PairStaging G;
  if ((rc = stage_pairs(G, device, cams, pair_cam_a, pair_cam_b, pair_offset, num_pairs, xy_a, xy_b, subsets, m, tasks_per_pair, chunk_pairs, 8))) return rc;
  if ((rc = alloc_pair_loop(G, true))) return rc;
  DeviceBuffers& B = G.B;

  // scratch of the largest chunk: the hypotheses of its tasks (five-point: ten slots per task), the refit of its pairs
  const size_t T = (size_t)chunk_pairs * tasks_per_pair, slots = m == 5 ? T * 10 : T;
  EpiEightArgs A{};
  EpiFiveArgs F{};
  EpiScoreArgs S{};
  EpiPickArgs K{};
  EpiEightArgs RA{};
  EpiScoreArgs RS{};
  A.na = F.na = S.na = RA.na = RS.na = G.na;
  A.nb = F.nb = S.nb = RA.nb = RS.nb = G.nb;
  A.n = F.n = RA.n = (int)G.points;
  S.thr2 = RS.thr2 = threshold_px * threshold_px;
  if (m == 5) {
    RSBA_HIP_TRY(B.alloc(&F.E_out, T * 90));
    RSBA_HIP_TRY(B.alloc(&F.num_solutions, T));
    RSBA_HIP_TRY(B.alloc(&F.slot_status, T * 10));
    RSBA_HIP_TRY(B.alloc(&F.status, T));
    S.E = F.E_out; S.status_in = F.slot_status; S.tasks_per_pair = tasks_per_pair * 10;
    RSBA_HIP_TRY(B.alloc(&K.E_out, T * 9));
    RSBA_HIP_TRY(B.alloc(&K.poses_out, T * 6));
    RSBA_HIP_TRY(B.alloc(&K.num_inliers, T));
    RSBA_HIP_TRY(B.alloc(&K.num_front, T * 4));
    RSBA_HIP_TRY(B.alloc(&K.status, T));
  } else {
    A.m = 8;
    RSBA_HIP_TRY(B.alloc(&A.E_out, T * 9));
    RSBA_HIP_TRY(B.alloc(&A.status, T));
    S.E = A.E_out; S.status_in = A.status; S.tasks_per_pair = tasks_per_pair;
  }
  RSBA_HIP_TRY(B.alloc(&S.num_inliers, slots));
  RSBA_HIP_TRY(B.alloc(&S.num_front, slots * 4));
  RSBA_HIP_TRY(B.alloc(&S.poses_out, slots * 6));
  RSBA_HIP_TRY(B.alloc(&S.status, slots));
  if (m == 5) { K.slot_status = S.status; K.slot_inliers = S.num_inliers; K.slot_front = S.num_front; K.slot_E = F.E_out; K.slot_poses = S.poses_out; }
  RSBA_HIP_TRY(B.alloc(&RA.E_out, (size_t)chunk_pairs * 9));
  RSBA_HIP_TRY(B.alloc(&RA.status, (size_t)chunk_pairs));
  RS.E = RA.E_out; RS.status_in = RA.status; RS.tasks_per_pair = 1;
  RSBA_HIP_TRY(B.alloc(&RS.num_inliers, (size_t)chunk_pairs));
  RSBA_HIP_TRY(B.alloc(&RS.num_front, (size_t)chunk_pairs * 4));
  RSBA_HIP_TRY(B.alloc(&RS.poses_out, (size_t)chunk_pairs * 6));
  RSBA_HIP_TRY(B.alloc(&RS.status, (size_t)chunk_pairs));

  for (int32_t p0 = 0; p0 < num_pairs; p0 += chunk_pairs) {
    const PairChunk C = pair_chunk(G, p0);
    const int32_t tasks = C.np * tasks_per_pair;
    S.pairs = RS.pairs = C.S.pairs;
    WinnerArgs W{};
    W.tasks_per_pair = tasks_per_pair; W.front_breaks_ties = m == 5 ? 1 : 0;
    if (m == 5) {
      F.num_tasks = tasks; F.subsets = G.subsets + (size_t)p0 * G.per_pair;
      RSBA_HIP_TRY(launch_epipolar_five_point(F, nullptr));
      S.num_tasks = tasks * 10;
      RSBA_HIP_TRY(launch_epipolar_score(S, nullptr));
      K.num_tasks = tasks;
      RSBA_HIP_TRY(launch_epipolar_pick(K, nullptr));
      W.status = K.status; W.num_inliers = K.num_inliers; W.num_front = K.num_front; W.models = K.E_out; W.poses = K.poses_out;
    } else {
      A.num_tasks = tasks; A.subsets = G.subsets + (size_t)p0 * G.per_pair;
      RSBA_HIP_TRY(launch_epipolar_eight_point(A, nullptr));
      S.num_tasks = tasks;
      RSBA_HIP_TRY(launch_epipolar_score(S, nullptr));
      W.status = S.status; W.num_inliers = S.num_inliers; W.num_front = S.num_front; W.models = A.E_out; W.poses = S.poses_out;
    }
    RA.num_tasks = RS.num_tasks = C.np; RA.subsets = C.S.inlier_idx; RA.sub_start = G.starts + p0; RA.sub_count = C.S.inlier_count;
    AdoptArgs D{};
    D.status = RS.status; D.num_inliers = RS.num_inliers; D.num_front = RS.num_front; D.models = RA.E_out; D.poses = RS.poses_out;
    rc = run_pair_loop(G, C, W, D, PairRule::Sampson, 8, refits, S.thr2, [&]() -> int32_t {
      RSBA_HIP_TRY(launch_epipolar_eight_point(RA, nullptr));
      RSBA_HIP_TRY(launch_epipolar_score(RS, nullptr));
      return RSBA_OK;
    });
    if (rc) return rc;
  }

  // ---- one download; E and the pose of a pair without a winner stay the caller's ----
  std::vector<double> ps((size_t)num_pairs * 6);
  std::vector<int32_t> front((size_t)num_pairs * 4);
  std::vector<uint8_t> st;
  RSBA_HIP_TRY(hipMemcpy(ps.data(), G.all.pose, ps.size() * sizeof(double), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(front.data(), G.all.num_front, front.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if ((rc = download_pairs(G, status, winner_task, refits_adopted, num_inliers, inlier_mask, E_out, st))) return rc;
  for (size_t p = 0; p < (size_t)num_pairs; ++p) {
    for (int c = 0; c < 4; ++c) num_front[p * 4 + c] = front[p * 4 + c];
    if (st[p]) for (int k = 0; k < 6; ++k) poses_out[p * 6 + k] = ps[p * 6 + k];
  }
  return RSBA_OK;
}
