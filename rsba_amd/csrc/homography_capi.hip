// C-ABI of the two-view degeneracy test (include/rsba_amd.h: rsba_homography_dlt, rsba_homography_score, rsba_homography_inliers,
// rsba_homography_hypotheses, rsba_two_view_classify_pairs).  Host-side glue only: argument checks (the codes rsba_epipolar_* return for the
// same mistakes), staging of the caller's arrays and the launches; what it shares with epipolar_capi.hip is pair_capi_util.hpp.  Every
// number comes from kernels_homography.hip and pnp_normalise_kernel (kernels_pnp_dlt.hip).
#include "../../include/rsba_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "homography_state.hpp"
#include "pair_capi_util.hpp"

using namespace rsba;

namespace {

constexpr const char* kTooFewPoints = "bad sizes (a homography takes at least 4 correspondences)";
constexpr const char* kBadSubsets = "bad sizes (a homography subset has at least 4 correspondences, n >= m)";

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
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 4, kTooFewPoints);
  if (rc) return rc;
  if (!H_out || !status) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets(n, subsets, m, num_tasks, 4, kBadSubsets))) return rc;
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
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 4, kTooFewPoints);
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
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 4, kTooFewPoints);
  if (rc) return rc;
  if (!H_out || !status || !num_inliers) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets(n, subsets, m, num_tasks, 4, kBadSubsets))) return rc;
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
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n, 4, kTooFewPoints);
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
// loop of homo_detail::ransac per pair kept on the device.  The staging and the loop are pair_capi_util.hpp's and kernels_pair_loop.hip's,
// shared with the essential matrix; here, what is this call's own: the DLT stage and the parallax launch with its inputs ----
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
  int32_t rc = check_pair_table(num_cams, pair_cam_a, pair_cam_b, pair_offset, num_pairs);
  if (rc) return rc;
  const int32_t chunk_pairs = pairs_per_launch(num_pairs, tasks_per_pair, max_tasks_per_launch);
  if ((int64_t)chunk_pairs * tasks_per_pair > INT32_MAX / 16) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (tasks per launch)");
  PairStaging G;
  if ((rc = stage_pairs(G, device, cams, pair_cam_a, pair_cam_b, pair_offset, num_pairs, xy_a, xy_b, subsets, 4, tasks_per_pair, chunk_pairs, 4))) return rc;
  DeviceBuffers& B = G.B;
  ParallaxArgs X{};
  RSBA_HIP_TRY(B.upload(&X.E, E, (size_t)num_pairs * 9));
  RSBA_HIP_TRY(B.upload(&X.poses, poses, (size_t)num_pairs * 6));
  RSBA_HIP_TRY(B.upload(&X.pair_status, pair_status, (size_t)num_pairs));
  if ((rc = alloc_pair_loop(G, false))) return rc;

  // scratch of the largest chunk: the hypotheses of its tasks, the refit of its pairs
  const size_t T = (size_t)chunk_pairs * tasks_per_pair;
  HomoDltArgs A{}, RA{};
  HomoScoreArgs S{}, RS{};
  A.na = S.na = RA.na = RS.na = G.na;
  A.nb = S.nb = RA.nb = RS.nb = G.nb;
  A.n = RA.n = (int)G.points;
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

  for (int32_t p0 = 0; p0 < num_pairs; p0 += chunk_pairs) {
    const PairChunk C = pair_chunk(G, p0);
    S.pairs = RS.pairs = C.S.pairs;
    A.num_tasks = S.num_tasks = C.np * tasks_per_pair; A.subsets = G.subsets + (size_t)p0 * G.per_pair;
    RSBA_HIP_TRY(launch_homography_dlt(A, nullptr));
    RSBA_HIP_TRY(launch_homography_score(S, nullptr));
    WinnerArgs W{};
    W.tasks_per_pair = tasks_per_pair; W.status = S.status; W.num_inliers = S.num_inliers; W.models = A.H_out;
    RA.num_tasks = RS.num_tasks = C.np; RA.subsets = C.S.inlier_idx; RA.sub_start = G.starts + p0; RA.sub_count = C.S.inlier_count;
    AdoptArgs D{};
    D.status = RS.status; D.num_inliers = RS.num_inliers; D.models = RA.H_out;
    rc = run_pair_loop(G, C, W, D, PairRule::Transfer, 5, refits, S.thr2, [&]() -> int32_t {   // (a refit takes at least five inliers)
      RSBA_HIP_TRY(launch_homography_dlt(RA, nullptr));
      RSBA_HIP_TRY(launch_homography_score(RS, nullptr));
      return RSBA_OK;
    });
    if (rc) return rc;
  }
  // the parallax counts: one wave per pair over the given E and pose, all pairs in one launch (a pair's counts are its own)
  X.num_pairs = num_pairs; X.pairs = G.table; X.na = G.na; X.nb = G.nb; X.thr2 = S.thr2; X.cos_min = cos_min_parallax;
  RSBA_HIP_TRY(B.alloc(&X.num_front, (size_t)num_pairs));
  RSBA_HIP_TRY(B.alloc(&X.num_parallax, (size_t)num_pairs));
  RSBA_HIP_TRY(launch_two_view_parallax(X, nullptr));

  // ---- one download; H of a pair without a winner stays the caller's ----
  std::vector<int32_t> front((size_t)num_pairs), par((size_t)num_pairs);
  std::vector<uint8_t> st;
  RSBA_HIP_TRY(hipMemcpy(front.data(), X.num_front, front.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(par.data(), X.num_parallax, par.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if ((rc = download_pairs(G, h_status, h_winner_task, h_refits_adopted, num_h_inliers, h_inlier_mask, H_out, st))) return rc;
  for (size_t p = 0; p < (size_t)num_pairs; ++p) { num_front[p] = front[p]; num_parallax[p] = par[p]; }
  return RSBA_OK;
}
