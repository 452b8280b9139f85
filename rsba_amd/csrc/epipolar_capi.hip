// C-ABI of the two-view bootstrap (include/rsba_amd.h: rsba_epipolar_eight_point, rsba_epipolar_score, rsba_epipolar_hypotheses,
// rsba_epipolar_inliers, rsba_epipolar_five_point, rsba_epipolar_hypotheses_five_point).  Host-side glue only: argument checks (the codes
// rsba_pnp_dlt returns for the same mistakes), staging of the caller's arrays and the launches; every number comes from kernels_epipolar.hip,
// kernels_five_point.hip and pnp_normalise_kernel (kernels_pnp_dlt.hip).
#include "../../include/rsba_amd.h"

#include <string>
#include <vector>

#include "capi_util.hpp"
#include "epipolar_state.hpp"
#include "pnp_state.hpp"

using namespace rsba;

namespace {

int32_t check_points(const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n) {
  if (!cam_a || !cam_b || !xy_a || !xy_b) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 8) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (an essential matrix takes at least 8 correspondences)");
  return RSBA_OK;
}
int32_t check_subsets(int32_t n, const int32_t* subsets, int32_t m, int32_t num_tasks) {
  if (!subsets) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (m < 8 || n < m || num_tasks <= 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (an eight-point subset has at least 8 correspondences, n >= m)");
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
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n);
  if (rc) return rc;
  if (!E_out || !status) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets(n, subsets, m, num_tasks))) return rc;
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
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n);
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
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n);
  if (rc) return rc;
  if (!E_out || !poses_out || !status || !num_inliers || !num_front) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = check_subsets(n, subsets, m, num_tasks))) return rc;
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
  int32_t rc = check_points(cam_a, cam_b, xy_a, xy_b, n);
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

int32_t check_points_five(const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n) {
  if (!cam_a || !cam_b || !xy_a || !xy_b) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 5) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (the five-point solver takes at least 5 correspondences)");
  return RSBA_OK;
}
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
  int32_t rc = check_points_five(cam_a, cam_b, xy_a, xy_b, n);
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
  int32_t rc = check_points_five(cam_a, cam_b, xy_a, xy_b, n);
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
