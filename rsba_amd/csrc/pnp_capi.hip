// C-ABI of the RS-PnP hypothesis path (include/rsba_amd.h: rsba_pnp_tasks, rsba_pnp_inliers, rsba_pnp_dlt, rsba_pnp_gs_hypotheses, rsba_pnp_p3p,
// rsba_pnp_gs_hypotheses_p3p).  Host-side glue only: staging of the caller's arrays and the launches; every number comes from kernels_pnp.hip /
// kernels_pnp_dlt.hip / kernels_pnp_p3p.hip.
#include "../../include/rsba_amd.h"

#include <string>
#include <vector>

#include "capi_util.hpp"
#include "pnp_state.hpp"

using namespace rsba;

namespace {

int32_t fill_camera(PnpArgs& A, const double* cam, int32_t shutter, const int32_t* scanlines, float reprojection_error) {
  if (!cam || !scanlines) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (shutter < 0 || shutter > 2) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "shutter must be 0 (GLOBAL), 1 (HORIZONTAL) or 2 (VERTICAL)");
  if (shutter != 0 && scanlines[0] == scanlines[1]) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "scanlines[0] == scanlines[1]");
  for (int k = 0; k < 9; ++k) A.cam[k] = cam[k];
  A.shutter = shutter; A.scan0 = scanlines[0]; A.scan1 = scanlines[1];
  A.reprojection_error = reprojection_error;
  return RSBA_OK;
}

}  // namespace

extern "C" int32_t rsba_pnp_tasks(int32_t device, const double* cam, int32_t shutter, const int32_t* scanlines, const float* object_points,
                                  const float* image_points, int32_t n, const int32_t* subsets, int32_t m, int32_t num_tasks,
                                  const double* init_poses, int32_t init_stride, int32_t max_num_iterations, int32_t drop_coincident, float reprojection_error,
                                  double* poses_out, uint8_t* status, double* final_cost, int32_t* num_inliers) {
  if (!object_points || !image_points || !subsets || !init_poses || !poses_out || !status)
    return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (n <= 0 || m <= 0 || num_tasks <= 0 || max_num_iterations < 0 || (init_stride != 0 && init_stride != 12))
    return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (init_stride is 0 or 12)");
  for (size_t k = 0; k < (size_t)num_tasks * m; ++k)
    if (subsets[k] < 0 || subsets[k] >= n) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "subset index out of range");
  PnpArgs A{};
  int32_t rc = fill_camera(A, cam, shutter, scanlines, reprojection_error);
  if (rc) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  A.n = n; A.m = m; A.num_tasks = num_tasks; A.init_stride = init_stride; A.max_num_iterations = max_num_iterations; A.drop_coincident = drop_coincident;
  DeviceBuffers B;
  RSBA_HIP_TRY(B.upload(&A.object_points, object_points, (size_t)n * 3));
  RSBA_HIP_TRY(B.upload(&A.image_points, image_points, (size_t)n * 2));
  RSBA_HIP_TRY(B.upload(&A.subsets, subsets, (size_t)num_tasks * m));
  RSBA_HIP_TRY(B.upload(&A.init_poses, init_poses, init_stride ? (size_t)num_tasks * 12 : 12));
  RSBA_HIP_TRY(B.alloc(&A.poses_out, (size_t)num_tasks * 12));
  RSBA_HIP_TRY(B.alloc(&A.status, (size_t)num_tasks));
  RSBA_HIP_TRY(B.alloc(&A.final_cost, (size_t)num_tasks));
  RSBA_HIP_TRY(B.alloc(&A.num_inliers, (size_t)num_tasks));
  RSBA_HIP_TRY(hipMemset(A.poses_out, 0, (size_t)num_tasks * 12 * sizeof(double)));
  RSBA_HIP_TRY(hipMemset(A.final_cost, 0, (size_t)num_tasks * sizeof(double)));
  RSBA_HIP_TRY(hipMemset(A.num_inliers, 0, (size_t)num_tasks * sizeof(int32_t)));
  RSBA_HIP_TRY(launch_pnp_tasks(A, nullptr));
  RSBA_HIP_TRY(hipMemcpy(poses_out, A.poses_out, (size_t)num_tasks * 12 * sizeof(double), hipMemcpyDeviceToHost));
  RSBA_HIP_TRY(hipMemcpy(status, A.status, (size_t)num_tasks, hipMemcpyDeviceToHost));
  if (final_cost) RSBA_HIP_TRY(hipMemcpy(final_cost, A.final_cost, (size_t)num_tasks * sizeof(double), hipMemcpyDeviceToHost));
  if (num_inliers) RSBA_HIP_TRY(hipMemcpy(num_inliers, A.num_inliers, (size_t)num_tasks * sizeof(int32_t), hipMemcpyDeviceToHost));
  return RSBA_OK;
}

extern "C" int32_t rsba_pnp_inliers(int32_t device, const double* cam, int32_t shutter, const int32_t* scanlines, const float* object_points,
                                    const float* image_points, int32_t n, const double* poses, float reprojection_error, uint8_t* inlier_mask) {
  if (!object_points || !image_points || !poses || !inlier_mask) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (n <= 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes");
  PnpArgs A{};
  int32_t rc = fill_camera(A, cam, shutter, scanlines, reprojection_error);
  if (rc) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  A.n = n;
  DeviceBuffers B;
  const double* d_poses = nullptr; uint8_t* d_mask = nullptr;
  RSBA_HIP_TRY(B.upload(&A.object_points, object_points, (size_t)n * 3));
  RSBA_HIP_TRY(B.upload(&A.image_points, image_points, (size_t)n * 2));
  RSBA_HIP_TRY(B.upload(&d_poses, poses, 12));
  RSBA_HIP_TRY(B.alloc(&d_mask, (size_t)n));
  RSBA_HIP_TRY(launch_pnp_inliers(A, d_poses, d_mask, nullptr));
  RSBA_HIP_TRY(hipMemcpy(inlier_mask, d_mask, (size_t)n, hipMemcpyDeviceToHost));
  return RSBA_OK;
}

namespace {

// the argument checks rsba_pnp_dlt and rsba_pnp_gs_hypotheses share (the codes rsba_pnp_tasks returns for the same mistakes)
int32_t check_dlt_arguments(const double* cam, const float* object_points, const float* image_points, int32_t n, const int32_t* subsets, int32_t m,
                            int32_t num_tasks, const double* poses_out, const uint8_t* status) {
  if (!cam || !object_points || !image_points || !subsets || !poses_out || !status) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (n <= 0 || m < 6 || n < m || num_tasks <= 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (a DLT subset has at least 6 points, n >= m)");
  for (size_t k = 0; k < (size_t)num_tasks * m; ++k)
    if (subsets[k] < 0 || subsets[k] >= n) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "subset index out of range");
  return RSBA_OK;
}

// upload, normalise, DLT: D.poses_out / D.status stay on the device
int32_t run_dlt(DeviceBuffers& B, PnpDltArgs& D, const double* cam, const float* object_points, const float* image_points, int32_t n,
                const int32_t* subsets, int32_t m, int32_t num_tasks) {
  for (int k = 0; k < 9; ++k) D.cam[k] = cam[k];
  D.n = n; D.m = m; D.num_tasks = num_tasks;
  RSBA_HIP_TRY(B.upload(&D.object_points, object_points, (size_t)n * 3));
  RSBA_HIP_TRY(B.upload(&D.image_points, image_points, (size_t)n * 2));
  RSBA_HIP_TRY(B.upload(&D.subsets, subsets, (size_t)num_tasks * m));
  RSBA_HIP_TRY(B.alloc(&D.normalised, (size_t)n * 2));
  RSBA_HIP_TRY(B.alloc(&D.poses_out, (size_t)num_tasks * 6));
  RSBA_HIP_TRY(B.alloc(&D.status, (size_t)num_tasks));
  RSBA_HIP_TRY(hipMemset(D.poses_out, 0, (size_t)num_tasks * 6 * sizeof(double)));
  RSBA_HIP_TRY(launch_pnp_normalise(D, nullptr));
  RSBA_HIP_TRY(launch_pnp_dlt(D, nullptr));
  return RSBA_OK;
}

// What rsba_pnp_gs_hypotheses and rsba_pnp_gs_hypotheses_p3p do after their start-pose kernel: the accepted subsets packed, refined from
// their start poses (both pose slots the same) and scored by pnp_tasks_kernel with shutter GLOBAL, the results scattered back to the
// caller's task order.  d_*, start_poses [num_tasks][6] and start_status [num_tasks] are device arrays.
int32_t refine_and_scatter(DeviceBuffers& B, const double* cam, const float* d_object_points, const float* d_image_points, int32_t n, const int32_t* d_subsets_in,
                           int32_t m, int32_t num_tasks, const double* start_poses, const uint8_t* start_status, int32_t max_num_iterations,
                           float reprojection_error, double* poses_out, uint8_t* status, double* final_cost, int32_t* num_inliers) {
  // which subsets were accepted: one byte per subset comes back; the poses stay where they are
  std::vector<uint8_t> accepted((size_t)num_tasks);
  RSBA_HIP_TRY(hipMemcpy(accepted.data(), start_status, accepted.size(), hipMemcpyDeviceToHost));
  std::vector<int32_t> map;
  for (int32_t t = 0; t < num_tasks; ++t) if (accepted[(size_t)t]) map.push_back(t);
  const int32_t count = (int32_t)map.size();
  std::vector<double> poses((size_t)count * 12), cost((size_t)count);
  std::vector<uint8_t> st((size_t)count);
  std::vector<int32_t> inl((size_t)count);
  if (count > 0) {
    PnpArgs A{};
    const int32_t scanlines[2] = {0, 1};
    const int32_t rc = fill_camera(A, cam, 0 /* GLOBAL */, scanlines, reprojection_error);
    if (rc) return rc;
    A.n = n; A.m = m; A.num_tasks = count; A.init_stride = 12; A.max_num_iterations = max_num_iterations; A.drop_coincident = 0;
    A.object_points = d_object_points; A.image_points = d_image_points;
    const int32_t* d_map = nullptr; int32_t* d_subsets = nullptr; double* d_init = nullptr;
    RSBA_HIP_TRY(B.upload(&d_map, map.data(), (size_t)count));
    RSBA_HIP_TRY(B.alloc(&d_subsets, (size_t)count * m));
    RSBA_HIP_TRY(B.alloc(&d_init, (size_t)count * 12));
    RSBA_HIP_TRY(launch_pnp_compact(d_map, count, m, d_subsets_in, start_poses, d_subsets, d_init, nullptr));
    A.subsets = d_subsets; A.init_poses = d_init;
    RSBA_HIP_TRY(B.alloc(&A.poses_out, (size_t)count * 12));
    RSBA_HIP_TRY(B.alloc(&A.status, (size_t)count));
    RSBA_HIP_TRY(B.alloc(&A.final_cost, (size_t)count));
    RSBA_HIP_TRY(B.alloc(&A.num_inliers, (size_t)count));
    RSBA_HIP_TRY(hipMemset(A.poses_out, 0, (size_t)count * 12 * sizeof(double)));
    RSBA_HIP_TRY(hipMemset(A.final_cost, 0, (size_t)count * sizeof(double)));
    RSBA_HIP_TRY(hipMemset(A.num_inliers, 0, (size_t)count * sizeof(int32_t)));
    RSBA_HIP_TRY(launch_pnp_tasks(A, nullptr));
    RSBA_HIP_TRY(hipMemcpy(poses.data(), A.poses_out, poses.size() * sizeof(double), hipMemcpyDeviceToHost));
    RSBA_HIP_TRY(hipMemcpy(st.data(), A.status, st.size(), hipMemcpyDeviceToHost));
    RSBA_HIP_TRY(hipMemcpy(cost.data(), A.final_cost, cost.size() * sizeof(double), hipMemcpyDeviceToHost));
    RSBA_HIP_TRY(hipMemcpy(inl.data(), A.num_inliers, inl.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  for (int32_t t = 0; t < num_tasks; ++t) {
    status[t] = 0;
    if (final_cost) final_cost[t] = 0.0;
    if (num_inliers) num_inliers[t] = 0;
  }
  for (int32_t j = 0; j < count; ++j) {
    const size_t t = (size_t)map[(size_t)j];
    for (int k = 0; k < 6; ++k) poses_out[t * 6 + k] = poses[(size_t)j * 12 + k];
    status[t] = st[(size_t)j];
    if (final_cost) final_cost[t] = cost[(size_t)j];
    if (num_inliers) num_inliers[t] = inl[(size_t)j];
  }
  return RSBA_OK;
}

}  // namespace

extern "C" int32_t rsba_pnp_dlt(int32_t device, const double* cam, const float* object_points, const float* image_points, int32_t n,
                                const int32_t* subsets, int32_t m, int32_t num_tasks, double* poses_out, uint8_t* status) {
  int32_t rc = check_dlt_arguments(cam, object_points, image_points, n, subsets, m, num_tasks, poses_out, status);
  if (rc) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  PnpDltArgs D{};
  if ((rc = run_dlt(B, D, cam, object_points, image_points, n, subsets, m, num_tasks))) return rc;
  std::vector<uint8_t> st;
  return download_accepted(D.status, D.poses_out, 6, num_tasks, status, poses_out, st);
}

extern "C" int32_t rsba_pnp_gs_hypotheses(int32_t device, const double* cam, const float* object_points, const float* image_points, int32_t n,
                                          const int32_t* subsets, int32_t m, int32_t num_tasks, int32_t max_num_iterations, float reprojection_error,
                                          double* poses_out, uint8_t* status, double* final_cost, int32_t* num_inliers) {
  int32_t rc = check_dlt_arguments(cam, object_points, image_points, n, subsets, m, num_tasks, poses_out, status);
  if (rc) return rc;
  if (max_num_iterations < 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (max_num_iterations < 0)");
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  PnpDltArgs D{};
  if ((rc = run_dlt(B, D, cam, object_points, image_points, n, subsets, m, num_tasks))) return rc;
  return refine_and_scatter(B, cam, D.object_points, D.image_points, n, D.subsets, m, num_tasks, D.poses_out, D.status, max_num_iterations, reprojection_error,
                            poses_out, status, final_cost, num_inliers);
}

namespace {

// the argument checks rsba_pnp_p3p and rsba_pnp_gs_hypotheses_p3p share (the codes the DLT calls return for the same mistakes)
int32_t check_p3p_arguments(const double* cam, const float* object_points, const float* image_points, int32_t n, const int32_t* subsets, int32_t num_tasks,
                            const double* poses_out, const uint8_t* status) {
  if (!cam || !object_points || !image_points || !subsets || !poses_out || !status) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 4 || num_tasks <= 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (a P3P subset has four points, n >= 4)");
  for (size_t k = 0; k < (size_t)num_tasks * 4; ++k)
    if (subsets[k] < 0 || subsets[k] >= n) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "subset index out of range");
  return RSBA_OK;
}

// upload, normalise, P3P: P.poses_out / P.status / P.num_solutions stay on the device (D carries the uploaded points and subsets)
int32_t run_p3p(DeviceBuffers& B, PnpDltArgs& D, PnpP3pArgs& P, const double* cam, const float* object_points, const float* image_points, int32_t n,
                const int32_t* subsets, int32_t num_tasks) {
  for (int k = 0; k < 9; ++k) D.cam[k] = cam[k];
  D.n = n; D.m = 4; D.num_tasks = num_tasks;
  RSBA_HIP_TRY(B.upload(&D.object_points, object_points, (size_t)n * 3));
  RSBA_HIP_TRY(B.upload(&D.image_points, image_points, (size_t)n * 2));
  RSBA_HIP_TRY(B.upload(&D.subsets, subsets, (size_t)num_tasks * 4));
  RSBA_HIP_TRY(B.alloc(&D.normalised, (size_t)n * 2));
  P.n = n; P.num_tasks = num_tasks; P.object_points = D.object_points; P.normalised = D.normalised; P.subsets = D.subsets;
  RSBA_HIP_TRY(B.alloc(&P.poses_out, (size_t)num_tasks * 6));
  RSBA_HIP_TRY(B.alloc(&P.status, (size_t)num_tasks));
  RSBA_HIP_TRY(B.alloc(&P.num_solutions, (size_t)num_tasks));
  RSBA_HIP_TRY(hipMemset(P.poses_out, 0, (size_t)num_tasks * 6 * sizeof(double)));
  RSBA_HIP_TRY(launch_pnp_normalise(D, nullptr));
  RSBA_HIP_TRY(launch_pnp_p3p(P, nullptr));
  return RSBA_OK;
}

}  // namespace

extern "C" int32_t rsba_pnp_p3p(int32_t device, const double* cam, const float* object_points, const float* image_points, int32_t n,
                                const int32_t* subsets, int32_t num_tasks, double* poses_out, uint8_t* status, int32_t* num_solutions) {
  int32_t rc = check_p3p_arguments(cam, object_points, image_points, n, subsets, num_tasks, poses_out, status);
  if (rc) return rc;
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  PnpDltArgs D{};
  PnpP3pArgs P{};
  if ((rc = run_p3p(B, D, P, cam, object_points, image_points, n, subsets, num_tasks))) return rc;
  if (num_solutions) RSBA_HIP_TRY(hipMemcpy(num_solutions, P.num_solutions, (size_t)num_tasks * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<uint8_t> st;
  return download_accepted(P.status, P.poses_out, 6, num_tasks, status, poses_out, st);
}

// rsba_pnp_gs_hypotheses with the minimal solver in the DLT's place: the same steps after the start-pose kernel, for m = 4
extern "C" int32_t rsba_pnp_gs_hypotheses_p3p(int32_t device, const double* cam, const float* object_points, const float* image_points, int32_t n,
                                              const int32_t* subsets, int32_t num_tasks, int32_t max_num_iterations, float reprojection_error,
                                              double* poses_out, uint8_t* status, double* final_cost, int32_t* num_inliers) {
  int32_t rc = check_p3p_arguments(cam, object_points, image_points, n, subsets, num_tasks, poses_out, status);
  if (rc) return rc;
  if (max_num_iterations < 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad sizes (max_num_iterations < 0)");
  if ((rc = rsba_select_device(device))) return rc;
  DeviceBuffers B;
  PnpDltArgs D{};
  PnpP3pArgs P{};
  if ((rc = run_p3p(B, D, P, cam, object_points, image_points, n, subsets, num_tasks))) return rc;
  return refine_and_scatter(B, cam, D.object_points, D.image_points, n, D.subsets, 4, num_tasks, P.poses_out, P.status, max_num_iterations, reprojection_error,
                            poses_out, status, final_cost, num_inliers);
}
