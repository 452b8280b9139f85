// Arguments of the RS-PnP hypothesis kernels (kernels_pnp.hip); all pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rsba {

struct PnpArgs {
  double cam[9];                 // {fx,fy,k1,k2,p1,p2,k3,cx,cy}
  int shutter, scan0, scan1;
  int n, m, num_tasks, init_stride, max_num_iterations, drop_coincident;
  float reprojection_error;
  const float* object_points;    // [n][3]
  const float* image_points;     // [n][2]
  const int32_t* subsets;        // [num_tasks][m]
  const double* init_poses;      // [num_tasks][12] (init_stride 12) or [12] shared (init_stride 0)
  double* poses_out;             // [num_tasks][12]
  uint8_t* status;               // [num_tasks] 0 skipped, 1 solved and usable, 2 solve failed (initial poses kept)
  double* final_cost;            // [num_tasks]
  int32_t* num_inliers;          // [num_tasks]
};

// Arguments of the DLT start-pose kernels (kernels_pnp_dlt.hip)
struct PnpDltArgs {
  double cam[9];
  int n, m, num_tasks;
  const float* object_points;    // [n][3]
  const float* image_points;     // [n][2]
  const int32_t* subsets;        // [num_tasks][m]
  double* normalised;            // [n][2] undistorted, normalised image points: written by the normalise kernel, read by the DLT kernel
  double* poses_out;             // [num_tasks][6]; declined slots are not written
  uint8_t* status;               // [num_tasks] 0 declined, 1 general DLT, 2 planar branch
};

// Arguments of the minimal-solver kernel (kernels_pnp_p3p.hip)
struct PnpP3pArgs {
  int n, num_tasks;
  const float* object_points;    // [n][3]
  const double* normalised;      // [n][2], from the normalise kernel
  const int32_t* subsets;        // [num_tasks][4]: three solved points, the fourth chooses among the solutions
  double* poses_out;             // [num_tasks][6]; declined slots are not written
  uint8_t* status;               // [num_tasks] 0 declined, 1 solved
  int32_t* num_solutions;        // [num_tasks] admissible solutions, 0..4
};

hipError_t launch_pnp_normalise(const PnpDltArgs& args, hipStream_t st);
hipError_t launch_pnp_p3p(const PnpP3pArgs& args, hipStream_t st);
hipError_t launch_pnp_dlt(const PnpDltArgs& args, hipStream_t st);
// subsets_out[j] = subsets[map[j]], init_out[j] = (dlt_poses[map[j]], dlt_poses[map[j]]) for j < count
hipError_t launch_pnp_compact(const int32_t* map, int count, int m, const int32_t* subsets, const double* dlt_poses, int32_t* subsets_out,
                              double* init_out, hipStream_t st);
hipError_t launch_pnp_tasks(const PnpArgs& args, hipStream_t st);
hipError_t launch_pnp_inliers(const PnpArgs& args, const double* poses, uint8_t* mask, hipStream_t st);

}  // namespace rsba
