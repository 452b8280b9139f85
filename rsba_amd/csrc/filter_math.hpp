// Device helpers shared by the filter kernels (kernels_filter.hip) and the track-creation kernels (kernels_tracks.hip):
//   vision::sfm::getPose (copying overload)   rsba/src/rsba/struct/VideoSfM.cc:103-133
//   w2i(..., validate = true)                 rsba/src/rsba/mat/cam.h:400-419
#pragma once
#include "obs_math.hpp"

namespace rsba {

// interpolate_rs with the true observation (mat/cam.h:315-349): pose at the observation's scan line
// P == 0: a frame with MORE than two poses — one per scan line ("fullDoF"): the pose whose index is the rounded, clamped scan
// line of the observation (struct/VideoSfM.cc:118-132: x for HORIZONTAL, y otherwise — a GLOBAL session included; std::round,
// halves away from zero); np = f.poses.size()
template <int P>
__device__ __forceinline__ void pose_at(const Model& m, const double* __restrict__ poses, double ox, double oy, double out[6], int np = P) {
  if (P == 0) {
    double line = (m.shutter == kHorizontal) ? ox : oy;
    if (line < 0.0) line = 0.0; else if (line > double(np - 1)) line = double(np - 1);
    const double* q = poses + 6 * (size_t)round(line);
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = q[k];
    return;
  }
  if (P == 1 || m.shutter == kGlobal) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = poses[k];
    return;
  }
  const double coord = (m.shutter == kVertical) ? oy : ox;            // cam.h:325-331
  double tau = (coord - double(m.scan0)) / double(m.scan1 - m.scan0);
  if (tau < 0.0) tau = 0.0;
  if (tau > 1.0) tau = 1.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) out[k] = (k < 3 && !m.interp_rotation) ? poses[k] : poses[k] + (poses[6 + k] - poses[k]) * tau;
}

// w2i(cam, pose, X, proj, validate = true) (mat/cam.h:400-419) through the shared single-pose evaluation
__device__ __forceinline__ bool project(const double* cam, const double pose[6], const double X[3], double proj[2]) {
  const Model gs = {kGlobal, 0, 1, 1};
  ObsOut<true, 1> o;
  eval_observation<true, 1, false>(gs, cam, pose, X, 0.0, 0.0, o);     // residual against (0,0) = the projection
  proj[0] = o.r[0]; proj[1] = o.r[1];
  return o.ok;
}

}  // namespace rsba
