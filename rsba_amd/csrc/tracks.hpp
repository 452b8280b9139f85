// Arguments of the track-creation kernels (kernels_tracks.hip), staged by tracks_capi.hip.  Every index has been checked on
// the host before the launch: obs_frame in [0, F), frame_cam in [0, num_cams), cand_a / cand_b in [0, num_obs), and every
// frame an observation belongs to has at least one pose.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rsba_amd.h"

namespace rsba {

struct TrackGeometryArgs {
  const double* cams;          // [num_cams][9]
  const int32_t* frame_cam;    // [F]
  const double* poses;         // [pose_offset[F]][6]
  const int64_t* pose_offset;  // [F + 1]
  const int32_t* obs_frame;    // [num_obs]
  const double2* obs_xy;       // [num_obs]
  const int32_t* cand_a;       // [num_cand] observation o
  const int32_t* cand_b;       // [num_cand] observation o2 (read only for RSBA_TRACK_TRIANGULATE)
  const uint8_t* request;      // [num_cand] RSBA_TRACK_* bits
  const double* track_pt;      // [num_cand][3] (read only for RSBA_TRACK_REPROJECT)
  int64_t num_obs, num_cand;
  int shutter, scan0, scan1, interp_rotation;
  double sq_threshold, min_distance;
};

hipError_t launch_track_rays(const TrackGeometryArgs& a, double* ray, uint8_t* ray_ok, hipStream_t st);
hipError_t launch_track_candidates(const TrackGeometryArgs& a, const double* ray, const uint8_t* ray_ok, uint8_t* tri_ok, double* tri_pt,
                                   uint8_t* reproj_ok, hipStream_t st);

}  // namespace rsba
