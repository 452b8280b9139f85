// C-ABI of the stateless track-creation geometry (include/rsba_amd.h: rsba_track_candidates) — the predicates that
// VideoSfMHandler::createTracks / reprojectMatches (VideoSfMHandler.cc:231-372) evaluate per (observation, match) pair, for a
// whole batch of candidates at once.  No handle: each host thread keeps one growing device arena + pinned staging buffers +
// stream, so a call is one upload, one or two launches and one download.  Kernels: kernels_tracks.hip.
#include "../../include/rsba_amd.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "capi_util.hpp"
#include "tracks.hpp"

using namespace rsba;

namespace {

inline size_t up16(size_t b) { return (b + 15) & ~size_t(15); }

// per host thread and device: one input block (uploaded in one copy), one output block (downloaded in one copy) and the
// rays of the observations, which never leave the device
struct Arena {
  int device = -1;
  hipStream_t stream = nullptr;
  size_t in_cap = 0, out_cap = 0, ray_cap = 0;   // bytes
  char *d_in = nullptr, *d_out = nullptr, *d_ray = nullptr, *h_in = nullptr, *h_out = nullptr;
  void release() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_ray); (void)hipHostFree(h_in); (void)hipHostFree(h_out);
    d_in = d_out = d_ray = h_in = h_out = nullptr; in_cap = out_cap = ray_cap = 0;
  }
  // (thread_local, as the filter's arena: destroyed when its thread ends; errors of the frees are ignored)
  ~Arena() { release(); if (stream) (void)hipStreamDestroy(stream); }
  static size_t grow(size_t have, size_t need) { size_t c = std::max<size_t>(have, 1 << 16); while (c < need) c *= 2; return c; }
  int32_t reserve(int dev, size_t in_bytes, size_t out_bytes, size_t ray_bytes) {
    if (dev != device) { release(); if (stream) { (void)hipStreamDestroy(stream); stream = nullptr; } device = dev; }
    RSBA_HIP_TRY(hipSetDevice(dev));
    if (!stream) RSBA_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (in_bytes > in_cap) {
      (void)hipFree(d_in); (void)hipHostFree(h_in); d_in = h_in = nullptr; in_cap = 0;
      const size_t c = grow(in_cap, in_bytes);
      RSBA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_in), c));
      RSBA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_in), c));
      in_cap = c;
    }
    if (out_bytes > out_cap) {
      (void)hipFree(d_out); (void)hipHostFree(h_out); d_out = h_out = nullptr; out_cap = 0;
      const size_t c = grow(out_cap, out_bytes);
      RSBA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_out), c));
      RSBA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_out), c));
      out_cap = c;
    }
    if (ray_bytes > ray_cap) {
      (void)hipFree(d_ray); d_ray = nullptr; ray_cap = 0;
      const size_t c = grow(ray_cap, ray_bytes);
      RSBA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_ray), c));
      ray_cap = c;
    }
    return RSBA_OK;
  }
};
thread_local Arena g_arena;

// bump allocation of sections in one staging block (16-byte aligned: obs_xy is read as double2)
struct Layout {
  size_t size = 0;
  size_t add(size_t bytes) { const size_t at = size; size = up16(size + bytes); return at; }
};

}  // namespace

extern "C" int32_t rsba_track_candidates(int32_t device, const double* cams, int32_t num_cams, const int32_t* frame_cam, int32_t num_frames,
                                         const double* poses, const int64_t* pose_offset, int32_t shutter, const int32_t* scanlines,
                                         int32_t interpolate_rotation, const int32_t* obs_frame, const double* obs_xy, int64_t num_obs,
                                         const int32_t* cand_a, const int32_t* cand_b, const uint8_t* request, const double* track_pt,
                                         int64_t num_cand, double sq_threshold, double min_distance, uint8_t* tri_ok, double* tri_pt,
                                         uint8_t* reproj_ok) {
  if (num_cand <= 0) return RSBA_OK;
  if (num_cand > 0x7fffffff || num_obs > 0x7fffffff) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "too many candidates or observations for one call");
  if (!cams || !poses || !pose_offset || !scanlines || !obs_frame || !obs_xy || !cand_a || !request)
    return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (num_cams < 1 || num_frames < 1 || num_obs < 1) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "num_cams, num_frames and num_obs must be positive");
  if (num_cams > 1 && !frame_cam) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "frame_cam is needed with more than one camera");
  if (shutter < 0 || shutter > 2) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "shutter");
  // every index the kernels follow is checked here
  if (pose_offset[0] != 0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "pose_offset[0] != 0");
  for (int32_t f = 0; f < num_frames; ++f) {
    if (pose_offset[f + 1] < pose_offset[f]) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "pose_offset decreases");
    if (frame_cam && (frame_cam[f] < 0 || frame_cam[f] >= num_cams)) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "frame_cam out of range");
    if (shutter != RSBA_SHUTTER_GLOBAL && pose_offset[f + 1] - pose_offset[f] == 2 && scanlines[0] == scanlines[1])
      return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "scanlines[0] == scanlines[1]");
  }
  for (int64_t i = 0; i < num_obs; ++i) {
    const int32_t f = obs_frame[i];
    if (f < 0 || f >= num_frames) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "obs_frame out of range");
    if (pose_offset[f + 1] == pose_offset[f]) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "empty frame");   // getPose throws (struct/VideoSfM.cc:105)
  }
  bool any_tri = false, any_rep = false;
  for (int64_t c = 0; c < num_cand; ++c) {
    const uint8_t rq = request[c];
    if (rq & ~uint8_t(RSBA_TRACK_TRIANGULATE | RSBA_TRACK_REPROJECT)) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "request");
    if (cand_a[c] < 0 || cand_a[c] >= num_obs) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "cand_a out of range");
    if (rq & RSBA_TRACK_TRIANGULATE) {
      if (!cand_b) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
      if (cand_b[c] < 0 || cand_b[c] >= num_obs) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "cand_b out of range");
      any_tri = true;
    }
    any_rep = any_rep || (rq & RSBA_TRACK_REPROJECT);
  }
  if ((any_tri && (!tri_ok || !tri_pt)) || (any_rep && (!track_pt || !reproj_ok))) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  int32_t rc = rsba_check_device(device);
  if (rc) return rc;

  const size_t F = (size_t)num_frames, NP = (size_t)pose_offset[num_frames], M = (size_t)num_obs, N = (size_t)num_cand;
  Layout in;
  const size_t o_cams = in.add(9 * (size_t)num_cams * sizeof(double)), o_fcam = in.add(F * sizeof(int32_t)), o_poses = in.add(6 * NP * sizeof(double)),
               o_poff = in.add((F + 1) * sizeof(int64_t)), o_of = in.add(M * sizeof(int32_t)), o_xy = in.add(2 * M * sizeof(double)),
               o_ca = in.add(N * sizeof(int32_t)), o_cb = in.add(any_tri ? N * sizeof(int32_t) : 0), o_rq = in.add(N),
               o_tp = in.add(any_rep ? 3 * N * sizeof(double) : 0);
  Layout out;
  const size_t o_tri = out.add(N), o_tpt = out.add(3 * N * sizeof(double)), o_rep = out.add(N);
  Arena& A = g_arena;
  if ((rc = A.reserve(device, in.size, out.size, any_tri ? M * (3 * sizeof(double) + 1) + 8 : 8))) return rc;

  std::memcpy(A.h_in + o_cams, cams, 9 * (size_t)num_cams * sizeof(double));
  if (frame_cam) std::memcpy(A.h_in + o_fcam, frame_cam, F * sizeof(int32_t));
  else std::memset(A.h_in + o_fcam, 0, F * sizeof(int32_t));
  std::memcpy(A.h_in + o_poses, poses, 6 * NP * sizeof(double));
  std::memcpy(A.h_in + o_poff, pose_offset, (F + 1) * sizeof(int64_t));
  std::memcpy(A.h_in + o_of, obs_frame, M * sizeof(int32_t));
  std::memcpy(A.h_in + o_xy, obs_xy, 2 * M * sizeof(double));
  std::memcpy(A.h_in + o_ca, cand_a, N * sizeof(int32_t));
  if (any_tri) std::memcpy(A.h_in + o_cb, cand_b, N * sizeof(int32_t));
  std::memcpy(A.h_in + o_rq, request, N);
  if (any_rep) std::memcpy(A.h_in + o_tp, track_pt, 3 * N * sizeof(double));
  RSBA_HIP_TRY(hipMemcpyAsync(A.d_in, A.h_in, in.size, hipMemcpyHostToDevice, A.stream));

  TrackGeometryArgs a;
  a.cams = reinterpret_cast<const double*>(A.d_in + o_cams);
  a.frame_cam = reinterpret_cast<const int32_t*>(A.d_in + o_fcam);
  a.poses = reinterpret_cast<const double*>(A.d_in + o_poses);
  a.pose_offset = reinterpret_cast<const int64_t*>(A.d_in + o_poff);
  a.obs_frame = reinterpret_cast<const int32_t*>(A.d_in + o_of);
  a.obs_xy = reinterpret_cast<const double2*>(A.d_in + o_xy);
  a.cand_a = reinterpret_cast<const int32_t*>(A.d_in + o_ca);
  a.cand_b = any_tri ? reinterpret_cast<const int32_t*>(A.d_in + o_cb) : nullptr;
  a.request = reinterpret_cast<const uint8_t*>(A.d_in + o_rq);
  a.track_pt = any_rep ? reinterpret_cast<const double*>(A.d_in + o_tp) : nullptr;
  a.num_obs = num_obs; a.num_cand = num_cand;
  a.shutter = shutter; a.scan0 = scanlines[0]; a.scan1 = scanlines[1]; a.interp_rotation = interpolate_rotation != 0;
  a.sq_threshold = sq_threshold; a.min_distance = min_distance;
  double* d_ray = reinterpret_cast<double*>(A.d_ray);
  uint8_t* d_ray_ok = reinterpret_cast<uint8_t*>(A.d_ray + 3 * M * sizeof(double));
  if (any_tri) RSBA_HIP_TRY(launch_track_rays(a, d_ray, d_ray_ok, A.stream));
  RSBA_HIP_TRY(launch_track_candidates(a, d_ray, d_ray_ok, reinterpret_cast<uint8_t*>(A.d_out + o_tri), reinterpret_cast<double*>(A.d_out + o_tpt),
                                     reinterpret_cast<uint8_t*>(A.d_out + o_rep), A.stream));
  // one download: the triangulation outputs only when asked for
  const size_t down = any_tri ? out.size : N;
  if (any_tri) RSBA_HIP_TRY(hipMemcpyAsync(A.h_out, A.d_out, down, hipMemcpyDeviceToHost, A.stream));
  else RSBA_HIP_TRY(hipMemcpyAsync(A.h_out + o_rep, A.d_out + o_rep, N, hipMemcpyDeviceToHost, A.stream));
  RSBA_HIP_TRY(hipStreamSynchronize(A.stream));
  if (tri_ok) { if (any_tri) std::memcpy(tri_ok, A.h_out + o_tri, N); else std::memset(tri_ok, 0, N); }
  if (tri_pt) { if (any_tri) std::memcpy(tri_pt, A.h_out + o_tpt, 3 * N * sizeof(double)); else std::memset(tri_pt, 0, 3 * N * sizeof(double)); }
  if (reproj_ok) std::memcpy(reproj_ok, A.h_out + o_rep, N);
  return RSBA_OK;
}
