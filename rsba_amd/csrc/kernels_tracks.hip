// Geometry of track creation (VideoSfMHandler::createTracks / reprojectMatches, rsba/src/rsba/VideoSfMHandler.cc:231-372):
//   vision::sfm::getPose (copying overload)   rsba/src/rsba/struct/VideoSfM.cc:103-133
//   direction (pixel) / undistort / c2direction   rsba/src/rsba/mat/cam.h:77-112, 130-138, 154-176
//   triangulate (two rays)                    rsba/src/rsba/mat/cam.h:188-243
//   vision::validate                          rsba/src/rsba/mat/cam.h:424-457
// Two passes, fp64.  The ray pass runs one lane per distinct observation: getPose at the observation's own (x, y), the
// fixed-point undistortion (up to 200 steps, the only loop whose trip count varies from lane to lane) and the rotation into
// the world frame.  An observation takes part in several candidates, so undistorting once per observation instead of once
// per candidate removes the work that dominates.  The candidate pass runs one lane per (observation, match) pair: both
// poses again (cheap), their bitwise comparison, the 3x3 solve, both camera distances and both reprojection checks; and,
// when asked, the reprojection check of the observation against a given track point (vision::sfm::validate).
#include "device_state.hpp"
#include "filter_math.hpp"
#include "obs_math.hpp"
#include "tracks.hpp"

namespace rsba {

namespace {

// getPose for an observation of frame f: one pose, two (rolling-shutter interpolation) or one per scan line
__device__ __forceinline__ void obs_pose(const TrackGeometryArgs& a, int f, double ox, double oy, double pose[6]) {
  const int64_t p0 = a.pose_offset[f];
  const int np = (int)(a.pose_offset[f + 1] - p0);
  const Model m = {a.shutter, a.scan0, a.scan1, a.interp_rotation};
  const double* ps = a.poses + 6 * p0;
  if (np == 1) pose_at<1>(m, ps, ox, oy, pose);
  else if (np == 2) pose_at<2>(m, ps, ox, oy, pose);
  else pose_at<0>(m, ps, ox, oy, pose, np);
}

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }   // mat/core.h:164-167

// vision::validate (mat/cam.h:444-457): w2i with validation, squared pixel error below the threshold
__device__ __forceinline__ bool validate(const double* cam, const double pose[6], double ox, double oy, const double X[3], double sq_threshold) {
  double proj[2];
  if (!project(cam, pose, X, proj)) return false;
  const double ex = proj[0] - ox, ey = proj[1] - oy;
  return (ex * ex + ey * ey) < sq_threshold;
}

// mat/core.h:20-33 det33 (row-major)
__device__ __forceinline__ double det33(const double m[9]) {
  return m[0] * (m[4] * m[8] - m[7] * m[5]) - m[1] * (m[3] * m[8] - m[6] * m[5]) + m[2] * (m[3] * m[7] - m[6] * m[4]);
}

// triangulate(center1, d1, center2, d2, p) (mat/cam.h:188-231): A = (I - a a^T) + (I - b b^T), x = A^-1 ((I - a a^T) c1 + (I - b b^T) c2).
// The reference aborts when det(A) < eps; here that is a failure.
__device__ __forceinline__ bool triangulate(const double c1[3], const double a[3], const double c2[3], const double b[3], double p[3]) {
  double A[9], Pa[9], Pb[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double I = (i == j) ? 1.0 : 0.0;
      Pa[3 * i + j] = I - a[i] * a[j];
      Pb[3 * i + j] = I - b[i] * b[j];
      A[3 * i + j] = Pa[3 * i + j] + Pb[3 * i + j];
    }
  const double d = det33(A);
  if (d < kDblEps) return false;
  double y[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    y[i] = Pa[3 * i] * c1[0] + Pa[3 * i + 1] * c1[1] + Pa[3 * i + 2] * c1[2] + Pb[3 * i] * c2[0] + Pb[3 * i + 1] * c2[1] + Pb[3 * i + 2] * c2[2];
  // the inverse by cofactors (A is symmetric)
  const double Ai[9] = {(A[4] * A[8] - A[7] * A[5]) / d, (A[2] * A[7] - A[1] * A[8]) / d, (A[1] * A[5] - A[2] * A[4]) / d,
                        (A[5] * A[6] - A[3] * A[8]) / d, (A[0] * A[8] - A[2] * A[6]) / d, (A[3] * A[2] - A[0] * A[5]) / d,
                        (A[3] * A[7] - A[6] * A[4]) / d, (A[6] * A[1] - A[0] * A[7]) / d, (A[0] * A[4] - A[3] * A[1]) / d};
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = Ai[3 * i] * y[0] + Ai[3 * i + 1] * y[1] + Ai[3 * i + 2] * y[2];
  return true;
}

__global__ __launch_bounds__(256) void ray_kernel(const TrackGeometryArgs a, double* __restrict__ ray, uint8_t* __restrict__ ray_ok) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.num_obs) return;
  const int f = a.obs_frame[i];
  const double2 xy = a.obs_xy[i];
  const double* cam = a.cams + 9 * (size_t)a.frame_cam[f];
  double pose[6];
  obs_pose(a, f, xy.x, xy.y, pose);
  const double fx = cam[0], fy = cam[1], k1 = cam[2], k2 = cam[3], p1 = cam[4], p2 = cam[5], k3 = cam[6];
  bool ok = !(fx < kDblEps) && !(fy < kDblEps);                         // cam.h:160-161
  // cam.h:163-165: centred, normalised pixel
  const double nx = (xy.x - cam[7]) / fx, ny = (xy.y - cam[8]) / fy;
  // undistort (cam.h:77-112): p_u -= distort(p_u) - p_n; stop when the error exceeds |p_n| (diverging, invalid) or falls below
  // |p_n| * 0.001 / fx (valid); at most 200 steps
  const double nrm = sqrt(nx * nx + ny * ny);
  const double tol = nrm * 0.001 / fx;
  double ux = nx, uy = ny;
  bool converged = false;
  for (int it = 0; ok && it < 200; ++it) {
    const double r2 = ux * ux + uy * uy;
    const double dd = 1.0 + r2 * (k1 + r2 * (k2 + (r2 * k3)));
    const double xy2 = ux * uy;
    const double dx = (dd * ux) + (2.0 * p1 * xy2 + p2 * (r2 + 2.0 * ux * ux)) - nx;   // cam.h:65-71
    const double dy = (dd * uy) + (p1 * (r2 + 2.0 * uy * uy) + 2.0 * p2 * xy2) - ny;
    const double dist = sqrt(dx * dx + dy * dy);
    if (dist > nrm) break;
    ux -= dx; uy -= dy;
    if (dist < tol) { converged = true; break; }
  }
  ok = ok && converged;                                                  // cam.h:168-170 (validate = true)
  // c2direction (cam.h:130-138): rotate by the inverse rotation into the world frame, normalise
  const double w[3] = {-pose[0], -pose[1], -pose[2]}, q[3] = {ux, uy, 1.0};
  double d[3], R[3][3], D[3][3];
  rotate_with_derivative<false>(w, q, d, R, D);
  const double n = norm3(d[0], d[1], d[2]);
  ok = ok && !(n < kDblEps);                                             // normalize3, mat/core.h:170-177
  const double inv = 1.0 / n;
  ray[3 * i] = ok ? d[0] * inv : 0.0;
  ray[3 * i + 1] = ok ? d[1] * inv : 0.0;
  ray[3 * i + 2] = ok ? d[2] * inv : 0.0;
  ray_ok[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void candidate_kernel(const TrackGeometryArgs a, const double* __restrict__ ray, const uint8_t* __restrict__ ray_ok,
                                                        uint8_t* __restrict__ tri_ok, double* __restrict__ tri_pt, uint8_t* __restrict__ reproj_ok) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.num_cand) return;
  const int rq = a.request[c];
  const int ia = a.cand_a[c];
  const int fa = a.obs_frame[ia];
  const double2 xa = a.obs_xy[ia];
  const double* cama = a.cams + 9 * (size_t)a.frame_cam[fa];
  double pa[6];
  obs_pose(a, fa, xa.x, xa.y, pa);
  // reprojectMatches (VideoSfMHandler.cc:250-262) with the distance taken at getPose(o): = vision::sfm::validate (VideoSfM.cc:159-169)
  bool rep = false;
  if (rq & RSBA_TRACK_REPROJECT) {
    const double X[3] = {a.track_pt[3 * c], a.track_pt[3 * c + 1], a.track_pt[3 * c + 2]};
    rep = !(norm3(pa[3] - X[0], pa[4] - X[1], pa[5] - X[2]) < a.min_distance) && validate(cama, pa, xa.x, xa.y, X, a.sq_threshold);
  }
  reproj_ok[c] = rep ? 1 : 0;
  // the creation branch (VideoSfMHandler.cc:310-345)
  bool tri = false, solved = false;
  double pt[3] = {0.0, 0.0, 0.0};
  if (rq & RSBA_TRACK_TRIANGULATE) {
    const int ib = a.cand_b[c];
    const int fb = a.obs_frame[ib];
    const double2 xb = a.obs_xy[ib];
    const double* camb = a.cams + 9 * (size_t)a.frame_cam[fb];
    double pb[6];
    obs_pose(a, fb, xb.x, xb.y, pb);
    bool same = true;                                                    // memcmp(pose, pose2) == 0 (:321): bitwise, +0.0 != -0.0
#pragma unroll
    for (int k = 0; k < 6; ++k) same = same && (__double_as_longlong(pa[k]) == __double_as_longlong(pb[k]));
    if (!same && ray_ok[ia] && ray_ok[ib]) {
      const double da[3] = {ray[3 * (size_t)ia], ray[3 * (size_t)ia + 1], ray[3 * (size_t)ia + 2]};
      const double db[3] = {ray[3 * (size_t)ib], ray[3 * (size_t)ib + 1], ray[3 * (size_t)ib + 2]};
      solved = triangulate(pa + 3, da, pb + 3, db, pt);
      tri = solved && !(norm3(pa[3] - pt[0], pa[4] - pt[1], pa[5] - pt[2]) < a.min_distance)   // :326-333
                   && !(norm3(pb[3] - pt[0], pb[4] - pt[1], pb[5] - pt[2]) < a.min_distance)
                   && validate(cama, pa, xa.x, xa.y, pt, a.sq_threshold)                     // :335-337
                   && validate(camb, pb, xb.x, xb.y, pt, a.sq_threshold);
    }
  }
  tri_ok[c] = tri ? 1 : 0;
  tri_pt[3 * c] = solved ? pt[0] : 0.0;
  tri_pt[3 * c + 1] = solved ? pt[1] : 0.0;
  tri_pt[3 * c + 2] = solved ? pt[2] : 0.0;
}

}  // namespace

hipError_t launch_track_rays(const TrackGeometryArgs& a, double* ray, uint8_t* ray_ok, hipStream_t st) {
  if (a.num_obs <= 0) return hipSuccess;
  hipLaunchKernelGGL(ray_kernel, dim3((unsigned)((a.num_obs + 255) / 256)), dim3(256), 0, st, a, ray, ray_ok);
  return hipGetLastError();
}

hipError_t launch_track_candidates(const TrackGeometryArgs& a, const double* ray, const uint8_t* ray_ok, uint8_t* tri_ok, double* tri_pt,
                                   uint8_t* reproj_ok, hipStream_t st) {
  if (a.num_cand <= 0) return hipSuccess;
  hipLaunchKernelGGL(candidate_kernel, dim3((unsigned)((a.num_cand + 255) / 256)), dim3(256), 0, st, a, ray, ray_ok, tri_ok, tri_pt, reproj_ok);
  return hipGetLastError();
}

}  // namespace rsba
