// Start poses of the global-shutter RANSAC hypotheses (include/rsba/hyp_host.hpp: hyp_detail::normalised_point; solve_rs_pnp.hpp: pnp_detail::dlt_pose and
// what dlt_pose calls — planar_pose and hyp_detail::eigen3, smallest_eigenvector12, nearest_rotation, pose_from_rt), for every subset at once.
// The host functions are the definition; this file restates them for the device, fp64 throughout, every loop with the host's
// fixed bound (60 / 40 Jacobi sweeps, 30 nearest-rotation steps, 20 undistortion steps).
//   pnp_normalise_kernel  one lane per image point, once per call
//   pnp_dlt_kernel        one lane per subset, one wave per workgroup.  The 12 x 12 Gram matrix (lower triangle, 78 entries) and the
//                         144 entries of the accumulated rotations live in LDS, lane-interleaved as pnp_tasks_kernel keeps its normal
//                         matrix (entry e of lane l at [e][l]: conflict-free, and indexable by the run-time (p, q) of a Jacobi rotation,
//                         which registers are not).  222 x 64 doubles = 113 664 bytes per workgroup: above 64 KB, asked for explicitly.
//                         The Jacobi rotation is applied in its symmetric form (rows and columns at once on the triangle, the pivot
//                         set to zero) — the same rotation angles as the host's column-then-row update, a different operation order.
//   pnp_compact_kernel    gathers the accepted subsets and their poses (both pose slots the same) for pnp_tasks_kernel
// A lane's result depends on its own subset only: no cross-lane operation, no atomics, no dependence on the launch geometry.
#include "hyp_math.hpp"
#include "pnp_state.hpp"

namespace rsba {

namespace {

constexpr int kDltBlock = 64;                 // one wave per workgroup
constexpr int kTri = 78;                      // lower triangle of 12 x 12
constexpr int kVec = 144;                     // the eigenvector matrix

__global__ __launch_bounds__(256) void pnp_normalise_kernel(const PnpDltArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const double* cam = A.cam;
  const double pn0 = ((double)A.image_points[2 * (size_t)i] - cam[7]) / cam[0], pn1 = ((double)A.image_points[2 * (size_t)i + 1] - cam[8]) / cam[1];
  double pu0 = pn0, pu1 = pn1;
  for (int it = 0; it < 20; ++it) {
    const double x = pu0, y = pu1, r2 = x * x + y * y, d = 1.0 + r2 * (cam[2] + r2 * (cam[3] + r2 * cam[6])), xy = x * y;
    const double dx = d * x + 2.0 * cam[4] * xy + cam[5] * (r2 + 2.0 * x * x), dy = d * y + cam[4] * (r2 + 2.0 * y * y) + 2.0 * cam[5] * xy;
    pu0 -= dx - pn0; pu1 -= dy - pn1;
  }
  A.normalised[2 * (size_t)i] = pu0; A.normalised[2 * (size_t)i + 1] = pu1;
}

__device__ __forceinline__ double det3(const double R[9]) {
  return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

__global__ __launch_bounds__(kDltBlock) void pnp_dlt_kernel(const PnpDltArgs A) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x, t = blockIdx.x * kDltBlock + lane;
  if (t >= A.num_tasks) return;                  // (no barrier anywhere below)
  double* G = smem + lane;                       // G[e * 64]: Gram matrix, lower triangle
  double* V = smem + kTri * kDltBlock + lane;    // V[(k * 12 + col) * 64]
  const int32_t* sub = A.subsets + (size_t)t * A.m;
  const int m = A.m;
  const float* op = A.object_points;
  const double* nrm2 = A.normalised;
  A.status[t] = 0;

  // ---- centroid, scale, scatter (dlt_pose) ----
  double c[3] = {0, 0, 0}, scale = 0.0;
  for (int i = 0; i < m; ++i) {
    const size_t j = 3 * (size_t)sub[i];
    c[0] += op[j] / m; c[1] += op[j + 1] / m; c[2] += op[j + 2] / m;   // float quotients, as on the host (float / int)
  }
  for (int i = 0; i < m; ++i) {
    const size_t j = 3 * (size_t)sub[i];
    const double d0 = (double)op[j] - c[0], d1 = (double)op[j + 1] - c[1], d2 = (double)op[j + 2] - c[2];
    scale += sqrt(d0 * d0 + d1 * d1 + d2 * d2) / m;
  }
  if (!(scale > 0.0)) return;
  double sc[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < m; ++i) {
    const size_t j = 3 * (size_t)sub[i];
    const double d0 = ((double)op[j] - c[0]) / scale, d1 = ((double)op[j + 1] - c[1]) / scale, d2 = ((double)op[j + 2] - c[2]) / scale;
    sc[0] += d0 * d0; sc[1] += d0 * d1; sc[2] += d0 * d2; sc[3] += d1 * d1; sc[4] += d1 * d2; sc[5] += d2 * d2;
  }
  // ---- eigen3: cyclic Jacobi in registers (every index below is a compile-time constant after unrolling).  The text of hyp_math.hpp's eigen3,
  // kept in line: a call in its place changes how the compiler contracts the planar branch's sums of products below (the last bits of
  // its poses), whichever way the function hands its results back ----
  double val[3], e1[3], e2[3];                   // planar branch: e1 / e2 = eigenvectors of the largest / middle eigenvalue
  {
    double a[3][3] = {{sc[0], sc[1], sc[2]}, {sc[1], sc[3], sc[4]}, {sc[2], sc[4], sc[5]}}, v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 40; ++sweep) {
      const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
      if (off < 1e-300) break;
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int q = p + 1; q < 3; ++q) {
          if (fabs(a[p][q]) < 1e-300) continue;
          const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
          const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)), cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
          for (int k = 0; k < 3; ++k) { const double akp = a[k][p], akq = a[k][q]; a[k][p] = cs * akp - sn * akq; a[k][q] = sn * akp + cs * akq; }
#pragma unroll
          for (int k = 0; k < 3; ++k) { const double apk = a[p][k], aqk = a[q][k]; a[p][k] = cs * apk - sn * aqk; a[q][k] = sn * apk + cs * aqk; }
#pragma unroll
          for (int k = 0; k < 3; ++k) { const double vkp = v[k][p], vkq = v[k][q]; v[k][p] = cs * vkp - sn * vkq; v[k][q] = sn * vkp + cs * vkq; }
        }
      }
    }
    // ascending order, the host's three compare-and-swap steps on (value, eigenvector column)
    double d[3] = {a[0][0], a[1][1], a[2][2]};
#define RSBA_DLT_CSWAP(i, j)                                                                      \
    if (d[j] < d[i]) {                                                                            \
      const double td = d[i]; d[i] = d[j]; d[j] = td;                                             \
      _Pragma("unroll") for (int r = 0; r < 3; ++r) { const double tv = v[r][i]; v[r][i] = v[r][j]; v[r][j] = tv; } \
    }
    RSBA_DLT_CSWAP(0, 1) RSBA_DLT_CSWAP(0, 2) RSBA_DLT_CSWAP(1, 2)
#undef RSBA_DLT_CSWAP
#pragma unroll
    for (int r = 0; r < 3; ++r) { val[r] = d[r]; e1[r] = v[r][2]; e2[r] = v[r][1]; }
  }
  if (!(val[1] > 1e-4 * val[2])) return;         // collinear: declined
  const bool planar = val[0] < 1e-3 * val[1];
  const double nv[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};

  // planar branch: Hartley normalisation of the image points (planar_pose)
  double cu = 0.0, cv = 0.0, su = 1.0;
  if (planar) {
    for (int i = 0; i < m; ++i) { const size_t j = 2 * (size_t)sub[i]; cu += nrm2[j] / m; cv += nrm2[j + 1] / m; }
    su = 0.0;
    for (int i = 0; i < m; ++i) { const size_t j = 2 * (size_t)sub[i]; su += hypot(nrm2[j] - cu, nrm2[j + 1] - cv) / m; }
    if (!(su > 0.0)) return;
    su /= 1.4142135623730951;
  }

  // ---- the Gram matrix of the two rows each point contributes (12 unknowns; the homography uses the first 9) ----
  for (int e = 0; e < kTri; ++e) G[e * kDltBlock] = 0.0;
  for (int i = 0; i < m; ++i) {
    const size_t j = 3 * (size_t)sub[i], j2 = 2 * (size_t)sub[i];
    const double d0 = ((double)op[j] - c[0]) / scale, d1 = ((double)op[j + 1] - c[1]) / scale, d2 = ((double)op[j + 2] - c[2]) / scale;
    double r0[12], r1[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { r0[k] = 0.0; r1[k] = 0.0; }
    if (planar) {
      const double x = d0 * e1[0] + d1 * e1[1] + d2 * e1[2], y = d0 * e2[0] + d1 * e2[1] + d2 * e2[2];
      const double u = (nrm2[j2] - cu) / su, v = (nrm2[j2 + 1] - cv) / su;
      r0[0] = x; r0[1] = y; r0[2] = 1.0; r0[6] = -u * x; r0[7] = -u * y; r0[8] = -u;
      r1[3] = x; r1[4] = y; r1[5] = 1.0; r1[6] = -v * x; r1[7] = -v * y; r1[8] = -v;
    } else {
      const double X[4] = {d0, d1, d2, 1.0};
      const double u = nrm2[j2], v = nrm2[j2 + 1];
#pragma unroll
      for (int k = 0; k < 4; ++k) { r0[k] = X[k]; r0[8 + k] = -u * X[k]; r1[4 + k] = X[k]; r1[8 + k] = -v * X[k]; }
    }
#pragma unroll
    for (int a = 0; a < 12; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) G[(a * (a + 1) / 2 + b) * kDltBlock] += r0[a] * r0[b] + r1[a] * r1[b];
    }
  }
  if (planar) {   // three idle unknowns far from the null space
    double big = 0.0;
    for (int a = 0; a < 9; ++a) big += G[sym(a, a) * kDltBlock];
    if (!(big > 0.0)) return;
    for (int a = 9; a < 12; ++a) G[sym(a, a) * kDltBlock] = 2.0 * big;
  }

  // ---- smallest_eigenvector12: cyclic Jacobi on the triangle in LDS ----
  const int best = smallest_eigenvector_lds<12, kDltBlock>(G, V, 0.0);
  if (best < 0) return;                          // an ambiguous null space is not an initialisation
  double pv[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) pv[k] = V[(k * 12 + best) * kDltBlock];

  // ---- [R | t] up to scale -> the nearest rotation -> world coordinates ----
  double Q[9], tp[3];
  if (planar) {
    double H[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) { H[k] = su * pv[k] + cu * pv[6 + k]; H[3 + k] = su * pv[3 + k] + cv * pv[6 + k]; H[6 + k] = pv[6 + k]; }
    if (H[8] < 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) H[k] = -H[k];
    }
    const double n1 = sqrt(H[0] * H[0] + H[3] * H[3] + H[6] * H[6]), n2 = sqrt(H[1] * H[1] + H[4] * H[4] + H[7] * H[7]);
    if (!(n1 > 1e-300) || !(n2 > 1e-300) || !isfinite(n1 + n2)) return;
    const double r1[3] = {H[0] / n1, H[3] / n1, H[6] / n1}, r2[3] = {H[1] / n2, H[4] / n2, H[7] / n2};
    const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    const double lam = 0.5 * (n1 + n2);
    tp[0] = scale * (H[2] / lam); tp[1] = scale * (H[5] / lam); tp[2] = scale * (H[8] / lam);
#pragma unroll
    for (int r = 0; r < 3; ++r) { Q[3 * r] = r1[r]; Q[3 * r + 1] = r2[r]; Q[3 * r + 2] = r3[r]; }
  } else {
    double M[9], tv[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) M[3 * r + k] = pv[4 * r + k];
      tv[r] = pv[4 * r + 3];
    }
    if (tv[2] < 0) {   // the centroid in front of the camera
#pragma unroll
      for (int k = 0; k < 9; ++k) M[k] = -M[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) tv[k] = -tv[k];
    }
    double lambda = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) lambda += sqrt(M[3 * r] * M[3 * r] + M[3 * r + 1] * M[3 * r + 1] + M[3 * r + 2] * M[3 * r + 2]) / 3.0;
    if (!(lambda > 1e-300) || !isfinite(lambda)) return;
#pragma unroll
    for (int k = 0; k < 9; ++k) Q[k] = M[k] / lambda;
#pragma unroll
    for (int k = 0; k < 3; ++k) tp[k] = scale * tv[k] / lambda;
  }
  // nearest_rotation: R <- (R + R^-T) / 2, 30 steps
  for (int it = 0; it < 30; ++it) {
    const double det = det3(Q);
    if (!(fabs(det) > 1e-12)) return;
    const double iT[9] = {(Q[4] * Q[8] - Q[5] * Q[7]) / det, (Q[5] * Q[6] - Q[3] * Q[8]) / det, (Q[3] * Q[7] - Q[4] * Q[6]) / det,
                          (Q[2] * Q[7] - Q[1] * Q[8]) / det, (Q[0] * Q[8] - Q[2] * Q[6]) / det, (Q[1] * Q[6] - Q[0] * Q[7]) / det,
                          (Q[1] * Q[5] - Q[2] * Q[4]) / det, (Q[2] * Q[3] - Q[0] * Q[5]) / det, (Q[0] * Q[4] - Q[1] * Q[3]) / det};
#pragma unroll
    for (int k = 0; k < 9; ++k) Q[k] = 0.5 * (Q[k] + iT[k]);
  }
  if (!(det3(Q) > 0)) return;
  double R[9];
  if (planar) {   // x_cam ~ Q [e1 e2 n]^T (X - c) / scale + tp
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) R[3 * r + k] = Q[3 * r] * e1[k] + Q[3 * r + 1] * e2[k] + Q[3 * r + 2] * nv[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Q[k];
  }
  double tvec[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) tvec[r] = tp[r] - (R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]);

  double pose[6];
  if (!pose_from_rt(R, tvec, pose)) return;
#pragma unroll
  for (int k = 0; k < 6; ++k) A.poses_out[(size_t)t * 6 + k] = pose[k];
  A.status[t] = planar ? 2 : 1;
}

// the accepted subsets, packed: task j of pnp_tasks_kernel is subset map[j]; both of its pose slots start from the DLT pose
__global__ __launch_bounds__(256) void pnp_compact_kernel(const int32_t* __restrict__ map, int count, int m, const int32_t* __restrict__ subsets,
                                                          const double* __restrict__ dlt_poses, int32_t* __restrict__ subsets_out, double* __restrict__ init_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= count) return;
  const size_t src = (size_t)map[j];
  for (int i = 0; i < m; ++i) subsets_out[(size_t)j * m + i] = subsets[src * m + i];
#pragma unroll
  for (int k = 0; k < 6; ++k) { const double v = dlt_poses[src * 6 + k]; init_out[(size_t)j * 12 + k] = v; init_out[(size_t)j * 12 + 6 + k] = v; }
}

}  // namespace

hipError_t launch_pnp_normalise(const PnpDltArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(pnp_normalise_kernel, dim3((A.n + 255) / 256), dim3(256), 0, st, A);
  return hipGetLastError();
}
hipError_t launch_pnp_dlt(const PnpDltArgs& A, hipStream_t st) {
  const size_t lds = (size_t)(kTri + kVec) * kDltBlock * sizeof(double);   // 113 664 bytes
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pnp_dlt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pnp_dlt_kernel, dim3((A.num_tasks + kDltBlock - 1) / kDltBlock), dim3(kDltBlock), lds, st, A);
  return hipGetLastError();
}
hipError_t launch_pnp_compact(const int32_t* map, int count, int m, const int32_t* subsets, const double* dlt_poses, int32_t* subsets_out,
                              double* init_out, hipStream_t st) {
  hipLaunchKernelGGL(pnp_compact_kernel, dim3((count + 255) / 256), dim3(256), 0, st, map, count, m, subsets, dlt_poses, subsets_out, init_out);
  return hipGetLastError();
}

}  // namespace rsba
