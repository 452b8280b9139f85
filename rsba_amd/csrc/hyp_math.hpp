// The small algebra the hypothesis kernels share (kernels_pnp_dlt.hip, kernels_pnp_p3p.hip, kernels_epipolar.hip, kernels_homography.hip): the device restatement of
// include/rsba/hyp_host.hpp's hyp_detail::rotate, pose_from_rt, eigen3 and smallest_eigenvector12, which solve_rs_pnp.hpp and two_view.hpp call
// alike.  The host functions are the definition; fp64 throughout, every loop with the host's fixed bound (40 / 60 Jacobi sweeps).  No anonymous
// namespace: a tool that includes two kernel files into one translation unit sees one definition.
#pragma once
#include <hip/hip_runtime.h>

namespace rsba {

// entry (a, b) of a symmetric matrix kept as its lower triangle, row by row
__device__ __forceinline__ int sym(int a, int b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }

// ceres::AngleAxisRotatePoint, as hyp_detail::rotate
__device__ __forceinline__ void rotate(const double w[3], const double p[3], double out[3]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double wxp[3] = {w[1] * p[2] - w[2] * p[1], w[2] * p[0] - w[0] * p[2], w[0] * p[1] - w[1] * p[0]};
  if (th2 > 2.220446049250313e-16) {
    const double th = sqrt(th2), c = cos(th), s = sin(th), it = 1.0 / th;
    const double k[3] = {w[0] * it, w[1] * it, w[2] * it};
    const double kxp[3] = {wxp[0] * it, wxp[1] * it, wxp[2] * it};
    const double kp = (k[0] * p[0] + k[1] * p[1] + k[2] * p[2]) * (1.0 - c);
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = p[i] * c + kxp[i] * s + k[i] * kp;
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = p[i] + wxp[i];
  }
}

// hyp_detail::pose_from_rt: x_cam = R X + tvec as the pose (rvec, -R(rvec)^T tvec); false where one of the six numbers is not finite
__device__ __forceinline__ bool pose_from_rt(const double R[9], const double tvec[3], double pose[6]) {
  double rvec[3];
  const double tr = R[0] + R[4] + R[8], csn = fmin(1.0, fmax(-1.0, 0.5 * (tr - 1.0))), th = acos(csn);
  const double ax[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double sn = 0.5 * sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  if (sn > 1e-8) {
#pragma unroll
    for (int k = 0; k < 3; ++k) rvec[k] = ax[k] * (th / (2.0 * sn));
  } else if (csn > 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) rvec[k] = 0.5 * ax[k];
  } else {   // a half turn: the axis from the diagonal
    const double d[3] = {sqrt(fmax(0.0, 0.5 * (R[0] + 1.0))), sqrt(fmax(0.0, 0.5 * (R[4] + 1.0))), sqrt(fmax(0.0, 0.5 * (R[8] + 1.0)))};
    rvec[0] = th * d[0]; rvec[1] = th * d[1] * (R[1] + R[3] >= 0 ? 1.0 : -1.0); rvec[2] = th * d[2] * (R[2] + R[6] >= 0 ? 1.0 : -1.0);
  }
  const double rinv[3] = {-rvec[0], -rvec[1], -rvec[2]}, nt[3] = {-tvec[0], -tvec[1], -tvec[2]};
  double centre[3];
  rotate(rinv, nt, centre);
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) { pose[k] = rvec[k]; pose[3 + k] = centre[k]; finite = finite && isfinite(rvec[k]) && isfinite(centre[k]); }
  return finite;
}

// hyp_detail::eigen3 in registers (every index is a compile-time constant after unrolling): values ascending, v[r][k] = component r of the
// unit eigenvector of val[k]
__device__ __forceinline__ void eigen3(const double s[6], double val[3], double v[3][3]) {
  double a[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[r][k] = r == k ? 1.0 : 0.0;
  }
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
  auto cswap = [&](int i, int j) {
    if (d[j] < d[i]) {
      const double td = d[i]; d[i] = d[j]; d[j] = td;
#pragma unroll
      for (int r = 0; r < 3; ++r) { const double tv = v[r][i]; v[r][i] = v[r][j]; v[r][j] = tv; }
    }
  };
  cswap(0, 1); cswap(0, 2); cswap(1, 2);
#pragma unroll
  for (int r = 0; r < 3; ++r) val[r] = d[r];
}

// hyp_detail::smallest_eigenvector12 on N unknowns, one lane per matrix: cyclic Jacobi on the lower triangle G (N (N + 1) / 2 entries) with the
// accumulated rotations V (N x N), both in LDS and lane-interleaved (entry e of this lane at [e * BLOCK]: conflict-free, and indexable by the
// run-time (p, q) of a rotation, which registers are not).  The rotation is applied in its symmetric form (rows and columns at once on the
// triangle, the pivot set to zero) — the same rotation angles as the host's column-then-row update, a different operation order.  `largest` starts
// from the eigenvalue of unknowns the caller left out of G (0.0 where there are none).  -1 where the gap test declines: an ambiguous null
// space; otherwise the column c of V that holds the unit eigenvector of the smallest eigenvalue (component k at V[(k * N + c) * BLOCK]; the
// caller reads it: handing the components back through an array changed the last bits of the DLT kernel's planar poses).
template <int N, int BLOCK>
__device__ __forceinline__ int smallest_eigenvector_lds(double* G, double* V, double largest) {
  for (int e = 0; e < N * N; ++e) V[e * BLOCK] = 0.0;
  for (int k = 0; k < N; ++k) V[(k * N + k) * BLOCK] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0;
    for (int i = 1; i < N; ++i) for (int j = 0; j < i; ++j) { const double g = G[(i * (i + 1) / 2 + j) * BLOCK]; off += g * g; }
    if (off < 1e-30) break;
#pragma unroll 1
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll 1
      for (int q = p + 1; q < N; ++q) {
        const int ipq = q * (q + 1) / 2 + p, ipp = p * (p + 1) / 2 + p, iqq = q * (q + 1) / 2 + q;
        const double apq = G[ipq * BLOCK];
        if (fabs(apq) < 1e-300) continue;
        const double app = G[ipp * BLOCK], aqq = G[iqq * BLOCK];
        const double theta = (aqq - app) / (2.0 * apq);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)), cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
        for (int k = 0; k < N; ++k) {
          if (k == p || k == q) continue;
          const int ikp = sym(k, p), ikq = sym(k, q);
          const double akp = G[ikp * BLOCK], akq = G[ikq * BLOCK];
          G[ikp * BLOCK] = cs * akp - sn * akq; G[ikq * BLOCK] = sn * akp + cs * akq;
        }
        G[ipp * BLOCK] = app - tt * apq; G[iqq * BLOCK] = aqq + tt * apq; G[ipq * BLOCK] = 0.0;
        for (int k = 0; k < N; ++k) {
          const double vkp = V[(k * N + p) * BLOCK], vkq = V[(k * N + q) * BLOCK];
          V[(k * N + p) * BLOCK] = cs * vkp - sn * vkq; V[(k * N + q) * BLOCK] = sn * vkp + cs * vkq;
        }
      }
    }
  }
  int best = 0;
  double dbest = G[0];
  for (int i = 1; i < N; ++i) { const double di = G[sym(i, i) * BLOCK]; if (di < dbest) { dbest = di; best = i; } }
  double second = 0.0;
  bool have_second = false;
  for (int i = 0; i < N; ++i) {
    const double di = G[sym(i, i) * BLOCK];
    if (i != best && (!have_second || di < second)) { second = di; have_second = true; }
    largest = fmax(largest, di);
  }
  if (!(second > 1e-9 * largest) || !(dbest < 0.05 * second)) return -1;
  return best;
}

}  // namespace rsba
