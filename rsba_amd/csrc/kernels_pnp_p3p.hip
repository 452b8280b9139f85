// The minimal solver of the global-shutter RANSAC hypotheses (include/rsba_amd.h: rsba_pnp_p3p; include/rsba/solve_rs_pnp.hpp:
// pnp_detail::p3p_pose and what it calls — p3p_bearing, p3p_setup, p3p_roots, p3p_depths, p3p_polish, p3p_rt, p3p_fourth, hyp_detail::pose_from_rt),
// for every four-point subset at once.  The host functions are the definition; this file restates them for the device, fp64 throughout,
// every loop with the host's fixed bound (40 bisection steps per interval, two Newton steps per root, two per depth triple).
//   pnp_p3p_kernel   one lane per subset, one wave per workgroup.  Everything lives in registers: every array below is indexed by
//                    constants once the small loops are unrolled (the polynomials' degrees are template arguments, the four intervals
//                    and the up to four roots are walked by unrolled loops), so there is no LDS table and no scratch.
// The image points come from pnp_normalise_kernel (kernels_pnp_dlt.hip), the accepted subsets go on through pnp_compact_kernel.
// A lane's result depends on its own subset only: no cross-lane operation, no atomics, no dependence on the launch geometry.
#include "hyp_math.hpp"
#include "pnp_state.hpp"

namespace rsba {

namespace {

constexpr int kP3pBlock = 64;   // one wave per workgroup

struct P3pProblem {
  double P[3][3], j[3][3];
  double a2, b2, c2, ca, cb, cg, b;
  double N[3], D[2], c[5];
};

template <int DEG>
__device__ __forceinline__ double p3p_eval(const double (&c)[DEG + 1], double t) {
  double h = c[DEG];
#pragma unroll
  for (int k = DEG - 1; k >= 0; --k) h = h * t + c[k];
  return h;
}

// the root of a polynomial that is monotonic on [lo, hi], where it changes sign there; otherwise hi
template <int DEG>
__device__ __forceinline__ bool p3p_bisect(const double (&c)[DEG + 1], double lo, double hi, double& root) {
  root = hi;
  const bool plo = p3p_eval<DEG>(c, lo) > 0.0, phi = p3p_eval<DEG>(c, hi) > 0.0;
  if (plo == phi) return false;
#pragma unroll 1
  for (int it = 0; it < 40; ++it) {
    const double mid = 0.5 * (lo + hi);
    const bool same = (p3p_eval<DEG>(c, mid) > 0.0) == plo;
    lo = same ? mid : lo; hi = same ? hi : mid;
  }
  root = 0.5 * (lo + hi);
  return true;
}

__device__ __forceinline__ bool p3p_setup(P3pProblem& S) {
  const double (&P)[3][3] = S.P;
  const double (&j)[3][3] = S.j;
  const double d12[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, d13[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
  const double d23[3] = {P[2][0] - P[1][0], P[2][1] - P[1][1], P[2][2] - P[1][2]};
  const double a2 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2], b2 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
  const double c2 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
  if (!(a2 > 0.0) || !(b2 > 0.0) || !(c2 > 0.0)) return false;
  const double nx = d12[1] * d13[2] - d12[2] * d13[1], ny = d12[2] * d13[0] - d12[0] * d13[2], nz = d12[0] * d13[1] - d12[1] * d13[0];
  const double tr = (a2 + b2 + c2) / 3.0, prod = (nx * nx + ny * ny + nz * nz) / 3.0;
  const double big = 0.5 * (tr + sqrt(fmax(0.0, tr * tr - 4.0 * prod))), small = prod / big;
  if (!(small > 1e-8 * big)) return false;     // collinear: declined
  const double ca = j[1][0] * j[2][0] + j[1][1] * j[2][1] + j[1][2] * j[2][2], cb = j[0][0] * j[2][0] + j[0][1] * j[2][1] + j[0][2] * j[2][2];
  const double cg = j[0][0] * j[1][0] + j[0][1] * j[1][1] + j[0][2] * j[1][2];
  const double K = (a2 - c2) / b2, g = c2 / b2;
  S.a2 = a2; S.b2 = b2; S.c2 = c2; S.ca = ca; S.cb = cb; S.cg = cg; S.b = sqrt(b2);
  S.N[0] = K + 1.0; S.N[1] = -2.0 * K * cb; S.N[2] = K - 1.0;
  S.D[0] = cg; S.D[1] = -ca;
  const double n0 = S.N[0], n1 = S.N[1], n2 = S.N[2], d0 = S.D[0], d1 = S.D[1];
  const double nn[5] = {n0 * n0, 2.0 * n0 * n1, 2.0 * n0 * n2 + n1 * n1, 2.0 * n1 * n2, n2 * n2};
  const double nd[5] = {n0 * d0, n0 * d1 + n1 * d0, n1 * d1 + n2 * d0, n2 * d1, 0.0};
  const double dd[3] = {d0 * d0, 2.0 * d0 * d1, d1 * d1}, q[3] = {1.0 - g, 2.0 * g * cb, -g};
  const double e[5] = {dd[0] * q[0], dd[0] * q[1] + dd[1] * q[0], dd[0] * q[2] + dd[1] * q[1] + dd[2] * q[0], dd[1] * q[2] + dd[2] * q[1], dd[2] * q[2]};
  double A[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) A[k] = nn[k] - 4.0 * cg * nd[k] + 4.0 * e[k];
  // P(t) = sum_i A_i t^i (1 - t)^(4 - i)
  S.c[0] = A[0];
  S.c[1] = A[1] - 4.0 * A[0];
  S.c[2] = A[2] - 3.0 * A[1] + 6.0 * A[0];
  S.c[3] = A[3] - 2.0 * A[2] + 3.0 * A[1] - 4.0 * A[0];
  S.c[4] = A[4] - A[3] + A[2] - A[1] + A[0];
  return true;
}

__device__ __forceinline__ bool p3p_positive(const P3pProblem& S, const double s[3]) {
  const double least = 1e-9 * S.b;
  return s[0] > least && s[1] > least && s[2] > least && isfinite(s[0] + s[1] + s[2]);
}

__device__ __forceinline__ bool p3p_depths(const P3pProblem& S, double t, double s[3]) {
  const double r = 1.0 - t;
  const double w = sqrt(r * r + t * t - 2.0 * t * r * S.cb);
  const double Nh = S.N[2] * t * t + S.N[1] * t * r + S.N[0] * r * r, Dh = S.D[1] * t + S.D[0] * r;
  if (!(fabs(Dh) > 1e-12) || !(w > 0.0)) return false;
  s[0] = S.b * r / w; s[1] = S.b * Nh / (2.0 * Dh * w); s[2] = S.b * t / w;
  return p3p_positive(S, s);
}

// two Newton steps on the three cosine laws, in the depths
__device__ __forceinline__ bool p3p_polish(const P3pProblem& S, double s[3]) {
  bool live = true;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double F0 = s[1] * s[1] + s[2] * s[2] - 2.0 * s[1] * s[2] * S.ca - S.a2, F1 = s[0] * s[0] + s[2] * s[2] - 2.0 * s[0] * s[2] * S.cb - S.b2;
    const double F2 = s[0] * s[0] + s[1] * s[1] - 2.0 * s[0] * s[1] * S.cg - S.c2;
    const double p = s[1] - s[2] * S.ca, q = s[2] - s[1] * S.ca, r = s[0] - s[2] * S.cb, w = s[2] - s[0] * S.cb;
    const double x = s[0] - s[1] * S.cg, y = s[1] - s[0] * S.cg;
    const double det = 2.0 * (p * w * x + q * r * y);
    live = live && fabs(det) > 0.0;              // (the host leaves the loop at a singular Jacobian)
    if (live) {
      s[0] -= (-w * y * F0 + q * y * F1 + p * w * F2) / det;
      s[1] -= (w * x * F0 - q * x * F1 + q * r * F2) / det;
      s[2] -= (r * y * F0 + p * x * F1 - p * r * F2) / det;
    }
  }
  return p3p_positive(S, s);
}

__device__ __forceinline__ void p3p_triad(const double A[3], const double B[3], const double C[3], double e[3][3]) {
  const double u[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, v[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
  const double iu = 1.0 / sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) e[0][k] = u[k] * iu;
  const double n[3] = {e[0][1] * v[2] - e[0][2] * v[1], e[0][2] * v[0] - e[0][0] * v[2], e[0][0] * v[1] - e[0][1] * v[0]};
  const double in = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) e[2][k] = n[k] * in;
  e[1][0] = e[2][1] * e[0][2] - e[2][2] * e[0][1]; e[1][1] = e[2][2] * e[0][0] - e[2][0] * e[0][2]; e[1][2] = e[2][0] * e[0][1] - e[2][1] * e[0][0];
}

// x_cam = R X + tvec takes P_i onto s_i j_i (e: the world triangle's triad)
__device__ __forceinline__ void p3p_rt(const P3pProblem& S, const double e[3][3], const double pc[3], const double s[3], double R[9], double tvec[3]) {
  double Q[3][3], f[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) Q[i][k] = s[i] * S.j[i][k];
  }
  p3p_triad(Q[0], Q[1], Q[2], f);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) R[3 * r + k] = f[0][r] * e[0][k] + f[1][r] * e[1][k] + f[2][r] * e[2][k];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) tvec[r] = (Q[0][r] + Q[1][r] + Q[2][r]) / 3.0 - (R[3 * r] * pc[0] + R[3 * r + 1] * pc[1] + R[3 * r + 2] * pc[2]);
}

__global__ __launch_bounds__(kP3pBlock) void pnp_p3p_kernel(const PnpP3pArgs A) {
  const int t = blockIdx.x * kP3pBlock + threadIdx.x;
  if (t >= A.num_tasks) return;
  A.status[t] = 0;
  A.num_solutions[t] = 0;
  const int32_t i0 = A.subsets[(size_t)t * 4], i1 = A.subsets[(size_t)t * 4 + 1], i2 = A.subsets[(size_t)t * 4 + 2], i3 = A.subsets[(size_t)t * 4 + 3];
  if (i0 == i1 || i0 == i2 || i0 == i3 || i1 == i2 || i1 == i3 || i2 == i3) return;
  const int32_t idx[3] = {i0, i1, i2};
  P3pProblem S;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) S.P[i][k] = (double)A.object_points[3 * (size_t)idx[i] + k];
    const double x = A.normalised[2 * (size_t)idx[i]], y = A.normalised[2 * (size_t)idx[i] + 1];
    const double inv = 1.0 / sqrt(x * x + y * y + 1.0);
    S.j[i][0] = x * inv; S.j[i][1] = y * inv; S.j[i][2] = inv;
  }
  if (!p3p_setup(S)) return;
  const double X4[3] = {(double)A.object_points[3 * (size_t)i3], (double)A.object_points[3 * (size_t)i3 + 1], (double)A.object_points[3 * (size_t)i3 + 2]};
  const double x4 = A.normalised[2 * (size_t)i3], y4 = A.normalised[2 * (size_t)i3 + 1];

  // ---- p3p_roots: the intervals on which P is monotonic, from the roots of its derivatives ----
  const double c3[4] = {S.c[1], 2.0 * S.c[2], 3.0 * S.c[3], 4.0 * S.c[4]}, c2[3] = {S.c[2], 3.0 * S.c[3], 6.0 * S.c[4]}, c1[2] = {S.c[3], 4.0 * S.c[4]};
  double x1, x2a, x2b, x3a, x3b, x3c;
  p3p_bisect<1>(c1, 0.0, 1.0, x1);
  p3p_bisect<2>(c2, 0.0, x1, x2a); p3p_bisect<2>(c2, x1, 1.0, x2b);
  p3p_bisect<3>(c3, 0.0, x2a, x3a); p3p_bisect<3>(c3, x2a, x2b, x3b); p3p_bisect<3>(c3, x2b, 1.0, x3c);
  const double edge[5] = {0.0, x3a, x3b, x3c, 1.0};

  // the world triangle's triad and centroid, once for all solutions
  double e[3][3];
  p3p_triad(S.P[0], S.P[1], S.P[2], e);
  const double pc[3] = {(S.P[0][0] + S.P[1][0] + S.P[2][0]) / 3.0, (S.P[0][1] + S.P[1][1] + S.P[2][1]) / 3.0, (S.P[0][2] + S.P[1][2] + S.P[2][2]) / 3.0};

  double bestR[9], bestT[3], best = 0.0;
  int found = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double tr;
    if (!p3p_bisect<4>(S.c, edge[i], edge[i + 1], tr)) continue;
#pragma unroll
    for (int it = 0; it < 2; ++it) {   // Newton on P, a step taken only while it stays inside (0, 1)
      const double p = p3p_eval<4>(S.c, tr), dp = p3p_eval<3>(c3, tr), tn = tr - p / dp;
      if (tn > 0.0 && tn < 1.0) tr = tn;
    }
    double s[3], R[9], tvec[3];
    if (!p3p_depths(S, tr, s) || !p3p_polish(S, s)) continue;
    p3p_rt(S, e, pc, s, R, tvec);
    const double z = R[6] * X4[0] + R[7] * X4[1] + R[8] * X4[2] + tvec[2];
    if (!(z > 0.0)) continue;
    const double dx = (R[0] * X4[0] + R[1] * X4[1] + R[2] * X4[2] + tvec[0]) / z - x4, dy = (R[3] * X4[0] + R[4] * X4[1] + R[5] * X4[2] + tvec[1]) / z - y4;
    const double d2 = dx * dx + dy * dy;
    if (!isfinite(d2)) continue;
    if (found == 0 || d2 < best) {
      best = d2;
#pragma unroll
      for (int k = 0; k < 9; ++k) bestR[k] = R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) bestT[k] = tvec[k];
    }
    ++found;
  }
  if (found == 0) return;

  double pose[6];
  if (!pose_from_rt(bestR, bestT, pose)) return;
#pragma unroll
  for (int k = 0; k < 6; ++k) A.poses_out[(size_t)t * 6 + k] = pose[k];
  A.num_solutions[t] = found;
  A.status[t] = 1;
}

}  // namespace

hipError_t launch_pnp_p3p(const PnpP3pArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(pnp_p3p_kernel, dim3((A.num_tasks + kP3pBlock - 1) / kP3pBlock), dim3(kP3pBlock), 0, st, A);
  return hipGetLastError();
}

}  // namespace rsba
