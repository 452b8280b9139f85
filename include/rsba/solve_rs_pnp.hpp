// Host-side mirror of rsba's rolling-shutter PnP entry points, over librsba_amd:
//   vision::solveRsPnP          /root/reference/src/rsba/solveRSpnp.cpp:100-192  (solveRSpnp.h:14-26)
//   vision::solveRsPnPRansac    /root/reference/src/rsba/solveRSpnp.cpp:413-524  (solveRSpnp.h:29-46)
// Same names, argument order and meaning, with plain arrays where the reference takes cv::Mat (OpenCV is not a
// dependency here): object points [n][3] float, image points [n][2] float, the 9 sfm intrinsics instead of
// cameraMatrix + distCoeffs (what sfmCam() makes of them), rvec / tvec / rvec2 / tvec2 as double[3] in OpenCV's
// convention (x_cam = R(rvec) X + tvec).  What the reference runs sequentially — one ceres::Solve per random subset
// (pnpTask, :265-335) — is ONE device launch here (rsba_pnp_tasks); the subsets come from the same generator
// (cv::RNG's multiply-with-carry, restated) walked in the same order, and the winner is chosen by replaying the
// reference's sequential rule (first strictly better hypothesis wins, stop once minInliersCount is reached) over the
// batch's inlier counts, so the result is the one the single-threaded reference would return for these subsets.
// The global-shutter initialisation the reference takes from OpenCV when all four vectors are zero (cv::solvePnP, :111-117;
// cv::solvePnPRansac, :437-449) is provided natively, in OpenCV's own shape (SOLVEPNP_ITERATIVE = a direct linear transform
// followed by a Levenberg-Marquardt refinement of the reprojection error): the DLT of the undistorted, normalised image points is
// glue on this side (a 12 x 12 symmetric eigenproblem); the refinement, and for the RANSAC form the refinement and inlier count of
// every sampled hypothesis, run on the device through the same rsba_pnp_tasks with shutter GLOBAL — one launch.  OpenCV's sampling
// order cannot be replayed without OpenCV, so this half is functionally, not bitwise, the reference's.
// Everything numeric that decides a result is computed by librsba_amd; a missing device throws std::runtime_error.
// pnp_detail holds what is about PnP; the glue and the algebra it shares with two_view.hpp and new_frame.hpp are hyp_host.hpp's hyp_detail,
// which pnp_detail takes in whole by one using-directive (no per-name aliases, no second definition).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "hyp_host.hpp"

namespace rsba_amd {

namespace pnp_detail {

using namespace hyp_detail;   // one definition each, in hyp_host.hpp; the solvers below call it unqualified, and a program written against pnp_detail still finds it

// ---- global-shutter initialisation (what cv::solvePnP(ITERATIVE) starts from): direct linear transform ----
// A PLANAR target (a wall, a checkerboard): the 12-unknown DLT has a two-dimensional null space there, and cv::solvePnP — what the
// reference calls, solveRSpnp.cpp:111-117 — starts from the plane's homography instead (its cvFindExtrinsicCameraParams2 takes that branch
// when the two smallest singular values of the centred points' scatter are in a ratio below 1e-3).  Here: the points in the plane's own
// frame (e1, e2, n = eigenvectors of the scatter, centred at c, divided by `scale`), the homography (x, y, 1) -> normalised image point
// from the 9-unknown DLT (image points Hartley-normalised), then [r1 r2 t] ~ H: r1, r2 the normalised first columns, r3 = r1 x r2,
// t = h3 over the mean of the two column norms, the nearest rotation to [r1 r2 r3] — and back to world coordinates.
inline bool planar_pose(const float* opoints, const double* normalised, const int32_t* idx, int m, const double c[3], double scale, const double axes[3][3] /* e1 e2 n (ascending eigenvalues reversed) */,
                        double pose[6]) {
  if (m < 4) return false;
  double e1[3] = {axes[0][0], axes[0][1], axes[0][2]}, e2[3] = {axes[1][0], axes[1][1], axes[1][2]};
  double nrm[3], cuv[2], su;
  cross3(e1, e2, nrm);   // right-handed whatever the eigenvectors' signs
  if (!hartley_side(normalised, idx, m, cuv, &su)) return false;
  const double cu = cuv[0], cv = cuv[1];
  double ata[9][9] = {};
  for (int i = 0; i < m; ++i) {
    const double d[3] = {(opoints[3 * (size_t)idx[i]] - c[0]) / scale, (opoints[3 * (size_t)idx[i] + 1] - c[1]) / scale, (opoints[3 * (size_t)idx[i] + 2] - c[2]) / scale};
    const double x = d[0] * e1[0] + d[1] * e1[1] + d[2] * e1[2], y = d[0] * e2[0] + d[1] * e2[1] + d[2] * e2[2];
    const double u = (normalised[2 * (size_t)idx[i]] - cu) / su, v = (normalised[2 * (size_t)idx[i] + 1] - cv) / su;
    const double r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, -u}, r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, -v};
    for (int a = 0; a < 9; ++a) for (int b = 0; b < 9; ++b) ata[a][b] += r0[a] * r0[b] + r1[a] * r1[b];
  }
  double hv[9];
  if (!null_vector9(ata, hv)) return false;   // collinear image or object points: no single homography
  // undo the image normalisation: H = [[su 0 cu] [0 su cv] [0 0 1]] Hn
  double H[9];
  for (int k = 0; k < 3; ++k) { H[k] = su * hv[k] + cu * hv[6 + k]; H[3 + k] = su * hv[3 + k] + cv * hv[6 + k]; H[6 + k] = hv[6 + k]; }
  if (H[8] < 0) for (double& x : H) x = -x;   // the centroid (x = y = 0) in front of the camera
  const double n1 = std::sqrt(H[0] * H[0] + H[3] * H[3] + H[6] * H[6]), n2 = std::sqrt(H[1] * H[1] + H[4] * H[4] + H[7] * H[7]);
  if (!(n1 > 1e-300) || !(n2 > 1e-300) || !std::isfinite(n1 + n2)) return false;
  const double r1[3] = {H[0] / n1, H[3] / n1, H[6] / n1}, r2[3] = {H[1] / n2, H[4] / n2, H[7] / n2};
  double r3[3];
  cross3(r1, r2, r3);
  const double lam = 0.5 * (n1 + n2), tp[3] = {H[2] / lam, H[5] / lam, H[8] / lam};
  double Rp[9] = {r1[0], r2[0], r3[0], r1[1], r2[1], r3[1], r1[2], r2[2], r3[2]};
  if (!nearest_rotation(Rp)) return false;
  // x_cam ~ Rp [e1 e2 n]^T (X - c) / scale + tp
  double R[9], tvec[3];
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) R[3 * r + k] = Rp[3 * r] * e1[k] + Rp[3 * r + 1] * e2[k] + Rp[3 * r + 2] * nrm[k];
  for (int r = 0; r < 3; ++r) tvec[r] = scale * tp[r] - (R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]);
  return pose_from_rt(R, tvec, pose);
}
// rsba pose (angle-axis world->camera, camera centre) from >= 6 correspondences idx[0..m): false when the points are degenerate
inline bool dlt_pose(const float* opoints, const double* normalised, const int32_t* idx, int m, double pose[6]) {
  if (m < 6) return false;
  double c[3] = {0, 0, 0}, scale = 0.0;
  for (int i = 0; i < m; ++i) for (int k = 0; k < 3; ++k) c[k] += opoints[3 * (size_t)idx[i] + k] / m;
  for (int i = 0; i < m; ++i) { double d2 = 0; for (int k = 0; k < 3; ++k) { const double d = opoints[3 * (size_t)idx[i] + k] - c[k]; d2 += d * d; } scale += std::sqrt(d2) / m; }
  if (!(scale > 0.0)) return false;
  // The shape of the cloud, from the eigenvalues l0 <= l1 <= l2 of the centred points' 3 x 3 scatter: collinear points determine no pose
  // (declined: the caller starts from the zero pose, as the reference does whenever the GS initialisation fails); coplanar points —
  // l0 < 1e-3 l1, cv::solvePnP's own test — go through the plane's homography (planar_pose), everything else through the 12-unknown DLT.
  {
    double sc[6] = {0, 0, 0, 0, 0, 0};   // xx xy xz yy yz zz
    for (int i = 0; i < m; ++i) {
      const double d[3] = {(opoints[3 * (size_t)idx[i]] - c[0]) / scale, (opoints[3 * (size_t)idx[i] + 1] - c[1]) / scale, (opoints[3 * (size_t)idx[i] + 2] - c[2]) / scale};
      sc[0] += d[0] * d[0]; sc[1] += d[0] * d[1]; sc[2] += d[0] * d[2]; sc[3] += d[1] * d[1]; sc[4] += d[1] * d[2]; sc[5] += d[2] * d[2];
    }
    double val[3], vec[3][3];
    eigen3(sc, val, vec);
    if (!(val[1] > 1e-4 * val[2])) return false;   // (a strip a hundred times longer than wide counts as a line)
    if (val[0] < 1e-3 * val[1]) { const double axes[3][3] = {{vec[2][0], vec[2][1], vec[2][2]}, {vec[1][0], vec[1][1], vec[1][2]}, {vec[0][0], vec[0][1], vec[0][2]}}; return planar_pose(opoints, normalised, idx, m, c, scale, axes, pose); }
  }
  double ata[12][12] = {};
  for (int i = 0; i < m; ++i) {
    const double X[4] = {(opoints[3 * (size_t)idx[i]] - c[0]) / scale, (opoints[3 * (size_t)idx[i] + 1] - c[1]) / scale, (opoints[3 * (size_t)idx[i] + 2] - c[2]) / scale, 1.0};
    const double u = normalised[2 * (size_t)idx[i]], v = normalised[2 * (size_t)idx[i] + 1];
    double r0[12] = {}, r1[12] = {};
    for (int k = 0; k < 4; ++k) { r0[k] = X[k]; r0[8 + k] = -u * X[k]; r1[4 + k] = X[k]; r1[8 + k] = -v * X[k]; }
    for (int a = 0; a < 12; ++a) for (int b = 0; b < 12; ++b) ata[a][b] += r0[a] * r0[b] + r1[a] * r1[b];
  }
  double pvec[12], gap[3];
  smallest_eigenvector12(ata, pvec, gap);
  if (!single_null_direction(gap)) return false;   // a second (near-)null direction, or no null direction to speak of: an ambiguous DLT is not an initialisation
  double M[9], t[3];
  for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) M[3 * r + k] = pvec[4 * r + k]; t[r] = pvec[4 * r + 3]; }
  // the points must end up in front of the camera (z of the centroid = t[2] in the shifted frame)
  if (t[2] < 0) { for (double& x : M) x = -x; for (double& x : t) x = -x; }
  double lambda = 0.0;
  for (int r = 0; r < 3; ++r) lambda += std::sqrt(M[3 * r] * M[3 * r] + M[3 * r + 1] * M[3 * r + 1] + M[3 * r + 2] * M[3 * r + 2]) / 3.0;
  if (!(lambda > 1e-300) || !std::isfinite(lambda)) return false;
  double R[9];
  for (int k = 0; k < 9; ++k) R[k] = M[k] / lambda;
  if (!nearest_rotation(R)) return false;
  // x_cam ~ R (X - c) / scale + t / lambda  =>  tvec = scale t / lambda - R c (up to the common factor 1 / scale, which the projection ignores)
  double tvec[3];
  for (int r = 0; r < 3; ++r) tvec[r] = scale * t[r] / lambda - (R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]);
  return pose_from_rt(R, tvec, pose);
}

// ---- the minimal solver of the global-shutter RANSAC (what cv::solvePnPRansac(..., CV_P3P) runs per sample): three points solved, a
// fourth chooses among the solutions.  The rule is stated in rsba_amd.h (rsba_pnp_p3p); this is its definition and the host path.
// Formulation: Grunert's ratio substitution.  With depths s1, s2, s3 along the unit bearings j1, j2, j3, sides a = |P2 P3|, b = |P1 P3|,
// c = |P1 P2| and cos(alpha) = j2.j3, cos(beta) = j1.j3, cos(gamma) = j1.j2, put s2 = u s1, s3 = v s1.  The three cosine laws give
//   u = N(v) / (2 D(v)),  N = (K - 1) v^2 - 2 K cos(beta) v + (K + 1),  D = cos(gamma) - v cos(alpha),  K = (a^2 - c^2) / b^2,
// and the quartic F(v) = N^2 - 4 cos(gamma) N D + 4 D^2 (1 - (c^2 / b^2)(v^2 - 2 cos(beta) v + 1)) = 0, whose coefficients are formed by
// polynomial arithmetic on N and D.  Positive depths mean v in (0, inf): the roots are looked for in t = v / (1 + v) in (0, 1), where
// F becomes P(t) = sum_i A_i t^i (1 - t)^(4 - i).  Between the roots of P' (themselves isolated between the roots of P'', and those by the
// root of P''') P is monotonic: each of the four intervals is bisected a fixed 40 times where P changes sign, then polished by two Newton
// steps on P.  Roots come in ascending t (ascending s3 / s1): that is the root order of the tie rule.
struct P3pProblem {
  double P[3][3];       // the three world points
  double j[3][3];       // their unit bearings
  double a2, b2, c2;    // squared sides |P2 P3|^2, |P1 P3|^2, |P1 P2|^2
  double cos_alpha, cos_beta, cos_gamma;   // j2 . j3, j1 . j3, j1 . j2
  double b;             // |P1 P3|
  double N[3], D[2];    // N(v) = N[0] + N[1] v + N[2] v^2, D(v) = D[0] + D[1] v
  double c[5];          // P(t), power basis
};
inline void p3p_bearing(double x, double y, double j[3]) {
  const double inv = 1.0 / std::sqrt(x * x + y * y + 1.0);
  j[0] = x * inv; j[1] = y * inv; j[2] = inv;
}
// false: two of the three world points coincide, or the three are collinear (smaller singular value of the centred triple below 1e-4 of the
// larger — on the eigenvalues of the scatter, their squares, that is 1e-8)
inline bool p3p_setup(const double P[3][3], const double j[3][3], P3pProblem& S) {
  for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) { S.P[i][k] = P[i][k]; S.j[i][k] = j[i][k]; }
  const double d12[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, d13[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
  const double d23[3] = {P[2][0] - P[1][0], P[2][1] - P[1][1], P[2][2] - P[1][2]};
  const double a2 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2], b2 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
  const double c2 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
  if (!(a2 > 0.0) || !(b2 > 0.0) || !(c2 > 0.0)) return false;
  // the two non-zero eigenvalues of the centred triple's scatter: their sum is (a^2 + b^2 + c^2) / 3, their product |d12 x d13|^2 / 3
  const double nx = d12[1] * d13[2] - d12[2] * d13[1], ny = d12[2] * d13[0] - d12[0] * d13[2], nz = d12[0] * d13[1] - d12[1] * d13[0];
  const double tr = (a2 + b2 + c2) / 3.0, prod = (nx * nx + ny * ny + nz * nz) / 3.0;
  const double big = 0.5 * (tr + std::sqrt(std::fmax(0.0, tr * tr - 4.0 * prod))), small = prod / big;
  if (!(small > 1e-8 * big)) return false;
  const double ca = j[1][0] * j[2][0] + j[1][1] * j[2][1] + j[1][2] * j[2][2], cb = j[0][0] * j[2][0] + j[0][1] * j[2][1] + j[0][2] * j[2][2];
  const double cg = j[0][0] * j[1][0] + j[0][1] * j[1][1] + j[0][2] * j[1][2];
  const double K = (a2 - c2) / b2, g = c2 / b2;
  S.a2 = a2; S.b2 = b2; S.c2 = c2; S.cos_alpha = ca; S.cos_beta = cb; S.cos_gamma = cg; S.b = std::sqrt(b2);
  S.N[0] = K + 1.0; S.N[1] = -2.0 * K * cb; S.N[2] = K - 1.0;
  S.D[0] = cg; S.D[1] = -ca;
  const double* n = S.N; const double* d = S.D;
  const double nn[5] = {n[0] * n[0], 2.0 * n[0] * n[1], 2.0 * n[0] * n[2] + n[1] * n[1], 2.0 * n[1] * n[2], n[2] * n[2]};
  const double nd[5] = {n[0] * d[0], n[0] * d[1] + n[1] * d[0], n[1] * d[1] + n[2] * d[0], n[2] * d[1], 0.0};
  const double dd[3] = {d[0] * d[0], 2.0 * d[0] * d[1], d[1] * d[1]}, q[3] = {1.0 - g, 2.0 * g * cb, -g};
  const double e[5] = {dd[0] * q[0], dd[0] * q[1] + dd[1] * q[0], dd[0] * q[2] + dd[1] * q[1] + dd[2] * q[0], dd[1] * q[2] + dd[2] * q[1], dd[2] * q[2]};
  double A[5];
  for (int k = 0; k < 5; ++k) A[k] = nn[k] - 4.0 * cg * nd[k] + 4.0 * e[k];
  // P(t) = sum_i A_i t^i (1 - t)^(4 - i)
  S.c[0] = A[0];
  S.c[1] = A[1] - 4.0 * A[0];
  S.c[2] = A[2] - 3.0 * A[1] + 6.0 * A[0];
  S.c[3] = A[3] - 2.0 * A[2] + 3.0 * A[1] - 4.0 * A[0];
  S.c[4] = A[4] - A[3] + A[2] - A[1] + A[0];
  return true;
}
// the roots of P in (0, 1), ascending
inline int p3p_roots(const P3pProblem& S, double roots[4]) {
  const double (&c4)[5] = S.c;
  const double c3[4] = {c4[1], 2.0 * c4[2], 3.0 * c4[3], 4.0 * c4[4]}, c2[3] = {c4[2], 3.0 * c4[3], 6.0 * c4[4]}, c1[2] = {c4[3], 4.0 * c4[4]};
  double x1, x2[2], x3[3];
  poly_bisect(c1, 1, 0.0, 1.0, &x1);
  poly_bisect(c2, 2, 0.0, x1, &x2[0]); poly_bisect(c2, 2, x1, 1.0, &x2[1]);
  poly_bisect(c3, 3, 0.0, x2[0], &x3[0]); poly_bisect(c3, 3, x2[0], x2[1], &x3[1]); poly_bisect(c3, 3, x2[1], 1.0, &x3[2]);
  const double edge[5] = {0.0, x3[0], x3[1], x3[2], 1.0};
  int count = 0;
  for (int i = 0; i < 4; ++i) {
    double t;
    if (!poly_bisect(c4, 4, edge[i], edge[i + 1], &t)) continue;
    for (int it = 0; it < 2; ++it) {   // Newton on P, a step taken only while it stays inside (0, 1)
      const double p = poly_eval(c4, 4, t), dp = poly_eval(c3, 3, t), tn = t - p / dp;
      if (tn > 0.0 && tn < 1.0) t = tn;
    }
    roots[count++] = t;
  }
  return count;
}
// the depths of one root; false unless all three are positive — above 1e-9 b: a camera centre in a world point is no solution — and finite
// (D = 0, where u = N / 2D is undefined, drops the root)
inline bool p3p_depths(const P3pProblem& S, double t, double s[3]) {
  const double r = 1.0 - t;
  const double w = std::sqrt(r * r + t * t - 2.0 * t * r * S.cos_beta);
  const double Nh = S.N[2] * t * t + S.N[1] * t * r + S.N[0] * r * r, Dh = S.D[1] * t + S.D[0] * r;
  if (!(std::fabs(Dh) > 1e-12) || !(w > 0.0)) return false;
  s[0] = S.b * r / w; s[1] = S.b * Nh / (2.0 * Dh * w); s[2] = S.b * t / w;
  const double least = 1e-9 * S.b;
  return s[0] > least && s[1] > least && s[2] > least && std::isfinite(s[0] + s[1] + s[2]);
}
// two Newton steps on the three cosine laws themselves, in the depths: the quartic's coefficients are formed with cancellation, the laws
// are not, so this is what makes a solution as accurate as its conditioning allows.  false: no longer three positive depths.
inline bool p3p_polish(const P3pProblem& S, double s[3]) {
  for (int it = 0; it < 2; ++it) {
    const double F[3] = {s[1] * s[1] + s[2] * s[2] - 2.0 * s[1] * s[2] * S.cos_alpha - S.a2, s[0] * s[0] + s[2] * s[2] - 2.0 * s[0] * s[2] * S.cos_beta - S.b2,
                         s[0] * s[0] + s[1] * s[1] - 2.0 * s[0] * s[1] * S.cos_gamma - S.c2};
    // Jacobian rows (0, p, q), (r, 0, w), (x, y, 0), halved
    const double p = s[1] - s[2] * S.cos_alpha, q = s[2] - s[1] * S.cos_alpha, r = s[0] - s[2] * S.cos_beta, w = s[2] - s[0] * S.cos_beta;
    const double x = s[0] - s[1] * S.cos_gamma, y = s[1] - s[0] * S.cos_gamma;
    const double det = 2.0 * (p * w * x + q * r * y);
    if (!(std::fabs(det) > 0.0)) break;
    s[0] -= (-w * y * F[0] + q * y * F[1] + p * w * F[2]) / det;
    s[1] -= (w * x * F[0] - q * x * F[1] + q * r * F[2]) / det;
    s[2] -= (r * y * F[0] + p * x * F[1] - p * r * F[2]) / det;
  }
  const double least = 1e-9 * S.b;
  return s[0] > least && s[1] > least && s[2] > least && std::isfinite(s[0] + s[1] + s[2]);
}
// the rigid motion that takes P_i onto s_i j_i, through the orthonormal triad of each triangle: x_cam = R X + tvec
inline void p3p_triad(const double A[3], const double B[3], const double C[3], double e[3][3]) {
  const double u[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, v[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
  const double iu = 1.0 / std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int k = 0; k < 3; ++k) e[0][k] = u[k] * iu;
  double n[3];
  cross3(e[0], v, n);
  const double in = 1.0 / std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  for (int k = 0; k < 3; ++k) e[2][k] = n[k] * in;
  cross3(e[2], e[0], e[1]);
}
inline void p3p_rt(const P3pProblem& S, const double s[3], double R[9], double tvec[3]) {
  double Q[3][3], e[3][3], f[3][3];
  for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) Q[i][k] = s[i] * S.j[i][k];
  p3p_triad(S.P[0], S.P[1], S.P[2], e);
  p3p_triad(Q[0], Q[1], Q[2], f);
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) R[3 * r + k] = f[0][r] * e[0][k] + f[1][r] * e[1][k] + f[2][r] * e[2][k];
  for (int r = 0; r < 3; ++r) {
    const double pc[3] = {(S.P[0][0] + S.P[1][0] + S.P[2][0]) / 3.0, (S.P[0][1] + S.P[1][1] + S.P[2][1]) / 3.0, (S.P[0][2] + S.P[1][2] + S.P[2][2]) / 3.0};
    tvec[r] = (Q[0][r] + Q[1][r] + Q[2][r]) / 3.0 - (R[3 * r] * pc[0] + R[3 * r + 1] * pc[1] + R[3 * r + 2] * pc[2]);
  }
}
// squared distance between the projection of X and the normalised image point (x, y); false: X is not in front of the camera
inline bool p3p_fourth(const double R[9], const double tvec[3], const double X[3], double x, double y, double* dist2) {
  const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + tvec[2];
  if (!(z > 0.0)) return false;
  const double dx = (R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + tvec[0]) / z - x, dy = (R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + tvec[1]) / z - y;
  *dist2 = dx * dx + dy * dy;
  return std::isfinite(*dist2);
}
// rsba pose from the correspondences idx[0..3), chosen by idx[3].  false: declined (pose untouched).  num_solutions (may be null): the
// admissible solutions — three positive depths and the fourth point in front of the camera.
inline bool p3p_pose(const float* opoints, const double* normalised, const int32_t idx[4], double pose[6], int* num_solutions = nullptr) {
  if (num_solutions) *num_solutions = 0;
  for (int i = 0; i < 4; ++i) for (int k = i + 1; k < 4; ++k) if (idx[i] == idx[k]) return false;
  double P[3][3], j[3][3];
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) P[i][k] = opoints[3 * (size_t)idx[i] + k];
    p3p_bearing(normalised[2 * (size_t)idx[i]], normalised[2 * (size_t)idx[i] + 1], j[i]);
  }
  P3pProblem S;
  if (!p3p_setup(P, j, S)) return false;
  const double X4[3] = {opoints[3 * (size_t)idx[3]], opoints[3 * (size_t)idx[3] + 1], opoints[3 * (size_t)idx[3] + 2]};
  double roots[4], bestR[9], bestT[3], best = 0.0;
  const int count = p3p_roots(S, roots);
  int found = 0;
  for (int i = 0; i < count; ++i) {
    double s[3], R[9], tvec[3], d2;
    if (!p3p_depths(S, roots[i], s) || !p3p_polish(S, s)) continue;
    p3p_rt(S, s, R, tvec);
    if (!p3p_fourth(R, tvec, X4, normalised[2 * (size_t)idx[3]], normalised[2 * (size_t)idx[3] + 1], &d2)) continue;
    if (found == 0 || d2 < best) { best = d2; for (int k = 0; k < 9; ++k) bestR[k] = R[k]; for (int k = 0; k < 3; ++k) bestT[k] = tvec[k]; }
    ++found;
  }
  if (found == 0) return false;
  double out[6];
  if (!pose_from_rt(bestR, bestT, out)) return false;   // (num_solutions stays 0: a declined subset reports none)
  for (int k = 0; k < 6; ++k) pose[k] = out[k];
  if (num_solutions) *num_solutions = found;
  return true;
}

// The global-shutter RANSAC behind solveGsPnPRansac and solveGsPnPRansacP3P: `iterationsCount` subsets of m distinct indices
// (distinct_subsets), a start pose per subset, every start refined and scored on the device, the first task with the most
// inliers among those with a status wins.  start_pose(normalised, pick, p) is the host minimal solver — a subset it declines is no task —
// and its poses go through rsba_pnp_tasks (GLOBAL, 5 iterations) in one launch; with hypotheses_on_device the whole batch, start poses
// included, is device_hypotheses(subsets, tasks, poses [tasks][6], status, count) instead.  Returns the winner's inliers (0: none found).
template <class StartPose, class DeviceHypotheses>
inline int gs_ransac(const float* opoints, const float* ipoints, int n, const double cam[NUM_CAM_PARAMS], double pose[6], int m, int iterationsCount,
                     float reprojectionError, uint64_t rng_state, int device, bool hypotheses_on_device, StartPose&& start_pose,
                     DeviceHypotheses&& device_hypotheses) {
  if (n < m || iterationsCount <= 0) return 0;
  const std::vector<int32_t> all_subsets = distinct_subsets(n, m, iterationsCount, rng_state);
  std::vector<double> poses;
  std::vector<uint8_t> status;
  std::vector<int32_t> count;
  int tasks = iterationsCount, stride = 6;
  if (hypotheses_on_device) {
    poses.resize((size_t)tasks * 6); status.resize((size_t)tasks); count.resize((size_t)tasks);
    device_hypotheses(all_subsets.data(), tasks, poses.data(), status.data(), count.data());
  } else {
    const std::vector<double> nrm = normalised_points(cam, ipoints, n);
    std::vector<int32_t> subsets; std::vector<double> inits;
    for (int it = 0; it < iterationsCount; ++it) {
      const int32_t* pick = &all_subsets[(size_t)it * m];
      double p[6];
      if (!start_pose(nrm.data(), pick, p)) continue;
      subsets.insert(subsets.end(), pick, pick + m);
      inits.insert(inits.end(), p, p + 6); inits.insert(inits.end(), p, p + 6);
    }
    tasks = (int)(inits.size() / 12); stride = 12;
    if (tasks == 0) return 0;
    std::vector<double> cost((size_t)tasks);
    poses.resize((size_t)tasks * 12); status.resize((size_t)tasks); count.resize((size_t)tasks);
    const int32_t sl[2] = {0, 1};
    check(rsba_pnp_tasks(device, cam, (int32_t)GLOBAL, sl, opoints, ipoints, n, subsets.data(), m, tasks, inits.data(), 12, 5, 0, reprojectionError,
                                     poses.data(), status.data(), cost.data(), count.data()));
  }
  const int best = most_inliers(status.data(), count.data(), tasks, [](uint8_t st) { return st != 0; });
  if (best < 0) return 0;
  for (int k = 0; k < 6; ++k) pose[k] = poses[(size_t)best * stride + k];
  return count[(size_t)best];
}

// The start of solveRsPnP and solveRsPnPRansac: init = the two poses of the four vectors.  true: all four are zero, which is where the
// reference takes a global-shutter initialisation instead.
inline bool start_poses(const double rvec[3], const double tvec[3], const double rvec2[3], const double tvec2[3], double init[12]) {
  double l1 = 0.0;
  for (int i = 0; i < 3; ++i) l1 += std::fabs(rvec[i]) + std::fabs(tvec[i]) + std::fabs(rvec2[i]) + std::fabs(tvec2[i]);
  to_pose(rvec, tvec, init);
  to_pose(rvec2, tvec2, init + 6);
  return l1 == 0.0;
}

}  // namespace pnp_detail

// cv::solvePnP(..., SOLVEPNP_ITERATIVE) as the reference uses it at solveRSpnp.cpp:111-117: DLT over all points, then a
// Levenberg-Marquardt refinement of the global-shutter reprojection error (on the device).  pose = rsba's 6-vector.
inline bool solveGsPnP(const float* opoints, const float* ipoints, int n, const double cam[NUM_CAM_PARAMS], double pose[6], int device = 0) {
  const std::vector<double> nrm = hyp_detail::normalised_points(cam, ipoints, n);
  const std::vector<int32_t> all = hyp_detail::all_indices(n);
  double init[12], out[12], cost = 0.0; uint8_t status = 0; int32_t inl = 0;
  if (!pnp_detail::dlt_pose(opoints, nrm.data(), all.data(), n, init)) return false;
  for (int k = 0; k < 6; ++k) init[6 + k] = init[k];
  const int32_t sl[2] = {0, 1};
  hyp_detail::check(rsba_pnp_tasks(device, cam, (int32_t)GLOBAL, sl, opoints, ipoints, n, all.data(), n, 1, init, 0, 20, 0, 0.0f, out, &status, &cost, &inl));
  for (int k = 0; k < 6; ++k) pose[k] = status == 1 ? out[k] : init[k];
  return true;
}

// cv::solvePnPRansac as the reference uses it at solveRSpnp.cpp:437-449: minimal subsets, a pose per subset, the pose with the most
// points inside reprojectionError wins (pnp_detail::gs_ransac).  The subsets' DLT poses are refined and scored on the device in ONE
// launch.  Returns the number of inliers of the winner (0: none found).  hypotheses_on_device: the subsets' DLT poses are computed on the
// device too (rsba_pnp_gs_hypotheses) instead of by pnp_detail::dlt_pose here — the same subsets, the same rule for the winner.
inline int solveGsPnPRansac(const float* opoints, const float* ipoints, int n, const double cam[NUM_CAM_PARAMS], double pose[6], int iterationsCount,
                            float reprojectionError, int min_points_count = 6, uint64_t rng_state = 0x9e3779b97f4a7c15ULL, int device = 0,
                            bool hypotheses_on_device = false) {
  const int m = min_points_count < 6 ? 6 : min_points_count;
  return pnp_detail::gs_ransac(opoints, ipoints, n, cam, pose, m, iterationsCount, reprojectionError, rng_state, device, hypotheses_on_device,
    [&](const double* nrm, const int32_t* pick, double p[6]) { return pnp_detail::dlt_pose(opoints, nrm, pick, m, p); },
    [&](const int32_t* subsets, int tasks, double* poses, uint8_t* status, int32_t* count) {
      hyp_detail::check(rsba_pnp_gs_hypotheses(device, cam, opoints, ipoints, n, subsets, m, tasks, 5, reprojectionError, poses, status, nullptr, count));
    });
}

// cv::solvePnPRansac(..., CV_P3P) as the reference uses it without a guess at VideoSfMHandler.cc:726-731: four-point samples from the same
// generator and the same distinct-index sampling as solveGsPnPRansac, the minimal solver's pose per sample (pnp_detail::p3p_pose: three
// points solved, the fourth chooses), refined and scored like the DLT hypotheses (rsba_pnp_tasks, GLOBAL, 5 iterations, m = 4), the same rule
// for the winner.  Returns the winner's inliers (0: none found).  hypotheses_on_device: the whole batch in one call (rsba_pnp_gs_hypotheses_p3p).
inline int solveGsPnPRansacP3P(const float* opoints, const float* ipoints, int n, const double cam[NUM_CAM_PARAMS], double pose[6], int iterationsCount,
                               float reprojectionError, uint64_t rng_state = 0x9e3779b97f4a7c15ULL, int device = 0, bool hypotheses_on_device = false) {
  return pnp_detail::gs_ransac(opoints, ipoints, n, cam, pose, 4, iterationsCount, reprojectionError, rng_state, device, hypotheses_on_device,
    [&](const double* nrm, const int32_t* pick, double p[6]) { return pnp_detail::p3p_pose(opoints, nrm, pick, p); },
    [&](const int32_t* subsets, int tasks, double* poses, uint8_t* status, int32_t* count) {
      hyp_detail::check(rsba_pnp_gs_hypotheses_p3p(device, cam, opoints, ipoints, n, subsets, tasks, 5, reprojectionError, poses, status, nullptr, count));
    });
}

// solveRSpnp.cpp:100-192.  Returns summary.IsSolutionUsable(); the four vectors are updated only then.
inline bool solveRsPnP(const float* opoints, const float* ipoints, int n, const double cam[NUM_CAM_PARAMS], double rvec[3], double tvec[3],
                       double rvec2[3], double tvec2[3], const SHUTTER shutter, const int scanlines[2], int device = 0) {
  double init[12], out[12], cost = 0.0; uint8_t status = 0; int32_t inl = 0;
  if (pnp_detail::start_poses(rvec, tvec, rvec2, tvec2, init) && solveGsPnP(opoints, ipoints, n, cam, init, device))   // GS Init (:111-117): both poses start from the global-shutter one
    for (int k = 0; k < 6; ++k) init[6 + k] = init[k];
  const std::vector<int32_t> all = hyp_detail::all_indices(n);
  const int32_t sl[2] = {scanlines[0], scanlines[1]};
  hyp_detail::check(rsba_pnp_tasks(device, cam, (int32_t)shutter, sl, opoints, ipoints, n, all.data(), n, 1, init, 0, 10, 0, 0.0f, out, &status, &cost, &inl));
  if (status != 1) return false;
  hyp_detail::from_pose(out, rvec, tvec);
  hyp_detail::from_pose(out + 6, rvec2, tvec2);
  return true;
}

// solveRSpnp.cpp:413-524.  inliers (may be null) receives the indices of the winning hypothesis' inliers.
inline void solveRsPnPRansac(const float* opoints, const float* ipoints, int n, const double cam[NUM_CAM_PARAMS], double rvec[3], double tvec[3],
                             double rvec2[3], double tvec2[3], const SHUTTER shutter, const int scanlines[2], int iterationsCount = 100,
                             float reprojectionError = 8.0f, int minInliersCount = 100, std::vector<int>* inliers = nullptr,
                             int min_points_count = 6, uint64_t rng_state = 0xffffffffULL, int device = 0, bool hypotheses_on_device = false) {
  double init[12];
  if (pnp_detail::start_poses(rvec, tvec, rvec2, tvec2, init)) {   // GS Init (:437-449): global-shutter RANSAC at twice the threshold, taken when it finds more than four inliers
    double gs[6];
    if (solveGsPnPRansac(opoints, ipoints, n, cam, gs, iterationsCount, reprojectionError * 2, min_points_count, rng_state ^ 0x9e3779b97f4a7c15ULL, device, hypotheses_on_device) > 4)
      for (int k = 0; k < 6; ++k) init[k] = init[6 + k] = gs[k];
  }
  if (minInliersCount <= 0) minInliersCount = n;                                        // :453-454
  const int32_t sl[2] = {scanlines[0], scanlines[1]};
  double best_pose[12];
  for (int k = 0; k < 12; ++k) best_pose[k] = init[k];
  int best_count = 0; bool have_best = false;
  if (n >= min_points_count && iterationsCount > 0) {                                   // :473-478
    // the subsets PnPSolver::operator() draws: one mask, shuffled cumulatively by generateVar (:334-337, :381-391)
    const int m = min_points_count;
    std::vector<char> mask((size_t)n, 0);
    for (int i = 0; i < m; ++i) mask[(size_t)i] = 1;
    hyp_detail::Rng gen(rng_state);
    std::vector<int32_t> subsets((size_t)iterationsCount * m);
    for (int it = 0; it < iterationsCount; ++it) {
      for (int i = 0; i < n; ++i) { const int i1 = gen.uniform(0, n), i2 = gen.uniform(0, n); const char c = mask[(size_t)i1]; mask[(size_t)i1] = mask[(size_t)i2]; mask[(size_t)i2] = c; }
      int col = 0;
      for (int i = 0; i < n; ++i) if (mask[(size_t)i]) subsets[(size_t)it * m + col++] = i;
    }
    std::vector<double> poses((size_t)iterationsCount * 12), cost((size_t)iterationsCount);
    std::vector<uint8_t> status((size_t)iterationsCount);
    std::vector<int32_t> count((size_t)iterationsCount);
    hyp_detail::check(rsba_pnp_tasks(device, cam, (int32_t)shutter, sl, opoints, ipoints, n, subsets.data(), m, iterationsCount, init, 0, 10, 1,
                                     reprojectionError, poses.data(), status.data(), cost.data(), count.data()));
    for (int it = 0; it < iterationsCount; ++it) {                                      // pnpTask's bookkeeping, in order (:312-326, :339-346)
      if (status[(size_t)it] != 0 && count[(size_t)it] > best_count) {
        best_count = count[(size_t)it]; have_best = true;
        for (int k = 0; k < 12; ++k) best_pose[k] = poses[(size_t)it * 12 + k];
      }
      if (best_count >= minInliersCount) break;
    }
  }
  if (have_best && best_count >= min_points_count) {                                    // :480-512
    std::vector<uint8_t> flags((size_t)n);
    hyp_detail::check(rsba_pnp_inliers(device, cam, (int32_t)shutter, sl, opoints, ipoints, n, best_pose, reprojectionError, flags.data()));
    std::vector<int32_t> idx;
    for (int i = 0; i < n; ++i) if (flags[(size_t)i]) idx.push_back(i);
    // final solveRsPnP over the inliers from the winning poses (:496-502)
    double refined[12], c = 0.0; uint8_t st = 0; int32_t cnt = 0;
    hyp_detail::check(rsba_pnp_tasks(device, cam, (int32_t)shutter, sl, opoints, ipoints, n, idx.data(), (int32_t)idx.size(), 1, best_pose, 0, 10, 0,
                                     reprojectionError, refined, &st, &c, &cnt));
    const double* fin = st == 1 ? refined : best_pose;
    hyp_detail::from_pose(fin, rvec, tvec);
    hyp_detail::from_pose(fin + 6, rvec2, tvec2);
    if (inliers) inliers->assign(idx.begin(), idx.end());
  } else {                                                                              // :513-521
    for (int i = 0; i < 3; ++i) { rvec[i] = tvec[i] = rvec2[i] = tvec2[i] = 0.0; }
    if (inliers) inliers->clear();
  }
}

}  // namespace rsba_amd
