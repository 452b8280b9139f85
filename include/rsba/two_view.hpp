// Two-view bootstrap: the relative pose of two frames from their 2-D / 2-D correspondences alone — what gives the first two frames of a
// video their poses, so that createTracks, processFrame and BA (create_tracks.hpp, new_frame.hpp) have something to start from.  The
// reference has no such step (its initialize() is a BA over frames that already carry 3-D points), so this text and rsba_amd.h
// (rsba_epipolar_*) are the definition; epi_detail below is its host form, which the device kernels (rsba_amd/csrc/kernels_epipolar.hip,
// kernels_five_point.hip) restate and the tests hold both to.
//
// Conventions.  a = (xa, ya, 1), b = (xb, yb, 1) are the undistorted, normalised image points of one correspondence in frame A and frame B
// (hyp_detail::normalised_point).  E is row-major with b^T E a = 0.  Camera A is the origin; camera B sees x_B = R x_A + t, E = [t]x R, and
// the pose of B in A's frame is hyp_detail::pose_from_rt(R, t) with |t| = 1: the length of the baseline is the unit of the reconstruction.
//
// eight_point.  Hartley normalisation of each side's m points (centroid, mean distance scaled to sqrt 2), the 9 x 9 Gram matrix of the rows
// (xb xa, xb ya, xb, yb xa, yb ya, yb, xa, ya, 1), its null vector by hyp_detail::null_vector9 (smallest_eigenvector12 with three idle unknowns
// at twice the trace, as planar_pose takes it; zero off-diagonals are skipped, so the rotations are those of a 9 x 9 sweep; the DLT's two
// gap tests), the normalisation undone, then the projection onto the essential manifold: V and the singular values s1 >= s2 from eigen3 of
// E^T E, u_i = E v_i / s_i for the two largest, u3 = u1 x u2, v3 = v1 x v2 (so det U = det V = +1), result u1 v1^T + u2 v2^T.
// Declined: m < 8, a repeated index, a Hartley scale that is not positive, a second null direction (coplanar scene points, a pure rotation),
// s2 not above 1e-6 s1, a result that is not finite.
// Sign rule: the entry of E with the largest magnitude (the first such entry, row-major) is positive.  Flipping E swaps the two rotations
// below and leaves the set of candidates, and so the chosen pose, as it is; comparisons of E are made up to sign.
//
// Pose recovery.  From the same decomposition of a given E: R1 = U W V^T, R2 = U W^T V^T (W a quarter turn about z), t = u3 / |u3|; the
// candidates in the fixed order (R1, +t), (R1, -t), (R2, +t), (R2, -t) — the pair (v1, v2) taken the way round that makes the largest
// component of v3 positive, since s1 = s2 leaves that to rounding.  A correspondence is in front for a candidate when the least-squares
// depths of z_a R a + t = z_b b are both positive (2 x 2 normal equations, closed form).  The candidate with the most INLIERS in front wins,
// ties go to the first.
// five_point.  The minimal solver beside it (TwoViewOptions::solver; rsba_amd.h at rsba_epipolar_five_point states the rule): the null space
// X, Y, Z, W of the five constraint rows by Householder reflections, the ten cubics of E = x X + y Y + z Z + W in a 10 x 20 matrix,
// Gauss-Jordan with row pivoting, Nister's degree-10 eliminant in z, its real roots from a ladder of derivatives with fixed bisection and
// Newton counts (|z| > 1 through the reversed polynomial), (x, y) per root, a Gauss-Newton polish on the cubics, unit norm and the sign rule
// above; up to ten solutions in the order of fp_key.  Coplanar scene points are not declined; a pure rotation (a singular elimination) is.
// Inlier rule.  Sampson distance in normalised coordinates, fp64: d^2 = (b^T E a)^2 / ((E a)_x^2 + (E a)_y^2 + (E^T b)_x^2 + (E^T b)_y^2);
// inlier iff d^2 f^2 <= threshold_px^2 with f = (fx_a + fy_a + fx_b + fy_b) / 4.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "ceres_handler.hpp"
#include "create_tracks.hpp"
#include "solve_rs_pnp.hpp"

namespace rsba_amd {

namespace epi_detail {

// V (columns v1 v2 v3, singular values descending), U (columns u1 u2 u3) and s1, s2 of a 3 x 3 matrix that has rank two (or nearly);
// false: s2 is not above 1e-6 s1
inline bool essential_svd(const double E[9], double U[3][3] /* [column][row] */, double V[3][3] /* [column][row] */, double s[2]) {
  double sym[6] = {0, 0, 0, 0, 0, 0};   // E^T E: xx xy xz yy yz zz
  for (int r = 0; r < 3; ++r) {
    sym[0] += E[3 * r] * E[3 * r]; sym[1] += E[3 * r] * E[3 * r + 1]; sym[2] += E[3 * r] * E[3 * r + 2];
    sym[3] += E[3 * r + 1] * E[3 * r + 1]; sym[4] += E[3 * r + 1] * E[3 * r + 2]; sym[5] += E[3 * r + 2] * E[3 * r + 2];
  }
  double val[3], vec[3][3];
  hyp_detail::eigen3(sym, val, vec);
  s[0] = std::sqrt(std::fmax(0.0, val[2])); s[1] = std::sqrt(std::fmax(0.0, val[1]));
  if (!(s[1] > 1e-6 * s[0])) return false;
  for (int k = 0; k < 3; ++k) { V[0][k] = vec[2][k]; V[1][k] = vec[1][k]; }
  for (int c = 0; c < 2; ++c)
    for (int r = 0; r < 3; ++r) U[c][r] = (E[3 * r] * V[c][0] + E[3 * r + 1] * V[c][1] + E[3 * r + 2] * V[c][2]) / s[c];
  hyp_detail::cross3(U[0], U[1], U[2]);
  hyp_detail::cross3(V[0], V[1], V[2]);
  // s1 = s2 for an essential matrix, so (v1, v2) is any orthonormal pair of their plane and rounding alone decides which way round it
  // runs — which swaps (R1, +t) with (R2, -t).  Fixed here: the component of v3 with the largest magnitude (the first such) is positive.
  int lead = 0;
  for (int k = 1; k < 3; ++k) if (std::fabs(V[2][k]) > std::fabs(V[2][lead])) lead = k;
  if (V[2][lead] < 0) for (int k = 0; k < 3; ++k) { V[1][k] = -V[1][k]; U[1][k] = -U[1][k]; V[2][k] = -V[2][k]; U[2][k] = -U[2][k]; }
  return true;
}

// the pieces of eight_point, apart so that the tests can seed errors between them
struct Hartley { double ca[2], cb[2], sa, sb; };   // x' = (x - c) / s per side
inline bool hartley(const double* na, const double* nb, const int32_t* idx, int m, Hartley& H) {
  const bool a = hyp_detail::hartley_side(na, idx, m, H.ca, &H.sa), b = hyp_detail::hartley_side(nb, idx, m, H.cb, &H.sb);
  return a && b;
}
// the null direction of the m epipolar constraints in the coordinates of H, taken back to the normalised image coordinates; false: ambiguous
inline bool null_matrix(const double* na, const double* nb, const int32_t* idx, int m, const Hartley& H, double F[9]) {
  double ata[9][9] = {};
  for (int i = 0; i < m; ++i) {
    const size_t j = 2 * (size_t)idx[i];
    const double xa = (na[j] - H.ca[0]) / H.sa, ya = (na[j + 1] - H.ca[1]) / H.sa, xb = (nb[j] - H.cb[0]) / H.sb, yb = (nb[j + 1] - H.cb[1]) / H.sb;
    const double r[9] = {xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, 1.0};
    for (int a = 0; a < 9; ++a) for (int b = 0; b < 9; ++b) ata[a][b] += r[a] * r[b];
  }
  double ev[9];
  if (!hyp_detail::null_vector9(ata, ev)) return false;   // a second null direction: a plane, or no baseline
  // undo the normalisation: F = Tb^T Fn Ta, T = [[1/s 0 -cx/s] [0 1/s -cy/s] [0 0 1]]
  double M[9];
  for (int r = 0; r < 3; ++r) {
    M[3 * r] = ev[3 * r] / H.sa; M[3 * r + 1] = ev[3 * r + 1] / H.sa;
    M[3 * r + 2] = ev[3 * r + 2] - (H.ca[0] * ev[3 * r] + H.ca[1] * ev[3 * r + 1]) / H.sa;
  }
  for (int k = 0; k < 3; ++k) {
    F[k] = M[k] / H.sb; F[3 + k] = M[3 + k] / H.sb;
    F[6 + k] = M[6 + k] - (H.cb[0] * M[k] + H.cb[1] * M[3 + k]) / H.sb;
  }
  return true;
}
// the nearest matrix with singular values (1, 1, 0)
inline bool project_essential(const double F[9], double out[9]) {
  double U[3][3], V[3][3], s[2];
  if (!essential_svd(F, U, V, s)) return false;
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) out[3 * r + k] = U[0][r] * V[0][k] + U[1][r] * V[1][k];
  return true;
}
// the sign rule, and the last reason to decline
inline bool signed_finite(double out[9]) {
  int lead = 0;
  for (int k = 1; k < 9; ++k) if (std::fabs(out[k]) > std::fabs(out[lead])) lead = k;
  if (out[lead] < 0) for (int k = 0; k < 9; ++k) out[k] = -out[k];
  for (int k = 0; k < 9; ++k) if (!std::isfinite(out[k])) return false;
  return true;
}
// the essential matrix of the correspondences idx[0..m) of the normalised points na, nb [.][2]; false: declined (E untouched)
inline bool eight_point(const double* na, const double* nb, const int32_t* idx, int m, double E[9]) {
  if (m < 8) return false;
  for (int i = 0; i < m; ++i) for (int k = i + 1; k < m; ++k) if (idx[i] == idx[k]) return false;
  Hartley H;
  double F[9], out[9];
  if (!hartley(na, nb, idx, m, H) || !null_matrix(na, nb, idx, m, H, F) || !project_essential(F, out) || !signed_finite(out)) return false;
  for (int k = 0; k < 9; ++k) E[k] = out[k];
  return true;
}

// the two rotations and the baseline direction of E; false: declined
struct Candidates { double R[2][9]; double t[3]; };
inline bool decompose(const double E[9], Candidates& C) {
  double U[3][3], V[3][3], s[2];
  if (!essential_svd(E, U, V, s)) return false;
  const double nt = std::sqrt(U[2][0] * U[2][0] + U[2][1] * U[2][1] + U[2][2] * U[2][2]);
  if (!(nt > 0.0)) return false;
  for (int k = 0; k < 3; ++k) C.t[k] = U[2][k] / nt;
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) {
    const double w = U[1][r] * V[0][k] - U[0][r] * V[1][k], z = U[2][r] * V[2][k];   // U W V^T = u2 v1^T - u1 v2^T + u3 v3^T
    C.R[0][3 * r + k] = w + z; C.R[1][3 * r + k] = z - w;
  }
  for (int c = 0; c < 2; ++c) for (int k = 0; k < 9; ++k) if (!std::isfinite(C.R[c][k])) return false;
  return std::isfinite(C.t[0] + C.t[1] + C.t[2]);
}

// the two deciding comparisons: the device evaluates these operations in this order (rsba_amd/csrc/two_view_rules.hpp, contraction off)
inline bool sampson_inlier(const double E[9], double xa, double ya, double xb, double yb, double f2, double thr2, double* d2_out = nullptr) {
  const double l0 = E[0] * xa + E[1] * ya + E[2], l1 = E[3] * xa + E[4] * ya + E[5], l2 = E[6] * xa + E[7] * ya + E[8];
  const double m0 = E[0] * xb + E[3] * yb + E[6], m1 = E[1] * xb + E[4] * yb + E[7];
  const double r = xb * l0 + yb * l1 + l2;
  const double den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
  const double d2 = (r * r) / den;
  if (d2_out) *d2_out = d2;
  return d2 * f2 <= thr2;
}
inline bool in_front(const double R[9], const double t[3], double sign, double xa, double ya, double xb, double yb) {
  const double p0 = R[0] * xa + R[1] * ya + R[2], p1 = R[3] * xa + R[4] * ya + R[5], p2 = R[6] * xa + R[7] * ya + R[8];
  const double t0 = sign * t[0], t1 = sign * t[1], t2 = sign * t[2];
  const double pp = p0 * p0 + p1 * p1 + p2 * p2, qq = xb * xb + yb * yb + 1.0, pq = p0 * xb + p1 * yb + p2;
  const double pt = p0 * t0 + p1 * t1 + p2 * t2, qt = xb * t0 + yb * t1 + t2;
  const double det = pp * qq - pq * pq;
  const double za = (pq * qt - qq * pt) / det, zb = (pp * qt - pq * pt) / det;
  return za > 0.0 && zb > 0.0;
}

inline double mean_focal2(const double cam_a[NUM_CAM_PARAMS], const double cam_b[NUM_CAM_PARAMS]) {
  const double f = (cam_a[0] + cam_a[1] + cam_b[0] + cam_b[1]) / 4.0;
  return f * f;
}

// counts of one E over all n correspondences, the winning candidate and its pose; false: declined (nothing written but zero counts)
inline bool score(const double* na, const double* nb, int n, const double E[9], double f2, double thr2, int32_t* num_inliers, int32_t num_front[4],
                  double pose[6], int* winner = nullptr, uint8_t* mask = nullptr) {
  *num_inliers = 0;
  for (int c = 0; c < 4; ++c) num_front[c] = 0;
  Candidates C;
  if (!decompose(E, C)) return false;
  int32_t inl = 0, front[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const double xa = na[2 * (size_t)i], ya = na[2 * (size_t)i + 1], xb = nb[2 * (size_t)i], yb = nb[2 * (size_t)i + 1];
    const bool in = sampson_inlier(E, xa, ya, xb, yb, f2, thr2);
    if (mask) mask[i] = in ? 1 : 0;
    if (!in) continue;
    ++inl;
    for (int c = 0; c < 4; ++c) if (in_front(C.R[c >> 1], C.t, (c & 1) ? -1.0 : 1.0, xa, ya, xb, yb)) ++front[c];
  }
  int best = 0;
  for (int c = 1; c < 4; ++c) if (front[c] > front[best]) best = c;
  const double tb[3] = {(best & 1) ? -C.t[0] : C.t[0], (best & 1) ? -C.t[1] : C.t[1], (best & 1) ? -C.t[2] : C.t[2]};
  double out[6];
  if (!hyp_detail::pose_from_rt(C.R[best >> 1], tb, out)) return false;
  for (int k = 0; k < 6; ++k) pose[k] = out[k];
  *num_inliers = inl;
  for (int c = 0; c < 4; ++c) num_front[c] = front[c];
  if (winner) *winner = best;
  return true;
}

// ---- five_point: the minimal solver (rsba_amd.h: rsba_epipolar_five_point states the rule; this is its definition and the host path) ----
// Polynomials in (x, y, z) by coefficient arrays.  Linear: (x, y, z, 1).  Quadratic, 10: x^2 xy xz x y^2 yz y z^2 z 1 (kQuad[i][j] = the
// product of linear terms i and j).  Cubic, 20, in the column order the elimination wants: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy |
// xz^2 xz x yz^2 yz y z^3 z^2 z 1 (kCubic[q][l] = quadratic term q times linear term l).
constexpr int kQuad[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
constexpr int kCubic[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {5, 9, 11, 12}, {3, 1, 6, 7},
                               {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
constexpr double kFiveRankTol = 1e-7;    // a Householder diagonal not above this times the longest constraint row: a fifth null direction
constexpr double kFivePivotTol = 1e-7;   // an elimination pivot not above this times the largest entry of the 10 x 20 matrix: singular
constexpr int kFiveNewton = 2, kFivePolish = 2;

struct FivePointDiag { double rank_ratio = -1.0, pivot_ratio = -1.0; };   // the smallest of each quantity the two tolerances are compared with

// q += s a b (linear times linear), c += s q l (quadratic times linear)
inline void fp_quad_add(double q[10], const double a[4], const double b[4], double s) {
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) q[kQuad[i][j]] += s * (a[i] * b[j]);
}
inline void fp_cubic_add(double c[20], const double q[10], const double l[4], double s) {
  for (int k = 0; k < 10; ++k) for (int j = 0; j < 4; ++j) c[kCubic[k][j]] += s * (q[k] * l[j]);
}

// orthonormal basis N[4][9] of the null space of the five constraint rows, by Householder reflections of the 9 x 5 matrix of the rows
// (no Gram matrix: the conditioning is that of the rows themselves); false: a fifth null direction
inline bool fp_null_space(double a[5][9], double N[4][9], FivePointDiag* diag) {
  double longest = 0.0, beta[5];
  for (int k = 0; k < 5; ++k) { double s = 0.0; for (int i = 0; i < 9; ++i) s += a[k][i] * a[k][i]; longest = std::fmax(longest, std::sqrt(s)); }
  double smallest = -1.0;
  for (int k = 0; k < 5; ++k) {
    double s = 0.0;
    for (int i = k; i < 9; ++i) s += a[k][i] * a[k][i];
    const double nrm = std::sqrt(s);
    if (smallest < 0.0 || nrm < smallest) smallest = nrm;
    if (diag) diag->rank_ratio = smallest / longest;
    if (!(nrm > kFiveRankTol * longest)) return false;
    a[k][k] -= a[k][k] >= 0.0 ? -nrm : nrm;
    double vv = 0.0;
    for (int i = k; i < 9; ++i) vv += a[k][i] * a[k][i];
    beta[k] = 2.0 / vv;
    for (int j = k + 1; j < 5; ++j) {
      double d = 0.0;
      for (int i = k; i < 9; ++i) d += a[k][i] * a[j][i];
      d *= beta[k];
      for (int i = k; i < 9; ++i) a[j][i] -= d * a[k][i];
    }
  }
  for (int m = 0; m < 4; ++m) {
    for (int i = 0; i < 9; ++i) N[m][i] = i == 5 + m ? 1.0 : 0.0;
    for (int k = 4; k >= 0; --k) {
      double d = 0.0;
      for (int i = k; i < 9; ++i) d += a[k][i] * N[m][i];
      d *= beta[k];
      for (int i = k; i < 9; ++i) N[m][i] -= d * a[k][i];
    }
  }
  return true;
}

// the ten cubics of E = x N0 + y N1 + z N2 + N3: row 0 det E, rows 1..9 (E E^T - trace_factor tr(E E^T) I) E, trace_factor = 1/2
inline void fp_constraints(const double N[4][9], double M[10][20], double trace_factor = 0.5) {
  double e[9][4];
  for (int k = 0; k < 9; ++k) for (int m = 0; m < 4; ++m) e[k][m] = N[m][k];
  for (int r = 0; r < 10; ++r) for (int c = 0; c < 20; ++c) M[r][c] = 0.0;
  for (int i = 0; i < 3; ++i) {   // det: e[0][i] (e[1][j] e[2][k] - e[1][k] e[2][j]), (i, j, k) cyclic
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    fp_quad_add(q, e[3 + j], e[6 + k], 1.0); fp_quad_add(q, e[3 + k], e[6 + j], -1.0);
    fp_cubic_add(M[0], q, e[i], 1.0);
  }
  double tr[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 9; ++k) fp_quad_add(tr, e[k], e[k], 1.0);
  for (int i = 0; i < 3; ++i) {
    double L[3][10];   // row i of E E^T - trace_factor tr I
    for (int j = 0; j < 3; ++j) {
      for (int c = 0; c < 10; ++c) L[j][c] = i == j ? -trace_factor * tr[c] : 0.0;
      for (int k = 0; k < 3; ++k) fp_quad_add(L[j], e[3 * i + k], e[3 * j + k], 1.0);
    }
    for (int c = 0; c < 3; ++c) for (int j = 0; j < 3; ++j) fp_cubic_add(M[1 + 3 * i + c], L[j], e[3 * j + c], 1.0);
  }
}

// Gauss-Jordan on the first ten columns, partial (row) pivoting; false: singular
inline bool fp_eliminate(double M[10][20], FivePointDiag* diag) {
  double big = 0.0, smallest = -1.0;
  for (int r = 0; r < 10; ++r) for (int c = 0; c < 20; ++c) big = std::fmax(big, std::fabs(M[r][c]));
  for (int c = 0; c < 10; ++c) {
    int piv = c;
    for (int r = c + 1; r < 10; ++r) if (std::fabs(M[r][c]) > std::fabs(M[piv][c])) piv = r;
    const double p = M[piv][c];
    if (smallest < 0.0 || std::fabs(p) < smallest) smallest = std::fabs(p);
    if (diag) diag->pivot_ratio = smallest / big;
    if (!(std::fabs(p) > kFivePivotTol * big)) return false;
    for (int k = 0; k < 20; ++k) { const double t = M[piv][k]; M[piv][k] = M[c][k]; M[c][k] = t / p; }
    for (int r = 0; r < 10; ++r) {
      if (r == c) continue;
      const double f = M[r][c];
      for (int k = 0; k < 20; ++k) M[r][k] -= f * M[c][k];
    }
  }
  return true;
}

// rows (4, 5), (6, 7), (8, 9) of the eliminated matrix, <upper> - z <lower>: B(z) (x, y, 1)^T = 0 with B[r] = (cubic, cubic, quartic) in z,
// ascending powers (B[r][0][4] = B[r][1][4] = 0)
inline void fp_reduce(const double M[10][20], double B[3][3][5]) {
  for (int r = 0; r < 3; ++r) {
    const double* u = M[4 + 2 * r]; const double* l = M[5 + 2 * r];
    for (int v = 0; v < 2; ++v) {   // x: columns 10 11 12 (z^2 z 1), y: 13 14 15
      const int c = 10 + 3 * v;
      B[r][v][0] = u[c + 2]; B[r][v][1] = u[c + 1] - l[c + 2]; B[r][v][2] = u[c] - l[c + 1]; B[r][v][3] = -l[c]; B[r][v][4] = 0.0;
    }
    B[r][2][0] = u[19]; B[r][2][1] = u[18] - l[19]; B[r][2][2] = u[17] - l[18]; B[r][2][3] = u[16] - l[17]; B[r][2][4] = -l[16];
  }
}
// det B(z), degree 10, ascending powers
inline void fp_eliminant(const double B[3][3][5], double p[11]) {
  for (int k = 0; k < 11; ++k) p[k] = 0.0;
  for (int r = 0; r < 3; ++r) {
    const int i = (r + 1) % 3, j = (r + 2) % 3;
    double C[7] = {0, 0, 0, 0, 0, 0, 0};   // bx_i by_j - bx_j by_i
    for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) C[a + b] += B[i][0][a] * B[j][1][b] - B[j][0][a] * B[i][1][b];
    for (int a = 0; a < 7; ++a) for (int b = 0; b < 5; ++b) p[a + b] += C[a] * B[r][2][b];
  }
}
// the real roots of a degree-10 polynomial in [-1, 1], ascending: the roots of each derivative bracket those of the one above it
// (hyp_detail::poly_bisect, its fixed kBisections halvings per bracket)
inline int fp_roots_unit(const double p[11], double roots[10], int newton = kFiveNewton) {
  double c[11][11], edge[12], next[12];
  for (int k = 0; k < 11; ++k) c[10][k] = p[k];
  for (int d = 10; d >= 2; --d) for (int k = 0; k < d; ++k) c[d - 1][k] = (k + 1) * c[d][k + 1];
  edge[0] = -1.0; edge[1] = 1.0;
  int count = 0;
  for (int d = 1; d <= 10; ++d) {
    next[0] = -1.0;
    for (int i = 0; i < d; ++i) {
      const bool found = hyp_detail::poly_bisect(c[d], d, edge[i], edge[i + 1], &next[i + 1]);
      if (d < 10 || !found) continue;
      double t = next[i + 1];
      for (int it = 0; it < newton; ++it) {   // Newton on the polynomial, a step taken only while it stays inside [-1, 1]
        const double tn = t - hyp_detail::poly_eval(c[10], 10, t) / hyp_detail::poly_eval(c[9], 9, t);
        if (tn >= -1.0 && tn <= 1.0) t = tn;
      }
      roots[count++] = t;
    }
    next[d + 1] = 1.0;
    for (int i = 0; i <= d + 1; ++i) edge[i] = next[i];
  }
  return count;
}
// Gauss-Newton steps on the ten cubics themselves, in (x, y, z): the eliminant's coefficients went through an elimination and a 3 x 3
// determinant of polynomials, the cubics are evaluated from the null space directly — r0 = det E, r(1 + 3i + c) = (2 E E^T E - tr(E E^T) E)_ic,
// the Jacobian from the directional derivatives along N0, N1, N2, the 3 x 3 normal equations solved by cofactors.  A step that is not
// finite ends the polish.
inline void fp_polish(const double N[4][9], double v[3], int steps) {
  for (int it = 0; it < steps; ++it) {
    double E[9], G[3][3], r[10], J[10][3];
    for (int m = 0; m < 9; ++m) E[m] = v[0] * N[0][m] + v[1] * N[1][m] + v[2] * N[2][m] + N[3][m];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) G[i][j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
    const double tr = G[0][0] + G[1][1] + G[2][2];
    const double cof[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                           E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                           E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
    r[0] = E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2];
    for (int i = 0; i < 3; ++i) for (int c = 0; c < 3; ++c)
      r[1 + 3 * i + c] = 2.0 * (G[i][0] * E[c] + G[i][1] * E[3 + c] + G[i][2] * E[6 + c]) - tr * E[3 * i + c];
    for (int d = 0; d < 3; ++d) {
      const double* D = N[d];
      double dG[3][3], dtr = 0.0, dd = 0.0;
      for (int m = 0; m < 9; ++m) { dtr += E[m] * D[m]; dd += cof[m] * D[m]; }
      dtr *= 2.0;
      J[0][d] = dd;
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j)
        dG[i][j] = D[3 * i] * E[3 * j] + D[3 * i + 1] * E[3 * j + 1] + D[3 * i + 2] * E[3 * j + 2] + E[3 * i] * D[3 * j] + E[3 * i + 1] * D[3 * j + 1] + E[3 * i + 2] * D[3 * j + 2];
      for (int i = 0; i < 3; ++i) for (int c = 0; c < 3; ++c)
        J[1 + 3 * i + c][d] = 2.0 * (dG[i][0] * E[c] + dG[i][1] * E[3 + c] + dG[i][2] * E[6 + c] + G[i][0] * D[c] + G[i][1] * D[3 + c] + G[i][2] * D[6 + c])
                              - dtr * E[3 * i + c] - tr * D[3 * i + c];
    }
    double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};   // J^T J: 00 01 02 11 12 22
    for (int k = 0; k < 10; ++k) {
      A[0] += J[k][0] * J[k][0]; A[1] += J[k][0] * J[k][1]; A[2] += J[k][0] * J[k][2]; A[3] += J[k][1] * J[k][1]; A[4] += J[k][1] * J[k][2]; A[5] += J[k][2] * J[k][2];
      b[0] += J[k][0] * r[k]; b[1] += J[k][1] * r[k]; b[2] += J[k][2] * r[k];
    }
    const double c00 = A[3] * A[5] - A[4] * A[4], c01 = A[2] * A[4] - A[1] * A[5], c02 = A[1] * A[4] - A[2] * A[3];
    const double c11 = A[0] * A[5] - A[2] * A[2], c12 = A[1] * A[2] - A[0] * A[4], c22 = A[0] * A[3] - A[1] * A[1];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    const double s0 = (c00 * b[0] + c01 * b[1] + c02 * b[2]) / det, s1 = (c01 * b[0] + c11 * b[1] + c12 * b[2]) / det, s2 = (c02 * b[0] + c12 * b[1] + c22 * b[2]) / det;
    if (!std::isfinite(s0 + s1 + s2)) return;
    v[0] -= s0; v[1] -= s1; v[2] -= s2;
  }
}
// (x, y) of a root z from the two rows of B(z) whose 2 x 2 minor in (x, y) is largest, the polish, E = x N0 + y N1 + z N2 + N3 scaled to
// unit Frobenius norm and signed; false: not finite
inline bool fp_solution(const double N[4][9], const double B[3][3][5], double z, double E[9], int polish = kFivePolish) {
  double b[3][3];
  for (int r = 0; r < 3; ++r) for (int v = 0; v < 3; ++v) b[r][v] = hyp_detail::poly_eval(B[r][v], 4, z);
  const double C[3] = {b[1][0] * b[2][1] - b[2][0] * b[1][1], b[2][0] * b[0][1] - b[0][0] * b[2][1], b[0][0] * b[1][1] - b[1][0] * b[0][1]};
  int k = 0;
  for (int r = 1; r < 3; ++r) if (std::fabs(C[r]) > std::fabs(C[k])) k = r;
  const int i = (k + 1) % 3, j = (k + 2) % 3;
  const double x = (b[i][1] * b[j][2] - b[i][2] * b[j][1]) / C[k], y = (b[i][2] * b[j][0] - b[i][0] * b[j][2]) / C[k];
  double v[3] = {x, y, z}, fro = 0.0;
  fp_polish(N, v, polish);
  for (int m = 0; m < 9; ++m) { E[m] = v[0] * N[0][m] + v[1] * N[1][m] + v[2] * N[2][m] + N[3][m]; fro += E[m] * E[m]; }
  fro = std::sqrt(fro);
  for (int m = 0; m < 9; ++m) E[m] /= fro;
  return signed_finite(E);
}
// the key the solutions are ordered by: |sum_k (k + 1) E[k]|, a fixed linear form with nine different weights — free of E's sign and of the
// null-space basis (which the roots z are not), and not zero or equal for two solutions just because the motion is along an axis
inline double fp_key(const double E[9]) {
  double s = 0.0;
  for (int k = 0; k < 9; ++k) s += (k + 1) * E[k];
  return std::fabs(s);
}
// every essential matrix of exactly five correspondences idx[0..5): E[s] for s < *count, ascending fp_key (the order of the roots where
// two are equal); false: declined (E and *count untouched).  trace_factor, transpose, newton (which also switches the polish): the seeded
// errors of the tests.
inline bool five_point(const double* na, const double* nb, const int32_t* idx, double E[10][9], int* count, FivePointDiag* diag = nullptr,
                       double trace_factor = 0.5, bool transpose = false, int newton = kFiveNewton) {
  const int polish = newton > 0 ? kFivePolish : 0;
  for (int i = 0; i < 5; ++i) for (int k = i + 1; k < 5; ++k) if (idx[i] == idx[k]) return false;
  double a[5][9], N[4][9], M[10][20], B[3][3][5], p[11], q[11], roots[10], sol[10][9], key[10];
  for (int i = 0; i < 5; ++i) {
    const size_t j = 2 * (size_t)idx[i];
    const double xa = na[j], ya = na[j + 1], xb = nb[j], yb = nb[j + 1];
    const double r[9] = {xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, 1.0};
    for (int k = 0; k < 9; ++k) a[i][k] = transpose ? r[3 * (k % 3) + k / 3] : r[k];
  }
  if (!fp_null_space(a, N, diag)) return false;
  fp_constraints(N, M, trace_factor);
  if (!fp_eliminate(M, diag)) return false;
  fp_reduce(M, B);
  fp_eliminant(B, p);
  for (int k = 0; k < 11; ++k) q[k] = p[10 - k];   // the roots with |z| > 1 are those of the reversed polynomial in 1 / z
  int ns = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const int nr = fp_roots_unit(pass ? q : p, roots, newton);
    for (int s = 0; s < nr; ++s) {
      if (pass && (roots[s] == 1.0 || roots[s] == -1.0)) continue;   // (|z| = 1 belongs to the first pass)
      if (ns == 10) break;                                            // (a root within rounding of |z| = 1 seen by both passes)
      if (!fp_solution(N, B, pass ? 1.0 / roots[s] : roots[s], sol[ns], polish)) return false;
      ++ns;
    }
  }
  if (ns == 0) return false;
  for (int s = 0; s < ns; ++s) key[s] = fp_key(sol[s]);
  for (int s = 0; s < ns; ++s) {
    int rank = 0;
    for (int o = 0; o < ns; ++o) if (key[o] < key[s] || (key[o] == key[s] && o < s)) ++rank;
    for (int m = 0; m < 9; ++m) E[rank][m] = sol[s][m];
  }
  *count = ns;
  return true;
}

// the chain per subset: every solution scored, the one with the most inliers kept, ties to the most in front (of its winning candidate),
// then to the first; false: declined (no solution, or none that score() accepts)
inline bool five_point_hypothesis(const double* na, const double* nb, int n, const int32_t* idx, double f2, double thr2, double E[9], double pose[6],
                                  int32_t* num_inliers, int32_t num_front[4], int* num_solutions = nullptr, int* chosen = nullptr) {
  double sol[10][9];
  int ns = 0, best = -1;
  int32_t best_inl = 0, best_front = 0;
  *num_inliers = 0;
  for (int c = 0; c < 4; ++c) num_front[c] = 0;
  if (num_solutions) *num_solutions = 0;
  if (!five_point(na, nb, idx, sol, &ns)) return false;
  if (num_solutions) *num_solutions = ns;
  for (int s = 0; s < ns; ++s) {
    int32_t inl, front[4];
    double ps[6];
    if (!score(na, nb, n, sol[s], f2, thr2, &inl, front, ps)) continue;
    int32_t most = front[0];
    for (int c = 1; c < 4; ++c) if (front[c] > most) most = front[c];
    if (best >= 0 && (inl < best_inl || (inl == best_inl && most <= best_front))) continue;
    best = s; best_inl = inl; best_front = most;
    *num_inliers = inl;
    for (int c = 0; c < 4; ++c) num_front[c] = front[c];
    for (int k = 0; k < 6; ++k) pose[k] = ps[k];
    for (int k = 0; k < 9; ++k) E[k] = sol[s][k];
  }
  if (chosen) *chosen = best;
  return best >= 0;
}

}  // namespace epi_detail

struct TwoViewOptions {
  int iterations = 1000;
  double threshold_px = 4.0;
  int refits = 3;
  int min_inliers = 16;
  uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
  bool hypotheses_on_device = true;   // false: the same loop from the host definitions above (what the tests compare with; no session-level code takes it)
  // what a subset is and how it is solved: eight correspondences by eight_point, or five by five_point (every solution scored, the best
  // kept per subset).  The refits are eight-point fits over the current inliers either way.
  enum class EssentialSolver { EightPoint, FivePoint } solver = EssentialSolver::EightPoint;
};

struct TwoViewResult {
  bool ok = false;
  double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double pose_b[6] = {0, 0, 0, 0, 0, 0};   // camera B in A's frame, unit baseline
  int num_inliers = 0;                     // Sampson inliers of E
  int num_front = 0;                       // those of them in front of both cameras for the chosen candidate
  int winner_task = -1, refits_adopted = 0;
  std::vector<uint8_t> inliers;            // [n]
};

namespace epi_detail {
// The RANSAC loop over a backend: hypotheses(subsets, m, tasks, E, poses, status, num_inliers, num_front) fills the arrays of `tasks` tasks
// (m = 5: five-point subsets, which only the first call passes; m >= 8: eight-point), inlier_mask(E, mask) the flags [n] of one matrix.
template <class Hypotheses, class InlierMask>
inline TwoViewResult ransac(int n, const TwoViewOptions& opt, Hypotheses&& hypotheses, InlierMask&& inlier_mask) {
  TwoViewResult res;
  res.inliers.assign((size_t)(n > 0 ? n : 0), 0);
  if (n < 8 || opt.iterations <= 0) return res;
  const int T = opt.iterations;
  const int m = opt.solver == TwoViewOptions::EssentialSolver::FivePoint ? 5 : 8;
  const std::vector<int32_t> subsets = hyp_detail::distinct_subsets(n, m, T, opt.rng_state);
  std::vector<double> E((size_t)T * 9), poses((size_t)T * 6);
  std::vector<uint8_t> status((size_t)T);
  std::vector<int32_t> inl((size_t)T), front((size_t)T * 4);
  hypotheses(subsets.data(), m, T, E.data(), poses.data(), status.data(), inl.data(), front.data());
  int best = -1;
  // five-point subsets: a tie in inliers goes to the hypothesis with more of them in front, as within a subset — a scene plane gives its
  // twin motion the same inliers and only the cheirality tells the two apart; then (and for eight-point subsets at once) to the lowest task
  auto most_front = [&](int t) { int32_t b = front[(size_t)t * 4]; for (int c = 1; c < 4; ++c) if (front[(size_t)t * 4 + c] > b) b = front[(size_t)t * 4 + c]; return b; };
  for (int t = 0; t < T; ++t) {
    if (status[(size_t)t] == 0) continue;
    if (best < 0 || inl[(size_t)t] > inl[(size_t)best] || (m == 5 && inl[(size_t)t] == inl[(size_t)best] && most_front(t) > most_front(best))) best = t;
  }
  if (best < 0) return res;
  res.winner_task = best;
  int32_t cur_inl = inl[(size_t)best], cur_front[4];
  for (int k = 0; k < 9; ++k) res.E[k] = E[(size_t)best * 9 + k];
  for (int k = 0; k < 6; ++k) res.pose_b[k] = poses[(size_t)best * 6 + k];
  for (int c = 0; c < 4; ++c) cur_front[c] = front[(size_t)best * 4 + c];
  inlier_mask(res.E, res.inliers.data());
  for (int round = 0; round < opt.refits; ++round) {
    std::vector<int32_t> idx;
    for (int i = 0; i < n; ++i) if (res.inliers[(size_t)i]) idx.push_back(i);
    if (idx.size() < 8) break;
    double e2[9], p2[6]; uint8_t st = 0; int32_t inl2 = 0, front2[4] = {0, 0, 0, 0};
    hypotheses(idx.data(), (int)idx.size(), 1, e2, p2, &st, &inl2, front2);
    if (!st || inl2 < cur_inl) break;   // not adopted: the next round would refit the same set
    cur_inl = inl2;
    for (int k = 0; k < 9; ++k) res.E[k] = e2[k];
    for (int k = 0; k < 6; ++k) res.pose_b[k] = p2[k];
    for (int c = 0; c < 4; ++c) cur_front[c] = front2[c];
    inlier_mask(res.E, res.inliers.data());
    ++res.refits_adopted;
  }
  int cand = 0;
  for (int c = 1; c < 4; ++c) if (cur_front[c] > cur_front[cand]) cand = c;
  res.num_inliers = cur_inl;
  res.num_front = cur_front[cand];
  res.ok = res.num_front >= opt.min_inliers;
  return res;
}

// the loop from the host definitions alone: what the device path is compared with
inline TwoViewResult host_ransac(const float* xy_a, const float* xy_b, int n, const double cam_a[NUM_CAM_PARAMS], const double cam_b[NUM_CAM_PARAMS],
                                 const TwoViewOptions& opt) {
  if (n < 8) return ransac(n, opt, [](auto&&...) {}, [](auto&&...) {});
  const std::vector<double> na = hyp_detail::normalised_points(cam_a, xy_a, n), nb = hyp_detail::normalised_points(cam_b, xy_b, n);
  const double f2 = mean_focal2(cam_a, cam_b), thr2 = opt.threshold_px * opt.threshold_px;
  return ransac(n, opt,
    [&](const int32_t* sub, int m, int tasks, double* E, double* poses, uint8_t* status, int32_t* inl, int32_t* front) {
      for (int t = 0; t < tasks; ++t) {
        double e[9];
        if (m == 5) status[t] = five_point_hypothesis(na.data(), nb.data(), n, sub + (size_t)t * m, f2, thr2, e, poses + 6 * (size_t)t, &inl[t], &front[4 * (size_t)t]) ? 1 : 0;
        else status[t] = eight_point(na.data(), nb.data(), sub + (size_t)t * m, m, e) &&
                    score(na.data(), nb.data(), n, e, f2, thr2, &inl[t], &front[4 * (size_t)t], poses + 6 * (size_t)t) ? 1 : 0;
        if (status[t]) for (int k = 0; k < 9; ++k) E[9 * (size_t)t + k] = e[k];
        else { inl[t] = 0; for (int c = 0; c < 4; ++c) front[4 * (size_t)t + c] = 0; }
      }
    },
    [&](const double E[9], uint8_t* mask) {
      for (int i = 0; i < n; ++i)
        mask[i] = sampson_inlier(E, na[2 * (size_t)i], na[2 * (size_t)i + 1], nb[2 * (size_t)i], nb[2 * (size_t)i + 1], f2, thr2) ? 1 : 0;
    });
}
}  // namespace epi_detail

// RANSAC over eight-point hypotheses: `iterations` subsets from hyp_detail::distinct_subsets(n, 8, ...), all scored in one device call
// (rsba_epipolar_hypotheses); the most inliers win, ties go to the lowest task.  With opt.solver = FivePoint the subsets are
// distinct_subsets(n, 5, ...) and the call is rsba_epipolar_hypotheses_five_point, which hands back each subset's best solution; a tie in
// inliers between subsets then goes to the one with more of them in front before it goes to the lowest task, and the rest of the loop is
// the same (n >= 8 still: the refits are eight-point fits).  Then up to `refits` rounds of "eight-point over the current
// inliers (one task, m = their number), recount", a refit adopted only when its count is not lower.  ok iff the final inliers in front of
// both cameras number at least min_inliers.  xy_a / xy_b [n][2] are pixel coordinates (float, as everywhere in solve_rs_pnp.hpp).
inline TwoViewResult findEssentialRansac(const float* xy_a, const float* xy_b, int n, const double cam_a[NUM_CAM_PARAMS], const double cam_b[NUM_CAM_PARAMS],
                                         const TwoViewOptions& opt = TwoViewOptions(), int device = 0) {
  if (!opt.hypotheses_on_device) return epi_detail::host_ransac(xy_a, xy_b, n, cam_a, cam_b, opt);
  return epi_detail::ransac(n, opt,
    [&](const int32_t* sub, int m, int tasks, double* E, double* poses, uint8_t* status, int32_t* inl, int32_t* front) {
      if (m == 5) hyp_detail::check(rsba_epipolar_hypotheses_five_point(device, cam_a, cam_b, xy_a, xy_b, n, sub, tasks, opt.threshold_px, E, poses, status, inl, front, nullptr));
      else hyp_detail::check(rsba_epipolar_hypotheses(device, cam_a, cam_b, xy_a, xy_b, n, sub, m, tasks, opt.threshold_px, E, poses, status, inl, front));
    },
    [&](const double E[9], uint8_t* mask) { hyp_detail::check(rsba_epipolar_inliers(device, cam_a, cam_b, xy_a, xy_b, n, E, opt.threshold_px, mask)); });
}

// ---- geometric verification: the same RANSAC for many frame pairs in one device call (rsba_amd.h: rsba_epipolar_ransac_pairs) ----
// One pair's correspondences and cameras; the arrays stay the caller's.
struct EssentialPair {
  const float* xy_a = nullptr;   // [n][2] pixels in frame A
  const float* xy_b = nullptr;   // [n][2] pixels in frame B
  int n = 0;
  const double* cam_a = nullptr; // [NUM_CAM_PARAMS]
  const double* cam_b = nullptr;
};

// The arrays of a batched call (rsba_epipolar_ransac_pairs, rsba_two_view_classify_pairs) from the pairs: the cameras by value, each once
// (the call normalises a run of pairs that share a camera in one launch), the offsets, the concatenated points, and for every pair of at
// least min_n correspondences its subsets distinct_subsets(n_p, m, T, rng_state) — the draw a single-pair call makes for that pair alone; a
// smaller pair is an empty result and the call does not read its subsets.
struct PairArrays {
  std::vector<double> cams;                // [num_cams][NUM_CAM_PARAMS]
  std::vector<int32_t> cam_a, cam_b;       // [P] indices into cams
  std::vector<int32_t> offset;             // [P + 1]
  std::vector<float> xy_a, xy_b;           // [offset[P]][2] (two zeros where every pair is empty: the call still wants arrays)
  std::vector<int32_t> subsets;            // [P][T][m]
  int32_t num_cams() const { return (int32_t)(cams.size() / NUM_CAM_PARAMS); }
};
inline PairArrays pair_arrays(const std::vector<EssentialPair>& pairs, int min_n, int m, int T, uint64_t rng_state) {
  const size_t P = pairs.size();
  PairArrays A;
  auto cam_index = [&](const double* cam) {
    for (size_t c = 0; c * NUM_CAM_PARAMS < A.cams.size(); ++c)
      if (std::memcmp(&A.cams[c * NUM_CAM_PARAMS], cam, NUM_CAM_PARAMS * sizeof(double)) == 0) return (int32_t)c;
    A.cams.insert(A.cams.end(), cam, cam + NUM_CAM_PARAMS);
    return A.num_cams() - 1;
  };
  A.cam_a.resize(P); A.cam_b.resize(P); A.offset.assign(P + 1, 0); A.subsets.assign(P * (size_t)T * m, 0);
  for (size_t p = 0; p < P; ++p) {
    const EssentialPair& q = pairs[p];
    const int n = q.n > 0 ? q.n : 0;
    A.cam_a[p] = cam_index(q.cam_a); A.cam_b[p] = cam_index(q.cam_b);
    A.offset[p + 1] = A.offset[p] + n;
    A.xy_a.insert(A.xy_a.end(), q.xy_a, q.xy_a + 2 * (size_t)n); A.xy_b.insert(A.xy_b.end(), q.xy_b, q.xy_b + 2 * (size_t)n);
    if (n < min_n) continue;
    const std::vector<int32_t> s = hyp_detail::distinct_subsets(n, m, T, rng_state);
    std::copy(s.begin(), s.end(), A.subsets.begin() + (std::ptrdiff_t)(p * (size_t)T * m));
  }
  if (A.xy_a.empty()) { A.xy_a.assign(2, 0.0f); A.xy_b.assign(2, 0.0f); }
  return A;
}

// findEssentialRansac for every pair, result p what findEssentialRansac(pairs[p]..., opt, device) returns: pair p's subsets are
// distinct_subsets(n_p, m, opt.iterations, opt.rng_state), the draw the single call makes for that pair alone, and the loop per pair is
// epi_detail::ransac, kept on the device by rsba_epipolar_ransac_pairs — one upload, one download, the hypothesis kernels launched over the
// subsets of all pairs at once.  hypotheses_on_device == false: epi_detail::host_ransac per pair.  max_tasks_per_launch: the C call's (0: its default).
inline std::vector<TwoViewResult> findEssentialRansacPairs(const std::vector<EssentialPair>& pairs, const TwoViewOptions& opt = TwoViewOptions(), int device = 0,
                                                           int max_tasks_per_launch = 0) {
  std::vector<TwoViewResult> out(pairs.size());
  if (!opt.hypotheses_on_device) {
    for (size_t p = 0; p < pairs.size(); ++p) out[p] = epi_detail::host_ransac(pairs[p].xy_a, pairs[p].xy_b, pairs[p].n, pairs[p].cam_a, pairs[p].cam_b, opt);
    return out;
  }
  for (size_t p = 0; p < pairs.size(); ++p) out[p].inliers.assign((size_t)(pairs[p].n > 0 ? pairs[p].n : 0), 0);
  if (pairs.empty() || opt.iterations <= 0) return out;
  const int T = opt.iterations, m = opt.solver == TwoViewOptions::EssentialSolver::FivePoint ? 5 : 8;
  const size_t P = pairs.size();
  const PairArrays A = pair_arrays(pairs, 8, m, T, opt.rng_state);
  const std::vector<int32_t>& offset = A.offset;
  std::vector<double> E(P * 9, 0.0), poses(P * 6, 0.0);
  std::vector<uint8_t> status(P, 0), mask((size_t)offset[P] + 1, 0);
  std::vector<int32_t> winner(P, -1), adopted(P, 0), inl(P, 0), front(P * 4, 0);
  hyp_detail::check(rsba_epipolar_ransac_pairs(device, A.cams.data(), A.num_cams(), A.cam_a.data(), A.cam_b.data(), offset.data(), (int32_t)P, A.xy_a.data(), A.xy_b.data(),
                                               A.subsets.data(), m, T, opt.threshold_px, opt.refits, max_tasks_per_launch, E.data(), poses.data(), status.data(), winner.data(),
                                               adopted.data(), inl.data(), front.data(), mask.data()));
  for (size_t p = 0; p < P; ++p) {
    TwoViewResult& r = out[p];
    if (!status[p]) continue;
    for (int k = 0; k < 9; ++k) r.E[k] = E[p * 9 + k];
    for (int k = 0; k < 6; ++k) r.pose_b[k] = poses[p * 6 + k];
    r.winner_task = winner[p]; r.refits_adopted = adopted[p]; r.num_inliers = inl[p];
    int cand = 0;
    for (int c = 1; c < 4; ++c) if (front[p * 4 + c] > front[p * 4 + cand]) cand = c;
    r.num_front = front[p * 4 + cand];
    r.ok = r.num_front >= opt.min_inliers;
    std::copy(mask.begin() + offset[p], mask.begin() + offset[p + 1], r.inliers.begin());
  }
  return out;
}

// What verifyMatches found for one frame pair.
struct PairReport {
  int32_t frameA = 0, frameB = 0;
  int correspondences = 0;                 // the refs of frame B's observations into frame A
  bool ok = false;                         // TwoViewResult::ok of the pair
  int num_inliers = 0, num_front = 0;
  double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double pose_b[6] = {0, 0, 0, 0, 0, 0};   // camera B in A's frame, unit baseline
  int removed = 0;                         // refs erased from frame B's observations
};
struct VerifyOptions {
  bool drop_unverified = false;   // true: a pair that is not ok (under 8 correspondences, or no accepted geometry) loses all its refs
  int max_tasks_per_launch = 0;   // rsba_epipolar_ransac_pairs' (0: its default)
};

// Geometric verification of the matches of a session, between matchSession and createTracks / initializeTwoView: every frame B and every
// earlier frame A that B's matches reach make a pair, whose correspondences are all refs of B's observations into A — in observation
// order, then in the order of an observation's list; cameras f.cam if set, else sess.cam.  All pairs go through findEssentialRansacPairs
// (one batched device call, or as many launches as its chunking needs).  Of a pair whose result is ok, the refs flagged as outliers are
// erased from Observation::matches; a pair that is not ok is left as it is unless drop_unverified.  Nothing but `matches` is touched; refs
// to later frames, to the frame itself or out of range are neither verified nor erased.  The rule is a global-shutter approximation of a
// rolling-shutter pair (rsba_amd.h): widen tv.threshold_px for such sessions.  Reports in the order (frameB, frameA) ascending.
inline std::vector<PairReport> verifyMatches(Session& sess, const TwoViewOptions& tv = TwoViewOptions(), int device = 0, const VerifyOptions& vo = VerifyOptions()) {
  struct Ref { size_t obs, slot; };
  struct Found { std::vector<Ref> refs; std::vector<float> xa, xb; };
  std::vector<PairReport> reports;
  std::vector<Found> found;
  for (size_t fb = 0; fb < sess.frames.size(); ++fb) {
    const Frame& B = sess.frames[fb];
    std::map<int32_t, Found> reached;   // (ascending frame A)
    for (size_t oi = 0; oi < B.obs.size(); ++oi)
      for (size_t ri = 0; ri < B.obs[oi].matches.size(); ++ri) {
        const ObservationRef& ref = B.obs[oi].matches[ri];
        if (ref.frame < 0 || (size_t)ref.frame >= fb || ref.obs < 0 || (size_t)ref.obs >= sess.frames[(size_t)ref.frame].obs.size()) continue;
        const Observation& oa = sess.frames[(size_t)ref.frame].obs[(size_t)ref.obs];
        Found& f = reached[ref.frame];
        f.refs.push_back(Ref{oi, ri});
        f.xa.push_back((float)oa.x); f.xa.push_back((float)oa.y); f.xb.push_back((float)B.obs[oi].x); f.xb.push_back((float)B.obs[oi].y);
      }
    for (auto& kv : reached) {
      PairReport r;
      r.frameA = kv.first; r.frameB = (int32_t)fb; r.correspondences = (int)kv.second.refs.size();
      reports.push_back(r);
      found.push_back(std::move(kv.second));
    }
  }
  std::vector<EssentialPair> pairs(reports.size());
  for (size_t p = 0; p < reports.size(); ++p) {
    const Frame& A = sess.frames[(size_t)reports[p].frameA];
    const Frame& B = sess.frames[(size_t)reports[p].frameB];
    pairs[p].xy_a = found[p].xa.data(); pairs[p].xy_b = found[p].xb.data(); pairs[p].n = reports[p].correspondences;
    pairs[p].cam_a = A.__isset.cam ? A.cam.data() : sess.cam.data();
    pairs[p].cam_b = B.__isset.cam ? B.cam.data() : sess.cam.data();
  }
  const std::vector<TwoViewResult> results = findEssentialRansacPairs(pairs, tv, device, vo.max_tasks_per_launch);
  std::vector<std::tuple<size_t, size_t, size_t>> erase;   // (frame B, observation, slot)
  for (size_t p = 0; p < reports.size(); ++p) {
    PairReport& r = reports[p];
    const TwoViewResult& res = results[p];
    r.ok = res.ok; r.num_inliers = res.num_inliers; r.num_front = res.num_front;
    for (int k = 0; k < 9; ++k) r.E[k] = res.E[k];
    for (int k = 0; k < 6; ++k) r.pose_b[k] = res.pose_b[k];
    if (!res.ok && !vo.drop_unverified) continue;
    for (size_t i = 0; i < found[p].refs.size(); ++i) {
      if (res.ok && res.inliers[i]) continue;
      erase.push_back(std::make_tuple((size_t)r.frameB, found[p].refs[i].obs, found[p].refs[i].slot));
      ++r.removed;
    }
  }
  // an observation's list holds refs of several pairs: all of them erased from the back, so that the slots in front keep their numbers
  std::sort(erase.begin(), erase.end());
  for (size_t i = erase.size(); i-- > 0;) {
    std::vector<ObservationRef>& list = sess.frames[std::get<0>(erase[i])].obs[std::get<1>(erase[i])].matches;
    list.erase(list.begin() + (std::ptrdiff_t)std::get<2>(erase[i]));
  }
  return reports;
}

// The pair to start a reconstruction from: the ok pair with the most inliers in front of both cameras; ties go to the lowest frameB, then
// the lowest frameA.  -1: no pair is ok.
inline int pickBootstrapPair(const std::vector<PairReport>& reports) {
  int best = -1;
  for (size_t p = 0; p < reports.size(); ++p) {
    const PairReport& r = reports[p];
    if (!r.ok) continue;
    if (best >= 0) {
      const PairReport& b = reports[(size_t)best];
      if (r.num_front < b.num_front) continue;
      if (r.num_front == b.num_front && (r.frameB > b.frameB || (r.frameB == b.frameB && r.frameA >= b.frameA))) continue;
    }
    best = (int)p;
  }
  return best;
}

namespace epi_detail {
// the pose of a camera that sees x = R_rel x_A + t_rel, where camera A has pose_a: x = R_rel R_A (X - c_A) + t_rel
inline bool compose_pose(const double pose_a[6], const double rel[6], double out[6]) {
  double rvec[3], tvec[3], R[9];
  hyp_detail::from_pose(rel, rvec, tvec);
  for (int k = 0; k < 3; ++k) {
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double ra[3], rb[3];
    hyp_detail::rotate(pose_a, e, ra);
    hyp_detail::rotate(rvec, ra, rb);
    for (int r = 0; r < 3; ++r) R[3 * r + k] = rb[r];
  }
  for (int r = 0; r < 3; ++r) tvec[r] -= R[3 * r] * pose_a[3] + R[3 * r + 1] * pose_a[4] + R[3 * r + 2] * pose_a[5];
  return hyp_detail::pose_from_rt(R, tvec, out);
}
}  // namespace epi_detail

// Poses for two frames that have none (frame A may have them already): the essential-matrix RANSAC over the matches of frame B that
// reach frame A, frame A at the origin (zero poses: two in a rolling-shutter session, else one, as CeresHandler::Add starts frame 0) or
// where it is, frame B at the recovered relative pose composed onto A's poses[0] — both pose slots the same in a rolling-shutter session,
// the global-shutter approximation the GS PnP attempts of new_frame.hpp also start from.  Then createTracks(frameB) and, for neighbouring
// frames and baIterations > 0, BA(frameA, frameB, reproject), whose verdict (a usable solution) is then the return value.  false otherwise:
// fewer than 8 correspondences or no accepted geometry — the session is left untouched.  Requires frameA < frameB (matches live on the later frame) and a frame B without poses.
// createTracks refuses a match into a frame without poses, as the reference does: every frame that frame B's matches reach must have poses
// by then, so match a bootstrap pair against each other (and against frames that are already posed) only.
struct TwoViewReport { int correspondences = 0, num_inliers = 0, num_front = 0; };
inline bool initializeTwoView(Session& sess, const int32_t frameA, const int32_t frameB, const SfmOptions& opt, const TwoViewOptions& tv = TwoViewOptions(),
                              int device = 0, bool progress = true, const int32_t baIterations = 20, TwoViewReport* report = nullptr) {
  if (frameA < 0 || frameA >= frameB || (size_t)frameB >= sess.frames.size()) throw std::invalid_argument("initializeTwoView: 0 <= frameA < frameB < frames");
  Frame& fa = sess.frames[(size_t)frameA];
  Frame& fb = sess.frames[(size_t)frameB];
  if (fb.__isset.poses && !fb.poses.empty()) throw std::invalid_argument("initializeTwoView: frame B has poses");
  std::vector<float> xa, xb;
  for (const Observation& o : fb.obs)
    for (const ObservationRef& ref : o.matches) {
      if (ref.frame != frameA) continue;
      const Observation& o2 = fa.obs[(size_t)ref.obs];
      xa.push_back((float)o2.x); xa.push_back((float)o2.y); xb.push_back((float)o.x); xb.push_back((float)o.y);
      break;
    }
  const int n = (int)(xa.size() / 2);
  if (report) { *report = TwoViewReport(); report->correspondences = n; }
  if (n < 8) return false;
  const double* cam_a = fa.__isset.cam ? fa.cam.data() : sess.cam.data();
  const double* cam_b = fb.__isset.cam ? fb.cam.data() : sess.cam.data();
  const TwoViewResult res = findEssentialRansac(xa.data(), xb.data(), n, cam_a, cam_b, tv, device);
  if (report) { report->num_inliers = res.num_inliers; report->num_front = res.num_front; }
  if (!res.ok) return false;
  const size_t slots = opt.model.rolling_shutter ? 2 : 1;
  std::vector<double> pose(res.pose_b, res.pose_b + NUM_POSE_PARAMS);
  if (fa.__isset.poses && !fa.poses.empty()) {
    if (!epi_detail::compose_pose(fa.poses[0].data(), res.pose_b, pose.data())) return false;
  } else {
    fa.poses.assign(slots, std::vector<double>(NUM_POSE_PARAMS, 0.0));
    fa.__isset.poses = true;
  }
  fb.poses.assign(slots, pose);
  fb.__isset.poses = true;
  createTracks(sess, (size_t)frameB, opt, device);
  if (baIterations > 0 && frameB == frameA + 1) return BA(sess, frameA, frameB, opt, baIterations, nullptr, progress, nullptr, true);
  return true;
}

}  // namespace rsba_amd
