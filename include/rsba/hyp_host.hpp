// What the host forms of the hypothesis generators share (solve_rs_pnp.hpp: DLT and P3P start poses; two_view.hpp: eight-point and
// five-point essential matrices; new_frame.hpp: the sampled refinements), once: the glue around a batch of RANSAC tasks, the conversions
// between rvec / tvec and rsba's 6-vector, the cyclic Jacobi eigen-solver, the bisection of a monotonic polynomial, Hartley's normalisation
// and the null vector of a 9-unknown Gram matrix.  The host counterpart of rsba_amd/csrc/hyp_math.hpp, which restates part of this for the
// device kernels; the two are separate texts on purpose (sharing one changes how the device compiler fuses operations), and the tests hold
// both to an extended-precision reference.  These functions are part of the DEFINITION of the hypotheses: the order of their floating-point
// operations is what the host programs under tests/ print and the kernels are compared with.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "session.hpp"

extern "C" {
#include "../rsba_amd.h"
}

namespace rsba_amd {

namespace hyp_detail {

// ---- glue around a batch of tasks ----
inline void check(int32_t st) {
  if (st != RSBA_OK) throw std::runtime_error(std::string(rsba_status_string(st)) + ": " + rsba_last_error());
}

// cv::RNG (OpenCV core, restated): multiply-with-carry, uniform(a, b) = a + next() % (b - a)
struct Rng {
  uint64_t state;
  explicit Rng(uint64_t s = 0xffffffffULL) : state(s ? s : 0xffffffffULL) {}
  unsigned next() { state = (uint64_t)(unsigned)state * 4164903690ULL + (unsigned)(state >> 32); return (unsigned)state; }
  int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

// the subsets of every RANSAC here but solveRsPnPRansac's own: m distinct indices below n per iteration, from cv::RNG's generator
inline std::vector<int32_t> distinct_subsets(int n, int m, int iterations, uint64_t rng_state) {
  Rng gen(rng_state);
  std::vector<int32_t> out((size_t)iterations * m);
  for (int it = 0; it < iterations; ++it)
    for (int k = 0; k < m;) {
      const int c = gen.uniform(0, n); bool dup = false;
      for (int j = 0; j < k; ++j) dup = dup || out[(size_t)it * m + j] == c;
      if (!dup) out[(size_t)it * m + k++] = c;
    }
  return out;
}
// 0 .. n-1: the subset that is every point
inline std::vector<int32_t> all_indices(int n) {
  std::vector<int32_t> all((size_t)n);
  for (int i = 0; i < n; ++i) all[(size_t)i] = i;
  return all;
}
// the winner of a batch: the first task with the most inliers among those whose status `accepted` lets through; -1: none
template <class Accepted>
inline int most_inliers(const uint8_t* status, const int32_t* count, int tasks, Accepted&& accepted) {
  int best = -1;
  for (int t = 0; t < tasks; ++t) if (accepted(status[t]) && (best < 0 || count[t] > count[best])) best = t;
  return best;
}

// ---- poses and points ----
inline void cross3(const double a[3], const double b[3], double out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1]; out[1] = a[2] * b[0] - a[0] * b[2]; out[2] = a[0] * b[1] - a[1] * b[0];
}
inline double det3(const double R[9]) {
  return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}
// ceres::AngleAxisRotatePoint for the two rvec/tvec <-> (rotation, camera centre) conversions either side of a call
// (solveRSpnp.cpp:119-128, :166-176): glue on two 3-vectors, not part of the solve.
inline void rotate(const double w[3], const double p[3], double out[3]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double wxp[3];
  cross3(w, p, wxp);
  if (th2 > 2.220446049250313e-16) {
    const double th = std::sqrt(th2), c = std::cos(th), s = std::sin(th), it = 1.0 / th;
    const double k[3] = {w[0] * it, w[1] * it, w[2] * it};
    const double kxp[3] = {wxp[0] * it, wxp[1] * it, wxp[2] * it};
    const double kp = (k[0] * p[0] + k[1] * p[1] + k[2] * p[2]) * (1.0 - c);
    for (int i = 0; i < 3; ++i) out[i] = p[i] * c + kxp[i] * s + k[i] * kp;
  } else {
    for (int i = 0; i < 3; ++i) out[i] = p[i] + wxp[i];
  }
}
// pose = (rvec, -R(rvec)^T tvec)
inline void to_pose(const double rvec[3], const double tvec[3], double pose[6]) {
  const double rinv[3] = {-rvec[0], -rvec[1], -rvec[2]}, nt[3] = {-tvec[0], -tvec[1], -tvec[2]};
  for (int i = 0; i < 3; ++i) pose[i] = rvec[i];
  rotate(rinv, nt, pose + 3);
}
// tvec = -R(rvec) centre
inline void from_pose(const double pose[6], double rvec[3], double tvec[3]) {
  double t[3];
  rotate(pose, pose + 3, t);
  for (int i = 0; i < 3; ++i) { rvec[i] = pose[i]; tvec[i] = -t[i]; }
}
// the undistorted, normalised image point of a pixel; sfm intrinsics (mat/cam.h:33): fx, fy, k1, k2, p1, p2, k3, cx, cy
inline void normalised_point(const double cam[NUM_CAM_PARAMS], double u, double v, double out[2]) {
  const double pn[2] = {(u - cam[7]) / cam[0], (v - cam[8]) / cam[1]};
  double pu[2] = {pn[0], pn[1]};
  for (int it = 0; it < 20; ++it) {   // the fixed-point undistortion of mat/cam.h:77-112, a few steps of it
    const double x = pu[0], y = pu[1], r2 = x * x + y * y, d = 1.0 + r2 * (cam[2] + r2 * (cam[3] + r2 * cam[6])), xy = x * y;
    const double dx = d * x + 2.0 * cam[4] * xy + cam[5] * (r2 + 2.0 * x * x), dy = d * y + cam[4] * (r2 + 2.0 * y * y) + 2.0 * cam[5] * xy;
    pu[0] -= dx - pn[0]; pu[1] -= dy - pn[1];
  }
  out[0] = pu[0]; out[1] = pu[1];
}
inline std::vector<double> normalised_points(const double cam[NUM_CAM_PARAMS], const float* ipoints, int n) {
  std::vector<double> out(2 * (size_t)n);
  for (int i = 0; i < n; ++i) normalised_point(cam, ipoints[2 * (size_t)i], ipoints[2 * (size_t)i + 1], &out[2 * (size_t)i]);
  return out;
}
// nearest rotation to a (nearly orthogonal) 3 x 3 matrix, R <- (R + R^-T) / 2; false: singular or a reflection
inline bool nearest_rotation(double R[9]) {
  for (int it = 0; it < 30; ++it) {
    const double det = det3(R);
    if (!(std::fabs(det) > 1e-12)) return false;
    const double it_[9] = {(R[4] * R[8] - R[5] * R[7]) / det, (R[5] * R[6] - R[3] * R[8]) / det, (R[3] * R[7] - R[4] * R[6]) / det,
                           (R[2] * R[7] - R[1] * R[8]) / det, (R[0] * R[8] - R[2] * R[6]) / det, (R[1] * R[6] - R[0] * R[7]) / det,
                           (R[1] * R[5] - R[2] * R[4]) / det, (R[2] * R[3] - R[0] * R[5]) / det, (R[0] * R[4] - R[1] * R[3]) / det};   // R^-T
    for (int k = 0; k < 9; ++k) R[k] = 0.5 * (R[k] + it_[k]);
  }
  return det3(R) > 0;
}
// (rotation matrix world->camera, tvec) -> rsba's 6-vector
inline bool pose_from_rt(const double R[9], const double tvec[3], double pose[6]) {
  double rvec[3];
  const double tr = R[0] + R[4] + R[8], cs = std::fmin(1.0, std::fmax(-1.0, 0.5 * (tr - 1.0))), th = std::acos(cs);
  const double ax[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double sn = 0.5 * std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  if (sn > 1e-8) for (int k = 0; k < 3; ++k) rvec[k] = ax[k] * (th / (2.0 * sn));
  else if (cs > 0) for (int k = 0; k < 3; ++k) rvec[k] = 0.5 * ax[k];
  else {   // a half turn: the axis from the diagonal
    const double d[3] = {std::sqrt(std::fmax(0.0, 0.5 * (R[0] + 1.0))), std::sqrt(std::fmax(0.0, 0.5 * (R[4] + 1.0))), std::sqrt(std::fmax(0.0, 0.5 * (R[8] + 1.0)))};
    rvec[0] = th * d[0]; rvec[1] = th * d[1] * (R[1] + R[3] >= 0 ? 1.0 : -1.0); rvec[2] = th * d[2] * (R[2] + R[6] >= 0 ? 1.0 : -1.0);
  }
  to_pose(rvec, tvec, pose);
  for (int k = 0; k < 6; ++k) if (!std::isfinite(pose[k])) return false;
  return true;
}

// ---- cyclic Jacobi on a symmetric N x N matrix: a is diagonalised in place, the columns of v become the eigenvectors.  At most `sweeps`
// sweeps over the pairs p < q in row-major order, ended once the sum of the squared off-diagonal entries is below `threshold` ----
template <int N>
inline void jacobi(double a[N][N], double v[N][N], int sweeps, double threshold) {
  for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < sweeps; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < N; ++i) for (int j = i + 1; j < N; ++j) off += a[i][j] * a[i][j];
    if (off < threshold) break;
    for (int p_ = 0; p_ < N; ++p_) for (int q = p_ + 1; q < N; ++q) {
      if (std::fabs(a[p_][q]) < 1e-300) continue;
      const double theta = (a[q][q] - a[p_][p_]) / (2.0 * a[p_][q]);
      const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0)), c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
      for (int k = 0; k < N; ++k) { const double akp = a[k][p_], akq = a[k][q]; a[k][p_] = c * akp - sn * akq; a[k][q] = sn * akp + c * akq; }
      for (int k = 0; k < N; ++k) { const double apk = a[p_][k], aqk = a[q][k]; a[p_][k] = c * apk - sn * aqk; a[q][k] = sn * apk + c * aqk; }
      for (int k = 0; k < N; ++k) { const double vkp = v[k][p_], vkq = v[k][q]; v[k][p_] = c * vkp - sn * vkq; v[k][q] = sn * vkp + c * vkq; }
    }
  }
}
// eigenvector of the smallest eigenvalue of a symmetric 12 x 12 matrix
inline void smallest_eigenvector12(double a[12][12], double vec[12], double gap[3] = nullptr) {
  double v[12][12];
  jacobi<12>(a, v, 60, 1e-30);
  int best = 0;
  for (int i = 1; i < 12; ++i) if (a[i][i] < a[best][best]) best = i;
  for (int k = 0; k < 12; ++k) vec[k] = v[k][best];
  if (gap) {   // the two smallest eigenvalues and the largest: is the null space ONE direction?
    double second = 0.0, largest = 0.0; bool have_second = false;   // (a flag, not a negative sentinel: rounding can leave a zero eigenvalue slightly negative)
    for (int i = 0; i < 12; ++i) { if (i != best && (!have_second || a[i][i] < second)) { second = a[i][i]; have_second = true; } largest = std::fmax(largest, a[i][i]); }
    gap[0] = a[best][best]; gap[1] = second; gap[2] = largest;
  }
}
// eigen decomposition of a symmetric 3 x 3 matrix: values ascending, vec[k] = unit eigenvector of val[k]
inline void eigen3(const double sym[6] /* xx xy xz yy yz zz */, double val[3], double vec[3][3]) {
  double a[3][3] = {{sym[0], sym[1], sym[2]}, {sym[1], sym[3], sym[4]}, {sym[2], sym[4], sym[5]}}, v[3][3];
  jacobi<3>(a, v, 40, 1e-300);
  int order[3] = {0, 1, 2};
  for (int i = 0; i < 3; ++i) for (int j = i + 1; j < 3; ++j) if (a[order[j]][order[j]] < a[order[i]][order[i]]) { const int t = order[i]; order[i] = order[j]; order[j] = t; }
  for (int k = 0; k < 3; ++k) { val[k] = a[order[k]][order[k]]; for (int r = 0; r < 3; ++r) vec[k][r] = v[r][order[k]]; }
}
// the two gap tests of a DLT, on smallest_eigenvector12's gap: false where there is a second (near-)null direction, or no null direction to
// speak of — an ambiguous null vector is not a solution
inline bool single_null_direction(const double gap[3]) { return gap[1] > 1e-9 * gap[2] && gap[0] < 0.05 * gap[1]; }
// the null vector of a 9-unknown Gram matrix, by the 12 x 12 solver with three idle unknowns at twice the trace, far from the null space
// (zero off-diagonals are skipped, so the rotations are those of a 9 x 9 sweep); false: a zero matrix, or not the single null direction
inline bool null_vector9(const double gram[9][9], double vec[9]) {
  double ata[12][12] = {}, big = 0.0;
  for (int a = 0; a < 9; ++a) for (int b = 0; b < 9; ++b) ata[a][b] = gram[a][b];
  for (int a = 0; a < 9; ++a) big += ata[a][a];
  if (!(big > 0.0)) return false;
  for (int a = 9; a < 12; ++a) ata[a][a] = 2.0 * big;
  double ev[12], gap[3];
  smallest_eigenvector12(ata, ev, gap);
  if (!single_null_direction(gap)) return false;
  for (int k = 0; k < 9; ++k) vec[k] = ev[k];
  return true;
}

// ---- Hartley normalisation of one side: the centroid c of the points p[idx[0..m)] ([.][2]) and s = their mean distance from it over
// sqrt 2, so that x' = (x - c) / s; false: s is not positive ----
inline bool hartley_side(const double* p, const int32_t* idx, int m, double c[2], double* s) {
  c[0] = c[1] = 0.0; *s = 0.0;
  for (int i = 0; i < m; ++i) { c[0] += p[2 * (size_t)idx[i]] / m; c[1] += p[2 * (size_t)idx[i] + 1] / m; }
  for (int i = 0; i < m; ++i) *s += std::hypot(p[2 * (size_t)idx[i]] - c[0], p[2 * (size_t)idx[i] + 1] - c[1]) / m;
  if (!(*s > 0.0)) return false;
  *s /= 1.4142135623730951;
  return true;
}

// ---- polynomials by coefficient arrays, ascending powers ----
constexpr int kBisections = 40;
inline double poly_eval(const double* c, int deg, double t) {
  double h = c[deg];
  for (int k = deg - 1; k >= 0; --k) h = h * t + c[k];
  return h;
}
// the root of a polynomial that is monotonic on [lo, hi], where it changes sign there; otherwise hi (which keeps breakpoints ordered)
inline bool poly_bisect(const double* c, int deg, double lo, double hi, double* root) {
  *root = hi;
  const bool plo = poly_eval(c, deg, lo) > 0.0, phi = poly_eval(c, deg, hi) > 0.0;
  if (plo == phi) return false;
  for (int it = 0; it < kBisections; ++it) {
    const double mid = 0.5 * (lo + hi);
    if ((poly_eval(c, deg, mid) > 0.0) == plo) lo = mid; else hi = mid;
  }
  *root = 0.5 * (lo + hi);
  return true;
}

}  // namespace hyp_detail

}  // namespace rsba_amd
