// Two-view degeneracy: what kind of geometry a verified frame pair has — enough parallax to triangulate from, or a rotation / a baseline that
// is a per cent of the depth, or a scene plane — so that the pair a reconstruction starts from is chosen by more than its inlier count.  An
// essential matrix fitted to a near-pure rotation collects as many Sampson inliers as a well-conditioned one and its translation is noise;
// neighbouring frames of a video are exactly such pairs, and pickBootstrapPair(reports) prefers them.  Two measurements per pair, the ones
// every incremental pipeline takes: how well a homography explains the correspondences compared with the essential matrix, and how many
// of the inliers in front of both cameras subtend at least a given angle.  The reference has no such step, so this text and rsba_amd.h
// (rsba_homography_*, rsba_two_view_classify_pairs) are the definition; homo_detail below is its host form, which the device kernels
// (rsba_amd/csrc/kernels_homography.hip) restate and the tests hold both to.
//
// Conventions as in two_view.hpp: a = (xa, ya, 1), b = (xb, yb, 1) normalised image points; H row-major with b ~ H a.
// dlt.  Hartley normalisation of each side's m >= 4 points, the 9 x 9 Gram matrix of the 2 m rows (-a', 0, xb' a') and (0, -a', yb' a') (a
// point's first row, then its second), its null vector by hyp_detail::null_vector9, the normalisation undone (H = Tb^-1 Hn Ta), unit Frobenius
// norm, (H a)_z > 0 for the first index.  Declined: a repeated index, a Hartley scale that is not positive, a second null direction (three
// of four points on a line), (H a)_z not of one sign over the subset, |det H| not above 1e-6, a result that is not finite.
// Inlier rule.  Both transfer errors in normalised coordinates, H^-1 the adjugate over the determinant; inlier iff (H a)_z > 0, (H^-1 b)_z > 0
// and max(d_ab^2, d_ba^2) f^2 <= threshold_px^2 with the epipolar rule's f.
// Parallax rule.  Of the Sampson inliers of a pair's E that are in front for its pose (num_front), those whose rays a and R^T b make an angle
// of at least the threshold (num_parallax): a . (R^T b) <= cos(threshold) sqrt(|a|^2 |R^T b|^2).
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "two_view.hpp"

namespace rsba_amd {

struct HomographyResult {
  bool ok = false;                         // a hypothesis was accepted
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int num_inliers = 0;
  int winner_task = -1, refits_adopted = 0;
  std::vector<uint8_t> inliers;            // [n]
};

namespace homo_detail {

// the homography of the correspondences idx[0..m) of the normalised points na, nb [.][2]; false: declined (H untouched)
inline bool dlt(const double* na, const double* nb, const int32_t* idx, int m, double H[9]) {
  if (m < 4) return false;
  for (int i = 0; i < m; ++i) for (int k = i + 1; k < m; ++k) if (idx[i] == idx[k]) return false;
  double ca[2], cb[2], sa, sb;
  const bool oka = hyp_detail::hartley_side(na, idx, m, ca, &sa), okb = hyp_detail::hartley_side(nb, idx, m, cb, &sb);
  if (!oka || !okb) return false;
  double ata[9][9] = {};
  for (int i = 0; i < m; ++i) {
    const size_t j = 2 * (size_t)idx[i];
    const double xa = (na[j] - ca[0]) / sa, ya = (na[j + 1] - ca[1]) / sa, xb = (nb[j] - cb[0]) / sb, yb = (nb[j + 1] - cb[1]) / sb;
    const double r1[9] = {-xa, -ya, -1.0, 0.0, 0.0, 0.0, xb * xa, xb * ya, xb};
    const double r2[9] = {0.0, 0.0, 0.0, -xa, -ya, -1.0, yb * xa, yb * ya, yb};
    for (int a = 0; a < 9; ++a) for (int b = 0; b < 9; ++b) ata[a][b] += r1[a] * r1[b];
    for (int a = 0; a < 9; ++a) for (int b = 0; b < 9; ++b) ata[a][b] += r2[a] * r2[b];
  }
  double ev[9];
  if (!hyp_detail::null_vector9(ata, ev)) return false;   // a second null direction: three of the four points on a line
  // undo the normalisation: H = Tb^-1 Hn Ta, Ta = [[1/sa 0 -cx/sa] [0 1/sa -cy/sa] [0 0 1]], Tb^-1 = [[sb 0 cx] [0 sb cy] [0 0 1]]
  double M[9], out[9], fro = 0.0;
  for (int r = 0; r < 3; ++r) {
    M[3 * r] = ev[3 * r] / sa; M[3 * r + 1] = ev[3 * r + 1] / sa;
    M[3 * r + 2] = ev[3 * r + 2] - (ca[0] * ev[3 * r] + ca[1] * ev[3 * r + 1]) / sa;
  }
  for (int k = 0; k < 3; ++k) { out[k] = sb * M[k] + cb[0] * M[6 + k]; out[3 + k] = sb * M[3 + k] + cb[1] * M[6 + k]; out[6 + k] = M[6 + k]; }
  for (int k = 0; k < 9; ++k) fro += out[k] * out[k];
  fro = std::sqrt(fro);
  for (int k = 0; k < 9; ++k) out[k] /= fro;
  if (out[6] * na[2 * (size_t)idx[0]] + out[7] * na[2 * (size_t)idx[0] + 1] + out[8] < 0) for (int k = 0; k < 9; ++k) out[k] = -out[k];
  for (int i = 0; i < m; ++i) if (!(out[6] * na[2 * (size_t)idx[i]] + out[7] * na[2 * (size_t)idx[i] + 1] + out[8] > 0.0)) return false;   // the orientation test
  if (!(std::fabs(hyp_detail::det3(out)) > 1e-6)) return false;
  for (int k = 0; k < 9; ++k) if (!std::isfinite(out[k])) return false;
  for (int k = 0; k < 9; ++k) H[k] = out[k];
  return true;
}

// the adjugate over the determinant; false: a determinant that is zero or not finite, an inverse that is not finite.  The device evaluates
// these operations in this order (rsba_amd/csrc/two_view_rules.hpp, contraction off): the inverse feeds the deciding comparison
inline bool invert(const double H[9], double Hi[9]) {
  const double c0 = H[4] * H[8] - H[5] * H[7], c1 = H[5] * H[6] - H[3] * H[8], c2 = H[3] * H[7] - H[4] * H[6];
  const double det = H[0] * c0 + H[1] * c1 + H[2] * c2;
  if (!(std::fabs(det) > 0.0)) return false;
  Hi[0] = c0 / det; Hi[1] = (H[2] * H[7] - H[1] * H[8]) / det; Hi[2] = (H[1] * H[5] - H[2] * H[4]) / det;
  Hi[3] = c1 / det; Hi[4] = (H[0] * H[8] - H[2] * H[6]) / det; Hi[5] = (H[2] * H[3] - H[0] * H[5]) / det;
  Hi[6] = c2 / det; Hi[7] = (H[1] * H[6] - H[0] * H[7]) / det; Hi[8] = (H[0] * H[4] - H[1] * H[3]) / det;
  for (int k = 0; k < 9; ++k) if (!std::isfinite(Hi[k])) return false;
  return true;
}

// the deciding comparison (the device: these operations in this order, contraction off); d2_out: max(d_ab^2, d_ba^2), -1 behind a camera
inline bool transfer_inlier(const double H[9], const double Hi[9], double xa, double ya, double xb, double yb, double f2, double thr2, double* d2_out = nullptr) {
  if (d2_out) *d2_out = -1.0;
  const double w = H[6] * xa + H[7] * ya + H[8];
  if (!(w > 0.0)) return false;
  const double u = (H[0] * xa + H[1] * ya + H[2]) / w, v = (H[3] * xa + H[4] * ya + H[5]) / w;
  const double eu = xb - u, ev = yb - v;
  const double dab = eu * eu + ev * ev;
  const double w2 = Hi[6] * xb + Hi[7] * yb + Hi[8];
  if (!(w2 > 0.0)) return false;
  const double u2 = (Hi[0] * xb + Hi[1] * yb + Hi[2]) / w2, v2 = (Hi[3] * xb + Hi[4] * yb + Hi[5]) / w2;
  const double fu = xa - u2, fv = ya - v2;
  const double dba = fu * fu + fv * fv;
  const double d2 = dab > dba ? dab : dba;
  if (d2_out) *d2_out = d2;
  return d2 * f2 <= thr2;
}

// the count of one H over all n correspondences; false: declined (a zero count, a zero mask)
inline bool score(const double* na, const double* nb, int n, const double H[9], double f2, double thr2, int32_t* num_inliers, uint8_t* mask = nullptr) {
  *num_inliers = 0;
  if (mask) for (int i = 0; i < n; ++i) mask[i] = 0;
  double Hi[9];
  if (!invert(H, Hi)) return false;
  int32_t inl = 0;
  for (int i = 0; i < n; ++i) {
    const bool in = transfer_inlier(H, Hi, na[2 * (size_t)i], na[2 * (size_t)i + 1], nb[2 * (size_t)i], nb[2 * (size_t)i + 1], f2, thr2);
    if (mask) mask[i] = in ? 1 : 0;
    if (in) ++inl;
  }
  *num_inliers = inl;
  return true;
}

// (R, t) of a pose of camera B in A's frame: column k of R is the rotated unit vector k, t = -R centre
inline void pose_rt(const double pose[6], double R[9], double t[3]) {
  for (int k = 0; k < 3; ++k) {
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double r[3];
    hyp_detail::rotate(pose, e, r);
    R[k] = r[0]; R[3 + k] = r[1]; R[6 + k] = r[2];
  }
  double r[3];
  hyp_detail::rotate(pose, pose + 3, r);
  for (int k = 0; k < 3; ++k) t[k] = -r[k];
}
// the angle between the rays a and R^T b is at least the angle whose cosine is c (the device: these operations in this order);
// margin_out: (c sqrt(|a|^2 |R^T b|^2) - a . R^T b) / sqrt(|a|^2 |R^T b|^2)
inline bool has_parallax(const double R[9], double xa, double ya, double xb, double yb, double c, double* margin_out = nullptr) {
  const double q0 = R[0] * xb + R[3] * yb + R[6], q1 = R[1] * xb + R[4] * yb + R[7], q2 = R[2] * xb + R[5] * yb + R[8];
  const double dot = xa * q0 + ya * q1 + q2;
  const double aa = xa * xa + ya * ya + 1.0, qq = q0 * q0 + q1 * q1 + q2 * q2;
  const double rhs = c * std::sqrt(aa * qq);
  if (margin_out) *margin_out = (rhs - dot) / std::sqrt(aa * qq);
  return dot <= rhs;
}
// num_front: the Sampson inliers of E in front for the pose; num_parallax: those of them with parallax
inline void parallax_counts(const double* na, const double* nb, int n, const double E[9], const double pose[6], double f2, double thr2, double cos_min,
                            int32_t* num_front, int32_t* num_parallax) {
  double R[9], t[3];
  pose_rt(pose, R, t);
  int32_t front = 0, par = 0;
  for (int i = 0; i < n; ++i) {
    const double xa = na[2 * (size_t)i], ya = na[2 * (size_t)i + 1], xb = nb[2 * (size_t)i], yb = nb[2 * (size_t)i + 1];
    if (!epi_detail::sampson_inlier(E, xa, ya, xb, yb, f2, thr2) || !epi_detail::in_front(R, t, 1.0, xa, ya, xb, yb)) continue;
    ++front;
    if (has_parallax(R, xa, ya, xb, yb, cos_min)) ++par;
  }
  *num_front = front; *num_parallax = par;
}

// The RANSAC loop over a backend: hypotheses(subsets, m, tasks, H, status, num_inliers) fills the arrays of `tasks` tasks, inlier_mask(H, mask)
// the flags [n] of one matrix.  The winner: most inliers, then the lowest task.  Then up to opt.refits rounds of "the DLT over the current
// inliers (one task, m = their number, at least 5), recount", a refit adopted only when its count is not lower.
template <class Hypotheses, class InlierMask>
inline HomographyResult ransac(int n, const TwoViewOptions& opt, Hypotheses&& hypotheses, InlierMask&& inlier_mask) {
  HomographyResult res;
  res.inliers.assign((size_t)(n > 0 ? n : 0), 0);
  if (n < 4 || opt.iterations <= 0) return res;
  const int T = opt.iterations;
  const std::vector<int32_t> subsets = hyp_detail::distinct_subsets(n, 4, T, opt.rng_state);
  std::vector<double> H((size_t)T * 9);
  std::vector<uint8_t> status((size_t)T);
  std::vector<int32_t> inl((size_t)T);
  hypotheses(subsets.data(), 4, T, H.data(), status.data(), inl.data());
  const int best = hyp_detail::most_inliers(status.data(), inl.data(), T, [](uint8_t s) { return s != 0; });
  if (best < 0) return res;
  res.ok = true;
  res.winner_task = best;
  res.num_inliers = inl[(size_t)best];
  for (int k = 0; k < 9; ++k) res.H[k] = H[(size_t)best * 9 + k];
  inlier_mask(res.H, res.inliers.data());
  for (int round = 0; round < opt.refits; ++round) {
    std::vector<int32_t> idx;
    for (int i = 0; i < n; ++i) if (res.inliers[(size_t)i]) idx.push_back(i);
    if (idx.size() < 5) break;
    double h2[9]; uint8_t st = 0; int32_t inl2 = 0;
    hypotheses(idx.data(), (int)idx.size(), 1, h2, &st, &inl2);
    if (!st || inl2 < res.num_inliers) break;   // not adopted: the next round would refit the same set
    res.num_inliers = inl2;
    for (int k = 0; k < 9; ++k) res.H[k] = h2[k];
    inlier_mask(res.H, res.inliers.data());
    ++res.refits_adopted;
  }
  return res;
}

// the loop from the host definitions alone: what the device path is compared with
inline HomographyResult host_ransac(const float* xy_a, const float* xy_b, int n, const double cam_a[NUM_CAM_PARAMS], const double cam_b[NUM_CAM_PARAMS],
                                    const TwoViewOptions& opt) {
  if (n < 4) return ransac(n, opt, [](auto&&...) {}, [](auto&&...) {});
  const std::vector<double> na = hyp_detail::normalised_points(cam_a, xy_a, n), nb = hyp_detail::normalised_points(cam_b, xy_b, n);
  const double f2 = epi_detail::mean_focal2(cam_a, cam_b), thr2 = opt.threshold_px * opt.threshold_px;
  return ransac(n, opt,
    [&](const int32_t* sub, int m, int tasks, double* H, uint8_t* status, int32_t* inl) {
      for (int t = 0; t < tasks; ++t) {
        double h[9];
        status[t] = dlt(na.data(), nb.data(), sub + (size_t)t * m, m, h) && score(na.data(), nb.data(), n, h, f2, thr2, &inl[t]) ? 1 : 0;
        if (status[t]) for (int k = 0; k < 9; ++k) H[9 * (size_t)t + k] = h[k];
        else inl[t] = 0;
      }
    },
    [&](const double H[9], uint8_t* mask) { int32_t c; score(na.data(), nb.data(), n, H, f2, thr2, &c, mask); });
}

}  // namespace homo_detail

// RANSAC over four-point homographies: opt.iterations subsets from hyp_detail::distinct_subsets(n, 4, ...), all scored in one device call
// (rsba_homography_hypotheses); the most inliers win, ties go to the lowest task; then the refits.  opt supplies iterations, threshold_px,
// refits, rng_state and hypotheses_on_device (false: the same loop from the host definitions); its other fields are not read.
inline HomographyResult findHomographyRansac(const float* xy_a, const float* xy_b, int n, const double cam_a[NUM_CAM_PARAMS], const double cam_b[NUM_CAM_PARAMS],
                                             const TwoViewOptions& opt = TwoViewOptions(), int device = 0) {
  if (!opt.hypotheses_on_device) return homo_detail::host_ransac(xy_a, xy_b, n, cam_a, cam_b, opt);
  return homo_detail::ransac(n, opt,
    [&](const int32_t* sub, int m, int tasks, double* H, uint8_t* status, int32_t* inl) {
      hyp_detail::check(rsba_homography_hypotheses(device, cam_a, cam_b, xy_a, xy_b, n, sub, m, tasks, opt.threshold_px, H, status, inl));
    },
    [&](const double H[9], uint8_t* mask) { hyp_detail::check(rsba_homography_inliers(device, cam_a, cam_b, xy_a, xy_b, n, H, opt.threshold_px, mask)); });
}

// ---- the classification of verified pairs ----
enum class PairKind { Unverified, LowParallax, Planar, General };
inline const char* pairKindName(PairKind k) {
  return k == PairKind::Unverified ? "Unverified" : k == PairKind::LowParallax ? "LowParallax" : k == PairKind::Planar ? "Planar" : "General";
}

struct PairGeometry {
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool h_ok = false;                       // the homography RANSAC found a winner
  int num_h_inliers = 0;                   // transfer-error inliers of H
  int num_front = 0;                       // Sampson inliers of the pair's E in front for its pose (0 where the essential result is not ok)
  int num_parallax = 0;                    // those of them whose rays make at least min_parallax_deg
  int h_winner_task = -1, h_refits_adopted = 0;
  std::vector<uint8_t> h_inliers;          // [n]
  PairKind kind = PairKind::Unverified;
};

// The thresholds are the usual defaults of incremental structure from motion and the caller's to set: neighbouring frames of a video
// rarely reach 16 degrees, and a smaller angle (a few degrees) is normal for them.
struct ClassifyOptions {
  double min_parallax_deg = 16.0;          // a correspondence has parallax when its rays make at least this angle
  double min_parallax_share = 0.5;         // LowParallax when fewer than this share of num_front have it (0.5: the median rule)
  double max_h_ratio = 0.8;                // Planar when the homography explains at least this share of the essential matrix's inliers
  int max_tasks_per_launch = 0;            // rsba_two_view_classify_pairs' (0: its default)
};

namespace homo_detail {
// the kind rule, in this order
inline PairKind kind_of(bool essential_ok, int num_inliers, const PairGeometry& g, const ClassifyOptions& co) {
  if (!essential_ok) return PairKind::Unverified;
  if ((double)g.num_parallax < co.min_parallax_share * (double)g.num_front) return PairKind::LowParallax;
  if ((double)g.num_h_inliers >= co.max_h_ratio * (double)num_inliers) return PairKind::Planar;
  return PairKind::General;
}
inline double cos_of_degrees(double deg) { return std::cos(deg * 3.14159265358979323846 / 180.0); }
}  // namespace homo_detail

// The geometry of every pair, result p from pairs[p] and its essential result essential_results[p] (findEssentialRansacPairs', or any
// TwoViewResult whose ok, E, pose_b and num_inliers are set): the homography RANSAC of findHomographyRansac(pairs[p]..., tv, device) and, for
// a pair whose essential result is ok, the parallax counts of its E and pose_b — all pairs in ONE batched device call
// (rsba_two_view_classify_pairs).  tv.hypotheses_on_device == false: the host loop per pair.
inline std::vector<PairGeometry> classifyPairs(const std::vector<EssentialPair>& pairs, const std::vector<TwoViewResult>& essential_results,
                                               const TwoViewOptions& tv = TwoViewOptions(), const ClassifyOptions& co = ClassifyOptions(), int device = 0) {
  if (pairs.size() != essential_results.size()) throw std::invalid_argument("classifyPairs: one essential result per pair");
  const size_t P = pairs.size();
  std::vector<PairGeometry> out(P);
  const double cos_min = homo_detail::cos_of_degrees(co.min_parallax_deg);
  for (size_t p = 0; p < P; ++p) out[p].h_inliers.assign((size_t)(pairs[p].n > 0 ? pairs[p].n : 0), 0);
  if (!tv.hypotheses_on_device) {
    for (size_t p = 0; p < P; ++p) {
      const EssentialPair& q = pairs[p];
      const HomographyResult h = homo_detail::host_ransac(q.xy_a, q.xy_b, q.n, q.cam_a, q.cam_b, tv);
      PairGeometry& g = out[p];
      g.h_ok = h.ok; g.num_h_inliers = h.num_inliers; g.h_winner_task = h.winner_task; g.h_refits_adopted = h.refits_adopted; g.h_inliers = h.inliers;
      for (int k = 0; k < 9; ++k) g.H[k] = h.H[k];
      if (essential_results[p].ok && q.n > 0) {
        const std::vector<double> na = hyp_detail::normalised_points(q.cam_a, q.xy_a, q.n), nb = hyp_detail::normalised_points(q.cam_b, q.xy_b, q.n);
        int32_t front = 0, par = 0;
        homo_detail::parallax_counts(na.data(), nb.data(), q.n, essential_results[p].E, essential_results[p].pose_b, epi_detail::mean_focal2(q.cam_a, q.cam_b),
                                     tv.threshold_px * tv.threshold_px, cos_min, &front, &par);
        g.num_front = front; g.num_parallax = par;
      }
    }
  } else if (P > 0 && tv.iterations > 0) {
    const int T = tv.iterations;
    const PairArrays A = pair_arrays(pairs, 4, 4, T, tv.rng_state);
    const std::vector<int32_t>& offset = A.offset;
    std::vector<double> E(P * 9, 0.0), poses(P * 6, 0.0);
    std::vector<uint8_t> pst(P, 0);
    for (size_t p = 0; p < P; ++p) {
      pst[p] = essential_results[p].ok ? 1 : 0;
      for (int k = 0; k < 9; ++k) E[p * 9 + k] = essential_results[p].E[k];
      for (int k = 0; k < 6; ++k) poses[p * 6 + k] = essential_results[p].pose_b[k];
    }
    std::vector<double> H(P * 9, 0.0);
    std::vector<uint8_t> status(P, 0), mask((size_t)offset[P] + 1, 0);
    std::vector<int32_t> winner(P, -1), adopted(P, 0), inl(P, 0), front(P, 0), par(P, 0);
    hyp_detail::check(rsba_two_view_classify_pairs(device, A.cams.data(), A.num_cams(), A.cam_a.data(), A.cam_b.data(), offset.data(), (int32_t)P, A.xy_a.data(), A.xy_b.data(),
                                                   E.data(), poses.data(), pst.data(), A.subsets.data(), T, tv.threshold_px, tv.refits, cos_min, co.max_tasks_per_launch, H.data(),
                                                   status.data(), winner.data(), adopted.data(), inl.data(), mask.data(), front.data(), par.data()));
    for (size_t p = 0; p < P; ++p) {
      PairGeometry& g = out[p];
      g.num_front = front[p]; g.num_parallax = par[p];
      if (!status[p]) continue;
      g.h_ok = true; g.num_h_inliers = inl[p]; g.h_winner_task = winner[p]; g.h_refits_adopted = adopted[p];
      for (int k = 0; k < 9; ++k) g.H[k] = H[p * 9 + k];
      std::copy(mask.begin() + offset[p], mask.begin() + offset[p + 1], g.h_inliers.begin());
    }
  }
  for (size_t p = 0; p < P; ++p) out[p].kind = homo_detail::kind_of(essential_results[p].ok, essential_results[p].num_inliers, out[p], co);
  return out;
}

// classifyPairs for the pairs of verifyMatches' reports: for every report, the refs of frame B's observations into frame A, collected
// exactly as verifyMatches collects them (observation order, then the order of an observation's list), E and pose_b from the report.  The
// call forms the inlier mask of E itself, so it gives the same counts before the erasure of the outliers as after it would for the refs
// that remain inliers.  Nothing in the session is touched.
inline std::vector<PairGeometry> classifyMatches(const Session& sess, const std::vector<PairReport>& reports, const TwoViewOptions& tv = TwoViewOptions(), int device = 0,
                                                 const ClassifyOptions& co = ClassifyOptions()) {
  struct Found { std::vector<float> xa, xb; };
  std::vector<Found> found(reports.size());
  std::vector<EssentialPair> pairs(reports.size());
  std::vector<TwoViewResult> results(reports.size());
  for (size_t p = 0; p < reports.size(); ++p) {
    const PairReport& r = reports[p];
    if (r.frameA < 0 || r.frameA >= r.frameB || (size_t)r.frameB >= sess.frames.size()) throw std::invalid_argument("classifyMatches: a report names frames the session does not have");
    const Frame& A = sess.frames[(size_t)r.frameA];
    const Frame& B = sess.frames[(size_t)r.frameB];
    for (size_t oi = 0; oi < B.obs.size(); ++oi)
      for (size_t ri = 0; ri < B.obs[oi].matches.size(); ++ri) {
        const ObservationRef& ref = B.obs[oi].matches[ri];
        if (ref.frame != r.frameA || ref.obs < 0 || (size_t)ref.obs >= A.obs.size()) continue;
        const Observation& oa = A.obs[(size_t)ref.obs];
        found[p].xa.push_back((float)oa.x); found[p].xa.push_back((float)oa.y); found[p].xb.push_back((float)B.obs[oi].x); found[p].xb.push_back((float)B.obs[oi].y);
      }
    pairs[p].xy_a = found[p].xa.data(); pairs[p].xy_b = found[p].xb.data(); pairs[p].n = (int)(found[p].xa.size() / 2);
    pairs[p].cam_a = A.__isset.cam ? A.cam.data() : sess.cam.data();
    pairs[p].cam_b = B.__isset.cam ? B.cam.data() : sess.cam.data();
    results[p].ok = r.ok; results[p].num_inliers = r.num_inliers; results[p].num_front = r.num_front;
    for (int k = 0; k < 9; ++k) results[p].E[k] = r.E[k];
    for (int k = 0; k < 6; ++k) results[p].pose_b[k] = r.pose_b[k];
  }
  return classifyPairs(pairs, results, tv, co, device);
}

// The pair to start a reconstruction from, with the geometry taken into account: among the ok pairs of kind General (and Planar, if
// allowed — a planar start needs the five-point solver's pose) the one with the most correspondences that have parallax; ties go to the
// lowest frameB, then the lowest frameA.  -1: none.
struct PickOptions { bool allow_planar = false; };
inline int pickBootstrapPair(const std::vector<PairReport>& reports, const std::vector<PairGeometry>& geometry, const PickOptions& po = PickOptions()) {
  if (reports.size() != geometry.size()) throw std::invalid_argument("pickBootstrapPair: one geometry per report");
  int best = -1;
  for (size_t p = 0; p < reports.size(); ++p) {
    const PairReport& r = reports[p];
    const PairGeometry& g = geometry[p];
    if (!r.ok || !(g.kind == PairKind::General || (po.allow_planar && g.kind == PairKind::Planar))) continue;
    if (best >= 0) {
      const PairReport& b = reports[(size_t)best];
      const int bp = geometry[(size_t)best].num_parallax;
      if (g.num_parallax < bp) continue;
      if (g.num_parallax == bp && (r.frameB > b.frameB || (r.frameB == b.frameB && r.frameA >= b.frameA))) continue;
    }
    best = (int)p;
  }
  return best;
}

}  // namespace rsba_amd
