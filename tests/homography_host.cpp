// Prints what the host definitions of include/rsba/pair_geometry.hpp (homo_detail::dlt, score, parallax_counts, host_ransac; classifyPairs
// and pickBootstrapPair on the host path) return for the cases of tests/homography_reference.py (test_homography_reference.py compiles and
// runs this; no device, and nothing of librsba_amd is called).
//   homography_host <cases.bin>
//     cases.bin: int32 count; per case int32 n, T, m, double cam_a[9], cam_b[9], float xy_a[n][2], xy_b[n][2], int32 subsets[T][m]
//     stdout, per subset: "<status> <H[0..9)>"
//   homography_host hypotheses <scene.bin> <T> <threshold_px> <rng_state>
//     scene.bin: int32 n, double cam_a[9], cam_b[9], float xy_a[n][2], xy_b[n][2]
//     stdout, per subset of distinct_subsets(n, 4, T, rng_state): "<status> <H[0..9)> <num_inliers> <margin> <depth margin>", margin = the smallest
//     |d^2 f^2 - thr^2| / thr^2 over the n correspondences that are in front both ways, depth margin = the smallest |(H a)_z|, |(H^-1 b)_z| met
//   homography_host ransac <scene.bin> <iterations> <threshold_px> <refits> <rng_state>
//     stdout: "<ok> <winner_task> <num_inliers> <refits_adopted>", H, the inlier flags, the indices H was fitted to (the inliers before the last
//     adopted refit, or the winner's subset) — one line each
//   homography_host subsets <n> <m> <iterations> <rng_state>   prints hyp_detail::distinct_subsets, one subset per line
//   homography_host parallax <pairs.bin> <threshold_px> <cos_min>
//     pairs.bin: int32 count; per pair int32 n, status, double cam_a[9], cam_b[9], E[9], pose[6], float xy_a[n][2], xy_b[n][2]
//     stdout, per pair: "<num_front> <num_parallax> <margin>", margin = the smallest distance of any of the three deciding comparisons of any
//     correspondence from changing sides (relative to the threshold for the Sampson distance, the smaller depth over the baseline for the
//     cheirality, in units of the cosine for the angle); zero counts and -1 for a pair with status 0
//   homography_host classify <pairs.bin> <iterations> <threshold_px> <refits> <min_inliers> <rng_state> <min_parallax_deg> [solver: 8 (default) or 5]
//     the essential RANSAC (epi_detail::host_ransac) and classifyPairs on the host path, pair p as frames (0, p + 1);
//     stdout, per pair: "<essential ok> <winner> <num_inliers> <num_front of the essential result> <kind> <h_ok> <h_winner> <h_refits> <num_h_inliers>
//     <num_front> <num_parallax>", then "pick <pickBootstrapPair(reports)> <pickBootstrapPair(reports, geometry)>"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rsba/pair_geometry.hpp"

using namespace rsba_amd;

// the library is not linked: the host path must not reach it
extern "C" int32_t rsba_two_view_classify_pairs(int32_t, const double*, int32_t, const int32_t*, const int32_t*, const int32_t*, int32_t, const float*, const float*, const double*,
                                                const double*, const uint8_t*, const int32_t*, int32_t, double, int32_t, double, int32_t, double*, uint8_t*, int32_t*, int32_t*,
                                                int32_t*, uint8_t*, int32_t*, int32_t*) {
  std::fprintf(stderr, "the host path called the device\n");
  std::abort();
}
extern "C" const char* rsba_status_string(int32_t) { return "status"; }
extern "C" const char* rsba_last_error(void) { return ""; }

struct Scene { int n = 0, status = 1; double cam_a[9], cam_b[9], E[9], pose[6]; std::vector<float> xa, xb; };
static bool read_points(FILE* f, Scene& S) {
  S.xa.resize((size_t)S.n * 2); S.xb.resize((size_t)S.n * 2);
  return std::fread(S.xa.data(), 4, S.xa.size(), f) == S.xa.size() && std::fread(S.xb.data(), 4, S.xb.size(), f) == S.xb.size();
}
static bool read_scene(const char* path, Scene& S) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  int32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1 && n >= 0 && std::fread(S.cam_a, 8, 9, f) == 9 && std::fread(S.cam_b, 8, 9, f) == 9;
  if (ok) { S.n = n; ok = read_points(f, S); }
  std::fclose(f);
  return ok;
}
static bool read_pairs(const char* path, std::vector<Scene>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  int32_t count = 0;
  bool ok = std::fread(&count, 4, 1, f) == 1 && count >= 0;
  for (int32_t p = 0; ok && p < count; ++p) {
    Scene S;
    int32_t hdr[2];
    ok = std::fread(hdr, 4, 2, f) == 2 && hdr[0] >= 0 && std::fread(S.cam_a, 8, 9, f) == 9 && std::fread(S.cam_b, 8, 9, f) == 9 && std::fread(S.E, 8, 9, f) == 9 &&
         std::fread(S.pose, 8, 6, f) == 6;
    if (ok) { S.n = hdr[0]; S.status = hdr[1]; ok = read_points(f, S); }
    if (ok) out.push_back(std::move(S));
  }
  std::fclose(f);
  return ok;
}

static void print_hypothesis(const std::vector<double>& na, const std::vector<double>& nb, int n, const int32_t* idx, double f2, double thr2) {
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Hi[9], margin = -1.0, depth = -1.0;
  int32_t inl = 0;
  const bool ok = homo_detail::dlt(na.data(), nb.data(), idx, 4, H) && homo_detail::score(na.data(), nb.data(), n, H, f2, thr2, &inl);
  if (ok && homo_detail::invert(H, Hi))
    for (int i = 0; i < n; ++i) {
      const double xa = na[2 * (size_t)i], ya = na[2 * (size_t)i + 1], xb = nb[2 * (size_t)i], yb = nb[2 * (size_t)i + 1];
      double d2;
      homo_detail::transfer_inlier(H, Hi, xa, ya, xb, yb, f2, thr2, &d2);
      const double w = std::fabs(H[6] * xa + H[7] * ya + H[8]), w2 = std::fabs(Hi[6] * xb + Hi[7] * yb + Hi[8]);
      if (depth < 0 || w < depth) depth = w;
      if (w2 < depth) depth = w2;
      if (d2 < 0) continue;
      const double rel = std::fabs(d2 * f2 - thr2) / thr2;
      if (margin < 0 || rel < margin) margin = rel;
    }
  std::printf("%d", ok ? 1 : 0);
  for (double x : H) std::printf(" %.17g", x);
  std::printf(" %d %.17g %.17g\n", inl, margin, depth);
}

int main(int argc, char** argv) {
  if (argc >= 6 && std::string(argv[1]) == "subsets") {
    const int n = std::atoi(argv[2]), m = std::atoi(argv[3]), it = std::atoi(argv[4]);
    const std::vector<int32_t> s = hyp_detail::distinct_subsets(n, m, it, std::strtoull(argv[5], nullptr, 0));
    for (int t = 0; t < it; ++t) { for (int k = 0; k < m; ++k) std::printf("%d ", s[(size_t)t * m + k]); std::printf("\n"); }
    return 0;
  }
  if (argc >= 7 && std::string(argv[1]) == "ransac") {
    Scene S;
    if (!read_scene(argv[2], S)) return 2;
    TwoViewOptions opt;
    opt.iterations = std::atoi(argv[3]); opt.threshold_px = std::atof(argv[4]); opt.refits = std::atoi(argv[5]);
    opt.rng_state = std::strtoull(argv[6], nullptr, 0); opt.hypotheses_on_device = false;
    const HomographyResult r = homo_detail::host_ransac(S.xa.data(), S.xb.data(), S.n, S.cam_a, S.cam_b, opt);
    std::printf("%d %d %d %d\n", r.ok ? 1 : 0, r.winner_task, r.num_inliers, r.refits_adopted);
    for (double x : r.H) std::printf("%.17g ", x);
    std::printf("\n");
    for (uint8_t b : r.inliers) std::printf("%d ", (int)b);
    std::printf("\n");
    // the indices H was fitted to: the inliers before the last adopted refit, or the winner's subset
    if (r.ok && r.refits_adopted > 0) {
      TwoViewOptions before = opt;
      before.refits = r.refits_adopted - 1;
      const HomographyResult q = homo_detail::host_ransac(S.xa.data(), S.xb.data(), S.n, S.cam_a, S.cam_b, before);
      for (int i = 0; i < S.n; ++i) if (q.inliers[(size_t)i]) std::printf("%d ", i);
    } else if (r.ok) {
      const std::vector<int32_t> sub = hyp_detail::distinct_subsets(S.n, 4, opt.iterations, opt.rng_state);
      for (int k = 0; k < 4; ++k) std::printf("%d ", sub[(size_t)r.winner_task * 4 + k]);
    }
    std::printf("\n");
    return 0;
  }
  if (argc >= 6 && std::string(argv[1]) == "hypotheses") {
    Scene S;
    if (!read_scene(argv[2], S)) return 2;
    const int T = std::atoi(argv[3]);
    const double thr = std::atof(argv[4]);
    if (S.n < 4 || T <= 0) return 2;
    const std::vector<int32_t> sub = hyp_detail::distinct_subsets(S.n, 4, T, std::strtoull(argv[5], nullptr, 0));
    const std::vector<double> na = hyp_detail::normalised_points(S.cam_a, S.xa.data(), S.n), nb = hyp_detail::normalised_points(S.cam_b, S.xb.data(), S.n);
    for (int t = 0; t < T; ++t) print_hypothesis(na, nb, S.n, &sub[(size_t)t * 4], epi_detail::mean_focal2(S.cam_a, S.cam_b), thr * thr);
    return 0;
  }
  if (argc >= 5 && std::string(argv[1]) == "parallax") {
    std::vector<Scene> pairs;
    if (!read_pairs(argv[2], pairs)) return 2;
    const double thr = std::atof(argv[3]), c = std::atof(argv[4]);
    for (const Scene& S : pairs) {
      int32_t front = 0, par = 0;
      double margin = -1.0;
      if (S.status && S.n > 0) {
        const std::vector<double> na = hyp_detail::normalised_points(S.cam_a, S.xa.data(), S.n), nb = hyp_detail::normalised_points(S.cam_b, S.xb.data(), S.n);
        const double f2 = epi_detail::mean_focal2(S.cam_a, S.cam_b), thr2 = thr * thr;
        homo_detail::parallax_counts(na.data(), nb.data(), S.n, S.E, S.pose, f2, thr2, c, &front, &par);
        double R[9], t[3];
        homo_detail::pose_rt(S.pose, R, t);
        auto take = [&](double v) { v = std::fabs(v); if (margin < 0 || v < margin) margin = v; };
        for (int i = 0; i < S.n; ++i) {
          const double xa = na[2 * (size_t)i], ya = na[2 * (size_t)i + 1], xb = nb[2 * (size_t)i], yb = nb[2 * (size_t)i + 1];
          double d2, pm;
          if (!epi_detail::sampson_inlier(S.E, xa, ya, xb, yb, f2, thr2, &d2)) { take((d2 * f2 - thr2) / thr2); continue; }
          take((d2 * f2 - thr2) / thr2);
          // the two depths of epi_detail::in_front, in units of the baseline
          const double p0 = R[0] * xa + R[1] * ya + R[2], p1 = R[3] * xa + R[4] * ya + R[5], p2 = R[6] * xa + R[7] * ya + R[8];
          const double pp = p0 * p0 + p1 * p1 + p2 * p2, qq = xb * xb + yb * yb + 1.0, pq = p0 * xb + p1 * yb + p2;
          const double pt = p0 * t[0] + p1 * t[1] + p2 * t[2], qt = xb * t[0] + yb * t[1] + t[2], det = pp * qq - pq * pq;
          take((pq * qt - qq * pt) / det); take((pp * qt - pq * pt) / det);
          if (!epi_detail::in_front(R, t, 1.0, xa, ya, xb, yb)) continue;
          homo_detail::has_parallax(R, xa, ya, xb, yb, c, &pm);
          take(pm);
        }
      }
      std::printf("%d %d %.17g\n", front, par, margin);
    }
    return 0;
  }
  if (argc >= 9 && std::string(argv[1]) == "classify") {
    std::vector<Scene> scenes;
    if (!read_pairs(argv[2], scenes)) return 2;
    TwoViewOptions opt;
    opt.iterations = std::atoi(argv[3]); opt.threshold_px = std::atof(argv[4]); opt.refits = std::atoi(argv[5]); opt.min_inliers = std::atoi(argv[6]);
    opt.rng_state = std::strtoull(argv[7], nullptr, 0); opt.hypotheses_on_device = false;
    ClassifyOptions co;
    co.min_parallax_deg = std::atof(argv[8]);
    if (argc > 9 && std::atoi(argv[9]) == 5) opt.solver = TwoViewOptions::EssentialSolver::FivePoint;
    std::vector<EssentialPair> pairs(scenes.size());
    std::vector<TwoViewResult> results(scenes.size());
    std::vector<PairReport> reports(scenes.size());
    for (size_t p = 0; p < scenes.size(); ++p) {
      const Scene& S = scenes[p];
      pairs[p].xy_a = S.xa.data(); pairs[p].xy_b = S.xb.data(); pairs[p].n = S.n; pairs[p].cam_a = S.cam_a; pairs[p].cam_b = S.cam_b;
      results[p] = epi_detail::host_ransac(S.xa.data(), S.xb.data(), S.n, S.cam_a, S.cam_b, opt);
      PairReport& r = reports[p];
      r.frameA = 0; r.frameB = (int32_t)p + 1; r.correspondences = S.n; r.ok = results[p].ok; r.num_inliers = results[p].num_inliers; r.num_front = results[p].num_front;
      for (int k = 0; k < 9; ++k) r.E[k] = results[p].E[k];
      for (int k = 0; k < 6; ++k) r.pose_b[k] = results[p].pose_b[k];
    }
    const std::vector<PairGeometry> geo = classifyPairs(pairs, results, opt, co);
    for (size_t p = 0; p < scenes.size(); ++p)
      std::printf("%d %d %d %d %s %d %d %d %d %d %d\n", results[p].ok ? 1 : 0, results[p].winner_task, results[p].num_inliers, results[p].num_front, pairKindName(geo[p].kind),
                  geo[p].h_ok ? 1 : 0, geo[p].h_winner_task, geo[p].h_refits_adopted, geo[p].num_h_inliers, geo[p].num_front, geo[p].num_parallax);
    std::printf("pick %d %d\n", pickBootstrapPair(reports), pickBootstrapPair(reports, geo));
    return 0;
  }
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  for (int32_t ci = 0; ci < count; ++ci) {
    int32_t hdr[3]; double cam_a[9], cam_b[9];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(cam_a, 8, 9, f) != 9 || std::fread(cam_b, 8, 9, f) != 9) return 2;
    const int n = hdr[0], T = hdr[1], m = hdr[2];
    if (n < 0 || T < 0 || m < 0) return 2;
    std::vector<float> xa((size_t)n * 2), xb((size_t)n * 2); std::vector<int32_t> sub((size_t)T * m);
    if (std::fread(xa.data(), 4, xa.size(), f) != xa.size() || std::fread(xb.data(), 4, xb.size(), f) != xb.size() || std::fread(sub.data(), 4, sub.size(), f) != sub.size()) return 2;
    for (int32_t s : sub) if (s < 0 || s >= n) return 2;
    const std::vector<double> na = hyp_detail::normalised_points(cam_a, xa.data(), n), nb = hyp_detail::normalised_points(cam_b, xb.data(), n);
    for (int t = 0; t < T; ++t) {
      double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      const bool ok = homo_detail::dlt(na.data(), nb.data(), &sub[(size_t)t * m], m, H);
      std::printf("%d", ok ? 1 : 0);
      for (double x : H) std::printf(" %.17g", x);
      std::printf("\n");
    }
  }
  std::fclose(f);
  return 0;
}
