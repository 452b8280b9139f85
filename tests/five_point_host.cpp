// Prints what the host definitions of the five-point solver (include/rsba/two_view.hpp: epi_detail::five_point, five_point_hypothesis,
// host_ransac with solver = FivePoint) return for the cases of tests/five_point_reference.py (test_five_point_reference.py compiles and
// runs this; no device, and nothing of librsba_amd is called).
//   five_point_host <cases.bin> [mode] [threshold_px]
//     cases.bin: as tests/two_view_host.cpp reads it, with m = 5
//     mode 0 (default) five_point as it is; the seeded errors of the test: mode 1 the factor 1/2 of the trace term dropped, mode 2 E
//     transposed (the constraint rows built for a^T E b), mode 3 no Newton steps after the bisection and no polish on the cubics
//     stdout, per subset: "<status> <count> <rank_ratio> <pivot_ratio> <E[0..90)> <chain status> <chosen> <num_inliers> <num_front[0..4)> <pose[0..6)>"
//     (slots past count are zero; the chain — every solution scored, the best kept — is printed for mode 0 only)
//   five_point_host ransac <scene.bin> <iterations> <threshold_px> <refits> <min_inliers> <rng_state> <solver: 8 | 5>
//     scene.bin and stdout as two_view_host's ransac
//   five_point_host hypotheses <scene.bin> <T> <threshold_px> <rng_state>   the chain of the first T five-point subsets of the RANSAC:
//     "<status> <num_solutions> <num_inliers> <num_front[0..4)> <E[0..9)> <pose[0..6)>" per subset
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rsba/two_view.hpp"

using namespace rsba_amd;
using namespace rsba_amd::epi_detail;

struct Scene { int n = 0; double cam_a[9], cam_b[9]; std::vector<float> xa, xb; };
static bool read_scene(const char* path, Scene& S) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  int32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1 && n >= 0 && std::fread(S.cam_a, 8, 9, f) == 9 && std::fread(S.cam_b, 8, 9, f) == 9;
  if (ok) {
    S.n = n; S.xa.resize((size_t)n * 2); S.xb.resize((size_t)n * 2);
    ok = std::fread(S.xa.data(), 4, S.xa.size(), f) == S.xa.size() && std::fread(S.xb.data(), 4, S.xb.size(), f) == S.xb.size();
  }
  std::fclose(f);
  return ok;
}

static void print_subset(const std::vector<double>& na, const std::vector<double>& nb, int n, const int32_t* idx, int mode, double f2, double thr2) {
  double E[10][9] = {}, one[9] = {}, pose[6] = {};
  int count = 0, chosen = -1;
  int32_t inl = 0, front[4] = {0, 0, 0, 0};
  FivePointDiag diag;
  const bool ok = five_point(na.data(), nb.data(), idx, E, &count, &diag, mode == 1 ? 1.0 : 0.5, mode == 2, mode == 3 ? 0 : kFiveNewton);
  const bool chain = mode == 0 && five_point_hypothesis(na.data(), nb.data(), n, idx, f2, thr2, one, pose, &inl, front, nullptr, &chosen);
  std::printf("%d %d %.17g %.17g", ok ? 1 : 0, ok ? count : 0, diag.rank_ratio, diag.pivot_ratio);
  for (int s = 0; s < 10; ++s) for (double x : E[s]) std::printf(" %.17g", ok && s < count ? x : 0.0);
  std::printf(" %d %d %d %d %d %d %d", chain ? 1 : 0, chosen, inl, front[0], front[1], front[2], front[3]);
  for (double x : pose) std::printf(" %.17g", x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc >= 9 && std::string(argv[1]) == "ransac") {
    Scene S;
    if (!read_scene(argv[2], S)) return 2;
    TwoViewOptions opt;
    opt.iterations = std::atoi(argv[3]); opt.threshold_px = std::atof(argv[4]); opt.refits = std::atoi(argv[5]); opt.min_inliers = std::atoi(argv[6]);
    opt.rng_state = std::strtoull(argv[7], nullptr, 0); opt.hypotheses_on_device = false;
    opt.solver = std::atoi(argv[8]) == 5 ? TwoViewOptions::EssentialSolver::FivePoint : TwoViewOptions::EssentialSolver::EightPoint;
    const TwoViewResult r = host_ransac(S.xa.data(), S.xb.data(), S.n, S.cam_a, S.cam_b, opt);
    std::printf("%d %d %d %d %d\n", r.ok ? 1 : 0, r.winner_task, r.num_inliers, r.num_front, r.refits_adopted);
    for (double x : r.E) std::printf("%.17g ", x);
    std::printf("\n");
    for (double x : r.pose_b) std::printf("%.17g ", x);
    std::printf("\n");
    for (uint8_t b : r.inliers) std::printf("%d ", (int)b);
    std::printf("\n");
    const std::vector<double> na = hyp_detail::normalised_points(S.cam_a, S.xa.data(), S.n), nb = hyp_detail::normalised_points(S.cam_b, S.xb.data(), S.n);
    const double f2 = mean_focal2(S.cam_a, S.cam_b), thr2 = opt.threshold_px * opt.threshold_px;
    for (int i = 0; i < S.n; ++i) {
      double d2 = 0.0;
      if (r.winner_task >= 0) sampson_inlier(r.E, na[2 * (size_t)i], na[2 * (size_t)i + 1], nb[2 * (size_t)i], nb[2 * (size_t)i + 1], f2, thr2, &d2);
      std::printf("%.17g ", d2 * f2 / thr2);
    }
    std::printf("\n");
    return 0;
  }
  if (argc >= 6 && std::string(argv[1]) == "hypotheses") {
    Scene S;
    if (!read_scene(argv[2], S)) return 2;
    const int T = std::atoi(argv[3]);
    const double thr = std::atof(argv[4]);
    if (S.n < 5 || T <= 0) return 2;
    const std::vector<int32_t> sub = hyp_detail::distinct_subsets(S.n, 5, T, std::strtoull(argv[5], nullptr, 0));
    const std::vector<double> na = hyp_detail::normalised_points(S.cam_a, S.xa.data(), S.n), nb = hyp_detail::normalised_points(S.cam_b, S.xb.data(), S.n);
    for (int t = 0; t < T; ++t) {
      double E[9] = {}, pose[6] = {};
      int32_t inl = 0, front[4] = {0, 0, 0, 0};
      int ns = 0;
      const bool ok = five_point_hypothesis(na.data(), nb.data(), S.n, &sub[(size_t)t * 5], mean_focal2(S.cam_a, S.cam_b), thr * thr, E, pose, &inl, front, &ns);
      std::printf("%d %d %d %d %d %d %d", ok ? 1 : 0, ns, inl, front[0], front[1], front[2], front[3]);
      for (double x : E) std::printf(" %.17g", x);
      for (double x : pose) std::printf(" %.17g", x);
      std::printf("\n");
    }
    return 0;
  }
  if (argc < 2) return 2;
  const int mode = argc > 2 ? std::atoi(argv[2]) : 0;
  const double thr = argc > 3 ? std::atof(argv[3]) : 4.0;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  for (int32_t ci = 0; ci < count; ++ci) {
    int32_t hdr[3]; double cam_a[9], cam_b[9];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(cam_a, 8, 9, f) != 9 || std::fread(cam_b, 8, 9, f) != 9) return 2;
    const int n = hdr[0], T = hdr[1], m = hdr[2];
    if (n < 0 || T < 0 || m != 5) return 2;
    std::vector<float> xa((size_t)n * 2), xb((size_t)n * 2); std::vector<int32_t> sub((size_t)T * m);
    if (std::fread(xa.data(), 4, xa.size(), f) != xa.size() || std::fread(xb.data(), 4, xb.size(), f) != xb.size() || std::fread(sub.data(), 4, sub.size(), f) != sub.size()) return 2;
    for (int32_t s : sub) if (s < 0 || s >= n) return 2;
    const std::vector<double> na = hyp_detail::normalised_points(cam_a, xa.data(), n), nb = hyp_detail::normalised_points(cam_b, xb.data(), n);
    for (int t = 0; t < T; ++t) print_subset(na, nb, n, &sub[(size_t)t * m], mode, mean_focal2(cam_a, cam_b), thr * thr);
  }
  std::fclose(f);
  return 0;
}
