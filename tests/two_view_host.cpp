// Prints what the host definitions of include/rsba/two_view.hpp (epi_detail::eight_point, score, host_ransac) return for the cases of
// tests/two_view_reference.py (test_two_view_reference.py compiles and runs this; no device, and nothing of librsba_amd is called).
//   two_view_host <cases.bin> [mode] [threshold_px]
//     cases.bin: int32 count; per case int32 n, T, m, double cam_a[9], cam_b[9], float xy_a[n][2], xy_b[n][2], int32 subsets[T][m]
//     mode 0 (default) eight_point as it is; the seeded errors of the test, composed from the same pieces:
//     mode 1 no Hartley normalisation, mode 2 the manifold projection dropped (the matrix only scaled), mode 3 E transposed
//     stdout, per subset: "<status> <E[0..9)> <score status> <num_inliers> <num_front[0..4)> <winner> <pose[0..6)> <margin>", margin = the
//     smallest |d^2 f^2 - thr^2| / thr^2 over the n correspondences (how far the nearest one is from changing sides)
//   two_view_host ransac <scene.bin> <iterations> <threshold_px> <refits> <min_inliers> <rng_state>
//     scene.bin: int32 n, double cam_a[9], cam_b[9], float xy_a[n][2], xy_b[n][2]
//     stdout: "<ok> <winner_task> <num_inliers> <num_front> <refits_adopted>", E, pose_b, the inlier flags, d^2 f^2 / thr^2 per correspondence
//   two_view_host hypotheses <scene.bin> <T> <threshold_px> <rng_state>   the per-subset lines above for the first T subsets of the RANSAC
//   two_view_host subsets <n> <m> <iterations> <rng_state>   prints hyp_detail::distinct_subsets, one subset per line
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rsba/two_view.hpp"

using namespace rsba_amd;
using namespace rsba_amd::epi_detail;

// eight_point with one seeded error
static bool seeded(const double* na, const double* nb, const int32_t* idx, int m, int mode, double E[9]) {
  if (m < 8) return false;
  for (int i = 0; i < m; ++i) for (int k = i + 1; k < m; ++k) if (idx[i] == idx[k]) return false;
  Hartley H;
  double F[9], out[9];
  if (!hartley(na, nb, idx, m, H)) return false;
  if (mode == 1) { H.ca[0] = H.ca[1] = H.cb[0] = H.cb[1] = 0.0; H.sa = H.sb = 1.0; }
  if (!null_matrix(na, nb, idx, m, H, F)) return false;
  if (mode == 2) {
    double fro = 0.0;
    for (double x : F) fro += x * x;
    for (int k = 0; k < 9; ++k) out[k] = F[k] / std::sqrt(0.5 * fro);
  } else if (!project_essential(F, out)) return false;
  if (mode == 3) { const double tr[9] = {out[0], out[3], out[6], out[1], out[4], out[7], out[2], out[5], out[8]}; for (int k = 0; k < 9; ++k) out[k] = tr[k]; }
  if (!signed_finite(out)) return false;
  for (int k = 0; k < 9; ++k) E[k] = out[k];
  return true;
}

static void print_subset(const std::vector<double>& na, const std::vector<double>& nb, int n, const int32_t* idx, int m, int mode, double f2, double thr2) {
  double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, pose[6] = {0, 0, 0, 0, 0, 0}, margin = -1.0;
  int32_t inl = 0, front[4] = {0, 0, 0, 0};
  int winner = -1;
  const bool ok = mode == 0 ? eight_point(na.data(), nb.data(), idx, m, E) : seeded(na.data(), nb.data(), idx, m, mode, E);
  const bool scored = ok && score(na.data(), nb.data(), n, E, f2, thr2, &inl, front, pose, &winner);
  if (scored)
    for (int i = 0; i < n; ++i) {
      double d2;
      sampson_inlier(E, na[2 * (size_t)i], na[2 * (size_t)i + 1], nb[2 * (size_t)i], nb[2 * (size_t)i + 1], f2, thr2, &d2);
      const double rel = std::fabs(d2 * f2 - thr2) / thr2;
      if (margin < 0 || rel < margin) margin = rel;
    }
  std::printf("%d", ok ? 1 : 0);
  for (double x : E) std::printf(" %.17g", x);
  std::printf(" %d %d %d %d %d %d %d", scored ? 1 : 0, inl, front[0], front[1], front[2], front[3], winner);
  for (double x : pose) std::printf(" %.17g", x);
  std::printf(" %.17g\n", margin);
}

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

int main(int argc, char** argv) {
  if (argc >= 6 && std::string(argv[1]) == "subsets") {
    const int n = std::atoi(argv[2]), m = std::atoi(argv[3]), it = std::atoi(argv[4]);
    const std::vector<int32_t> s = hyp_detail::distinct_subsets(n, m, it, std::strtoull(argv[5], nullptr, 0));
    for (int t = 0; t < it; ++t) { for (int k = 0; k < m; ++k) std::printf("%d ", s[(size_t)t * m + k]); std::printf("\n"); }
    return 0;
  }
  if (argc >= 8 && std::string(argv[1]) == "ransac") {
    Scene S;
    if (!read_scene(argv[2], S)) return 2;
    TwoViewOptions opt;
    opt.iterations = std::atoi(argv[3]); opt.threshold_px = std::atof(argv[4]); opt.refits = std::atoi(argv[5]); opt.min_inliers = std::atoi(argv[6]);
    opt.rng_state = std::strtoull(argv[7], nullptr, 0); opt.hypotheses_on_device = false;
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
    if (S.n < 8 || T <= 0) return 2;
    const std::vector<int32_t> sub = hyp_detail::distinct_subsets(S.n, 8, T, std::strtoull(argv[5], nullptr, 0));
    const std::vector<double> na = hyp_detail::normalised_points(S.cam_a, S.xa.data(), S.n), nb = hyp_detail::normalised_points(S.cam_b, S.xb.data(), S.n);
    for (int t = 0; t < T; ++t) print_subset(na, nb, S.n, &sub[(size_t)t * 8], 8, 0, mean_focal2(S.cam_a, S.cam_b), thr * thr);
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
    if (n < 0 || T < 0 || m < 0) return 2;
    std::vector<float> xa((size_t)n * 2), xb((size_t)n * 2); std::vector<int32_t> sub((size_t)T * m);
    if (std::fread(xa.data(), 4, xa.size(), f) != xa.size() || std::fread(xb.data(), 4, xb.size(), f) != xb.size() || std::fread(sub.data(), 4, sub.size(), f) != sub.size()) return 2;
    for (int32_t s : sub) if (s < 0 || s >= n) return 2;
    const std::vector<double> na = hyp_detail::normalised_points(cam_a, xa.data(), n), nb = hyp_detail::normalised_points(cam_b, xb.data(), n);
    for (int t = 0; t < T; ++t) print_subset(na, nb, n, &sub[(size_t)t * m], m, mode, mean_focal2(cam_a, cam_b), thr * thr);
  }
  std::fclose(f);
  return 0;
}
