// Prints what the host pnp_detail::p3p_pose (include/rsba/solve_rs_pnp.hpp) returns for the cases of tests/p3p_reference.py
// (test_p3p_reference.py compiles and runs this; no device, and nothing of librsba_amd is called).
//   p3p_host <cases.bin> [mode]   cases.bin: int32 count; per case int32 n, T, double cam[9], float X[n][3], float xy[n][2], int32 subsets[T][4]
//     mode 0 (default) p3p_pose as it is; the seeded errors of the test, composed from the same pieces:
//     mode 1 the runner-up solution is chosen, mode 2 the polish of the depths is dropped, mode 3 the bearing (x, y, 1) is not normalised
//   p3p_host subsets <n> <m> <iterations> <rng_state>   prints hyp_detail::distinct_subsets, one subset per line
//   stdout, per subset: "<status 0|1> <num_solutions> <pose[0..6) %.17g>"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rsba/solve_rs_pnp.hpp"

using namespace rsba_amd::pnp_detail;

// p3p_pose with one seeded error
static bool seeded(const float* X, const double* nrm, const int32_t idx[4], int mode, double pose[6], int* num) {
  *num = 0;
  for (int i = 0; i < 4; ++i) for (int k = i + 1; k < 4; ++k) if (idx[i] == idx[k]) return false;
  double P[3][3], j[3][3];
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) P[i][k] = X[3 * (size_t)idx[i] + k];
    p3p_bearing(nrm[2 * (size_t)idx[i]], nrm[2 * (size_t)idx[i] + 1], j[i]);
    if (mode == 3) { j[i][0] = nrm[2 * (size_t)idx[i]]; j[i][1] = nrm[2 * (size_t)idx[i] + 1]; j[i][2] = 1.0; }
  }
  P3pProblem S;
  if (!p3p_setup(P, j, S)) return false;
  const double X4[3] = {X[3 * (size_t)idx[3]], X[3 * (size_t)idx[3] + 1], X[3 * (size_t)idx[3] + 2]};
  double roots[4], dist[4], depth_of[4][3];
  const int count = p3p_roots(S, roots);
  int found = 0;
  for (int i = 0; i < count; ++i) {
    double s[3], R[9], tvec[3], d2;
    if (!p3p_depths(S, roots[i], s) || (mode != 2 && !p3p_polish(S, s))) continue;
    p3p_rt(S, s, R, tvec);
    if (!p3p_fourth(R, tvec, X4, nrm[2 * (size_t)idx[3]], nrm[2 * (size_t)idx[3] + 1], &d2)) continue;
    dist[found] = d2; for (int k = 0; k < 3; ++k) depth_of[found][k] = s[k]; ++found;
  }
  if (found == 0) return false;
  int best = 0, second = -1;
  for (int i = 1; i < found; ++i) if (dist[i] < dist[best]) best = i;
  for (int i = 0; i < found; ++i) if (i != best && (second < 0 || dist[i] < dist[second])) second = i;
  double R[9], tvec[3];
  p3p_rt(S, depth_of[mode == 1 && second >= 0 ? second : best], R, tvec);
  if (!rsba_amd::hyp_detail::pose_from_rt(R, tvec, pose)) return false;
  *num = found;
  return true;
}

int main(int argc, char** argv) {
  if (argc >= 6 && std::string(argv[1]) == "subsets") {
    const int n = std::atoi(argv[2]), m = std::atoi(argv[3]), it = std::atoi(argv[4]);
    const std::vector<int32_t> s = rsba_amd::hyp_detail::distinct_subsets(n, m, it, std::strtoull(argv[5], nullptr, 0));
    for (int t = 0; t < it; ++t) { for (int k = 0; k < m; ++k) std::printf("%d ", s[(size_t)t * m + k]); std::printf("\n"); }
    return 0;
  }
  if (argc < 2) return 2;
  const int mode = argc > 2 ? std::atoi(argv[2]) : 0;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  for (int32_t ci = 0; ci < count; ++ci) {
    int32_t hdr[2]; double cam[9];
    if (std::fread(hdr, 4, 2, f) != 2 || std::fread(cam, 8, 9, f) != 9) return 2;
    const int n = hdr[0], T = hdr[1];
    if (n < 0 || T < 0) return 2;
    std::vector<float> X((size_t)n * 3), xy((size_t)n * 2); std::vector<int32_t> sub((size_t)T * 4);
    if (std::fread(X.data(), 4, X.size(), f) != X.size() || std::fread(xy.data(), 4, xy.size(), f) != xy.size() || std::fread(sub.data(), 4, sub.size(), f) != sub.size()) return 2;
    for (int32_t s : sub) if (s < 0 || s >= n) return 2;
    const std::vector<double> nrm = rsba_amd::hyp_detail::normalised_points(cam, xy.data(), n);
    for (int t = 0; t < T; ++t) {
      double p[6] = {0, 0, 0, 0, 0, 0};
      int num = 0;
      const bool ok = mode == 0 ? p3p_pose(X.data(), nrm.data(), &sub[(size_t)t * 4], p, &num) : seeded(X.data(), nrm.data(), &sub[(size_t)t * 4], mode, p, &num);
      std::printf("%d %d %.17g %.17g %.17g %.17g %.17g %.17g\n", ok ? 1 : 0, num, p[0], p[1], p[2], p[3], p[4], p[5]);
    }
  }
  std::fclose(f);
  return 0;
}
