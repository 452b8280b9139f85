// Prints what the host pnp_detail::dlt_pose (include/rsba/solve_rs_pnp.hpp) returns for the cases of tests/pnp_dlt_reference.py
// (test_pnp_dlt_reference.py compiles and runs this; no device, and nothing of librsba_amd is called).
//   pnp_dlt_host <cases.bin>      cases.bin: int32 count; per case int32 n, m, T, double cam[9], float X[n][3], float xy[n][2], int32 subsets[T][m]
//   stdout, per subset: "<accepted 0|1> <pose[0..6) %.17g>"
#include <cstdio>
#include <vector>

#include "rsba/solve_rs_pnp.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  for (int32_t ci = 0; ci < count; ++ci) {
    int32_t hdr[3]; double cam[9];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(cam, 8, 9, f) != 9) return 2;
    const int n = hdr[0], m = hdr[1], T = hdr[2];
    std::vector<float> X((size_t)n * 3), xy((size_t)n * 2); std::vector<int32_t> sub((size_t)T * m);
    if (std::fread(X.data(), 4, X.size(), f) != X.size() || std::fread(xy.data(), 4, xy.size(), f) != xy.size() || std::fread(sub.data(), 4, sub.size(), f) != sub.size()) return 2;
    const std::vector<double> nrm = rsba_amd::hyp_detail::normalised_points(cam, xy.data(), n);
    for (int t = 0; t < T; ++t) {
      double p[6] = {0, 0, 0, 0, 0, 0};
      const bool ok = rsba_amd::pnp_detail::dlt_pose(X.data(), nrm.data(), &sub[(size_t)t * m], m, p);
      std::printf("%d %.17g %.17g %.17g %.17g %.17g %.17g\n", ok ? 1 : 0, p[0], p[1], p[2], p[3], p[4], p[5]);
    }
  }
  std::fclose(f);
  return 0;
}
