// The scene of the DLT timing tools (pnp_dlt_time.hip, pnp_gs_e2e.cpp): n points in front of one camera, observed with distortion and
// half a pixel of noise, a fifth of them outliers; six-point subsets from the generator solveGsPnPRansac uses.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

struct PnpTimeScene {
  double cam[9] = {800.0, 800.0, -0.05, 0.01, 1e-3, -1e-3, 2e-3, 640.0, 360.0};
  std::vector<float> X, xy;
  uint64_t state = 0x2545f4914f6cdd1dULL;
  double uniform() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0; }
  double normal() { return std::sqrt(-2.0 * std::log(1.0 - uniform())) * std::cos(6.283185307179586 * uniform()); }
  explicit PnpTimeScene(int n) : X((size_t)n * 3), xy((size_t)n * 2) {
    const double c[3] = {0.3, -0.2, 0.1}, w[3] = {0.04, -0.06, 0.03};   // small rotation: x_cam ~ (I + [w]x)(X - c), exact enough for a timing scene
    for (int i = 0; i < n; ++i) {
      const double P[3] = {-5 + 10 * uniform(), -3 + 6 * uniform(), 6 + 8 * uniform()};
      const double d[3] = {P[0] - c[0], P[1] - c[1], P[2] - c[2]};
      const double q[3] = {d[0] + w[1] * d[2] - w[2] * d[1], d[1] + w[2] * d[0] - w[0] * d[2], d[2] + w[0] * d[1] - w[1] * d[0]};
      const double x = q[0] / q[2], y = q[1] / q[2], r2 = x * x + y * y, dd = 1 + r2 * (cam[2] + r2 * (cam[3] + r2 * cam[6]));
      double u = cam[0] * (dd * x + 2 * cam[4] * x * y + cam[5] * (r2 + 2 * x * x)) + cam[7], v = cam[1] * (dd * y + cam[4] * (r2 + 2 * y * y) + 2 * cam[5] * x * y) + cam[8];
      u += 0.5 * normal(); v += 0.5 * normal();
      if (uniform() < 0.2) { u += 40 * normal(); v += 40 * normal(); }
      for (int k = 0; k < 3; ++k) X[(size_t)i * 3 + k] = (float)P[k];
      xy[(size_t)i * 2] = (float)u; xy[(size_t)i * 2 + 1] = (float)v;
    }
  }
  std::vector<int32_t> subsets(int T, int m) const {
    const int n = (int)(X.size() / 3);
    uint64_t s = 0x9e3779b97f4a7c15ULL;
    auto next = [&] { s = (uint64_t)(unsigned)s * 4164903690ULL + (unsigned)(s >> 32); return (unsigned)s; };
    std::vector<int32_t> out((size_t)T * m);
    for (int t = 0; t < T; ++t)
      for (int k = 0; k < m;) {
        const int c = (int)(next() % (unsigned)n); bool dup = false;
        for (int j = 0; j < k; ++j) dup = dup || out[(size_t)t * m + j] == c;
        if (!dup) out[(size_t)t * m + k++] = c;
      }
    return out;
  }
};
