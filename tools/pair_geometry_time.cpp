// Times the batched degeneracy test (classifyPairs -> rsba_two_view_classify_pairs: the homography RANSAC and the parallax counts of many frame
// pairs) beside the batched essential-matrix RANSAC on the same pairs (findEssentialRansacPairs -> rsba_epipolar_ransac_pairs, eight-point
// subsets), and beside P sequential findHomographyRansac calls, in one process on one box (tools/pair_geometry_time.py builds and runs
// this).  A host program over the C ABI.
//   Shapes: those of tools/verify_pairs_time.cpp — P = 1, 16, 256 pairs x 1 024 subsets x 500 correspondences (a pinhole camera, 30 % of frame
//   B's points replaced by random ones, 0.3 px of noise, another scene per pair), three refits.  Three warm-ups, ten timed repetitions of
//   each, wall clock around the whole call(s): the median with min .. max, one JSON line per shape.  The batched homographies are compared
//   with the sequential ones pair by pair on the way (the "equal" field).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "rsba/pair_geometry.hpp"

using namespace rsba_amd;

struct Lcg {
  uint64_t s;
  double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0; }
  double normal() { const double u = next() + 1e-300, v = next(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); }
};

struct Scene { std::vector<float> xa, xb; };
static const double kCam[9] = {900.0, 900.0, 0, 0, 0, 0, 0, 640.0, 360.0};

static Scene make_scene(int n, uint64_t seed) {   // (tools/verify_pairs_time.cpp's)
  Lcg g{seed * 2654435761ULL + 12345};
  const double w[3] = {0.04 * (g.next() - 0.5), 0.2 * (g.next() - 0.5), 0.04 * (g.next() - 0.5)}, c[3] = {0.8 + 0.4 * g.next(), 0.2 * (g.next() - 0.5), 0.3 * (g.next() - 0.5)};
  Scene s;
  for (int i = 0; i < n; ++i) {
    const double X[3] = {6.0 * (g.next() - 0.5), 4.0 * (g.next() - 0.5), 5.0 + 6.0 * g.next()};
    const double d[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
    double Y[3];
    hyp_detail::rotate(w, d, Y);
    s.xa.push_back((float)(kCam[0] * X[0] / X[2] + kCam[7] + 0.3 * g.normal())); s.xa.push_back((float)(kCam[1] * X[1] / X[2] + kCam[8] + 0.3 * g.normal()));
    if (g.next() < 0.3) { s.xb.push_back((float)(1280.0 * g.next())); s.xb.push_back((float)(720.0 * g.next())); }
    else { s.xb.push_back((float)(kCam[0] * Y[0] / Y[2] + kCam[7] + 0.3 * g.normal())); s.xb.push_back((float)(kCam[1] * Y[1] / Y[2] + kCam[8] + 0.3 * g.normal())); }
  }
  return s;
}

template <class F> static void timed(F&& f, double out[3]) {
  std::vector<double> ms;
  for (int rep = 0; rep < 13; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    f();
    const auto t1 = std::chrono::steady_clock::now();
    if (rep >= 3) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  out[0] = 0.5 * (ms[4] + ms[5]); out[1] = ms.front(); out[2] = ms.back();
}

static bool same(const PairGeometry& g, const HomographyResult& h) {
  bool eq = g.h_ok == h.ok && g.h_winner_task == h.winner_task && g.num_h_inliers == h.num_inliers && g.h_refits_adopted == h.refits_adopted && g.h_inliers == h.inliers;
  for (int k = 0; k < 9; ++k) eq = eq && g.H[k] == h.H[k];
  return eq;
}

int main() {
  const int n = 500;
  try {
    for (int P : {1, 16, 256}) {
      std::vector<Scene> scenes;
      for (int p = 0; p < P; ++p) scenes.push_back(make_scene(n, (uint64_t)p + 1));
      std::vector<EssentialPair> pairs((size_t)P);
      for (int p = 0; p < P; ++p) pairs[(size_t)p] = EssentialPair{scenes[(size_t)p].xa.data(), scenes[(size_t)p].xb.data(), n, kCam, kCam};
      TwoViewOptions tv;
      tv.iterations = 1024; tv.refits = 3;
      ClassifyOptions co;
      std::vector<TwoViewResult> essential;
      std::vector<PairGeometry> geometry;
      std::vector<HomographyResult> sequential((size_t)P);
      double te[3], tc[3], ts[3];
      timed([&] { essential = findEssentialRansacPairs(pairs, tv, 0); }, te);
      timed([&] { geometry = classifyPairs(pairs, essential, tv, co, 0); }, tc);
      timed([&] { for (int p = 0; p < P; ++p) sequential[(size_t)p] = findHomographyRansac(pairs[(size_t)p].xy_a, pairs[(size_t)p].xy_b, n, kCam, kCam, tv, 0); }, ts);
      int equal = 0, general = 0;
      for (int p = 0; p < P; ++p) { equal += same(geometry[(size_t)p], sequential[(size_t)p]) ? 1 : 0; general += geometry[(size_t)p].kind == PairKind::General ? 1 : 0; }
      std::printf("{\"pairs\": %d, \"subsets\": 1024, \"correspondences\": %d, \"refits\": 3, \"epipolar_pairs_ms\": %.3f, \"epipolar_pairs_min_ms\": %.3f, \"epipolar_pairs_max_ms\": %.3f, "
                  "\"classify_pairs_ms\": %.3f, \"classify_pairs_min_ms\": %.3f, \"classify_pairs_max_ms\": %.3f, \"sequential_homography_ms\": %.3f, \"sequential_homography_min_ms\": %.3f, "
                  "\"sequential_homography_max_ms\": %.3f, \"classify_over_epipolar\": %.2f, \"speedup_over_sequential\": %.2f, \"equal\": %d, \"general\": %d}\n",
                  P, n, te[0], te[1], te[2], tc[0], tc[1], tc[2], ts[0], ts[1], ts[2], tc[0] / te[0], ts[0] / tc[0], equal, general);
      std::fflush(stdout);
    }
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 3; }
  return 0;
}
