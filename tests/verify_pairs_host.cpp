// The host side of the geometric verification of include/rsba/two_view.hpp (findEssentialRansacPairs with the hypotheses from the host
// definitions, verifyMatches, pickBootstrapPair); test_verify_pairs_host.py compiles and runs this.  No device, and nothing of librsba_amd is
// linked: the three entry points the header's inline functions name are defined here, and the batched one ends the program — the host path
// must not reach it.
//   verify_pairs_host pairs <pairs.bin> <which: pairs|single> <iterations> <threshold_px> <refits> <min_inliers> <rng_state> <solver: 8|5>
//     pairs.bin: int32 P; per pair int32 n, double cam_a[9], cam_b[9], float xy_a[n][2], xy_b[n][2]
//     which = pairs: findEssentialRansacPairs(hypotheses_on_device = false); single: epi_detail::host_ransac pair by pair
//     stdout per pair: "<ok> <winner_task> <num_inliers> <num_front> <refits_adopted>", E, pose_b, the inlier flags — one line each
//   verify_pairs_host session <session.bin> <drop_unverified> <iterations> <threshold_px> <refits> <min_inliers> <rng_state> <solver: 8|5>
//     session.bin: int32 F, double cam[9]; per frame int32 has_cam, double cam[9] if so, int32 nobs; per observation double x, y, int32 nm,
//     nm x {int32 frame, int32 obs}
//     stdout: "pairs <P>"; per pair "<frameA> <frameB> <correspondences> <ok> <num_inliers> <num_front> <removed>" then E and pose_b;
//     "bootstrap <pickBootstrapPair>"; per observation with refs left "refs <frame> <obs>" and its refs as "<frame> <obs>" pairs; then
//     "untouched <0|1>": whether everything but the match lists is what it was
//   verify_pairs_host pick {<frameA> <frameB> <ok> <num_front>}...   prints pickBootstrapPair of those reports
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rsba/two_view.hpp"

using namespace rsba_amd;

extern "C" int32_t rsba_epipolar_ransac_pairs(int32_t, const double*, int32_t, const int32_t*, const int32_t*, const int32_t*, int32_t, const float*, const float*,
                                              const int32_t*, int32_t, int32_t, double, int32_t, int32_t, double*, double*, uint8_t*, int32_t*, int32_t*, int32_t*, int32_t*,
                                              uint8_t*) {
  std::fprintf(stderr, "the host path called the device\n");
  std::abort();
}
extern "C" const char* rsba_status_string(int32_t) { return "status"; }
extern "C" const char* rsba_last_error(void) { return ""; }

static TwoViewOptions options(char** a) {   // <iterations> <threshold_px> <refits> <min_inliers> <rng_state> <solver>
  TwoViewOptions opt;
  opt.iterations = std::atoi(a[0]); opt.threshold_px = std::atof(a[1]); opt.refits = std::atoi(a[2]); opt.min_inliers = std::atoi(a[3]);
  opt.rng_state = std::strtoull(a[4], nullptr, 0); opt.hypotheses_on_device = false;
  opt.solver = std::atoi(a[5]) == 5 ? TwoViewOptions::EssentialSolver::FivePoint : TwoViewOptions::EssentialSolver::EightPoint;
  return opt;
}

static void print_result(const TwoViewResult& r) {
  std::printf("%d %d %d %d %d\n", r.ok ? 1 : 0, r.winner_task, r.num_inliers, r.num_front, r.refits_adopted);
  for (double x : r.E) std::printf("%.17g ", x);
  std::printf("\n");
  for (double x : r.pose_b) std::printf("%.17g ", x);
  std::printf("\n");
  for (uint8_t b : r.inliers) std::printf("%d ", (int)b);
  std::printf("\n");
}

static bool same_but_matches(const Session& a, const Session& b) {
  if (a.cam != b.cam || a.frames.size() != b.frames.size() || a.tracks.size() != b.tracks.size() || a.rs != b.rs || a.scanlines != b.scanlines) return false;
  for (size_t f = 0; f < a.frames.size(); ++f) {
    const Frame& x = a.frames[f]; const Frame& y = b.frames[f];
    if (x.poses != y.poses || x.cam != y.cam || x.__isset.cam != y.__isset.cam || x.__isset.poses != y.__isset.poses || x.obs.size() != y.obs.size()) return false;
    for (size_t o = 0; o < x.obs.size(); ++o)
      if (x.obs[o].x != y.obs[o].x || x.obs[o].y != y.obs[o].y || x.obs[o].track != y.obs[o].track || x.obs[o].__isset.track != y.obs[o].__isset.track ||
          x.obs[o].__isset.matches != y.obs[o].__isset.matches) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "pick") {
    std::vector<PairReport> reports;
    for (int i = 2; i + 3 < argc; i += 4) {
      PairReport r;
      r.frameA = std::atoi(argv[i]); r.frameB = std::atoi(argv[i + 1]); r.ok = std::atoi(argv[i + 2]) != 0; r.num_front = std::atoi(argv[i + 3]);
      reports.push_back(r);
    }
    std::printf("%d\n", pickBootstrapPair(reports));
    return 0;
  }
  if (mode == "pairs" && argc >= 10) {
    struct Data { int32_t n = 0; double cam_a[9], cam_b[9]; std::vector<float> xa, xb; };
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    int32_t P = 0;
    if (std::fread(&P, 4, 1, f) != 1 || P < 0) return 2;
    std::vector<Data> data((size_t)P);
    for (Data& d : data) {
      if (std::fread(&d.n, 4, 1, f) != 1 || d.n < 0 || std::fread(d.cam_a, 8, 9, f) != 9 || std::fread(d.cam_b, 8, 9, f) != 9) return 2;
      d.xa.resize((size_t)d.n * 2); d.xb.resize((size_t)d.n * 2);
      if (std::fread(d.xa.data(), 4, d.xa.size(), f) != d.xa.size() || std::fread(d.xb.data(), 4, d.xb.size(), f) != d.xb.size()) return 2;
    }
    std::fclose(f);
    const TwoViewOptions opt = options(argv + 4);
    if (std::string(argv[3]) == "pairs") {
      std::vector<EssentialPair> pairs(data.size());
      for (size_t p = 0; p < data.size(); ++p) pairs[p] = EssentialPair{data[p].xa.data(), data[p].xb.data(), data[p].n, data[p].cam_a, data[p].cam_b};
      for (const TwoViewResult& r : findEssentialRansacPairs(pairs, opt)) print_result(r);
    } else {
      for (const Data& d : data) print_result(epi_detail::host_ransac(d.xa.data(), d.xb.data(), d.n, d.cam_a, d.cam_b, opt));
    }
    return 0;
  }
  if (mode == "session" && argc >= 10) {
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    Session sess;
    int32_t F = 0;
    if (std::fread(&F, 4, 1, f) != 1 || F < 0 || std::fread(sess.cam.data(), 8, 9, f) != 9) return 2;
    sess.frames.resize((size_t)F);
    for (Frame& fr : sess.frames) {
      int32_t has_cam = 0, nobs = 0;
      if (std::fread(&has_cam, 4, 1, f) != 1) return 2;
      if (has_cam) { fr.cam.resize(9); fr.__isset.cam = true; if (std::fread(fr.cam.data(), 8, 9, f) != 9) return 2; }
      if (std::fread(&nobs, 4, 1, f) != 1 || nobs < 0) return 2;
      fr.obs.resize((size_t)nobs);
      for (Observation& o : fr.obs) {
        int32_t nm = 0;
        if (std::fread(&o.x, 8, 1, f) != 1 || std::fread(&o.y, 8, 1, f) != 1 || std::fread(&nm, 4, 1, f) != 1 || nm < 0) return 2;
        o.matches.resize((size_t)nm);
        o.__isset.matches = nm > 0;
        for (ObservationRef& r : o.matches) if (std::fread(&r.frame, 4, 1, f) != 1 || std::fread(&r.obs, 4, 1, f) != 1) return 2;
      }
    }
    std::fclose(f);
    VerifyOptions vo;
    vo.drop_unverified = std::atoi(argv[3]) != 0;
    const Session before = sess;
    const std::vector<PairReport> reports = verifyMatches(sess, options(argv + 4), 0, vo);
    std::printf("pairs %zu\n", reports.size());
    for (const PairReport& r : reports) {
      std::printf("%d %d %d %d %d %d %d", r.frameA, r.frameB, r.correspondences, r.ok ? 1 : 0, r.num_inliers, r.num_front, r.removed);
      for (double x : r.E) std::printf(" %.17g", x);
      for (double x : r.pose_b) std::printf(" %.17g", x);
      std::printf("\n");
    }
    std::printf("bootstrap %d\n", pickBootstrapPair(reports));
    for (size_t fi = 0; fi < sess.frames.size(); ++fi)
      for (size_t o = 0; o < sess.frames[fi].obs.size(); ++o) {
        const std::vector<ObservationRef>& list = sess.frames[fi].obs[o].matches;
        if (list.empty()) continue;
        std::printf("refs %zu %zu", fi, o);
        for (const ObservationRef& ref : list) std::printf(" %d %d", ref.frame, ref.obs);
        std::printf("\n");
      }
    std::printf("untouched %d\n", same_but_matches(before, sess) ? 1 : 0);
    return 0;
  }
  return 2;
}
