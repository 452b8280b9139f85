// What kind of geometry the matched frame pairs of a Session cache have (include/rsba/pair_geometry.hpp: classifyMatches, pickBootstrapPair):
// loads a cache (VideoSfMCache, Thrift binary; include/rsba/session_cache.hpp), verifies the matches (verifyMatches: the essential-matrix
// RANSAC of every pair in one batched device call, the outliers erased), then classifies every pair — the homography RANSAC and the parallax
// counts of all pairs in one more batched call — and prints a line per pair and the bootstrap pair with and without the geometry.  The
// session is not written back: classifyMatches touches nothing in it.
//
//   classify_pairs <session.cache> [key=value ...]
//     keys: iterations (1000), threshold (4), refits (3), minInliers (16), seed (0x9e3779b97f4a7c15), solver (eight_point; five_point),
//           hostHypotheses (0; 1: both RANSACs from the host definitions, no device), maxTasks (0: the library's default of tasks per launch),
//           minParallaxDeg (16), minParallaxShare (0.5), maxHRatio (0.8), allowPlanar (0)
//     stdout: "pairs <P>"; per pair "<frameA> <frameB> <correspondences> <ok> <inliers> <in front> <kind> <h ok> <h inliers> <front> <with
//     parallax>"; "bootstrap <pickBootstrapPair(reports)> <pickBootstrapPair(reports, geometry)>"; "untouched <1: classifyMatches left every
//     observation's refs as they were>"
//   classify_pairs pairs <pairs.bin> <batched|sequential> <iterations> <threshold> <refits> <minInliers> <seed> <hostHypotheses> <solver> <minParallaxDeg> [maxTasks]
//     findEssentialRansacPairs and classifyPairs (batched), or pair by pair findEssentialRansac, findHomographyRansac and the host parallax
//     counts (sequential), on plain arrays.  pairs.bin: int32 P; per pair int32 n, int32 (not read), double cam_a[9], cam_b[9], 15 doubles (not
//     read), float xy_a[n][2], xy_b[n][2].  stdout per pair: "<essential ok> <kind> <h ok> <h winner task> <h refits adopted> <h inliers> <front>
//     <with parallax>", H, the homography's inlier flags — one line each
//   exit status: 0 done, 2 bad input, 3 something threw (message on stderr)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "rsba/pair_geometry.hpp"
#include "rsba/session_cache.hpp"

using namespace rsba_amd;

static bool parse_solver(const std::string& name, TwoViewOptions& tv) {
  if (name == "five_point") tv.solver = TwoViewOptions::EssentialSolver::FivePoint;
  else if (name == "eight_point") tv.solver = TwoViewOptions::EssentialSolver::EightPoint;
  else { std::fprintf(stderr, "solver is eight_point or five_point\n"); return false; }
  return true;
}

static void print_geometry(bool essential_ok, const PairGeometry& g) {
  std::printf("%d %s %d %d %d %d %d %d\n", essential_ok ? 1 : 0, pairKindName(g.kind), g.h_ok ? 1 : 0, g.h_winner_task, g.h_refits_adopted, g.num_h_inliers, g.num_front,
              g.num_parallax);
  for (double x : g.H) std::printf("%.17g ", x);
  std::printf("\n");
  for (uint8_t b : g.h_inliers) std::printf("%d ", (int)b);
  std::printf("\n");
}

static int pairs_only(int argc, char** argv) {
  if (argc < 12) {
    std::fprintf(stderr, "usage: %s pairs <pairs.bin> <batched|sequential> <iterations> <threshold> <refits> <minInliers> <seed> <hostHypotheses> <solver> <minParallaxDeg> [maxTasks]\n", argv[0]);
    return 2;
  }
  struct Data { int32_t n = 0; double cam_a[9], cam_b[9]; std::vector<float> xa, xb; };
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::perror("pairs"); return 2; }
  int32_t P = 0;
  bool ok = std::fread(&P, 4, 1, f) == 1 && P >= 0;
  std::vector<Data> data(ok ? (size_t)P : 0);
  for (Data& d : data) {
    int32_t unused_status; double unused[15];
    ok = ok && std::fread(&d.n, 4, 1, f) == 1 && d.n >= 0 && std::fread(&unused_status, 4, 1, f) == 1 && std::fread(d.cam_a, 8, 9, f) == 9 && std::fread(d.cam_b, 8, 9, f) == 9 &&
         std::fread(unused, 8, 15, f) == 15;
    if (!ok) break;
    d.xa.resize((size_t)d.n * 2); d.xb.resize((size_t)d.n * 2);
    ok = std::fread(d.xa.data(), 4, d.xa.size(), f) == d.xa.size() && std::fread(d.xb.data(), 4, d.xb.size(), f) == d.xb.size();
  }
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "bad pairs file\n"); return 2; }
  const std::string mode = argv[3];
  if (mode != "batched" && mode != "sequential") { std::fprintf(stderr, "mode is batched or sequential\n"); return 2; }
  TwoViewOptions tv;
  tv.iterations = std::atoi(argv[4]); tv.threshold_px = std::atof(argv[5]); tv.refits = std::atoi(argv[6]); tv.min_inliers = std::atoi(argv[7]);
  tv.rng_state = std::strtoull(argv[8], nullptr, 0); tv.hypotheses_on_device = std::atoi(argv[9]) == 0;
  if (!parse_solver(argv[10], tv)) return 2;
  ClassifyOptions co;
  co.min_parallax_deg = std::atof(argv[11]);
  co.max_tasks_per_launch = argc > 12 ? std::atoi(argv[12]) : 0;
  try {
    if (mode == "batched") {
      std::vector<EssentialPair> pairs(data.size());
      for (size_t p = 0; p < data.size(); ++p) pairs[p] = EssentialPair{data[p].xa.data(), data[p].xb.data(), data[p].n, data[p].cam_a, data[p].cam_b};
      const std::vector<TwoViewResult> results = findEssentialRansacPairs(pairs, tv, 0, co.max_tasks_per_launch);
      const std::vector<PairGeometry> geo = classifyPairs(pairs, results, tv, co, 0);
      for (size_t p = 0; p < data.size(); ++p) print_geometry(results[p].ok, geo[p]);
    } else {
      const double cos_min = homo_detail::cos_of_degrees(co.min_parallax_deg);
      for (const Data& d : data) {
        const TwoViewResult e = findEssentialRansac(d.xa.data(), d.xb.data(), d.n, d.cam_a, d.cam_b, tv, 0);
        const HomographyResult h = findHomographyRansac(d.xa.data(), d.xb.data(), d.n, d.cam_a, d.cam_b, tv, 0);
        PairGeometry g;
        g.h_ok = h.ok; g.num_h_inliers = h.num_inliers; g.h_winner_task = h.winner_task; g.h_refits_adopted = h.refits_adopted; g.h_inliers = h.inliers;
        for (int k = 0; k < 9; ++k) g.H[k] = h.H[k];
        if (e.ok) {
          const std::vector<double> na = hyp_detail::normalised_points(d.cam_a, d.xa.data(), d.n), nb = hyp_detail::normalised_points(d.cam_b, d.xb.data(), d.n);
          int32_t front = 0, par = 0;
          homo_detail::parallax_counts(na.data(), nb.data(), d.n, e.E, e.pose_b, epi_detail::mean_focal2(d.cam_a, d.cam_b), tv.threshold_px * tv.threshold_px, cos_min, &front, &par);
          g.num_front = front; g.num_parallax = par;
        }
        g.kind = homo_detail::kind_of(e.ok, e.num_inliers, g, co);
        print_geometry(e.ok, g);
      }
    }
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 3; }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "pairs") return pairs_only(argc, argv);
  if (argc < 2) { std::fprintf(stderr, "usage: %s <session.cache> [key=value ...]\n", argv[0]); return 2; }
  std::map<std::string, std::string> kv;
  for (int i = 2; i < argc; ++i) {
    const char* eq = std::strchr(argv[i], '=');
    if (!eq) { std::fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    kv[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
  }
  auto num = [&](const char* k, double d) { auto it = kv.find(k); return it == kv.end() ? d : std::atof(it->second.c_str()); };
  Session sess;
  try { loadCache(argv[1], sess); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
  TwoViewOptions tv;
  tv.iterations = (int)num("iterations", 1000);
  tv.threshold_px = num("threshold", 4.0);
  tv.refits = (int)num("refits", 3);
  tv.min_inliers = (int)num("minInliers", 16);
  if (kv.count("seed")) tv.rng_state = std::strtoull(kv["seed"].c_str(), nullptr, 0);
  tv.hypotheses_on_device = num("hostHypotheses", 0) == 0;
  if (kv.count("solver") && !parse_solver(kv["solver"], tv)) return 2;
  VerifyOptions vo;
  vo.max_tasks_per_launch = (int)num("maxTasks", 0);
  ClassifyOptions co;
  co.min_parallax_deg = num("minParallaxDeg", co.min_parallax_deg);
  co.min_parallax_share = num("minParallaxShare", co.min_parallax_share);
  co.max_h_ratio = num("maxHRatio", co.max_h_ratio);
  co.max_tasks_per_launch = vo.max_tasks_per_launch;
  PickOptions po;
  po.allow_planar = num("allowPlanar", 0) != 0;
  try {
    const std::vector<PairReport> reports = verifyMatches(sess, tv, 0, vo);
    std::vector<std::vector<std::vector<std::pair<int32_t, int32_t>>>> before(sess.frames.size());
    auto refs_of = [&](std::vector<std::vector<std::vector<std::pair<int32_t, int32_t>>>>& out) {
      out.assign(sess.frames.size(), {});
      for (size_t f = 0; f < sess.frames.size(); ++f) {
        out[f].resize(sess.frames[f].obs.size());
        for (size_t o = 0; o < sess.frames[f].obs.size(); ++o)
          for (const ObservationRef& ref : sess.frames[f].obs[o].matches) out[f][o].push_back(std::make_pair(ref.frame, ref.obs));
      }
    };
    refs_of(before);
    const std::vector<PairGeometry> geo = classifyMatches(sess, reports, tv, 0, co);
    std::vector<std::vector<std::vector<std::pair<int32_t, int32_t>>>> after;
    refs_of(after);
    std::printf("pairs %zu\n", reports.size());
    for (size_t p = 0; p < reports.size(); ++p) {
      const PairReport& r = reports[p];
      std::printf("%d %d %d %d %d %d %s %d %d %d %d\n", r.frameA, r.frameB, r.correspondences, r.ok ? 1 : 0, r.num_inliers, r.num_front, pairKindName(geo[p].kind),
                  geo[p].h_ok ? 1 : 0, geo[p].num_h_inliers, geo[p].num_front, geo[p].num_parallax);
    }
    std::printf("bootstrap %d %d\n", pickBootstrapPair(reports), pickBootstrapPair(reports, geo, po));
    std::printf("untouched %d\n", before == after ? 1 : 0);
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 3; }
  return 0;
}
