// Geometric verification of a Session cache's matches (include/rsba/two_view.hpp: verifyMatches): loads a cache (VideoSfMCache, Thrift
// binary; include/rsba/session_cache.hpp), runs the essential-matrix RANSAC of every matched frame pair in one batched device call, erases
// the refs it flags from Observation::matches, prints the reports and writes the session back — the step between matchSession and
// createTracks / initializeTwoView.
//
//   verify_matches <session.cache> <out.cache> [key=value ...]
//     keys: iterations (1000), threshold (4), refits (3), minInliers (16), seed (0x9e3779b97f4a7c15), solver (eight_point; five_point),
//           hostHypotheses (0; 1: the RANSAC from the host definitions, no device), dropUnverified (0), maxTasks (0: the library's default
//           of tasks per launch), dump (0; 1: also print every observation's remaining refs)
//     stdout: "pairs <P>"; per pair "<frameA> <frameB> <correspondences> <ok> <inliers> <in front> <removed>" then E and the pose of camera B
//     on the same line; "bootstrap <index of pickBootstrapPair, or -1>"; with dump=1 per observation that has refs
//     "refs <frame> <obs>" followed by its refs as "<frame> <obs>" pairs
//   verify_matches pairs <pairs.bin> <batched|sequential> <iterations> <threshold> <refits> <minInliers> <seed> <hostHypotheses> <solver> [maxTasks]
//     findEssentialRansacPairs (batched) or findEssentialRansac pair by pair (sequential) on plain arrays.  pairs.bin: int32 P; per pair
//     int32 n, double cam_a[9], cam_b[9], float xy_a[n][2], xy_b[n][2].  stdout per pair: "<ok> <winner task> <inliers> <in front> <refits
//     adopted>", E, the pose of camera B, the inlier flags — one line each
//   exit status: 0 done, 2 bad input, 3 something threw (message on stderr)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "rsba/session_cache.hpp"
#include "rsba/two_view.hpp"

using namespace rsba_amd;

static bool parse_solver(const std::string& name, TwoViewOptions& tv) {
  if (name == "five_point") tv.solver = TwoViewOptions::EssentialSolver::FivePoint;
  else if (name == "eight_point") tv.solver = TwoViewOptions::EssentialSolver::EightPoint;
  else { std::fprintf(stderr, "solver is eight_point or five_point\n"); return false; }
  return true;
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

static int pairs_only(int argc, char** argv) {
  if (argc < 11) { std::fprintf(stderr, "usage: %s pairs <pairs.bin> <batched|sequential> <iterations> <threshold> <refits> <minInliers> <seed> <hostHypotheses> <solver> [maxTasks]\n", argv[0]); return 2; }
  struct Data { int32_t n = 0; double cam_a[9], cam_b[9]; std::vector<float> xa, xb; };
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::perror("pairs"); return 2; }
  int32_t P = 0;
  bool ok = std::fread(&P, 4, 1, f) == 1 && P >= 0;
  std::vector<Data> data(ok ? (size_t)P : 0);
  for (Data& d : data) {
    ok = ok && std::fread(&d.n, 4, 1, f) == 1 && d.n >= 0 && std::fread(d.cam_a, 8, 9, f) == 9 && std::fread(d.cam_b, 8, 9, f) == 9;
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
  const int max_tasks = argc > 11 ? std::atoi(argv[11]) : 0;
  try {
    if (mode == "batched") {
      std::vector<EssentialPair> pairs(data.size());
      for (size_t p = 0; p < data.size(); ++p) pairs[p] = EssentialPair{data[p].xa.data(), data[p].xb.data(), data[p].n, data[p].cam_a, data[p].cam_b};
      for (const TwoViewResult& r : findEssentialRansacPairs(pairs, tv, 0, max_tasks)) print_result(r);
    } else {
      for (const Data& d : data) print_result(findEssentialRansac(d.xa.data(), d.xb.data(), d.n, d.cam_a, d.cam_b, tv, 0));
    }
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 3; }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "pairs") return pairs_only(argc, argv);
  if (argc < 3) { std::fprintf(stderr, "usage: %s <session.cache> <out.cache> [key=value ...]\n", argv[0]); return 2; }
  std::map<std::string, std::string> kv;
  for (int i = 3; i < argc; ++i) {
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
  vo.drop_unverified = num("dropUnverified", 0) != 0;
  vo.max_tasks_per_launch = (int)num("maxTasks", 0);
  try {
    const std::vector<PairReport> reports = verifyMatches(sess, tv, 0, vo);
    std::printf("pairs %zu\n", reports.size());
    for (const PairReport& r : reports) {
      std::printf("%d %d %d %d %d %d %d", r.frameA, r.frameB, r.correspondences, r.ok ? 1 : 0, r.num_inliers, r.num_front, r.removed);
      for (double x : r.E) std::printf(" %.17g", x);
      for (double x : r.pose_b) std::printf(" %.17g", x);
      std::printf("\n");
    }
    std::printf("bootstrap %d\n", pickBootstrapPair(reports));
    if (num("dump", 0) != 0)
      for (size_t f = 0; f < sess.frames.size(); ++f)
        for (size_t o = 0; o < sess.frames[f].obs.size(); ++o) {
          const std::vector<ObservationRef>& list = sess.frames[f].obs[o].matches;
          if (list.empty()) continue;
          std::printf("refs %zu %zu", f, o);
          for (const ObservationRef& ref : list) std::printf(" %d %d", ref.frame, ref.obs);
          std::printf("\n");
        }
    saveCache(argv[2], sess);
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 3; }
  return 0;
}
