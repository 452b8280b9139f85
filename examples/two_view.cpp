// The two-view bootstrap over a Session cache (include/rsba/two_view.hpp): loads a cache (VideoSfMCache, Thrift binary;
// include/rsba/session_cache.hpp), drops ALL tracks and ALL poses — frame a's are kept with keepPoseA=1 — and gives frames a and b their
// poses from the matches between them alone (initializeTwoView: essential-matrix RANSAC on the device, createTracks, and for neighbouring
// frames a bundle adjustment of the pair).
//
//   two_view <session.cache> <out.bin> [key=value ...]
//     keys: a (0), b (1), iterations (1000), threshold (4), refits (3), minInliers (16), seed (0x9e3779b97f4a7c15), ba (20; BA iterations, run
//           when b == a + 1), hostHypotheses (0; 1: the RANSAC from the host definitions, for comparison), keepPoseA (0), sqrdThreshold (16),
//           minReprojections (3), maxReprojections (10), fixFirstN (0), rolling (default: the first frame of the cache has two poses),
//           keepPoses (0; 1: frames a and b both keep the poses of the cache and no RANSAC runs — createTracks and the bundle adjustment from
//           a known relative geometry, what the result is compared with), solver (eight_point; five_point: TwoViewOptions::solver — the RANSAC
//           draws five-point subsets and takes the best solution of each)
//   out.bin (little endian): int64 ok, int64 correspondences, int64 inliers, int64 inliers in front, int64 tracks created; then the
//     session's state in the layout of examples/new_frame.cpp: int64 F; per frame: int64 np, double poses[np][6], int64 nobs, per
//     observation: int64 track, int64 isset_track, int64 nmatches, int64 ref_valid[nmatches]; then int64 T; per track: double pt[3] (zeros
//     without a point), int64 valid, int64 n, n x {int64 frame, int64 obs, int64 valid}
//   two_view ransac <scene.bin> <iterations> <threshold> <refits> <minInliers> <seed> <hostHypotheses> [solver]
//     findEssentialRansac alone, on plain arrays; solver eight_point (default) or five_point.  scene.bin: int32 n, double cam_a[9], cam_b[9], float xy_a[n][2], xy_b[n][2]; stdout:
//     "<ok> <winner task> <inliers> <in front> <refits adopted>", E, the pose of camera B, the inlier flags — one line each
//   exit status: 0 done, 2 bad input, 3 something threw (message on stderr)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "rsba/session_cache.hpp"
#include "rsba/two_view.hpp"

using namespace rsba_amd;

static void w64(FILE* g, int64_t v) { std::fwrite(&v, sizeof v, 1, g); }
static void wd(FILE* g, const double* v, size_t n) { std::fwrite(v, sizeof(double), n, g); }

static void write_state(FILE* g, const Session& sess) {
  w64(g, (int64_t)sess.frames.size());
  for (const Frame& f : sess.frames) {
    w64(g, f.__isset.poses ? (int64_t)f.poses.size() : 0);
    if (f.__isset.poses) for (const auto& p : f.poses) wd(g, p.data(), NUM_POSE_PARAMS);
    w64(g, (int64_t)f.obs.size());
    for (const Observation& o : f.obs) {
      w64(g, o.track); w64(g, o.__isset.track ? 1 : 0);
      w64(g, (int64_t)o.matches.size());
      for (const ObservationRef& r : o.matches) w64(g, r.valid ? 1 : 0);
    }
  }
  w64(g, (int64_t)sess.tracks.size());
  for (const Track& t : sess.tracks) {
    const double zero[3] = {0, 0, 0};
    wd(g, t.pt.size() == 3 ? t.pt.data() : zero, 3);
    w64(g, t.valid ? 1 : 0);
    w64(g, (int64_t)t.obs.size());
    for (const ObservationRef& r : t.obs) { w64(g, r.frame); w64(g, r.obs); w64(g, r.valid ? 1 : 0); }
  }
}

static bool parse_solver(const std::string& name, TwoViewOptions& tv) {
  if (name == "five_point") tv.solver = TwoViewOptions::EssentialSolver::FivePoint;
  else if (name == "eight_point") tv.solver = TwoViewOptions::EssentialSolver::EightPoint;
  else { std::fprintf(stderr, "solver is eight_point or five_point\n"); return false; }
  return true;
}

static int ransac_only(int argc, char** argv) {
  if (argc < 9) { std::fprintf(stderr, "usage: %s ransac <scene.bin> <iterations> <threshold> <refits> <minInliers> <seed> <hostHypotheses>\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::perror("scene"); return 2; }
  int32_t n = 0; double cam_a[9], cam_b[9];
  std::vector<float> xa, xb;
  bool ok = std::fread(&n, 4, 1, f) == 1 && n >= 0 && std::fread(cam_a, 8, 9, f) == 9 && std::fread(cam_b, 8, 9, f) == 9;
  if (ok) { xa.resize((size_t)n * 2); xb.resize((size_t)n * 2); ok = std::fread(xa.data(), 4, xa.size(), f) == xa.size() && std::fread(xb.data(), 4, xb.size(), f) == xb.size(); }
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "bad scene file\n"); return 2; }
  TwoViewOptions tv;
  tv.iterations = std::atoi(argv[3]); tv.threshold_px = std::atof(argv[4]); tv.refits = std::atoi(argv[5]); tv.min_inliers = std::atoi(argv[6]);
  tv.rng_state = std::strtoull(argv[7], nullptr, 0); tv.hypotheses_on_device = std::atoi(argv[8]) == 0;
  if (argc > 9 && !parse_solver(argv[9], tv)) return 2;
  try {
    const TwoViewResult r = findEssentialRansac(xa.data(), xb.data(), n, cam_a, cam_b, tv, 0);
    std::printf("%d %d %d %d %d\n", r.ok ? 1 : 0, r.winner_task, r.num_inliers, r.num_front, r.refits_adopted);
    for (double x : r.E) std::printf("%.17g ", x);
    std::printf("\n");
    for (double x : r.pose_b) std::printf("%.17g ", x);
    std::printf("\n");
    for (uint8_t b : r.inliers) std::printf("%d ", (int)b);
    std::printf("\n");
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 3; }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "ransac") return ransac_only(argc, argv);
  if (argc < 3) { std::fprintf(stderr, "usage: %s <session.cache> <out.bin> [key=value ...]\n", argv[0]); return 2; }
  std::map<std::string, std::string> kv;
  for (int i = 3; i < argc; ++i) {
    const char* eq = std::strchr(argv[i], '=');
    if (!eq) { std::fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    kv[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
  }
  auto num = [&](const char* k, double d) { auto it = kv.find(k); return it == kv.end() ? d : std::atof(it->second.c_str()); };
  Session sess;
  try { loadCache(argv[1], sess); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
  const int32_t a = (int32_t)num("a", 0), b = (int32_t)num("b", 1);
  if (a < 0 || a >= b || (size_t)b >= sess.frames.size()) { std::fprintf(stderr, "need 0 <= a < b < number of frames\n"); return 2; }
  SfmOptions opt;
  opt.model.rolling_shutter = num("rolling", sess.frames[0].poses.size() != 1) != 0;
  opt.ceres.fixFirstNCameras = (unsigned)num("fixFirstN", 0);
  opt.tracks.sqrdThreshold = num("sqrdThreshold", 16.0);
  opt.tracks.minReprojections = (unsigned)num("minReprojections", 3);
  opt.tracks.maxReprojections = (unsigned)num("maxReprojections", 10);
  TwoViewOptions tv;
  tv.iterations = (int)num("iterations", 1000);
  tv.threshold_px = num("threshold", 4.0);
  tv.refits = (int)num("refits", 3);
  tv.min_inliers = (int)num("minInliers", 16);
  if (kv.count("seed")) tv.rng_state = std::strtoull(kv["seed"].c_str(), nullptr, 0);
  tv.hypotheses_on_device = num("hostHypotheses", 0) == 0;
  if (kv.count("solver") && !parse_solver(kv["solver"], tv)) return 2;
  const bool keepPoseA = num("keepPoseA", 0) != 0, keepPoses = num("keepPoses", 0) != 0;

  // nothing is known but the observations and their matches
  sess.tracks.clear();
  for (size_t f = 0; f < sess.frames.size(); ++f) {
    Frame& fr = sess.frames[f];
    for (Observation& o : fr.obs) { o.track = 0; o.__isset.track = false; }
    if (!((keepPoseA || keepPoses) && (int32_t)f == a) && !(keepPoses && (int32_t)f == b)) { fr.poses.clear(); fr.__isset.poses = false; }
  }

  FILE* g = std::fopen(argv[2], "wb");
  if (!g) { std::perror("out"); return 2; }
  try {
    TwoViewReport rep;
    bool ok = true;
    if (keepPoses) {   // what initializeTwoView does once frame b has its pose
      createTracks(sess, (size_t)b, opt, 0);
      if (num("ba", 20) > 0 && b == a + 1) ok = BA(sess, a, b, opt, (int32_t)num("ba", 20), nullptr, false, nullptr, true);
    } else {
      ok = initializeTwoView(sess, a, b, opt, tv, 0, false, (int32_t)num("ba", 20), &rep);
    }
    w64(g, ok ? 1 : 0); w64(g, rep.correspondences); w64(g, rep.num_inliers); w64(g, rep.num_front); w64(g, (int64_t)sess.tracks.size());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    std::fclose(g);
    return 3;
  }
  write_state(g, sess);
  std::fclose(g);
  return 0;
}
