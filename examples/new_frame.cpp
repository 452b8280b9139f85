// The incremental step over a Session cache (include/rsba/new_frame.hpp): loads a cache written by the reference (VideoSfMCache,
// Thrift binary; include/rsba/session_cache.hpp), takes the last k frames out of the session — their poses removed (unless keepPoses=1),
// their observations no longer in any track — and re-adds them one by one through processFrame (VideoSfMClient.cc:231-251: newFrame,
// solve, solveRsPnP, createTracks, the windowed BA).
//
//   new_frame <session.cache> <out.bin> [key=value ...]
//     keys: k (1), keepPoses (0; 1: the frames keep the poses of the cache, so that only pnpNewFrame moves them), keepPriors (1; 0: priorPoses dropped),
//           reuseLastPose (1), solveGsPnP (0), solveRsPnP (1), minPnPfeatures (6), refinePnP (0), pnpNewFrame (0), baIterationsOnNewFrame (0),
//           baWindowOnNewFrame (0), sqrdThreshold (16), minReprojections (3), maxReprojections (10), fixFirstN (0), useOnlyValidMatches (1),
//           rolling (default: the first frame has two poses)
//   out.bin (little endian): int64 k; per re-added frame: int64 key, int64 processFrame's return value, int64 localised (the frame has
//     poses), int64 tracks before, int64 tracks after; then the session's state in the layout of examples/create_tracks.cpp: int64 F; per
//     frame: int64 np, double poses[np][6], int64 nobs, per observation: int64 track, int64 isset_track, int64 nmatches, int64
//     ref_valid[nmatches]; then int64 T; per track: double pt[3] (zeros without a point), int64 valid, int64 n, n x {int64 frame, int64 obs,
//     int64 valid}
//   exit status: 0 done, 2 bad input, 3 something threw (message on stderr)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "rsba/new_frame.hpp"
#include "rsba/session_cache.hpp"

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

int main(int argc, char** argv) {
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
  const size_t k = (size_t)num("k", 1);
  if (k == 0 || sess.frames.size() <= k) { std::fprintf(stderr, "k must be positive and smaller than the number of frames\n"); return 2; }
  SfmOptions opt;
  opt.model.rolling_shutter = num("rolling", sess.frames[0].poses.size() != 1) != 0;
  opt.mod_init.reuseLastPose = num("reuseLastPose", 1) != 0;
  opt.mod_init.solveGsPnP = num("solveGsPnP", 0) != 0;
  opt.mod_init.solveRsPnP = num("solveRsPnP", 1) != 0;
  opt.mod_init.minPnPfeatures = (unsigned)num("minPnPfeatures", 6);
  opt.mod_init.refinePnP = num("refinePnP", 0) != 0;
  opt.ceres.pnpNewFrame = num("pnpNewFrame", 0) != 0;
  opt.ceres.baIterationsOnNewFrame = (unsigned)num("baIterationsOnNewFrame", 0);
  opt.ceres.baWindowOnNewFrame = (unsigned)num("baWindowOnNewFrame", 0);
  opt.ceres.fixFirstNCameras = (unsigned)num("fixFirstN", 0);
  opt.ceres.useOnlyValidMatches = num("useOnlyValidMatches", 1) != 0;
  opt.tracks.sqrdThreshold = num("sqrdThreshold", 16.0);
  opt.tracks.minReprojections = (unsigned)num("minReprojections", 3);
  opt.tracks.maxReprojections = (unsigned)num("maxReprojections", 10);
  const bool keepPoses = num("keepPoses", 0) != 0, keepPriors = num("keepPriors", 1) != 0;

  // take the last k frames out: no track refers to them any more, their observations belong to no track
  const size_t first = sess.frames.size() - k;
  std::vector<Frame> later(sess.frames.begin() + (std::ptrdiff_t)first, sess.frames.end());
  sess.frames.resize(first);
  for (Track& t : sess.tracks) {
    std::vector<ObservationRef> kept;
    for (const ObservationRef& r : t.obs) if ((size_t)r.frame < first) kept.push_back(r);
    t.obs.swap(kept);
  }
  for (Frame& f : later) {
    for (Observation& o : f.obs) { o.track = 0; o.__isset.track = false; }
    if (!keepPoses) { f.poses.clear(); f.__isset.poses = false; }
    if (!keepPriors) { f.priorPoses.clear(); f.__isset.priorPoses = false; }
  }

  FILE* g = std::fopen(argv[2], "wb");
  if (!g) { std::perror("out"); return 2; }
  w64(g, (int64_t)k);
  try {
    for (const Frame& f : later) {
      const int64_t before = (int64_t)sess.tracks.size();
      int32_t key = -1;
      const bool ok = processFrame(sess, f, opt, &key, 0, false);
      w64(g, key); w64(g, ok ? 1 : 0); w64(g, sess.frames[(size_t)key].__isset.poses ? 1 : 0); w64(g, before); w64(g, (int64_t)sess.tracks.size());
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    std::fclose(g);
    return 3;
  }
  write_state(g, sess);
  std::fclose(g);
  return 0;
}
