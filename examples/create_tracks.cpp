// Track creation on a Session cache (include/rsba/create_tracks.hpp): loads a cache written by the reference (VideoSfMCache,
// Thrift binary; include/rsba/session_cache.hpp), runs one of
//   frame   createTracks(sess, fi, opt) for fi = first..last in order          (VideoSfMHandler.cc:283-372)
//   batch   createTracks(sess, first, last, opt): one triangulation call for the range
//   full    fullBA(sess, opt, maxIter, ..., reproject = true)                  (VideoSfMHandler.cc:153-180, :600)
//   window  windowedBA(sess, opt, first, last, maxIter, ..., reproject = true) (VideoSfMHandler.cc:185-214, :600)
//   replay  replayCreateTracks(sess, fi, opt, flags) for fi = first..last, the flags read from a file (no device)
// and writes the resulting state as a flat binary file.
//
//   create_tracks <mode> <session.cache> <out.bin> [key=value ...]
//     keys: first, last (default 0 and the last frame), maxIter (20), fixFirstN (1), sqrdThreshold (16), minReprojections (3),
//           maxReprojections (10), minDistanceToCamera (0), const3d (0), synthetic (0), interpolateRotation (1),
//           useOnlyValidMatches (1), flags (replay: the flag file)
//   flag file (little endian), per frame first..last: int64 n, then n entries {int64 tri, int64 reproj, double pt[3]} in the
//     order of TrackFlags (observation, then match); 0 / 1, or 2 = not computed
//   out.bin (little endian): int64 F; per frame: int64 np, double poses[np][6], int64 nobs, per observation: int64 track,
//     int64 isset_track, int64 nmatches, int64 ref_valid[nmatches]; then int64 T; per track: double pt[3] (zeros without a
//     point), int64 valid, int64 n, n x {int64 frame, int64 obs, int64 valid}
//   exit status: 0 done, 1 the solve's result was not usable, 2 bad input, 3 createTracks threw (message on stderr)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "rsba/ceres_handler.hpp"
#include "rsba/create_tracks.hpp"
#include "rsba/session_cache.hpp"

using namespace rsba_amd;

static void w64(FILE* g, int64_t v) { std::fwrite(&v, sizeof v, 1, g); }
static void wd(FILE* g, const double* v, size_t n) { std::fwrite(v, sizeof(double), n, g); }

static int write_state(const char* path, const Session& sess) {
  FILE* g = std::fopen(path, "wb");
  if (!g) { std::perror("out"); return 2; }
  w64(g, (int64_t)sess.frames.size());
  for (const Frame& f : sess.frames) {
    w64(g, (int64_t)f.poses.size());
    for (const auto& p : f.poses) wd(g, p.data(), NUM_POSE_PARAMS);
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
  std::fclose(g);
  return 0;
}

static bool read_flags(const char* path, const Session& sess, size_t first, size_t last, std::vector<TrackFlags>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  for (size_t fi = first; fi <= last; ++fi) {
    TrackFlags g(sess.frames[fi]);
    int64_t n = 0;
    if (std::fread(&n, sizeof n, 1, f) != 1 || (size_t)n != g.tri.size()) { std::fclose(f); return false; }
    for (int64_t e = 0; e < n; ++e) {
      int64_t tri, rep; double pt[3];
      if (std::fread(&tri, sizeof tri, 1, f) != 1 || std::fread(&rep, sizeof rep, 1, f) != 1 || std::fread(pt, sizeof(double), 3, f) != 3) { std::fclose(f); return false; }
      g.tri[(size_t)e] = (uint8_t)tri; g.reproj[(size_t)e] = (uint8_t)rep;
      for (int q = 0; q < 3; ++q) g.pt[3 * (size_t)e + q] = pt[q];
    }
    out.push_back(g);
  }
  std::fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s frame|batch|full|window|replay <session.cache> <out.bin> [key=value ...]\n", argv[0]); return 2; }
  const std::string mode = argv[1];
  std::map<std::string, std::string> kv;
  for (int i = 4; i < argc; ++i) {
    const char* eq = std::strchr(argv[i], '=');
    if (!eq) { std::fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    kv[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
  }
  auto num = [&](const char* k, double d) { auto it = kv.find(k); return it == kv.end() ? d : std::atof(it->second.c_str()); };
  Session sess;
  try { loadCache(argv[2], sess); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
  if (sess.frames.empty()) { std::fprintf(stderr, "empty session\n"); return 2; }
  SfmOptions opt;
  opt.model.rolling_shutter = sess.frames[0].poses.size() != 1;
  opt.model.interpolateRotation = num("interpolateRotation", 1) != 0;
  opt.tracks.sqrdThreshold = num("sqrdThreshold", 16.0);
  opt.tracks.minReprojections = (unsigned)num("minReprojections", 3);
  opt.tracks.maxReprojections = (unsigned)num("maxReprojections", 10);
  opt.tracks.minDistanceToCamera = (unsigned)num("minDistanceToCamera", 0);
  opt.tracks.synthetic = num("synthetic", 0) != 0;
  opt.ceres.const3d = num("const3d", 0) != 0;
  opt.ceres.fixFirstNCameras = (unsigned)num("fixFirstN", 1);
  opt.ceres.useOnlyValidMatches = num("useOnlyValidMatches", 1) != 0;
  const int maxIter = (int)num("maxIter", 20);
  const size_t first = (size_t)num("first", 0), last = (size_t)num("last", (double)(sess.frames.size() - 1));
  if (first > last || last >= sess.frames.size()) { std::fprintf(stderr, "bad frame range\n"); return 2; }
  bool usable = true;
  try {
    if (mode == "frame") {
      for (size_t fi = first; fi <= last; ++fi) createTracks(sess, fi, opt);
    } else if (mode == "batch") {
      createTracks(sess, first, last, opt);
    } else if (mode == "full") {
      usable = fullBA(sess, opt, maxIter, nullptr, false, nullptr, true);
    } else if (mode == "window") {
      usable = windowedBA(sess, opt, (int32_t)first, (int32_t)last, maxIter, nullptr, false, nullptr, true);
    } else if (mode == "replay") {
      std::vector<TrackFlags> flags;
      if (!kv.count("flags") || !read_flags(kv["flags"].c_str(), sess, first, last, flags)) { std::fprintf(stderr, "cannot read the flag file\n"); return 2; }
      for (size_t fi = first; fi <= last; ++fi) replayCreateTracks(sess, fi, opt, flags[fi - first]);
    } else {
      std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
      return 2;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  const int rc = write_state(argv[3], sess);
  return rc ? rc : (usable ? 0 : 1);
}
