// End-to-end wall time of the batched createTracks (include/rsba/create_tracks.hpp) on a scene written by tools/tracks_time.py:
// every observation matched to its point's two previous observations (frame order), the tracks of the even points kept (their
// observations listed, their points set, valid), the odd points untracked — so the call triangulates new tracks and checks
// the later observations of a point against the tracks it created.  Runs createTracks(sess, 0, F - 1, opt) twice on copies of the session (the first
// also grows the device arena and the pinned staging buffers) and prints the CreateTracksTimes of both.
//   usage: tracks_e2e <dir>   (dir/header.bin int64 F,P,M,N,rs,scan0,scan1; cam.bin double[9]; poses.bin double[F][P][6];
//                              points.bin double[M][3]; xy.bin double[N][2]; frame.bin int32[N]; point.bin int32[N])
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "rsba/create_tracks.hpp"

using namespace rsba_amd;

template <class T>
static std::vector<T> load(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f || std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); std::exit(2); }
  std::fclose(f);
  return v;
}

static void report(const char* what, const CreateTracksTimes& t, const Session& before, const Session& after) {
  size_t joined = 0, joined_new = 0;   // observations that joined by reprojection: existing tracks / tracks of this call (beyond its first two)
  for (size_t i = 0; i < before.tracks.size(); ++i) joined += after.tracks[i].obs.size() - before.tracks[i].obs.size();
  for (size_t i = before.tracks.size(); i < after.tracks.size(); ++i) joined_new += after.tracks[i].obs.size() - 2;
  std::printf("%s: total %.1f ms = gather %.1f + triangulation call %.1f + reprojection checks %.1f (%lld calls) + replay %.1f;"
              " %lld triangulations, %lld checks; %zu new tracks, %zu observations joined existing tracks, %zu joined new ones\n",
              what, 1e3 * t.total_s, 1e3 * t.gather_s, 1e3 * t.triangulate_s, 1e3 * t.reproject_s, (long long)t.check_calls, 1e3 * t.replay_s,
              (long long)t.triangulations, (long long)t.checks, after.tracks.size() - before.tracks.size(), joined, joined_new);
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
  const std::string d = argv[1];
  const std::vector<int64_t> h = load<int64_t>(d + "/header.bin", 7);
  const size_t F = (size_t)h[0], P = (size_t)h[1], M = (size_t)h[2], N = (size_t)h[3];
  const std::vector<double> cam = load<double>(d + "/cam.bin", 9), poses = load<double>(d + "/poses.bin", F * P * 6),
                            points = load<double>(d + "/points.bin", M * 3), xy = load<double>(d + "/xy.bin", N * 2);
  const std::vector<int32_t> frame = load<int32_t>(d + "/frame.bin", N), point = load<int32_t>(d + "/point.bin", N);
  Session sess;
  sess.cam = cam;
  sess.rs = (int32_t)h[4];
  sess.scanlines = {(int32_t)h[5], (int32_t)h[6]};
  sess.frames.resize(F);
  for (size_t f = 0; f < F; ++f) {
    for (size_t q = 0; q < P; ++q) sess.frames[f].poses.emplace_back(poses.begin() + (f * P + q) * 6, poses.begin() + (f * P + q + 1) * 6);
    sess.frames[f].__isset.poses = true;
  }
  std::vector<size_t> order(N);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return frame[a] < frame[b]; });
  std::vector<std::vector<ObservationRef>> seen(M);
  for (size_t i : order) {
    Frame& fr = sess.frames[(size_t)frame[i]];
    Observation o;
    o.x = xy[2 * i]; o.y = xy[2 * i + 1];
    const std::vector<ObservationRef>& prev = seen[(size_t)point[i]];
    for (size_t back = 1; back <= 2 && back <= prev.size(); ++back) o.matches.push_back(ObservationRef{prev[prev.size() - back].frame, prev[prev.size() - back].obs, false});
    o.__isset.matches = !o.matches.empty();
    seen[(size_t)point[i]].push_back(ObservationRef{frame[i], (int32_t)fr.obs.size(), true});
    fr.obs.push_back(o);
  }
  for (size_t j = 0; j < M; j += 2) {
    if (seen[j].empty()) continue;
    Track t;
    t.obs = seen[j];
    t.pt.assign(points.begin() + 3 * j, points.begin() + 3 * j + 3);
    t.__isset.pt = true;
    t.valid = true;
    for (const ObservationRef& r : t.obs) { Observation& o = sess.frames[(size_t)r.frame].obs[(size_t)r.obs]; o.track = (int32_t)sess.tracks.size(); o.__isset.track = true; }
    sess.tracks.push_back(t);
  }
  SfmOptions opt;
  std::printf("%zu frames, %zu observations, %zu tracks kept of %zu points\n", F, N, sess.tracks.size(), M);
  try {
    for (int run = 0; run < 2; ++run) {
      Session s = sess;
      CreateTracksTimes t;
      createTracks(s, 0, F - 1, opt, 0, &t);
      report(run == 0 ? "first call (grows the device arena)" : "second call", t, sess, s);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  return 0;
}
