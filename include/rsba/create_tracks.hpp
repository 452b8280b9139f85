// Host-side mirror of track creation, with its geometry on the device:
//   VideoSfMHandler::reprojectMatches   rsba/src/rsba/VideoSfMHandler.cc:231-280
//   VideoSfMHandler::createTracks       rsba/src/rsba/VideoSfMHandler.cc:283-372
//   VideoSfMHandler::evalTracks         rsba/src/rsba/VideoSfMHandler.cc:377-410
//   inTrack                             rsba/src/rsba/struct/VideoSfM.h:155-160
// Same names, argument meaning and order of decisions.  Two deviations:
//   * reprojectMatches reads the camera centre for its minDistanceToCamera gate before getPose has filled the pose in
//     (:253-256, then :260) — a read of an uninitialised value.  Here the gate uses getPose(o), which every later pass of the
//     same loop uses anyway; the geometric part of the decision is then vision::sfm::validate(sess, f, opt, t.pt, obs).
//   * triangulate aborts the reference when det(A) < eps (mat/cam.h:204-207); here that candidate just fails.
// Reproduced as written: evalTracks drops the observations that validate ACCEPTS (:389); the loop over a match list does not
// stop after it creates a track (a later match can create another one, and o.track then names the newest); the second
// reprojectMatches can move o to an older track; reprojectMatches also runs for an observation that already has a track.
// A match inside frameKey throws std::runtime_error in the creation branch (the reference's CHECK, :308) and is taken by the
// reprojection branch; a match into a frame without poses throws there too (CHECK(f2.__isset.poses), :310); getPose on a frame
// without poses throws "empty frame" (struct/VideoSfM.cc:105) when the replay reaches the predicate that needs it, as in the
// reference.
//
// Why one device pass plus a host replay gives exactly the reference's result.  Within one createTracks(frameKey) call:
//   1. poses and the points of existing tracks never change;
//   2. a triangulation depends only on poses and observations;
//   3. an observation of another frame changes track only from "untracked" to a track created in the call;
//   4. every track created in the call, and every track an observation of frameKey joins, then contains an observation of
//      frameKey, so inTrack skips it before any validation (an observation of frameKey that o matches and that moves to
//      another track moves to such a track).
// So, for a session in which every tracked observation is listed in its track, every geometric predicate of the call can be
// computed up front: the triangulation of every candidate (o, o2) whose o2 has no track when the call starts, and the check of
// o against the track o2 holds when the call starts, for the tracks that do not contain frameKey then.  replayCreateTracks
// then takes the integer decisions in the reference's order from those flags.  Over frames [first, last] the triangulations
// are all computed in one call (1. and 2. hold across frames; an o2 untracked at some frame's start was untracked at the
// batch's start); the reprojection checks need the tracks at each frame's start, so they are one call per frame that carries
// that frame's camera, poses and named observations only, and none when no candidate of the frame needs one.  Everything
// is computed by librsba_amd (rsba_track_candidates); a missing device throws std::runtime_error.
#pragma once
#include <chrono>
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "session.hpp"
#include "video_sfm.hpp"

namespace rsba_amd {

// The geometric flags of one createTracks(frameKey) call, per match of each observation of the frame: entry
// ref_offset[obsKey] + j belongs to f.obs[obsKey].matches[j].  kFlagUnknown marks a flag that was not computed; the replay
// throws std::logic_error if it needs one.  kFlagEmptyFrame marks a predicate that needs the pose of an observation whose frame
// has none: the replay throws std::runtime_error("empty frame") when it reaches it, where the reference's getPose throws
// (struct/VideoSfM.cc:105).
constexpr uint8_t kFlagUnknown = 2;
constexpr uint8_t kFlagEmptyFrame = 3;
struct TrackFlags {
  std::vector<size_t> ref_offset;   // [f.obs.size() + 1]
  std::vector<uint8_t> tri;         // createTracks' creation test passed (triangulation, distances, both validations)
  std::vector<double> pt;           // [3 per entry] the triangulated point
  std::vector<uint8_t> reproj;      // vision::sfm::validate of o against the track o2 held when the call started
  TrackFlags() = default;
  explicit TrackFlags(const Frame& f) : ref_offset(f.obs.size() + 1, 0) {
    for (size_t k = 0; k < f.obs.size(); ++k) ref_offset[k + 1] = ref_offset[k] + (f.obs[k].__isset.matches ? f.obs[k].matches.size() : 0);
    tri.assign(ref_offset.back(), kFlagUnknown);
    pt.assign(3 * ref_offset.back(), 0.0);
    reproj.assign(ref_offset.back(), kFlagUnknown);
  }
};

// struct/VideoSfM.h:155-160
inline bool inTrack(const Track& t, const size_t frameKey) {
  for (const ObservationRef& ref : t.obs)
    if ((size_t)ref.frame == frameKey) return true;
  return false;
}

namespace tracks_detail {
inline bool flag(uint8_t v, const char* what) {
  if (v == kFlagEmptyFrame) throw std::runtime_error("empty frame");
  if (v > 1) throw std::logic_error(std::string("createTracks replay: the ") + what + " flag of a candidate it reached was not computed");
  return v != 0;
}
}  // namespace tracks_detail

// reprojectMatches (VideoSfMHandler.cc:231-280) over precomputed flags
inline bool replayReprojectMatches(Session& sess, const size_t frameKey, const size_t obsKey, const SfmOptions& opt, const TrackFlags& g) {
  Observation& o = sess.frames[frameKey].obs[obsKey];
  if (!o.__isset.matches) return false;
  for (size_t j = 0; j < o.matches.size(); ++j) {
    const ObservationRef& ref = o.matches[j];
    const Observation& o2 = sess.frames[(size_t)ref.frame].obs[(size_t)ref.obs];
    if (!o2.__isset.track) continue;
    Track& t = sess.getTrack((size_t)o2.track);
    if (opt.tracks.maxReprojections > 0 && t.obs.size() >= opt.tracks.maxReprojections) continue;
    // the distance gate (:253-256) and the validation (:262) are one flag; both only skip the match, so inTrack may go first
    if (inTrack(t, frameKey)) continue;
    if (tracks_detail::flag(g.reproj[g.ref_offset[obsKey] + j], "reprojection")) {
      o.track = o2.track;
      o.__isset.track = true;
      t.obs.push_back(ObservationRef{(int32_t)frameKey, (int32_t)obsKey, true});
      if (!opt.ceres.const3d && t.obs.size() >= opt.tracks.minReprojections) t.valid = true;
      return true;
    }
  }
  return false;
}

// createTracks (VideoSfMHandler.cc:283-372, the non-synthetic branch) over precomputed flags: the decision replay, a pure host function
inline void replayCreateTracks(Session& sess, const size_t frameKey, const SfmOptions& opt, const TrackFlags& g) {
  Frame& f = sess.frames[frameKey];
  if (g.ref_offset.size() != f.obs.size() + 1) throw std::logic_error("createTracks replay: flags of another frame");
  for (size_t obsKey = 0; obsKey < f.obs.size(); obsKey++) {
    Observation& o = f.obs[obsKey];
    if (!o.__isset.matches) continue;
    replayReprojectMatches(sess, frameKey, obsKey, opt, g);
    if (opt.ceres.const3d || o.__isset.track) continue;
    for (size_t j = 0; j < o.matches.size(); ++j) {
      ObservationRef& ref = o.matches[j];
      if (ref.frame == (int32_t)frameKey) throw std::runtime_error("createTracks: a match inside frame " + std::to_string(frameKey));   // :308
      Frame& f2 = sess.frames[(size_t)ref.frame];
      if (!f2.__isset.poses) throw std::runtime_error("createTracks: a match into frame " + std::to_string(ref.frame) + ", which has no poses");   // :310
      Observation& o2 = f2.obs[(size_t)ref.obs];
      if (o2.__isset.track) continue;
      const size_t k = g.ref_offset[obsKey] + j;
      if (!tracks_detail::flag(g.tri[k], "triangulation")) continue;
      Track nt;                                                          // sess.newTrack(Track(pt, o.color), o.track)
      nt.pt.assign(g.pt.begin() + 3 * k, g.pt.begin() + 3 * k + 3);
      nt.__isset.pt = true;
      o.track = (int32_t)sess.tracks.size();
      sess.tracks.push_back(nt);
      Track& t = sess.tracks.back();
      o2.track = o.track;
      ref.valid = true;
      t.obs.push_back(ref);
      t.obs.push_back(ObservationRef{(int32_t)frameKey, (int32_t)obsKey, true});
      t.valid = (t.obs.size() >= opt.tracks.minReprojections);
      o.__isset.track = o2.__isset.track = true;
      replayReprojectMatches(sess, frameKey, obsKey, opt, g);
    }
  }
}

// evalTracks (VideoSfMHandler.cc:377-410), with the condition as the reference writes it: an observation whose track point
// validate ACCEPTS (:389) leaves its track.  One batched device validation for the frame.
inline void evalTracks(Session& sess, const size_t frameKey, const SfmOptions& opt, int device = 0) {
  Frame& f = sess.frames[frameKey];
  std::vector<size_t> which;
  std::vector<const double*> pts;
  std::vector<std::array<double, 2>> xy;
  for (size_t oi = 0; oi < f.obs.size(); oi++) {
    if (!f.obs[oi].__isset.track) continue;
    which.push_back(oi);
    pts.push_back(sess.getTrack((size_t)f.obs[oi].track).pt.data());
    xy.push_back({f.obs[oi].x, f.obs[oi].y});
  }
  const std::vector<uint8_t> ok = validate(sess, f, opt, pts, xy, device);
  unsigned countObs = 0, countTrack = 0;
  for (size_t n = 0; n < which.size(); ++n) {
    if (!ok[n]) continue;
    const size_t oi = which[n];
    Observation& o = f.obs[oi];
    Track& t = sess.getTrack((size_t)o.track);
    o.__isset.track = false;
    countObs++;
    for (size_t i = 0; i < t.obs.size(); i++) {
      if (t.obs[i].frame == (int32_t)frameKey && t.obs[i].obs == (int32_t)oi) {
        t.obs.erase(t.obs.begin() + (std::ptrdiff_t)i);
        if (t.valid && t.obs.size() < opt.tracks.minReprojections) { t.valid = false; countTrack++; }
        break;
      }
    }
  }
  if (countTrack || countObs) std::cout << countObs << " bad reprojections and " << countTrack << " bad tracks removed" << std::endl;
}

namespace tracks_detail {

// the whole session's frames, and the observations the triangulation candidates name, in the layout of rsba_track_candidates
struct TriangulationBatch {
  std::vector<double> cams, poses;
  std::vector<int32_t> frame_cam;
  std::vector<int64_t> pose_offset;
  std::vector<std::vector<int32_t>> slot;       // [frame][obsKey] -> index in obs_frame / obs_xy, or -1 (allocated on first use)
  std::vector<int32_t> obs_frame;
  std::vector<double> obs_xy;
  explicit TriangulationBatch(const Session& sess) : slot(sess.frames.size()) {
    if (sess.cam.size() != NUM_CAM_PARAMS) throw std::runtime_error("createTracks: session camera");
    cams.assign(sess.cam.begin(), sess.cam.end());
    pose_offset.push_back(0);
    for (const Frame& f : sess.frames) {
      if (f.__isset.cam) {
        if (f.cam.size() != NUM_CAM_PARAMS) throw std::runtime_error("createTracks: frame camera");
        frame_cam.push_back((int32_t)(cams.size() / NUM_CAM_PARAMS));
        cams.insert(cams.end(), f.cam.begin(), f.cam.end());
      } else {
        frame_cam.push_back(0);
      }
      for (const auto& p : f.poses) {
        if (p.size() != NUM_POSE_PARAMS) throw std::runtime_error("createTracks: pose size");
        poses.insert(poses.end(), p.begin(), p.end());
      }
      pose_offset.push_back(pose_offset.back() + (int64_t)f.poses.size());
    }
    if (poses.empty()) poses.assign(NUM_POSE_PARAMS, 0.0);
  }
  bool has_poses(size_t f) const { return pose_offset[f + 1] > pose_offset[f]; }
  int32_t obs(const Session& sess, size_t f, size_t k) {
    if (slot[f].empty()) slot[f].assign(sess.frames[f].obs.size(), -1);
    int32_t& s = slot[f][k];
    if (s < 0) {
      s = (int32_t)obs_frame.size();
      obs_frame.push_back((int32_t)f);
      obs_xy.push_back(sess.frames[f].obs[k].x);
      obs_xy.push_back(sess.frames[f].obs[k].y);
    }
    return s;
  }
  // one device call: tri_ok / tri_pt per candidate (a[c], b[c])
  void run(const Session& sess, const SfmOptions& opt, int device, const std::vector<int32_t>& a, const std::vector<int32_t>& b,
           std::vector<uint8_t>& tri_ok, std::vector<double>& tri_pt) const {
    const size_t n = a.size();
    tri_ok.assign(n, 0); tri_pt.assign(3 * n, 0.0);
    if (n == 0) return;
    const std::vector<uint8_t> request(n, RSBA_TRACK_TRIANGULATE);
    const int32_t scan[2] = {sess.scanlines.at(0), sess.scanlines.at(1)};
    if (rsba_track_candidates(device, cams.data(), (int32_t)(cams.size() / NUM_CAM_PARAMS), frame_cam.data(), (int32_t)frame_cam.size(), poses.data(),
                              pose_offset.data(), sess.rs, scan, opt.model.interpolateRotation, obs_frame.data(), obs_xy.data(), (int64_t)obs_frame.size(),
                              a.data(), b.data(), request.data(), nullptr, (int64_t)n, opt.tracks.sqrdThreshold, (double)opt.tracks.minDistanceToCamera,
                              tri_ok.data(), tri_pt.data(), nullptr) != RSBA_OK)
      throw std::runtime_error(std::string("rsba_amd: ") + rsba_last_error());
  }
};

// the reprojection checks of frame fi's observations obs_keys[c] against track_pt[c] (vision::sfm::validate): one device call
// that carries that frame only (its camera, its poses and the observations named), so its cost follows the frame, not the
// session
inline void reprojection_checks(const Session& sess, size_t fi, const SfmOptions& opt, int device, const std::vector<int32_t>& obs_keys,
                                const std::vector<double>& track_pt, std::vector<uint8_t>& ok) {
  const size_t n = obs_keys.size();
  ok.assign(n, 0);
  if (n == 0) return;
  const Frame& f = sess.frames[fi];
  const std::vector<double>& cam = f.__isset.cam ? f.cam : sess.cam;
  if (cam.size() != NUM_CAM_PARAMS) throw std::runtime_error("createTracks: camera");
  std::vector<double> poses;
  for (const auto& p : f.poses) {
    if (p.size() != NUM_POSE_PARAMS) throw std::runtime_error("createTracks: pose size");
    poses.insert(poses.end(), p.begin(), p.end());
  }
  const int64_t pose_offset[2] = {0, (int64_t)f.poses.size()};
  std::vector<int32_t> slot(f.obs.size(), -1), a(n);
  std::vector<double> xy;
  for (size_t c = 0; c < n; ++c) {
    int32_t& s = slot[(size_t)obs_keys[c]];
    if (s < 0) { s = (int32_t)(xy.size() / 2); xy.push_back(f.obs[(size_t)obs_keys[c]].x); xy.push_back(f.obs[(size_t)obs_keys[c]].y); }
    a[c] = s;
  }
  const std::vector<int32_t> obs_frame(xy.size() / 2, 0);
  const std::vector<uint8_t> request(n, RSBA_TRACK_REPROJECT);
  const int32_t scan[2] = {sess.scanlines.at(0), sess.scanlines.at(1)};
  if (rsba_track_candidates(device, cam.data(), 1, nullptr, 1, poses.data(), pose_offset, sess.rs, scan, opt.model.interpolateRotation, obs_frame.data(),
                            xy.data(), (int64_t)obs_frame.size(), a.data(), nullptr, request.data(), track_pt.data(), (int64_t)n, opt.tracks.sqrdThreshold,
                            (double)opt.tracks.minDistanceToCamera, nullptr, nullptr, ok.data()) != RSBA_OK)
    throw std::runtime_error(std::string("rsba_amd: ") + rsba_last_error());
}

inline const Observation& matched(const Session& sess, const ObservationRef& ref) {
  if (ref.frame < 0 || (size_t)ref.frame >= sess.frames.size() || ref.obs < 0 || (size_t)ref.obs >= sess.frames[(size_t)ref.frame].obs.size())
    throw std::out_of_range("createTracks: a match names no observation");
  return sess.frames[(size_t)ref.frame].obs[(size_t)ref.obs];
}

inline const Track& track_of(const Session& sess, const Observation& o) {
  if (o.track < 0 || (size_t)o.track >= sess.tracks.size()) throw std::out_of_range("createTracks: an observation names no track");
  return sess.tracks[(size_t)o.track];
}

// the checks of frame fi's matches against the tracks as they stand now (the frame's start): those whose o2 has a track that
// does not contain the frame and that maxReprojections leaves open.  Without poses in the frame the entry is kFlagEmptyFrame.
inline void frame_reprojection_flags(const Session& sess, size_t fi, const SfmOptions& opt, int device, TrackFlags& g, int64_t* checks, int64_t* calls) {
  const Frame& f = sess.frames[fi];
  std::vector<int32_t> keys;
  std::vector<size_t> entry;
  std::vector<double> tpt;
  for (size_t k = 0; k < f.obs.size(); ++k) {
    const Observation& o = f.obs[k];
    if (!o.__isset.matches) continue;
    for (size_t j = 0; j < o.matches.size(); ++j) {
      const Observation& o2 = matched(sess, o.matches[j]);
      if (!o2.__isset.track) continue;
      const Track& t = track_of(sess, o2);
      if (opt.tracks.maxReprojections > 0 && t.obs.size() >= opt.tracks.maxReprojections) continue;
      if (inTrack(t, fi)) continue;
      if (f.poses.empty()) { g.reproj[g.ref_offset[k] + j] = kFlagEmptyFrame; continue; }
      if (t.pt.size() != NUM_POINT_PARAMS) throw std::runtime_error("createTracks: a track without a point");
      keys.push_back((int32_t)k);
      entry.push_back(g.ref_offset[k] + j);
      tpt.insert(tpt.end(), t.pt.begin(), t.pt.end());
    }
  }
  if (keys.empty()) return;
  std::vector<uint8_t> ok;
  reprojection_checks(sess, fi, opt, device, keys, tpt, ok);
  for (size_t c = 0; c < keys.size(); ++c) g.reproj[entry[c]] = ok[c];
  if (checks) *checks += (int64_t)keys.size();
  if (calls) *calls += 1;
}

inline double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace tracks_detail

// where the time of a batched createTracks goes (wall clock, host thread): the host gathering, the triangulation call
// (staging, upload, kernels, download), the per-frame reprojection-check calls with their gathering, and the host replay
struct CreateTracksTimes {
  double gather_s = 0, triangulate_s = 0, reproject_s = 0, replay_s = 0, total_s = 0;
  int64_t triangulations = 0, checks = 0, check_calls = 0;
};

// createTracks over frames [first, last], identical to calling createTracks(sess, fi, opt) for fi = first..last in order:
// one device call triangulates every candidate of the range, then each frame makes one reprojection-check call over its own
// observations (none when no candidate of the frame needs one) and replays its decisions.
inline void createTracks(Session& sess, const size_t first, const size_t last, const SfmOptions& opt, int device = 0, CreateTracksTimes* times = nullptr) {
  using tracks_detail::seconds_since;
  const auto t_start = std::chrono::steady_clock::now();
  if (last >= sess.frames.size() || first > last) throw std::out_of_range("createTracks: frame range");
  if (sess.scanlines.size() < 2) throw std::runtime_error("createTracks: session without scanlines");
  if (opt.tracks.synthetic) {                                            // :285-288
    for (size_t fi = first; fi <= last; ++fi) evalTracks(sess, fi, opt, device);
    return;
  }
  CreateTracksTimes tm;
  auto t0 = std::chrono::steady_clock::now();
  tracks_detail::TriangulationBatch batch(sess);
  std::vector<TrackFlags> flags;
  flags.reserve(last - first + 1);
  // every candidate of the creation branch: o2 without a track now.  Matches inside the frame or into a frame without
  // __isset.poses are left to the replay, which throws when it reaches them; a pose-less frame on either side is kFlagEmptyFrame.
  std::vector<int32_t> a, b;
  std::vector<size_t> at_frame, at_entry;
  for (size_t fi = first; fi <= last; ++fi) {
    const Frame& f = sess.frames[fi];
    flags.emplace_back(f);
    for (size_t k = 0; k < f.obs.size(); ++k) {
      const Observation& o = f.obs[k];
      if (!o.__isset.matches) continue;
      for (size_t j = 0; j < o.matches.size(); ++j) {
        const ObservationRef& ref = o.matches[j];
        const Observation& o2 = tracks_detail::matched(sess, ref);
        if (o2.__isset.track) { tracks_detail::track_of(sess, o2); continue; }
        if (opt.ceres.const3d || (size_t)ref.frame == fi) continue;
        if (!batch.has_poses(fi) || !batch.has_poses((size_t)ref.frame)) { flags.back().tri[flags.back().ref_offset[k] + j] = kFlagEmptyFrame; continue; }
        a.push_back(batch.obs(sess, fi, k));
        b.push_back(batch.obs(sess, (size_t)ref.frame, (size_t)ref.obs));
        at_frame.push_back(fi - first);
        at_entry.push_back(flags.back().ref_offset[k] + j);
      }
    }
  }
  tm.gather_s = seconds_since(t0);
  t0 = std::chrono::steady_clock::now();
  {
    std::vector<uint8_t> tri_ok;
    std::vector<double> tri_pt;
    batch.run(sess, opt, device, a, b, tri_ok, tri_pt);
    for (size_t c = 0; c < a.size(); ++c) {
      TrackFlags& g = flags[at_frame[c]];
      g.tri[at_entry[c]] = tri_ok[c];
      for (int q = 0; q < 3; ++q) g.pt[3 * at_entry[c] + q] = tri_pt[3 * c + q];
    }
  }
  tm.triangulate_s = seconds_since(t0);
  tm.triangulations = (int64_t)a.size();
  for (size_t fi = first; fi <= last; ++fi) {
    TrackFlags& g = flags[fi - first];
    t0 = std::chrono::steady_clock::now();
    tracks_detail::frame_reprojection_flags(sess, fi, opt, device, g, &tm.checks, &tm.check_calls);
    tm.reproject_s += seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    replayCreateTracks(sess, fi, opt, g);
    tm.replay_s += seconds_since(t0);
  }
  tm.total_s = seconds_since(t_start);
  if (times) *times = tm;
}

// createTracks (VideoSfMHandler.cc:283-372)
inline void createTracks(Session& sess, const size_t frameKey, const SfmOptions& opt, int device = 0) {
  createTracks(sess, frameKey, frameKey, opt, device);
}

// reprojectMatches (VideoSfMHandler.cc:231-280) on its own: one device call for the observation's checks, then the replay
inline bool reprojectMatches(Session& sess, const size_t frameKey, const size_t obsKey, const SfmOptions& opt, int device = 0) {
  const Frame& f = sess.frames[frameKey];
  TrackFlags g(f);
  const Observation& o = f.obs[obsKey];
  if (!o.__isset.matches || o.matches.empty()) return false;
  if (sess.scanlines.size() < 2) throw std::runtime_error("createTracks: session without scanlines");
  std::vector<int32_t> keys;
  std::vector<size_t> entry;
  std::vector<double> tpt;
  for (size_t j = 0; j < o.matches.size(); ++j) {
    const Observation& o2 = tracks_detail::matched(sess, o.matches[j]);
    if (!o2.__isset.track) continue;
    const Track& t = tracks_detail::track_of(sess, o2);
    if ((opt.tracks.maxReprojections > 0 && t.obs.size() >= opt.tracks.maxReprojections) || inTrack(t, frameKey)) continue;
    if (f.poses.empty()) { g.reproj[g.ref_offset[obsKey] + j] = kFlagEmptyFrame; continue; }
    if (t.pt.size() != NUM_POINT_PARAMS) throw std::runtime_error("createTracks: a track without a point");
    keys.push_back((int32_t)obsKey);
    entry.push_back(g.ref_offset[obsKey] + j);
    tpt.insert(tpt.end(), t.pt.begin(), t.pt.end());
  }
  std::vector<uint8_t> ok;
  tracks_detail::reprojection_checks(sess, frameKey, opt, device, keys, tpt, ok);
  for (size_t c = 0; c < keys.size(); ++c) g.reproj[entry[c]] = ok[c];
  return replayReprojectMatches(sess, frameKey, obsKey, opt, g);
}

}  // namespace rsba_amd
