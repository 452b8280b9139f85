// Host-side mirror of the incremental step of rsba's video pipeline — what the client runs for every frame of a video — over the
// facade, create_tracks.hpp and solve_rs_pnp.hpp:
//   VideoSfMClient::processFrame        /root/reference/src/rsba/VideoSfMClient.cc:231-251
//   VideoSfMHandler::newFrame           /root/reference/src/rsba/VideoSfMHandler.cc:83-98
//   VideoSfMHandler::initialize         /root/reference/src/rsba/VideoSfMHandler.cc:139-148
//   VideoSfMHandler::solve              /root/reference/src/rsba/VideoSfMHandler.cc:415-506
//   VideoSfMHandler::cvCorrespondences  /root/reference/src/rsba/VideoSfMHandler.cc:635-663
//   VideoSfMHandler::solveRsPnP         /root/reference/src/rsba/VideoSfMHandler.cc:668-804
// Same names and argument meaning, with a plain Session& / SfmOptions where the reference takes a session key and its own _opt.  Not
// here: the PLY dumps, printFrame and the progress lines, the RPC.
// The global-shutter attempts of solveRsPnP (:713-733) are cv::solvePnPRansac in three flavours (ITERATIVE with the extrinsic guess, EPNP,
// P3P without a guess).  OpenCV is not a dependency; the three are three native attempts, each made when the one before found at most
// four inliers: the refinement of sampled six-point subsets from the shared guess (rsba_pnp_tasks, shutter GLOBAL); hypotheses from the
// direct linear transform of six points, in EPnP's place (solveGsPnPRansac(..., hypotheses_on_device = true)); hypotheses from the minimal
// solver, three points and a fourth that chooses (solveGsPnPRansacP3P(..., hypotheses_on_device = true), :726-731).  The first two need six
// correspondences, the third four: a frame with exactly five — which the reference accepts (:686) — is localised by the third alone.
// This is functionally the reference's, not bitwise.  The rolling-shutter RANSAC (:737-746) is solveRsPnPRansac as everywhere else.
// One more difference, on purpose: a frame's priorPoses are copied into its poses (:694-696) AND taken as the start of the solve; the
// reference copies them and still starts from its epsilon vectors, so the copy never reaches the solver there.
#pragma once
#include <cmath>
#include <limits>
#include <vector>

#include "ceres_handler.hpp"
#include "create_tracks.hpp"
#include "solve_rs_pnp.hpp"

namespace rsba_amd {

// VideoSfMHandler.cc:635-663: the 3-D point of every observation that has one — its own track first, otherwise the first of its matches
// whose track has a point — appended to pts [.][3] / obs [.][2] (float, as cv::Point3f / cv::Point2f)
inline void cvCorrespondences(const Frame& f, const Session& sess, std::vector<float>& pts, std::vector<float>& obs, bool useOnlyValid = true) {
  auto push = [&](const Track& t, const Observation& o) {
    for (int k = 0; k < 3; ++k) pts.push_back((float)t.pt[(size_t)k]);
    obs.push_back((float)o.x); obs.push_back((float)o.y);
  };
  for (const Observation& o : f.obs) {
    if (o.__isset.track) {
      const Track& t = sess.getTrack((size_t)o.track);
      if ((t.valid || !useOnlyValid) && t.__isset.pt) { push(t, o); continue; }   // next observation
    }
    for (const ObservationRef& ref : o.matches) {
      const Observation& o2 = sess.frames[(size_t)ref.frame].obs[(size_t)ref.obs];
      if (!o2.__isset.track) continue;
      const Track& t = sess.getTrack((size_t)o2.track);
      if ((t.valid || !useOnlyValid) && t.__isset.pt) { push(t, o); break; }     // next observation
    }
  }
}

// VideoSfMHandler.cc:668-804: the pose(s) of the LAST frame of the session from its 2-D / 3-D correspondences.  false: not enough
// correspondences, or no attempt found more than four inliers — the frame is left as it was.
inline bool solveRsPnP(Session& sess, const SfmOptions& opt, const int32_t maxIter = 20, int device = 0, bool progress = true) {
  const size_t frameKey = sess.frames.size() - 1;
  Frame& f = sess.frames[frameKey];
  const double* cam = f.__isset.cam ? f.cam.data() : sess.cam.data();
  std::vector<float> pts, obs;
  cvCorrespondences(f, sess, pts, obs);
  if (pts.size() / 3 <= 4) cvCorrespondences(f, sess, pts, obs, false);   // "Using all tracks!" (:681-684; appended to what was found, as there)
  const int n = (int)(pts.size() / 3);
  if (n <= 4) return false;                                               // :798-800

  const double eps = std::numeric_limits<double>::epsilon();              // _EPS: not all zero, so solveRsPnPRansac runs no GS initialisation of its own (:690-691)
  double rvec[3] = {eps, eps, eps}, tvec[3] = {eps, eps, eps}, rvec2[3], tvec2[3];
  bool two_starts = false;
  if (f.__isset.priorPoses && !f.priorPoses.empty()) {                    // :694-696 (and the start of the solve, see the header)
    f.poses = f.priorPoses;
    hyp_detail::from_pose(f.poses[0].data(), rvec, tvec);
    if (f.poses.size() > 1) { hyp_detail::from_pose(f.poses[1].data(), rvec2, tvec2); two_starts = true; }
  } else if (opt.mod_init.reuseLastPose && frameKey > 0) {                // :697-711
    const std::vector<double>* pose = nullptr;
    if (f.poses.size() > 1) pose = &f.poses[0];
    else if (!sess.frames[frameKey - 1].poses.empty()) pose = &sess.frames[frameKey - 1].poses.back();   // the last pose
    if (pose) hyp_detail::from_pose(pose->data(), rvec, tvec);
  }

  int inliers = 0;
  if (opt.mod_init.solveGsPnP) {                                          // :713-733
    const int iterations = 500, m = 6;
    const float threshold = (float)(std::sqrt(opt.tracks.sqrdThreshold) * 2);
    const uint64_t seed = 0x9e3779b97f4a7c15ULL;
    if (opt.mod_init.reuseLastPose && n >= m) {   // useExtrinsicGuess: every sampled subset refined from the shared guess
      const std::vector<int32_t> subsets = hyp_detail::distinct_subsets(n, m, iterations, seed);
      double init[12];
      hyp_detail::to_pose(rvec, tvec, init);
      for (int k = 0; k < 6; ++k) init[6 + k] = init[k];
      std::vector<double> poses((size_t)iterations * 12);
      std::vector<uint8_t> status((size_t)iterations);
      std::vector<int32_t> count((size_t)iterations);
      const int32_t sl[2] = {0, 1};
      hyp_detail::check(rsba_pnp_tasks(device, cam, (int32_t)GLOBAL, sl, pts.data(), obs.data(), n, subsets.data(), m, iterations, init, 0, 5, 0, threshold,
                                       poses.data(), status.data(), nullptr, count.data()));
      const int best = hyp_detail::most_inliers(status.data(), count.data(), iterations, [](uint8_t st) { return st == 1; });
      if (best >= 0 && count[(size_t)best] > 4) { inliers = count[(size_t)best]; hyp_detail::from_pose(&poses[(size_t)best * 12], rvec, tvec); }
    }
    if (inliers <= 4) {                           // no extrinsic guess: hypotheses from the DLT, on the device
      double gs[6];
      const int found = solveGsPnPRansac(pts.data(), obs.data(), n, cam, gs, iterations, threshold, m, seed, device, true);
      if (found > 4) { inliers = found; hyp_detail::from_pose(gs, rvec, tvec); }
    }
    if (inliers <= 4) {                           // :726-731, CV_P3P without a guess: hypotheses from the minimal solver, on the device
      double gs[6];
      const int found = solveGsPnPRansacP3P(pts.data(), obs.data(), n, cam, gs, iterations, threshold, seed, device, true);
      if (found > 4) { inliers = found; hyp_detail::from_pose(gs, rvec, tvec); }
    }
    two_starts = false;
  }
  if (!two_starts) for (int k = 0; k < 3; ++k) { rvec2[k] = rvec[k]; tvec2[k] = tvec[k]; }   // :735

  if (opt.model.rolling_shutter && opt.mod_init.solveRsPnP) {             // :737-746
    const int scan[2] = {sess.scanlines[0], sess.scanlines[1]};
    std::vector<int> inl;
    solveRsPnPRansac(pts.data(), obs.data(), n, cam, rvec, tvec, rvec2, tvec2, (SHUTTER)sess.rs, scan, 1000, (float)std::sqrt(opt.tracks.sqrdThreshold),
                     (int)(n * .7), &inl, (int)opt.mod_init.minPnPfeatures, 0xffffffffULL, device, true);
    inliers = (int)inl.size();
  }

  if (!(inliers > 4 || (!opt.mod_init.solveGsPnP && !opt.mod_init.solveRsPnP))) return false;   // :748, :795-797
  std::vector<double> pose(NUM_POSE_PARAMS);
  hyp_detail::to_pose(rvec, tvec, pose.data());
  f.poses.assign(opt.model.rolling_shutter ? 2 : 1, pose);               // :751-759
  f.__isset.poses = true;
  if (f.poses.size() == 2) hyp_detail::to_pose(rvec2, tvec2, f.poses[1].data());   // :761-767

  if (opt.mod_init.refinePnP) {                                           // :769-792
    createTracks(sess, frameKey, opt, device);
    SfmOptions o(opt);
    o.ceres.const3d = true;
    o.model.calibrated = true;
    o.ceres.fixScale = false;
    BA(sess, (int32_t)frameKey, (int32_t)frameKey, o, maxIter, nullptr, progress);
  }
  return true;
}

// VideoSfMHandler.cc:415-506: initialise the frame and search for good tracks.  Returns whether the frame has poses afterwards.
inline bool solve(Session& sess, const int32_t frameKey, const SfmOptions& options, int device = 0, bool progress = true) {
  if (sess.frames[(size_t)frameKey].obs.empty()) return sess.frames[(size_t)frameKey].__isset.poses;
  if (!sess.frames[(size_t)frameKey].__isset.poses) solveRsPnP(sess, options, 20, device, progress);   // (the last frame of the session, as there: :424, :671)
  Frame& f = sess.frames[(size_t)frameKey];
  if ((!f.__isset.poses || options.ceres.pnpNewFrame) && (unsigned)frameKey >= options.tracks.minReprojections) {   // :427-486 "Direct PnP"
    ceres::Solver::Options cOpt;
    cOpt.linear_solver_type = ceres::SPARSE_SCHUR;
    cOpt.minimizer_progress_to_stdout = progress;
    cOpt.max_num_iterations = (int)options.ceres.baIterationsOnNewFrame;
    SfmOptions opt = options;                                             // alternative options for PnP
    opt.ceres.const3d = true;
    if (opt.ceres.useOnlyValidMatches) {                                  // :437-457
      size_t ntracks = 0;
      for (const Observation& o : f.obs)
        for (const ObservationRef& ref : o.matches) {
          const Observation& o2 = sess.frames[(size_t)ref.frame].obs[(size_t)ref.obs];
          if (o2.__isset.track && sess.getTrack((size_t)o2.track).valid) { ntracks++; break; }
        }
      if (ntracks < 100) opt.ceres.useOnlyValidMatches = false;           // "!!! Not enough valid matches !!!"
    }
    opt.ceres.fixScale = false;                                           // :470-485
    CeresHandler solver2(opt);
    solver2.Add((size_t)frameKey, sess, true);
    solver2.solve(&cOpt);
  }
  if (f.__isset.poses) createTracks(sess, (size_t)frameKey, options, device);   // :488-492
  return f.__isset.poses;
}

// VideoSfMHandler.cc:83-98: add a frame and return its key; new tracks are generated where matches are available
inline int32_t newFrame(Session& sess, const Frame& frame, const SfmOptions& opt, int device = 0, bool progress = true) {
  const size_t frameKey = sess.frames.size();
  sess.frames.push_back(frame);
  solve(sess, (int32_t)frameKey, opt, device, progress);
  return (int32_t)frameKey;
}

// VideoSfMClient.cc:231-251: newFrame, then the windowed bundle adjustment over the last baWindowOnNewFrame frames (or all of them), tracks
// re-created.  Returns whether the frame is localised and the bundle adjustment, where it ran, gave a usable solution; *key = the frame's key.
inline bool processFrame(Session& sess, const Frame& frame, const SfmOptions& opt, int32_t* key = nullptr, int device = 0, bool progress = true) {
  const int32_t frameKey = newFrame(sess, frame, opt, device, progress);
  if (key) *key = frameKey;
  bool ok = sess.frames[(size_t)frameKey].__isset.poses;
  if (opt.ceres.baIterationsOnNewFrame > 0 && (unsigned)frameKey + 1 >= opt.tracks.minReprojections) {   // improve solution (:241-247)
    const unsigned w = opt.ceres.baWindowOnNewFrame;
    const int32_t start = (w && (unsigned)frameKey >= w) ? (int32_t)(1 + (unsigned)frameKey - w) : 0;
    ok = windowedBA(sess, opt, start, frameKey, (int32_t)opt.ceres.baIterationsOnNewFrame, nullptr, progress, nullptr, true) && ok;
  }
  return ok;
}

// VideoSfMHandler.cc:139-148: initialize frame poses — one bundle adjustment over every frame, tracks re-created
inline bool initialize(Session& sess, const SfmOptions& opt, bool progress = true) {
  return BA(sess, 0, (int32_t)sess.frames.size() - 1, opt, 20, nullptr, progress, nullptr, true);
}

}  // namespace rsba_amd
