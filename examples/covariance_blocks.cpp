// ceres::Covariance beyond the blocks of one frame: loads the flat scene file of ba_session.cpp, adds every frame through the
// CeresHandler mirror (no solve: the covariance is taken at the parameters of the file) and asks the facade for
//   1. the (p0,p0), (p0,p1), (p1,p1) blocks of frame A — the request VideoSfMHandler::BA makes, served frame by frame as before;
//   2. in ONE request: the pose blocks between frame A and frame B, those of frame A again, the block of the first point frame A
//      sees and, uncalibrated sessions, the intrinsics block — served by one selected inverse on the device
//      (rsba_covariance_compute); the blocks of (B, A), which were not asked for, come back as the transposes of (A, B);
//   3. a pose of frame A against a point: not served, Compute() must say so.
// Used by tests/test_gpu_cov_blocks.py.
//
//   covariance_blocks scene.bin out.bin A B
//   out.bin (doubles): ok of request 1, 2, 3; [CD][CD] of (A, A) by request 1; [CD][CD] of (A, A), of (A, B), [9][9] intrinsics by
//   request 2; then the point's index, its [3][3] block and [CD][CD] of (B, A) by request 2 (zeros where not asked or not served)
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "rsba/ceres_handler.hpp"

namespace ceres = rsba_amd::ceres;
using namespace rsba_amd;

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: %s scene.bin out.bin A B\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror("scene"); return 2; }
  int32_t hd[11]; int64_t N; double huber, reval, covf, motion[3], cam[9];
  if (!rd(f, hd, 11) || !rd(f, &N, 1) || !rd(f, &huber, 1) || !rd(f, &reval, 1) || !rd(f, &covf, 1) || !rd(f, motion, 3) || !rd(f, cam, 9)) return 2;
  const int F = hd[0], P = hd[1], M = hd[2], CD = 6 * P;
  const int A = std::atoi(argv[3]), B = std::atoi(argv[4]);
  if (A < 0 || A >= F || B < 0 || B >= F) { std::fprintf(stderr, "frames out of range\n"); return 2; }
  std::vector<double> poses((size_t)F * P * 6), points((size_t)M * 3), xy((size_t)N * 2);
  std::vector<int32_t> of(N), op(N);
  if (!rd(f, poses.data(), poses.size()) || !rd(f, points.data(), points.size()) || !rd(f, xy.data(), xy.size()) || !rd(f, of.data(), N) || !rd(f, op.data(), N)) return 2;
  std::fclose(f);

  Session sess;
  sess.cam.assign(cam, cam + 9);
  sess.rs = hd[3]; sess.scanlines = {hd[4], hd[5]}; sess.width = 1280; sess.height = 720;
  sess.frames.resize(F); sess.tracks.resize(M);
  for (int i = 0; i < F; ++i) {
    sess.frames[i].__isset.poses = true;
    for (int q = 0; q < P; ++q) sess.frames[i].poses.emplace_back(poses.begin() + ((size_t)i * P + q) * 6, poses.begin() + ((size_t)i * P + q + 1) * 6);
  }
  for (int j = 0; j < M; ++j) { sess.tracks[j].pt.assign(points.begin() + (size_t)j * 3, points.begin() + (size_t)j * 3 + 3); sess.tracks[j].__isset.pt = true; sess.tracks[j].valid = true; }
  for (int64_t i = 0; i < N; ++i) {
    Observation o; o.x = xy[2 * i]; o.y = xy[2 * i + 1]; o.track = op[i]; o.__isset.track = true;
    ObservationRef ref; ref.frame = of[i]; ref.obs = (int32_t)sess.frames[of[i]].obs.size(); ref.valid = true;
    sess.tracks[op[i]].obs.push_back(ref);
    sess.frames[of[i]].obs.push_back(o);
  }
  SfmOptions opt;
  opt.model.rolling_shutter = P == 2; opt.model.calibrated = hd[6] != 0; opt.model.interpolateRotation = hd[7] != 0;
  opt.ceres.fixFirstNCameras = (unsigned)hd[8]; opt.ceres.fixScale = hd[9] != 0; opt.ceres.huberLoss = huber;
  opt.ceres.constFrameVelocity = motion[0]; opt.ceres.constFrameAcceleration = motion[1]; opt.ceres.interFrameRatio = motion[2];
  (void)reval; (void)covf;
  CeresHandler cs(opt, 0);
  for (int fi = 0; fi < F; ++fi) cs.Add((size_t)fi, sess);

  typedef std::vector<std::pair<const double*, const double*>> Blocks;
  const Frame &fa = sess.frames[(size_t)A], &fb = sess.frames[(size_t)B];
  // the [CD][CD] block of two frames out of the facade's 6 x 6 blocks
  auto frame_block = [&](const ceres::Covariance& c, const Frame& x, const Frame& y, double* out) {
    bool ok = true;
    for (int q = 0; q < P; ++q) for (int r = 0; r < P; ++r) {
      double blk[36];
      ok = c.GetCovarianceBlock(x.poses[q].data(), y.poses[r].data(), blk) && ok;
      for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) out[(size_t)(6 * q + a) * CD + 6 * r + b] = blk[a * 6 + b];
    }
    return ok;
  };
  std::vector<double> out(3 + 3 * (size_t)CD * CD + 81 + 10 + (size_t)CD * CD, 0.0);
  double* same1 = &out[3]; double* same2 = same1 + (size_t)CD * CD; double* cross = same2 + (size_t)CD * CD; double* intr = cross + (size_t)CD * CD;
  double* point = intr + 81; double* back = point + 10;
  int track = -1;
  for (const Observation& o : fa.obs) if (o.__isset.track) { track = o.track; break; }
  const double* pt = track >= 0 ? sess.tracks[(size_t)track].pt.data() : nullptr;
  point[0] = (double)track;
  {
    Blocks blocks;
    for (int q = 0; q < P; ++q) for (int r = q; r < P; ++r) blocks.push_back(std::make_pair(fa.poses[q].data(), fa.poses[r].data()));
    ceres::Covariance c;
    bool ok = c.Compute(blocks, &cs.problem);
    if (ok) {   // (the facade serves the blocks that were asked for: the upper triangle of the frame's pose pairs, as BA asks)
      for (int q = 0; q < P; ++q) for (int r = q; r < P; ++r) {
        double blk[36];
        ok = c.GetCovarianceBlock(fa.poses[q].data(), fa.poses[r].data(), blk) && ok;
        for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) {
          same1[(size_t)(6 * q + a) * CD + 6 * r + b] = blk[a * 6 + b];
          if (r != q) same1[(size_t)(6 * r + b) * CD + 6 * q + a] = blk[a * 6 + b];   // (the block below the diagonal was not asked for: the transpose)
        }
      }
    }
    out[0] = ok ? 1.0 : 0.0;
    std::printf("frame %d on its own: %s\n", A, ok ? "ok" : "refused");
  }
  {
    Blocks blocks;
    for (int q = 0; q < P; ++q) for (int r = 0; r < P; ++r) {
      blocks.push_back(std::make_pair(fa.poses[q].data(), fb.poses[r].data()));
      blocks.push_back(std::make_pair(fa.poses[q].data(), fa.poses[r].data()));
    }
    if (!opt.model.calibrated) blocks.push_back(std::make_pair(sess.cam.data(), sess.cam.data()));
    if (pt) blocks.push_back(std::make_pair(pt, pt));
    ceres::Covariance c;
    bool ok = c.Compute(blocks, &cs.problem);
    if (ok) {
      ok = frame_block(c, fa, fa, same2) && ok;
      ok = frame_block(c, fa, fb, cross) && ok;
      ok = frame_block(c, fb, fa, back) && ok;
      if (pt) ok = c.GetCovarianceBlock(pt, pt, point + 1) && ok;
      if (!opt.model.calibrated) ok = c.GetCovarianceBlock(sess.cam.data(), sess.cam.data(), intr) && ok;
    }
    out[1] = ok ? 1.0 : 0.0;
    std::printf("frames %d and %d, point %d%s in one request: %s\n", A, B, track, opt.model.calibrated ? "" : " and the intrinsics", ok ? "ok" : "refused");
  }
  {
    Blocks blocks;
    blocks.push_back(std::make_pair(fa.poses[0].data(), pt ? pt : fa.poses[0].data()));
    ceres::Covariance c;
    const bool ok = pt && c.Compute(blocks, &cs.problem);
    out[2] = ok ? 1.0 : 0.0;
    std::printf("a pose of frame %d against a point: %s\n", A, ok ? "ok" : "refused");
  }
  FILE* g = std::fopen(argv[2], "wb");
  if (!g) { std::perror("out"); return 2; }
  std::fwrite(out.data(), sizeof(double), out.size(), g);
  std::fclose(g);
  return 0;
}
