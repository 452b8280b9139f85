// The facade's choice of linear solver: loads the flat scene file of ba_session.cpp, adds every frame through the CeresHandler
// mirror and solves with the options of VideoSfMHandler::BA (VideoSfMHandler.cc:579-583) except for linear_solver_type, which
// the command line names — ITERATIVE_SCHUR (the solver min_linear_solver_iterations = 3 is meant for) goes to the device's
// preconditioned conjugate gradients, every other type to the exact Schur-complement solver.  Used by tests/test_gpu_pcg.py.
//
//   iterative_schur scene.bin out.bin [ITERATIVE_SCHUR|SPARSE_SCHUR|DENSE_SCHUR]
//   out.bin: initial cost, final cost, iterations, reduced residual blocks, termination, usable, linear solver iterations
//            (7 doubles), poses [F][P][6], points [M][3]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rsba/ceres_handler.hpp"

namespace ceres = rsba_amd::ceres;
using namespace rsba_amd;

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s scene.bin out.bin [ITERATIVE_SCHUR|SPARSE_SCHUR|DENSE_SCHUR]\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror("scene"); return 2; }
  int32_t hd[11]; int64_t N; double huber, reval, covf, motion[3], cam[9];
  if (!rd(f, hd, 11) || !rd(f, &N, 1) || !rd(f, &huber, 1) || !rd(f, &reval, 1) || !rd(f, &covf, 1) || !rd(f, motion, 3) || !rd(f, cam, 9)) return 2;
  const int F = hd[0], P = hd[1], M = hd[2];
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
  if (reval > 0) { opt.ceres.revalidateReprojections = true; opt.tracks.sqrdThreshold = reval; }
  opt.debug.calcCovariances = covf >= 0;
  opt.ceres.constFrameVelocity = motion[0]; opt.ceres.constFrameAcceleration = motion[1]; opt.ceres.interFrameRatio = motion[2];

  const char* type = argc > 3 ? argv[3] : "ITERATIVE_SCHUR";
  ceres::Solver::Options cOpt;
  cOpt.linear_solver_type = !std::strcmp(type, "ITERATIVE_SCHUR") ? ceres::ITERATIVE_SCHUR : !std::strcmp(type, "DENSE_SCHUR") ? ceres::DENSE_SCHUR : ceres::SPARSE_SCHUR;
  cOpt.minimizer_progress_to_stdout = true;
  cOpt.max_num_iterations = hd[10];
  cOpt.min_linear_solver_iterations = 3;
  CeresHandler cs(opt, 0);
  for (int fi = 0; fi < F; ++fi) cs.Add((size_t)fi, sess);
  ceres::Solver::Summary summary = cs.solve(&cOpt);
  std::printf("%s", summary.FullReport().c_str());
  std::printf("linear solver iterations: %d\n", summary.num_linear_solver_iterations);
  if (!summary.IsSolutionUsable()) std::fprintf(stderr, "%s\n", summary.message.c_str());
  FILE* g = std::fopen(argv[2], "wb");
  if (!g) { std::perror("out"); return 2; }
  const double out[7] = {summary.initial_cost, summary.final_cost, (double)summary.iterations.size(), (double)summary.num_residual_blocks_reduced,
                         (double)(int)summary.termination_type, summary.IsSolutionUsable() ? 1.0 : 0.0, (double)summary.num_linear_solver_iterations};
  std::fwrite(out, sizeof(double), 7, g);
  for (const Frame& fr : sess.frames) for (const auto& pose : fr.poses) std::fwrite(pose.data(), sizeof(double), 6, g);
  for (const Track& t : sess.tracks) std::fwrite(t.pt.data(), sizeof(double), 3, g);
  std::fclose(g);
  return summary.IsSolutionUsable() ? 0 : 1;
}
