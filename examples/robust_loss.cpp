// The facade's loss functions: loads the flat scene file of ba_session.cpp, adds every frame through the CeresHandler mirror with the
// loss the command line names in place of the handler's HuberLoss, and solves with the options of VideoSfMHandler::BA.  The facade
// lowers the loss to rsba_set_loss; a loss it cannot lower (here: a user-defined class) fails the solve with a message.
// Used by tests/test_gpu_loss.py.
//
//   robust_loss scene.bin out.bin LOSS      LOSS: trivial | huber:A | softlone:A | cauchy:A | arctan:A | tolerant:A:B | user,
//                                                 or scaled:S:<one of those>   (ScaledLoss(new ..., S, TAKE_OWNERSHIP))
//   out.bin: initial cost, final cost, iterations, reduced residual blocks, termination, usable, 0 (7 doubles), poses [F][P][6], points [M][3]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rsba/ceres_handler.hpp"

namespace ceres = rsba_amd::ceres;
using namespace rsba_amd;

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

// a loss the library does not know: the caller's own class
class UserLoss : public ceres::LossFunction {
 public:
  void Evaluate(double s, double rho[3]) const override { rho[0] = s; rho[1] = 1.0; rho[2] = 0.0; }
};

static ceres::LossFunction* parse_loss(std::string spec) {
  auto next = [&spec]() { const size_t k = spec.find(':'); std::string t = spec.substr(0, k); spec = k == std::string::npos ? "" : spec.substr(k + 1); return t; };
  const std::string kind = next();
  if (kind == "scaled") { const double s = std::atof(next().c_str()); return new ceres::ScaledLoss(parse_loss(spec), s, ceres::TAKE_OWNERSHIP); }
  if (kind == "trivial") return new ceres::TrivialLoss;
  if (kind == "user") return new UserLoss;
  const double a = std::atof(next().c_str());
  if (kind == "huber") return new ceres::HuberLoss(a);
  if (kind == "softlone") return new ceres::SoftLOneLoss(a);
  if (kind == "cauchy") return new ceres::CauchyLoss(a);
  if (kind == "arctan") return new ceres::ArctanLoss(a);
  if (kind == "tolerant") return new ceres::TolerantLoss(a, std::atof(next().c_str()));
  return nullptr;
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s scene.bin out.bin LOSS\n", argv[0]); return 2; }
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
  opt.ceres.fixFirstNCameras = (unsigned)hd[8]; opt.ceres.fixScale = hd[9] != 0; opt.ceres.huberLoss = 0; (void)huber;   // (the loss comes from the command line)
  if (reval > 0) { opt.ceres.revalidateReprojections = true; opt.tracks.sqrdThreshold = reval; }
  opt.debug.calcCovariances = covf >= 0;
  opt.ceres.constFrameVelocity = motion[0]; opt.ceres.constFrameAcceleration = motion[1]; opt.ceres.interFrameRatio = motion[2];

  ceres::Solver::Options cOpt;
  cOpt.linear_solver_type = ceres::SPARSE_SCHUR;
  cOpt.minimizer_progress_to_stdout = true;
  cOpt.max_num_iterations = hd[10];
  CeresHandler cs(opt, 0);
  cs.lossFunction = parse_loss(argv[3]);   // one loss shared by every block, where the handler puts its HuberLoss (the problem owns it)
  if (!cs.lossFunction) { std::fprintf(stderr, "unknown loss %s\n", argv[3]); return 2; }
  for (int fi = 0; fi < F; ++fi) cs.Add((size_t)fi, sess);
  ceres::Solver::Summary summary = cs.solve(&cOpt);
  std::printf("%s", summary.FullReport().c_str());
  if (!summary.IsSolutionUsable()) std::fprintf(stderr, "%s\n", summary.message.c_str());
  FILE* g = std::fopen(argv[2], "wb");
  if (!g) { std::perror("out"); return 2; }
  const double out[7] = {summary.initial_cost, summary.final_cost, (double)summary.iterations.size(), (double)summary.num_residual_blocks_reduced,
                         (double)(int)summary.termination_type, summary.IsSolutionUsable() ? 1.0 : 0.0, 0.0};
  std::fwrite(out, sizeof(double), 7, g);
  for (const Frame& fr : sess.frames) for (const auto& pose : fr.poses) std::fwrite(pose.data(), sizeof(double), 6, g);
  for (const Track& t : sess.tracks) std::fwrite(t.pt.data(), sizeof(double), 3, g);
  std::fclose(g);
  return summary.IsSolutionUsable() ? 0 : 1;
}
