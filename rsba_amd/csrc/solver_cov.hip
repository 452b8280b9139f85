// The covariance entry points of the C ABI, over the solver's plan and factorisation (solver.hpp): one frame's block by unit-vector
// solves (rsba_pose_covariance), every frame and point by the selected inverse (rsba_covariance_compute and its getters).
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "solver.hpp"

using namespace rsba;

// Covariance of one frame's pose block(s): the (frame, frame) block of (J^T J)^-1, J = loss-corrected Jacobian of the
// problem at the current parameters on the tangent space of its parameterizations — what ceres::Covariance returns
// for the blocks (p0,p0), (p0,p1), (p1,p1) that VideoSfMHandler::BA asks for (VideoSfMHandler.cc:602-621).
// It is the same block of the inverse of the reduced camera system: S without damping and without Jacobi scaling
// (radius 1e300: fixed coordinates keep a vanishing, decoupled diagonal instead of an exact zero), one solve per
// unit vector through the factorisation.  Fixed coordinates have zero covariance.
extern "C" int32_t rsba_pose_covariance(rsba_handle* h, int32_t frame, double* cov) {
  if (!h || !cov) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (frame < 0 || frame >= h->dp.F) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "frame out of range");
  RSBA_HIP_TRY(hipSetDevice(h->device));
  int32_t rc = build_solver(h);
  if (rc) return rc;
  Solver* s = h->solver; SolverDev& sv = s->sv; hipStream_t st = h->stream; const int CD = sv.CD;
  if ((rc = reset_scales(h))) return rc;
  if ((rc = linearize(h))) return rc;
  RSBA_HIP_TRY(launch_clamp_diagonal(h->dp, sv, 1e-6, 1e32, st));   // only its floor matters: the decoupled diagonal of fixed coordinates
  RSBA_HIP_TRY(launch_pose_prior_clamp(h->dp, s->pp, 1e-6, 1e32, st));
  RSBA_HIP_TRY(hipMemsetAsync(sv.chol_fail, 0, sizeof(int), st));
  // (CD + 1 right-hand sides through ONE factorisation: the substitution-only solves walk every column's factor tiles, so a sharded
  // plan takes its replicated form here — the whole of S summed onto every rank)
  struct ShardedOff { Solver* s; bool was; ~ShardedOff() { s->sharded_off = was; } } sharded_guard{s, s->sharded_off};
  s->sharded_off = true;
  if ((rc = reduce_system(h, 1e300))) return rc;
  if (s->hp.two_rhs) RSBA_HIP_TRY(launch_ratio_prepare(s->ratio4, 1.0, 0.0, 0.0, st));   // (a plan that carries the ratio's column through its factorisation: s eta = 0 here — the plain solves S y = e_k)
  std::vector<double> col((size_t)CD * CD, 0.0);
  const double one = 1.0;
  // CD (+1 with the border) solves through the factorisation; the DAG driver's verification flag is sticky, so one read after
  // the last solve covers them all — a suspect result is thrown away and the solves are repeated on the level schedule
  const bool levels_before = s->use_levels;
  std::vector<double> vf; double hb[3] = {0.0, 0.0, 0.0};
  for (int attempt = 0; attempt < 2; ++attempt) {
  RSBA_HIP_TRY(hipMemsetAsync(sv.scalars + kDagSuspect, 0, sizeof(double), st));
  for (int k = 0; k < CD; ++k) {
    RSBA_HIP_TRY(hipMemsetAsync(sv.rhs, 0, (size_t)sv.npad * sizeof(double), st));
    RSBA_HIP_TRY(hipMemcpyAsync(sv.rhs + (size_t)frame * CD + k, &one, sizeof(double), hipMemcpyHostToDevice, st));
    const double* y = sv.yv;
    if (k == 0) { if ((rc = solve_reduced_system(h))) return rc; y = sv.yv; }   // the factorisation, once; every other column is a pair of substitutions
    else if ((rc = solve_again(h, sv.rhs, &y))) return rc;
    RSBA_HIP_TRY(hipMemcpyAsync(&col[(size_t)k * CD], y + (size_t)frame * CD, (size_t)CD * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  // A free interFrameRatio is one more parameter block of J^T J, coupled to every pose through its column b (the 1-wide
  // border of the reduced system, diagonal entry h): by the block inverse the pose block of the bordered system is
  // S^-1 + v v^T / (h - b.v) with S v = b — what ceres::Covariance returns for the problem CeresHandler builds by default.
  if (s->border) {
    const double* v = nullptr;
    if ((rc = solve_again(h, s->border, &v))) return rc;
    RSBA_HIP_TRY(launch_border_dots(s->border, v, v, sv.npad, s->ratio4 + 2, st));
    vf.resize(CD);
    RSBA_HIP_TRY(hipMemcpyAsync(vf.data(), v + (size_t)frame * CD, (size_t)CD * sizeof(double), hipMemcpyDeviceToHost, st));
    RSBA_HIP_TRY(hipMemcpyAsync(hb, s->ratio4, sizeof hb, hipMemcpyDeviceToHost, st));     // {h, g, b.v}
  }
  double suspect = 0.0;
  if ((rc = await_verification(h))) return rc;
  RSBA_HIP_TRY(hipMemcpyAsync(&suspect, sv.scalars + kDagSuspect, sizeof(double), hipMemcpyDeviceToHost, st));
  RSBA_HIP_TRY(hipStreamSynchronize(st));
  if (suspect == 0.0 || s->use_levels) break;
  s->use_levels = true; ++s->dag_fallbacks;
  }
  s->use_levels = levels_before;
  int fail = 0, nfail = 0;
  std::vector<double> ud(CD, 0.0);   // diag(U) of the frame: exactly zero where no residual touches the coordinate
  RSBA_HIP_TRY(hipMemcpyAsync(&fail, sv.chol_fail, sizeof(int), hipMemcpyDeviceToHost, st));
  RSBA_HIP_TRY(hipMemcpyAsync(&nfail, h->dp.fail_count, sizeof(int), hipMemcpyDeviceToHost, st));
  RSBA_HIP_TRY(hipMemcpyAsync(ud.data(), sv.udiag + (size_t)frame * CD, (size_t)CD * sizeof(double), hipMemcpyDeviceToHost, st));
  RSBA_HIP_TRY(hipStreamSynchronize(st));
  if (nfail) return rsba_set_error(RSBA_ERR_EVALUATION_FAILED, "residual and Jacobian evaluation failed");
  if (fail) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "J^T J is rank deficient (fix the gauge): no covariance, as ceres::Covariance::Compute returns false");
  double border_scale = 0.0;
  if (s->border) {
    const double schur = hb[0] - hb[2];    // the ratio's own pivot of the bordered system
    if (!(schur > 0.0) || !std::isfinite(schur)) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "J^T J is rank deficient in the interFrameRatio: no covariance");
    border_scale = 1.0 / schur;
  }
  for (int a = 0; a < CD; ++a) for (int b = 0; b < CD; ++b) {
    // (a coordinate no residual touches — a frame without observations or priors — is not a parameter of the program: like a fixed
    // one it sits in S as a vanishing, decoupled diagonal, whose inverse is not a covariance)
    const double ma = ud[a] != 0.0 ? h->mask_pose[(size_t)frame * CD + a] : 0.0, mb = ud[b] != 0.0 ? h->mask_pose[(size_t)frame * CD + b] : 0.0;
    cov[(size_t)a * CD + b] = (ma != 0.0 && mb != 0.0) ? col[(size_t)b * CD + a] + (s->border ? vf[a] * vf[b] * border_scale : 0.0) : 0.0;
  }
  return RSBA_OK;
}

// ---- covariance of every frame: the selected inverse of the undamped reduced camera system (kernels_selinv.hip) ----
// rsba_covariance_compute linearises and factors exactly as rsba_pose_covariance does, then runs the Takahashi recurrence over the
// factor's own tile pattern into a tile array of its own — every (f, f) block, every (f, g) block whose tile the factor has and the
// intrinsics blocks are then one gather away (rsba_covariance_frame_blocks / rsba_covariance_intrinsics_block).
void rsba_covariance_invalidate(rsba_handle* h) { if (h && h->solver) h->solver->cov.valid = false; }

namespace {
// RSBA_COV_TIMES=1: HIP events around the covariance kernels (rsba_covariance_times; tools/cov_time.py).  Off, no event is created.
bool cov_times_on() { static const bool on = cov_times_switch(); return on; }
// one kernel between two events, where the times are asked for
struct CovStopwatch {
  hipEvent_t t0 = nullptr, t1 = nullptr; bool on = cov_times_on();
  ~CovStopwatch() { if (t0) (void)hipEventDestroy(t0); if (t1) (void)hipEventDestroy(t1); }
  hipError_t start(hipStream_t st) { if (!on) return hipSuccess; hipError_t e = hipEventCreate(&t0); if (e == hipSuccess) e = hipEventCreate(&t1); return e == hipSuccess ? hipEventRecord(t0, st) : e; }
  hipError_t stop(hipStream_t st) { return on ? hipEventRecord(t1, st) : hipSuccess; }
  void read(double* ms) { float f = 0.f; if (on && t0 && t1 && hipEventElapsedTime(&f, t0, t1) == hipSuccess) *ms = f; }   // (after the stream's synchronisation)
};
int32_t covariance_ready(rsba_handle* h) {
  if (!h) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null handle");
  if (!h->solver || !h->solver->cov.valid) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "no covariance computed (rsba_covariance_compute comes first, and again after anything that changes the parameters or the problem)");
  return RSBA_OK;
}
// n blocks of dim x dim entries of Sigma: block p starts at camera-side scalar row row0[p], column col0[p] (a block may cross one tile
// edge each way).  *missing = the first block that needs a tile the factor's pattern does not have (-1: none; nothing was gathered then)
int32_t covariance_gather(rsba_handle* h, const std::vector<int64_t>& row0, const std::vector<int64_t>& col0, int dim, double* out, int64_t* missing) {
  Solver* s = h->solver; hipStream_t st = h->stream;
  const int64_t n = (int64_t)row0.size();
  *missing = -1;
  if (n == 0) return RSBA_OK;
  std::vector<int32_t> desc(8 * (size_t)n, -1);
  for (int64_t p = 0; p < n; ++p) {
    int32_t* d = &desc[8 * (size_t)p];
    d[0] = (int32_t)row0[p]; d[1] = (int32_t)col0[p];
    const int tr0 = (int)(row0[p] / kTile), tc0 = (int)(col0[p] / kTile);
    const int nr = (row0[p] % kTile + dim > kTile) ? 2 : 1, nc = (col0[p] % kTile + dim > kTile) ? 2 : 1;
    for (int x = 0; x < nr; ++x) for (int y = 0; y < nc; ++y) {
      const int pi = s->hp.iperm[tr0 + x], pj = s->hp.iperm[tc0 + y];
      const int32_t slot = pi >= pj ? s->hp.slot_of(pi, pj) : s->hp.slot_of(pj, pi);
      if (slot < 0) { *missing = p; return RSBA_OK; }
      d[2 + 2 * x + y] = 2 * slot + (pi < pj ? 1 : 0);
    }
  }
  void* d_desc = nullptr; void* d_out = nullptr;
  const size_t out_bytes = (size_t)n * dim * dim * sizeof(double);
  RSBA_HIP_TRY(dev_malloc(&d_desc, desc.size() * sizeof(int32_t)));
  hipError_t e = dev_malloc(&d_out, out_bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
  CovStopwatch watch;
  if (e == hipSuccess) e = watch.start(st);
  if (e == hipSuccess) e = launch_cov_gather(s->cov.sigma, static_cast<const int32_t*>(d_desc), n, dim, static_cast<double*>(d_out), st);
  if (e == hipSuccess) e = watch.stop(st);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);   // (also before the blocks go back to the cache)
  if (e == hipSuccess && e2 == hipSuccess) watch.read(&s->cov.ms[4]);
  dev_free(d_desc); if (d_out) dev_free(d_out);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return rsba_set_error(e == hipErrorOutOfMemory ? RSBA_ERR_OUT_OF_MEMORY : RSBA_ERR_HIP, hipGetErrorString(e));
  return RSBA_OK;
}
}  // namespace

extern "C" int32_t rsba_covariance_compute(rsba_handle* h) {
  if (!h) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null handle");
  if (h->allreduce) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "rsba_covariance_compute does not take a handle with an exchange attached (one rank only)");
  RSBA_HIP_TRY(hipSetDevice(h->device));
  int32_t rc = build_solver(h);
  if (rc) return rc;
  Solver* s = h->solver; SolverDev& sv = s->sv; hipStream_t st = h->stream; const int CD = sv.CD;
  s->cov.valid = false;
  if (!s->cov.ready) {
    int bi = -1, bk = -1;
    if (!selinv_plan(s->hp, &s->cov.sel, &bi, &bk))
      return rsba_set_error(RSBA_ERR_UNSUPPORTED, ("selected inverse: tile (" + std::to_string(bi) + ", " + std::to_string(bk) + ") of the factor's fill pattern has no slot").c_str());
    SelinvPlan& d = s->cov.sel_dev;
    if ((rc = s_upload_const(s, &d.g_info, s->cov.sel.g_info)) || (rc = s_upload_const(s, &d.off_info, s->cov.sel.off_info)) || (rc = s_upload_const(s, &d.off_ptr, s->cov.sel.off_ptr)) ||
        (rc = s_upload_const(s, &d.off_list, s->cov.sel.off_list)) || (rc = s_upload_const(s, &d.diag_info, s->cov.sel.diag_info)) || (rc = s_upload_const(s, &d.diag_ptr, s->cov.sel.diag_ptr)) ||
        (rc = s_upload_const(s, &d.diag_list, s->cov.sel.diag_list))) return rc;
    // every tile pair of Sigma by unpermuted tile indices: the point blocks look entries up by camera-side coordinates
    std::vector<int32_t> tmap((size_t)sv.nt * sv.nt, -1);
    for (int a = 0; a < sv.nt; ++a) for (int b = 0; b < sv.nt; ++b) {
      const int pi = s->hp.iperm[a], pj = s->hp.iperm[b];
      const int32_t slot = pi >= pj ? s->hp.slot_of(pi, pj) : s->hp.slot_of(pj, pi);
      if (slot >= 0) tmap[(size_t)a * sv.nt + b] = 2 * slot + (pi < pj ? 1 : 0);
    }
    if ((rc = s_upload_const(s, &s->cov.tmap, tmap))) return rc;
    s->cov.plan_bytes = (int64_t)sizeof(int32_t) * (int64_t)(tmap.size() + s->cov.sel.g_info.size() + s->cov.sel.off_info.size() + s->cov.sel.off_ptr.size() + s->cov.sel.off_list.size() +
                                                               s->cov.sel.diag_info.size() + s->cov.sel.diag_ptr.size() + s->cov.sel.diag_list.size());
    if (sv.slot_xy) s->cov.slot_xy = sv.slot_xy;
    else {
      double2* sxy = nullptr;
      if ((rc = s_alloc(s, &sxy, (size_t)h->dp.N))) return rc;
      RSBA_HIP_TRY(launch_slot_xy(h->dp, sxy, st));
      s->cov.slot_xy = sxy;
      s->cov.plan_bytes += (int64_t)sizeof(double2) * h->dp.N;
    }
    s->cov.ready = true;
  }
  const size_t tile_bytes = (size_t)sv.nslots * kTile * kTile * sizeof(double);
  for (double** p : {&s->cov.sigma, &s->cov.g}) if (!*p) { void* q = nullptr; RSBA_HIP_TRY(dev_malloc(&q, tile_bytes)); *p = static_cast<double*>(q); }
  for (double** p : {&s->cov.live, &s->cov.vdev}) if (!*p) { void* q = nullptr; RSBA_HIP_TRY(dev_malloc(&q, (size_t)sv.npad * sizeof(double))); *p = static_cast<double*>(q); }
  // the undamped, unscaled reduced system and its factor: as rsba_pose_covariance
  if ((rc = reset_scales(h))) return rc;
  if ((rc = linearize(h))) return rc;
  RSBA_HIP_TRY(launch_clamp_diagonal(h->dp, sv, 1e-6, 1e32, st));
  RSBA_HIP_TRY(launch_pose_prior_clamp(h->dp, s->pp, 1e-6, 1e32, st));
  RSBA_HIP_TRY(hipMemsetAsync(sv.chol_fail, 0, sizeof(int), st));
  if ((rc = reduce_system(h, 1e300))) return rc;
  if (s->hp.two_rhs) RSBA_HIP_TRY(launch_ratio_prepare(s->ratio4, 1.0, 0.0, 0.0, st));
  // the factorisation rides on one solve (the right-hand side reduce_system left: its result is only what the persistent driver's
  // verification looks at), the border column of a free interFrameRatio on a second; a suspect result is redone on the level schedule
  double hb[3] = {0.0, 0.0, 0.0};
  int fail = 0, nfail = 0;
  s->cov.v.clear();
  {
  struct LevelsGuard { Solver* s; bool was; ~LevelsGuard() { s->use_levels = was; } } levels_guard{s, s->use_levels};   // (whichever way the attempts end)
  for (int attempt = 0; attempt < 2; ++attempt) {
    RSBA_HIP_TRY(hipMemsetAsync(sv.scalars + kDagSuspect, 0, sizeof(double), st));
    if ((rc = solve_reduced_system(h))) return rc;
    if (s->border) {
      const double* v = nullptr;
      if ((rc = solve_again(h, s->border, &v))) return rc;
      RSBA_HIP_TRY(launch_border_dots(s->border, v, v, sv.npad, s->ratio4 + 2, st));
      s->cov.v.resize((size_t)sv.npad);
      RSBA_HIP_TRY(hipMemcpyAsync(s->cov.v.data(), v, (size_t)sv.npad * sizeof(double), hipMemcpyDeviceToHost, st));
      RSBA_HIP_TRY(hipMemcpyAsync(s->cov.vdev, v, (size_t)sv.npad * sizeof(double), hipMemcpyDeviceToDevice, st));
      RSBA_HIP_TRY(hipMemcpyAsync(hb, s->ratio4, sizeof hb, hipMemcpyDeviceToHost, st));     // {h, g, b.v}
    }
    double suspect = 0.0;
    if ((rc = await_verification(h))) return rc;
    // (the two failure flags and diag(U) ride on the synchronisation the verification needs anyway)
    s->cov.ud.resize((size_t)h->dp.F * CD);
    RSBA_HIP_TRY(hipMemcpyAsync(&suspect, sv.scalars + kDagSuspect, sizeof(double), hipMemcpyDeviceToHost, st));
    RSBA_HIP_TRY(hipMemcpyAsync(&fail, sv.chol_fail, sizeof(int), hipMemcpyDeviceToHost, st));
    RSBA_HIP_TRY(hipMemcpyAsync(&nfail, h->dp.fail_count, sizeof(int), hipMemcpyDeviceToHost, st));
    RSBA_HIP_TRY(hipMemcpyAsync(s->cov.ud.data(), sv.udiag, s->cov.ud.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    RSBA_HIP_TRY(hipStreamSynchronize(st));
    if (suspect == 0.0 || s->use_levels) break;
    s->use_levels = true; ++s->dag_fallbacks;
  }
  }
  // a failed evaluation or a rank-deficient factor: nothing to invert, no launch
  if (nfail) return rsba_set_error(RSBA_ERR_EVALUATION_FAILED, "residual and Jacobian evaluation failed");
  if (fail) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "J^T J is rank deficient (fix the gauge): no covariance, as ceres::Covariance::Compute returns false");
  // Sigma on the factor's pattern: every G tile at once (they only read the factor), then level after level, descending, OFF before DIAG
  const SelinvHostPlan& sp = s->cov.sel;
  // (RSBA_COV_TIMES=1: an event between the launches, rsba_covariance_times splits the compute by kind; otherwise no event at all)
  struct Marks {
    bool on = cov_times_on(); std::vector<hipEvent_t> ev; std::vector<int> kind;
    ~Marks() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    hipError_t mark(int k, hipStream_t st) { if (!on) return hipSuccess; hipEvent_t e; hipError_t rc = hipEventCreate(&e); if (rc != hipSuccess) return rc; ev.push_back(e); kind.push_back(k); return hipEventRecord(e, st); }
  } marks;
  RSBA_HIP_TRY(launch_cov_live(sv, h->d_mask_pose, s->cov.live, st));
  RSBA_HIP_TRY(marks.mark(0, st));
  RSBA_HIP_TRY(launch_selinv_g(sv, s->cov.sel_dev, s->cov.live, s->cov.g, 0, (int)(sp.g_info.size() / 2), st));
  for (int p = 0; p < sp.nlev; ++p) {
    RSBA_HIP_TRY(marks.mark(1, st));
    RSBA_HIP_TRY(launch_selinv_off(s->cov.sel_dev, s->cov.sigma, s->cov.g, sp.lev_off_ptr[p], sp.lev_off_ptr[p + 1] - sp.lev_off_ptr[p], st));
    RSBA_HIP_TRY(marks.mark(2, st));
    RSBA_HIP_TRY(launch_selinv_diag(sv, s->cov.sel_dev, s->cov.live, s->cov.sigma, s->cov.g, sp.lev_diag_ptr[p], sp.lev_diag_ptr[p + 1] - sp.lev_diag_ptr[p], st));
  }
  RSBA_HIP_TRY(marks.mark(-1, st));
  RSBA_HIP_TRY(hipStreamSynchronize(st));
  s->cov.ms[0] = s->cov.ms[1] = s->cov.ms[2] = 0.0;
  for (size_t k = 0; k + 1 < marks.ev.size(); ++k) { float ms = 0.f; RSBA_HIP_TRY(hipEventElapsedTime(&ms, marks.ev[k], marks.ev[k + 1])); s->cov.ms[marks.kind[k]] += ms; }
  s->cov.border_scale = 0.0;
  if (s->border) {
    const double schur = hb[0] - hb[2];
    if (!(schur > 0.0) || !std::isfinite(schur)) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "J^T J is rank deficient in the interFrameRatio: no covariance");
    s->cov.border_scale = 1.0 / schur;
  }
  s->cov.valid = true;
  return RSBA_OK;
}

extern "C" int32_t rsba_covariance_frame_blocks(rsba_handle* h, const int32_t* frame_a, const int32_t* frame_b, int64_t n, double* cov) {
  if (int32_t rc = covariance_ready(h)) return rc;
  if (n < 0 || (n > 0 && (!frame_a || !frame_b || !cov))) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad covariance block arguments");
  RSBA_HIP_TRY(hipSetDevice(h->device));
  Solver* s = h->solver; const int CD = s->sv.CD, F = h->dp.F;
  std::vector<int64_t> row0((size_t)n), col0((size_t)n);
  for (int64_t p = 0; p < n; ++p) {
    if (frame_a[p] < 0 || frame_a[p] >= F || frame_b[p] < 0 || frame_b[p] >= F) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "frame out of range");
    row0[p] = (int64_t)frame_a[p] * CD; col0[p] = (int64_t)frame_b[p] * CD;
  }
  int64_t missing = -1;
  if (int32_t rc = covariance_gather(h, row0, col0, CD, cov, &missing)) return rc;
  if (missing >= 0)
    return rsba_set_error(RSBA_ERR_UNSUPPORTED, ("frames " + std::to_string(frame_a[missing]) + " and " + std::to_string(frame_b[missing]) +
                                                 " share no tile of the factor's pattern: their covariance block is not part of the selected inverse").c_str());
  const bool border = !s->cov.v.empty();
  for (int64_t p = 0; p < n; ++p) {
    const size_t ra = (size_t)frame_a[p] * CD, rb = (size_t)frame_b[p] * CD;
    double* c = cov + (size_t)p * CD * CD;
    for (int a = 0; a < CD; ++a) for (int b = 0; b < CD; ++b) {
      // (fixed coordinates and coordinates no residual touches are no parameters of the program: exact zeros, as rsba_pose_covariance)
      const bool live = s->cov.ud[ra + a] != 0.0 && h->mask_pose[ra + a] != 0.0 && s->cov.ud[rb + b] != 0.0 && h->mask_pose[rb + b] != 0.0;
      c[a * CD + b] = live ? c[a * CD + b] + (border ? s->cov.v[ra + a] * s->cov.v[rb + b] * s->cov.border_scale : 0.0) : 0.0;
    }
  }
  return RSBA_OK;
}

extern "C" int32_t rsba_covariance_intrinsics_block(rsba_handle* h, int32_t block, double* cov) {
  if (int32_t rc = covariance_ready(h)) return rc;
  Solver* s = h->solver; const SolverDev& sv = s->sv;
  if (!cov) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (block < 0 || block >= sv.NIB) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, sv.NIB ? "intrinsics block out of range" : "the problem has no intrinsics parameter blocks (calibrated)");
  RSBA_HIP_TRY(hipSetDevice(h->device));
  // the 9 coordinates of block c sit at the front of its pseudo frames, behind the real frames
  const int64_t r0 = ((int64_t)sv.F + (int64_t)block * sv.NPF) * sv.CD;
  int64_t missing = -1;
  if (int32_t rc = covariance_gather(h, {r0}, {r0}, 9, cov, &missing)) return rc;
  if (missing >= 0) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "the intrinsics block crosses a tile edge whose off-diagonal tile the factor's pattern does not have");
  const bool border = !s->cov.v.empty();
  for (int a = 0; a < 9; ++a) for (int b = 0; b < 9; ++b) {
    const bool live = h->mask_intr[(size_t)block * 9 + a] != 0.0 && h->mask_intr[(size_t)block * 9 + b] != 0.0;
    cov[a * 9 + b] = live ? cov[a * 9 + b] + (border ? s->cov.v[(size_t)r0 + a] * s->cov.v[(size_t)r0 + b] * s->cov.border_scale : 0.0) : 0.0;
  }
  return RSBA_OK;
}

// The 3 x 3 block of every asked point (kernels_selinv.hip: cov_point_kernel).  A constant point and a point nobody sees are no unknowns:
// exact zeros.
extern "C" int32_t rsba_covariance_point_blocks(rsba_handle* h, const int32_t* points, int64_t n, double* cov) {
  if (int32_t rc = covariance_ready(h)) return rc;
  const int64_t M = h->dp.M;
  if (n < 0 || (n > 0 && !cov) || (!points && n > M)) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad covariance block arguments");
  if (points) for (int64_t p = 0; p < n; ++p) if (points[p] < 0 || points[p] >= M) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "point out of range");
  if (n == 0) return RSBA_OK;
  RSBA_HIP_TRY(hipSetDevice(h->device));
  Solver* s = h->solver; hipStream_t st = h->stream;
  void *d_pts = nullptr, *d_out = nullptr, *d_miss = nullptr;
  const size_t out_bytes = (size_t)n * 9 * sizeof(double);
  int missing = 0;
  hipError_t e = dev_malloc(&d_out, out_bytes);
  if (e == hipSuccess) e = dev_malloc(&d_miss, sizeof(int));
  if (e == hipSuccess && points) e = dev_malloc(&d_pts, (size_t)n * sizeof(int32_t));
  if (e == hipSuccess && points) e = hipMemcpyAsync(d_pts, points, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_miss, 0, sizeof(int), st);
  CovStopwatch watch;
  if (e == hipSuccess) e = watch.start(st);
  if (e == hipSuccess) e = launch_cov_points(h->dp, s->sv, s->cov.sigma, s->cov.tmap, s->cov.v.empty() ? nullptr : s->cov.vdev, s->cov.border_scale, static_cast<const int32_t*>(d_pts), n,
                                             s->cov.slot_xy, static_cast<double*>(d_out), static_cast<int*>(d_miss), st);
  if (e == hipSuccess) e = watch.stop(st);
  if (e == hipSuccess) e = hipMemcpyAsync(cov, d_out, out_bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&missing, d_miss, sizeof(int), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);   // (also before the blocks go back to the cache)
  if (e == hipSuccess && e2 == hipSuccess) watch.read(&s->cov.ms[3]);
  for (void* p : {d_pts, d_out, d_miss}) if (p) dev_free(p);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return rsba_set_error(e == hipErrorOutOfMemory ? RSBA_ERR_OUT_OF_MEMORY : RSBA_ERR_HIP, hipGetErrorString(e));
  if (missing) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "two frames of one point share no tile of the factor's pattern: the plan of the reduced system does not cover the point's pairs");
  for (int64_t p = 0; p < n; ++p) {
    const int64_t j = points ? points[p] : p;
    if (h->mask_point[(size_t)j * 3] == 0.0) for (int k = 0; k < 9; ++k) cov[(size_t)p * 9 + k] = 0.0;
  }
  return RSBA_OK;
}

// Device memory the covariance holds on this handle right now: the tile arrays and vectors of a computed covariance (gone after
// rsba_covariance_release) plus the lists the first compute uploaded (with the plan).
extern "C" int32_t rsba_covariance_memory(rsba_handle* h, int64_t* bytes) {
  if (!h || !bytes) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  *bytes = 0;
  if (!h->solver) return RSBA_OK;
  const Solver* s = h->solver;
  *bytes = s->cov.plan_bytes;
  if (s->cov.sigma) *bytes += 2 * (int64_t)s->sv.nslots * kTile * kTile * (int64_t)sizeof(double);
  if (s->cov.live) *bytes += 2 * (int64_t)s->sv.npad * (int64_t)sizeof(double);
  return RSBA_OK;
}

// HIP-event times of the covariance kernels, ms: {G, OFF, DIAG launches of the last compute, the last point getter's kernel, the last gather's};
// taken only in a process started with RSBA_COV_TIMES=1 (zeros otherwise: the calls create no events then)
extern "C" int32_t rsba_covariance_times(rsba_handle* h, double* ms5) {
  if (!h || !ms5) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  for (int k = 0; k < 5; ++k) ms5[k] = h->solver ? h->solver->cov.ms[k] : 0.0;
  return RSBA_OK;
}

extern "C" int32_t rsba_covariance_release(rsba_handle* h) {
  if (!h) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null handle");
  if (!h->solver) return RSBA_OK;
  Solver* s = h->solver;
  s->cov.valid = false;
  if (s->cov.sigma || s->cov.g || s->cov.live || s->cov.vdev) {
    RSBA_HIP_TRY(hipSetDevice(h->device));
    RSBA_HIP_TRY(hipStreamSynchronize(h->stream));   // nothing on the device touches the tiles any more: they go back to the cache (devmem.hpp)
    for (double** p : {&s->cov.sigma, &s->cov.g, &s->cov.live, &s->cov.vdev}) if (*p) { dev_free(*p); *p = nullptr; }
  }
  s->cov.v.clear(); s->cov.v.shrink_to_fit(); s->cov.ud.clear(); s->cov.ud.shrink_to_fit();
  return RSBA_OK;
}
