// K9 of SURVEY §2.1: the scalar reductions of the trust-region loop, the candidate, the trust-region control on the device and the
// pack / unpack kernels of the linearisation.
#include "pass_common.hpp"

namespace rsba {

namespace {

__global__ __launch_bounds__(256) void reduce_sum_kernel(const double* partial, int n, double* out, double sign) {
  __shared__ double s_red[4];
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += 256) v += partial[k];
  v = wsum(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *out = sign * (s_red[0] + s_red[1] + s_red[2] + s_red[3]);
}

// two sums in one launch: workgroup b reduces partial[b * n .. b * n + n) into out0 (b = 0) resp. out1 (b = 1), same order as reduce_sum_kernel
__global__ __launch_bounds__(256) void reduce_sum2_kernel(const double* partial, int n, double* out0, double* out1) {
  __shared__ double s_red[4];
  const double* src = partial + (size_t)blockIdx.x * n;
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += 256) v += src[k];
  v = wsum(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *(blockIdx.x == 0 ? out0 : out1) = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// reduce_sum_kernel(pa, na, outa, -1) and reduce_sum2_kernel(pb, nb, out0, out1) by one launch of three workgroups
__global__ __launch_bounds__(256) void reduce_sum3_kernel(const double* pa, int na, double* outa, const double* pb, int nb, double* out0, double* out1) {
  __shared__ double s_red[4];
  const double* src = blockIdx.x == 0 ? pa : pb + (size_t)(blockIdx.x - 1) * nb;
  const int n = blockIdx.x == 0 ? na : nb;
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += 256) v += src[k];
  v = wsum(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sum = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  if (blockIdx.x == 0) *outa = -1.0 * sum; else *(blockIdx.x == 1 ? out0 : out1) = sum;
}

// x_plus_delta = x + scale .* step; |x - x_plus_delta|^2 and |x|^2 over the reduced program's blocks
__global__ __launch_bounds__(256) void candidate_kernel(const DeviceProblem dp, const SolverDev sv, double* __restrict__ part) {
  __shared__ double s_red[2][4];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nc = sv.n, np = 3 * (int64_t)dp.M;
  double st = 0.0, xx = 0.0;
  if (t < nc + np) {
    const bool cam = t < nc;
    const int64_t npose = (int64_t)sv.F * sv.CD;
    const bool intr = cam && t >= npose;
    const int64_t u = cam ? (intr ? t - npose : t) : t - nc;
    const int ii = intr ? intr_index(sv, u) : 0;     // coordinate of its intrinsics block, -1 = padding of a pseudo frame
    if (intr && ii < 0) { st = 0.0; xx = 0.0; }
    else {
    const double x = cam ? (intr ? dp.intr[ii] : dp.poses[u]) : dp.points[u];
    const double sc = cam ? cam_scale(dp, sv, t) : dp.scale_point[u];
    const double y = cam ? sv.step[t] : sv.yp[u];
    const double in = cam ? (intr ? sv.inprog_intr[u] : sv.inprog_pose[u]) : sv.inprog_point[u];
    const double xn = (sc > 0.0) ? x + (-y * sc) : x;
    if (intr) sv.trial_intr[ii] = xn; else if (cam) sv.trial_poses[u] = xn; else sv.trial_points[u] = xn;
    if (in > 0.0) { const double e = x - xn; st = e * e; xx = x * x; }
    }
  }
  st = wsum(st); xx = wsum(xx);
  if ((threadIdx.x & 63) == 0) { s_red[0][threadIdx.x >> 6] = st; s_red[1][threadIdx.x >> 6] = xx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
    part[gridDim.x + blockIdx.x] = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
  }
}

// sharded solve, after the last iteration: every rank contributes the points it owns (the ones it has observations of),
// buf = [M][3] values | [M] owner count; after the all-reduce the owners' values replace the local copies
__global__ void own_points_kernel(const DeviceProblem dp, const SolverDev sv, double* buf) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= dp.M) return;
  const bool own = sv.point_ptr[j + 1] > sv.point_ptr[j];
  for (int k = 0; k < 3; ++k) buf[3 * j + k] = own ? dp.points[3 * j + k] : 0.0;
  buf[3 * (int64_t)dp.M + j] = own ? 1.0 : 0.0;
}
__global__ void merge_points_kernel(const DeviceProblem dp, const double* buf) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= dp.M || buf[3 * (int64_t)dp.M + j] != 1.0) return;
  for (int k = 0; k < 3; ++k) dp.points[3 * j + k] = buf[3 * j + k];
}

// exchange buffer (1): g_c | diag(U) | cost, fixed cost, failed blocks
// ---- trust-region control on the device ----
// Ceres 1.9's TrustRegionMinimizer loop body behind the linear solve, the same rules in the same
// order as the host form in solver.hip (rsba_solve) — one thread; every operation is an IEEE add / multiply / divide / sqrt /
// compare, so the two forms take bit-identical decisions.  Scalars of the iteration: sv.scalars (ScalarSlot), state: ctl (LmCtlSlot).
__device__ __forceinline__ void lm_push(double* ctl, rsba_iteration* trace, int cap, const rsba_iteration& it) {
  const int n = (int)ctl[kCtlNumTrace];
  if (trace && n < cap) trace[n] = it;
  ctl[kCtlNumTrace] = (double)(n + 1);
}
__device__ __forceinline__ void lm_decide_step(const SolverDev& sv, double* ctl, const LmRules& R, rsba_iteration* trace, int cap) {
#pragma clang fp contract(off)   // every product and sum rounded on its own, as the host form's are (1 - (t t) t would become an fma: one ulp of the radius)
  if (ctl[kCtlStatus] != 0.0) return;
  ctl[kCtlAccept] = 0.0;
  const double* sc = sv.scalars;
  if (sc[kDagSuspect] != 0.0) { ctl[kCtlStatus] = -1.0; return; }   // nothing of this iteration has touched x: the host repeats it on the level schedule
  double radius = ctl[kCtlRadius], decrease = ctl[kCtlDecrease];
  const double cost = ctl[kCtlCost], fixed = ctl[kCtlFixed], gmax = ctl[kCtlGmax];
  const int iteration = (int)ctl[kCtlIteration] + 1;
  ctl[kCtlIteration] = (double)iteration;
  rsba_iteration it;
  it.iteration = iteration; it.step_is_valid = 0; it.step_is_successful = 0; it.reserved = 0;
  it.cost = 0.0; it.cost_change = 0.0; it.gradient_max_norm = 0.0; it.step_norm = 0.0; it.relative_decrease = 0.0; it.trust_region_radius = 0.0; it.model_cost_change = 0.0;
  const double model_cost_change = sc[kModelCostChange];
  const bool cfail = sc[kSolveFailed] != 0.0, nfail = sc[kEvalFailed] != 0.0;
  double step_sq = sc[kStepSq], x_sq = sc[kXSq];
  if (sv.rt) {   // a free interFrameRatio is one more coordinate of x (its candidate: ratio_candidate_kernel)
    const double ratio = sv.rt[kRtRatio], rn = sv.rt[kRtRatioNew];
    step_sq += (ratio - rn) * (ratio - rn); x_sq += ratio * ratio;
  }
  const bool solved = !cfail && isfinite(model_cost_change) && isfinite(step_sq);
  const bool valid = solved && model_cost_change >= 0.0;
  it.model_cost_change = solved ? model_cost_change : 0.0;
  auto done = [&](int term) { it.cost = cost + fixed; it.trust_region_radius = radius; lm_push(ctl, trace, cap, it); ctl[kCtlStatus] = 1.0 + term; };
  if (!valid) {
    const int streak = (int)ctl[kCtlInvalidStreak] + 1;
    ctl[kCtlInvalidStreak] = (double)streak;
    if (streak >= R.max_num_consecutive_invalid_steps) { done(RSBA_FAILURE); return; }
    radius /= decrease; decrease *= 2.0;
    ctl[kCtlUnsuccessful] += 1.0;
    it.gradient_max_norm = gmax;
  } else {
    ctl[kCtlInvalidStreak] = 0.0; it.step_is_valid = 1;
    const double new_cost = nfail ? 1.7976931348623157e308 : (sc[kCost] + 0.0) - fixed;   // (the trial evaluation reports the total in kCost)
    it.step_norm = sqrt(step_sq);
    const double x_norm = sqrt(x_sq);
    if (it.step_norm <= R.parameter_tolerance * (x_norm + R.parameter_tolerance)) { done(RSBA_CONVERGENCE); return; }
    it.cost_change = cost - new_cost;
    if (fabs(it.cost_change) < R.function_tolerance * cost) { done(RSBA_CONVERGENCE); return; }
    it.relative_decrease = it.cost_change / model_cost_change;
    if (it.relative_decrease > R.min_relative_decrease) {
      it.step_is_successful = 1; ctl[kCtlSuccessful] += 1.0;
      const double t = 2.0 * it.relative_decrease - 1.0;
      radius = radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
      radius = fmin(R.max_trust_region_radius, radius); decrease = 2.0;
      ctl[kCtlRadius] = radius; ctl[kCtlDecrease] = decrease; ctl[kCtlAccept] = 1.0;
      ctl[kCtlRecSel] = 1.0 - ctl[kCtlRecSel];   // (problems that keep records: the candidate's are the current point's from here on — device_state.hpp: lm_records)
      if (sv.rt) sv.rt[kRtRatio] = sv.rt[kRtRatioNew];
      // (the iteration's record is finished by lm_decide_gradient_kernel once the accepted point is linearised)
      ctl[kCtlPending] = it.relative_decrease; ctl[kCtlPending + 1] = it.cost_change; ctl[kCtlPending + 2] = it.step_norm; ctl[kCtlPending + 3] = it.model_cost_change;
      return;
    }
    ctl[kCtlUnsuccessful] += 1.0; it.gradient_max_norm = gmax;
    radius /= decrease; decrease *= 2.0;
  }
  ctl[kCtlRadius] = radius; ctl[kCtlDecrease] = decrease;
  it.cost = cost + fixed; it.trust_region_radius = radius;
  lm_push(ctl, trace, cap, it);
  if (radius < R.min_trust_region_radius) ctl[kCtlStatus] = 1.0 + RSBA_CONVERGENCE;
  else if (iteration >= R.max_num_iterations) ctl[kCtlStatus] = 1.0 + RSBA_NO_CONVERGENCE;
}
__global__ void lm_decide_step_kernel(const SolverDev sv, double* ctl, const LmRules R, rsba_iteration* trace, int cap) { lm_decide_step(sv, ctl, R, trace, cap); }
// after the linearisation of an accepted step: its cost, the gradient test, the iteration's record
__device__ __forceinline__ void lm_decide_gradient(const SolverDev& sv, double* ctl, const LmRules& R, rsba_iteration* trace, int cap) {
#pragma clang fp contract(off)
  if (ctl[kCtlStatus] != 0.0 || ctl[kCtlAccept] == 0.0) return;
  const double* sc = sv.scalars;
  rsba_iteration it;
  it.iteration = (int)ctl[kCtlIteration]; it.step_is_valid = 1; it.step_is_successful = 1; it.reserved = 0;
  it.relative_decrease = ctl[kCtlPending]; it.cost_change = ctl[kCtlPending + 1]; it.step_norm = ctl[kCtlPending + 2]; it.model_cost_change = ctl[kCtlPending + 3];
  const double fixed = ctl[kCtlFixed], radius = ctl[kCtlRadius];
  if (sc[kEvalFailed] != 0.0) {   // the evaluation at the accepted point failed: the host reports it (RSBA_ERR_EVALUATION_FAILED)
    it.cost = 0.0; it.gradient_max_norm = 0.0; it.trust_region_radius = 0.0;
    lm_push(ctl, trace, cap, it);
    ctl[kCtlStatus] = -2.0;
    return;
  }
  double gmax = sc[kGradMax];
  if (sv.rt) { const double ratio = sv.rt[kRtRatio]; gmax = fmax(gmax, fabs(ratio - fmax(sv.rt[kRtLb], ratio - sv.rt[kRtG]))); }   // the ratio's projected gradient (its block is bounded below)
  const double cost = sc[kCost];
  ctl[kCtlCost] = cost; ctl[kCtlGmax] = gmax;
  ctl[kCtlFinalCost] = fmin(ctl[kCtlFinalCost], cost + fixed);
  it.gradient_max_norm = gmax; it.cost = cost + fixed; it.trust_region_radius = radius;
  lm_push(ctl, trace, cap, it);
  if (gmax <= R.gradient_tolerance) ctl[kCtlStatus] = 1.0 + RSBA_CONVERGENCE;
  else if (radius < R.min_trust_region_radius) ctl[kCtlStatus] = 1.0 + RSBA_CONVERGENCE;
  else if (it.iteration >= R.max_num_iterations) ctl[kCtlStatus] = 1.0 + RSBA_NO_CONVERGENCE;
}
__global__ void lm_decide_gradient_kernel(const SolverDev sv, double* ctl, const LmRules R, rsba_iteration* trace, int cap) { lm_decide_gradient(sv, ctl, R, trace, cap); }

// ---- the same steps in fewer launches (the loop that never waits for the host pays ~4 us per launch of a dependent chain; at 100
// cameras that was a seventh of the iteration: profiles/r04/iteration_gaps.txt).  Same arithmetic in the same order as the kernels
// they stand for: the two forms of the trust-region loop still take bit-identical decisions. ----
// reduce_cost_kernel (kernels_eval.hip) + pack_trial_kernel + lm_decide_step_kernel
// (n < 0: the cost was reduced already — and the motion priors' added to it — by kernels of their own)
__global__ __launch_bounds__(256) void lm_verdict_step_kernel(const DeviceProblem dp, const SolverDev sv, double* cost2, int n, double* ctl, const LmRules R, rsba_iteration* trace, int cap) {
  if (ctl[kCtlStatus] != 0.0) return;
  if (n < 0) {
    if (threadIdx.x == 0) {
      sv.scalars[kCost] = cost2[0] + cost2[1]; sv.scalars[kFixedCost] = 0.0; sv.scalars[kEvalFailed] = (double)*dp.fail_count; sv.scalars[kSolveFailed] = (double)*sv.chol_fail;
      lm_decide_step(sv, ctl, R, trace, cap);
    }
    return;
  }
  __shared__ double s_red[3][4];
  double c = 0.0, f = 0.0, nf = 0.0;
  int k = threadIdx.x;
  for (; k + 15 * 256 < n; k += 16 * 256) {   // (as reduce_cost_kernel: sixteen strides' loads together, added in stride order)
    double vc[16], vf[16], vn[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) { vc[u] = dp.cost_partial[k + 256 * u]; vf[u] = dp.fixed_partial[k + 256 * u]; vn[u] = dp.fail_partial[k + 256 * u]; }
#pragma unroll
    for (int u = 0; u < 16; ++u) { c += vc[u]; f += vf[u]; nf += vn[u]; }
  }
  for (; k < n; k += 256) { c += dp.cost_partial[k]; f += dp.fixed_partial[k]; nf += dp.fail_partial[k]; }
  c = wsum(c); f = wsum(f); nf = wsum(nf);
  if ((threadIdx.x & 63) == 0) { s_red[0][threadIdx.x >> 6] = c; s_red[1][threadIdx.x >> 6] = f; s_red[2][threadIdx.x >> 6] = nf; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double cost = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3], fixed = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
  const int fails = (int)(s_red[2][0] + s_red[2][1] + s_red[2][2] + s_red[2][3]);
  cost2[0] = cost; cost2[1] = fixed; *dp.fail_count = fails;
  sv.scalars[kCost] = cost + fixed; sv.scalars[kFixedCost] = 0.0; sv.scalars[kEvalFailed] = (double)fails; sv.scalars[kSolveFailed] = (double)*sv.chol_fail;
  lm_decide_step(sv, ctl, R, trace, cap);
}
// local_linearize_kernel + gradient_max_kernel
__global__ __launch_bounds__(256) void lm_linearize_gradient_kernel(const DeviceProblem dp, const SolverDev sv, const double* cost2) {
  __shared__ double s_red[4];
  const int64_t nc = sv.n, np = 3 * (int64_t)dp.M;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (!lm_not_accepted(sv.ctl)) {
    if (t < nc) sv.udiag[t] = u_diag(sv, t);
    if (t == 0) { sv.scalars[kCost] = cost2[0]; sv.scalars[kFixedCost] = cost2[1]; sv.scalars[kEvalFailed] = (double)*dp.fail_count; }
  }
  double m = 0.0;
  if (t < nc + np) {
    const double sc = (t < nc) ? cam_scale(dp, sv, t) : dp.scale_point[t - nc];
    const double g = (t < nc) ? sv.gc[t] : sv.gp[t - nc];
    if (sc > 0.0) m = fabs(g / sc);
  }
  m = wmax(m);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) sv.partial[blockIdx.x] = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
}
// reduce_max_kernel + lm_decide_gradient_kernel; the state after the iteration goes to the host's slot for it
__global__ __launch_bounds__(256) void lm_verdict_gradient_kernel(const SolverDev sv, int n, double* ctl, const LmRules R, rsba_iteration* trace, int cap, double* snapshot, double seq) {
  __shared__ double s_red[4];
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += 256) v = fmax(v, sv.partial[k]);
  v = wmax(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    if (n >= 0) sv.scalars[kGradMax] = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));   // (n < 0: several ranks — the maximum came with the camera exchange)
    lm_decide_gradient(sv, ctl, R, trace, cap);
    *sv.chol_fail = 0; sv.scalars[kDagSuspect] = 0.0;   // begin_solve_kernel's job for the NEXT iteration: both flags were read by this iteration's first verdict
  }
  __syncthreads();
  // the state to the host's slot: a word per lane (stores to host memory one after the other cost a bus round trip each), the stamp behind them
  if (threadIdx.x < kCtlSeq) __hip_atomic_store(snapshot + threadIdx.x, ctl[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(snapshot + kCtlSeq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // the host polls this word: everything above is there when it shows
}

// x = x + delta: the candidate the last decision accepted becomes the current point (the host form swaps the two buffers)
__global__ void lm_take_candidate_kernel(const DeviceProblem dp, const SolverDev sv, int64_t npose, int64_t npoint, int64_t nintr) {
  if (lm_not_accepted(sv.ctl)) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < npose) dp.poses[t] = sv.trial_poses[t];
  else if (t < npose + npoint) dp.points[t - npose] = sv.trial_points[t - npose];
  else if (t < npose + npoint + nintr) dp.intr[t - npose - npoint] = sv.trial_intr[t - npose - npoint];
}

__global__ void pack_linearize_kernel(const DeviceProblem dp, const SolverDev sv, const double* cost2, int nslots) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < nslots) sv.xbuf[2 * sv.n + 3 + t] = 0.0;   // the ranks' gradient maxima (launch_gradient_max_points fills this rank's)
  if (t < sv.n) {
    sv.xbuf[t] = sv.gc[t];
    sv.xbuf[sv.n + t] = u_diag(sv, t);
  }
  if (t == 0) { sv.xbuf[2 * sv.n] = cost2[0]; sv.xbuf[2 * sv.n + 1] = cost2[1]; sv.xbuf[2 * sv.n + 2] = (double)*dp.fail_count; }
}
// without an exchange (one rank) the round trip through xbuf is one kernel: udiag = diag(U), the three scalars
__global__ void local_linearize_kernel(const DeviceProblem dp, const SolverDev sv, const double* cost2) {
  if (lm_not_accepted(sv.ctl)) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < sv.n) sv.udiag[t] = u_diag(sv, t);
  if (t == 0) { sv.scalars[kCost] = cost2[0]; sv.scalars[kFixedCost] = cost2[1]; sv.scalars[kEvalFailed] = (double)*dp.fail_count; }
}
__global__ void unpack_linearize_kernel(const DeviceProblem dp, const SolverDev sv) {
  if (lm_not_accepted(sv.ctl)) return;   // (device-side trust region on several ranks: the exchange of a rejected candidate's iteration carried nothing new)
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < sv.n) { sv.gc[t] = sv.xbuf[t]; sv.udiag[t] = sv.xbuf[sv.n + t]; }
  if (t == 0) { sv.scalars[kCost] = sv.xbuf[2 * sv.n]; sv.scalars[kFixedCost] = sv.xbuf[2 * sv.n + 1]; sv.scalars[kEvalFailed] = sv.xbuf[2 * sv.n + 2]; }
}
__global__ void pack_trial_kernel(const DeviceProblem dp, const SolverDev sv, const double* cost2) {
  sv.scalars[kCost] = cost2[0] + cost2[1];
  sv.scalars[kFixedCost] = 0.0;
  sv.scalars[kEvalFailed] = (double)*dp.fail_count;
  sv.scalars[kSolveFailed] = (double)*sv.chol_fail;
  if (!sv.lead) sv.scalars[kGradMax] = 0.0;   // several ranks: slots 0 - 11 travel in ONE sum; the maximum (the same on every rank) comes back as the lead rank's
}

}  // namespace

hipError_t launch_pack_linearize(const DeviceProblem& dp, const SolverDev& sv, const double* cost2, hipStream_t st, int nslots) {
  LAUNCH(pack_linearize_kernel, nblocks256(std::max<int64_t>(sv.n, nslots)), 256, st, dp, sv, cost2, nslots);
  return hipSuccess;
}
__global__ void begin_solve_kernel(const SolverDev sv) { *sv.chol_fail = 0; sv.scalars[kDagSuspect] = 0.0; }
hipError_t launch_begin_solve(const SolverDev& sv, hipStream_t st) {
  LAUNCH(begin_solve_kernel, 1, 1, st, sv);
  return hipSuccess;
}
hipError_t launch_local_linearize(const DeviceProblem& dp, const SolverDev& sv, const double* cost2, hipStream_t st) {
  LAUNCH(local_linearize_kernel, nblocks256(sv.n), 256, st, dp, sv, cost2);
  return hipSuccess;
}
hipError_t launch_unpack_linearize(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  LAUNCH(unpack_linearize_kernel, nblocks256(sv.n), 256, st, dp, sv);
  return hipSuccess;
}
hipError_t launch_pack_trial(const DeviceProblem& dp, const SolverDev& sv, const double* cost2, hipStream_t st) {
  LAUNCH(pack_trial_kernel, 1, 1, st, dp, sv, cost2);
  return hipSuccess;
}
// -> scalars[kModelCostChange]; must follow launch_back_substitute directly (it reduces that kernel's partials)
hipError_t launch_model_cost_change(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  LAUNCH(reduce_sum_kernel, 1, 256, st, sv.partial, dp.M > 0 ? point_step_blocks(dp, sv) : 0, sv.scalars + kModelCostChange, -1.0);
  return hipSuccess;
}
hipError_t launch_own_points(const DeviceProblem& dp, const SolverDev& sv, double* buf, hipStream_t st) {
  LAUNCH(own_points_kernel, nblocks256(dp.M), 256, st, dp, sv, buf);
  return hipSuccess;
}
hipError_t launch_merge_points(const DeviceProblem& dp, const double* buf, hipStream_t st) {
  LAUNCH(merge_points_kernel, nblocks256(dp.M), 256, st, dp, buf);
  return hipSuccess;
}
hipError_t launch_lm_verdict_step(const DeviceProblem& dp, const SolverDev& sv, double* cost2, double* ctl, const LmRules& rules, rsba_iteration* trace, int trace_cap, hipStream_t st, bool cost_reduced) {
  LAUNCH(lm_verdict_step_kernel, 1, 256, st, dp, sv, cost2, cost_reduced ? -1 : eval_num_blocks(dp.N), ctl, rules, trace, trace_cap);
  return hipSuccess;
}
hipError_t launch_lm_linearize_gradient(const DeviceProblem& dp, const SolverDev& sv, const double* cost2, hipStream_t st) {
  LAUNCH(lm_linearize_gradient_kernel, nblocks256(sv.n + 3 * (int64_t)dp.M), 256, st, dp, sv, cost2);
  return hipSuccess;
}
hipError_t launch_lm_verdict_gradient(const DeviceProblem& dp, const SolverDev& sv, double* ctl, const LmRules& rules, rsba_iteration* trace, int trace_cap, double* snapshot, double seq, hipStream_t st, bool gradmax_done, int extra_partials) {
  LAUNCH(lm_verdict_gradient_kernel, 1, 256, st, sv, gradmax_done ? -1 : nblocks256(sv.n + 3 * (int64_t)dp.M) + extra_partials, ctl, rules, trace, trace_cap, snapshot, seq);
  return hipSuccess;
}
hipError_t launch_lm_decide_step(const SolverDev& sv, double* ctl, const LmRules& rules, rsba_iteration* trace, int trace_cap, hipStream_t st) {
  LAUNCH(lm_decide_step_kernel, 1, 1, st, sv, ctl, rules, trace, trace_cap);
  return hipSuccess;
}
hipError_t launch_lm_decide_gradient(const SolverDev& sv, double* ctl, const LmRules& rules, rsba_iteration* trace, int trace_cap, hipStream_t st) {
  LAUNCH(lm_decide_gradient_kernel, 1, 1, st, sv, ctl, rules, trace, trace_cap);
  return hipSuccess;
}
hipError_t launch_lm_take_candidate(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  const int64_t npose = (int64_t)dp.F * dp.P * 6, npoint = 3 * (int64_t)dp.M, nintr = sv.NPF > 0 ? 9 * (int64_t)dp.NI : 0;
  LAUNCH(lm_take_candidate_kernel, (unsigned)((npose + npoint + nintr + 255) / 256), 256, st, dp, sv, npose, npoint, nintr);
  return hipSuccess;
}
hipError_t launch_candidate(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  const int nb = nblocks256(sv.n + 3 * (int64_t)dp.M);
  LAUNCH(candidate_kernel, nb, 256, st, dp, sv, sv.partial);
  LAUNCH(reduce_sum2_kernel, 2, 256, st, sv.partial, nb, sv.scalars + kStepSq, sv.scalars + kXSq);   // (one launch: workgroup 0 -> |step|^2, workgroup 1 -> |x|^2)
  return hipSuccess;
}
hipError_t launch_candidate_and_model_cost(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  const int nb = nblocks256(sv.n + 3 * (int64_t)dp.M);
  LAUNCH(candidate_kernel, nb, 256, st, dp, sv, sv.partial_c);   // (its sums beside the back-substitution's, which are still waiting in sv.partial)
  LAUNCH(reduce_sum3_kernel, 3, 256, st, sv.partial, dp.M > 0 ? point_step_blocks(dp, sv) : 0, sv.scalars + kModelCostChange, sv.partial_c, nb, sv.scalars + kStepSq, sv.scalars + kXSq);
  return hipSuccess;
}

}  // namespace rsba
