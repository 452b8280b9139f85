// Camera-side blocks of the normal equations (K2a of SURVEY §2.1), the Jacobi scales, the LM diagonal, the gradient's maximum and
// the point factors (K5a).  All fp64; all sums are taken in a fixed order (no floating-point atomics).
#include "camera_reduce.hpp"

namespace rsba {

namespace {

template <int CD, bool CAL>
__global__ __launch_bounds__(256) void camera_reduce_kernel(const DeviceProblem dp, const SolverDev sv) {
  if (lm_not_accepted(sv.ctl)) return;   // (device-side trust region: a rejected candidate is not linearised)
  if ((int)blockIdx.x >= dp.F) { take_candidate_block(dp, sv, (int64_t)blockIdx.x - dp.F); return; }   // workgroups behind the frames' (launch_camera_blocks with take_candidate) — this kernel reads no parameters
  camera_reduce_frame<CD, CAL>(dp, sv, (int)blockIdx.x);
}

// one workgroup per (intrinsics block c, entry t of the 45 + 9 sums): lanes stride the frames that use the block (in
// frame order), fixed-order wave / workgroup reduction
__global__ __launch_bounds__(256) void intr_reduce_kernel(const DeviceProblem dp, const SolverDev sv) {
  if (lm_not_accepted(sv.ctl)) return;
  __shared__ double s_red[4];
  const int c = blockIdx.x / 54, t = blockIdx.x % 54, tid = threadIdx.x;
  double v = 0.0;
  for (int q = sv.intr_frame_ptr[c] + tid; q < sv.intr_frame_ptr[c + 1]; q += 256) v += sv.intr_part[(size_t)sv.intr_frame_list[q] * 54 + t];
  v = wsum(v);
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  if (tid != 0) return;
  v = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  const int CD = sv.CD;
  if (t >= 45) { sv.gc[((size_t)sv.F + (size_t)c * sv.NPF) * CD + (t - 45)] = v; return; }
  int a = 0, rem = t;
  while (rem >= 9 - a) { rem -= 9 - a; ++a; }
  const int b = a + rem;
  sv.U[u_self_off(sv, c, a / CD, b / CD) + (size_t)(a % CD) * CD + (b % CD)] = v;
  sv.U[u_self_off(sv, c, b / CD, a / CD) + (size_t)(b % CD) * CD + (a % CD)] = v;
}

// Ceres 1.9 TrustRegionMinimizer: EstimateScale  scale_i = 1 / (1 + sqrt(|J_i|^2)), once, from the first
// Jacobian.  dp.scale_* holds the 0/1 mask at that moment.
__global__ void jacobi_scale_kernel(const DeviceProblem dp, const SolverDev sv) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nc = sv.n;
  if (t < nc) {
    double* sp = cam_scale_ptr(dp, sv, t);
    if (sp) *sp *= 1.0 / (1.0 + sqrt(sv.udiag[t]));
  } else if (t < nc + 3 * (int64_t)dp.M) {
    const int64_t u = t - nc; const int j = (int)(u / 3), a = (int)(u % 3);
    const int dg = (a == 0) ? 0 : (a == 1 ? 3 : 5);
    dp.scale_point[u] *= 1.0 / (1.0 + sqrt(sv.V[(size_t)j * 6 + dg]));
  }
}

// LevenbergMarquardtStrategy::ComputeStep: diagonal_ = clamp(|J_i|^2, min_lm_diagonal, max_lm_diagonal)
__global__ void clamp_diagonal_kernel(const DeviceProblem dp, const SolverDev sv, double lo, double hi) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nc = sv.n;
  if (t < nc) {
    sv.diag_c[t] = fmin(fmax(sv.udiag[t], lo), hi);
  } else if (t < nc + 3 * (int64_t)dp.M) {
    const int64_t u = t - nc; const int j = (int)(u / 3), a = (int)(u % 3);
    const int dg = (a == 0) ? 0 : (a == 1 ? 3 : 5);
    sv.diag_p[u] = fmin(fmax(sv.V[(size_t)j * 6 + dg], lo), hi);
  }
}

// max |g_i| of the UNSCALED gradient (Ceres evaluates the gradient before ScaleColumns): g = g_scaled / scale
// part: 0 = every coordinate, 1 = the points' only, 2 = the cameras' only (several ranks: a rank's own points before the camera exchange —
// their maximum travels in it —, the cameras' from the summed gradient behind it)
__global__ __launch_bounds__(256) void gradient_max_kernel(const DeviceProblem dp, const SolverDev sv, int part) {
  __shared__ double s_red[4];
  double m = 0.0;
  const int64_t nc = sv.n, np = 3 * (int64_t)dp.M;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x + (part == 1 ? nc : 0);
  if (t < (part == 2 ? nc : nc + np)) {
    const double sc = (t < nc) ? cam_scale(dp, sv, t) : dp.scale_point[t - nc];
    const double g = (t < nc) ? sv.gc[t] : sv.gp[t - nc];
    if (sc > 0.0) m = fabs(g / sc);
  }
  m = wmax(m);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) sv.partial[blockIdx.x] = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
}
// (+ `nextra` more values at `extra`: the other ranks' maxima that came with the camera exchange)
__global__ __launch_bounds__(256) void reduce_max_kernel(const double* partial, int n, double* out, const double* extra = nullptr, int nextra = 0) {
  __shared__ double s_red[4];
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += 256) v = fmax(v, partial[k]);
  for (int k = threadIdx.x; k < nextra; k += 256) v = fmax(v, extra[k]);
  v = wmax(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *out = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
}

__global__ void unscaled_gradient_kernel(const DeviceProblem dp, const SolverDev sv, double* g_pose, double* g_point) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nc = sv.n;
  if (t < nc) { const double sc = cam_scale(dp, sv, t); g_pose[t] = sc > 0.0 ? sv.gc[t] / sc : 0.0; }
  else if (t < nc + 3 * (int64_t)dp.M) { const int64_t u = t - nc; const double sc = dp.scale_point[u]; g_point[u] = sc > 0.0 ? sv.gp[u] / sc : 0.0; }
}

// ---------------------------------------------------------------------------------------------
// K5a  per point: V' = V + D_p^2 (D^2 = diagonal_/radius), 3x3 Cholesky, L^-1, z = L^-1 g_p
// (SchurEliminator::Eliminate inverts each e-block)
// ---------------------------------------------------------------------------------------------
// CLAMP: clamp_diagonal_kernel's job done on the way (the loop that runs without the host recomputes the diagonal every iteration —
// after a rejected step that is what is there already — and saves the launch): the point's own three entries by its thread, the
// camera side by the first sv.n threads of the grid.
template <bool CLAMP>
__global__ __launch_bounds__(256) void point_factor_kernel(const DeviceProblem dp, const SolverDev sv, double inv_radius, double lo, double hi) {
  if (sv.ctl) inv_radius = 1.0 / sv.ctl[kCtlRadius];   // (device-side trust region: the radius lives in HBM)
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (CLAMP && j < sv.n) sv.diag_c[j] = fmin(fmax(sv.udiag[j], lo), hi);
  if (j >= dp.M) return;
  const double* v = sv.V + (size_t)j * 6;
  double dg[3];
  if (CLAMP) {
    dg[0] = fmin(fmax(v[0], lo), hi); dg[1] = fmin(fmax(v[3], lo), hi); dg[2] = fmin(fmax(v[5], lo), hi);
    sv.diag_p[(size_t)j * 3] = dg[0]; sv.diag_p[(size_t)j * 3 + 1] = dg[1]; sv.diag_p[(size_t)j * 3 + 2] = dg[2];
  } else { dg[0] = sv.diag_p[(size_t)j * 3]; dg[1] = sv.diag_p[(size_t)j * 3 + 1]; dg[2] = sv.diag_p[(size_t)j * 3 + 2]; }
  const double a00 = v[0] + dg[0] * inv_radius, a10 = v[1], a20 = v[2], a11 = v[3] + dg[1] * inv_radius, a21 = v[4], a22 = v[5] + dg[2] * inv_radius;
  const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
  const double d11 = a11 - l10 * l10, l11 = sqrt(d11), l21 = (a21 - l20 * l10) / l11;
  const double d22 = a22 - l20 * l20 - l21 * l21, l22 = sqrt(d22);
  if (!(a00 > 0.0) || !(d11 > 0.0) || !(d22 > 0.0) || !isfinite(l22)) atomicExch(sv.chol_fail, 1);
  const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
  const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
  double* li = sv.Linv + (size_t)j * 6;
  li[0] = i00; li[1] = i10; li[2] = i11; li[3] = i20; li[4] = i21; li[5] = i22;
  const double* g = sv.gp + (size_t)j * 3;
  double* z = sv.z + (size_t)j * 3;
  z[0] = i00 * g[0]; z[1] = i10 * g[0] + i11 * g[1]; z[2] = i20 * g[0] + i21 * g[1] + i22 * g[2];
}

}  // namespace

hipError_t launch_camera_blocks(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st, bool take_candidate, bool padding_is_zero) {
  const size_t CD2 = (size_t)sv.CD * sv.CD;
  const int64_t nparam = (int64_t)dp.F * dp.P * 6 + 3 * (int64_t)dp.M + (sv.NPF > 0 ? 9 * (int64_t)dp.NI : 0);
  const unsigned grid = (unsigned)dp.F + (take_candidate ? (unsigned)((nparam + 255) / 256) : 0u);   // (launch_lm_take_candidate's copy by extra workgroups of the same launch)
  if (sv.NPF > 0 && !padding_is_zero) {   // the padding coordinates of the pseudo frames stay zero (every other entry of these regions is ASSIGNED by the kernels below: once zero, the padding stays zero — the loop that must not touch U after a rejected step says so)
    hipError_t e = hipMemsetAsync(sv.U + (size_t)sv.F * CD2, 0, ((size_t)sv.NPF * sv.F + (size_t)sv.NIB * sv.NPF * sv.NPF) * CD2 * sizeof(double), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(sv.gc + (size_t)sv.F * sv.CD, 0, (size_t)sv.NIB * sv.NPF * sv.CD * sizeof(double), st);
    if (e != hipSuccess) return e;
  }
  if (!dp.cam_part) {   // no observations on this rank: nothing was accumulated
    if (take_candidate) { hipError_t e = launch_lm_take_candidate(dp, sv, st); if (e != hipSuccess) return e; }
    hipError_t e = hipMemsetAsync(sv.U, 0, (size_t)sv.F * CD2 * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(sv.gc, 0, (size_t)sv.F * sv.CD * sizeof(double), st);
    if (e == hipSuccess && sv.NPF > 0) e = hipMemsetAsync(sv.intr_part, 0, (size_t)sv.F * 54 * sizeof(double), st);
    return e;
  }
  if (sv.CD == 12) { if (dp.calibrated) LAUNCH((camera_reduce_kernel<12, true>), grid, 256, st, dp, sv); else LAUNCH((camera_reduce_kernel<12, false>), grid, 256, st, dp, sv); }
  else { if (dp.calibrated) LAUNCH((camera_reduce_kernel<6, true>), grid, 256, st, dp, sv); else LAUNCH((camera_reduce_kernel<6, false>), grid, 256, st, dp, sv); }
  return hipSuccess;
}
hipError_t launch_jacobi_scale(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  LAUNCH(jacobi_scale_kernel, nblocks256(sv.n + 3 * (int64_t)dp.M), 256, st, dp, sv);
  return hipSuccess;
}
hipError_t launch_clamp_diagonal(const DeviceProblem& dp, const SolverDev& sv, double lo, double hi, hipStream_t st) {
  LAUNCH(clamp_diagonal_kernel, nblocks256(sv.n + 3 * (int64_t)dp.M), 256, st, dp, sv, lo, hi);
  return hipSuccess;
}
hipError_t launch_gradient_max(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  const int nb = nblocks256(sv.n + 3 * (int64_t)dp.M);
  LAUNCH(gradient_max_kernel, nb, 256, st, dp, sv, 0);
  LAUNCH(reduce_max_kernel, 1, 256, st, sv.partial, nb, sv.scalars + kGradMax, nullptr, 0);
  return hipSuccess;
}
// several ranks: max |g| over this rank's own points -> its slot behind the camera exchange's payload (xbuf[2n + 3 + rank]; the other
// ranks' slots are zeroed by launch_pack_linearize, which runs first: a SUM all-reduce then carries every rank's maximum) ...
hipError_t launch_gradient_max_points(const DeviceProblem& dp, const SolverDev& sv, int rank, hipStream_t st) {
  const int nb = std::max(1, nblocks256(3 * (int64_t)dp.M));
  LAUNCH(gradient_max_kernel, nb, 256, st, dp, sv, 1);
  LAUNCH(reduce_max_kernel, 1, 256, st, sv.partial, nb, sv.xbuf + 2 * sv.n + 3 + rank, nullptr, 0);
  return hipSuccess;
}
// ... and behind the exchange: the cameras' maximum from the summed gradient, with the ranks' point maxima -> scalars[kGradMax]
hipError_t launch_gradient_max_cameras(const DeviceProblem& dp, const SolverDev& sv, int world, hipStream_t st) {
  const int nb = std::max(1, nblocks256(sv.n));
  LAUNCH(gradient_max_kernel, nb, 256, st, dp, sv, 2);
  LAUNCH(reduce_max_kernel, 1, 256, st, sv.partial, nb, sv.scalars + kGradMax, sv.xbuf + 2 * sv.n + 3, world);
  return hipSuccess;
}
hipError_t launch_unscaled_gradient(const DeviceProblem& dp, const SolverDev& sv, double* g_pose, double* g_point, hipStream_t st) {
  LAUNCH(unscaled_gradient_kernel, nblocks256(sv.n + 3 * (int64_t)dp.M), 256, st, dp, sv, g_pose, g_point);
  return hipSuccess;
}
hipError_t launch_point_factor(const DeviceProblem& dp, const SolverDev& sv, double radius, hipStream_t st, const double* clamp) {
  if (clamp) LAUNCH(point_factor_kernel<true>, nblocks256(std::max<int64_t>(dp.M, sv.n)), 256, st, dp, sv, 1.0 / radius, clamp[0], clamp[1]);
  else LAUNCH(point_factor_kernel<false>, nblocks256(dp.M), 256, st, dp, sv, 1.0 / radius, 0.0, 0.0);
  return hipSuccess;
}
// intrinsics as a parameter block: the self block and the intrinsics gradient, summed over the frames
hipError_t launch_intr_blocks(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  if (sv.NPF == 0) return hipSuccess;
  LAUNCH(intr_reduce_kernel, 54 * sv.NIB, 256, st, dp, sv);
  return hipSuccess;
}

}  // namespace rsba
