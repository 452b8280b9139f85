// The camera blocks of one frame and the copy of an accepted candidate over x, by workgroup: shared by camera_reduce_kernel
// (kernels_camera.hip) and the one-launch linearisation (kernels_point.hip: linearize_blocks_kernel).
#pragma once
#include "pass_common.hpp"

namespace rsba {

namespace {   // (internal linkage, as in a kernel file of its own: what a pass leaves unread the compiler may drop)

// ---------------------------------------------------------------------------------------------
// K2a  per-frame camera block  U_f = sum Jc^T Jc,  g_f = sum Jc^T r  and, with intrinsics as a parameter block
// (opt.model.calibrated == false, shared sess.cam), the blocks of J^T J that are NOT block-diagonal:
//   cross: U[F+v][f] rows = intrinsics coordinates of pseudo frame v, cols = pose coordinates of frame f
//   self : per-frame partials of Ji^T Ji (45 unique) and Ji^T r (9), summed over frames by intr_reduce_kernel.
// The products themselves are formed by the evaluation kernel (kernels_eval.hip): every wave leaves, per frame it touches, the one or two
// 16 x 16 blocks that hold everything on and below the diagonal of G = [Ji | Jc | r]^T [Ji | Jc | r] (device_state.hpp: cam_part_blocks /
// cam_part_entry).  Here one workgroup per frame sums its waves' partials in wave order (fixed order: deterministic) and files the entries of G.
// ---------------------------------------------------------------------------------------------
// lm_take_candidate_kernel's copy, by workgroup `block` of a launch that carries it along
__device__ __forceinline__ void take_candidate_block(const DeviceProblem& dp, const SolverDev& sv, int64_t block) {
  const int64_t t = block * 256 + threadIdx.x, npose = (int64_t)dp.F * dp.P * 6, npoint = 3 * (int64_t)dp.M, nintr = sv.NPF > 0 ? (int64_t)dp.NI * 9 : 0;
  if (t < npose) dp.poses[t] = sv.trial_poses[t];
  else if (t < npose + npoint) dp.points[t - npose] = sv.trial_points[t - npose];
  else if (t < npose + npoint + nintr) dp.intr[t - npose - npoint] = sv.trial_intr[t - npose - npoint];
}
template <int CD, bool CAL>
__device__ __forceinline__ void camera_reduce_frame(const DeviceProblem& dp, const SolverDev& sv, const int f) {
  constexpr int NI = CAL ? 0 : 9, NCOL = NI + CD + 1, NBLK = cam_part_blocks(NCOL);   // (device_state.hpp: where the evaluation kernel leaves which entry of G)
  __shared__ double G[NBLK][256];
  const int e = threadIdx.x;
  const int64_t s0 = sv.frame_ptr[f], s1 = sv.frame_ptr[f + 1];
  double sum[NBLK];
#pragma unroll
  for (int q = 0; q < NBLK; ++q) sum[q] = 0.0;
  if (s1 > s0) {
    // where each of the frame's waves left its partial: looked up by a thread per wave first (three dependent loads), so that the sums
    // below — in wave order, as ever — issue their loads back to back instead of behind that chain
    __shared__ int s_seg[256];
    const int rk = dp.frame_rank[f];
    const int64_t w0 = s0 >> 6, w1 = (s1 - 1) >> 6;
    for (int64_t wb = w0; wb <= w1; wb += 256) {
      const int nw = (int)(w1 - wb + 1 < 256 ? w1 - wb + 1 : 256);
      __syncthreads();
      if (e < nw) s_seg[e] = dp.wave_seg_base[wb + e] + rk - dp.frame_rank[dp.obs_frame[(wb + e) << 6]];
      __syncthreads();
      int i = 0;
      for (; i + 4 <= nw; i += 4) {
        double v[4][NBLK];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int q = 0; q < NBLK; ++q) v[u][q] = dp.cam_part[((size_t)s_seg[i + u] * NBLK + q) * 256 + e];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int q = 0; q < NBLK; ++q) sum[q] += v[u][q];
      }
      for (; i < nw; ++i)
#pragma unroll
        for (int q = 0; q < NBLK; ++q) sum[q] += dp.cam_part[((size_t)s_seg[i] * NBLK + q) * 256 + e];
    }
  }
#pragma unroll
  for (int q = 0; q < NBLK; ++q) G[q][e] = sum[q];
  __syncthreads();
  auto g = [&](int a, int b) {   // entry (a, b) of the symmetric G
    if (a < b) { const int t = a; a = b; b = t; }
    return NBLK == 1 ? G[0][a * 16 + b] : (&G[0][0])[cam_part_entry(a, b)];
  };
  for (int idx = e; idx < CD * CD; idx += 256) sv.U[(size_t)f * CD * CD + idx] = g(NI + idx / CD, NI + idx % CD);
  if (e < CD) sv.gc[(size_t)f * CD + e] = g(NI + CD, NI + e);
  if (!CAL) {
    for (int idx = e; idx < 9 * CD; idx += 256) {
      const int kk = idx / CD, c = idx % CD;
      sv.U[u_cross_off(sv, kk / CD, f) + (size_t)(kk % CD) * CD + c] = g(NI + c, kk);
    }
    if (e < 54) {
      double v;
      if (e >= 45) v = g(NI + CD, e - 45);
      else { int a = 0, rem = e; while (rem >= 9 - a) { rem -= 9 - a; ++a; } v = g(a + rem, a); }
      sv.intr_part[(size_t)f * 54 + e] = v;
    }
  }
}

}  // namespace

}  // namespace rsba
