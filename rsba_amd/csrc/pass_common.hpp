// What the kernel files of the normal equations share (kernels_camera.hip, kernels_schur.hip, kernels_point.hip, kernels_lm.hip,
// kernels_exchange.hip; kernels_selinv.hip for the dispatcher): wave reductions, the camera-side coordinate maps, the group positions
// of the P records, launch geometry, the launch macro and the choice of a kernel's (calibrated, poses per frame, loss) instantiation.
// Device code: host-only sources include solver_state.hpp, not this.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "solver_state.hpp"
#include "switches.hpp"

namespace rsba {

namespace {   // (device functions: internal linkage, as in a kernel file of its own)

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ double wmax(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

// Camera-side coordinate t in [0, Fx*CD): the real pose coordinates, then the intrinsics pseudo frames
// (9 coordinates + zero-scaled padding) when the intrinsics are a parameter block.
// Intrinsics block c (shared sess.cam: the only one; per-frame f.cam blocks: one each, CeresHandler.h:260,277) rides as
// pseudo frames F + c * NPF + v; coordinate t behind the poses is coordinate k = v * CD + t % CD of block c (k >= 9: padding).
__device__ __forceinline__ int intr_index(const SolverDev& sv, int64_t u /* t - F*CD */) {
  const int blk = (int)(u / sv.CD), c = blk / sv.NPF, k = (blk % sv.NPF) * sv.CD + (int)(u % sv.CD);
  return k < 9 ? c * 9 + k : -1;
}
__device__ __forceinline__ double* cam_scale_ptr(const DeviceProblem& dp, const SolverDev& sv, int64_t t) {
  const int64_t npose = (int64_t)sv.F * sv.CD;
  if (t < npose) return dp.scale_pose + t;
  const int idx = intr_index(sv, t - npose);
  return idx >= 0 ? dp.scale_intr + idx : nullptr;
}
__device__ __forceinline__ double cam_scale(const DeviceProblem& dp, const SolverDev& sv, int64_t t) {
  const double* p = cam_scale_ptr(dp, sv, t);
  return p ? *p : 0.0;
}
__device__ __forceinline__ size_t u_cross_off(const SolverDev& sv, int v, int f) { return ((size_t)sv.F + (size_t)v * sv.F + f) * sv.CD * sv.CD; }
__device__ __forceinline__ size_t u_self_off(const SolverDev& sv, int c, int v, int w) { return ((size_t)sv.F + (size_t)sv.NPF * sv.F + ((size_t)c * sv.NPF + v) * sv.NPF + w) * sv.CD * sv.CD; }
__device__ __forceinline__ double u_diag(const SolverDev& sv, int64_t t) {
  const int f = (int)(t / sv.CD), a = (int)(t % sv.CD);
  const size_t base = f < sv.F ? (size_t)f * sv.CD * sv.CD : u_self_off(sv, (f - sv.F) / sv.NPF, (f - sv.F) % sv.NPF, (f - sv.F) % sv.NPF);
  return sv.U[base + (size_t)a * sv.CD + a];
}

// where a slot's P record goes (solver_state.hpp: slot_gpos = element offset of its group | position of its frame in the tile << 1 | kind)
__device__ __forceinline__ size_t gpos_group(uint32_t gpos) { return (size_t)(gpos & ~15u); }
__device__ __forceinline__ int gpos_pos(uint32_t gpos) { return (int)((gpos >> 1) & 7u); }
__device__ __forceinline__ bool gpos_factored(uint32_t gpos) { return (gpos & 1u) != 0; }

}  // namespace

// (Sixteen points — a few hundred slots — per wave: the records are computed, not streamed, so the pass wants many waves in flight,
// not long ones; 64 points per wave left the 100-camera scene with 40 workgroups.)
constexpr int kSweepPoints = 16;
// ... and fewer when the problem is small: the waves of a pass all run at once (10 000 points are 625 waves of sixteen on 1 024 SIMDs),
// so what a pass takes is what ONE wave takes — its points' slots, 64 at a time — and a wave with four points is done in a third of
// the time of a wave with sixteen.  sweep_points(M): 16 from 32 k points, 8 from 16 k, 4 below.
inline int sweep_points(int64_t M) {
  static const int forced = sweep_points_override(kSweepPoints);   // (tuning aid: switches.hpp)
  return forced ? forced : M >= 32768 ? 16 : M >= 16384 ? 8 : 4;
}
// workgroups of the back-substitution (kernels_point.hip), whose partials the model cost change sums (kernels_lm.hip)
inline int point_step_blocks(const DeviceProblem& dp, const SolverDev& sv) { const int sp = sweep_points(dp.M); return sv.slot_xy ? (int)((dp.M + 4 * sp - 1) / (4 * sp)) : (int)((dp.M + 255) / 256); }

inline int nblocks256(int64_t n) { return (int)((n + 255) / 256); }

// The instantiation of a kernel that recomputes records, from the problem: f(cal, two_pose, gen) with std::bool_constants —
// calibrated (dp.calibrated), two poses per frame (sv.CD == 12), a general loss (dp.loss_general: the GEN instantiations, lm_record.hpp).
// f is a generic lambda around ONE launch; a combination its kernel does not exist for is left out there with `if constexpr`.
template <class F>
inline void with_record_variant(const DeviceProblem& dp, const SolverDev& sv, F f) {
  auto by_gen = [&](auto cal, auto two) { if (dp.loss_general) f(cal, two, std::true_type{}); else f(cal, two, std::false_type{}); };
  auto by_p = [&](auto cal) { if (sv.CD == 12) by_gen(cal, std::true_type{}); else by_gen(cal, std::false_type{}); };
  if (dp.calibrated) by_p(std::true_type{}); else by_p(std::false_type{});
}

}  // namespace rsba

#define LAUNCH(kernel, grid, block, st, ...)                       \
  do {                                                             \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__); \
    hipError_t e_ = hipGetLastError();                             \
    if (e_ != hipSuccess) return e_;                               \
  } while (0)
