// The sweep over the points' recomputed records (kernels_point.hip) and the one pass of it that the one-launch linearisation
// shares with point_blocks_rc_kernel.
#pragma once
#include "pass_common.hpp"
#include "slot_record.hpp"

namespace rsba {

namespace {   // (internal linkage, as in a kernel file of its own: what a pass leaves unread the compiler may drop)

// One wave owns kSweepPoints (pass_common.hpp; fewer when the problem is small: sweep_points) consecutive points = one contiguous slot range and walks it 64 slots at a time: every lane reduces ITS
// slot's recomputed record to NC numbers (per_slot), and the lane that owns a point adds its slots' numbers in slot order (fixed
// order: deterministic) before per_point finishes the point.  -> what per_point returns, summed over the workgroup (fixed order).
// The sums are taken by ALL 64 lanes: the wave's (point, component) pairs — 16 x NC — are dealt to the lanes, each adding its pairs'
// numbers over the point's slots in slot order (the same order as ever: same bits) — when only the 16 lanes that own a point did
// this, the other 48 waited through 20 x NC dependent LDS reads and adds per point: most of the sweep's time (the virtual-record sweep
// of a shared intrinsics block, NC = 27, took 0.91 ms at 4k cameras against 0.35 for NC = 9 over the same records).
// NCP: the slots' numbers go through LDS NCP components at a time (NC / NCP passes per 64 slots, the record computed once): the 27 of the
// virtual-record sweep in three passes of nine take 18 KB per workgroup instead of 55 — room beside the projection pass, which runs at the
// same time on its own stream — and the pairs' slot ranges are kept once per pass layout, not per component.
// WAVE_DOUBLES: a wave's share of the dynamic LDS (>= 64 NCP; the fused sweep, kernels_point.hip: virtual_project_rc_kernel, keeps a staging area in the same doubles).  per_slot also
// gets the slot's index and the wave's LDS; per_batch(wave's LDS, slots of the batch) runs once the 64 slots of a batch have been through
// per_slot, between two wave barriers, BEFORE the batch's numbers go into the same LDS.
template <bool CAL, int P, bool GEN, int NC, int NCP, int WAVE_DOUBLES, class PerSlot, class PerBatch, class PerPoint>
__device__ __forceinline__ double point_sweep_hooked(const DeviceProblem& dp, const SolverDev& sv, double* smem, int sp, int64_t block, PerSlot per_slot, PerBatch per_batch, PerPoint per_point) {
  static_assert(NC % NCP == 0 && kSweepPoints * NC <= 64 * NCP && WAVE_DOUBLES >= 64 * NCP, "passes of equal width; the final gather fits the buffer");
  constexpr int NPART = NC / NCP, NPAIR = kSweepPoints * NCP, PER = (NPAIR + 63) / 64;   // pairs (point, component of a pass): sized for the most points a wave takes; sp <= kSweepPoints of them this launch
  __shared__ double s_red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* cbuf = smem + (size_t)wave * WAVE_DOUBLES;
  const int64_t j0 = (block * 4 + wave) * sp;
  double ret = 0.0;
  auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); };
  if (j0 < dp.M) {   // wave-uniform
    const int jn = (int)(dp.M - j0 < sp ? dp.M - j0 : sp);
    const bool mine = lane < jn;
    const int64_t j = j0 + (mine ? lane : 0);
    const int64_t lo = mine ? sv.point_ptr[j] : 0, hi = mine ? sv.point_ptr[j + 1] : 0;
    const int64_t sb = sv.point_ptr[j0], se = sv.point_ptr[j0 + jn];
    // this lane's pairs: pair = lane + 64 i -> point pair / NCP of the wave, component pair % NCP of every pass; the point's slot range from its owner lane
    double acc[NPART][PER]; int64_t plo[PER], phi[PER]; int pq[PER], pp[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int pair = lane + 64 * i, pj = pair / NCP;
#pragma unroll
      for (int part = 0; part < NPART; ++part) acc[part][i] = 0.0;
      pq[i] = pair % NCP; pp[i] = pj;
      const long long l = __shfl((long long)lo, pj < kSweepPoints ? pj : 0, 64), h = __shfl((long long)hi, pj < kSweepPoints ? pj : 0, 64);
      const bool live = pair < jn * NCP;
      plo[i] = live ? l : 0; phi[i] = live ? h : 0;
    }
    for (int64_t c0 = sb; c0 < se; c0 += 64) {
      const int nrec = (int)(se - c0 < 64 ? se - c0 : 64);
      double c[NC];
      {
        const int64_t s = c0 + lane < se ? c0 + lane : se - 1;
        ObsOut<CAL, P> o;
        int frame, pt;
        slot_record<CAL, P, GEN>(dp, sv, sv.slot_xy, s, o, frame, pt);
        per_slot(o, frame, pt, s, cbuf, c);
      }
      per_batch(cbuf, nrec, wave_sync);
#pragma unroll
      for (int part = 0; part < NPART; ++part) {
#pragma unroll
        for (int q = 0; q < NCP; ++q) cbuf[lane * NCP + q] = c[part * NCP + q];
        wave_sync();
        // (four numbers of a pair are READ before the first of them is added — in slot order, as ever: the same bits — with the rows' offsets
        // in the instructions: 2.5 instructions per number instead of the 9 of the plain loop, which was 17 - 29 % of these passes)
#pragma unroll
        for (int i = 0; i < PER; ++i) {
          const int klo = (int)((plo[i] > c0 ? plo[i] : c0) - c0), khi = (int)((phi[i] < c0 + nrec ? phi[i] : c0 + nrec) - c0);
          const double* col = cbuf + pq[i];
          int k = klo;
          for (; k + 4 <= khi; k += 4) {
            const double* p = col + k * NCP;
            const double v0 = p[0], v1 = p[NCP], v2 = p[2 * NCP], v3 = p[3 * NCP];
            acc[part][i] += v0; acc[part][i] += v1; acc[part][i] += v2; acc[part][i] += v3;
          }
          for (; k < khi; ++k) acc[part][i] += col[k * NCP];
        }
        wave_sync();
      }
    }
    // the sums of a point back to the lane that owns it: [point][NC]
#pragma unroll
    for (int i = 0; i < PER; ++i)
#pragma unroll
      for (int part = 0; part < NPART; ++part) if (lane + 64 * i < NPAIR) cbuf[pp[i] * NC + part * NCP + pq[i]] = acc[part][i];
    wave_sync();
    if (mine) {
      double a[NC];
#pragma unroll
      for (int q = 0; q < NC; ++q) a[q] = cbuf[lane * NC + q];
      ret = per_point(j, a);
    }
  }
  ret = wsum(ret);
  if (lane == 0) s_red[wave] = ret;
  __syncthreads();
  return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}
template <bool CAL, int P, bool GEN, int NC, int NCP = NC, class PerSlot, class PerPoint>
__device__ __forceinline__ double point_sweep(const DeviceProblem& dp, const SolverDev& sv, double* smem, int sp, int64_t block, PerSlot per_slot, PerPoint per_point) {
  return point_sweep_hooked<CAL, P, GEN, NC, NCP, 64 * NCP>(dp, sv, smem, sp, block,
    [&](const ObsOut<CAL, P>& o, int frame, int pt, int64_t, double*, double* c) { per_slot(o, frame, pt, c); },
    [](double*, int, auto&) {}, per_point);
}

// K2b without records: V_j, g_p,j
template <bool CAL, int P, bool GEN>
__device__ __forceinline__ void point_blocks_sweep(const DeviceProblem& dp, const SolverDev& sv, double* smem, int sp, int64_t block) {
  constexpr int CD = (CAL ? 0 : 9) + 6 * P;   // columns in front of the point's
  point_sweep<CAL, P, GEN, 9>(dp, sv, smem, sp, block,
    [&](const ObsOut<CAL, P>& o, int, int, double c[9]) {
      const double r0 = o.r[0], r1 = o.r[1], p0[3] = {o.J[0][CD], o.J[0][CD + 1], o.J[0][CD + 2]}, p1[3] = {o.J[1][CD], o.J[1][CD + 1], o.J[1][CD + 2]};
      c[0] = p0[0] * p0[0] + p1[0] * p1[0]; c[1] = p0[0] * p0[1] + p1[0] * p1[1]; c[2] = p0[0] * p0[2] + p1[0] * p1[2];
      c[3] = p0[1] * p0[1] + p1[1] * p1[1]; c[4] = p0[1] * p0[2] + p1[1] * p1[2]; c[5] = p0[2] * p0[2] + p1[2] * p1[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) c[6 + k] = p0[k] * r0 + p1[k] * r1;
    },
    [&](int64_t j, const double acc[9]) {
#pragma unroll
      for (int k = 0; k < 6; ++k) sv.V[(size_t)j * 6 + k] = acc[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) sv.gp[(size_t)j * 3 + k] = acc[6 + k];
      return 0.0;
    });
}

}  // namespace

}  // namespace rsba
