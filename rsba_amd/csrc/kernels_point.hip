// K2b, K5b, K7 and K8 of SURVEY §2.1: the point-side passes — point blocks, P records (and the virtual records of the intrinsics
// pseudo frames), point steps — from stored records and from recomputed ones.  All fp64; all sums are taken in a fixed order
// (no floating-point atomics), so a solve is bit-reproducible from run to run.
//
// These replace, for rsba's BA problems, what Ceres-Solver 1.9's SchurEliminator / SchurComplementSolver
// and TrustRegionMinimizer compute on the CPU (call site
// /root/reference/src/rsba/CeresHandler.h:419).  They are HBM/latency-bound block operations on 12x12,
// 12x3 and 3x3 blocks — deliberately NOT reshaped into MFMA GEMMs: on gfx950 the fp64 MFMA rate equals
// the fp64 VALU rate, and padding 12 -> 16 would waste 44 % of it.
#include "camera_reduce.hpp"
#include "point_sweep.hpp"

namespace rsba {

namespace {

// virtual observation records of the pseudo frames: one group per (point j, intrinsics block c the point is seen through),
// Q_j,c = sum_{o of j in frames that use c} Ji_o^T (Jp_o L_j^-T)   (9 x 3), cut into the NPF pseudo-frame records of the group
template <int CD>
__global__ __launch_bounds__(256) void virtual_records_kernel(const DeviceProblem dp, const SolverDev sv) {
  if (lm_stopped(sv.ctl)) return;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= sv.nvgroups) return;
  const int j = sv.vgroup_point[g], c = sv.vgroup_intr[g];
  const int REC = 2 + 2 * dp.K, KC = dp.K - 3;
  const double* li = sv.Linv + (size_t)j * 6;
  const double linv[6] = {li[0], li[1], li[2], li[3], li[4], li[5]};   // (read once, in front of the loop over the slots)
  double Q[9][3];
#pragma unroll
  for (int k = 0; k < 9; ++k) { Q[k][0] = 0.0; Q[k][1] = 0.0; Q[k][2] = 0.0; }
  for (int64_t s = sv.point_ptr[j]; s < sv.point_ptr[j + 1]; ++s) {
    if (sv.NIB > 1 && dp.frame_intr[sv.slot_frame[s]] != c) continue;
    const double* rec = lm_records(dp, false) + (size_t)s * REC;
    double B[2][3];
    jp_linv(rec + 2, 3, linv, B);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double a0 = rec[8 + k], a1 = rec[8 + KC + k];
#pragma unroll
      for (int m = 0; m < 3; ++m) Q[k][m] += a0 * B[0][m] + a1 * B[1][m];
    }
  }
  for (int v = 0; v < sv.NPF; ++v) {
    const uint32_t gpos = sv.slot_gpos[dp.N + g * sv.NPF + v];   // the virtual slot's place: its group (always full form: a pseudo frame's tile), frame position of its tile
    double* out = sv.Pm + gpos_group(gpos) + gpos_pos(gpos) * CD;
#pragma unroll
    for (int rl = 0; rl < CD; ++rl) {
      const int k = v * CD + rl;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        double q = 0.0;
#pragma unroll
        for (int kk = 0; kk < 9; ++kk) if (kk == k) q = Q[kk][m];
        out[m * kTile + rl] = q;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// K2b  per-point block  V_j = sum Jp^T Jp (6 unique),  g_p,j = sum Jp^T r   (point-major records)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void point_blocks_kernel(const DeviceProblem dp, const SolverDev sv) {
  if (lm_not_accepted(sv.ctl)) return;   // (device-side trust region: a rejected candidate is not linearised)
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= dp.M) return;
  const int REC = 2 + 2 * dp.K;
  double v[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  for (int64_t s = sv.point_ptr[j]; s < sv.point_ptr[j + 1]; ++s) {
    const double2* rp = reinterpret_cast<const double2*>(lm_records(dp, false) + (size_t)s * REC);
    const double2 a = rp[0], b = rp[1], c = rp[2], d = rp[3];   // r0 r1 | p00 p01 | p02 p10 | p11 p12
    const double r0 = a.x, r1 = a.y, p0[3] = {b.x, b.y, c.x}, p1[3] = {c.y, d.x, d.y};
    v[0] += p0[0] * p0[0] + p1[0] * p1[0]; v[1] += p0[0] * p0[1] + p1[0] * p1[1]; v[2] += p0[0] * p0[2] + p1[0] * p1[2];
    v[3] += p0[1] * p0[1] + p1[1] * p1[1]; v[4] += p0[1] * p0[2] + p1[1] * p1[2]; v[5] += p0[2] * p0[2] + p1[2] * p1[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] += p0[k] * r0 + p1[k] * r1;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) sv.V[(size_t)j * 6 + k] = v[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) sv.gp[(size_t)j * 3 + k] = g[k];
}

// K5b  per observation (point-major): P = Jc^T (Jp L^-T)   (CD x 3)
// One wave = 64 consecutive slots.  Records are moved from HBM to LDS with fully coalesced 512-B wave
// accesses (a lane-per-record global access pattern touches 64 cache lines per instruction and ran 4x
// slower); each lane then works on its own record out of LDS (odd pitch: no bank conflicts).
// The results go to the GROUP layout the Schur kernel reads (solver_state.hpp, Pm): coordinate c of the point
// against the CD rows of the slot's frame is a run of CD doubles at row c of the slot's (point, tile) group,
// position (frame % FT) * CD.  Consecutive slots of a point are consecutive frames, so the runs of one
// coordinate line up back to back: the wave stores coordinate by coordinate, each store instruction covering
// (mostly) whole 128-B lines.
constexpr int kProjectChunks = 2;   // consecutive 64-slot chunks per wave of the projection kernel at most (one when the scene is small: project_chunks).  Round 6: 8 until then — swept again on the slim (all-factored, three workgroups per CU) form: C4 project phase 0.096 / 0.096 / 0.101 / 0.112 / 0.113 / 0.150 ms for 1 / 2 / 4 / 8 / 16 / 32
inline int project_chunks(int64_t N) {   // ~2 k waves or more
  static const int forced = project_chunks_override();   // (tuning aid: switches.hpp)
  const int64_t c = N / 64 / 2048;
  return forced ? forced : (int)(c < 1 ? 1 : c > kProjectChunks ? kProjectChunks : c);
}

template <int CD, int KC>
__global__ __launch_bounds__(256) void project_kernel(const DeviceProblem dp, const SolverDev sv) {
  if (lm_stopped(sv.ctl)) return;
  constexpr int REC = 8 + 2 * KC, OUT = CD * 3;
  constexpr int PITCH = (REC > OUT ? REC : OUT) | 1;          // odd
  constexpr int off = KC - CD;                                  // 9 when intrinsics columns precede the pose
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* buf = smem + (size_t)wave * (64 * PITCH + 32);
  uint32_t* s_gpos = reinterpret_cast<uint32_t*>(buf + 64 * PITCH);   // [64] where each slot of the chunk goes (problems that keep records store every group in full form)
  const int64_t sb = ((int64_t)blockIdx.x * 4 + wave) * 64 * kProjectChunks;
  if (sb >= dp.N) return;
  const int64_t se = sb + 64 * kProjectChunks < dp.N ? sb + 64 * kProjectChunks : dp.N;
  // the next chunk's records (and the point of each slot) travel in registers while this one is worked on; indices
  // are clamped rather than predicated so that nothing next to the loads waits for them
  double pre[REC];
  int pre_point = 0; uint32_t pre_gpos = 0;
  auto issue = [&](int64_t c0) {
    const int64_t last = (se - c0) * REC - 1;
    const double* src = lm_records(dp, false) + (size_t)c0 * REC;
#pragma unroll
    for (int k = 0; k < REC; ++k) { const int64_t idx = k * 64 + lane; pre[k] = src[idx < last ? idx : last]; }
    const int64_t sl = c0 + lane < se ? c0 + lane : se - 1;
    pre_point = sv.slot_point[sl]; pre_gpos = sv.slot_gpos[sl];
  };
  issue(sb);
  for (int64_t s0 = sb; s0 < se; s0 += 64) {
    const int64_t nslot = se - s0 < 64 ? se - s0 : 64;
#pragma unroll
    for (int k = 0; k < REC; ++k) { const int idx = k * 64 + lane; buf[(idx / REC) * PITCH + idx % REC] = pre[k]; }
    const double* li = sv.Linv + (size_t)pre_point * 6;
    const double linv[6] = {li[0], li[1], li[2], li[3], li[4], li[5]};   // (requested here, in front of the next chunk's loads)
    s_gpos[lane] = pre_gpos;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (s0 + 64 < se) issue(s0 + 64);
    double out[OUT];
    {
      const double* rec = buf + lane * PITCH;   // lanes past nslot work on stale LDS; their results are not stored
      double B[2][3];
      jp_linv(rec + 2, 3, linv, B);
#pragma unroll
      for (int a = 0; a < CD; ++a) {
        const double c0 = rec[8 + off + a], c1 = rec[8 + KC + off + a];
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k * CD + a] = c0 * B[0][k] + c1 * B[1][k];   // component-major inside the record
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int e = 0; e < OUT; ++e) buf[lane * PITCH + e] = out[e];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // Stores: a lane owns one double (w) of the CD-long runs; kPer = 64 / CD consecutive slots per instruction (their runs of one
    // coordinate sit back to back while the slots stay inside one group), three instructions — one per coordinate, 48 doubles
    // apart: the store's immediate offset — per address computation.  (64 % CD lanes idle.)
    constexpr int kPer = 64 / CD;
    const int my = lane / CD, w = lane % CD;
    if (my < kPer) {
#pragma unroll 2
      for (int i = 0; i * kPer < 64; ++i) {
        const int sl = i * kPer + my;
        if (sl < nslot) {
          const uint32_t gpos = s_gpos[sl];
          double* dst = sv.Pm + (gpos_group(gpos) + (size_t)(gpos_pos(gpos) * CD + w));
          const double* src = buf + sl * PITCH + w;
#pragma unroll
          for (int comp = 0; comp < 3; ++comp) dst[comp * kTile] = src[comp * CD];
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// K7 + K8  point steps and the model cost change in ONE pass over the point-major records:
//   y_p,j = L_j^-T ( z_j - L_j^-1 u_j ),  u_j = sum_o Jp_o^T t_o,  t_o = Jc_o y_c(frame(o)) + Ji_o y_i
// (the back-substitution y_p = L^-T (z - sum_o P_o^T y_c) with P_o = Jc_o^T Jp_o L^-T written out), and
//   model_cost_change = -sum_o m_o.(r_o + m_o / 2),  m_o = -(t_o + Jp_o y_p)      (TrustRegionMinimizer)
// expanded per point so that it needs nothing per observation beyond what the same pass accumulates:
//   sum_o m.(r + m/2) = -sum r.t - y_p.g_p + 1/2 sum |t|^2 + y_p.u + 1/2 y_p^T V y_p      (V, g_p from K2b).
// The records (256 B at 1k cameras) are read once — before, the P records (288 B) and then the Jacobian records
// were each streamed by their own kernel.  One wave owns 64 consecutive points = one contiguous slot range, moves it
// through LDS 64 records at a time with fully coalesced 512-B wave loads (the next 64 already in flight in
// registers), every lane reduces ITS record to 5 numbers, and the lane that owns the point sums its records' numbers
// in slot order (fixed order: deterministic).
template <int CD, int KC>
__global__ __launch_bounds__(256) void point_step_kernel(const DeviceProblem dp, const SolverDev sv) {
  if (lm_stopped(sv.ctl)) return;
  constexpr int REC = 8 + 2 * KC, PITCH = REC | 1, off = KC - CD, NC = 5;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ double s_red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* buf = smem + (size_t)wave * (64 * PITCH + 64 * NC);
  double* cbuf = buf + 64 * PITCH;
  const int64_t j0 = ((int64_t)blockIdx.x * 4 + wave) * 64;
  double mc = 0.0;
  if (j0 < dp.M) {   // wave-uniform
    const int jn = (int)(dp.M - j0 < 64 ? dp.M - j0 : 64);
    const bool mine = lane < jn;
    const int64_t j = j0 + (mine ? lane : 0);
    const int64_t lo = mine ? sv.point_ptr[j] : 0, hi = mine ? sv.point_ptr[j + 1] : 0;
    const int64_t sb = sv.point_ptr[j0], se = sv.point_ptr[j0 + jn];
    double acc[NC] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double pre[REC];
    int pre_frame = 0;
    // loads of the chunk at c0; indices are clamped into the wave's range instead of predicated (the values of a
    // clamped lane are never used), so nothing next to the load makes the compiler wait for it
    auto issue = [&](int64_t c0) {
      const int64_t last = (se - c0) * REC - 1;
      const double* src = lm_records(dp, false) + (size_t)c0 * REC;
#pragma unroll
      for (int k = 0; k < REC; ++k) { const int64_t idx = k * 64 + lane; pre[k] = src[idx < last ? idx : last]; }
      pre_frame = sv.slot_frame[c0 + lane < se ? c0 + lane : se - 1];
    };
    if (sb < se) issue(sb);
    for (int64_t c0 = sb; c0 < se; c0 += 64) {
      const int nrec = (int)(se - c0 < 64 ? se - c0 : 64);
#pragma unroll
      for (int k = 0; k < REC; ++k) { const int idx = k * 64 + lane; buf[(idx / REC) * PITCH + idx % REC] = pre[k]; }
      const int frame = pre_frame;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (c0 + 64 < se) issue(c0 + 64);
      if (lane < nrec) {
        const double* rec = buf + lane * PITCH;
        const double* yc = sv.step + (size_t)frame * CD;
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int a = 0; a < CD; ++a) { const double y = yc[a]; t0 += rec[8 + off + a] * y; t1 += rec[8 + KC + off + a] * y; }
        if (off > 0) {
          const double* yi = sv.step + ((size_t)sv.F + (size_t)(sv.NIB > 1 ? dp.frame_intr[frame] : 0) * sv.NPF) * CD;   // step of the frame's intrinsics block: 9 coordinates across its pseudo frames
#pragma unroll
          for (int k = 0; k < off; ++k) { const double y = yi[k]; t0 += rec[8 + k] * y; t1 += rec[8 + KC + k] * y; }
        }
        double* c = cbuf + lane * NC;
        c[0] = rec[2] * t0 + rec[5] * t1; c[1] = rec[3] * t0 + rec[6] * t1; c[2] = rec[4] * t0 + rec[7] * t1;   // Jp^T t
        c[3] = t0 * t0 + t1 * t1;
        c[4] = rec[0] * t0 + rec[1] * t1;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int64_t s_lo = lo > c0 ? lo : c0, s_hi = hi < c0 + nrec ? hi : c0 + nrec;
      for (int64_t sidx = s_lo; sidx < s_hi; ++sidx) {
        const double* c = cbuf + (sidx - c0) * NC;
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] += c[q];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (mine) {
      const double* li = sv.Linv + (size_t)j * 6;
      const double* z = sv.z + (size_t)j * 3;
      const double i00 = li[0], i10 = li[1], i11 = li[2], i20 = li[3], i21 = li[4], i22 = li[5];
      const double u0 = acc[0], u1 = acc[1], u2 = acc[2];
      const double w0 = z[0] - i00 * u0, w1 = z[1] - (i10 * u0 + i11 * u1), w2 = z[2] - (i20 * u0 + i21 * u1 + i22 * u2);
      const double y0 = i00 * w0 + i10 * w1 + i20 * w2, y1 = i11 * w1 + i21 * w2, y2 = i22 * w2;
      double* yp = sv.yp + (size_t)j * 3;
      yp[0] = y0; yp[1] = y1; yp[2] = y2;
      const double* v = sv.V + (size_t)j * 6;   // xx xy xz yy yz zz
      const double* g = sv.gp + (size_t)j * 3;
      const double vy0 = v[0] * y0 + v[1] * y1 + v[2] * y2, vy1 = v[1] * y0 + v[3] * y1 + v[4] * y2, vy2 = v[2] * y0 + v[4] * y1 + v[5] * y2;
      mc = -acc[4] - (y0 * g[0] + y1 * g[1] + y2 * g[2]) + 0.5 * acc[3] + (y0 * u0 + y1 * u1 + y2 * u2) + 0.5 * (y0 * vy0 + y1 * vy1 + y2 * vy2);
    }
  }
  mc = wsum(mc);
  if (lane == 0) s_red[wave] = mc;
  __syncthreads();
  if (threadIdx.x == 0) sv.partial[blockIdx.x] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// ---------------------------------------------------------------------------------------------
// The point-side passes RECOMPUTE every observation's record (lm_record.hpp) instead of reading the point-major copy the
// evaluation kernel used to leave for them — 24 B of observation + cached poses in, not 256 - 400 B of record.  Same arithmetic
// as the record-based kernels above, which remain for problems with SEVERAL intrinsics parameter blocks (per-frame f.cam:
// a point then owns one virtual record group per block it is seen through).
// ---------------------------------------------------------------------------------------------
__global__ void slot_xy_kernel(const DeviceProblem dp, double2* __restrict__ slot_xy) {   // once per plan: observations in slot (point-major) order
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < dp.N) slot_xy[dp.obs_slot[i]] = dp.xy[i];
}

// ---- the pieces the projection pass, the virtual-record sweep and the fused sweep of both share: one text, the same bits ----
// A slot's FACTORED P record (see project_rc_kernel) into its 19 doubles of a wave's staging area: q = Jq^T B component-major | tau
template <bool CAL, int P>
__device__ __forceinline__ void stage_factored_record(const ObsOut<CAL, P>& o, const double B[2][3], double* dst) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k * 6 + a] = o.Jq[0][a] * B[0][k] + o.Jq[1][a] * B[1][k];
  dst[18] = o.tau;
}
// ... and the staged records of a batch's first nslot slots (pitch doubles apart; s_gpos: where each goes) into their groups: six lanes
// per slot (a pose coordinate each), ten slots per pass; the lane of coordinate 0 also stores tau.  ALLF: every slot of the batch is
// factored (known when the kernel is compiled); otherwise the slots whose group is not are left to the caller.
template <bool ALLF, class Count>
__device__ __forceinline__ void store_factored_groups(const SolverDev& sv, const double* staging, int pitch, const uint32_t* s_gpos, Count nslot, int lane) {
  constexpr int kPerF = 10;
  const int my = lane / 6, w = lane % 6;
  if (my < kPerF) {
#pragma unroll 2
    for (int i = 0; i * kPerF < 64; ++i) {
      const int sl = i * kPerF + my;
      if (sl < nslot) {
        const uint32_t gp = s_gpos[sl];
        if (ALLF || gpos_factored(gp)) {
          const int src_no = 6 * gpos_pos(gp) + w;   // source 0..23 of the group
          double* dst = sv.Pm + gpos_group(gp) + (src_no < 16 ? src_no : 48 + (src_no - 16));
          const int stride = src_no < 16 ? 16 : 8;
          const double* src = staging + sl * pitch + w;
#pragma unroll
          for (int comp = 0; comp < 3; ++comp) dst[comp * stride] = src[comp * 6];
          if (w == 0) sv.Pm[gpos_group(gp) + 72 + gpos_pos(gp)] = staging[sl * pitch + 18];
        }
      }
    }
  }
}
// The 27 numbers of a slot that the virtual records of ONE intrinsics block sum per point: Ji_o^T B (9 x 3), B = Jp_o L_j^-T
template <int P>
__device__ __forceinline__ void virtual_record_terms(const ObsOut<false, P>& o, const double B[2][3], double c[27]) {
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int m = 0; m < 3; ++m) c[3 * k + m] = o.J[0][k] * B[0][m] + o.J[1][k] * B[1][m];
}
// ... and their sums over point j's slots, Q_j (9 x 3), cut into the NPF pseudo-frame records of the point's virtual slots (see virtual_records_kernel)
template <int CD>
__device__ __forceinline__ double store_virtual_records(const DeviceProblem& dp, const SolverDev& sv, int64_t j, const double acc[27]) {
  const int64_t g = sv.point_vgroup[j];
  if (g < 0) return 0.0;
  for (int v = 0; v < sv.NPF; ++v) {
    const uint32_t gpos = sv.slot_gpos[dp.N + g * sv.NPF + v];   // (a pseudo frame's tile: full form)
    double* out = sv.Pm + gpos_group(gpos) + gpos_pos(gpos) * CD;
#pragma unroll
    for (int rl = 0; rl < CD; ++rl) {
      const int k = v * CD + rl;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        double q = 0.0;
#pragma unroll
        for (int kk = 0; kk < 9; ++kk) if (kk == k) q = acc[3 * kk + m];
        out[m * kTile + rl] = q;
      }
    }
  }
  return 0.0;
}

// K5b without records: P = Jc^T (Jp L^-T) of 64 consecutive slots per wave and step, into the group layout (see project_kernel).
// A slot whose group is stored FACTORED (two-pose frame tiles, solver_state.hpp: kGroupFactored) leaves q = Jq^T (Jp L^-T), 6 x 3 — the
// block with respect to the interpolated pose, loss-corrected, WITHOUT the (1 - tau) / tau weights and without the column scales — and
// tau: the twelve rows (1 - tau) q | tau q are formed by the Schur kernel in registers, the column scales are applied where its partial
// tiles are merged.  Half the bytes written here (the pass is bound by its stores) and read there.
//   group layout: [c][16] sources s = 0..15 of coordinate c | [c][8] sources 16..23 | tau[4];  source s = 6 (frame position in the tile) + pose coordinate
// ALLF: every slot's group is factored (SolverDev::all_real_factored — the rule for two-pose problems; a tile that mixes real and pseudo
// frames is the exception): 19 doubles per slot go through LDS instead of 36 — 40 KB per workgroup instead of 76, and with the register
// budget of three waves per SIMD the pass, which is bound by its fp64 arithmetic, runs three workgroups per CU instead of two.
template <bool CAL, int P, bool ALLF, bool GEN = false>
__global__ __launch_bounds__(256, ALLF ? 3 : 1) void project_rc_kernel(const DeviceProblem dp, const SolverDev sv, int nch) {
  if (lm_stopped(sv.ctl)) return;   // (device-side trust region: the solve is over, iterations enqueued ahead fall through)
  static_assert(!ALLF || P == 2, "factored groups are a two-pose form");
  constexpr int CD = 6 * P, OUT = CD * 3, PITCH = ALLF ? 19 : (OUT | 1), kPer = 64 / CD, OP = CAL ? 0 : 9;   // OP: the pose columns follow the 9 intrinsics columns
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* buf = smem + (size_t)wave * (64 * PITCH + 32);
  uint32_t* s_gpos = reinterpret_cast<uint32_t*>(buf + 64 * PITCH);
  const int64_t sb = ((int64_t)blockIdx.x * 4 + wave) * 64 * nch;
  if (sb >= dp.N) return;
  const int64_t se = sb + 64 * nch < dp.N ? sb + 64 * nch : dp.N;
  for (int64_t s0 = sb; s0 < se; s0 += 64) {
    const int64_t nslot = se - s0 < 64 ? se - s0 : 64;
    const int64_t s = s0 + lane < se ? s0 + lane : se - 1;   // (lanes past the end repeat the last slot; nothing of theirs is stored)
    ObsOut<CAL, P> o;
    int frame, j;
    slot_record<CAL, P, GEN>(dp, sv, sv.slot_xy, s, o, frame, j);
    double B[2][3];
    jp_linv(&o.J[0][OP + CD], o.K, sv.Linv + (size_t)j * 6, B);
    const uint32_t gpos = sv.slot_gpos[s];
    if (ALLF || (P == 2 && gpos_factored(gpos))) {
      stage_factored_record(o, B, buf + lane * PITCH);
    } else {
#pragma unroll
      for (int a = 0; a < CD; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) buf[lane * PITCH + k * CD + a] = o.J[0][OP + a] * B[0][k] + o.J[1][OP + a] * B[1][k];
    }
    s_gpos[lane] = gpos;
    const bool any_factored = ALLF || (P == 2 && __ballot(gpos_factored(gpos)) != 0ull), any_full = !ALLF && __ballot(!(P == 2 && gpos_factored(gpos))) != 0ull;   // (wave-uniform: a wave's slots are almost always of one kind)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (any_factored) store_factored_groups<ALLF>(sv, buf, PITCH, s_gpos, nslot, lane);
    if (any_full) {
      const int my = lane / CD, w = lane % CD;
      if (my < kPer) {
#pragma unroll 2
        for (int i = 0; i * kPer < 64; ++i) {
          const int sl = i * kPer + my;
          if (sl < nslot) {
            const uint32_t gp = s_gpos[sl];
            if (!gpos_factored(gp)) {
              double* dst = sv.Pm + (gpos_group(gp) + (size_t)(gpos_pos(gp) * CD + w));
              const double* src = buf + sl * PITCH + w;
#pragma unroll
              for (int comp = 0; comp < 3; ++comp) dst[comp * kTile] = src[comp * CD];
            }
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

template <bool CAL, int P, bool GEN = false>
__global__ __launch_bounds__(256) void point_blocks_rc_kernel(const DeviceProblem dp, const SolverDev sv, int sp) {
  if (lm_not_accepted(sv.ctl)) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  point_blocks_sweep<CAL, P, GEN>(dp, sv, smem, sp, blockIdx.x);
}
// The linearisation of an accepted candidate in ONE launch (the loop that runs without the host): the frames' camera blocks, the copy of
// the candidate over x, and the points' blocks side by side — neither reads what the other writes; the point sweeps read the candidate
// where it still lies (dq: dp with the trial buffers for parameters), since the copy over x is in flight beside them.
template <bool CAL, int P, bool GEN = false>
__global__ __launch_bounds__(256) void linearize_blocks_kernel(const DeviceProblem dp, const DeviceProblem dq, const SolverDev sv, int sp, int ntake) {
  if (lm_not_accepted(sv.ctl)) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x;
  if (b < dp.F) camera_reduce_frame<6 * P, CAL>(dp, sv, b);
  else if (b < dp.F + ntake) take_candidate_block(dp, sv, b - dp.F);
  else point_blocks_sweep<CAL, P, GEN>(dq, sv, smem, sp, (int64_t)b - dp.F - ntake);
}

// K7 + K8 without records (see point_step_kernel)
template <bool CAL, int P, bool GEN = false>
__global__ __launch_bounds__(256) void point_step_rc_kernel(const DeviceProblem dp, const SolverDev sv, int sp) {
  if (lm_stopped(sv.ctl)) return;
  constexpr int CD = 6 * P, OP = CAL ? 0 : 9, OX = OP + CD;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const double mc = point_sweep<CAL, P, GEN, 5>(dp, sv, smem, sp, blockIdx.x,
    [&](const ObsOut<CAL, P>& o, int frame, int, double c[5]) {
      const double* yc = sv.step + (size_t)frame * CD;
      double t0 = 0.0, t1 = 0.0;
#pragma unroll
      for (int a = 0; a < CD; ++a) { const double y = yc[a]; t0 += o.J[0][OP + a] * y; t1 += o.J[1][OP + a] * y; }
      if (!CAL) {
        const double* yi = sv.step + (size_t)sv.F * CD;   // step of the (one) intrinsics block: 9 coordinates across its pseudo frames
#pragma unroll
        for (int k = 0; k < 9; ++k) { const double y = yi[k]; t0 += o.J[0][k] * y; t1 += o.J[1][k] * y; }
      }
      c[0] = o.J[0][OX] * t0 + o.J[1][OX] * t1; c[1] = o.J[0][OX + 1] * t0 + o.J[1][OX + 1] * t1; c[2] = o.J[0][OX + 2] * t0 + o.J[1][OX + 2] * t1;   // Jp^T t
      c[3] = t0 * t0 + t1 * t1;
      c[4] = o.r[0] * t0 + o.r[1] * t1;
    },
    [&](int64_t j, const double acc[5]) {
      const double* li = sv.Linv + (size_t)j * 6;
      const double* z = sv.z + (size_t)j * 3;
      const double i00 = li[0], i10 = li[1], i11 = li[2], i20 = li[3], i21 = li[4], i22 = li[5];
      const double u0 = acc[0], u1 = acc[1], u2 = acc[2];
      const double w0 = z[0] - i00 * u0, w1 = z[1] - (i10 * u0 + i11 * u1), w2 = z[2] - (i20 * u0 + i21 * u1 + i22 * u2);
      const double y0 = i00 * w0 + i10 * w1 + i20 * w2, y1 = i11 * w1 + i21 * w2, y2 = i22 * w2;
      double* yp = sv.yp + (size_t)j * 3;
      yp[0] = y0; yp[1] = y1; yp[2] = y2;
      const double* v = sv.V + (size_t)j * 6;   // xx xy xz yy yz zz
      const double* g = sv.gp + (size_t)j * 3;
      const double vy0 = v[0] * y0 + v[1] * y1 + v[2] * y2, vy1 = v[1] * y0 + v[3] * y1 + v[4] * y2, vy2 = v[2] * y0 + v[4] * y1 + v[5] * y2;
      return -acc[4] - (y0 * g[0] + y1 * g[1] + y2 * g[2]) + 0.5 * acc[3] + (y0 * u0 + y1 * u1 + y2 * u2) + 0.5 * (y0 * vy0 + y1 * vy1 + y2 * vy2);
    });
  if (threadIdx.x == 0) sv.partial[blockIdx.x] = mc;
}

// the virtual records of the intrinsics pseudo frames without records, ONE intrinsics block (the shared sess.cam): per point
// Q_j = sum_o Ji_o^T (Jp_o L_j^-T) (9 x 3), cut into the NPF pseudo-frame records of the point's virtual slots (see virtual_records_kernel)
template <int P, bool GEN = false>
__global__ __launch_bounds__(256) void virtual_records_rc_kernel(const DeviceProblem dp, const SolverDev sv, int sp) {
  if (lm_stopped(sv.ctl)) return;
  constexpr int CD = 6 * P, OX = 9 + CD;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  point_sweep<false, P, GEN, 27, 9>(dp, sv, smem, sp, blockIdx.x,
    [&](const ObsOut<false, P>& o, int, int j, double c[27]) {
      double B[2][3];
      jp_linv(&o.J[0][OX], o.K, sv.Linv + (size_t)j * 6, B);
      virtual_record_terms(o, B, c);
    },
    [&](int64_t j, const double acc[27]) { return store_virtual_records<CD>(dp, sv, j, acc); });
}

// The same sweep writing the slots' (factored) P records as well — project_rc_kernel<false, 2, true> and virtual_records_rc_kernel<2> in ONE
// pass over the observations of a problem with ONE shared intrinsics block whose real frames' tiles are all factored (C5's class): the two
// passes evaluate the same observations against the same point factors, and together they are bound by the vector unit they share.
// A wave's LDS: [64][19] staging of q = Jq^T (Jp L^-T) | tau per slot, then 64 group positions; the sums' nine-component passes reuse its front.
constexpr int kFusedStage = 19, kFusedWaveDoubles = 64 * kFusedStage + 32;
template <bool GEN = false>
__global__ __launch_bounds__(256) void virtual_project_rc_kernel(const DeviceProblem dp, const SolverDev sv, int sp) {
  if (lm_stopped(sv.ctl)) return;
  constexpr int P = 2, CD = 12, OX = 9 + CD;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63;
  point_sweep_hooked<false, P, GEN, 27, 9, kFusedWaveDoubles>(dp, sv, smem, sp, blockIdx.x,
    [&](const ObsOut<false, P>& o, int, int j, int64_t s, double* wl, double c[27]) {
      double B[2][3];
      jp_linv(&o.J[0][OX], o.K, sv.Linv + (size_t)j * 6, B);
      virtual_record_terms(o, B, c);
      stage_factored_record(o, B, wl + lane * kFusedStage);   // the slot's factored P record, as project_rc_kernel leaves it
      reinterpret_cast<uint32_t*>(wl + 64 * kFusedStage)[lane] = sv.slot_gpos[s];
    },
    [&](double* wl, int nrec, auto& wave_sync) {
      wave_sync();
      store_factored_groups<true>(sv, wl, kFusedStage, reinterpret_cast<const uint32_t*>(wl + 64 * kFusedStage), nrec, lane);
      wave_sync();
    },
    [&](int64_t j, const double acc[27]) { return store_virtual_records<CD>(dp, sv, j, acc); });
}

}  // namespace

// camera blocks + the accepted candidate's copy over x + point blocks by one launch (linearize_blocks_kernel); *done = false: not for
// this problem (records kept, or nothing to sweep) — the caller launches them one after the other
hipError_t launch_linearize_blocks(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st, bool* done) {
  *done = false;
  if (!sv.slot_xy || !dp.cam_part || dp.M <= 0 || dp.F <= 0) return hipSuccess;
  DeviceProblem dq = dp;
  dq.poses = sv.trial_poses; dq.points = sv.trial_points;
  if (sv.NPF > 0) dq.intr = sv.trial_intr;
  const int64_t nparam = (int64_t)dp.F * dp.P * 6 + 3 * (int64_t)dp.M + (sv.NPF > 0 ? 9 * (int64_t)dp.NI : 0);
  const int ntake = (int)((nparam + 255) / 256), sp = sweep_points(dp.M), npts = (int)((dp.M + 4 * sp - 1) / (4 * sp));
  const size_t lds = (size_t)4 * 64 * 9 * sizeof(double);
  const dim3 grid((unsigned)(dp.F + ntake + npts));
  with_record_variant(dp, sv, [&](auto cal, auto two, auto gen) {
    hipLaunchKernelGGL((linearize_blocks_kernel<decltype(cal)::value, decltype(two)::value ? 2 : 1, decltype(gen)::value>), grid, dim3(256), lds, st, dp, dq, sv, sp, ntake);
  });
  *done = true;
  return hipGetLastError();
}
hipError_t launch_slot_xy(const DeviceProblem& dp, double2* slot_xy, hipStream_t st) {
  if (dp.N > 0) LAUNCH(slot_xy_kernel, nblocks256(dp.N), 256, st, dp, slot_xy);
  return hipSuccess;
}
hipError_t launch_point_blocks(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  if (sv.slot_xy) {   // calibrated: from the observations themselves
    if (dp.M <= 0) return hipSuccess;
    const size_t lds = (size_t)4 * 64 * 9 * sizeof(double);
    const int sp = sweep_points(dp.M), grid = (int)((dp.M + 4 * sp - 1) / (4 * sp));
    with_record_variant(dp, sv, [&](auto cal, auto two, auto gen) {
      hipLaunchKernelGGL((point_blocks_rc_kernel<decltype(cal)::value, decltype(two)::value ? 2 : 1, decltype(gen)::value>), dim3(grid), dim3(256), lds, st, dp, sv, sp);
    });
    return hipGetLastError();
  }
  LAUNCH(point_blocks_kernel, nblocks256(dp.M), 256, st, dp, sv);
  return hipSuccess;
}
template <int CD, int KC>
static hipError_t launch_project_as(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  constexpr int REC = 8 + 2 * KC, OUT = CD * 3;
  const size_t lds = (size_t)4 * (64 * ((REC > OUT ? REC : OUT) | 1) + 32) * sizeof(double);
  const int grid = (int)((dp.N + 256 * kProjectChunks - 1) / (256 * kProjectChunks));
  hipError_t e = allow_dynamic_lds(project_kernel<CD, KC>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((project_kernel<CD, KC>), dim3(grid), dim3(256), lds, st, dp, sv);
  return hipGetLastError();
}
// does launch_project do the virtual records too?  (decided with the plan, SolverDev::fused_sweep: one shared intrinsics block, recomputed
// records, two-pose frames all in factored tiles; RSBA_NO_FUSED_SWEEP=1 keeps the two passes apart)
bool project_covers_virtual_records(const DeviceProblem& dp, const SolverDev& sv) { return sv.fused_sweep != 0 && dp.N > 0; }
hipError_t launch_project(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  if (dp.N == 0) return hipSuccess;
  if (project_covers_virtual_records(dp, sv)) {
    const size_t lds = (size_t)4 * kFusedWaveDoubles * sizeof(double);
    const int sp = sweep_points(dp.M), grid = (int)((dp.M + 4 * sp - 1) / (4 * sp));
    hipError_t e = hipErrorInvalidValue;   // (the fused sweep exists for uncalibrated two-pose problems: what the plan set fused_sweep for)
    with_record_variant(dp, sv, [&](auto cal, auto two, auto gen) {
      if constexpr (!decltype(cal)::value && decltype(two)::value) {
        hipLaunchKernelGGL((virtual_project_rc_kernel<decltype(gen)::value>), dim3(grid), dim3(256), lds, st, dp, sv, sp);
        e = hipGetLastError();
      }
    });
    return e;
  }
  const int KC = dp.K - 3;
  if (sv.slot_xy) {
    const int CD = sv.CD;
    const bool allf = CD == 12 && sv.all_real_factored != 0;
    const size_t lds = (size_t)4 * (64 * (allf ? 19 : ((CD * 3) | 1)) + 32) * sizeof(double);
    const int nch = project_chunks(dp.N), grid = (int)((dp.N + 256 * (int64_t)nch - 1) / (256 * (int64_t)nch));
    with_record_variant(dp, sv, [&](auto cal, auto two, auto gen) {
      constexpr bool CAL = decltype(cal)::value, GEN = decltype(gen)::value;
      constexpr int P = decltype(two)::value ? 2 : 1;
      if constexpr (P == 2) {   // (the all-factored form is a two-pose form)
        if (allf) { hipLaunchKernelGGL((project_rc_kernel<CAL, 2, true, GEN>), dim3(grid), dim3(256), lds, st, dp, sv, nch); return; }
      }
      hipLaunchKernelGGL((project_rc_kernel<CAL, P, false, GEN>), dim3(grid), dim3(256), lds, st, dp, sv, nch);
    });
    return hipGetLastError();
  }
  if (sv.CD == 12 && KC == 12) return launch_project_as<12, 12>(dp, sv, st);
  if (sv.CD == 6 && KC == 6) return launch_project_as<6, 6>(dp, sv, st);
  if (sv.CD == 12 && KC == 21) return launch_project_as<12, 21>(dp, sv, st);
  if (sv.CD == 6 && KC == 15) return launch_project_as<6, 15>(dp, sv, st);
  return hipErrorInvalidValue;
}
hipError_t launch_virtual_records(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  if (sv.NPF == 0) return hipSuccess;
  if (sv.nvgroups == 0) return hipSuccess;
  if (project_covers_virtual_records(dp, sv)) return hipSuccess;   // (launch_project's fused sweep wrote them)
  if (sv.slot_xy) {   // (one intrinsics block: recomputed like the rest)
    const size_t lds = (size_t)4 * 64 * 9 * sizeof(double);   // (nine of the 27 components at a time: point_sweep)
    const int sp = sweep_points(dp.M), grid = (int)((dp.M + 4 * sp - 1) / (4 * sp));
    hipError_t e = hipErrorInvalidValue;   // (intrinsics as a parameter block: an uncalibrated problem)
    with_record_variant(dp, sv, [&](auto cal, auto two, auto gen) {
      if constexpr (!decltype(cal)::value) {
        hipLaunchKernelGGL((virtual_records_rc_kernel<decltype(two)::value ? 2 : 1, decltype(gen)::value>), dim3(grid), dim3(256), lds, st, dp, sv, sp);
        e = hipGetLastError();
      }
    });
    return e;
  }
  if (sv.CD == 12) LAUNCH(virtual_records_kernel<12>, nblocks256(sv.nvgroups), 256, st, dp, sv);
  else LAUNCH(virtual_records_kernel<6>, nblocks256(sv.nvgroups), 256, st, dp, sv);
  return hipSuccess;
}
template <int CD, int KC>
static hipError_t launch_point_step(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  constexpr int REC = 8 + 2 * KC, PITCH = REC | 1;
  const size_t lds = (size_t)4 * (64 * PITCH + 64 * 5) * sizeof(double);
  hipError_t e = allow_dynamic_lds(point_step_kernel<CD, KC>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((point_step_kernel<CD, KC>), dim3(point_step_blocks(dp, sv)), dim3(256), lds, st, dp, sv);
  return hipGetLastError();
}
// point steps y_p and the per-workgroup partials of the model cost change (sv.partial)
hipError_t launch_back_substitute(const DeviceProblem& dp, const SolverDev& sv, hipStream_t st) {
  if (dp.M <= 0) return hipSuccess;
  const int KC = dp.K - 3;
  if (sv.slot_xy) {
    const size_t lds = (size_t)4 * 64 * 5 * sizeof(double);
    const int grid = point_step_blocks(dp, sv);
    const int sp = sweep_points(dp.M);
    with_record_variant(dp, sv, [&](auto cal, auto two, auto gen) {
      hipLaunchKernelGGL((point_step_rc_kernel<decltype(cal)::value, decltype(two)::value ? 2 : 1, decltype(gen)::value>), dim3(grid), dim3(256), lds, st, dp, sv, sp);
    });
    return hipGetLastError();
  }
  if (sv.CD == 12) return KC == 12 ? launch_point_step<12, 12>(dp, sv, st) : launch_point_step<12, 21>(dp, sv, st);
  return KC == 6 ? launch_point_step<6, 6>(dp, sv, st) : launch_point_step<6, 15>(dp, sv, st);
}

}  // namespace rsba
