// K5c of SURVEY §2.1: the reduced camera system (Schur complement) from the points' P-record groups — chunk, premerge and merge
// kernels.  The only kernel file of the normal equations with test hooks (the Schur kernel's ablation branches).
#include <type_traits>

#include "pass_common.hpp"
#include "test_hooks.hpp"

namespace rsba {

namespace {

// ---------------------------------------------------------------------------------------------
// K5c  reduced camera system  S = U + D_c^2 - sum_j (sum_a P_aj)(sum_b P_bj)^T ,  rhs = g_c - sum P z
// Work unit = ENTRY (point j, frame tiles I >= J): the point's P records in the FT frames of I and of J, stacked
// into A_j(I) and A_j(J) (48 x 3 each; a frame that does not see the point contributes zero rows) — exactly the
// (point, tile) GROUPS the projection kernel writes: group g is a [3][48] block of Pm, coordinate-major.
// The tile of the pair is the banded SYRK  S_IJ = sum_j A_j(I) A_j(J)^T  — GEMM-shaped, K = 3 per point — and runs
// on v_mfma_f64_16x16x4_f64 (four points fill three MFMA steps of k = 4), operands loaded from HBM/L2 straight
// into the instruction's register layout: lane (r = lane & 15, g = lane >> 4) holds P[row 16 Ib + r][one
// coordinate of one point] for the three 16-row blocks Ib of each side — in the group layout the sixteen lanes of
// a lane group read ONE aligned 128-B line, a wave instruction four of them (round 2 gathered the same sixteen
// values from slot-major records at a 24-B stride: three to four lines per lane group, and the kernel was bound by
// those gathers as much as by the matrix pipe).  No LDS, no barrier in the loop.
// 16 x 16 operand blocks that are all zero for the four points of an MFMA step — frames of the tile that do not see them —
// are found with one wave vote per block and their MFMAs are not issued (a fifth of them at 1k cameras; 0 * x adds nothing,
// so the result is the same to the bit), and a tile paired with itself only forms the blocks on and below the
// diagonal (nothing reads the upper triangle of a diagonal tile of S).
// One chunk of kSchurChunk entries at a time per workgroup (resident workgroups take chunk after chunk: schur_tile_kernel); its four waves take every fourth entry and keep all
// nine 16x16 blocks (loads run kDepth groups ahead of the MFMAs in a register ring), the four partial tiles meet
// once in LDS.  The fp64 VALU form of this product was bound by LDS operand reads at 2.0 ms per 1k-camera
// iteration.  Chunks write partial tiles; the merge kernel sums them in chunk order (fixed order, no atomics)
// and adds U, D_c^2, g_c.
// ---------------------------------------------------------------------------------------------
typedef double dbl4 __attribute__((ext_vector_type(4)));

// LDS of the loop (bytes): [2 kSchurChunk] uint32 element offsets of the entries' two groups | [kSchurChunk] uint16 block masks | (diagonal
// pairs) [3 kSchurChunk] doubles z.  The four partial tiles of the epilogue reuse it from the start.
constexpr int kSchurOffBytes = 2 * kSchurChunk * 4, kSchurMskBytes = kSchurChunk * 2;
constexpr unsigned kLowerBlocks = 0x1D9;   // bits 3 I + J with J <= I

// One chunk.  DIAG: a tile paired with itself — only the blocks on and below the diagonal are formed, and its entries carry
// the rhs term P z.  The loop is written for the instruction issue port: fp64 MFMAs run on the vector unit's fp64 datapath,
// so every vector / scalar instruction around them is time the matrix pipe idles (round 2's loop spent 6 scalar and 5 vector
// instructions per MFMA on 64-bit gather addresses, tail selects and per-step votes: the pipe was busy 39 % of the time,
// SQ_VALU_MFMA_BUSY_CYCLES).  Here: entry counts are padded to a multiple of 16 with entries that point at an all-zero group
// (no tail selects), the table holds ready element offsets (one 64-bit add per operand, the blocks ride on the load's immediate
// offset), and which of the nine 16 x 16 blocks of a group of four entries have anything to multiply
// is ONE scalar read of host-computed masks; every MFMA sits behind a scalar test of its block's bit (untaken for a full mask, the common case).
//
// FA / FB: the groups of the I / J side are stored FACTORED (solver_state.hpp: kGroupFactored; round 5).  The 48 camera-side rows of
// a two-pose frame tile are, frame by frame, (1 - tau) q | tau q with q = Jq^T Jp L^-T (6 x 3): such a group holds the 24 "sources"
// q per coordinate and the four tau, 640 B instead of 1152, and the operand rows are formed here — one multiply per operand double.
// The rows of a factored side are taken in an order of this kernel's own (the epilogue puts every result where it belongs, so
// nothing outside sees it): blocks 0 and 1 are the pose-0 and pose-1 rows of sources 0..15 — ONE loaded double feeds both — and block
// 2 the rows of sources 16..23 (lanes 0..7 pose 0, lanes 8..15 pose 1).  Per lane and group of four entries: 6 source doubles + 2 tau
// per side instead of 9 operand doubles.  The column scales (Jacobi scales, masks of fixed coordinates) factor out of the sum over
// the points: they are applied once, where the partial tiles are merged.
struct FactoredLane {   // per-lane constants of the row order above
  int main, left, tau_m, tau_l;   // element offsets inside a group (coordinate 0; + 16 / + 8 per coordinate)
  double a0, b0, a1, b1, a2, b2;  // weight of block b = a_b + b_b * tau
};
__device__ __forceinline__ FactoredLane factored_lane(int r, bool lerp_rot) {
  FactoredLane f;
  const int sl = 16 + (r & 7);
  f.main = r; f.left = 48 + (r & 7); f.tau_m = 72 + r / 6; f.tau_l = 72 + sl / 6;
  const bool rot_m = (r % 6) < 3 && !lerp_rot, rot_l = (sl % 6) < 3 && !lerp_rot;   // rotation rows without interpolateRotation: pose 0 carries them whole, pose 1 nothing (cam.h:303-304)
  f.a0 = 1.0; f.b0 = rot_m ? 0.0 : -1.0;
  f.a1 = 0.0; f.b1 = rot_m ? 0.0 : 1.0;
  const bool p1 = (r >> 3) != 0;
  f.a2 = p1 ? 0.0 : 1.0; f.b2 = rot_l ? 0.0 : (p1 ? 1.0 : -1.0);
  return f;
}
// the tile row of operand position (block Ib, row i of the block) of a factored side
__device__ __forceinline__ int factored_row(int Ib, int i) {
  const int s = Ib < 2 ? i : 16 + (i & 7), p = Ib == 0 ? 0 : Ib == 1 ? 1 : (i >> 3);
  return 12 * (s / 6) + 6 * p + s % 6;
}
template <bool F> struct SchurSide;
template <> struct SchurSide<true> { double qm[3], ql[3], tm, tl; };   // [coordinate]
template <> struct SchurSide<false> { double v[3][3]; };               // [coordinate][block]

// The table cells of a chunk that one thread stages (entries tid and tid + 256), loaded ahead of the chunk: the persistent form of the
// kernel issues these loads for its NEXT chunk before the epilogue of the current one, so that the dependent chain chunk -> entry list ->
// operands is not paid chunk by chunk (one workgroup per chunk spent 16 % of a CU slot's time between the end of one chunk and the
// first MFMA of the next: dispatch, four dependent reads; profiles/r05/schur_persistent.txt).
struct ChunkStage { uint32_t ga[2], gb[2]; unsigned pm[2]; int32_t pt[2]; };
static_assert(kSchurChunk == 512, "two table cells per thread");
__device__ __forceinline__ void stage_chunk(const SolverDev& sv, const int4& info, int tid, ChunkStage& st) {
  const int64_t e0 = (int64_t)(((uint64_t)(uint32_t)info.y << 32) | (uint32_t)info.x);
  const int n = info.z;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int k = tid + 256 * u;
    st.ga[u] = st.gb[u] = sv.zero_off;      // (behind the chunk's last entry: the all-zero group behind the last one)
    st.pm[u] = 0; st.pt[u] = 0;
    if (k < n) {
      const uint2 gg = *reinterpret_cast<const uint2*>(sv.ent_groups + 2 * (e0 + k));
      st.ga[u] = gg.x & ~15u; st.gb[u] = gg.y & ~15u;   // (the kind bit: the same for every entry of a tile pair — FA, FB)
      st.pm[u] = sv.ent_mask[e0 + k];     // 16 x 16 blocks of the entry with a frame that sees the point on both sides (host)
      if (info.w & 1) st.pt[u] = sv.ent_pt[e0 + k];
    }
  }
}

// -> the workgroup's next chunk (-1: none), `info` / `st` then hold that chunk's
template <bool DIAG, int kDepth, bool FA, bool FB>
__device__ __forceinline__ int schur_chunk(const SolverDev& sv, const double* __restrict__ Pm, const double* __restrict__ zz, int chunk, int4& info, ChunkStage& st, double* smem, int* s_next,
                                           bool persistent, int xcd, int per_xcd) {
  constexpr int TPITCH = kTile + 1;
  constexpr unsigned kFull = DIAG ? kLowerBlocks : 0x1FFu;
  uint32_t* s_off = reinterpret_cast<uint32_t*>(smem);
  uint16_t* s_msk = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(smem) + kSchurOffBytes);   // [(k & 3) * 128 + (k >> 2)]: the four entries of a wave's group are one 8-byte read
  double* s_z = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + kSchurOffBytes + kSchurMskBytes);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n = info.z, n16 = (n + 15) & ~15;
  long long* tr = sv.schur_trace ? sv.schur_trace + 8 * (size_t)chunk : nullptr;
  if (tr && tid == 0) { tr[0] = blockIdx.x; tr[1] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)); tr[2] = wall_clock64(); tr[6] = n; }   // HW_REG_HW_ID
  __syncthreads();   // (the previous chunk's epilogue has read its partial tiles: the same LDS)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int k = tid + 256 * u;
    if (k < n16) {
      uint32_t ga = st.ga[u], gb = st.gb[u];
      if (kTestHooks && sv.schur_variant == 5 && k < n) { ga = (uint32_t)(k & 63) * kGroupFull; gb = (uint32_t)(64 + (k & 63)) * kGroupFull; }   // ablation: operands out of the caches
      s_off[2 * k] = ga; s_off[2 * k + 1] = gb;
      s_msk[(k & 3) * (kSchurChunk / 4) + (k >> 2)] = (uint16_t)(st.pm[u] & kFull);
      if (DIAG) {
        const int32_t pt = st.pt[u];
#pragma unroll
        for (int c = 0; c < 3; ++c) s_z[3 * k + c] = pt < 0 ? zz[(size_t)(pt & 0x7fffffff) * 3 + c] : 0.0;   // top bit: diagonal entry of the point -> rhs term P z
      }
    }
  }
  __syncthreads();
  if (tr && tid == 0) { tr[3] = wall_clock64(); tr[7] = -clock64(); }
  // the workgroup's next chunk: the next one of its XCD's eighth of the list that nobody has taken (asked for now, needed behind the loop)
  unsigned ticket = 0;
  if (persistent && tid == 0) ticket = __hip_atomic_fetch_add(sv.schur_next + 16 * xcd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // K = 3 per point against 4 per MFMA: four of the wave's entries share three MFMA steps — step t takes coordinate t of the four,
  // lane group g holding entry g of them (one table cell per lane and group of four).  The wave's entries are wave, wave + 4, ..:
  // entry e of its group q is k = wave + 16 q + 4 e.
  const int tab = 8 * (wave + 4 * g), zof = 3 * (wave + 4 * g);
  const FactoredLane fl = factored_lane(r, sv.lerp_rot != 0);
  dbl4 acc[3][3];
#pragma unroll
  for (int I = 0; I < 3; ++I)
#pragma unroll
    for (int J = 0; J < 3; ++J) acc[I][J] = dbl4{0.0, 0.0, 0.0, 0.0};
  double racc[3] = {0.0, 0.0, 0.0};
  struct Group { SchurSide<FA> a; SchurSide<FB> b; double z[3]; };
  Group ring[kDepth];
  const int nq = n16 >> 4;   // groups of four entries per wave
  const char* lds = reinterpret_cast<const char*>(smem);
  auto fetch_side = [&](const double* p, auto& S) {
    using T = typename std::remove_reference<decltype(S)>::type;
    if constexpr (std::is_same<T, SchurSide<true>>::value) {
      S.tm = p[fl.tau_m]; S.tl = p[fl.tau_l];
#pragma unroll
      for (int t = 0; t < 3; ++t) { S.qm[t] = p[fl.main + 16 * t]; S.ql[t] = p[fl.left + 8 * t]; }
    } else {
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int Ib = 0; Ib < 3; ++Ib) S.v[t][Ib] = p[t * kTile + 16 * Ib + r];
    }
  };
  auto fetch = [&](int q, Group& G) {   // (q is wave-uniform; past the end the last group is read again instead of branching)
    const int qq = q < nq ? q : nq - 1;
    const uint2 o = *reinterpret_cast<const uint2*>(lds + tab + 128 * qq);
    fetch_side(Pm + (size_t)o.x, G.a);
    fetch_side(Pm + (size_t)o.y, G.b);
    if (DIAG) {
#pragma unroll
      for (int t = 0; t < 3; ++t) G.z[t] = s_z[zof + t + 48 * qq];
    }
  };
  // the three operand doubles of coordinate t (blocks 0, 1, 2)
  auto operands = [&](const auto& S, int t, double w0, double w1, double w2, double out[3]) {
    using T = typename std::remove_const<typename std::remove_reference<decltype(S)>::type>::type;
    if constexpr (std::is_same<T, SchurSide<true>>::value) { out[0] = S.qm[t] * w0; out[1] = S.qm[t] * w1; out[2] = S.ql[t] * w2; }
    else { out[0] = S.v[t][0]; out[1] = S.v[t][1]; out[2] = S.v[t][2]; }
  };
  unsigned issued = 0;
  if (nq > 0) {
#pragma unroll
    for (int d = 0; d < kDepth; ++d) fetch(d, ring[d]);
    for (int base = 0; base < nq; base += kDepth) {
#pragma unroll
      for (int d = 0; d < kDepth; ++d) {
        if (base + d < nq) {
          // blocks with something to multiply: OR of the four entries' masks, one 8-byte LDS read at a wave-uniform address
          const uint2 m4 = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(s_msk) + 2 * (wave * (kSchurChunk / 4) + 4 * (base + d)));
          unsigned mv = m4.x | m4.y; mv = (mv | (mv >> 16)) & 0x1FFu;
          unsigned pm = (unsigned)__builtin_amdgcn_readfirstlane((int)mv);
          const Group& G = ring[d];
          // the weights of a factored side's three blocks for this lane's entry: a + b tau (1 - tau and tau; 1 and 0 for rotation rows without interpolateRotation)
          double wa0 = 0, wa1 = 0, wa2 = 0, wb0 = 0, wb1 = 0, wb2 = 0;
          if constexpr (FA) { wa0 = __builtin_fma(fl.b0, G.a.tm, fl.a0); wa1 = __builtin_fma(fl.b1, G.a.tm, fl.a1); wa2 = __builtin_fma(fl.b2, G.a.tl, fl.a2); }
          if constexpr (FB) { wb0 = __builtin_fma(fl.b0, G.b.tm, fl.a0); wb1 = __builtin_fma(fl.b1, G.b.tm, fl.a1); wb2 = __builtin_fma(fl.b2, G.b.tl, fl.a2); }
          if (kTestHooks && sv.schur_variant == 4) pm = 0;   // ablation: loads only (instrumented build)
          // ONE code path for full and partial masks: every MFMA behind a scalar test of its block's bit (a second, branch-free path for the
          // full mask made the register allocator keep two homes for the 72 accumulator registers and copy them over around every group:
          // 3.5 v_mov_b64 per MFMA in the round-5 build, 2 in round 4's)
          const unsigned pm27 = pm * 0x40201u;   // the nine bits once per coordinate: every MFMA tests a bit of its own (one s_bitcmp1 + branch; the same bit three times made the compiler keep the tests as lane masks and turn them over on the vector unit)
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            double a[3], b[3];
            operands(G.a, t, wa0, wa1, wa2, a); operands(G.b, t, wb0, wb1, wb2, b);
#pragma unroll
            for (int I = 0; I < 3; ++I)
#pragma unroll
              for (int J = 0; J < 3; ++J)
                if ((!DIAG || J <= I) && __builtin_expect(((pm27 >> (9 * t + 3 * I + J)) & 1u) != 0u, 1)) acc[I][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[I], b[J], acc[I][J], 0, 0, 0);
            if (DIAG) {
#pragma unroll
              for (int I = 0; I < 3; ++I) racc[I] += a[I] * G.z[t];
            }
          }
          issued += 3u * (unsigned)__builtin_popcount(pm);
        }
        fetch(base + d + kDepth, ring[d]);
      }
    }
  }
  if (lane == 0 && issued) atomicAdd(sv.schur_mfma_count, (unsigned long long)issued);   // a statistic (bench.py: issued against useful flops), not a result
  if (wave == 0) {
    const int64_t slots = (int64_t)(gridDim.x >> 3);      // (the first gridDim.x / 8 of every eighth went to the workgroups as they started)
    int64_t i = slots + (unsigned)__builtin_amdgcn_readfirstlane((int)ticket), c = (int64_t)xcd * per_xcd + i;
    int nx = persistent && i < per_xcd && c < sv.nchunk ? (int)c : -1;
    // its own eighth is done: the next chunk of another XCD's (the eighths have the same number of chunks, not of entries).  The other
    // counters are LOOKED at first, all at once — one round trip — and asked only where the look says there is something left: at the end
    // of the launch (and in a launch with a workgroup per chunk) nobody queues seven dependent atomics in front of its last epilogue.
    if (persistent && nx < 0 && per_xcd > slots) {
      const unsigned seen = lane < 8 ? __hip_atomic_load(sv.schur_next + 16 * ((xcd + lane) & 7), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xffffffffu;
      for (int k = 1; k < 8 && nx < 0; ++k) {
        const int y = (xcd + k) & 7;
        const int64_t left = (int64_t)slots + (unsigned)__shfl((int)seen, k, 64);
        if (left >= per_xcd || (int64_t)y * per_xcd + left >= sv.nchunk) continue;
        unsigned t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(sv.schur_next + 16 * y, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        i = slots + (unsigned)__builtin_amdgcn_readfirstlane((int)t);
        c = (int64_t)y * per_xcd + i;
        if (i < per_xcd && c < sv.nchunk) nx = (int)c;
      }
    }
    if (lane == 0) s_next[0] = nx;
  }
  __syncthreads();   // everyone is done with the tables: the same LDS now takes the four partial tiles
  if (tr && tid == 0) { tr[4] = wall_clock64(); tr[7] += clock64(); }   // (shader cycles of the loop: the clock under this load)
  const int next = __builtin_amdgcn_readfirstlane(s_next[0]);
  info = next >= 0 ? sv.chunk_info[next] : int4{0, 0, 0, 0};
  stage_chunk(sv, info, tid, st);   // (in flight under the epilogue; nothing to read behind the last chunk)
  double* buf = smem + wave * (kTile * TPITCH);
  // every result to its place in the tile: a factored side's rows were taken in this kernel's own order (factored_row).  A factored tile
  // paired with itself formed the blocks J <= I of that order: each lands twice, as (row, column) and as (column, row) — the tile comes
  // out symmetric in full (S_ij and S_ji are the same products summed in the same order: the same bits).
#pragma unroll
  for (int I = 0; I < 3; ++I)
#pragma unroll
    for (int J = 0; J < 3; ++J) {
      if (DIAG && FA && J > I) continue;
      const int cb = FB ? factored_row(J, r) : 16 * J + r;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int ra = FA ? factored_row(I, g + 4 * v) : 16 * I + g + 4 * v;
        buf[ra * TPITCH + cb] = acc[I][J][v];
        if (DIAG && FA && J < I) buf[cb * TPITCH + ra] = acc[I][J][v];
      }
    }
  double* rvec = smem + 4 * kTile * TPITCH + wave * kTile;
  if (DIAG) {
#pragma unroll
    for (int I = 0; I < 3; ++I) {
      double x = racc[I];
      x += __shfl_xor(x, 16, 64);
      x += __shfl_xor(x, 32, 64);
      if (lane < 16) rvec[FA ? factored_row(I, lane) : 16 * I + lane] = x;
    }
  }
  __syncthreads();
  double* part = sv.schur_part + (size_t)chunk * (kTile * kTile + kTile);
  for (int e = tid; e < kTile * kTile; e += 256) {
    const int o = (e / kTile) * TPITCH + e % kTile;
    part[e] = (smem[o] + smem[kTile * TPITCH + o]) + (smem[2 * kTile * TPITCH + o] + smem[3 * kTile * TPITCH + o]);
  }
  if (DIAG && tid < kTile) { const double* v = smem + 4 * kTile * TPITCH; part[kTile * kTile + tid] = (v[tid] + v[kTile + tid]) + (v[2 * kTile + tid] + v[3 * kTile + tid]); }
  if (tr && tid == 0) tr[5] = wall_clock64();
  return next;
}

// kDepth = groups of four entries in flight per wave (18 loads each in full form, 16 factored: vmcnt counts to 63).  Two waves per SIMD (two workgroups
// per CU) fit 256 registers with two groups in flight; three need 300.
// PERSISTENT form (the default): 8 x min(an eighth of the chunk list, the XCD's workgroup slots) workgroups; workgroup b starts with chunk
// b >> 3 of eighth b & 7 (workgroups go round-robin over the 8 XCDs, so XCD x walks the x-th eighth of the chunk list in order and its L2
// sees the repeats: consecutive chunks share records — host: chunk numbering) and then takes the eighth's next untaken chunk (a counter per
// eighth) until there is none.  The last workgroup to leave puts the counters back to zero for the next launch.
// RSBA_SCHUR_VARIANT=2: one workgroup per chunk (rounds 2 - 4).
template <int kDepth, int kWavesPerSimd>
__global__ __launch_bounds__(256, kWavesPerSimd) void schur_tile_kernel(const SolverDev sv, const double* __restrict__ Pm, const double* __restrict__ zz, int persistent) {
  if (lm_stopped(sv.ctl)) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int s_next[2];
  const int per_xcd = (sv.nchunk + 7) / 8, xcd = (int)(blockIdx.x & 7);
  int chunk = sv.schur_linear ? (int)blockIdx.x : xcd * per_xcd + (int)(blockIdx.x >> 3);
  if (chunk >= sv.nchunk || (!sv.schur_linear && (int)(blockIdx.x >> 3) >= per_xcd)) chunk = -1;
  int4 info = int4{0, 0, 0, 0};
  ChunkStage st;
  if (chunk >= 0) { info = sv.chunk_info[chunk]; stage_chunk(sv, info, (int)threadIdx.x, st); }
  while (chunk >= 0) {
    const int f = info.w;
    if (f & 1) { if (f & 2) chunk = schur_chunk<true, kDepth, true, true>(sv, Pm, zz, chunk, info, st, smem, s_next, persistent != 0, xcd, per_xcd); else chunk = schur_chunk<true, kDepth, false, false>(sv, Pm, zz, chunk, info, st, smem, s_next, persistent != 0, xcd, per_xcd); }
    else if ((f & 6) == 6) chunk = schur_chunk<false, kDepth, true, true>(sv, Pm, zz, chunk, info, st, smem, s_next, persistent != 0, xcd, per_xcd);
    else if (f & 4) chunk = schur_chunk<false, kDepth, false, true>(sv, Pm, zz, chunk, info, st, smem, s_next, persistent != 0, xcd, per_xcd);        // an intrinsics pseudo tile (full form) against a frame tile
    else if (f & 2) chunk = schur_chunk<false, kDepth, true, false>(sv, Pm, zz, chunk, info, st, smem, s_next, persistent != 0, xcd, per_xcd);        // (a frame tile against a lower-numbered full-form tile: not produced by the plan today)
    else chunk = schur_chunk<false, kDepth, false, false>(sv, Pm, zz, chunk, info, st, smem, s_next, persistent != 0, xcd, per_xcd);
  }
  if (persistent && threadIdx.x == 0 && __hip_atomic_fetch_add(sv.schur_next + 128, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
    for (int e = 0; e < 8; ++e) __hip_atomic_store(sv.schur_next + 16 * e, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(sv.schur_next + 128, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// a group of a very long chunk list: partial[first] = sum of the group's partials, in list order (four running sums, chunk index mod 4).  An element
// per thread, kPremergeSplit workgroups per group (round 6; one workgroup per group walked its 2 352 elements in ten rounds of eight dependent
// loads each: 47 us at 4k cameras for 630 groups)
constexpr int kPremergeSplit = (kTile * kTile + kTile + 255) / 256;
__global__ __launch_bounds__(256) void schur_premerge_kernel(const SolverDev sv) {
  const int g0 = sv.pm_ptr[blockIdx.x], g1 = sv.pm_ptr[blockIdx.x + 1];
  constexpr size_t pstride = kTile * kTile + kTile;
  const int e = blockIdx.y * 256 + threadIdx.x;
  if (e >= (int)pstride) return;
  double ps[4] = {0, 0, 0, 0};
  for (int c = g0; c < g1; c += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) if (c + u < g1) ps[u & 3] += sv.schur_part[(size_t)sv.pm_list[c + u] * pstride + e];
  }
  sv.schur_part[(size_t)sv.pm_list[g0] * pstride + e] = (ps[0] + ps[1]) + (ps[2] + ps[3]);   // (this thread's own element of the group's first partial: read above, nobody else's)
}

// kMergeSplit workgroups per tile pair (an element per thread: with few tile pairs — 100 cameras have 140 — a workgroup walking its
// tile in nine dependent rounds of loads was 25 us of latency): sum the chunk partials in order, add U / D_c^2 / g_c, identity
// padding, and store into the packed tile slot (transposed when the tile ordering swapped the pair).
// The kernel moves 150 MB at 1k cameras and took 57 us: not bandwidth but a CHAIN of dependent reads per thread — pair -> (I, J, chunk range) ->
// chunk ids -> partials -> [is the side factored -> column scale], [U offset -> U], damping -> store: five round trips, hidden only by
// occupancy (profiles/r06/schur_inline_merge.txt: the same chain inside the Schur kernel, where nothing hides it, cost more than this
// launch).  Round 6: ONE 64-byte descriptor per pair (host: solver.hip, tp_desc) holds everything the first two links used to fetch —
// I, J, the packed slot, the flags AND the first eight chunk ids — and whatever depends on the descriptor alone is requested before the
// partials are summed: descriptor -> {partials, U, scales, damping} -> store.  The sums are formed in the order they always were (eight
// interleaved running sums over the chunk list, chunk index mod 8), to the bit.
constexpr int kMergeSplit = kTile * kTile / 256;
static_assert(kMergeSplit * 256 == kTile * kTile, "an element per thread");
struct PairDesc { int32_t I, J, dst, flags, c0, c1, pad0, pad1, head[8]; };   // flags: bit 0 = store transposed, bit 1 / 2 = I / J side factored; [c0, c1) = the pair's range in tp_chunk_list, head = its first eight ids (-1: none)
static_assert(sizeof(PairDesc) == 64, "one 64-byte line per pair");
// sum over the pair's chunk list of element `off` of the partials (tile elements, then the kTile rhs rows)
__device__ __forceinline__ double merge_sum(const SolverDev& sv, const PairDesc& d, int off) {
  constexpr size_t pstride = kTile * kTile + kTile;
  double ps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < 8; ++u) if (d.head[u] >= 0) ps[u] += sv.schur_part[(size_t)d.head[u] * pstride + off];
  for (int ch = d.c0 + 8; ch < d.c1; ch += 8) {   // (a pair with more than eight chunks: up to kMergeGroup heads of pre-reduced groups)
#pragma unroll
    for (int u = 0; u < 8; ++u) if (ch + u < d.c1) ps[u] += sv.schur_part[(size_t)sv.tp_chunk_list[ch + u] * pstride + off];
  }
  return ((ps[0] + ps[1]) + (ps[2] + ps[3])) + ((ps[4] + ps[5]) + (ps[6] + ps[7]));
}
__global__ __launch_bounds__(256) void schur_merge_kernel(const DeviceProblem dp, const SolverDev sv, double inv_radius) {
  const int tp = blockIdx.x, tid = threadIdx.x;
  const PairDesc d = *reinterpret_cast<const PairDesc*>(sv.tp_desc + 16 * (size_t)tp);
  const int I = d.I, J = d.J, CD = sv.CD, FT = sv.FT;
  {
    const int e = blockIdx.y * 256 + tid;
    const int rt = e / kTile, ct = e % kTile;
    const int x = rt / CD, y = ct / CD, r = rt % CD, c = ct % CD;
    const int a = I * FT + x, b = J * FT + y;
    const bool real = a < sv.Fx && b < sv.Fx, on_diag = a == b && r == c;
    // everything that hangs on the descriptor alone, requested BEFORE the partials are waited for (clamped addresses where the value is not used)
    const int64_t add = sv.tp_add[((size_t)tp * FT + x) * FT + y];
    const double sa = (d.flags & 2) ? (a < sv.F ? dp.scale_pose[(size_t)a * CD + r] : 0.0) : 1.0;
    const double sb = (d.flags & 4) ? (b < sv.F ? dp.scale_pose[(size_t)b * CD + c] : 0.0) : 1.0;
    const double lead_a = sv.frame_lead ? sv.frame_lead[a] : (sv.lead != 0 ? 1.0 : 0.0);   // does this rank add the frame's replicated terms (sharded factorisation: the owner of its part)
    const double damp = (real && on_diag) ? sv.diag_c[(size_t)a * CD + r] : 0.0;
    const double u = (real && add >= 0) ? sv.U[add + (size_t)r * CD + c] : 0.0;
    if (sv.ctl) inv_radius = 1.0 / sv.ctl[kCtlRadius];
    double sum = merge_sum(sv, d, e);
    // a factored side left its column scales out of the products (they do not depend on the point): applied here, once per element
    if (d.flags & 2) sum *= sa;
    if (d.flags & 4) sum *= sb;
    const bool lead = lead_a != 0.0;
    double val;
    if (!real) val = (on_diag && lead) ? 1.0 : 0.0;     // padding frames of the last tile
    else {
      val = u - sum;
      if (on_diag && lead) val += damp * inv_radius;
    }
    double* dst = sv.S + (size_t)d.dst * (kTile * kTile);
    if (d.flags & 1) dst[(size_t)ct * kTile + rt] = val; else dst[e] = val;
  }
  if (I == J && blockIdx.y == 0 && tid < kTile) {
    const int a = I * FT + tid / CD;
    const double sa = (d.flags & 2) ? (a < sv.F ? dp.scale_pose[(size_t)I * kTile + tid] : 0.0) : 1.0;
    const double lead_a = sv.frame_lead ? sv.frame_lead[a] : (sv.lead != 0 ? 1.0 : 0.0);
    const double g = a < sv.Fx ? sv.gc[(size_t)I * kTile + tid] : 0.0;
    double sum = merge_sum(sv, d, kTile * kTile + tid);
    if (d.flags & 2) sum *= sa;
    sv.rhs[(size_t)I * kTile + tid] = (a < sv.Fx) ? (lead_a != 0.0 ? g : 0.0) - sum : 0.0;
  }
}

}  // namespace

hipError_t launch_clear_system(const SolverDev& sv, hipStream_t st) {
  return hipMemsetAsync(sv.S, 0, (size_t)sv.nslots * kTile * kTile * sizeof(double), st);
}
hipError_t launch_schur_blocks(const DeviceProblem& dp, const SolverDev& sv, double radius, hipStream_t st) {
  if (sv.nchunk > 0) {
    // dynamic LDS: max(slot table of a chunk, four partial tiles + rhs partials)
    const size_t table = (size_t)kSchurOffBytes + kSchurMskBytes + (size_t)kSchurChunk * 3 * sizeof(double);
    const size_t tiles = (size_t)(4 * kTile * (kTile + 1) + 4 * kTile) * sizeof(double);
    const size_t lds = table > tiles ? table : tiles;
    const int per_xcd = (sv.nchunk + 7) / 8;
    const int persistent = sv.schur_variant != 2 && !sv.schur_linear;
    if (sv.schur_variant == 1) {   // (RSBA_SCHUR_VARIANT=1: three groups in flight, one wave per SIMD; 2: one workgroup per chunk; 4 / 5: ablations of variant 0)
      const dim3 grid(8 * (persistent ? std::min(per_xcd, 32) : per_xcd));
      hipError_t e = allow_dynamic_lds(schur_tile_kernel<3, 1>, lds); if (e != hipSuccess) return e;
      hipLaunchKernelGGL((schur_tile_kernel<3, 1>), grid, dim3(256), lds, st, sv, sv.Pm, sv.z, persistent);
    } else {
      const dim3 grid(8 * (persistent ? std::min(per_xcd, 64) : per_xcd));   // (32 CUs per XCD, two of these workgroups per CU)
      hipError_t e = allow_dynamic_lds(schur_tile_kernel<2, 2>, lds); if (e != hipSuccess) return e;
      hipLaunchKernelGGL((schur_tile_kernel<2, 2>), grid, dim3(256), lds, st, sv, sv.Pm, sv.z, persistent);
    }
    { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; }
  }
  if (sv.npremerge > 0) LAUNCH(schur_premerge_kernel, dim3(sv.npremerge, kPremergeSplit), 256, st, sv);
  LAUNCH(schur_merge_kernel, dim3(sv.ntp, kMergeSplit), 256, st, dp, sv, 1.0 / radius);
  return hipSuccess;
}

}  // namespace rsba
