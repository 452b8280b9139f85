// Tile Cholesky, layer 3: the bodies of the left-looking tile tasks.  The host orders the tile columns by nested dissection
// and lists, per tile of the factor, the finished tiles it pulls its updates from (left-looking: no two workgroups ever
// write the same tile, so no fp atomics and a fixed summation order).  Each task is run by one 256-thread workgroup:
//   UPDATE  partial = sum_{k in chunk} L_ik L_jk^T (+ sum L_jk z_k for a diagonal tile) -> scratch
//   DIAG    S_jj -= updates ; S_jj = L_jj L_jj^T ; W_j = L_jj^-1 ; z_j = W_j (b_j - updates)
//   SUB     S_ij -= updates ; L_ij = S_ij W_j^T
//   BACK    y_j = W_j^T ( z_j - sum_i L_ij^T y_i )
//   FWD2 / FWD2P, ETA   a second right-hand side beside the first (the free interFrameRatio's border column)
// The explicit inverse of the 48x48 diagonal factor turns every triangular solve behind it (dozens of SUB tiles
// per column, the forward and the backward substitution) into a product without a serial chain.
// DAG = true under the persistent drivers (inputs are write-once cells that may not be there yet: chol_cells.hpp), false under
// the level drivers (everything is there).  Same arithmetic in the same order either way: the schedules agree bit for bit.
#pragma once
#include "tile_factor.hpp"

namespace rsba {
namespace {

// the four per-wave partials of one element (tile buffers: stride kBuf; rhs vectors: stride T), in the fixed order of every task
__device__ __forceinline__ double sum4(const double* p, int o, int stride) { return (p[o] + p[stride + o]) + (p[2 * stride + o] + p[3 * stride + o]); }

// ---- MFMA tile products ------------------------------------------------------------------------------------
// C(48x48) += A B^T on v_mfma_f64_16x16x4_f64, operands straight from HBM/L2 into registers — no LDS, no barrier in the accumulation
// loop..  The four waves of the workgroup split K: wave w owns columns [12w, 12w+12) of both operand tiles, lane (r = lane & 15, g = lane >>
// 4) holds columns 12w + 3g + t (t < 3) of rows 16I + r — for MFMA step t that is A[i = r][k = g] and B[k = g][j = r] of the 16x16x4
// product over the k values {12w + 3g' + t}..  Every wave therefore accumulates all nine 16x16 blocks over its quarter of K (27 MFMAs, 64
// cycles each: the fp64 matrix rate of gfx950 equals its vector rate, but the VALU form of this product is bound by LDS operand reads at a
// third of it) and the four partial tiles meet once, in LDS, when the task has gone through all its contributors.
struct Frag {
  double v[3][3];   // [row block I][step t]
  // COHERENT = false: a cached first look (chol_cells.hpp) — the caller checks every double it got
  template <bool DAG, bool COHERENT>
  __device__ __forceinline__ void load(const double* tile, int wave, int lane) {
    const double* p = tile + (lane & 15) * T + 12 * wave + 3 * (lane >> 4);
#pragma unroll
    for (int I = 0; I < 3; ++I)
#pragma unroll
      for (int t = 0; t < 3; ++t) v[I][t] = (DAG && COHERENT) ? ld<true>(p + 16 * I * T + t) : gl(p + 16 * I * T + t);
    if (DAG && COHERENT) CHOL_COUNT(2, 1);
  }
};

struct Acc {
  dbl4 c[3][3];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int I = 0; I < 3; ++I)
#pragma unroll
      for (int J = 0; J < 3; ++J) c[I][J] = dbl4{0.0, 0.0, 0.0, 0.0};
  }
  template <bool LOWER>
  __device__ __forceinline__ void mac(const Frag& a, const Frag& b) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int I = 0; I < 3; ++I)
#pragma unroll
        for (int J = 0; J < 3; ++J)
          if (!LOWER || J <= I) c[I][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.v[I][t], b.v[J][t], c[I][J], 0, 0, 0);
  }
  // this wave's partial tile -> its LDS buffer (row-major, pitch TP)
  __device__ __forceinline__ void spill(double* buf, int lane) const {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int I = 0; I < 3; ++I)
#pragma unroll
      for (int J = 0; J < 3; ++J)
#pragma unroll
        for (int v = 0; v < 4; ++v) buf[(16 * I + g + 4 * v) * TP + 16 * J + r] = c[I][J][v];
  }
};

// sum_{p in [p0,p1)} L_a(p) L_b(p)^T into acc (K-split over the waves), and for DIAG lists sum L_jk z_k into
// bz[I] (this lane's share of rows 16I + r).  DIAG list entries are {slot_jk, tile of z_k}: A = B = L_jk and only
// the lower blocks are formed; SUB entries are {slot_ik, slot_jk}.
template <bool DAG, bool DIAG>
__device__ __forceinline__ void accumulate(const SolverDev& sv, const int32_t* list, int p0, int p1, Acc& acc, double bz[3], int wave, int lane) {
  if (p0 >= p1) return;
  // Operands travel in groups of kGroup contributors, one group ahead of the MFMAs: the HBM round trip of a tile (~2 us) is several times
  // the 0.7 us its product takes.  Loads are issued in straight lines (the tail of the list re-reads its last contributor rather than
  // branch).  The prefetch is speculative and goes through the caches — a tile that has not been produced yet reads as empty cells — and a
  // group is checked when it is about to be multiplied: a wave whose share is incomplete watches it, then reads it again coherently.
  // kGroup stays 1: with two, the operand registers push the persistent kernel past 256 per lane and a CU holds one workgroup instead of
  // two.  The group form stays too: written as plain cur / nxt the kernel comes out with another register allocation (244 VGPRs: none to spare).
  constexpr int kGroup = 1;
  struct Group { Frag a[kGroup], b[kGroup]; double z[kGroup][3]; };
  Group cur, nxt;
  auto fetch_group = [&](Group& g, int p, auto coherent) {   // (coherent: std::true_type — the second look at a group that came in incomplete)
    constexpr bool C = decltype(coherent)::value;
#pragma unroll
    for (int u = 0; u < kGroup; ++u) {
      const int q = min(p + u, p1 - 1);
      g.a[u].template load<DAG, C>(factor_ptr(sv, gl(list + 2 * q)), wave, lane);
      if (!DIAG) g.b[u].template load<DAG, C>(factor_ptr(sv, gl(list + 2 * q + 1)), wave, lane);
      else {
        const double* zk = sv.zv + (size_t)gl(list + 2 * q + 1) * T + 12 * wave + 3 * (lane >> 4);
        g.z[u][0] = ld<DAG>(zk); g.z[u][1] = ld<DAG>(zk + 1); g.z[u][2] = ld<DAG>(zk + 2);
      }
    }
  };
  auto complete = [&](const Group& g) {
    bool ok = true;
#pragma unroll
    for (int u = 0; u < kGroup; ++u) {
#pragma unroll
      for (int I = 0; I < 3; ++I)
#pragma unroll
        for (int t = 0; t < 3; ++t) { ok = ok && filled(g.a[u].v[I][t]); if (!DIAG) ok = ok && filled(g.b[u].v[I][t]); }
      if (DIAG) ok = ok && filled(g.z[u][0]) && filled(g.z[u][1]) && filled(g.z[u][2]);
    }
    return __ballot(!ok) == 0ull;
  };
  auto mac_group = [&](const Group& g, int p) {
#pragma unroll
    for (int u = 0; u < kGroup; ++u) {
      if (p + u < p1) {
        if (DIAG) {
          acc.mac<true>(g.a[u], g.a[u]);
#pragma unroll
          for (int I = 0; I < 3; ++I)
#pragma unroll
            for (int t = 0; t < 3; ++t) bz[I] += g.a[u].v[I][t] * g.z[u][t];
        } else {
          acc.mac<false>(g.a[u], g.b[u]);
        }
      }
    }
  };
  fetch_group(cur, p0, std::false_type{});
  for (int p = p0; p < p1; p += kGroup) {
    const int pn = p + kGroup;
    if (pn < p1) fetch_group(nxt, pn, std::false_type{});
    if (DAG) {
      bool late = false;
      while (!complete(cur)) {
        // the list is in the order the contributors finish: watch the last one of the group
        const int q = min(p + kGroup, p1) - 1;
        watch_cell<DAG>(factor_ptr(sv, gl(list + 2 * q)) + 12 * wave);
        if (!DIAG) watch_cell<DAG>(factor_ptr(sv, gl(list + 2 * q + 1)) + 12 * wave);
        fetch_group(cur, p, std::true_type{});
        late = true;
      }
      if (late) note_late_input();
    }
    mac_group(cur, p);
    if (pn < p1) cur = nxt;
  }
}

// this wave's rhs partials: fold the four lane groups, lanes g == 0 write rows 16I + r of their wave's LDS vector
__device__ __forceinline__ void spill_bz(double bz[3], double* vec, int lane) {
#pragma unroll
  for (int I = 0; I < 3; ++I) {
    double x = bz[I];
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    if (lane < 16) vec[16 * I + lane] = x;
  }
}

template <bool DAG>
__device__ __forceinline__ void task_update(const SolverDev& sv, const CholPlan& pl, int item, double* smem, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  const int32_t* u = pl.upd + 4 * item;
  const int u0 = gl(u), u1 = gl(u + 1), u2 = gl(u + 2), u3 = gl(u + 3);
  const bool diag = u0 == 0;
  Acc acc; acc.clear();
  double bz[3] = {0, 0, 0};
  if (diag) accumulate<DAG, true>(sv, pl.diag_list, u1, u2, acc, bz, wave, lane);
  else accumulate<DAG, false>(sv, pl.sub_list, u1, u2, acc, bz, wave, lane);
  CHOL_STAMP(3);
  acc.spill(smem + wave * kBuf, lane);
  if (diag) spill_bz(bz, smem + kVecOff + wave * T, lane);
  lds_barrier();
  double* out = sv.chol_part + (size_t)u3 * (T * T + T);
  for (int e = tid; e < T * T; e += 256) st<DAG>(out + e, sum4(smem, (e / T) * TP + e % T, kBuf));
  if (diag && tid < T) st<DAG>(out + T * T + tid, sum4(smem + kVecOff, tid, T));
  CHOL_STAMP(4);
}

// the partial tiles (and, WITH_B, rhs partials) of UPDATE tasks, four at a time: each thread re-reads its own nine
// cells of a partial until they are all there
template <bool DAG, bool WITH_B>
__device__ __forceinline__ void subtract_partials(const SolverDev& sv, int part0, int nparts, double sreg[9], double& breg, int tid) {
  for (int c0 = 0; c0 < nparts; c0 += 4) {
    double pv[4][9], pb[4] = {0.0, 0.0, 0.0, 0.0};
    bool late = false;
    for (;;) {
      bool ok = true;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double* part = sv.chol_part + (size_t)(part0 + min(c0 + u, nparts - 1)) * (T * T + T);
#pragma unroll
        for (int q = 0; q < 9; ++q) pv[u][q] = ld<DAG>(part + tid + 256 * q);
        if (WITH_B && tid < T) pb[u] = ld<DAG>(part + T * T + tid);
      }
      if (!DAG) break;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int q = 0; q < 9; ++q) ok = ok && filled(pv[u][q]);
        ok = ok && filled(pb[u]);
      }
      if (ok) break;
      late = true;
      watch_cell<DAG>(sv.chol_part + (size_t)(part0 + min(c0 + 3, nparts - 1)) * (T * T + T) + tid);
    }
    if (late) note_late_input();
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (c0 + u < nparts) {
#pragma unroll
        for (int q = 0; q < 9; ++q) sreg[q] -= pv[u][q];
        breg -= pb[u];
      }
  }
}

// L = X W_j^T for the tile X held in LDS (pitch TP): wave I < 3 forms row block I into c[J] (MFMA result layout: rows
// 16I + (lane >> 4) + 4v, column 16J + (lane & 15)); W is lower triangular, so column block J only needs k < 16 (J + 1).
// W_j comes from the DIAG task of column j: its cells are read until they are all there.
template <bool DAG>
__device__ __forceinline__ void times_inverse_transposed(const SolverDev& sv, int tile_j, const double* X, dbl4 c[3], int wave, int lane) {
  const int I = wave, r = lane & 15, g = lane >> 4;
  const double* Wg = sv.Winv + (size_t)tile_j * (T * T);
  double wv[3][12];   // B operand: W[16J + r][4kk + g]
  {
    bool late = false;
    // The FIRST look at W_j goes through the caches, like the operand tiles of accumulate() (chol_cells.hpp): a dozen SUB tasks of a column
    // read the same 18 KB ("Round 6: what the Cholesky reads from the memory side").  What comes back incomplete — not there
    // yet, or a stale empty — sends the task down the coherent path: watch a cell on the memory side, then read everything from there.
    bool cached_look = DAG;
    for (;;) {
      bool ok = true;
      if (cached_look) {
#pragma unroll
        for (int J = 0; J < 3; ++J)
#pragma unroll
          for (int kk = 0; kk < 4 * (J + 1); ++kk) { wv[J][kk] = gl(Wg + (16 * J + r) * T + 4 * kk + g); ok = ok && filled(wv[J][kk]); }
      } else {
#pragma unroll
        for (int J = 0; J < 3; ++J)
#pragma unroll
          for (int kk = 0; kk < 4 * (J + 1); ++kk) { wv[J][kk] = ld<DAG>(Wg + (16 * J + r) * T + 4 * kk + g); ok = ok && filled(wv[J][kk]); }
        if (DAG) CHOL_COUNT(3, 24);
      }
      if (!DAG || __ballot(!ok) == 0ull) break;
      // A SUB task watches one cell and reads again when it has landed (hundreds of them wait at a time): the last cell of one of the
      // last sixteen rows (all of them land with the last stores) — the SUB tasks of a column spread over sixteen cache lines instead of
      // all polling the one the producer is about to write.
      if (cached_look) { cached_look = false; watch_cell<DAG>(Wg + (T * T - 1) - T * (blockIdx.x & 15)); continue; }
      CHOL_COUNT(4, 24);
      late = true;
      watch_cell<DAG>(Wg + (T * T - 1) - T * (blockIdx.x & 15));
    }
    if (late) note_late_input();
  }
  c[0] = c[1] = c[2] = dbl4{0, 0, 0, 0};
#pragma unroll
  for (int kk = 0; kk < 12; ++kk) {
    const double a = X[(16 * I + r) * TP + 4 * kk + g];
#pragma unroll
    for (int J = 0; J < 3; ++J)
      if (kk < 4 * (J + 1)) c[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wv[J][kk], c[J], 0, 0, 0);
  }
}

// One column block of the same product for the DIAG task that follows column j on the critical chain: rows 16 I .., columns 16 Jc .. of
// L = X W_j^T (the instruction sequence of times_inverse_transposed for that block: same bits), polling only the rows 16 Jc .. of W_j it
// needs.  The rows are being written while it looks: coherent from the start, and the whole row block is read again straight away until
// it is complete — a DIAG task is the next link of the critical chain and only a handful wait for their W at any moment: one memory
// round trip less per level of the elimination tree than watching a cell first.
template <bool DAG>
__device__ __forceinline__ dbl4 times_inverse_block(const SolverDev& sv, int tile_j, const double* X, int Jc, int wave, int lane) {
  const int I = wave, r = lane & 15, g = lane >> 4;
  const double* Wg = sv.Winv + (size_t)tile_j * (T * T) + (16 * Jc + r) * T + g;
  double wv[12];
  bool late = false;
  for (;;) {
    bool ok = true;
#pragma unroll
    for (int kk = 0; kk < 12; ++kk) if (kk < 4 * (Jc + 1)) { wv[kk] = ld<DAG>(Wg + 4 * kk); ok = ok && filled(wv[kk]); }
    if (DAG) CHOL_COUNT(3, 4 * (Jc + 1));
    if (!DAG || __ballot(!ok) == 0ull) break;
    CHOL_COUNT(4, 4 * (Jc + 1));
    late = true;
    __builtin_amdgcn_s_sleep(2);
  }
  if (late) note_late_input();
  dbl4 c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < 12; ++kk)
    if (kk < 4 * (Jc + 1)) c = __builtin_amdgcn_mfma_f64_16x16x4f64(X[(16 * I + r) * TP + 4 * kk + g], wv[kk], c, 0, 0, 0);   // (one accumulator, k ascending: the bits of times_inverse_transposed)
  return c;
}

// DIAG task, early half: the updates formed so far are in acc / bz (K split over the waves), the tile and rhs (less the partial
// tiles) in sreg / breg — D = S_jj - updates (lower triangle) and b = rhs - updates go to LDS.  No barrier at the end.
__device__ __forceinline__ void diag_assemble(double sreg[9], double breg, Acc& acc, double bz[3], double* smem, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  double* D = smem;
  double* vec = smem + kVecOff; double* bvec = smem + kBVec;
  acc.spill(smem + wave * kBuf, lane);
  spill_bz(bz, vec + wave * T, lane);
  lds_barrier();
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int e = tid + 256 * q, r = e / T, c = e % T, o = r * TP + c;
    const double upd = sum4(smem, o, kBuf);
    sreg[q] = (c <= r) ? sreg[q] - upd : 0.0;
  }
  if (tid < T) bvec[tid] = breg - sum4(vec, tid, T);
  lds_barrier();
#pragma unroll
  for (int q = 0; q < 9; ++q) { const int e = tid + 256 * q; D[(e / T) * TP + e % T] = sreg[q]; }
}

// DIAG task, the serial half: D (LDS, complete) = L_jj L_jj^T, W_j = L_jj^-1, z_j = W_j b
template <bool DAG>
__device__ __forceinline__ void diag_factor(const SolverDev& sv, int tile_j, double* smem, int tid) {
  double* D = smem; double* Wl = smem + kBuf;
  const double* bvec = smem + kBVec;
  arm_pivot_messages(smem, tid);   // (rows of buffers 2 and 3 that held X / L of the last contributor until the barrier in front of this call)
  lds_barrier();
  CHOL_STAMP(4);
  // L_jj itself is never formed: everything downstream uses W_j
  const bool ok = factor_invert_tile<false, DAG>(D, Wl, smem + 2 * kBuf, smem + 3 * kBuf, tid, nullptr, sv.Winv + (size_t)tile_j * (T * T));   // (W leaves by row blocks from inside)
  if (tid == 0 && !ok) atomicExch(sv.chol_fail, 1);
  CHOL_STAMP(6);
  if (tid < 4 * T) {   // z_j = W b: four lanes per row, twelve columns each (the next DIAG task of the chain waits for it right behind the last rows of W)
    const int row = tid >> 2, q = tid & 3;
    double s0 = 0.0;
#pragma unroll
    for (int m = 0; m < T / 4; ++m) { const int c = (T / 4) * q + m; if (c <= row) s0 += Wl[row * TP + c] * bvec[c]; }
    s0 += __shfl_xor(s0, 1, 64);
    s0 += __shfl_xor(s0, 2, 64);
    if (q == 0) st<DAG>(sv.zv + (size_t)tile_j * T + row, s0);
  }
}

template <bool DAG>
__device__ __forceinline__ void task_diag(const SolverDev& sv, const CholPlan& pl, int b, double* smem, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  const int32_t* info = pl.diag_info + 4 * b;
  const int slot_jj = gl(info), tile_j = gl(info + 1), part0 = gl(info + 2), nparts = gl(info + 3);
  // The last contributor k* (the column that finishes one level before this one) is formed HERE from W_k* instead of being
  // read back from the SUB task of tile (j, k*) (item fs).
  const int fs = gl(pl.diag_fuse + b);
  const int p0 = gl(pl.diag_own + b), p1 = gl(pl.diag_ptr + b + 1) - (fs >= 0 ? 1 : 0);   // the owner's share of the contributor list
  double* XB = smem + kXBuf; double* LB = smem + kLBuf;
  // X = S_jk* - (older updates) comes from the SUB task of that tile, which publishes it before it starts waiting for W_k*:
  // requested here, looked at when it is needed
  double xreg[9];
  const double* xs = sv.Xpub + (size_t)b * (T * T);
  if (fs >= 0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) xreg[q] = ld<DAG>(xs + tid + 256 * q);
  }
  // the tile itself (left by the Schur kernels before this launch) travels while the updates are formed
  double sreg[9];
  const double* src = tile_ptr(sv, slot_jj);
#pragma unroll
  for (int q = 0; q < 9; ++q) sreg[q] = gl(src + tid + 256 * q);
  double breg = tid < T ? gl(sv.rhs + (size_t)tile_j * T + tid) : 0.0;
  // the early part of a long contributor list arrives pre-reduced (UPDATE tasks), well before the owner's own share
  subtract_partials<DAG, true>(sv, part0, nparts, sreg, breg, tid);
  Acc acc; acc.clear();
  double bz[3] = {0, 0, 0};
  accumulate<DAG, true>(sv, pl.diag_list, p0, p1, acc, bz, wave, lane);
  CHOL_STAMP(3);
  diag_assemble(sreg, breg, acc, bz, smem, tid);   // everything that does not need column k*: off the critical path
  if (fs >= 0) {
    const int tile_k = gl(pl.sub_col + fs);
    double* D = smem;
    double* bvec = smem + kBVec; double* zs = smem + kZVec;
    {
      bool late = false;
      for (;;) {
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 9; ++q) ok = ok && filled(xreg[q]);
        if (!DAG || ok) break;
        late = true;
        watch_cell<DAG>(xs + tid + 256 * 8);
#pragma unroll
        for (int q = 0; q < 9; ++q) xreg[q] = ld<DAG>(xs + tid + 256 * q);
      }
      if (late) note_late_input();
#pragma unroll
      for (int q = 0; q < 9; ++q) { const int e = tid + 256 * q; XB[(e / T) * TP + e % T] = xreg[q]; }
    }
    lds_barrier();   // X and D are in LDS
    // W_k* arrives by row blocks (factor_invert_tile): column block Jc of L = X W^T needs rows 16 Jc .. of W only, and D -= L L^T is a sum
    // over the column blocks of L — so each stage runs as its rows land, under the factorisation that produces the next ones, and only
    // the last stage (a third of both products) is left on the chain.  Stage Jc: waves 0-2 form their row block of L(:, Jc), barrier,
    // the six lower blocks of D take the rank-16 update (dealt to the four waves).  z_k* is stored behind the last rows of W.
#pragma unroll
    for (int Jc = 0; Jc < 3; ++Jc) {
      if (wave < 3) {
        const int r = lane & 15, g = lane >> 4;
        const dbl4 cj = times_inverse_block<DAG>(sv, tile_k, XB, Jc, wave, lane);
#pragma unroll
        for (int v = 0; v < 4; ++v) LB[(16 * wave + g + 4 * v) * TP + 16 * Jc + r] = cj[v];
      } else if (Jc == 2 && lane < T) {
        const double* zk = sv.zv + (size_t)tile_k * T + lane;
        double z = ld<DAG>(zk);
        while (DAG && !filled(z)) { __builtin_amdgcn_s_sleep(2); z = ld<DAG>(zk); }
        zs[lane] = z;
      }
      if (Jc == 2 && DAG && threadIdx.x == 0 && s_trace_slot) s_trace_slot[5] = wall_clock64();   // trace: the last rows of W_k* are in registers
      lds_barrier();
      const int mi = lane & 15, mg = lane >> 4;
#pragma unroll
      for (int blk = 0; blk < 6; ++blk) {
        if ((blk & 3) != wave) continue;
        const int I = blk < 1 ? 0 : (blk < 3 ? 1 : 2), J = blk - (I * (I + 1)) / 2;
        dbl4 a4 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 4 * Jc; kk < 4 * Jc + 4; ++kk)
          a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(LB[(16 * I + mi) * TP + 4 * kk + mg], LB[(16 * J + mi) * TP + 4 * kk + mg], a4, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = 16 * I + mg + 4 * v, c = 16 * J + mi;
          if (c <= r) D[r * TP + c] -= a4[v];
        }
      }
    }
    // b -= L z_k* by two lanes per row of waves 2 and 3, which only have one block each
    if (tid >= 128 && tid < 128 + 2 * T) {
      const int row = (tid - 128) >> 1, h = tid & 1;
      double s0 = 0.0;
#pragma unroll
      for (int m = 0; m < T / 2; ++m) s0 += LB[row * TP + (T / 2) * h + m] * zs[(T / 2) * h + m];
      s0 += __shfl_xor(s0, 1, 64);
      if (h == 0) bvec[row] -= s0;
    }
  }
  lds_barrier();
  diag_factor<DAG>(sv, tile_j, smem, tid);
}

template <bool DAG>
__device__ __forceinline__ void task_sub(const SolverDev& sv, const CholPlan& pl, int b, double* smem, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  double* X = smem;
  const int32_t* info = pl.sub_info + 4 * b;
  const int slot_ij = gl(info), part0 = gl(info + 2), nparts = gl(info + 3), tile_j = gl(pl.sub_col + b);
  const int p0 = gl(pl.sub_own + b), p1 = gl(pl.sub_ptr + b + 1);
  double sreg[9];
  const double* src = tile_ptr(sv, slot_ij);
#pragma unroll
  for (int q = 0; q < 9; ++q) sreg[q] = gl(src + tid + 256 * q);
  { double none = 0.0; subtract_partials<DAG, false>(sv, part0, nparts, sreg, none, tid); }
  Acc acc; acc.clear();
  double bz[3] = {0, 0, 0};
  accumulate<DAG, false>(sv, pl.sub_list, p0, p1, acc, bz, wave, lane);
  CHOL_STAMP(3);
  acc.spill(smem + wave * kBuf, lane);
  lds_barrier();
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int e = tid + 256 * q, o = (e / T) * TP + e % T;
    sreg[q] -= sum4(smem, o, kBuf);
  }
  lds_barrier();
#pragma unroll
  for (int q = 0; q < 9; ++q) { const int e = tid + 256 * q; X[(e / T) * TP + e % T] = sreg[q]; }
  if (const int pub = gl(pl.sub_pub + b); pub >= 0) {   // the DIAG task of row i multiplies this by W_j itself (look-ahead on the critical path)
    double* xp = sv.Xpub + (size_t)pub * (T * T);
#pragma unroll
    for (int q = 0; q < 9; ++q) st<DAG>(xp + tid + 256 * q, sreg[q]);
  }
  CHOL_STAMP(4);
  lds_barrier();
  CHOL_STAMP(5);
  // L_ij = X W_j^T
  if (wave < 3) {
    const int I = wave, r = lane & 15, g = lane >> 4;
    double* out = factor_ptr(sv, slot_ij);
    dbl4 c[3];
    times_inverse_transposed<DAG>(sv, tile_j, X, c, wave, lane);
#pragma unroll
    for (int J = 0; J < 3; ++J)
#pragma unroll
      for (int v = 0; v < 4; ++v) st<DAG>(out + (16 * I + g + 4 * v) * T + 16 * J + r, c[J][v]);
  }
  CHOL_STAMP(6);
}

template <bool DAG>
__device__ __forceinline__ void task_back(const SolverDev& sv, const CholPlan& pl, int b, double* smem, int tid) {
  double* part = smem;            // [10][T]
  double* tvec = smem + 10 * T;   // [T]
  const int32_t* list = pl.back_list;
  const int c2 = tid % 24, rg = tid / 24;   // column pair, row group (rg < 10 for tid < 240)
  const int tile_j = gl(pl.back_info + 2 * b + 1);
  const int p0 = gl(pl.back_ptr + b), p1 = gl(pl.back_ptr + b + 1);
  const bool worker = rg < 10;
  // rows of a 48 x 48 tile handled by this thread: rg, rg + 10, .. ; columns 2 c2, 2 c2 + 1 (threads without work
  // read nothing).  Whether the cells were all there is asked where the values are USED (gathered_ok), never next to
  // the loads: a test there would make the compiler wait for them on the spot and undo the prefetch.
  auto gather = [&](const double* tile, const double* y, double2 v[5], double yy[5], bool LDSY) {
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      const int r = rg + 10 * u;
      if (worker && r < T) {
        const double* q = tile + (size_t)r * T + 2 * c2;
        v[u] = make_double2(ld<DAG>(q), ld<DAG>(q + 1));
        yy[u] = LDSY ? y[r] : ld<DAG>(y + r);
      } else { v[u] = make_double2(0.0, 0.0); yy[u] = 0.0; }
    }
  };
  auto gathered_ok = [&](const double2 v[5], const double yy[5]) {
    bool ok = true;
#pragma unroll
    for (int u = 0; u < 5; ++u) ok = ok && filled(v[u].x) && filled(v[u].y) && filled(yy[u]);
    return ok;
  };
  // W_j and z_j (from the DIAG task of this column, long finished as a rule) are requested NOW and looked at behind the y_i the
  // task really waits for: their round trips would otherwise sit between the last y_i and the store of y_j, on the chain of the backward solve
  const double* Wg = sv.Winv + (size_t)tile_j * (T * T);
  double2 wpre[5];
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const int r = rg + 10 * u;
    if (worker && r < T) { const double* q = Wg + (size_t)r * T + 2 * c2; wpre[u] = make_double2(ld<DAG>(q), ld<DAG>(q + 1)); } else wpre[u] = make_double2(0.0, 0.0);
  }
  double zpre = tid < T ? ld<DAG>(sv.zv + (size_t)tile_j * T + tid) : 0.0;
  double z2pre = (tid < T && sv.zv2) ? ld<DAG>(sv.zv2 + (size_t)tile_j * T + tid) : 0.0;
  double s0 = 0.0, s1 = 0.0;
  if (p0 < p1) {
    // L_ij (forward phase) is long finished; y_i is what the task waits for.  The host lists the tiles of the
    // column bottom-up, the order in which the y_i become available; loads run one tile ahead (a group of one, as in
    // accumulate(), and kept in that form for the same reason) and a thread whose cells of a tile are not all there yet watches
    // its y, then reads the tile again.
    constexpr int kGroup = 1;
    struct Group { double2 v[kGroup][5]; double yy[kGroup][5]; };
    Group cur, nxt;
    auto fetch_group = [&](Group& g, int p) {
#pragma unroll
      for (int u = 0; u < kGroup; ++u) { const int q = min(p + u, p1 - 1); gather(factor_ptr(sv, gl(list + 2 * q)), sv.yv + (size_t)gl(list + 2 * q + 1) * T, g.v[u], g.yy[u], false); }
    };
    auto group_ok = [&](const Group& g) {
      bool ok = true;
#pragma unroll
      for (int u = 0; u < kGroup; ++u) ok = ok && gathered_ok(g.v[u], g.yy[u]);
      return ok;
    };
    auto mac_group = [&](const Group& g, int p) {
#pragma unroll
      for (int u = 0; u < kGroup; ++u)
        if (p + u < p1) {
#pragma unroll
          for (int k = 0; k < 5; ++k) { s0 += g.v[u][k].x * g.yy[u][k]; s1 += g.v[u][k].y * g.yy[u][k]; }
        }
    };
    fetch_group(cur, p0);
    for (int p = p0; p < p1; p += kGroup) {
      const int pn = p + kGroup;
      if (pn < p1) fetch_group(nxt, pn);
      if (DAG) {
        bool late = false;
        while (!group_ok(cur)) {
          watch_cell<DAG>(sv.yv + (size_t)gl(list + 2 * (min(p + kGroup, p1) - 1) + 1) * T);   // y of the last tile of the group
          fetch_group(cur, p);
          late = true;
        }
        if (late) note_late_input();
      }
      mac_group(cur, p);
      if (pn < p1) cur = nxt;
    }
  }
  if (worker) { part[rg * T + 2 * c2] = s0; part[rg * T + 2 * c2 + 1] = s1; }
  lds_barrier();
  CHOL_STAMP(3);
  if (tid < T) {
    double t = zpre;   // z_j, from the DIAG task of this column
    while (DAG && !filled(t)) { __builtin_amdgcn_s_sleep(8); t = ld<DAG>(sv.zv + (size_t)tile_j * T + tid); }
    if (sv.zv2) {   // two right-hand sides through one backward solve: L^T y = z - (s eta) z2 (the ETA task leaves s eta in its cell)
#pragma clang fp contract(off)
      double c = ld<DAG>(sv.ceta), z2 = z2pre;
      while (DAG && !filled(c)) { __builtin_amdgcn_s_sleep(8); c = ld<DAG>(sv.ceta); }
      while (DAG && !filled(z2)) { __builtin_amdgcn_s_sleep(8); z2 = ld<DAG>(sv.zv2 + (size_t)tile_j * T + tid); }
      t = t - c * z2;
    }
#pragma unroll
    for (int g = 0; g < 10; ++g) t -= part[g * T + tid];
    tvec[tid] = t;
  }
  lds_barrier();
  // y = W^T t
  {
    double2 v[5]; double yy[5];
#pragma unroll
    for (int u = 0; u < 5; ++u) { const int r = rg + 10 * u; v[u] = wpre[u]; yy[u] = (worker && r < T) ? tvec[r] : 0.0; }
    while (DAG && !gathered_ok(v, yy)) { __builtin_amdgcn_s_sleep(8); gather(Wg, tvec, v, yy, true); }
    s0 = 0.0; s1 = 0.0;
#pragma unroll
    for (int u = 0; u < 5; ++u) { s0 += v[u].x * yy[u]; s1 += v[u].y * yy[u]; }
  }
  lds_barrier();
  if (worker) { part[rg * T + 2 * c2] = s0; part[rg * T + 2 * c2 + 1] = s1; }
  lds_barrier();
  if (tid < T) {
    double y = 0.0;
#pragma unroll
    for (int g = 0; g < 10; ++g) y += part[g * T + tid];
    st<DAG>(sv.yv + (size_t)tile_j * T + tid, y);
  }
  CHOL_STAMP(4);
}

// ---- a second right-hand side ------------------------------------------------------------------------------------------------
// z2_j = W_j (b2_j - minus_j - sum_{p in [p0, p1)} L_jk z2_k) over the contributors p of DIAG item d's list: thread (row r = tid % T, column
// group cg = tid / T < 5) takes ten columns of its row of every tile — 240 threads, ten loads each per contributor, the next contributor's
// tile travelling while this one is multiplied.  Everything it reads is a write-once cell: beside a running factorisation (FWD2 tasks of
// the persistent driver) the rows of L_jk, z2_k and W_j are polled; behind a finished one (chol_solve_kernel, the level schedule) they are
// simply there.  minus (may be null): what other ranks' columns contribute to this column (sharded factorisation: summed by the exchange).
// partial_out (FWD2P, may be null): only the sum over this rank's part is formed, and left there.
template <bool DAG>
__device__ __forceinline__ void task_forward(const SolverDev& sv, const CholPlan& pl, int d, int p0, int p1, const double* __restrict__ b2, const double* __restrict__ minus, double* z2,
                                             double* smem, int tid, double* partial_out = nullptr) {
  constexpr int CG = 10;        // columns per thread
  double* zb = smem;            // [T] z2 of the contributor being multiplied
  double* sp = smem + T;        // [5][T] partial sums
  double* tv = smem + 6 * T;    // [T]
  const int cg = tid / T, r = tid % T, c0 = CG * cg;
  const bool worker = cg < 5;
  const int tile_j = gl(pl.diag_info + 4 * d + 1);
  auto load_row = [&](const double* tile, double v[CG]) {
#pragma unroll
    for (int m = 0; m < CG; ++m) v[m] = (worker && c0 + m < T) ? ld<DAG>(tile + (size_t)r * T + c0 + m) : 0.0;
  };
  auto row_ok = [&](const double v[CG]) { bool ok = true;
#pragma unroll
    for (int m = 0; m < CG; ++m) ok = ok && filled(v[m]);
    return ok; };
  double s = 0.0;
  double cur[CG], nxt[CG];
  if (p0 < p1) load_row(factor_ptr(sv, gl(pl.diag_list + 2 * p0)), cur);
  for (int p = p0; p < p1; ++p) {
    if (p + 1 < p1) load_row(factor_ptr(sv, gl(pl.diag_list + 2 * (p + 1))), nxt);
    if (tid < T) {
      const double* zk = z2 + (size_t)gl(pl.diag_list + 2 * p + 1) * T + tid;
      double z = ld<DAG>(zk);
      while (DAG && !filled(z)) { __builtin_amdgcn_s_sleep(2); z = ld<DAG>(zk); }
      zb[tid] = z;
    }
    while (DAG && !row_ok(cur)) { __builtin_amdgcn_s_sleep(2); load_row(factor_ptr(sv, gl(pl.diag_list + 2 * p)), cur); }
    lds_barrier();
#pragma unroll
    for (int m = 0; m < CG; ++m) if (worker && c0 + m < T) s += cur[m] * zb[c0 + m];
    lds_barrier();
#pragma unroll
    for (int m = 0; m < CG; ++m) cur[m] = nxt[m];
  }
  if (partial_out) {   // FWD2P: only the sum over this rank's part — it travels (plain stores: read behind this launch)
    if (worker) sp[cg * T + r] = s;
    lds_barrier();
    if (tid < T) { double t = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) t += sp[k * T + r];
      partial_out[r] = t; }
    return;
  }
  // W_j: requested before the sums meet (the DIAG task of this column has just produced it, or is about to)
  const double* Wg = sv.Winv + (size_t)tile_j * (T * T);
  double w[CG];
  load_row(Wg, w);
  if (worker) sp[cg * T + r] = s;
  lds_barrier();
  if (tid < T) {
    double t = gl(b2 + (size_t)tile_j * T + r);
    if (minus) t -= gl(minus + r);
#pragma unroll
    for (int k = 0; k < 5; ++k) t -= sp[k * T + r];
    tv[r] = t;
  }
  while (DAG && !row_ok(w)) { __builtin_amdgcn_s_sleep(2); load_row(Wg, w); }
  lds_barrier();
  s = 0.0;
#pragma unroll
  for (int m = 0; m < CG; ++m) if (worker && c0 + m < T && c0 + m <= r) s += w[m] * tv[c0 + m];   // (W is lower triangular: exact zeros right of the diagonal)
  lds_barrier();
  if (worker) sp[cg * T + r] = s;
  lds_barrier();
  if (tid < T) {
    double z = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) z += sp[k * T + r];
    st<DAG>(z2 + (size_t)tile_j * T + r, z);
  }
}

// The ratio's step from the two forward solves (solver_state.hpp): d1 = z2.z, d2 = z2.z2 over the columns [t0, t1) of this plan (+ what
// `extra` carries: sharded factorisation — the other ranks' parts, summed by the exchange), eta = (g_s - s d1) / (h_s + D - s^2 d2); s eta goes to
// the cell the BACK tasks wait for.  One workgroup, sums in a fixed order.
template <bool DAG>
__device__ __forceinline__ void task_eta(const SolverDev& sv, const CholPlan& pl, double* smem, int tid) {
#pragma clang fp contract(off)
  double a = 0.0, b = 0.0;
  for (int64_t t = tid; t < sv.npad; t += 256) {
    if (pl.eta_tiles && !gl(pl.eta_tiles + t / T)) continue;   // (a sharded factorisation: this launch's columns only)
    double z = ld<DAG>(sv.zv + t), w = ld<DAG>(sv.zv2 + t);
    while (DAG && !(filled(z) && filled(w))) { __builtin_amdgcn_s_sleep(8); z = ld<DAG>(sv.zv + t); w = ld<DAG>(sv.zv2 + t); }
    a += w * z; b += w * w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
  if ((tid & 63) == 0) { smem[tid >> 6] = a; smem[4 + (tid >> 6)] = b; }
  lds_barrier();
  if (tid == 0) {
    double d1 = sum4(smem, 0, 1), d2 = sum4(smem, 4, 1);
    if (pl.eta_partial) { pl.eta_partial[0] = d1; pl.eta_partial[1] = d2; return; }   // launch A of a sharded factorisation: this rank's part, to be summed by the exchange
    if (pl.eta_extra) { d1 += gl(pl.eta_extra); d2 += gl(pl.eta_extra + 1); }        // launch B: the separators' share (every rank alike) + all parts'
    const double sc = sv.rt[kRtScale];
    const double eta = (sv.rt[kRtGs] - sc * d1) / (sv.rt[kRtDiagTerm] - sc * sc * d2);
    const double c = sc * eta;
    sv.rt[kRtDot1] = d1; sv.rt[kRtDot2] = d2; sv.rt[kRtEta] = eta; sv.rt[kRtC] = c;
    st<DAG>(sv.ceta, c);
  }
}

template <bool DAG>
__device__ __forceinline__ void run_task(const SolverDev& sv, const CholPlan& pl, int kind, int item, double* smem, int tid) {
  switch (kind) {
    case kTaskUpdate: task_update<DAG>(sv, pl, item, smem, tid); break;
    case kTaskDiag: task_diag<DAG>(sv, pl, item, smem, tid); break;
    case kTaskSub: task_sub<DAG>(sv, pl, item, smem, tid); break;
    case kTaskFwd2: { const int tr = gl(pl.diag_toprow + item);
      task_forward<DAG>(sv, pl, item, gl(pl.fwd_range + 2 * item), gl(pl.fwd_range + 2 * item + 1), sv.border2, (pl.fwd2_minus && tr >= 0) ? pl.fwd2_minus + (size_t)tr * T : nullptr, sv.zv2, smem, tid); } break;
    case kTaskFwd2P: task_forward<DAG>(sv, pl, item, gl(pl.fwd_range + 2 * item), gl(pl.fwd_range + 2 * item + 1), sv.border2, nullptr, sv.zv2, smem, tid, pl.fwd2_partial + (size_t)gl(pl.diag_toprow + item) * T); break;
    case kTaskEta: task_eta<DAG>(sv, pl, smem, tid); break;
    default: task_back<DAG>(sv, pl, item, smem, tid); break;
  }
}

}  // namespace
}  // namespace rsba
