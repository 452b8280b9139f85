// Tile Cholesky, layer 2: W = chol(D)^-1 of one 48 x 48 tile in LDS by one 256-thread workgroup, on the matrix pipe — the serial
// core of the whole solve (the chain of diagonal tiles) — and the LDS map of a task, which the factorisation's scratch shares.
// History and measurements: DESIGN.md §3, "The Cholesky: round 2 … and round 3"; tools/tile_factor_bench.hip times and checks it outside the solver.
#pragma once
#include "chol_cells.hpp"

namespace rsba {
namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f64_16x16x4_f64: lane (c, g) = (lane & 15, lane >> 4) holds rows g + 4v (v < 4) of column c (measured, tools/mfma_f64_check.hip)

// LDS map of a task (doubles): four tile buffers (pitch TP), then eight vectors of T
constexpr int kBuf = T * TP;
constexpr int kVecOff = 4 * kBuf;            // [4][T] per-wave rhs partials
constexpr int kBVec = kVecOff + 4 * T;       // [T] b of a DIAG task: rhs less all updates
constexpr int kSpareVec = kVecOff + 5 * T;   // [2][T] idle in the library (tools/tile_factor_bench.hip keeps its baseline's reciprocal diagonal in the first)
constexpr int kZVec = kVecOff + 7 * T;       // [T] z of a DIAG task's last contributor
constexpr int kCholLds = kVecOff + 8 * T;    // 78 KB: two workgroups fit a CU
// Nothing else is allocated: what a DIAG task needs beyond the four tile buffers lives in parts of them that are idle at the time —
//   X (tile (j, k*) less its updates) in buffer 1 and L = X W^T in buffer 3 while the last contributor is applied (the
//   factorisation, which uses buffers 1 .. 3 as W, T and L-panel scratch, has not started), and
//   the pivot messages between the two waves of the tile factorisation in rows 0 .. 15 of buffers 2 and 3, which the
//   factorisation never touches (its scratch blocks sit in rows 16 .. 47): pivots 0 .. 7 in buffer 2, 8 .. 15 in buffer 3.
constexpr int kXBuf = 1 * kBuf, kLBuf = 3 * kBuf;
constexpr int kMsg = 64;                     // one pivot's message: a double per lane
__device__ __forceinline__ constexpr int msg_off(int jj) { return (jj < 8 ? 2 * kBuf : 3 * kBuf) + (jj & 7) * kMsg; }
static_assert(8 * kMsg <= 16 * TP, "the messages of eight pivots must fit the sixteen idle rows of a scratch tile");

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// ---- one 16 x 16 diagonal block: LDL^T by rank-1 MFMAs, on two waves ------------------------------------------------
// The block lives in the accumulator layout, kept in full (symmetric), so row jj — the multipliers of pivot jj, by symmetry — already sits
// in lane group g = jj % 4, register jj / 4, one column per lane: exactly where the instruction wants the k = g slice of its A and B
// operands..  D -= (row / d) row^T is then a select and a multiply per lane, no data movement at all..  The same multipliers applied to an
// identity give E = L'^-1 of the unit-lower LDL^T factor, and W = chol(D)^-1 = diag(d)^-1/2 E: no square root on the chain, and the factor
// itself is never formed (nothing downstream reads it). fp64 MFMAs and fp64 vector instructions do not overlap on this chip
// (tools/ldl_probe.hip: their times add up), so whatever one wave does per pivot is serial..  The step is therefore split over TWO waves (two
// SIMDs): the first eliminates and posts each pivot's multipliers and the pivot itself in LDS (ldl16_eliminate); the second picks a message
// up as soon as it is complete (the data is its own flag, as with the write-once cells in HBM) and applies it to the identity
// (ldl16_follow_rows)..  The messages must be armed (armed = the empty pattern of chol_cells.hpp) before the workgroup barrier that precedes
// the step.
__device__ __forceinline__ void arm_pivot_messages(double* smem, int tid) {
  for (int e = tid; e < 16 * kMsg; e += 256) smem[msg_off(e / kMsg) + e % kMsg] = __longlong_as_double(-1ll);
}
// one wave re-arms the messages of pivots [j0, j1) (between two diagonal blocks, while it has nothing else to do)
__device__ __forceinline__ void rearm_pivot_messages(double* smem, int lane, int j0, int j1) {
  for (int jj = j0; jj < j1; ++jj) smem[msg_off(jj) + lane] = __longlong_as_double(-1ll);
}
// first wave: d = symmetric positive definite 16 x 16 block, accumulator layout.  false on a non-positive / non-finite pivot.
// (estamp: tools/tile_factor_bench.hip — when each message is posted.)
__device__ __forceinline__ bool ldl16_eliminate(dbl4 d, double* msg, int lane, long long* estamp = nullptr) {
  const int c = lane & 15, g = lane >> 4;
  typedef __attribute__((address_space(3))) double* lds_ptr;
  lds_ptr lm = (lds_ptr)msg;
  bool ok = true;
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) {
    const int gg = jj & 3, vv = jj >> 2;
    const bool grp = g == gg;
    const double dv = d[vv];
    const double piv = readlane_f64(dv, 16 * gg + jj);
    ok = ok && (piv > 0.0) && isfinite(piv);
    // -dv / piv = -(dv y0) (1 + e + e^2), e = 1 - piv y0: v_rcp_f64 is good to ~2^-23, e^3 is far below rounding; dv y0 runs
    // beside e, so the chain behind v_rcp is three operations long
    const double y0 = __builtin_amdgcn_rcp(piv), e = fma(-piv, y0, 1.0), t = dv * y0;
    const double q = fma(t, fma(e, e, e), t);
    const double row = grp ? dv : 0.0;                  // B: row jj of D   (k = gg slice, zero elsewhere)
    const double mul = (grp && c > jj) ? -q : 0.0;      // A: -D[jj][i] / d for the rows i below the pivot
    lm[msg_off(jj) + lane] = (grp && c == jj) ? dv : mul;  // the message: the multipliers, with the pivot itself in the (otherwise zero) lane of the diagonal
    // The message must LEAVE here: left alone the compiler pairs the sixteen stores up (ds_write2st64_b64) and sinks them behind the
    // thirteenth MFMA of the unrolled loop, and the following wave sees its first message 2 800 cycles into a 3 400-cycle block
    // (read off the ISA; profiles/r06/tile_factor.txt).
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (estamp && lane == 0) estamp[jj] = clock64();
    if (jj < 15) d = __builtin_amdgcn_mfma_f64_16x16x4f64(mul, row, d, 0, 0, 0);
  }
  return ok;
}

// second wave, on the vector unit: writes the full 16 x 16 block W(o.., o..) = chol(d)^-1 (zeros above the diagonal) into Wl.
// Lane c (< 16) keeps COLUMN c of E = L'^-1 in sixteen registers; pivot jj adds (-m_i) E[jj][c] to the rows i > jj — its own register jj
// times multipliers that are the same for every lane and come as broadcast reads of the message — 15 - jj independent FMAs, so the wave
// keeps pace with the eliminating one; row jj is final the moment pivot jj has been applied and goes to W (scaled by d_jj^-1/2) right
// away: what trails the last pivot is one reciprocal square root and one row.
// (fstamp: tools/tile_factor_bench.hip — when each message is seen and each row stored.)
__device__ __forceinline__ void ldl16_follow_rows(const double* msg, double* Wl, int o, int lane, long long* fstamp = nullptr) {
  typedef const volatile __attribute__((address_space(3))) double* lds_cvptr;   // volatile: re-read on every look; explicitly LDS (a volatile generic pointer would be read with flat loads)
  typedef double dbl2_t __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(3))) dbl2_t* lds_c2ptr;
  typedef __attribute__((address_space(3))) double* lds_ptr;
  lds_cvptr vm = (lds_cvptr)msg;
  lds_ptr wl = (lds_ptr)Wl;
  if (lane >= 16) return;   // (the other lanes would only repeat the sixteen columns)
  const int c = lane;
  double e[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) e[i] = (i == c) ? 1.0 : 0.0;
  // Software pipeline, one pivot deep: when message jj is seen its multipliers are REQUESTED (same address in every lane: broadcast
  // reads, two cells each) and, while they travel, pivot jj - 1 — whose multipliers came in during the step before — is applied and
  // row jj - 2 (final since then) scaled and stored.  The eliminating wave writes a message with ONE LDS store and the sixteen cells of
  // lane group jj % 4 belong to one pass of it: once the pivot is there so are the multipliers; the compiler must not move their
  // loads above the polling loop, though.
  dbl2_t m2[2][8];
  double piv_prev = 0.0, piv_cur = 0.0;   // the pivots of messages jj - 1 and jj (each is used one step after it is seen)
  double next = vm[msg_off(0)];   // the pivot of message jj sits in the cell of lane 16 (jj % 4) + jj; requested one step ahead, looked at when needed
#pragma unroll
  for (int jj = 0; jj <= 16; ++jj) {
    if (jj < 16) {
      const int cell = msg_off(jj) + 16 * (jj & 3);
      // The look at message jj was requested one step ago, BEFORE that step's multipliers: this first test waits for that one read only
      // (s_waitcnt lgkmcnt(n) with the multipliers still in flight).  Written as a loop the compiler waits for everything at its head —
      // then a step costs a whole LDS round trip of its five reads, ~230 cycles against the 204 of the eliminating wave, and the wave
      // ends 1 650 cycles behind it.  The second look (message not there yet) may wait for all it likes.
      double piv = next;
      if (__builtin_expect(__ballot(!filled(piv)) != 0ull, 0)) { do { piv = vm[cell + jj]; } while (__ballot(!filled(piv)) != 0ull); }
      piv_prev = piv_cur; piv_cur = piv;
      if (fstamp && lane == 0) fstamp[4 * jj] = clock64();
      asm volatile("" ::: "memory");
      if (jj < 15) next = vm[msg_off(jj + 1) + 16 * ((jj + 1) & 3) + jj + 1];
#pragma unroll
      for (int h = 0; h < 8; ++h) if (2 * h + 1 > jj) m2[jj & 1][h] = *(lds_c2ptr)(msg + cell + 2 * h);
    }
    if (jj >= 1) {   // pivot jj - 1
      const int k = jj - 1;
      // d_k^-1/2 — from the hardware estimate y0 (good to ~2^-23) by one cubic step, e = 1 - x y0^2, y = y0 (1 + e/2 + 3 e^2/8); e^3 is far below
      // rounding — is threaded through the row updates: the four dependent steps behind v_rsq_f64 wait out their latencies
      // behind independent FMAs.  Everything is pinned where it stands: left alone, the compiler turns the fifteen independent
      // updates of a pivot into one dependent sum per row, formed right before the row is used — k FMA latencies on the chain.
      const double x = jj < 16 ? piv_prev : piv_cur;   // pivot k (at jj = 16 no new message has shifted the pair)
      double y0 = __builtin_amdgcn_rsq(x), t0 = 0.0, q0 = 0.0, p0 = 0.0;
      asm volatile("" : "+v"(y0));
#pragma unroll
      for (int i = k + 1; i < 16; ++i) {
        e[i] = fma(m2[k & 1][i >> 1][i & 1], e[k], e[i]); asm volatile("" : "+v"(e[i]));
        const int step = i - k;
        if (step == 2) { t0 = -x * y0; asm volatile("" : "+v"(t0)); }
        if (step == 4) { t0 = fma(t0, y0, 1.0); asm volatile("" : "+v"(t0)); }                       // e = 1 - x y0^2
        if (step == 6) { q0 = y0 * t0; p0 = fma(0.375, t0, 0.5); asm volatile("" : "+v"(q0), "+v"(p0)); }
      }
      const int nstep = 15 - k;   // (the pivots near the end of the block have too few updates to hide behind: the rest of the chain follows here)
      if (nstep < 2) t0 = -x * y0;
      if (nstep < 4) t0 = fma(t0, y0, 1.0);
      if (nstep < 6) { q0 = y0 * t0; p0 = fma(0.375, t0, 0.5); }
      const double rs = fma(q0, p0, y0);
      wl[(o + k) * TP + o + c] = rs * e[k];   // row k has been final since pivot k - 1 (exact zeros right of the diagonal: E is lower triangular)
      if (fstamp && lane == 0) fstamp[4 * k + 3] = clock64();
    }
  }
}
// how factor_invert_tile's second wave produces the block W(o.., o..): the form above (tools/tile_factor_baselines.hpp has the earlier one)
struct FollowRows { static __device__ __forceinline__ void run(const double* msg, double* Wl, int o, int lane) { ldl16_follow_rows(msg, Wl, o, lane); } };

// ---- 16 x 16 blocks of a tile in LDS (pitch TP), accumulator layout ---------------------------------------------------
// the block at (o, o) of a tile whose lower triangle is valid, mirrored
__device__ __forceinline__ dbl4 load_sym16(const double* D, int o, int lane) {
  const int c = lane & 15, g = lane >> 4;
  dbl4 d;
#pragma unroll
  for (int v = 0; v < 4; ++v) { const int r = g + 4 * v; d[v] = D[(o + (r > c ? r : c)) * TP + o + (r > c ? c : r)]; }
  return d;
}
__device__ __forceinline__ dbl4 load16(const double* M, int rb, int cb, int lane) {
  dbl4 d;
#pragma unroll
  for (int v = 0; v < 4; ++v) d[v] = M[(rb + (lane >> 4) + 4 * v) * TP + cb + (lane & 15)];
  return d;
}
__device__ __forceinline__ void put16(double* M, int rb, int cb, dbl4 x, int lane) {
#pragma unroll
  for (int v = 0; v < 4; ++v) M[(rb + (lane >> 4) + 4 * v) * TP + cb + (lane & 15)] = x[v];
}
// 16 x 16 x 16 block products: acc + sign * X(xr.., xc..) Y(yr.., yc..)^T  resp.  acc + sign * X Y
__device__ __forceinline__ dbl4 mm16_nt(const double* X, int xr, int xc, const double* Y, int yr, int yc, dbl4 acc, double sign, int lane) {
  const int mi = lane & 15, mg = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sign * X[(xr + mi) * TP + xc + 4 * kk + mg], Y[(yr + mi) * TP + yc + 4 * kk + mg], acc, 0, 0, 0);
  return acc;
}
__device__ __forceinline__ dbl4 mm16_nn(const double* X, int xr, int xc, const double* Y, int yr, int yc, dbl4 acc, double sign, int lane) {
  const int mi = lane & 15, mg = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sign * X[(xr + mi) * TP + xc + 4 * kk + mg], Y[(yr + 4 * kk + mg) * TP + yc + mi], acc, 0, 0, 0);
  return acc;
}

// ---- the tile ------------------------------------------------------------------------------------------------------------
// W = chol(D)^-1 for the T x T tile D in LDS (lower triangle valid, pitch TP; destroyed) into Wl (lower blocks; the blocks
// above the diagonal are left untouched), by 16 x 16 blocks: the first two waves walk the three diagonal blocks (the serial
// chain), the others keep the off-diagonal algebra out of their way:
//   L_I0 = D_I0 W_00^T ;  D_11 -= L_10 L_10^T, D_21 -= L_20 L_10^T, D_22 -= L_20 L_20^T ;  L_21 = D_21 W_11^T ;  D_22 -= L_21 L_21^T
//   W_10 = -W_11 (L_10 W_00),  W_21 = -W_22 (L_21 W_11),  W_20 = -W_22 (L_20 W_00 + L_21 W_10).
// D, Wl, Tm, Lp must be the task's LDS buffers 0 .. 3 (the pivot messages live in idle rows of Tm and Lp, see the LDS map) and the
// messages armed (arm_pivot_messages) before the barrier in front of this call.  All threads must call; ends with a barrier.  Returns (in the first wave)
// false on a non-positive pivot.
// wout (HBM, row-major T x T; null = keep W in LDS only): the inverse leaves by ROW BLOCKS as they become final — rows 0-15 after the
// first diagonal block (a third into the factorisation), rows 16-31 after the second, rows 32-47 at the end, stored by waves that
// have nothing else to do — so that the DIAG task of the next column on the critical chain (task_diag) forms L = X W^T and D -= L L^T
// column block by column block under the rest of this factorisation; what is left for it when the last rows land is a third of both.
// TRACE: phase stamps before / after every barrier (tools/tile_factor_bench.hip); Follower: the second wave's form.
template <bool TRACE = false, bool DAG = false, class Follower = FollowRows>
__device__ __forceinline__ bool factor_invert_tile(double* D, double* Wl, double* Tm, double* Lp, int tid, long long* stamps = nullptr, double* wout = nullptr) {
  const int wave = tid >> 6, lane = tid & 63;
  const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
  bool ok = true;
  int nstamp = 0;
  auto stamp = [&]() { if (TRACE && tid == 0) stamps[nstamp++] = clock64(); };
  double* msg = D;   // (D is the first LDS buffer of the task; the messages sit at msg_off() behind it)
  auto publish_rows = [&](int rb, int nthreads, int t) {   // rows 16 rb .. 16 rb + 15 of W: lower blocks from Wl, exact zeros right of the diagonal block
    for (int e = t; e < 16 * T; e += nthreads) { const int r = 16 * rb + e / T, c = e % T; st<DAG>(wout + r * T + c, c < 16 * (rb + 1) ? Wl[r * TP + c] : 0.0); }
  };
  stamp();
  // ONE copy of the two sixteen-pivot loops (the bulk of this function's code), gone through three times: inside the solver a task runs
  // this function once, and its instructions come from memory — spelled out, blocks 1 and 2 ran cold too ("What did help:
  // less code").  Blocks 1 and 2 now run from the instruction cache.
#pragma clang loop unroll(disable)
  for (int b = 0; b < 3; ++b) {
    const int o = 16 * b;
    if (wave == 0) {
      dbl4 d = load_sym16(D, o, lane);
      if (b > 0) d = mm16_nt(Lp, o, o - 16, Lp, o, o - 16, d, -1.0, lane);   // D_bb - L_b,b-1 L_b,b-1^T (block 2 has lost L_20 L_20^T already)
      ok = ldl16_eliminate(d, msg, lane) && ok;
    } else if (wave == 1) {
      Follower::run(msg, Wl, o, lane);
    } else if (b == 1) {
      if (wave == 2) {
        put16(D, 32, 16, mm16_nt(Lp, 32, 0, Lp, 16, 0, load16(D, 32, 16, lane), -1.0, lane), lane);
        put16(Tm, 16, 0, mm16_nn(Lp, 16, 0, Wl, 0, 0, zero, 1.0, lane), lane);                                         // T_10 = L_10 W_00
      } else {
        put16(D, 32, 32, mm16_nt(Lp, 32, 0, Lp, 32, 0, load16(D, 32, 32, lane), -1.0, lane), lane);                     // (its upper half is never read)
        if (wout) publish_rows(0, 64, lane);   // W_00 has been final since the first barrier; this step is long (sixteen pivots), the one before is not
      }
    } else if (b == 2) {
      if (wave == 2) put16(Tm, 32, 16, mm16_nn(Lp, 32, 16, Wl, 16, 16, zero, 1.0, lane), lane);                        // T_21 = L_21 W_11
      else {
        put16(Tm, 32, 0, mm16_nn(Lp, 32, 16, Wl, 16, 0, load16(Tm, 32, 0, lane), 1.0, lane), lane);                     // T_20 += L_21 W_10
        if (wout) publish_rows(1, 64, lane);   // W_10, W_11 have been final since the barrier above
      }
    }
    stamp(); lds_barrier(); stamp();
    if (b == 0) {
      if (wave < 2) put16(Lp, 16 + 16 * wave, 0, mm16_nt(D, 16 + 16 * wave, 0, Wl, 0, 0, zero, 1.0, lane), lane);   // L_10, L_20
      else rearm_pivot_messages(D, lane, 8 * (wave - 2), 8 * (wave - 1));   // (both waves of block 0 are done with them; block 1 starts behind the next barrier)
    } else if (b == 1) {
      if (wave == 0) put16(Lp, 32, 16, mm16_nt(D, 32, 16, Wl, 16, 16, zero, 1.0, lane), lane);       // L_21
      else if (wave == 1) put16(Wl, 16, 0, mm16_nn(Wl, 16, 16, Tm, 16, 0, zero, -1.0, lane), lane);  // W_10
      else if (wave == 2) put16(Tm, 32, 0, mm16_nn(Lp, 32, 0, Wl, 0, 0, zero, 1.0, lane), lane);     // T_20 = L_20 W_00
      else rearm_pivot_messages(D, lane, 0, 16);
    } else {
      if (wave == 0) put16(Wl, 32, 16, mm16_nn(Wl, 32, 32, Tm, 32, 16, zero, -1.0, lane), lane);      // W_21
      else if (wave == 1) put16(Wl, 32, 0, mm16_nn(Wl, 32, 32, Tm, 32, 0, zero, -1.0, lane), lane);   // W_20
    }
    stamp(); lds_barrier(); stamp();
  }
  if (wout) publish_rows(2, 256, tid);
  return ok;
}

}  // namespace
}  // namespace rsba
