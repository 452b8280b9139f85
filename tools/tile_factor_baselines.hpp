// Earlier forms of the tile factorisation (rsba_amd/csrc/tile_factor.hpp), kept as the baselines tools/tile_factor_bench.hip times and
// checks the library's form against.  The library runs none of this.
//   potrf_blocked + invert_lower_blocked   the lane-per-row blocked Cholesky and the blocked triangular inverse of round 1
//   ldl16_follow / FollowMfma              round 2's second wave of the MFMA-pivot LDL^T: rank-1 MFMAs on the identity — a chain of
//                                          dependent MFMAs (81 cycles each) with an LDS message wait in every link, 285 cycles per pivot
//                                          against the 206 of the eliminating wave ("The second wave of the tile factorisation")
#pragma once
#include "../rsba_amd/csrc/tile_factor.hpp"

namespace rsba {

namespace {

typedef dbl4 dbl4_t;   // (the spelling the baselines were written with)
constexpr int NB = 16;   // panel width of potrf_blocked: one MFMA block column

// 1/sqrt(x) to full fp64 accuracy: hardware estimate + two Newton steps (avoids the long fp64
// sqrt-then-divide dependency chain on the factorisation's critical path)
__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * (1.5 - 0.5 * x * y * y);
  y = y * (1.5 - 0.5 * x * y * y);
  return y;
}

// Factor the T x T tile held in LDS (lower triangle, pitch TP) in place: blocked right-looking Cholesky.
// Each 16-column panel is factored by the first wave entirely in registers (lane = row, pivot rows
// broadcast with v_readlane, 1/sqrt instead of sqrt + divide: no LDS round trips or barriers on the
// serial chain); the rank-16 trailing update runs on the matrix pipe, its blocks dealt to the four waves.
// All threads must call.
// Returns false (in the first wave) on a non-positive pivot.
__device__ __forceinline__ bool potrf_blocked(double* A, int tid) {
  bool ok = true;
#pragma unroll
  for (int bc = 0; bc < T / NB; ++bc) {
    const int c0 = NB * bc;
    if (tid < 64) {
      const int row = c0 + tid;
      const bool live = row < T;
      const int rr = live ? row : T - 1;
      double a[NB];
#pragma unroll
      for (int m = 0; m < NB; ++m) a[m] = A[rr * TP + c0 + m];
      // right-looking inside the panel: once column jj is scaled, the columns behind it are updated by independent
      // FMAs (the next pivot first), which fill the latency of the next 1/sqrt instead of forming one long sum
#pragma unroll
      for (int jj = 0; jj < NB; ++jj) {
        const double djj = readlane_f64(a[jj], jj);
        ok = ok && (djj > 0.0) && isfinite(djj);
        // the column is broadcast BEFORE it is scaled: the lane reads do not wait for the 1/sqrt chain, only the FMAs do
        double u[NB];
#pragma unroll
        for (int m = jj + 1; m < NB; ++m) u[m] = readlane_f64(a[jj], m);
        const double rinv = rsqrt_nr(djj);
        const double t = a[jj] * (rinv * rinv);                 // a_r / d
#pragma unroll
        for (int m = jj + 1; m < NB; ++m) a[m] -= t * u[m];      // a_rm -= a_r a_m / d
        a[jj] = (tid == jj) ? djj * rinv : a[jj] * rinv;
      }
      if (live) {
#pragma unroll
        for (int m = 0; m < NB; ++m) if (c0 + m <= row) A[row * TP + c0 + m] = a[m];
      }
    }
    lds_barrier();
    // rank-16 trailing update A[r][c] -= sum_m L[r][c0 + m] L[c][c0 + m] for c0 + 12 <= c <= r on the matrix pipe
    // (K = 16 = four MFMA steps): the 16 x 16 blocks of the tile grid that reach into the trailing part are
    // dealt to the waves, products formed in full and subtracted under a mask.
    if (c0 + NB < T) {
      const int wave = tid >> 6, lane = tid & 63, mi = lane & 15, mg = lane >> 4;
      const int first = (c0 + NB) >> 4;                        // first block row / column that has trailing entries
      int blk = 0;
#pragma unroll
      for (int I = 0; I < 3; ++I)
#pragma unroll
        for (int J = 0; J <= I; ++J) {
          if (J < first) continue;                             // I >= J >= first
          if ((blk++ & 3) != wave) continue;
          dbl4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int kk = 0; kk < NB / 4; ++kk)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(16 * I + mi) * TP + c0 + 4 * kk + mg], A[(16 * J + mi) * TP + c0 + 4 * kk + mg], acc, 0, 0, 0);
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int r = 16 * I + mg + 4 * v, c = 16 * J + mi;
            if (c >= c0 + NB && c <= r) A[r * TP + c] -= acc[v];
          }
        }
      lds_barrier();
    }
  }
  return ok;
}

// W = L^-1 for the factored lower-triangular tile L in LDS (pitch TP), into Wl (pitch TP; blocks above the
// diagonal left untouched), by 16 x 16 blocks:
//   W_bb = L_bb^-1 (forward substitution, one wave per block, a lane per column), then, as 16 x 16 MFMA products,
//   W_10 = -W_11 (L_10 W_00),  W_21 = -W_22 (L_21 W_11),  W_20 = -W_22 (L_20 W_00 + L_21 W_10).
// Tm (pitch TP) is scratch for the inner products.  All threads must call; ends with a barrier.
__device__ __forceinline__ void invert_lower_blocked(const double* L, const double* dinv, double* Wl, double* Tm, int tid) {
  constexpr int B = 16;
  const int wave = tid >> 6, lane = tid & 63;
  if (wave < 3) {
    const int o = B * wave, cc = lane < B ? lane : B - 1;
    double w[B];
#pragma unroll
    for (int i = 0; i < B; ++i) {
      double s = (i == cc) ? 1.0 : 0.0;
#pragma unroll
      for (int m = 0; m < i; ++m) s -= L[(o + i) * TP + o + m] * w[m];
      w[i] = s * dinv[o + i];
    }
    if (lane < B) {
#pragma unroll
      for (int i = 0; i < B; ++i) Wl[(o + i) * TP + o + cc] = w[i];
    }
  }
  lds_barrier();
  // 16 x 16 block products on the matrix pipe, one wave each: (rows xr.., columns xo.. of X) times (rows yo.., columns
  // yc.. of Y), result in the MFMA layout (this lane: column lane & 15, rows (lane >> 4) + 4v)
  const int mi = lane & 15, mg = lane >> 4;
  auto mm16 = [&](const double* X, int xr, int xo, const double* Y, int yo, int yc, dbl4 acc) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[(xr + mi) * TP + xo + 4 * kk + mg], Y[(yo + 4 * kk + mg) * TP + yc + mi], acc, 0, 0, 0);
    return acc;
  };
  auto put = [&](double* M, int rb, int cb, dbl4 v, double sign) {
#pragma unroll
    for (int q = 0; q < 4; ++q) M[(rb + mg + 4 * q) * TP + cb + mi] = sign * v[q];
  };
  const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
  if (wave == 0) put(Tm, 16, 0, mm16(L, 16, 0, Wl, 0, 0, zero), 1.0);          // T10 = L10 W00
  else if (wave == 1) put(Tm, 32, 16, mm16(L, 32, 16, Wl, 16, 16, zero), 1.0);  // T21 = L21 W11
  else if (wave == 2) put(Tm, 32, 0, mm16(L, 32, 0, Wl, 0, 0, zero), 1.0);      // T20 = L20 W00
  lds_barrier();
  if (wave == 0) put(Wl, 16, 0, mm16(Wl, 16, 16, Tm, 16, 0, zero), -1.0);       // W10 = -W11 T10
  else if (wave == 1) put(Wl, 32, 16, mm16(Wl, 32, 32, Tm, 32, 16, zero), -1.0);   // W21 = -W22 T21
  lds_barrier();
  if (wave == 0) {                                                              // T20 += L21 W10 ; W20 = -W22 T20
    dbl4 t;
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = Tm[(32 + mg + 4 * q) * TP + mi];
    put(Tm, 32, 0, mm16(L, 32, 16, Wl, 16, 0, t), 1.0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    put(Wl, 32, 0, mm16(Wl, 32, 32, Tm, 32, 0, zero), -1.0);
  }
  lds_barrier();
}

// second wave: W = chol(d)^-1 (lower, exact zeros above the diagonal), accumulator layout
__device__ __forceinline__ dbl4_t ldl16_follow(const double* msg, int lane, long long* fstamp = nullptr) {
  const int c = lane & 15, g = lane >> 4;
  typedef const volatile __attribute__((address_space(3))) double* lds_cvptr;   // volatile: re-read on every look; explicitly LDS (a volatile generic pointer would be read with flat loads)
  lds_cvptr vm = (lds_cvptr)msg;
  dbl4_t w;
#pragma unroll
  for (int v = 0; v < 4; ++v) w[v] = (g + 4 * v == c) ? 1.0 : 0.0;
  double pv[4] = {1.0, 1.0, 1.0, 1.0};   // the pivots of this lane's four rows
  double next = vm[msg_off(0) + lane];
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) {
    const int gg = jj & 3, vv = jj >> 2;
    const bool grp = g == gg;
    double m = next;
    while (__ballot(!filled(m)) != 0ull) m = vm[msg_off(jj) + lane];
    // the next message is requested BEFORE this pivot's MFMA and looked at after it (a speculative read: what is not there yet
    // is read again above) — the LDS round trip would otherwise sit between every two MFMAs of this wave
    if (jj < 15) next = vm[msg_off(jj < 15 ? jj + 1 : 15) + lane];
    __builtin_amdgcn_sched_barrier(0);
    const double piv = readlane_f64(m, 16 * gg + jj);
    const double mul = (grp && c == jj) ? 0.0 : m;
    const double wrow = grp ? w[vv] : 0.0;                     // B: row jj of W' = L'^-1 as it stands
    if (jj < 15) w = __builtin_amdgcn_mfma_f64_16x16x4f64(mul, wrow, w, 0, 0, 0);
    pv[vv] = grp ? piv : pv[vv];
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) w[v] *= rsqrt_nr(pv[v]);
  return w;
}
struct FollowMfma {
  static __device__ __forceinline__ void run(const double* msg, double* Wl, int o, int lane) { put16(Wl, o, o, ldl16_follow(msg, lane), lane); }
};

}  // namespace

}  // namespace rsba
