// Brute-force k-nearest-neighbour search over 128-float descriptors: the device part of VideoSfMClient::Match
// (VideoSfMClient.cc:73-129: cv::BFMatcher().knnMatch, NORM_L2, k = 2 or 5), for a list of (query frame, train frame) pairs.
//
// Three passes on one stream:
//   match_norms    ||row||^2 of every descriptor row, accumulated in double and rounded once
//   match_search   d2(i, j) = (||q_i||^2 + ||t_j||^2) - 2 q_i.t_j with the dot product on the f32-in / f32-accumulate MFMA
//                  (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, one rounding per product).  For integer descriptors in
//                  [0, 255] every partial sum stays below 2^24 — the dot product <= 128 * 255^2, the norm sum <= 2 * 128 * 255^2,
//                  and the last fmaf(-2, dot, norms) lands on the exact non-negative integer — so d2 is exact, not merely close.
//                  (The norms are never combined with +2 q.t, which could reach 2^25.)
//                  Orientation: TRAIN rows are the A operand, QUERIES the B operand, so that the C/D column — the lane — is
//                  the query and the 16 accumulator registers run over train rows.  Every lane keeps a private sorted top-K
//                  for its query and the epilogue is per-lane compares; no cross-lane traffic at all.  The two lane halves of
//                  a query (rows 4h .. 4h+3 of every group of 8) and the workgroups that split a pair's train tiles each
//                  write their own list; match_refine merges them.
//                  A workgroup owns 128 queries (4 waves x 32), whose fragments stay in registers (64 VGPRs), and streams
//                  128-row train tiles through LDS, stored k-major so that one ds_read_b128 per k-step feeds the four
//                  independent 32 x 32 accumulators of a wave (train row 4 r' + m of the tile is row r' of accumulator m).
//                  Two workgroups fit a CU (66.5 KiB LDS each): one loads while the other multiplies.
//                  The list is ordered by (sqrtf(d2), train index), which is what BFMatcher orders by: two different d2 can
//                  share a rounded root, and then the lower index wins.  A lane meets its train rows in ascending order, so
//                  a strict compare keeps the lower index; the root is taken only for the few candidates that pass the
//                  d2 pre-test against the list's worst entry.
//   match_refine   one thread per query: merges its lists, recomputes the K survivors' distances in direct form
//                  sum (q - t)^2 — an fmaf chain in k order, then sqrtf (correctly rounded: hipcc's default, no fast-math flag
//                  here) — and orders them by (that distance, index).  For non-integer descriptors the caller then sees the
//                  value a BFMatcher reports, not the cancellation-prone GEMM form.
// Rows and columns that pad a partial tile are loaded as zeros and can never enter a list: a padded train row fails the
// j < nt test, a padded query lane writes nothing.
#include <atomic>
#include <climits>
#include <cmath>

#include "match.hpp"

namespace rsba {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int LDT = MATCH_TTILE + 4;   // floats per k-row of the LDS tile: +4 keeps 16-byte alignment and spreads the fill's stores over all banks
constexpr size_t SEARCH_LDS = (size_t)(MATCH_DIM * LDT + MATCH_TTILE) * sizeof(float);

__global__ __launch_bounds__(256) void match_norms(const float* __restrict__ desc, float* __restrict__ norm, int64_t rows) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float4* p = reinterpret_cast<const float4*>(desc + r * MATCH_DIM);
  double s = 0.0;
  for (int c = 0; c < MATCH_DIM / 4; ++c) {
    const float4 v = p[c];
    s += (double)v.x * (double)v.x; s += (double)v.y * (double)v.y; s += (double)v.z * (double)v.z; s += (double)v.w * (double)v.w;
  }
  norm[r] = (float)s;
}

template <int K>
__global__ __launch_bounds__(256, 2) void match_search(const MatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tT = smem;                      // [128 k][LDT]: tT[k * LDT + row]
  float* tn = smem + MATCH_DIM * LDT;    // [128] norms of the tile's rows
  const MatchItem it = a.items[blockIdx.x];
  const MatchPair P = a.pairs[it.pair];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int q = it.q0 + wave * 32 + r;   // frame-local query of this lane (both lane halves)
  const bool q_ok = q < P.nq;

  // B operand of k-step s: Q[q][2 s + h]
  float qf[MATCH_DIM / 2];
  float qn = 0.f;
  {
    const float4* qrow = reinterpret_cast<const float4*>(a.desc + (P.q_row + (q_ok ? q : 0)) * MATCH_DIM);
#pragma unroll
    for (int u = 0; u < MATCH_DIM / 4; ++u) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q_ok) v = qrow[u];
      qf[2 * u] = h ? v.y : v.x;
      qf[2 * u + 1] = h ? v.w : v.z;
    }
    if (q_ok) qn = a.norm[P.q_row + q];
  }

  float ks[K], kd[K]; int ki[K];   // sorted by (ks, ki): ks = sqrtf(d2), kd = d2
#pragma unroll
  for (int i = 0; i < K; ++i) { ks[i] = INFINITY; kd[i] = INFINITY; ki[i] = INT_MAX; }

  const int jr = lane & 15, kq = lane >> 4;
  for (int tile = it.tile0; tile < it.tile1; ++tile) {
    const int base = tile * MATCH_TTILE;
    __syncthreads();   // the previous tile has been read
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int row = wave * 32 + (i & 1) * 16 + jr, quad = (i >> 1) * 4 + kq;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (base + row < P.nt) v = *reinterpret_cast<const float4*>(a.desc + (P.t_row + base + row) * MATCH_DIM + 4 * quad);
      float* dst = tT + (4 * quad) * LDT + row;
      dst[0] = v.x; dst[LDT] = v.y; dst[2 * LDT] = v.z; dst[3 * LDT] = v.w;
    }
    if (tid < MATCH_TTILE) tn[tid] = base + tid < P.nt ? a.norm[P.t_row + base + tid] : INFINITY;
    __syncthreads();

    f32x16 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;
#pragma unroll
    for (int s = 0; s < MATCH_DIM / 2; ++s) {
      const float4 av = *reinterpret_cast<const float4*>(tT + (2 * s + h) * LDT + 4 * r);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, qf[s], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, qf[s], acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, qf[s], acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, qf[s], acc[3], 0, 0, 0);
    }

    // C/D: column = lane & 31 (the query), row = (reg & 3) + 8 (reg >> 2) + 4 h; train row of the tile = 4 row + m:
    // ascending in (reg, m), so a lane meets its train rows in ascending order
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int rp = (reg & 3) + 8 * (reg >> 2) + 4 * h;
      const float4 n4 = *reinterpret_cast<const float4*>(tn + 4 * rp);
      const float nn[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int j = base + 4 * rp + m;
        const float d2 = fmaf(-2.f, acc[m][reg], qn + nn[m]);
        if (d2 < kd[K - 1] && j < P.nt) {
          const float s = sqrtf(fmaxf(d2, 0.f));
          if (s < ks[K - 1]) {
            ks[K - 1] = s; kd[K - 1] = d2; ki[K - 1] = j;
#pragma unroll
            for (int i = K - 1; i > 0; --i) {
              if (ks[i] < ks[i - 1]) {
                const float ts = ks[i]; ks[i] = ks[i - 1]; ks[i - 1] = ts;
                const float td = kd[i]; kd[i] = kd[i - 1]; kd[i - 1] = td;
                const int ti = ki[i]; ki[i] = ki[i - 1]; ki[i - 1] = ti;
              }
            }
          }
        }
      }
    }
  }

  if (q_ok) {
    const int64_t list = P.cand + (int64_t)q * P.lists + it.split * 2 + h;
#pragma unroll
    for (int i = 0; i < K; ++i) { a.cand_key[list * K + i] = ks[i]; a.cand_idx[list * K + i] = ki[i]; }
  }
}

template <int K>
__global__ __launch_bounds__(64) void match_refine(const MatchArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= a.num_queries) return;
  int64_t lo = 0, hi = a.num_pairs;   // the pair with query_pair_start[p] <= g < query_pair_start[p + 1]
  while (hi - lo > 1) { const int64_t mid = (lo + hi) / 2; if (a.query_pair_start[mid] <= g) lo = mid; else hi = mid; }
  const MatchPair P = a.pairs[lo];
  const int q = (int)(g - a.query_pair_start[lo]);
  const int k = a.k;
  const int64_t out = P.out + (int64_t)q * k;
  const int kk = P.nt < 2 ? 0 : (k < P.nt ? k : P.nt);

  float bs[K]; int bi[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { bs[i] = INFINITY; bi[i] = INT_MAX; }
  const int64_t list0 = P.cand + (int64_t)q * P.lists;
  for (int l = 0; l < (kk ? P.lists : 0); ++l) {
    for (int e = 0; e < K; ++e) {
      const float s = a.cand_key[(list0 + l) * K + e];
      const int j = a.cand_idx[(list0 + l) * K + e];
      if (j == INT_MAX) break;   // the rest of this list is empty
      if (s < bs[K - 1] || (s == bs[K - 1] && j < bi[K - 1])) {
        bs[K - 1] = s; bi[K - 1] = j;
#pragma unroll
        for (int i = K - 1; i > 0; --i) {
          if (bs[i] < bs[i - 1] || (bs[i] == bs[i - 1] && bi[i] < bi[i - 1])) {
            const float ts = bs[i]; bs[i] = bs[i - 1]; bs[i - 1] = ts;
            const int ti = bi[i]; bi[i] = bi[i - 1]; bi[i - 1] = ti;
          }
        }
      } else {
        break;   // a list ascends: nothing later in it can enter either
      }
    }
  }

  // the survivors' distances in direct form, then ordered by (distance, index)
  const float4* qrow = reinterpret_cast<const float4*>(a.desc + (P.q_row + q) * MATCH_DIM);
#pragma unroll
  for (int i = 0; i < K; ++i) {
    if (bi[i] == INT_MAX) { bs[i] = INFINITY; continue; }
    const float4* trow = reinterpret_cast<const float4*>(a.desc + (P.t_row + bi[i]) * MATCH_DIM);
    float d2 = 0.f;
    for (int c = 0; c < MATCH_DIM / 4; ++c) {
      const float4 x = qrow[c], y = trow[c];
      const float e0 = x.x - y.x, e1 = x.y - y.y, e2 = x.z - y.z, e3 = x.w - y.w;
      d2 = fmaf(e0, e0, d2); d2 = fmaf(e1, e1, d2); d2 = fmaf(e2, e2, d2); d2 = fmaf(e3, e3, d2);
    }
    bs[i] = sqrtf(d2);
  }
#pragma unroll
  for (int n = 1; n < K; ++n)
#pragma unroll
    for (int i = n; i > 0; --i)
      if (bs[i] < bs[i - 1] || (bs[i] == bs[i - 1] && bi[i] < bi[i - 1])) {
        const float ts = bs[i]; bs[i] = bs[i - 1]; bs[i - 1] = ts;
        const int ti = bi[i]; bi[i] = bi[i - 1]; bi[i - 1] = ti;
      }
#pragma unroll
  for (int i = 0; i < K; ++i)
    if (i < k) {
      const bool have = i < kk;
      a.nn_index[out + i] = have ? bi[i] : -1;
      a.nn_dist[out + i] = have ? bs[i] : INFINITY;
    }
  a.nn_count[out / k] = kk;
}

template <int K>
hipError_t launch_k(const MatchArgs& a, hipStream_t st) {
  // more than 64 KiB of LDS has to be asked for, once per device (all threads set the same value)
  static std::atomic<uint64_t> lds_set{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = uint64_t(1) << (dev & 63);
  if (!(lds_set.load(std::memory_order_acquire) & bit)) {
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&match_search<K>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEARCH_LDS)) != hipSuccess) return e;
    lds_set.fetch_or(bit, std::memory_order_release);
  }
  if (a.num_items > 0) hipLaunchKernelGGL(match_search<K>, dim3((unsigned)a.num_items), dim3(256), SEARCH_LDS, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.num_queries > 0) hipLaunchKernelGGL(match_refine<K>, dim3((unsigned)((a.num_queries + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_match(const MatchArgs& a, hipStream_t st) {
  if (a.rows > 0) hipLaunchKernelGGL(match_norms, dim3((unsigned)((a.rows + 255) / 256)), dim3(256), 0, st, a.desc, a.norm, a.rows);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return a.K == 2 ? launch_k<2>(a, st) : launch_k<MATCH_KMAX>(a, st);
}

}  // namespace rsba
