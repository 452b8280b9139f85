// The loop of the batched pair RANSAC (rsba_epipolar_ransac_pairs, rsba_two_view_classify_pairs) around a model's hypothesis kernels — the
// device form of epi_detail::ransac / homo_detail::ransac per pair, once for both models.  Integers and copies only, but for the inlier
// flags, which come from the one copy of the deciding comparisons (two_view_rules.hpp): nothing here can round differently from the
// single-pair calls.
//   pair_winner_kernel    one wave per pair over its tasks: the key (inliers, most in front) as one integer, its maximum and then the
//                         lowest task that reaches it, each by a butterfly over the wave
//   pair_masks_kernel     one lane per correspondence: the inlier flag by its pair's current matrix; one body, compiled per inlier rule
//   pair_compact_kernel   one wave per pair: the ascending inlier indices by ballot and the popcount of the lower lanes
//   pair_adopt_kernel     one lane per pair: a refit adopted iff accepted and its count is not lower; else the pair is done
// The pose and the four front counts belong to the essential matrix alone: where their pointers are null they are neither read nor written.
#include <climits>

#include "pair_loop_state.hpp"
#include "two_view_rules.hpp"

namespace rsba {

namespace {

constexpr int kWave = 64;   // one wave per workgroup

// what the winner is chosen by: most inliers, then most in front (zero where that does not break ties, or there are no front counts) — one
// integer per task, 0 for a declined one — then the lowest task.  With a zero low word the order is that of (inliers + 1) alone.  Two
// reductions of one value each (a maximum, then a minimum over the tasks that reach it), both by a butterfly over the wave: integers, so
// every lane ends with the value a serial scan ends with.
__device__ __forceinline__ unsigned long long winner_key(const WinnerArgs& A, size_t g) {
  if (!A.status[g]) return 0ull;
  int front = 0;
  if (A.front_breaks_ties && A.num_front) {
    front = A.num_front[g * 4];
    for (int k = 1; k < 4; ++k) front = max(front, A.num_front[g * 4 + k]);
  }
  return ((unsigned long long)((unsigned)A.num_inliers[g] + 1u) << 32) | (unsigned)front;
}

__global__ __launch_bounds__(kWave) void pair_winner_kernel(const WinnerArgs A) {
  const int lane = threadIdx.x, p = blockIdx.x, T = A.tasks_per_pair;
  unsigned long long best = 0ull;
  for (int t = lane; t < T; t += kWave) best = max(best, winner_key(A, (size_t)p * T + t));
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) best = max(best, (unsigned long long)__shfl_xor((long long)best, off));
  int first = INT_MAX;   // the lowest task with that key
  for (int t = lane; t < T; t += kWave) first = min(first, best != 0ull && winner_key(A, (size_t)p * T + t) == best ? t : INT_MAX);
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) first = min(first, __shfl_xor(first, off));
  if (lane != 0) return;
  const PairLoopState& S = A.S;
  const bool has = best != 0ull;
  const int winner = has ? first : -1;
  S.status[p] = has ? 1 : 0;
  S.done[p] = has ? 0 : 1;
  S.winner_task[p] = winner;
  S.refits_adopted[p] = 0;
  S.inlier_count[p] = 0;
  const size_t g = (size_t)p * T + (has ? winner : 0);
  S.num_inliers[p] = has ? A.num_inliers[g] : 0;
  if (S.num_front) for (int c = 0; c < 4; ++c) S.num_front[(size_t)p * 4 + c] = has ? A.num_front[g * 4 + c] : 0;
  if (!has) return;
  for (int k = 0; k < 9; ++k) S.model[(size_t)p * 9 + k] = A.models[g * 9 + k];
  if (S.pose) for (int k = 0; k < 6; ++k) S.pose[(size_t)p * 6 + k] = A.poses[g * 6 + k];
}

// the inlier rule of a model: what a lane keeps of its pair's matrix, and the flag of one correspondence
struct SampsonRule {
  double E[9];
  __device__ __forceinline__ void load(const double* M) {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = M[k];
  }
  __device__ __forceinline__ bool inlier(double xa, double ya, double xb, double yb, double f2, double thr2) const { return sampson_inlier(E, xa, ya, xb, yb, f2, thr2); }
};
struct TransferRule {
  double H[9], Hi[9];
  bool ok;
  __device__ __forceinline__ void load(const double* M) {
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = M[k];
    ok = invert(H, Hi);
  }
  __device__ __forceinline__ bool inlier(double xa, double ya, double xb, double yb, double f2, double thr2) const { return ok && transfer_inlier(H, Hi, xa, ya, xb, yb, f2, thr2); }
};

template <class Rule>
__global__ __launch_bounds__(256) void pair_masks_kernel(const PairLoopState S, const int32_t* __restrict__ point_pair, int first_point, int num_points, double thr2,
                                                         const double* __restrict__ na, const double* __restrict__ nb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= num_points) return;
  const size_t g = (size_t)first_point + i;
  const int p = point_pair[g];
  if (S.done[p]) return;   // (no winner: the flags stay zero; no adopted refit: they stay the last matrix's)
  Rule rule;
  rule.load(S.model + (size_t)p * 9);
  S.mask[g] = rule.inlier(na[2 * g], na[2 * g + 1], nb[2 * g], nb[2 * g + 1], S.pairs[p].f2, thr2) ? 1 : 0;
}

// one wave per pair: lane l of a ballot writes at the running base plus the number of set lanes below it — the order of a serial push_back.
// A pair under min_refit inliers is done and its count is stored as 0, as the state's comment says.  (The count is scratch of the loop: the
// fit kernel reads it as the length of the pair's list and declines a short list either way, the adopt kernel returns for a pair that is
// done, and it is never downloaded.)
__global__ __launch_bounds__(kWave) void pair_compact_kernel(const PairLoopState S, int min_refit) {
  const int lane = threadIdx.x, p = blockIdx.x;
  if (S.done[p]) { if (lane == 0) S.inlier_count[p] = 0; return; }   // (uniform across the wave)
  const PairRange P = S.pairs[p];
  int count = 0;
  for (int base = 0; base < P.n; base += kWave) {   // (uniform trip count)
    const int i = base + lane;
    const bool in = i < P.n && S.mask[(size_t)P.start + i] != 0;
    const unsigned long long ballot = __ballot(in);
    if (in) S.inlier_idx[(size_t)P.start + count + __popcll(ballot & ((1ull << lane) - 1ull))] = P.start + i;
    count += __popcll(ballot);
  }
  if (lane != 0) return;
  if (count < min_refit) { S.done[p] = 1; count = 0; }   // (later rounds skip the pair)
  S.inlier_count[p] = count;
}

__global__ __launch_bounds__(256) void pair_adopt_kernel(const AdoptArgs A) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const PairLoopState& S = A.S;
  if (p >= S.num_pairs || S.done[p]) return;
  if (!A.status[p] || A.num_inliers[p] < S.num_inliers[p]) { S.done[p] = 1; return; }   // not adopted: the next round would refit the same set
  S.num_inliers[p] = A.num_inliers[p];
  if (S.num_front) for (int c = 0; c < 4; ++c) S.num_front[(size_t)p * 4 + c] = A.num_front[(size_t)p * 4 + c];
  for (int k = 0; k < 9; ++k) S.model[(size_t)p * 9 + k] = A.models[(size_t)p * 9 + k];
  if (S.pose) for (int k = 0; k < 6; ++k) S.pose[(size_t)p * 6 + k] = A.poses[(size_t)p * 6 + k];
  S.refits_adopted[p] += 1;
}

}  // namespace

hipError_t launch_pair_winner(const WinnerArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(pair_winner_kernel, dim3(A.S.num_pairs), dim3(kWave), 0, st, A);
  return hipGetLastError();
}
hipError_t launch_pair_masks(PairRule rule, const PairLoopState& S, const int32_t* point_pair, int first_point, int num_points, double thr2, const double* na,
                             const double* nb, hipStream_t st) {
  if (num_points <= 0) return hipSuccess;
  const dim3 grid((num_points + 255) / 256), block(256);
  if (rule == PairRule::Sampson) hipLaunchKernelGGL(pair_masks_kernel<SampsonRule>, grid, block, 0, st, S, point_pair, first_point, num_points, thr2, na, nb);
  else hipLaunchKernelGGL(pair_masks_kernel<TransferRule>, grid, block, 0, st, S, point_pair, first_point, num_points, thr2, na, nb);
  return hipGetLastError();
}
hipError_t launch_pair_compact(const PairLoopState& S, int min_refit, hipStream_t st) {
  hipLaunchKernelGGL(pair_compact_kernel, dim3(S.num_pairs), dim3(kWave), 0, st, S, min_refit);
  return hipGetLastError();
}
hipError_t launch_pair_adopt(const AdoptArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(pair_adopt_kernel, dim3((A.S.num_pairs + 255) / 256), dim3(256), 0, st, A);
  return hipGetLastError();
}

}  // namespace rsba
