// Verification of the persistent Cholesky driver's result (cholesky.hip: chol_dag_kernel, chol_solve_kernel).
#include "chol_cells.hpp"

namespace rsba {
namespace {

// The task-DAG kernel has no safety net inside: its hand-offs are write-once cells found by polling.  What it returns is
// therefore checked against the system it was asked to solve: res = rhs - S y over the packed tiles (S symmetric, lower
// tiles stored), with den = |rhs| + |S| |y| as the yardstick of a backward-stable solve.  A stale or torn cell anywhere
// in the factorisation shows up here as a residual many orders above rounding; the solver then repeats the solve on the
// level schedule (solver.hip).  Sums are fp64 atomics in arbitrary order: this is a check, not a result.
// res / den start out zero (the check kernel re-arms them after it has looked): one workgroup per packed tile adds what the
// tile contributes — thread (r, q) = (tid / 4, tid % 4) takes a quarter of row r resp. column r.
__global__ __launch_bounds__(256) void chol_residual_kernel(const SolverDev sv, const int32_t* __restrict__ slot_tiles, const double* __restrict__ b_rhs, double* res, double* den) {
  __shared__ double tile[T * TP];
  __shared__ double yj[T], yi[T];
  const int slot = blockIdx.x, tid = threadIdx.x, r = tid >> 2, q = tid & 3;
  const int tile_i = slot_tiles[2 * slot], tile_j = slot_tiles[2 * slot + 1];
  auto quad_sum = [](double v) { v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); return v; };
  if (tid < T) { yj[tid] = sv.yv[(size_t)tile_j * T + tid]; yi[tid] = sv.yv[(size_t)tile_i * T + tid]; }
  const double* St = tile_ptr(sv, slot);
  for (int e = tid; e < T * T; e += 256) tile[(e / T) * TP + e % T] = St[e];
  __syncthreads();
  if (r >= T) return;
  if (tile_i == tile_j) {   // a diagonal tile through its lower triangle (what the factorisation reads); the rhs enters here
    double s = 0.0, a = 0.0;
    for (int c = 12 * q; c < 12 * q + 12; ++c) { const double v = tile[max(r, c) * TP + min(r, c)]; s += v * yj[c]; a += fabs(v) * fabs(yj[c]); }
    s = quad_sum(s); a = quad_sum(a);
    if (q == 0) { const double b = b_rhs[(size_t)tile_j * T + r]; atomicAdd(res + (size_t)tile_j * T + r, b - s); atomicAdd(den + (size_t)tile_j * T + r, fabs(b) + a); }
    return;
  }
  double s = 0.0, a = 0.0, st = 0.0, at = 0.0;
  for (int c = 12 * q; c < 12 * q + 12; ++c) {
    const double v = tile[r * TP + c]; s += v * yj[c]; a += fabs(v) * fabs(yj[c]);          // row r of tile (i, j) against y_j
    const double w = tile[c * TP + r]; st += w * yi[c]; at += fabs(w) * fabs(yi[c]);        // column r of it against y_i
  }
  s = quad_sum(s); a = quad_sum(a); st = quad_sum(st); at = quad_sum(at);
  if (q == 0) {
    atomicAdd(res + (size_t)tile_i * T + r, -s); atomicAdd(den + (size_t)tile_i * T + r, a);
    atomicAdd(res + (size_t)tile_j * T + r, -st); atomicAdd(den + (size_t)tile_j * T + r, at);
  }
}
// flag = 1 when some |res_t| exceeds tol * den_t (NaN included) although no pivot failed; res / den are zeroed for the next solve.
// The flag is STICKY: a clean solve leaves it alone, so that several solves between two host reads (the free interFrameRatio's
// second right-hand side, the columns of a covariance block) cannot mask each other; the host clears it before the first one.
__global__ __launch_bounds__(1024) void chol_residual_check_kernel(const SolverDev sv, double* res, double* den, double tol, double* flag, const uint8_t* __restrict__ row_mine) {
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  bool bad = false;
  for (int64_t t = threadIdx.x; t < sv.npad; t += 1024) {
    const double rr = fabs(res[t]), d = den[t];
    if (!(rr <= tol * d) && !(rr == 0.0) && (!row_mine || row_mine[t / T])) bad = true;
    res[t] = 0.0; den[t] = 0.0;
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (threadIdx.x == 0 && s_bad && *sv.chol_fail == 0) *flag = 1.0;   // a failed pivot is reported through chol_fail, not here
}

}  // namespace

hipError_t launch_chol_verify(const SolverDev& sv, const int32_t* slot_tiles, const double* b_rhs, double* res, double* den, double tol, double* flag, hipStream_t st, const uint8_t* row_mine) {
  hipLaunchKernelGGL(chol_residual_kernel, dim3(sv.nslots), dim3(256), 0, st, sv, slot_tiles, b_rhs, res, den);
  hipLaunchKernelGGL(chol_residual_check_kernel, dim3(1), dim3(1024), 0, st, sv, res, den, tol, flag, row_mine);
  return hipGetLastError();
}

}  // namespace rsba
