// NOTE (end of round 3): this file times the code as the compiler lays it out for THESE kernels; inside the solver's persistent kernel
// the same source is laid out, allocated and fetched differently (tools/chol_trace.py is the measurement that counts): the rolled
// three-block loop of factor_invert_tile made the tile 0.9 us faster there (8.3 -> 7.4 us) and 1.2 us slower here.
// Micro-benchmark + check of the serial core of the tile Cholesky (rsba_amd/csrc/tile_factor.hpp): W = chol(D)^-1 of one
// 48 x 48 tile by ONE 256-thread workgroup — the step that sits 42 times on the critical path of a 1k-camera solve.
// Variants: the library's MFMA-pivot LDL^T form, and the earlier forms of tools/tile_factor_baselines.hpp (the lane-per-row blocked
// potrf + blocked triangular inverse of round 1, round 2's second wave).
// Checks |W D W^T - I| and |W - W_ref| against a host factorisation, prints microseconds per tile (wall_clock64, 100 MHz).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics tools/tile_factor_bench.hip -o tools/tile_factor_bench
// tile_factor_bench --check IN OUT times nothing: it runs the two forms the library runs (plain, and publishing W as diag_factor does) on
// every tile of a file, one workgroup per tile in ONE launch, and writes ok and W of each back (check_kernel and run_check below;
// tests/test_gpu_tile_factor.py holds them against the extended-precision reference of tests/tile_factor_reference.py).
#include "tile_factor_baselines.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace rsba {
namespace {

template <int VARIANT>
__global__ __launch_bounds__(256, 2) void tile_kernel(const double* __restrict__ Din, double* __restrict__ Wout, long long* ticks, int reps, long long* stamps) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x;
  double* D = smem; double* Wl = smem + kBuf; double* Tm = smem + 2 * kBuf; double* Lp = smem + 3 * kBuf;
  double* dinv = smem + kSpareVec;
  long long total = 0;
  for (int it = 0; it < reps; ++it) {
    for (int e = tid; e < T * T; e += 256) { const int r = e / T, c = e % T; D[r * TP + c] = (c <= r) ? Din[e] : 0.0; }
    arm_pivot_messages(smem, tid);
    __syncthreads();
    const long long t0 = wall_clock64();
    if (VARIANT == 0) {
      potrf_blocked(D, tid);
      if (tid < T) dinv[tid] = 1.0 / D[tid * TP + tid];
      lds_barrier();
      invert_lower_blocked(D, dinv, Wl, Tm, tid);
    } else {
      if (VARIANT == 2) factor_invert_tile<true>(D, Wl, Tm, Lp, tid, stamps);   // 2: with phase stamps (every repetition: warm code)
      else if (VARIANT == 3) factor_invert_tile<false, false, FollowMfma>(D, Wl, Tm, Lp, tid);   // 3: round 2's second wave (rank-1 MFMAs on the identity)
      else if (VARIANT == 4) factor_invert_tile<false, true>(D, Wl, Tm, Lp, tid, nullptr, Wout + T * T);   // 4: as the persistent driver runs it — W published to write-once cells by row blocks
      else factor_invert_tile(D, Wl, Tm, Lp, tid);
    }
    const long long t1 = wall_clock64();
    total += t1 - t0;
    __syncthreads();
  }
  for (int e = tid; e < T * T; e += 256) { const int r = e / T, c = e % T; Wout[e] = (c <= r) ? Wl[r * TP + c] : 0.0; }
  if (tid == 0) ticks[0] = total;
}


// --check: workgroup b factors tile b twice, as the library does and with nothing of tools/tile_factor_baselines.hpp —
//   form 0  factor_invert_tile<false, false>: W stays in LDS;
//   form 1  factor_invert_tile<false, true> with wout, as diag_factor (chol_tasks.hpp) calls it: W also leaves by row blocks to Wout + 2 T T.
// Per tile Wout holds three T x T copies: W of form 0 and of form 1 read out of LDS, and what form 1 published (the host filled it with
// the empty pattern).  The LDS copies are read the way publish_rows reads them — the 16-blocks on and below the diagonal; the blocks above
// it are not the function's to write — from a W buffer that held the empty pattern in every cell before the call.  ok is tid 0's (wave 0's), as in diag_factor.
__global__ __launch_bounds__(256, 2) void check_kernel(const double* __restrict__ Din, double* __restrict__ Wout, int* __restrict__ okout) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x;
  double* D = smem; double* Wl = smem + kBuf; double* Tm = smem + 2 * kBuf; double* Lp = smem + 3 * kBuf;
  const double* Dt = Din + (size_t)blockIdx.x * (T * T);
  double* Wt = Wout + (size_t)blockIdx.x * (3 * T * T);
  for (int form = 0; form < 2; ++form) {
    for (int e = tid; e < T * T; e += 256) { const int r = e / T, c = e % T; D[r * TP + c] = (c <= r) ? Dt[e] : 0.0; }
    for (int e = tid; e < kBuf; e += 256) Wl[e] = __longlong_as_double(-1ll);
    arm_pivot_messages(smem, tid);
    __syncthreads();
    const bool ok = form == 0 ? factor_invert_tile<false, false>(D, Wl, Tm, Lp, tid) : factor_invert_tile<false, true>(D, Wl, Tm, Lp, tid, nullptr, Wt + 2 * T * T);
    if (tid == 0) okout[2 * blockIdx.x + form] = ok ? 1 : 0;
    for (int e = tid; e < T * T; e += 256) { const int r = e / T, c = e % T; Wt[form * T * T + e] = (c < 16 * (r / 16 + 1)) ? Wl[r * TP + c] : 0.0; }
    __syncthreads();
  }
}

// the two waves of one 16 x 16 diagonal block step on their own: MODE 0 both, 1 the eliminating wave alone, 2 the following wave alone
// on messages that are already there.  FW = which wave of the workgroup follows.
// What slows the following wave down when the eliminating wave runs beside it (both: 366 cycles per pivot; alone on ready messages: 204)?
// A STAND-IN for the eliminating wave posts the same messages (taken from a first, real elimination) at the eliminating wave's pace —
// with nothing but s_sleep between them (PACER 1), or with the real wave's sixteen dependent rank-1 MFMAs on a dummy block in between
// (PACER 2): if the follower keeps pace with 1 and not with 2, it is the matrix pipe's traffic that costs it, not the waiting.
template <int PACER>
__global__ __launch_bounds__(256) void paced_kernel(const double* __restrict__ Din, double* __restrict__ out, long long* t, int reps, int sleep_units) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double* D = smem; double* msg = smem;
  double* saved = smem + 4 * kBuf + 64;   // [16][64] the messages of a real elimination (behind the task's buffers)
  for (int e = tid; e < T * T; e += 256) { const int r = e / T, c = e % T; D[r * TP + c] = (c <= r) ? Din[e] : 0.0; }
  __syncthreads();
  const dbl4 d0 = load_sym16(D, 0, lane);
  arm_pivot_messages(smem, tid);
  __syncthreads();
  if (wave == 0) ldl16_eliminate(d0, msg, lane);
  __syncthreads();
  if (wave == 0) for (int jj = 0; jj < 16; ++jj) saved[jj * 64 + lane] = msg[msg_off(jj) + lane];
  __syncthreads();
  dbl4 acc = {0, 0, 0, 0}, dummy = d0;
  long long lead = 0, foll = 0, total = 0;
  for (int it = 0; it < reps; ++it) {
    arm_pivot_messages(smem, tid);
    __syncthreads();
    const long long c0 = clock64();
    if (wave == 0) {
      for (int jj = 0; jj < 16; ++jj) {
        if (PACER == 2) dummy = __builtin_amdgcn_mfma_f64_16x16x4f64(1e-30 * dummy[0], 1e-30, dummy, 0, 0, 0);   // (a dependent chain, like the real wave's)
        for (int u = 0; u < sleep_units; ++u) __builtin_amdgcn_s_sleep(1);
        msg[msg_off(jj) + lane] = saved[jj * 64 + lane];
      }
      lead += clock64() - c0;
    }
    if (wave == 1) { ldl16_follow_rows(msg, smem + kBuf, 0, lane); acc[0] += smem[kBuf + lane]; foll += clock64() - c0; }
    __syncthreads();
    total += clock64() - c0;
  }
  for (int v = 0; v < 4; ++v) out[tid * 4 + v] = acc[v] + dummy[v];
  if (tid == 0) { t[0] = lead; t[2] = total; }
  if (tid == 64) t[1] = foll;
}

template <int MODE, int FW, bool ROWS = false>
__global__ __launch_bounds__(256) void pair_kernel(const double* __restrict__ Din, double* __restrict__ out, long long* t, int reps, long long* stamps = nullptr) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double* D = smem; double* msg = smem;
  for (int e = tid; e < T * T; e += 256) { const int r = e / T, c = e % T; D[r * TP + c] = (c <= r) ? Din[e] : 0.0; }
  __syncthreads();
  const dbl4 d0 = load_sym16(D, 0, lane);
  dbl4 acc = {0, 0, 0, 0};
  long long lead = 0, foll = 0, total = 0;
  for (int it = 0; it < reps; ++it) {
    if (MODE != 2 || it == 0) arm_pivot_messages(smem, tid);
    __syncthreads();
    if (MODE == 2 && it == 0) { if (wave == 0) ldl16_eliminate(d0, msg, lane); __syncthreads(); }
    const long long c0 = clock64();
    const bool last = stamps && it == reps - 1;
    if (last && tid == 0) stamps[0] = c0;
    if (wave == 0 && MODE != 2) { dbl4 d = d0; asm volatile("" : "+v"(d)); const bool ok = ldl16_eliminate(d, msg, lane, last ? stamps + 1 : nullptr); acc[0] += ok; lead += clock64() - c0; }
    if (wave == FW && MODE != 1) {
      if (ROWS) { ldl16_follow_rows(msg, smem + kBuf, 0, lane, last ? stamps + 17 : nullptr); acc[0] += smem[kBuf + lane]; } else acc += ldl16_follow(msg, lane);
      foll += clock64() - c0;
    }
    __syncthreads();
    total += clock64() - c0;
  }
  for (int v = 0; v < 4; ++v) out[tid * 4 + v] = acc[v];
  if (tid == 0) { t[0] = lead; t[2] = total; }
  if (tid == 64 * FW) t[1] = foll;
}

}  // namespace
}  // namespace rsba

// IN: int32 n, then n tiles of T x T doubles (row-major, symmetric; the lower triangle is read).  OUT: int32 n, then per tile
// { int32 ok of form 0, int32 ok of form 1, W of form 0, W of form 1, the published copy of form 1 } — T x T doubles each, as they lie in HBM.
#define CHECK_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "tile_factor_bench --check: %s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)
static int run_check(const char* in_path, const char* out_path) {
  using namespace rsba;
  constexpr size_t tile = (size_t)T * T;
  std::FILE* f = std::fopen(in_path, "rb");
  if (!f) { std::fprintf(stderr, "tile_factor_bench --check: cannot open %s\n", in_path); return 1; }
  int32_t n = 0;
  if (std::fread(&n, sizeof n, 1, f) != 1 || n < 1 || n > 4096) { std::fprintf(stderr, "tile_factor_bench --check: %s: bad tile count\n", in_path); std::fclose(f); return 1; }
  std::vector<double> A(n * tile);
  const bool whole = std::fread(A.data(), sizeof(double), A.size(), f) == A.size() && std::fgetc(f) == EOF;
  std::fclose(f);
  if (!whole) { std::fprintf(stderr, "tile_factor_bench --check: %s does not hold exactly %d tiles\n", in_path, (int)n); return 1; }
  double *dA = nullptr, *dW = nullptr; int* dOk = nullptr;
  CHECK_HIP(hipMalloc(&dA, n * tile * sizeof(double)));
  CHECK_HIP(hipMalloc(&dW, 3 * n * tile * sizeof(double)));
  CHECK_HIP(hipMalloc(&dOk, 2 * n * sizeof(int)));
  CHECK_HIP(hipMemcpy(dA, A.data(), n * tile * sizeof(double), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemset(dW, 0xFF, 3 * n * tile * sizeof(double)));   // the empty pattern of chol_cells.hpp: a cell nobody wrote shows afterwards
  CHECK_HIP(hipMemset(dOk, 0xFF, 2 * n * sizeof(int)));
  const size_t lds = kCholLds * sizeof(double);
  CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(check_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(check_kernel, dim3(n), dim3(256), lds, 0, dA, dW, dOk);
  CHECK_HIP(hipGetLastError());
  CHECK_HIP(hipDeviceSynchronize());
  std::vector<double> W(3 * n * tile); std::vector<int32_t> ok(2 * n);
  CHECK_HIP(hipMemcpy(W.data(), dW, W.size() * sizeof(double), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(ok.data(), dOk, ok.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  CHECK_HIP(hipFree(dA)); CHECK_HIP(hipFree(dW)); CHECK_HIP(hipFree(dOk));
  f = std::fopen(out_path, "wb");
  if (!f) { std::fprintf(stderr, "tile_factor_bench --check: cannot write %s\n", out_path); return 1; }
  bool written = std::fwrite(&n, sizeof n, 1, f) == 1;
  for (int b = 0; b < n && written; ++b) written = std::fwrite(&ok[2 * b], sizeof(int32_t), 2, f) == 2 && std::fwrite(&W[3 * b * tile], sizeof(double), 3 * tile, f) == 3 * tile;
  written = (std::fclose(f) == 0) && written;
  if (!written) { std::fprintf(stderr, "tile_factor_bench --check: short write to %s\n", out_path); return 1; }
  return 0;
}

int main(int argc, char** argv) {
  using namespace rsba;
  if (argc == 4 && std::strcmp(argv[1], "--check") == 0) return run_check(argv[2], argv[3]);
  if (argc != 1) { std::fprintf(stderr, "usage: tile_factor_bench [--check IN OUT]\n"); return 2; }
  constexpr int n = T;
  // SPD tile with the conditioning of a damped reduced camera block: A = B B^T + 0.1 I
  std::vector<double> B(n * n), A(n * n, 0.0), L(n * n, 0.0), Wref(n * n, 0.0);
  unsigned long long st = 12345;
  auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return ((st >> 11) * (1.0 / 9007199254740992.0)) - 0.5; };
  for (double& b : B) b = rnd();
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double s = 0; for (int k = 0; k < n; ++k) s += B[i * n + k] * B[j * n + k]; A[i * n + j] = s + (i == j ? 0.1 : 0.0); }
  for (int j = 0; j < n; ++j) {   // host Cholesky and inverse of the factor
    double d = A[j * n + j]; for (int k = 0; k < j; ++k) d -= L[j * n + k] * L[j * n + k];
    L[j * n + j] = std::sqrt(d);
    for (int i = j + 1; i < n; ++i) { double s = A[i * n + j]; for (int k = 0; k < j; ++k) s -= L[i * n + k] * L[j * n + k]; L[i * n + j] = s / L[j * n + j]; }
  }
  for (int c = 0; c < n; ++c) for (int i = c; i < n; ++i) { double s = (i == c) ? 1.0 : 0.0; for (int k = c; k < i; ++k) s -= L[i * n + k] * Wref[k * n + c]; Wref[i * n + c] = s / L[i * n + i]; }
  double *dA, *dW; long long *dT, *dS;
  hipMalloc(&dS, 64 * 8); hipMemset(dS, 0, 64 * 8);
  hipMalloc(&dA, sizeof(double) * n * n); hipMalloc(&dW, 2 * sizeof(double) * n * n); hipMalloc(&dT, 8);
  hipMemcpy(dA, A.data(), sizeof(double) * n * n, hipMemcpyHostToDevice);
  const size_t lds = kCholLds * sizeof(double);
  hipFuncSetAttribute(reinterpret_cast<const void*>(tile_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipFuncSetAttribute(reinterpret_cast<const void*>(tile_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipFuncSetAttribute(reinterpret_cast<const void*>(tile_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipFuncSetAttribute(reinterpret_cast<const void*>(tile_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipFuncSetAttribute(reinterpret_cast<const void*>(tile_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const int reps = 2000;
  {   // what the instruction cache costs: the factorisation is ~20 KB of straight-line code that a DIAG task of the solver runs ONCE
    auto once = [&](int r, const char* what) {
      long long ticks = 0;
      hipLaunchKernelGGL(tile_kernel<1>, dim3(1), dim3(256), lds, 0, dA, dW, dT, r, dS); (void)hipDeviceSynchronize();
      (void)hipMemcpy(&ticks, dT, 8, hipMemcpyDeviceToHost);
      std::printf("MFMA-pivot LDL^T, %s: %.3f us for %d tile(s)\n", what, ticks * 0.01, r);
    };
    once(1, "first launch of the process, one tile (cold code)");
    once(1, "second launch, one tile");
    once(2, "third launch, two tiles");
    once(3, "fourth launch, three tiles");
  }
  for (int variant = 0; variant < 5; ++variant) {
    for (int pass = 0; pass < 2; ++pass) {   // first pass warms up
      if (variant == 0) hipLaunchKernelGGL(tile_kernel<0>, dim3(1), dim3(256), lds, 0, dA, dW, dT, reps, dS);
      else if (variant == 1) hipLaunchKernelGGL(tile_kernel<1>, dim3(1), dim3(256), lds, 0, dA, dW, dT, reps, dS);
      else if (variant == 2) hipLaunchKernelGGL(tile_kernel<2>, dim3(1), dim3(256), lds, 0, dA, dW, dT, reps, dS);
      else if (variant == 3) hipLaunchKernelGGL(tile_kernel<3>, dim3(1), dim3(256), lds, 0, dA, dW, dT, reps, dS);
      else hipLaunchKernelGGL(tile_kernel<4>, dim3(1), dim3(256), lds, 0, dA, dW, dT, reps, dS);
      hipDeviceSynchronize();
    }
    std::vector<double> W(n * n); long long ticks = 0;
    hipMemcpy(W.data(), dW, sizeof(double) * n * n, hipMemcpyDeviceToHost); hipMemcpy(&ticks, dT, 8, hipMemcpyDeviceToHost);
    double err_id = 0, err_ref = 0, wmax = 0;
    std::vector<double> WA(n * n, 0.0);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double s = 0; for (int k = 0; k < n; ++k) s += W[i * n + k] * A[k * n + j]; WA[i * n + j] = s; }
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
      double s = 0; for (int k = 0; k < n; ++k) s += WA[i * n + k] * W[j * n + k];
      err_id = std::fmax(err_id, std::fabs(s - (i == j ? 1.0 : 0.0)));
      err_ref = std::fmax(err_ref, std::fabs(W[i * n + j] - Wref[i * n + j])); wmax = std::fmax(wmax, std::fabs(Wref[i * n + j]));
    }
    std::printf("%s: %.3f us per tile (%d reps), |W A W^T - I| = %.2e, |W - W_host| = %.2e (|W| = %.2e), %s\n",
                variant == 0 ? "lane-per-row potrf + blocked inverse" : variant == 1 ? "MFMA-pivot LDL^T, W by rows (round 3)" : variant == 2 ? "  the same with phase stamps        " : variant == 3 ? "MFMA-pivot LDL^T, W by MFMAs (round 2)" : "  round 3 + W published by row blocks ", ticks * 0.01 / reps, reps, err_id, err_ref, wmax,
                hipGetErrorString(hipGetLastError()));
  }
  {
    double* dO; long long* dP; (void)hipMalloc(&dO, 256 * 4 * 8); (void)hipMalloc(&dP, 32);
    auto run_pair = [&](auto kern, const char* name) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      long long h[3];
      for (int pass = 0; pass < 2; ++pass) { hipLaunchKernelGGL(kern, dim3(1), dim3(256), lds, 0, dA, dO, dP, reps, (long long*)nullptr); (void)hipDeviceSynchronize(); }
      (void)hipMemcpy(h, dP, sizeof h, hipMemcpyDeviceToHost);
      std::printf("%-48s eliminating wave %7.1f  following wave %7.1f  both + barrier %7.1f ticks per 16-pivot block\n", name, h[0] / (double)reps, h[1] / (double)reps, h[2] / (double)reps);
    };
    run_pair(pair_kernel<1, 1>, "eliminating wave alone");
    run_pair(pair_kernel<2, 1>, "following wave alone (messages already there)");
    run_pair(pair_kernel<0, 1>, "both, wave 1 follows");
    run_pair(pair_kernel<0, 2>, "both, wave 2 follows");
    run_pair(pair_kernel<0, 3>, "both, wave 3 follows");
    run_pair(pair_kernel<2, 1, true>, "W by rows: following wave alone (messages there)");
    run_pair(pair_kernel<0, 1, true>, "W by rows: both, wave 1 follows");
    for (int sl : {0, 1, 2, 3, 4}) {
      auto run_paced = [&](auto kern, const char* name) {
        const size_t lds2 = lds + (64 + 16 * 64) * sizeof(double);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
        long long h[3];
        for (int pass = 0; pass < 2; ++pass) { hipLaunchKernelGGL(kern, dim3(1), dim3(256), lds2, 0, dA, dO, dP, reps, sl); (void)hipDeviceSynchronize(); }
        (void)hipMemcpy(h, dP, sizeof h, hipMemcpyDeviceToHost);
        std::printf("%-48s posting wave %7.1f  following wave %7.1f  both + barrier %7.1f ticks per 16-pivot block  (%d x s_sleep 1 per pivot)\n", name, h[0] / (double)reps, h[1] / (double)reps, h[2] / (double)reps, sl);
      };
      run_paced(paced_kernel<1>, "stand-in posts ready messages, sleeps between");
      run_paced(paced_kernel<2>, "stand-in posts ready messages + dependent MFMAs");
    }
    {   // when each pivot message is posted (eliminating wave), seen, and its row stored (following wave): the last repetition of the pair above
      long long* dQ; (void)hipMalloc(&dQ, 128 * 8); (void)hipMemset(dQ, 0, 128 * 8);
      hipLaunchKernelGGL((pair_kernel<0, 1, true>), dim3(1), dim3(256), lds, 0, dA, dO, dP, 50, dQ); (void)hipDeviceSynchronize();
      long long q[128]; (void)hipMemcpy(q, dQ, sizeof q, hipMemcpyDeviceToHost);
      std::printf("pivot k: message posted | seen | next look + multipliers requested | updates of pivot k done | row k stored (shader cycles since the block started)\n");
      for (int k = 0; k < 16; ++k) std::printf("  %2d: %6lld | %6lld | %6lld | %6lld | %6lld\n", k, q[1 + k] - q[0], q[17 + 4 * k] - q[0], q[17 + 4 * k + 1] - q[0], q[17 + 4 * k + 2] - q[0], q[17 + 4 * k + 3] - q[0]);
    }
  }
  long long hs[64]; hipMemcpy(hs, dS, sizeof hs, hipMemcpyDeviceToHost);
  std::printf("phases of the last MFMA-pivot tile (clock64 ticks since entry; pairs = before / after each barrier):");
  for (int k = 1; k < 13; ++k) std::printf(" %lld", hs[k] - hs[0]);
  std::printf("\n");
  return 0;
}
