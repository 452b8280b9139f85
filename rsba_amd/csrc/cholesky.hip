// K6  reduced camera system  S y = rhs  by a tile-sparse Cholesky factorisation, fp64.
//
// Replaces the CHOLMOD sparse Cholesky behind Ceres' SPARSE_SCHUR (reference call site
// /root/reference/src/rsba/CeresHandler.h:403,419).  S (lower triangle) is a grid of 48x48 tiles; the
// symbolic phase (host, once per problem) finds the tiles that are structurally non-zero after fill-in
// and only those are stored — packed back to back in HBM (tile slot s at S + s*48*48, row-major), which is
// also the buffer the multi-GPU exchange all-reduces.  rsba's problems are video:
// frames only share points with frames a few dozen positions away, so S is block-banded, fill stays
// inside the band, and the factorisation is O(n b^2) instead of O(n^3).
//
// A band factored column after column is a serial chain of ~n/48 dependent steps (250 at 1k cameras),
// each a few tens of microseconds of latency: the GPU idles.  So the host reorders the tile columns by
// nested dissection (BFS-level separators cut the band into independent segments), computes the levels of
// the resulting elimination structure, and the factorisation runs as a DAG of tile tasks in one persistent
// kernel (below); the forward solve rides along, the backward solve walks the tree back down in the same launch.
// The reduced system S itself is left untouched: the factor's sub-diagonal tiles go to their own array (Lf).
// 1k cameras: ~42 levels instead of 250 steps.
//
// Layer 4 of four: the drivers that run the task bodies of chol_tasks.hpp (over tile_factor.hpp, over the write-once cells of
// chol_cells.hpp) in this one translation unit, and their launchers.  Two kinds of driver run the same bodies:
//   * persistent (chol_dag_kernel, chol_solve_kernel) — ONE launch per solve.  Workgroups draw tickets from a global counter
//     over the topologically sorted task list.  A claimed task only waits for tasks with smaller tickets, which are claimed
//     by running workgroups, so progress never depends on how many workgroups are resident.  No flags: inputs are found by
//     polling write-once cells (9 us less per level of the dependency chain than release / flag / acquire hand-offs).
//   * by level (chol_level_kernel, chol_solve_level_kernel) — one launch per (level, kind), no waiting at all: the schedule
//     the persistent drivers are tested against bit for bit (RSBA_CHOL_LEVELS=1) and, after a failed residual check
//     (kernels_chol_verify.hip), fall back to.
#include "chol_tasks.hpp"

namespace rsba {
namespace {

// one launch per (level, kind): items first .. first + gridDim.x of one kind
__global__ __launch_bounds__(256) void chol_level_kernel(const SolverDev sv, const CholPlan pl, int kind, int first) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  run_task<false>(sv, pl, kind, first + blockIdx.x, smem, threadIdx.x);
}

// the whole factorisation + both triangular solves in one persistent launch
__global__ __launch_bounds__(256, 2) void chol_dag_kernel(const DagArgs* __restrict__ args) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int s_ticket;
  const int tid = threadIdx.x;
  const CholPlan& pl = args->pl;
  if (lm_stopped(args->sv.ctl)) return;   // (device-side trust region: the solve is over, iterations enqueued ahead fall through)
  for (;;) {
    lds_barrier();   // the previous task's LDS is free, s_ticket has been read by everyone
    if (tid == 0) {
      const int tk = (int)__hip_atomic_fetch_add(pl.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_ticket = tk;
      s_trace_slot = (pl.trace && tk < pl.ntasks) ? pl.trace + 8 * (size_t)tk : nullptr;
      if (s_trace_slot) { s_trace_slot[0] = blockIdx.x; s_trace_slot[1] = s_trace_slot[2] = wall_clock64(); }
    }
    lds_barrier();
    const int t = s_ticket;
    if (t >= pl.ntasks) {
      // The last workgroup to leave re-arms the ticket counters for the next launch (a 16-byte fill per solve was a launch of its
      // own: ~6 us of kernel boundary on a solve of a few hundred): counter [3] counts the leavers.
      if (tid == 0 && __hip_atomic_fetch_add(pl.ticket + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
        __hip_atomic_store(pl.ticket + 0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pl.ticket + 3, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      return;
    }
    // every task recomputes what it derives from the thread index: left alone, the compiler hoists dozens of per-thread LDS
    // offsets out of this loop, keeps them live across all task bodies and spills them to scratch — whose reloads (vmcnt)
    // then stall on every prefetch in flight
    int task_tid = tid;
    asm volatile("" : "+v"(task_tid));
    run_task<true>(args->sv, pl, gl(pl.tasks + 2 * t), gl(pl.tasks + 2 * t + 1), smem, task_tid);
    if (tid == 0 && s_trace_slot) s_trace_slot[7] = wall_clock64();
  }
}

// ---- one more right-hand side through a finished factorisation -----------------------------------------------------
// S v = b2 with the factor tiles and the W_j the last solve left (the free interFrameRatio's border column, the columns of a
// covariance block): forward tasks z_j = W_j (b2_j - sum_k L_jk z_k) in the order of the DIAG items, then the BACK tasks of the
// factorisation on z2 / y2 — one persistent launch over write-once z / y cells of its own, no tile product anywhere.
__global__ __launch_bounds__(256) void chol_solve_kernel(const DagArgs* __restrict__ args, const double* __restrict__ b2, double* zy2, unsigned int* ticket) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int s_ticket;
  const int tid = threadIdx.x;
  const CholPlan& pl = args->pl;
  const int nd = pl.ndiag;
  for (;;) {
    lds_barrier();
    if (tid == 0) { s_ticket = (int)__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); s_trace_slot = nullptr; }
    lds_barrier();
    const int t = s_ticket;
    if (t >= 2 * nd) return;
    int task_tid = tid;   // (as in chol_dag_kernel)
    asm volatile("" : "+v"(task_tid));
    if (t < nd) task_forward<true>(args->sv, pl, t, gl(pl.diag_ptr + t), gl(pl.diag_ptr + t + 1), b2, nullptr, zy2, smem, task_tid);
    else {
      SolverDev sv2 = args->sv;
      sv2.zv = zy2; sv2.yv = zy2 + sv2.npad; sv2.zv2 = nullptr;
      task_back<true>(sv2, pl, gl(pl.tasks + 2 * (pl.ntasks - 2 * nd + t) + 1), smem, task_tid);   // (the BACK tasks close the task list, in their order)
    }
  }
}

// the same tasks one launch per level (no polling): what the persistent form is checked against and falls back to
__global__ __launch_bounds__(256) void chol_solve_level_kernel(const SolverDev sv, const CholPlan pl, int backward, int first, const double* __restrict__ b2, double* zy2) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if (!backward) { const int d = first + blockIdx.x; task_forward<false>(sv, pl, d, pl.diag_ptr[d], pl.diag_ptr[d + 1], b2, nullptr, zy2, smem, threadIdx.x); }
  else {
    SolverDev sv2 = sv;
    sv2.zv = zy2; sv2.yv = zy2 + sv2.npad; sv2.zv2 = nullptr;
    task_back<false>(sv2, pl, first + blockIdx.x, smem, threadIdx.x);
  }
}

}  // namespace

hipError_t launch_chol_level(const SolverDev& sv, const CholPlan& pl, int kind, int first, int count, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  hipError_t e = allow_dynamic_lds(chol_level_kernel, kCholLds * sizeof(double));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(chol_level_kernel, dim3(count), dim3(256), kCholLds * sizeof(double), st, sv, pl, kind, first);
  return hipGetLastError();
}

// zy2: [2][npad] doubles (z | y of this right-hand side; y = the solution), ticket: one counter of the caller's
hipError_t launch_chol_solve(const SolverDev& sv, const CholPlan& pl, const DagArgs* device_args, const double* b2, double* zy2, unsigned int* ticket, int workgroups, hipStream_t st) {
  if (pl.ndiag <= 0) return hipSuccess;
  hipError_t e = allow_dynamic_lds(chol_solve_kernel, (size_t)84 * 1024);   // (one workgroup per CU, as the factorisation: polling waves do not share SIMDs with the waves they wait for)
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(zy2, 0xFF, 2 * (size_t)sv.npad * sizeof(double), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(ticket, 0, sizeof(unsigned int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(chol_solve_kernel, dim3(workgroups), dim3(256), (size_t)84 * 1024, st, device_args, b2, zy2, ticket);
  return hipGetLastError();
}

hipError_t launch_chol_solve_level(const SolverDev& sv, const CholPlan& pl, bool backward, int first, int count, const double* b2, double* zy2, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  hipError_t e = allow_dynamic_lds(chol_solve_level_kernel, kCholLds * sizeof(double));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(chol_solve_level_kernel, dim3(count), dim3(256), kCholLds * sizeof(double), st, sv, pl, backward ? 1 : 0, first, b2, zy2);
  return hipGetLastError();
}

hipError_t launch_chol_dag(const SolverDev& sv, const CholPlan& pl, const DagArgs* device_args, int workgroups, bool one_per_cu, hipStream_t st) {
  if (pl.ntasks <= 0) return hipSuccess;
  // The kernel needs 78 KB of LDS and would fit a CU twice — and two workgroups sharing a CU (polling waves on the SIMDs of the
  // waves they wait for) slow the solve down by orders of magnitude.  The production launch therefore asks for more than half
  // of a CU's 160 KB: the dispatcher cannot co-locate two of them, whatever else runs on the device.
  const size_t lds_bytes = one_per_cu ? (size_t)84 * 1024 : kCholLds * sizeof(double);
  static_assert(kCholLds * sizeof(double) <= (size_t)84 * 1024, "LDS map of the Cholesky tasks");
  hipError_t e = allow_dynamic_lds(chol_dag_kernel, lds_bytes);
  if (e != hipSuccess) return e;
  // (the ticket counters are zero: set so when the plan was made, and re-armed by the last workgroup of every launch; the caller has
  // re-armed the write-once cells: one memset over their common allocation, solver.hip)
  hipLaunchKernelGGL(chol_dag_kernel, dim3(workgroups), dim3(256), lds_bytes, st, device_args);
  return hipGetLastError();
}

}  // namespace rsba

#ifdef RSBA_TEST_HOOKS
// instrumented build only (not part of include/rsba_amd.h): the coherent-read counters of the persistent Cholesky kernel, since the last reset
extern "C" int32_t rsba_debug_chol_coherent(unsigned long long out[8], int32_t reset) {
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(rsba::g_chol_coherent), 8 * sizeof(unsigned long long)) != hipSuccess) return RSBA_ERR_HIP;
  if (reset) { const unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rsba::g_chol_coherent), zero, sizeof zero) != hipSuccess) return RSBA_ERR_HIP; }
  return RSBA_OK;
}
#endif
