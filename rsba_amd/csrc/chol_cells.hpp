// Tile Cholesky, layer 1: the write-once cells its tasks hand each other through HBM, and the constants every layer shares.
// (Layers: chol_cells.hpp — tile_factor.hpp — chol_tasks.hpp — cholesky.hip.  Internal linkage throughout: unused pieces are dropped per translation unit.)
#pragma once
#include "solver_state.hpp"

namespace rsba {
namespace {

constexpr int T = kTile;
constexpr int TP = T + 1;   // LDS row pitch (doubles): odd pitch keeps column walks conflict-free

__device__ __forceinline__ double* tile_ptr(const SolverDev& sv, int slot) { return sv.S + (size_t)slot * (T * T); }
__device__ __forceinline__ double* factor_ptr(const SolverDev& sv, int slot) { return sv.Lf + (size_t)slot * (T * T); }

// Workgroup barrier that orders LDS traffic only.  Everything the waves of a workgroup hand each other here goes through
// LDS; what they write to HBM (write-once cells, partial tiles) is for OTHER workgroups, which find it by polling.  A full
// __syncthreads() would also wait for those global stores — and for every prefetch still in flight — to drain (vmcnt(0)).
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ---- write-once cells ----------------------------------------------------------------------------------------------------
// Everything a task of the persistent driver hands to another one (factor tiles, partial tiles, W, z, y) is a WRITE-ONCE
// CELL: its array is filled with an "empty" bit pattern before the launch, a producer stores each double exactly once, and
// a consumer that reads "empty" reads again — the data is its own flag, there are no others ("The Cholesky").
//   * Empty is all ones — what hipMemset(0xFF) leaves; as a double it is a NaN with a payload that no arithmetic produces
//     (a failed factorisation yields the canonical NaN, which counts as data: no task can hang).  The pivot messages of
//     the tile factorisation in LDS (tile_factor.hpp) use the same pattern.
//   * Cells move through agent-coherent accesses (ld<true> / st<true>): relaxed agent-scope atomic loads / stores of the
//     individual doubles, which gfx950 issues with sc1 (the L2 of the other XCDs is not coherent with ours; sc1 accesses go
//     to the memory side), so neither side needs cache maintenance.  The level driver (DAG = false) uses plain loads and
//     stores: its launches order everything.
//   * Every access to HBM says so explicitly (address space 1: gl / ld / st).  The persistent kernel reads its pointers out of
//     a device copy of the plan, so the compiler cannot tell where they point: left alone it issues FLAT loads, which count
//     on the LDS counter (lgkmcnt) as well — and every LDS wait and LDS-only barrier of a task then also waits for the
//     prefetches in flight.
//   * Waiting costs memory traffic: a task that found a group of cells incomplete does not keep re-reading the whole group
//     (hundreds of claimed-but-waiting tasks doing that saturate the memory system) — it watches ONE cell of the missing
//     input, with a pause between looks (watch_cell), and reads the group again once that cell has landed.
//   * Cached first looks.  A task's FIRST look at an operand tile (Frag::load<DAG, false>) or at W_j
//     (times_inverse_transposed) is an ordinary load (gl), served by this XCD's L2 (and the CU's L1) when they hold the line:
//     a factor tile is an operand of ~12 products in as many tasks, a W_j of a dozen SUB tasks, and only the first of them
//     has to go to the fabric.  A cell is written once, so what such a load returns is either the cell's final value or
//     "empty" — possibly a STALE empty (a copy cached before the producer's store, which went to the memory side); the
//     caller checks every double it consumes, waits for an incomplete input on the memory side and reads it again
//     COHERENTLY.  Lines of an EARLIER solve cannot be met: the two sets of cells alternate from solve to solve; a set is
//     re-armed (hipMemsetAsync on the arming stream) while the OTHER set's kernel runs, and a kernel waits for its own set's
//     re-arming through an event.  A kernel dispatch packet carries an acquire fence of agent scope or wider (HSA AQL
//     header, set by the HIP runtime for every launch): the L2 of every XCD the launch lands on is invalidated before the
//     first wave runs, so a FILLED line of this set from two solves ago cannot be in any L2 when the kernel starts, and
//     inside the kernel a line of this set can only have been cached empty or final.  Should a runtime ever launch without
//     that fence, the result is a wrong factor — which the residual check that follows every DAG solve (verify_dag, on by
//     default: solver.hip, kernels_chol_verify.hip) catches and repairs on the level schedule; tools/dag_stress.py
//     alternates both sets for thousands of solves, tools/l2_boundary_probe.hip probes the invalidation itself.
#define RSBA_GLOBAL __attribute__((address_space(1)))
template <class V> __device__ __forceinline__ V gl(const V* p) { return *(const RSBA_GLOBAL V*)p; }
template <bool DAG> __device__ __forceinline__ double ld(const double* p) {
  if (DAG) return __hip_atomic_load((const RSBA_GLOBAL double*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return gl(p);
}
template <bool DAG> __device__ __forceinline__ void st(double* p, double v) {
  if (DAG) __hip_atomic_store((RSBA_GLOBAL double*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *(RSBA_GLOBAL double*)p = v;
}
__device__ __forceinline__ bool filled(double v) { return __double_as_longlong(v) != -1ll; }

// Instrumented build only (-DRSBA_TEST_HOOKS, librsba_amd_hooks.so): what the persistent kernel reads COHERENTLY (from the memory side), by
// kind — tools/chol_poll_split.py sets it beside the fabric-read counter of a rocprofv3 pass.  Wave-level events, one atomic per event by lane 0.
//   [0] looks at a watched cell (one 64-byte line each)      [1] of them: looks that found the cell still empty
//   [2] operand fragments read again coherently (9 x 512 B)   [3] W row blocks / tiles read (12 or 24 x 512 B)   [4] of them: reads that came back incomplete
#ifdef RSBA_TEST_HOOKS
__device__ unsigned long long g_chol_coherent[8];
#define CHOL_COUNT(k, n) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_chol_coherent[k], (unsigned long long)(n)); } while (0)
#else
#define CHOL_COUNT(k, n) do { } while (0)
#endif
template <bool DAG>
__device__ __forceinline__ void watch_cell(const double* p) {
  if (!DAG) return;
  for (;;) {
    const bool there = filled(ld<true>(p));
    CHOL_COUNT(0, 1);
    if (there) break;
    CHOL_COUNT(1, 1);
    __builtin_amdgcn_s_sleep(8);
  }
}

// RSBA_CHOL_TRACE: where the running task logs its time stamps (null = off; set by the driver that claimed the task).  Slots of a
// task's record: solver_state.hpp, CholPlan::trace.
__shared__ long long* s_trace_slot;
#define CHOL_STAMP(k) do { if (DAG && tid == 0 && s_trace_slot) s_trace_slot[k] = wall_clock64(); } while (0)
// a waiting task marks when its last late input arrived
__device__ __forceinline__ void note_late_input() { if (threadIdx.x == 0 && s_trace_slot) s_trace_slot[2] = wall_clock64(); }

}  // namespace
}  // namespace rsba
