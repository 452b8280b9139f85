// The RSBA_* environment switches of the solver's host side: the one place that reads them (with test_hooks.hpp, which this file
// goes through for the fault injections), and the moments at which they are read.  README.md, "Environment switches", is the table
// of what each one means; the measurements behind a default stay next to the code that uses it.
//   * when a handle's plan is built: PlanSwitches::read(), once per build_solver_impl, kept in Solver::sw for the handle's life;
//   * at every solve: SolveSwitches::read(), at the top of rsba_solve, kept in Solver::solve_sw;
//   * once per process: the *_override / device_cache_mb / rccl_lib_path readers, each behind a function-local static of its caller;
//   * at every call: chol_leaf_override() and debug_plan().
// Host only: no HIP header reaches this file (tile_order.hpp and the sources the host compiler builds include it).
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <string>

#include "test_hooks.hpp"

namespace rsba {

// ---- the parse rules: every switch is read through one of these ----
inline bool env_set(const char* name) { return std::getenv(name) != nullptr; }                                        // present, whatever its value ("=0" too)
inline bool env_is(const char* name, char c) { const char* e = std::getenv(name); return e && e[0] == c; }           // first character ('0': an on-by-default feature goes off; '1': an off-by-default one goes on)
inline std::optional<int> env_int(const char* name, int lo = INT_MIN, int hi = INT_MAX) {                            // a number clamped to [lo, hi]; unset: nothing
  const char* e = std::getenv(name);
  return e ? std::optional<int>(std::max(lo, std::min(hi, std::atoi(e)))) : std::nullopt;
}
inline std::optional<uint64_t> env_u64(const char* name) { const char* e = std::getenv(name); return e ? std::optional<uint64_t>(std::strtoull(e, nullptr, 10)) : std::nullopt; }
inline std::optional<std::string> env_path(const char* name) { const char* e = std::getenv(name); return e ? std::optional<std::string>(e) : std::nullopt; }   // set (even empty): the feature is on

// ---- at every call ----
inline bool debug_plan() { return env_set("RSBA_DEBUG_PLAN"); }                                       // handle create / destroy (capi.hip); a plan keeps its own (PlanSwitches)
inline std::optional<int> chol_leaf_override() { return env_int("RSBA_CHOL_LEAF", 2); }               // plan_leaf_size (tile_order.hpp): the plan and rsba_partition_points see the same, never cached

// ---- once per process (the caller's function-local static holds the value) ----
inline int sweep_points_override(int most) { const int v = env_int("RSBA_SWEEP_POINTS").value_or(0); return v >= 1 && v <= most ? v : 0; }   // 0: by scene size
inline int project_chunks_override() { const int v = env_int("RSBA_PROJECT_CHUNKS").value_or(0); return v >= 1 && v <= 64 ? v : 0; }        // 0: by scene size
inline bool cov_times_switch() { return env_is("RSBA_COV_TIMES", '1'); }
inline uint64_t device_cache_mb() { return env_u64("RSBA_DEVICE_CACHE_MB").value_or(2048); }
inline std::optional<std::string> rccl_lib_path() { return env_path("RSBA_RCCL_LIB"); }

// ---- when a handle's plan is built ----
struct PlanSwitches {
  static constexpr int kSchurBlockUnset = -1, kSchurPairMajor = 0;
  std::optional<int> plan_threads;               // RSBA_PLAN_THREADS, 1 .. 64; unset: by problem size
  bool keep_records = false;                     // RSBA_RECORDS=1
  bool records_alt = true;                       // RSBA_RECORDS_ALT=0 switches it off
  bool factored = true;                          // RSBA_FACTORED=0 switches it off
  bool plan_device = true;                       // RSBA_PLAN_DEVICE=0 switches it off
  bool listed_keys = false;                      // RSBA_PLAN_LISTED_KEYS set
  int schur_block = kSchurBlockUnset;            // RSBA_SCHUR_BLOCK: unset (default by size, may fall back to pair-major) / 0 pair-major / >= 16 points
  bool schur_linear = false;                     // RSBA_SCHUR_LINEAR=1
  int schur_variant = 0;                         // RSBA_SCHUR_VARIANT (4 / 5: instrumented build only)
  std::optional<std::string> schur_trace;        // RSBA_SCHUR_TRACE=<file>, written when the plan goes
  bool sharded = true;                           // RSBA_SHARDED=0 switches it off
  bool chol_fuse = true;                         // RSBA_CHOL_FUSE=0 switches it off
  int chol_tail = 2, chol_chunk = 12;            // RSBA_CHOL_TAIL >= 1, RSBA_CHOL_CHUNK >= tail (defaults: CholPlanOptions, chol_plan.hpp; tests/test_switches.py holds them equal)
  std::optional<int> chol_wgs;                   // RSBA_CHOL_WGS; the plan clamps it to its tasks and two per CU
  bool chol_verify = true;                       // RSBA_CHOL_VERIFY=0 switches it off
  bool chol_levels_before_solve = false;         // RSBA_CHOL_LEVELS=1 as the plan saw it: for covariance calls before any solve (then SolveSwitches::chol_levels)
  std::optional<std::string> chol_trace;         // RSBA_CHOL_TRACE=<file>, written when a solve ends
  bool no_fused_sweep = false;                   // RSBA_NO_FUSED_SWEEP set
  bool debug_plan = false;                       // RSBA_DEBUG_PLAN set
  // fault injection (test_hooks.hpp): false in the release library whatever the environment says
  bool test_fail_plan = false, test_fail_device_plan = false, test_chol_corrupt = false;   // RSBA_TEST_FAIL_PLAN / RSBA_TEST_FAIL_DEVICE_PLAN set, RSBA_CHOL_TEST_CORRUPT=1
  static PlanSwitches read();
};

// ---- at every solve ----
struct SolveSwitches {
  bool device_lm = true;                         // RSBA_DEVICE_LM=0 switches it off
  int lm_ahead = 0;                              // RSBA_LM_AHEAD, 0 .. ring - 2
  bool speculate = true;                         // RSBA_SPECULATE=0 switches it off
  bool chol_levels = false;                      // RSBA_CHOL_LEVELS=1 (rsba_solve ORs the option in)
  bool no_side_sweep = false;                    // RSBA_NO_SIDE_SWEEP set
  bool test_device_lm_off_on_this_rank = false;  // RSBA_DEVICE_LM_OFF_ON_THIS_RANK set (fault injection: as above)
  static SolveSwitches read(int ctl_ring);
};

// The two readers go through test_hook(), whose body depends on RSBA_TEST_HOOKS: they may be called from the translation units the
// Makefile builds both ways only (solver_plan.hip, solver.hip), or the instrumented library could link the release form.
inline PlanSwitches PlanSwitches::read() {
  PlanSwitches sw;
  sw.plan_threads = env_int("RSBA_PLAN_THREADS", 1, 64);
  sw.keep_records = env_is("RSBA_RECORDS", '1');
  sw.records_alt = !env_is("RSBA_RECORDS_ALT", '0');
  sw.factored = !env_is("RSBA_FACTORED", '0');
  sw.plan_device = !env_is("RSBA_PLAN_DEVICE", '0');
  sw.listed_keys = env_set("RSBA_PLAN_LISTED_KEYS");
  if (const auto v = env_int("RSBA_SCHUR_BLOCK")) sw.schur_block = *v > 0 ? std::max(16, *v) : kSchurPairMajor;
  sw.schur_linear = env_is("RSBA_SCHUR_LINEAR", '1');
  sw.schur_variant = env_int("RSBA_SCHUR_VARIANT").value_or(0);
  if (!kTestHooks && sw.schur_variant >= 4) sw.schur_variant = 0;
  sw.schur_trace = env_path("RSBA_SCHUR_TRACE");
  sw.sharded = !env_is("RSBA_SHARDED", '0');
  sw.chol_fuse = !env_is("RSBA_CHOL_FUSE", '0');
  sw.chol_tail = env_int("RSBA_CHOL_TAIL", 1).value_or(sw.chol_tail);
  sw.chol_chunk = env_int("RSBA_CHOL_CHUNK", sw.chol_tail).value_or(sw.chol_chunk);
  sw.chol_wgs = env_int("RSBA_CHOL_WGS");
  sw.chol_verify = !env_is("RSBA_CHOL_VERIFY", '0');
  sw.chol_levels_before_solve = env_is("RSBA_CHOL_LEVELS", '1');
  sw.chol_trace = env_path("RSBA_CHOL_TRACE");
  sw.no_fused_sweep = env_set("RSBA_NO_FUSED_SWEEP");
  sw.debug_plan = rsba::debug_plan();
  sw.test_fail_plan = test_hook("RSBA_TEST_FAIL_PLAN") != nullptr;
  sw.test_fail_device_plan = test_hook("RSBA_TEST_FAIL_DEVICE_PLAN") != nullptr;
  { const char* v = test_hook("RSBA_CHOL_TEST_CORRUPT"); sw.test_chol_corrupt = v && v[0] == '1'; }
  return sw;
}

inline SolveSwitches SolveSwitches::read(int ctl_ring) {
  SolveSwitches sw;
  sw.device_lm = !env_is("RSBA_DEVICE_LM", '0');
  sw.lm_ahead = env_int("RSBA_LM_AHEAD", 0, ctl_ring - 2).value_or(0);   // (a slot of the ring is written again only after the host has moved on from it)
  sw.speculate = !env_is("RSBA_SPECULATE", '0');
  sw.chol_levels = env_is("RSBA_CHOL_LEVELS", '1');
  sw.no_side_sweep = env_set("RSBA_NO_SIDE_SWEEP");
  sw.test_device_lm_off_on_this_rank = test_hook("RSBA_DEVICE_LM_OFF_ON_THIS_RANK") != nullptr;
  return sw;
}

}  // namespace rsba
