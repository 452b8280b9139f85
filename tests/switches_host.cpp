// What rsba_amd/csrc/switches.hpp makes of the environment this program is started in, as one JSON object on stdout: every field of
// PlanSwitches and SolveSwitches, chol_leaf_override(), debug_plan(), the once-per-process readers and — for the comparison with the
// defaults held in PlanSwitches — the defaults of CholPlanOptions (chol_plan.hpp).  argv[1] = slots of the LM control ring (the
// library passes Solver::kCtlRing).  tests/test_switches.py compiles it with and without -DRSBA_TEST_HOOKS.
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <string>

#include "../rsba_amd/csrc/chol_plan.hpp"
#include "../rsba_amd/csrc/switches.hpp"

namespace {
const char* b(bool v) { return v ? "true" : "false"; }
std::string opt_int(const std::optional<int>& v) { return v ? std::to_string(*v) : "null"; }
std::string opt_str(const std::optional<std::string>& v) { return v ? "\"" + *v + "\"" : "null"; }   // (the tests' paths need no escaping)
}  // namespace

int main(int argc, char** argv) {
  using namespace rsba;
  const int ring = argc > 1 ? std::atoi(argv[1]) : 4;
  const PlanSwitches p = PlanSwitches::read();
  const SolveSwitches s = SolveSwitches::read(ring);
  const CholPlanOptions o;
  std::printf("{\"plan\": {\"plan_threads\": %s, \"keep_records\": %s, \"records_alt\": %s, \"factored\": %s, \"plan_device\": %s, \"listed_keys\": %s, "
              "\"schur_block\": %d, \"schur_linear\": %s, \"schur_variant\": %d, \"schur_trace\": %s, \"sharded\": %s, \"chol_fuse\": %s, \"chol_tail\": %d, "
              "\"chol_chunk\": %d, \"chol_wgs\": %s, \"chol_verify\": %s, \"chol_levels_before_solve\": %s, \"chol_trace\": %s, \"no_fused_sweep\": %s, "
              "\"debug_plan\": %s, \"test_fail_plan\": %s, \"test_fail_device_plan\": %s, \"test_chol_corrupt\": %s},\n",
              opt_int(p.plan_threads).c_str(), b(p.keep_records), b(p.records_alt), b(p.factored), b(p.plan_device), b(p.listed_keys), p.schur_block,
              b(p.schur_linear), p.schur_variant, opt_str(p.schur_trace).c_str(), b(p.sharded), b(p.chol_fuse), p.chol_tail, p.chol_chunk,
              opt_int(p.chol_wgs).c_str(), b(p.chol_verify), b(p.chol_levels_before_solve), opt_str(p.chol_trace).c_str(), b(p.no_fused_sweep),
              b(p.debug_plan), b(p.test_fail_plan), b(p.test_fail_device_plan), b(p.test_chol_corrupt));
  std::printf(" \"solve\": {\"device_lm\": %s, \"lm_ahead\": %d, \"speculate\": %s, \"chol_levels\": %s, \"no_side_sweep\": %s, \"test_device_lm_off_on_this_rank\": %s},\n",
              b(s.device_lm), s.lm_ahead, b(s.speculate), b(s.chol_levels), b(s.no_side_sweep), b(s.test_device_lm_off_on_this_rank));
  std::printf(" \"chol_leaf_override\": %s, \"debug_plan\": %s,\n", opt_int(chol_leaf_override()).c_str(), b(debug_plan()));
  std::printf(" \"process\": {\"sweep_points_override\": %d, \"project_chunks_override\": %d, \"cov_times\": %s, \"device_cache_mb\": %llu, \"rccl_lib\": %s},\n",
              sweep_points_override(16), project_chunks_override(), b(cov_times_switch()), (unsigned long long)device_cache_mb(), opt_str(rccl_lib_path()).c_str());
  std::printf(" \"schur_block_unset\": %d, \"schur_pair_major\": %d, \"test_hooks\": %s,\n", PlanSwitches::kSchurBlockUnset, PlanSwitches::kSchurPairMajor, b(kTestHooks));
  std::printf(" \"chol_plan_options\": {\"chunk\": %d, \"tail\": %d, \"fuse_last\": %s}}\n", o.chunk, o.tail, b(o.fuse_last));
  return 0;
}
