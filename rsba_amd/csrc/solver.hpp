// What the units of the solver's host side share (solver.hip: the LM steps and rsba_solve; solver_plan.hip: the symbolic phase;
// solver_cov.hip: the covariance entry points): the state behind rsba_handle::solver, the phase timers, the allocation helpers
// and the step functions.  Private to these units: nothing here is part of the library's surface.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "capi_util.hpp"
#include "devmem.hpp"
#include "solver_state.hpp"
#include "chol_plan.hpp"
#include "pcg.hpp"
#include "switches.hpp"

namespace rsba {

// HIP-event timing of the phases of an LM iteration (rsba_solver_options::profile_phases): events are recorded on the
// solver's stream around each group of launches and read after the iteration's own synchronisation point, so the
// timed run has the same launch sequence and no extra waits.
struct PhaseTimer {
  bool on = false;
  struct Rec { int phase; hipEvent_t a, b; };
  std::vector<hipEvent_t> pool; size_t next = 0;
  std::vector<Rec> pending;
  double ms[RSBA_NUM_PHASES] = {}; int32_t calls[RSBA_NUM_PHASES] = {};
  hipEvent_t get() { if (next == pool.size()) { hipEvent_t e = nullptr; (void)hipEventCreate(&e); pool.push_back(e); } return pool[next++]; }
  void reset() { for (int p = 0; p < RSBA_NUM_PHASES; ++p) { ms[p] = 0.0; calls[p] = 0; } pending.clear(); next = 0; }
  void resolve() {   // the stream is idle
    for (const Rec& r : pending) { float t = 0.f; if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { ms[r.phase] += t; ++calls[r.phase]; } }
    pending.clear(); next = 0;
  }
  ~PhaseTimer() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
};

// The lists of the Cholesky plan (chol_plan.hpp) that a CholPlan names — one row per list: the host vector, the field its device copy
// goes to, and which plans take it (a sharded factorisation runs launch A and launch B on plans of their own, which differ from the
// replicated one in these rows only).  build_solver walks the table once to upload and once to fill the plans.
enum : unsigned { kPlanRep = 1, kPlanA = 2, kPlanB = 4, kPlanAll = 7 };
struct PlanListRow { std::vector<int32_t> CholHostPlan::*host; const int32_t* CholPlan::*field; unsigned plans; };
const PlanListRow kPlanLists[] = {
  {&CholHostPlan::upd, &CholPlan::upd, kPlanAll},
  {&CholHostPlan::diag_info, &CholPlan::diag_info, kPlanRep | kPlanA}, {&CholHostPlan::diag_info_sh, &CholPlan::diag_info, kPlanB},   // (B: the parts' partial tiles have been summed in by the exchange)
  {&CholHostPlan::diag_ptr, &CholPlan::diag_ptr, kPlanAll}, {&CholHostPlan::diag_list, &CholPlan::diag_list, kPlanAll},
  {&CholHostPlan::diag_own, &CholPlan::diag_own, kPlanAll}, {&CholHostPlan::diag_fuse, &CholPlan::diag_fuse, kPlanAll},
  {&CholHostPlan::sub_info, &CholPlan::sub_info, kPlanRep | kPlanA}, {&CholHostPlan::sub_info_sh, &CholPlan::sub_info, kPlanB},
  {&CholHostPlan::sub_ptr, &CholPlan::sub_ptr, kPlanAll}, {&CholHostPlan::sub_list, &CholPlan::sub_list, kPlanAll},
  {&CholHostPlan::sub_own, &CholPlan::sub_own, kPlanAll}, {&CholHostPlan::sub_col, &CholPlan::sub_col, kPlanAll}, {&CholHostPlan::sub_pub, &CholPlan::sub_pub, kPlanAll},
  {&CholHostPlan::back_info, &CholPlan::back_info, kPlanAll}, {&CholHostPlan::back_ptr, &CholPlan::back_ptr, kPlanAll}, {&CholHostPlan::back_list, &CholPlan::back_list, kPlanAll},
  {&CholHostPlan::tasks, &CholPlan::tasks, kPlanRep}, {&CholHostPlan::tasks_a, &CholPlan::tasks, kPlanA}, {&CholHostPlan::tasks_b, &CholPlan::tasks, kPlanB},
  // (read by the FWD2 / FWD2P tasks of a second right-hand side only)
  {&CholHostPlan::fwd_full, &CholPlan::fwd_range, kPlanRep}, {&CholHostPlan::fwd_a, &CholPlan::fwd_range, kPlanA}, {&CholHostPlan::fwd_b, &CholPlan::fwd_range, kPlanB},
  {&CholHostPlan::diag_toprow, &CholPlan::diag_toprow, kPlanAll},
};
constexpr size_t kNumPlanLists = sizeof kPlanLists / sizeof kPlanLists[0];

struct Solver {
  PhaseTimer timer;
  PhaseTimer xtimer;   // the same for the collectives of a sharded solve, by kind (RSBA_EXCHANGE_*)
  PlanSwitches sw;          // the environment as the plan saw it (switches.hpp): what the handle decided then stays decided
  SolveSwitches solve_sw;   // ... and as the last rsba_solve saw it (before the first one: as the plan did)
  rsba_plan_stats stats{};
  SolverDev sv{};
  std::vector<void*> allocs;
  // Cholesky plan over the packed tile slots: symbolic factorisation and task graph, the one owner of the host lists (the uploads
  // reference them; the level-scheduled fallback reads lev_*_ptr during solves); their device copies in the order of kPlanLists
  CholHostPlan hp;
  int32_t* d_plan_lists[kNumPlanLists] = {};
  DagArgs* d_dag_args = nullptr;
  int32_t* d_slot_tiles = nullptr;                                    // [nslots][2] {row tile, column tile} of every packed tile
  double* d_verify = nullptr;                                         // [2 * npad] residual and yardstick of the DAG verification
  // The verification runs on a stream of its own, beside the back-substitution / candidate / trial evaluation of the iteration: it
  // only has to be done when the step scalars are packed.  verify_b = the right-hand side of the solve (sv.rhs is overwritten by the step).
  hipStream_t vstream = nullptr; hipEvent_t ev_solved = nullptr, ev_verified = nullptr; double* verify_b = nullptr; bool verify_pending = false;
  bool test_corrupt_once = false;                                     // RSBA_CHOL_TEST_CORRUPT=1 (tests): the first DAG solve loses one entry of y
  int dag_fallbacks = 0;                                              // solves repeated on the level schedule after a failed check                                      // device copy of {sv, plan} for the persistent kernel
  unsigned int* d_dag_sync = nullptr;                                 // [ticket, pad x3]
  long long* d_trace = nullptr;                                       // sw.chol_trace: task time stamps of the last factorisation
  CholPlan plan{};
  int dag_workgroups = 0;
  bool dag_one_per_cu = true;                                         // LDS request above half a CU's: two persistent workgroups never share a CU (RSBA_CHOL_WGS above the CU count lifts it)
  bool use_levels = false;                                            // one launch per (level, kind): sw.chol_levels_before_solve, then every solve's solve_sw.chol_levels | its option; a suspect solve sets it
  uint8_t* d_row_sep = nullptr;                                       // [nt] tile columns (old index) in the separators
  int32_t* d_obs_slot = nullptr;
  double *d_gpose = nullptr, *d_gpoint = nullptr;
  int64_t num_pairs = 0;
  // The write-once cells of the DAG Cholesky (Lf | chol_part | Winv | zv | yv | Xpub) exist TWICE: while one set is in use the other
  // is re-armed (one memset) on a stream of its own, off the iteration's critical path; consecutive solves alternate.
  double* cells[2] = {nullptr, nullptr}; size_t ncells = 0, cell_off[5] = {0, 0, 0, 0, 0};
  DagArgs* d_dag_args2[2] = {nullptr, nullptr};
  int cur_cells = 0;
  hipStream_t mstream = nullptr; hipEvent_t ev_armed[2] = {nullptr, nullptr}, ev_released = nullptr; bool arm_pending[2] = {false, false};
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;   // the virtual-record sweep of a large shared-intrinsics problem runs on mstream beside the projection (reduce_system)
  int64_t schur_launches = 0;                                         // launches of the Schur kernel since the plan was built (statistics)
  double* d_ctl = nullptr;                                            // trust-region state on the device (device_state.hpp: LmCtlSlot; all zero while the host decides)
  rsba_iteration* d_trace_it = nullptr; int trace_it_cap = 0;         // the iteration records the deciding kernels write
  static constexpr int kCtlRing = 4;                                  // snapshots of d_ctl in flight (one per enqueued iteration): pinned host memory + the event behind each copy
  bool clamp_with_factor = false; double clamp_lo_hi[2] = {0.0, 0.0};   // device-side trust region: the diagonal's clamp rides in the point factor's launch
  double* h_ctl = nullptr; double* h_ctl_dev = nullptr;   // (h_ctl_dev: the same memory as the deciding kernel addresses it)
  bool gradmax_done = false;                              // the last linearisation's camera exchange carried max |g_i| (several ranks): gradient_max() has nothing left to do
  double ctl_seq = 0.0;                                   // stamp of the last snapshot asked for (never repeats within a handle: a stale slot cannot be mistaken for a new one)
  // Sharded factorisation (several ranks whose points respect the cut of tile_order.hpp): this rank factors the columns
  // of ITS part of the elimination tree from its own partial S (launch A), the ranks all-reduce the separators' tiles less what
  // their parts subtract from them, every rank factors the separators and solves them backward, then its own part (launch B).
  bool sharded_off = false;                                           // a suspect solve switched the sharded form (hp.sharded) off for this handle
  CholPlan plan_a{}, plan_b{}; DagArgs* d_dag_args_a[2] = {nullptr, nullptr}; DagArgs* d_dag_args_b[2] = {nullptr, nullptr};
  int ntop_slots = 0, ntop_tiles = 0;
  int32_t *d_top_slots = nullptr, *d_top_info = nullptr, *d_asm_ptr = nullptr, *d_asm_list = nullptr, *d_top_tiles = nullptr;
  double* topx_buf = nullptr;                                         // exchange (2) of the sharded form: the separators' tiles | their rows of the right-hand side
  uint8_t* d_row_mine = nullptr;                                      // [nt] tiles (old index) whose rows of y this rank contributes to the gather (its part; rank 0: the separators)
  uint8_t* d_row_check = nullptr;                                     // [nt] ... and whose residual it can check: its part (every tile of those rows is complete here)
  double* ybuf = nullptr;                                             // [npad] y of this rank's tiles, zero elsewhere: summed over the ranks
  int32_t* d_top_fill = nullptr; int ntop_fill = 0;                   // separator tiles that exist through fill only (zero in S; the sharded solve leaves its reduced values there)
  int num_reduced_blocks = 0, num_reduced_params = 0, num_priors_reduced = 0;
  int32_t* exch_slots = nullptr; double* exch_buf = nullptr; int exch_tiles = 0;   // exchange (2) of a sharded solve: the plan's tile pairs, packed
  double* zy2 = nullptr;                                              // [2][npad] z | y of one more right-hand side through the last factorisation (solve_again)
  double* border = nullptr, *ratio4 = nullptr;                       // free interFrameRatio: its column of S [npad]; its scalars on the device (solver_state.hpp: RatioSlot)
  PosePriorDev pp{};                                                  // per-pose priors: linearisation of the priorPoses coordinates
  double* merge_buf = nullptr;                                        // sharded solve: [4 M] owned point values | owner flags
  size_t ucross_len = 0;                                              // its doubles (rsba_solver_loss_changed clears them)
  double* ucross = nullptr;                                           // [F][CD][CD] motion-prior blocks (f, f-1), behind sv.U's J^T J blocks
  // iterative reduced solve (rsba_set_linear_solver type 1; pcg.hpp): lists and vectors, made by the first solve that asks for them
  struct Pcg { bool on = false, ready = false; PcgHostPlan hp; PcgDev dev{}; } pcg;
  // covariance of every frame (rsba_covariance_compute; solver_cov.hip): the selected inverse of the undamped S on the factor's pattern
  // (chol_plan.hpp: SelinvHostPlan; kernels_selinv.hip).  The lists and the tile map are uploaded by the first compute and live as long as the
  // plan; the two tile arrays ([nslots] tiles each: Sigma and G = L W) and the two vectors ([npad] each: the unknowns' marks, the border's v)
  // go back to the cache with rsba_covariance_release or the plan.
  struct Cov {
    bool ready = false; SelinvHostPlan sel; SelinvPlan sel_dev{};   // the lists, on the host and on the device
    double *sigma = nullptr, *g = nullptr, *live = nullptr, *vdev = nullptr;
    const int32_t* tmap = nullptr;          // [nt][nt] 2 * slot + transposed of every tile pair (unpermuted tile indices) of Sigma, -1 = not on the pattern
    const double2* slot_xy = nullptr;       // observations in slot order where the plan keeps none (sv.slot_xy == null: problems that keep records)
    int64_t plan_bytes = 0;                 // lists, tile map, slot_xy: as long as the plan
    double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // HIP-event times of the last compute's G, OFF and DIAG launches, of the last point getter's kernel and the last gather's
    bool valid = false;                     // the getters answer; cleared by whatever changes parameters or the problem
    std::vector<double> v, ud;              // free interFrameRatio: v = S^-1 b [npad]; diag(U) [F * CD] (zero: a coordinate no residual touches)
    double border_scale = 0.0;              // 1 / (h - b.v), 0 without the border
  } cov;
};

}  // namespace rsba

#pragma GCC visibility push(hidden)
namespace rsba {


template <class T>
inline int32_t s_alloc(Solver* s, T** p, size_t count) {
  void* q = nullptr;
  RSBA_HIP_TRY(dev_malloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
  s->allocs.push_back(q);
  *p = static_cast<T*>(q);
  return RSBA_OK;
}
template <class T>
inline int32_t s_upload(Solver* s, T** p, const std::vector<T>& v) {
  int32_t rc = s_alloc(s, p, v.size());
  if (rc) return rc;
  if (!v.empty()) RSBA_HIP_TRY(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return RSBA_OK;
}
template <class T>
inline int32_t s_upload_const(Solver* s, const T** p, const std::vector<T>& v) {
  T* q = nullptr;
  int32_t rc = s_upload(s, &q, v);
  *p = q;
  return rc;
}
struct PhaseScope {
  PhaseTimer* t = nullptr; int phase; hipStream_t st; hipEvent_t a = nullptr;
  PhaseScope(rsba_handle* h, int ph) : phase(ph), st(h->stream) {
    if (h->solver && h->solver->timer.on) { t = &h->solver->timer; start(); }
  }
  // a phase that another one interrupts (the exchange between the two launches of a sharded factorisation): stop() ... start()
  void start() { if (t && !a) { a = t->get(); (void)hipEventRecord(a, st); } }
  void stop() { if (t && a) { hipEvent_t b = t->get(); (void)hipEventRecord(b, st); t->pending.push_back({phase, a, b}); a = nullptr; } }
  ~PhaseScope() { stop(); }
};

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// motion priors: replicated terms from the lead rank — or, sharded factorisation, every rank its share
inline bool owns_motion_priors(const rsba_handle* h) { return h->solver->ucross && (h->solver->sv.lead || h->prior_split); }

// ---- solver_plan.hip ----
int32_t build_solver(rsba_handle* h);   // the symbolic phase, on first use

// ---- solver.hip: the steps of an iteration ----
struct RatioStep { double diag, gs, scale, eta; };   // (factor_and_solve)
int32_t reset_scales(rsba_handle* h);
int32_t exchange(rsba_handle* h, double* buf, int64_t count, int op, int kind);
DeviceProblem all_priors(const rsba_handle* h);
int32_t linearize(rsba_handle* h, bool have_eval = false, bool want_gradmax = false);
int32_t gradient_max(rsba_handle* h);
int32_t reduce_system(rsba_handle* h, double radius);
int32_t await_verification(rsba_handle* h);
int32_t solve_reduced_system(rsba_handle* h, bool rhs_stays = false);
int32_t solve_again(rsba_handle* h, const double* b2, const double** v_out);
int32_t factor_and_solve(rsba_handle* h, double radius, RatioStep* ratio = nullptr);
int32_t ensure_pcg(rsba_handle* h);

}  // namespace rsba
#pragma GCC visibility pop
