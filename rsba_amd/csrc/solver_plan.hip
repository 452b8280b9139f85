// The symbolic phase of the solver's host side, once per problem: frame / point adjacency, the per-block pair lists of the reduced
// camera system, the tile-level fill pattern of its Cholesky factor and its task graph, then the uploads and allocations of the plan.
// Ceres does the equivalent in its preprocessor (block structure detection, Schur ordering, CHOLMOD analyse) — SURVEY Appendix C.4.
// build_solver_impl is a driver over the stages of PlanBuild; the passes over observations, points and entries exist twice, on the
// host (lists_on_host) and on the device (lists_on_device: plan_device.hip), and fill the same fields.
#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <functional>
#include <limits>
#include <string>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <optional>
#include <thread>
#include <unordered_map>
#include <vector>

#include "solver.hpp"
#include "tile_order.hpp"
#include "plan_device.hpp"

using namespace rsba;

namespace {

// The symbolic phase hands its finished arrays to ONE background thread that allocates and copies them while the host goes on
// with the next pass (a fresh handle's plan is the per-call cost of windowedBA, VideoSfMHandler.cc:185-214: at 1k cameras 60 MB of
// index arrays, 6 ms of copies from pageable memory that used to sit behind the passes instead of under them).  The vectors must
// stay untouched until finish(); the allocations end up in Solver::allocs like everyone else's.
struct Uploader {
  Solver* s; int device;
  std::thread th; std::mutex m; std::condition_variable cv; std::deque<std::function<hipError_t()>> q;
  bool closing = false, joined = false; hipError_t err = hipSuccess; std::string what;
  std::vector<void*> allocs;
  Uploader(Solver* s_, int dev) : s(s_), device(dev) {
    th = std::thread([this]() {
      (void)hipSetDevice(device);
      for (;;) {
        std::function<hipError_t()> job;
        { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return closing || !q.empty(); }); if (q.empty()) return; job = std::move(q.front()); q.pop_front(); }
        if (err == hipSuccess) err = job();
      }
    });
  }
  void push(std::function<hipError_t()> job) { { std::lock_guard<std::mutex> lk(m); q.push_back(std::move(job)); } cv.notify_one(); }
  // *_ref: the vector outlives this object and is not touched before finish() (the plan scratch, members of the Solver); the plain
  // forms take a copy (small tables that are locals of build_solver: an early return destroys them before this object)
  template <class T>
  void upload_ref(T** dst, const std::vector<T>& v) {
    push([this, dst, &v]() -> hipError_t {
      void* d = nullptr;
      hipError_t e = dev_malloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T));
      if (e != hipSuccess) return e;
      allocs.push_back(d); *dst = static_cast<T*>(d);
      return v.empty() ? hipSuccess : hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    });
  }
  template <class T>
  void upload(T** dst, const std::vector<T>& v) {
    auto own = std::make_shared<std::vector<T>>(v);
    push([this, dst, own]() -> hipError_t {
      void* d = nullptr;
      hipError_t e = dev_malloc(&d, std::max<size_t>(own->size(), 1) * sizeof(T));
      if (e != hipSuccess) return e;
      allocs.push_back(d); *dst = static_cast<T*>(d);
      return own->empty() ? hipSuccess : hipMemcpy(d, own->data(), own->size() * sizeof(T), hipMemcpyHostToDevice);
    });
  }
  template <class T>
  void upload_const(const T** dst, const std::vector<T>& v) { upload(const_cast<T**>(dst), v); }
  template <class T>
  void upload_const_ref(const T** dst, const std::vector<T>& v) { upload_ref(const_cast<T**>(dst), v); }
  hipError_t finish() {
    if (!joined) {
      { std::lock_guard<std::mutex> lk(m); closing = true; } cv.notify_one();
      th.join(); joined = true;
      s->allocs.insert(s->allocs.end(), allocs.begin(), allocs.end()); allocs.clear();
    }
    return err;
  }
  ~Uploader() { (void)finish(); }
};

// Host scratch of the symbolic phase — everything sized by the observations or the entries (85 MB at 1k cameras).  It lives across
// calls: as plain locals these vectors cost more than the passes that fill them — every fresh handle page-faulted them in and
// unmapped them on return (on a 256-core host, after 16 threads had touched them, the unmap alone was 25 ms of a 51 ms plan;
// measured with glibc told to keep its memory: 14.5 ms).  One build at a time uses the shared set (a second concurrent one gets
// its own, freed on return); rsba_release_host_scratch() gives the memory back.
struct PlanScratch {
  std::vector<int64_t> point_ptr, fill, vgroup_ptr, pt_group;
  std::vector<int32_t> obs_slot, real_frame, slot_frame, slot_point, g_tile, g_rows, ent_pt, vgroup_point, vgroup_intr;
  std::vector<uint32_t> slot_gpos, ent_groups, g_off;
  std::vector<int64_t> pt_goff;
  std::vector<uint8_t> group_mask, group_present;
  std::vector<uint16_t> ent_mask;
  std::vector<std::vector<int32_t>> thread_cnt;
  std::vector<double> inprog_point;
};
std::mutex g_plan_scratch_mutex;
std::unique_ptr<PlanScratch> g_plan_scratch;

// fn(a, b, t) over nthr contiguous ranges of [0, n)
template <class F>
void parallel_ranges(int nthr, int64_t n, F&& fn) {
  if (nthr <= 1) { fn((int64_t)0, n, 0); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < nthr; ++t) pool.emplace_back([&, t]() { fn(n * t / nthr, n * (t + 1) / nthr, t); });
  for (auto& th : pool) th.join();
}

// What the stages of the symbolic phase share.  The references into the scratch and the Solver are set once; everything else is
// filled stage by stage, in the order of build_solver_impl.
struct PlanBuild {
  rsba_handle* const h; Solver* const s; const DeviceProblem& dp; SolverDev& sv; CholHostPlan& hp; CholPlan& pl;
  const TileLayout lay;
  // FR real frames; NIB intrinsics parameter blocks: sess.cam and / or per-frame f.cam (CeresHandler.h:260,277), NPF pseudo frames each;
  // F camera-side blocks of the reduced system, FT to a tile
  const int FR, M, CD, NIB, NPF, F, FT, nt;
  const int64_t N;
  const std::vector<int32_t>& fi;          // frame -> intrinsics block
  const std::vector<int32_t>& of; const std::vector<int32_t>& op;
  int intr_of(int f) const { return NIB > 1 ? fi[f] : 0; }
  const bool lead;
  // A plan that cannot be built on THIS rank must not leave the other ranks waiting in the vote (one all-reduce in the middle of the
  // plan; the same ranks ask the ordering for one part each): a rank-local failure is carried into that vote and every rank fails
  // together; a single rank returns at once.  fail() is the one place that knows.
  const bool plan_votes;
  int32_t local_fail = RSBA_OK; std::string local_why;
  int32_t fail(int32_t code, const std::string& why) {
    if (!plan_votes) return rsba_set_error(code, why.c_str());
    if (!local_fail) { local_fail = code; local_why = why; }
    return RSBA_OK;
  }
  const PlanSwitches& sw;   // the environment, read once (build_solver_impl)
  // RSBA_DEBUG_PLAN: host time of every stage
  const bool dbg_plan = sw.debug_plan;
  std::string phases; double t_phase = now_s();
  void tick(const char* name) {
    if (!dbg_plan) return;
    const double t = now_s();
    char b[64]; std::snprintf(b, sizeof b, " %s %.1f ms;", name, (t - t_phase) * 1e3); phases += b; t_phase = t;
  }
  // the host scratch: the shared set, or one of its own while another build holds that
  std::unique_lock<std::mutex> scratch_lock; std::unique_ptr<PlanScratch> own_scratch; PlanScratch& scr;
  std::vector<int64_t>& point_ptr;
  std::vector<int32_t>& obs_slot; std::vector<int32_t>& real_frame;
  std::vector<int64_t>& vgroup_ptr; std::vector<int32_t>& vgroup_point; std::vector<int32_t>& vgroup_intr;
  std::vector<int32_t>& slot_frame_host; std::vector<int32_t>& slot_point;
  std::vector<int64_t>& pt_group;     // groups of point j: [pt_group[j], pt_group[j+1])
  std::vector<int32_t>& g_tile; std::vector<int32_t>& g_rows;   // tile of each group; FT slots per group (NS = not observed)
  std::vector<uint32_t>& slot_gpos;         // where every slot's P record goes: group offset | position << 1 | kind (solver_state.hpp)
  std::vector<uint8_t>& group_mask;        // which of the three 16-row blocks of a group's records can be non-zero
  std::vector<uint8_t>& group_present;  // frames of the group's tile that see the point (plan statistics)
  std::vector<uint32_t>& g_off;                 // element offset of every group in Pm
  std::vector<int64_t>& pt_goff;   // doubles of the groups of the points before j
  std::vector<int32_t>& ent_pt;   // (host passes only; the device plan hands the chunk numbering the entry list's segments instead)
  std::vector<std::vector<int32_t>>& thread_cnt;
  // what the switches come to on this problem (settle_switches)
  int plan_threads = 1; bool recompute = false, factored = false, dev_plan = false;
  std::vector<uint8_t> tile_factored;
  // the lists of slots, groups, tile pairs and entries (lists_on_host / lists_on_device)
  DevicePlanOut dpo;
  std::vector<int64_t> frame_ptr;
  int64_t NVG = 0, NS;
  int64_t pt_total = 0;                          // doubles of all groups
  const bool dense_keys;
  std::vector<int64_t> dense_cnt; std::unordered_map<int64_t, int64_t> sparse_cnt;
  std::vector<uint32_t> struct_keys;   // (device plan: the keys of the pairs that exist whatever the points say)
  bool listed_keys = false; int nthreads = 1;
  std::unordered_map<int64_t, int32_t> tp_index; std::vector<int32_t> dense_index;
  std::vector<int32_t> tp_I, tp_J; std::vector<int64_t> tp_ptr{0};
  int64_t nent = 0; int ntp = 0;
  std::vector<int64_t> products_part{0};   // (plan statistics: block products that are not structurally zero)
  // ordering, task graph, chunks
  TileOrder tord; bool sharded = false, two_rhs = false;
  std::vector<int32_t> chunk_tp, chunk_n; std::vector<int64_t> chunk_e0;
  std::vector<std::vector<int32_t>> pair_chunks;
  std::vector<int32_t> tp_chunk0, tp_chunk_list, pm_ptr{0}, pm_list;
  std::vector<uint8_t> has_prior; int64_t ucross_base = 0;
  std::vector<int32_t> tp_dst; std::vector<uint8_t> tp_trans; std::vector<int64_t> tp_add;
  std::vector<double> inprog_pose, inprog_intr;
  std::optional<Uploader> up;   // (last: gone first — it joins its thread before anything it might still read goes)

  static PlanScratch& pick_scratch(bool shared, std::unique_ptr<PlanScratch>& own) {
    if (shared) { if (!g_plan_scratch) g_plan_scratch.reset(new PlanScratch()); return *g_plan_scratch; }
    own.reset(new PlanScratch()); return *own;
  }
  PlanBuild(rsba_handle* h_, Solver* s_)
      : h(h_), s(s_), dp(h_->dp), sv(s_->sv), hp(s_->hp), pl(s_->plan), lay(h_->dp.P, h_->dp.F, h_->dp.calibrated != 0, h_->dp.NI),
        FR(lay.FR), M(h_->dp.M), CD(lay.CD), NIB(lay.NIB), NPF(lay.NPF), F(lay.F), FT(lay.FT), nt(lay.nt), N(h_->dp.N),
        fi(h_->frame_intr), of(h_->obs_frame), op(h_->obs_point), lead(h_->rank == 0),
        plan_votes(h_->allreduce && h_->world > 1 && !h_->union_mask.empty()), sw(s_->sw),
        scratch_lock(g_plan_scratch_mutex, std::try_to_lock), scr(pick_scratch(scratch_lock.owns_lock(), own_scratch)),
        point_ptr(scr.point_ptr), obs_slot(scr.obs_slot), real_frame(scr.real_frame), vgroup_ptr(scr.vgroup_ptr), vgroup_point(scr.vgroup_point),
        vgroup_intr(scr.vgroup_intr), slot_frame_host(scr.slot_frame), slot_point(scr.slot_point), pt_group(scr.pt_group), g_tile(scr.g_tile),
        g_rows(scr.g_rows), slot_gpos(scr.slot_gpos), group_mask(scr.group_mask), group_present(scr.group_present), g_off(scr.g_off),
        pt_goff(scr.pt_goff), ent_pt(scr.ent_pt), thread_cnt(scr.thread_cnt), NS(h_->dp.N), dense_keys((int64_t)lay.nt * lay.nt <= (int64_t)1 << 26) {
    sv.F = FR; sv.Fx = F; sv.NPF = NPF; sv.NIB = NIB;
    sv.CD = CD; sv.n = (int64_t)F * CD;
    sv.nt = lay.nt; sv.npad = (int64_t)sv.nt * kTile;
  }
  std::vector<int32_t>& slot_frame() { return dev_plan ? dpo.slot_frame_h : slot_frame_host; }   // (device plan: the real slots only, and only when a later pass asks for them)

  void settle_switches();
  void start_uploads();
  int32_t plan_test_hook();
  int32_t check_group_doubles();
  void bump(int I, int J, int64_t by);
  void structural_pairs();
  // the passes over observations, points and entries, on the host ...
  void host_slots();
  void host_groups();
  template <class Fn> void for_each_entry(int j, Fn&& fn);
  std::pair<int, int> point_range(int t) const { return std::pair<int, int>((int)((int64_t)M * t / nthreads), (int)((int64_t)M * (t + 1) / nthreads)); }
  void host_entry_count();
  void host_entry_index();
  void host_entry_fill();
  int32_t lists_on_host();
  // ... or on the device
  int32_t lists_on_device();
  void order_and_symbolic();
  int32_t vote();
  int32_t split_motion_priors();
  void task_graph();
  void number_chunks(int64_t kBlock);
  int32_t schur_chunks();
  void pair_tiles();
  void reduced_program();
  int32_t uploads();
  int32_t allocations();
  int32_t dag_arguments();
  void statistics();
};

// ---- stage 1: the switches ----
void PlanBuild::settle_switches() {
  // host threads of the passes over observations / points / entries: sixteen are worth their start-up (~1 ms on a busy 256-thread host)
  // from a few hundred thousand observations on; a 100-camera window (187 k) plans fastest on four — symbolic phase 4.1 / 3.9 / 2.8 /
  // 3.4 ms on 1 / 2 / 4 / 8 threads (RSBA_PLAN_THREADS overrides: A/B)
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  plan_threads = N >= 400000 ? (int)std::min(16u, hw) : N >= 50000 ? (int)std::min(4u, hw) : 1;
  plan_threads = sw.plan_threads.value_or(plan_threads);
  // Which frame tiles store their groups FACTORED (solver_state.hpp: kGroupFactored): two-pose frames of a problem whose point-side passes
  // recompute the records — the 12 camera-side rows of a frame are (1 - tau) q | tau q, so 6 rows and tau say it all —
  // except a tile that holds an intrinsics pseudo frame (its virtual records have no such structure).  RSBA_FACTORED=0: none (A/B).
  recompute = (dp.calibrated != 0 || NIB == 1) && !sw.keep_records;
  factored = recompute && dp.P == 2 && sw.factored;
  tile_factored.assign((size_t)nt, 0);
  for (int t = 0; t < nt && factored; ++t) tile_factored[t] = !((int64_t)(t + 1) * FT > FR && (int64_t)t * FT < F && F > FR);   // (no pseudo frame in [t FT, (t + 1) FT))
  // The passes over observations, points and entries run ON THE DEVICE (plan_device.hip: stable sorts and prefix sums — the lists come
  // out as from the host passes below, which stay as the path for what the device form leaves out: several intrinsics blocks (their
  // per-point block lists), more than 8 192 tile columns (a dense pair map), and RSBA_PLAN_DEVICE=0 for A/B runs and the test that
  // compares the two).  The host keeps the O(tiles) part: ordering, symbolic factorisation, task lists, chunk numbering.
  dev_plan = N > 0 && NIB <= 1 && (int64_t)nt * nt <= ((int64_t)1 << 26) && N < ((int64_t)1 << 31) && sw.plan_device;
  frame_ptr.assign((size_t)FR + 1, 0);
}

void PlanBuild::start_uploads() {
  up.emplace(s, h->device);
  up->upload_const(&sv.frame_ptr, frame_ptr);
}

int32_t PlanBuild::plan_test_hook() {   // (after the uploader has started)
  return kTestHooks && sw.test_fail_plan ? fail(RSBA_ERR_UNSUPPORTED, "RSBA_TEST_FAIL_PLAN: the plan was made to fail (test hook)") : RSBA_OK;
}
// (more than 2^32 doubles of groups: the offsets of the group pass wrap; the plan is given up right behind it)
int32_t PlanBuild::check_group_doubles() {
  return pt_total + kGroupFull >= ((int64_t)1 << 32) ? fail(RSBA_ERR_UNSUPPORTED, "more than 2^32 doubles of P records: the Schur kernel indexes them with 32 bits") : RSBA_OK;
}

// ---- the tile pairs that exist whatever the points say ----
void PlanBuild::bump(int I, int J, int64_t by) {
  const int64_t key = (int64_t)I * nt + J;
  if (dev_plan) { struct_keys.push_back((uint32_t)key); return; }
  if (dense_keys) { int64_t& c = dense_cnt[key]; c = (c < 0 ? 0 : c) + by; }
  else sparse_cnt[key] += by;
}
void PlanBuild::structural_pairs() {
  if (dense_keys && !dev_plan) dense_cnt.assign((size_t)nt * nt, -1);
  for (int I = 0; I < nt; ++I) bump(I, I, 0);                // every diagonal tile exists (U + D^2, rhs)
  auto bump_blocks = [&](int a, int b) { const int I = std::max(a, b) / FT, J = std::min(a, b) / FT; bump(I, J, 0); };
  if (!h->union_mask.empty())                                  // multi-GPU: tiles other ranks fill, so all ranks share one layout
    for (int a = 0; a < FR; ++a) for (int b = 0; b <= a; ++b) if (h->union_mask[(size_t)a * FR + b]) {
      bump(a / FT, b / FT, 0);
      for (int v = 0; v < NPF; ++v) {                          // ... and the rows of the two frames' intrinsics blocks
        bump_blocks(FR + intr_of(a) * NPF + v, b); bump_blocks(FR + intr_of(b) * NPF + v, a);
        for (int w = 0; w < NPF; ++w) bump_blocks(FR + intr_of(a) * NPF + v, FR + intr_of(b) * NPF + w);
      }
    }
  // J^T J blocks that do not come from a point: (intrinsics block of a frame) x (that frame), and an intrinsics block with itself
  for (int f = 0; f < FR && NIB > 0; ++f) for (int v = 0; v < NPF; ++v) bump_blocks(FR + intr_of(f) * NPF + v, f);
  for (int c = 0; c < NIB; ++c) for (int v = 0; v < NPF; ++v) for (int w = 0; w <= v; ++w) bump_blocks(FR + c * NPF + v, FR + c * NPF + w);
  for (int32_t f : h->prior_frames) bump(f / FT, (f - 1) / FT, 0);   // motion priors couple frame f with f - 1 (every rank: one layout)
}

// ---- host form: slots and virtual groups ----
void PlanBuild::host_slots() {
  point_ptr.assign((size_t)M + 1, 0);
  // slots: stable counting sort of the frame-major list by point -> ascending frame inside a point.  On several threads: every
  // thread counts the points of ITS range of observations, the counts of the threads before it are where its share of a point's
  // slots starts — the slots come out exactly as from one thread.
  obs_slot.resize((size_t)N);
  real_frame.resize((size_t)N);
  const int nthr_obs = (N >= 200000 && (int64_t)plan_threads * M <= ((int64_t)1 << 26)) ? plan_threads : 1;
  if (nthr_obs > 1) {
    std::vector<std::vector<int32_t>> cnt((size_t)nthr_obs);
    std::vector<std::vector<int64_t>> fcnt((size_t)nthr_obs);
    parallel_ranges(nthr_obs, N, [&](int64_t a, int64_t b, int t) {
      std::vector<int32_t>& c = cnt[(size_t)t]; c.assign((size_t)M, 0);
      std::vector<int64_t>& fc = fcnt[(size_t)t]; fc.assign((size_t)FR, 0);
      for (int64_t i = a; i < b; ++i) { ++c[op[i]]; ++fc[of[i]]; }
    });
    for (int f = 0; f < FR; ++f) { int64_t sum = 0; for (int t = 0; t < nthr_obs; ++t) sum += fcnt[(size_t)t][f]; frame_ptr[f + 1] = frame_ptr[f] + sum; }
    // point_ptr, and per thread the first slot of its share of every point (in place of its count)
    parallel_ranges(nthr_obs, M, [&](int64_t a, int64_t b, int) {
      for (int64_t j = a; j < b; ++j) { int64_t sum = 0; for (int t = 0; t < nthr_obs; ++t) sum += cnt[(size_t)t][j]; point_ptr[j + 1] = sum; }
    });
    for (int j = 0; j < M; ++j) point_ptr[j + 1] += point_ptr[j];
    std::vector<std::vector<int64_t>> first((size_t)nthr_obs);
    for (auto& v : first) v.resize((size_t)M);
    parallel_ranges(nthr_obs, M, [&](int64_t a, int64_t b, int) {
      for (int64_t j = a; j < b; ++j) { int64_t at = point_ptr[j]; for (int t = 0; t < nthr_obs; ++t) { first[(size_t)t][j] = at; at += cnt[(size_t)t][j]; } }
    });
    parallel_ranges(nthr_obs, N, [&](int64_t a, int64_t b, int t) {
      std::vector<int64_t>& fill = first[(size_t)t];
      for (int64_t i = a; i < b; ++i) { const int64_t sl = fill[op[i]]++; obs_slot[i] = (int32_t)sl; real_frame[sl] = of[i]; }
    });
  } else {
    for (int64_t i = 0; i < N; ++i) { frame_ptr[of[i] + 1]++; point_ptr[op[i] + 1]++; }
    for (int f = 0; f < FR; ++f) frame_ptr[f + 1] += frame_ptr[f];
    for (int j = 0; j < M; ++j) point_ptr[j + 1] += point_ptr[j];
    std::vector<int64_t>& fill = scr.fill; fill.assign(point_ptr.begin(), point_ptr.end() - 1);
    for (int64_t i = 0; i < N; ++i) { const int64_t sl = fill[op[i]]++; obs_slot[i] = (int32_t)sl; real_frame[sl] = of[i]; }
  }
  // virtual groups: one per (observed point, intrinsics block it is seen through), blocks ascending; each owns NPF virtual
  // slots behind the real ones
  vgroup_ptr.assign((size_t)M + 1, 0);
  vgroup_point.clear(); vgroup_intr.clear();
  if (NIB == 1) {   // one shared block (the usual uncalibrated session): every observed point is seen through it — no lists to sort
    vgroup_point.reserve((size_t)M); vgroup_intr.reserve((size_t)M);
    for (int j = 0; j < M; ++j) {
      if (point_ptr[j + 1] > point_ptr[j]) { vgroup_point.push_back(j); vgroup_intr.push_back(0); }
      vgroup_ptr[j + 1] = (int64_t)vgroup_point.size();
    }
  } else if (NIB > 0) {
    std::vector<int32_t> seen;
    for (int j = 0; j < M; ++j) {
      seen.clear();
      for (int64_t x = point_ptr[j]; x < point_ptr[j + 1]; ++x) seen.push_back(intr_of(real_frame[x]));
      std::sort(seen.begin(), seen.end()); seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
      for (int32_t c : seen) { vgroup_point.push_back(j); vgroup_intr.push_back(c); }
      vgroup_ptr[j + 1] = (int64_t)vgroup_point.size();
    }
  }
  NVG = (int64_t)vgroup_point.size();
  NS = N + NVG * NPF;
  slot_frame_host.resize((size_t)NS);
  slot_point.resize((size_t)NS);
  parallel_ranges(nthr_obs, N, [&](int64_t a, int64_t b, int) { for (int64_t x = a; x < b; ++x) slot_frame_host[x] = real_frame[x]; });
  parallel_ranges(nthr_obs, M, [&](int64_t a, int64_t b, int) { for (int64_t j = a; j < b; ++j) for (int64_t x = point_ptr[j]; x < point_ptr[j + 1]; ++x) slot_point[x] = (int32_t)j; });
  for (int64_t g = 0; g < NVG; ++g) for (int v = 0; v < NPF; ++v) { slot_frame_host[N + g * NPF + v] = FR + vgroup_intr[g] * NPF + v; slot_point[N + g * NPF + v] = vgroup_point[g]; }
}

// ---- host form: the (tile, layer) groups ----
// ---- work list of the point elimination: one ENTRY per (point, pair of frame tiles I >= J) ----
// An entry lists the point's observation slot in each of the FT frames of tile I (sa) and of tile J (sb),
// -1 where it is not observed.  One wave turns an entry into up to FT x FT block products P_a P_b^T with
// every P record loaded once (frame-pair-major accumulation, no atomics).  A point seen
// twice in one frame gets a second "layer" of slots and the cross-layer entries.
// Per point, the (tile, layer) groups of its slots — computed once, flat (no per-point allocations: this pass used
// to be 85 % of the symbolic phase): group g of point j covers one tile and one layer and owns FT slot entries.
void PlanBuild::host_groups() {
  pt_group.assign((size_t)M + 1, 0); slot_gpos.resize((size_t)NS);
  // the slots of point j in ascending frame order (virtual ones last, by intrinsics block; only for points that are observed)
  auto slots_of = [&](int j, std::vector<int64_t>& out) {
    out.clear();
    for (int64_t x = point_ptr[j]; x < point_ptr[j + 1]; ++x) out.push_back(x);
    for (int64_t g = vgroup_ptr[j]; g < vgroup_ptr[j + 1]; ++g) for (int v = 0; v < NPF; ++v) out.push_back(N + g * NPF + v);
  };
  const int nthr_pts = M >= 4096 ? plan_threads : 1;
  pt_goff.assign((size_t)M + 1, 0);
  // one walk over a point's slots: on_group(g, tile) for every new (tile, layer) group g = 0, 1, .. of the point, on_slot(g, pos, slot)
  auto walk = [&](int j, std::vector<int64_t>& pslots, auto&& on_group, auto&& on_slot) -> int64_t {
    slots_of(j, pslots);
    int prev_frame = -1, layer = 0, cur_tile = -1;
    int64_t ng = 0, tile_first = 0;            // first group (layer 0) of the current tile
    for (int64_t sl : pslots) {
      const int f = slot_frame_host[sl], tile = f / FT, pos = f % FT;
      layer = (f == prev_frame) ? layer + 1 : 0; prev_frame = f;
      if (tile != cur_tile) { cur_tile = tile; tile_first = ng; }
      while (ng - tile_first <= layer) { on_group(ng, tile); ++ng; }   // a new layer of this tile
      on_slot(tile_first + layer, pos, sl);
    }
    return ng;
  };
  // count, prefix, fill — over contiguous point ranges on a few threads (the lists come out as from one thread)
  parallel_ranges(nthr_pts, M, [&](int64_t a, int64_t b, int) {
    std::vector<int64_t> ps;
    for (int64_t j = a; j < b; ++j) {
      int64_t doubles = 0;
      pt_group[j + 1] = walk((int)j, ps, [&](int64_t, int tile) { doubles += tile_factored[tile] ? kGroupFactored : kGroupFull; }, [](int64_t, int, int64_t) {});
      pt_goff[j + 1] = doubles;
    }
  });
  for (int j = 0; j < M; ++j) { pt_group[j + 1] += pt_group[j]; pt_goff[j + 1] += pt_goff[j]; }
  const int64_t NG = pt_group[M];
  // (more than 2^32 doubles of groups: the offsets below wrap; the plan is given up right behind this pass — on several ranks through the vote)
  g_tile.resize((size_t)NG); g_rows.assign((size_t)NG * FT, (int32_t)NS);   // NS = the all-zero record behind the last slot: "not observed"
  g_off.resize((size_t)NG + 1);
  group_mask.assign((size_t)NG + 1, 0); group_present.assign((size_t)NG + 1, 0);
  parallel_ranges(nthr_pts, M, [&](int64_t a, int64_t b, int) {
    std::vector<int64_t> ps;
    for (int64_t j = a; j < b; ++j) {
      const int64_t base = pt_group[j];
      int64_t at = pt_goff[j];
      walk((int)j, ps, [&](int64_t g, int tile) { g_tile[(size_t)(base + g)] = tile; g_off[(size_t)(base + g)] = (uint32_t)at; at += tile_factored[tile] ? kGroupFactored : kGroupFull; },
           [&](int64_t g, int pos, int64_t sl) {
             const size_t gg = (size_t)(base + g);
             const bool fac = tile_factored[g_tile[gg]] != 0;
             g_rows[gg * FT + pos] = (int32_t)sl;
             slot_gpos[sl] = g_off[gg] | ((uint32_t)pos << 1) | (fac ? 1u : 0u);
             ++group_present[gg];
             if (fac) group_mask[gg] |= (uint8_t)(pos < 2 ? 0b011 : pos == 2 ? 0b111 : 0b100);   // (factored: blocks 0 / 1 hold sources 0..15 = frames 0, 1 and two thirds of 2; block 2 the rest)
             else for (int row = pos * CD; row < (pos + 1) * CD; row += 4) group_mask[gg] |= (uint8_t)(1u << (row / 16));
           });
    }
  });
  g_off[(size_t)NG] = (uint32_t)pt_goff[M];
  pt_total = pt_goff[M];
  sv.ngroups = (int64_t)g_tile.size();
}

// entries of point j: every pair of its tiles (X >= Y) times every combination of their layers — for X == Y both
// orders of two different layers (the diagonal tile pair is stored in full)
template <class Fn>
void PlanBuild::for_each_entry(int j, Fn&& fn) {
  for (int64_t xa = pt_group[j]; xa < pt_group[j + 1];) {
    int64_t xb = xa; while (xb < pt_group[j + 1] && g_tile[xb] == g_tile[xa]) ++xb;
    for (int64_t ya = pt_group[j]; ya < xb;) {
      int64_t yb = ya; while (yb < pt_group[j + 1] && g_tile[yb] == g_tile[ya]) ++yb;
      for (int64_t gx = xa; gx < xb; ++gx) for (int64_t gy = ya; gy < yb; ++gy) fn(gx, gy);
      ya = yb;
    }
    xa = xb;
  }
}

// The two passes over all (point, tile pair) entries — count, then fill — are most of the symbolic phase (2 M entries at 1k cameras):
// with dense keys they run on a few host threads over contiguous point ranges, each with its own counters per tile pair, and
// the fill starts every thread where the threads before it end: the entry lists come out exactly as from one thread.
// Beyond 2 048 tile columns (8 k cameras) a counter per tile pair and thread would be 4 nt^2 bytes each: the threads first mark which
// pairs exist (one shared byte map), the pairs are numbered, and the per-thread counters are as long as that list (~9 nt).
// host_entry_count: how many entries every tile pair has; host_entry_index: the pairs in (I, J) order and where their entries start;
// host_entry_fill: the entries.
void PlanBuild::host_entry_count() {
  const bool small_keys = dense_keys && (int64_t)nt * nt <= ((int64_t)1 << 22) && !sw.listed_keys;   // (the variable: the large-problem path at any size — its plan must be the same)
  listed_keys = dense_keys && !small_keys && plan_threads > 1;
  nthreads = (small_keys || listed_keys) && M >= 4096 ? plan_threads : 1;   // (small_keys: per-thread counters of 4 nt^2 bytes)
  thread_cnt.resize(nthreads > 1 ? nthreads : 0);
  std::vector<int32_t> pair_no;   // listed_keys: key -> number of the pair in (I, J) order (what dense_index will hold further down)
  if (nthreads > 1 && listed_keys) {
    std::vector<uint8_t> seen((size_t)nt * nt, 0);
    {
      std::vector<std::thread> pool;
      for (int t = 0; t < nthreads; ++t)
        pool.emplace_back([&, t]() {
          const auto r = point_range(t);
          for (int j = r.first; j < r.second; ++j) for_each_entry(j, [&](int64_t gx, int64_t gy) { __atomic_store_n(&seen[(size_t)g_tile[gx] * nt + g_tile[gy]], (uint8_t)1, __ATOMIC_RELAXED); });
        });
      for (auto& th : pool) th.join();
    }
    pair_no.assign((size_t)nt * nt, -1);
    int32_t np = 0;
    for (int I = 0; I < nt; ++I) for (int J = 0; J <= I; ++J) {
      const size_t key = (size_t)I * nt + J;
      if (seen[key] && dense_cnt[key] < 0) dense_cnt[key] = 0;   // the pair exists (its entries are counted below)
      if (dense_cnt[key] >= 0) pair_no[key] = np++;
    }
    std::vector<uint8_t>().swap(seen);
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; ++t)
      pool.emplace_back([&, t]() {
        std::vector<int32_t>& c = thread_cnt[t];
        c.assign((size_t)np, 0);
        const auto r = point_range(t);
        for (int j = r.first; j < r.second; ++j) for_each_entry(j, [&](int64_t gx, int64_t gy) { ++c[pair_no[(size_t)g_tile[gx] * nt + g_tile[gy]]]; });
      });
    for (auto& th : pool) th.join();
    for (int I = 0; I < nt; ++I) for (int J = 0; J <= I; ++J) {
      const size_t key = (size_t)I * nt + J;
      if (pair_no[key] < 0) continue;
      int64_t sum = 0;
      for (int t = 0; t < nthreads; ++t) sum += thread_cnt[t][pair_no[key]];
      dense_cnt[key] += sum;
    }
  } else if (nthreads > 1) {
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; ++t)
      pool.emplace_back([&, t]() {
        std::vector<int32_t>& c = thread_cnt[t];
        c.assign((size_t)nt * nt, 0);
        const auto r = point_range(t);
        for (int j = r.first; j < r.second; ++j) for_each_entry(j, [&](int64_t gx, int64_t gy) { ++c[(size_t)g_tile[gx] * nt + g_tile[gy]]; });
      });
    for (auto& th : pool) th.join();
    for (size_t key = 0; key < (size_t)nt * nt; ++key) {
      int64_t sum = 0;
      for (int t = 0; t < nthreads; ++t) sum += thread_cnt[t][key];
      if (sum > 0) { int64_t& c = dense_cnt[key]; c = (c < 0 ? 0 : c) + sum; }
    }
  } else
  for (int j = 0; j < M; ++j) for_each_entry(j, [&](int64_t gx, int64_t gy) { bump(g_tile[gx], g_tile[gy], 1); });
}

void PlanBuild::host_entry_index() {
  if (dense_keys) {
    dense_index.assign((size_t)nt * nt, -1);
    for (int I = 0; I < nt; ++I) for (int J = 0; J <= I; ++J) {
      const int64_t c = dense_cnt[(size_t)I * nt + J];
      if (c >= 0) { dense_index[(size_t)I * nt + J] = (int32_t)tp_I.size(); tp_I.push_back(I); tp_J.push_back(J); tp_ptr.push_back(tp_ptr.back() + c); }
    }
    std::vector<int64_t>().swap(dense_cnt);
  } else {
    std::vector<int64_t> keys; keys.reserve(sparse_cnt.size());
    for (auto& kv : sparse_cnt) keys.push_back(kv.first);
    std::sort(keys.begin(), keys.end());
    for (int64_t key : keys) { tp_index[key] = (int32_t)tp_I.size(); tp_I.push_back((int32_t)(key / nt)); tp_J.push_back((int32_t)(key % nt)); tp_ptr.push_back(tp_ptr.back() + sparse_cnt[key]); }
  }
  nent = tp_ptr.back();
}

void PlanBuild::host_entry_fill() {
  auto index_of = [&](int I, int J) -> int32_t { return dense_keys ? dense_index[(size_t)I * nt + J] : tp_index[(int64_t)I * nt + J]; };
  // an entry is the pair of groups (of tile I, of tile J) plus its point: the kernel looks the slots up in g_rows
  std::vector<uint32_t>& ent_groups = scr.ent_groups; ent_groups.resize((size_t)nent * 2);   // (where the two groups start in Pm | kind: solver_state.hpp)
  ent_pt.resize((size_t)nent);
  // ... and, per entry, which of the 3 x 3 block products of its two groups can be non-zero
  std::vector<uint16_t>& ent_mask = scr.ent_mask; ent_mask.resize((size_t)nent);
  products_part.assign((size_t)std::max(nthreads, 1), 0);
  auto put_entry = [&](int64_t w, int64_t gx, int64_t gy, int j, int64_t& prod) {
    ent_groups[2 * (size_t)w] = g_off[(size_t)gx] | (tile_factored[g_tile[(size_t)gx]] ? 1u : 0u);
    ent_groups[2 * (size_t)w + 1] = g_off[(size_t)gy] | (tile_factored[g_tile[(size_t)gy]] ? 1u : 0u);
    ent_pt[w] = j | (gx == gy ? (int32_t)0x80000000 : 0);   // top bit: the entry carries the rhs term P z
    const unsigned ma = group_mask[(size_t)gx], mb = group_mask[(size_t)gy];
    unsigned pm = 0;
    for (int I = 0; I < 3; ++I) if ((ma >> I) & 1u) pm |= mb << (3 * I);
    ent_mask[(size_t)w] = (uint16_t)pm;
    prod += (int64_t)group_present[(size_t)gx] * group_present[(size_t)gy];
  };
  {
    std::vector<int64_t> fill(tp_ptr.begin(), tp_ptr.end() - 1);
    if (nthreads > 1) {
      // per thread and tile pair: where its entries start (the counters become cursors)
      std::vector<std::vector<int64_t>> cursor(nthreads, std::vector<int64_t>(tp_I.size(), 0));
      for (size_t t_ = 0; t_ < tp_I.size(); ++t_) {
        const size_t key = listed_keys ? t_ : (size_t)tp_I[t_] * nt + tp_J[t_];   // (listed_keys: the counters are indexed by the pair's number, which is t_)
        int64_t at = fill[t_];
        for (int t = 0; t < nthreads; ++t) { cursor[t][t_] = at; at += thread_cnt[t][key]; }
      }
      std::vector<std::thread> pool;
      for (int t = 0; t < nthreads; ++t)
        pool.emplace_back([&, t]() {
          std::vector<int64_t>& cur = cursor[t];
          const auto r = point_range(t);
          int64_t prod = 0;
          for (int j = r.first; j < r.second; ++j)
            for_each_entry(j, [&](int64_t gx, int64_t gy) { put_entry(cur[dense_index[(size_t)g_tile[gx] * nt + g_tile[gy]]]++, gx, gy, j, prod); });
          products_part[t] = prod;
        });
      for (auto& th : pool) th.join();
    } else {
      int64_t prod = 0;
      for (int j = 0; j < M; ++j) for_each_entry(j, [&](int64_t gx, int64_t gy) { put_entry(fill[index_of(g_tile[gx], g_tile[gy])]++, gx, gy, j, prod); });
      products_part[0] = prod;
    }
  }
  std::vector<int32_t>().swap(dense_index);
  up->upload_const_ref(&sv.ent_groups, ent_groups);
  up->upload_const_ref(&sv.ent_pt, ent_pt);
  up->upload_const_ref(&sv.ent_mask, ent_mask);
}

int32_t PlanBuild::lists_on_host() {
  int32_t rc;
  host_slots();
  start_uploads();
  up->upload_const_ref(&sv.point_ptr, point_ptr);
  up->upload_const_ref(&sv.slot_frame, slot_frame_host);
  up->upload_const_ref(&sv.slot_point, slot_point);
  up->upload_ref(&s->d_obs_slot, obs_slot);
  tick("slots");
  host_groups();
  if ((rc = plan_test_hook()) || (rc = check_group_doubles())) return rc;
  up->upload_const_ref(&sv.slot_gpos, slot_gpos);
  structural_pairs();
  host_entry_count();
  host_entry_index();
  host_entry_fill();
  return RSBA_OK;
}

// ---- device form of the same passes (plan_device.hip) ----
// (a failure here — the arena allocations are the likeliest out-of-memory of the symbolic phase — goes through fail() like the checks
// of the host form)
int32_t PlanBuild::lists_on_device() {
  int32_t rc;
  for (int f = 0; f <= FR; ++f) frame_ptr[f] = (int64_t)(std::lower_bound(of.begin(), of.end(), (int32_t)f) - of.begin());   // (the list is frame-major)
  start_uploads();
  tick("slots");
  if ((rc = plan_test_hook())) return rc;
  structural_pairs();
  ent_pt.clear();
  uint8_t* d_tf = nullptr;
  if (factored) {
    if (int32_t rc_ = s_upload(s, &d_tf, tile_factored)) {
      if ((rc = fail(rc_, std::string(plan_votes ? "device plan: " : "") + rsba_last_error()))) return rc;
    }
  }
  bool any_const_point = false;
  for (int j = 0; j < M && !any_const_point; ++j) any_const_point = h->mask_point[(size_t)j * 3] == 0.0;
  int64_t chunk_block = sw.schur_block != PlanSwitches::kSchurBlockUnset ? sw.schur_block : nt > 500 ? 2048 : 0;   // (the chunk numbering by blocks of points, below: it gets the entry list's segments instead of the list)
  if (chunk_block >= M) chunk_block = 0;
  DevicePlanIn din{dp.obs_frame, dp.obs_point, N, M, FR, NPF, NIB, FT, CD, nt, d_tf, struct_keys.data(), (int64_t)struct_keys.size(), chunk_block, any_const_point, sw.debug_plan, h->stream};
  hipError_t pe = local_fail ? hipSuccess : device_plan_lists(din, &dpo);
  if (pe == hipSuccess && !local_fail && kTestHooks && sw.test_fail_device_plan) pe = hipErrorOutOfMemory;   // (test hook: the lists' allocations fail on this rank)
  s->allocs.insert(s->allocs.end(), dpo.owned.begin(), dpo.owned.end());
  if (pe != hipSuccess) {
    (void)hipGetLastError();
    const int32_t code = pe == hipErrorOutOfMemory ? RSBA_ERR_OUT_OF_MEMORY : pe == hipErrorInvalidValue ? RSBA_ERR_UNSUPPORTED : RSBA_ERR_HIP;
    if ((rc = fail(code, pe == hipErrorInvalidValue ? std::string("device plan: 2^32 or more (point, tile pair) entries — the lists are indexed with 32 bits") : std::string("device plan: ") + hipGetErrorString(pe)))) return rc;
  }
  if (local_fail) {
    // nothing of the lists can be used: an empty plan (no points' entries) walks through the host-side passes up to the vote, where every rank gives up together
    dpo = DevicePlanOut{};
    dpo.point_ptr_h.assign((size_t)M + 1, 0); dpo.tp_ptr.assign(1, 0);
  }
  point_ptr.swap(dpo.point_ptr_h);
  sv.point_ptr = dpo.point_ptr; sv.slot_frame = dpo.slot_frame; sv.slot_point = dpo.slot_point; s->d_obs_slot = dpo.obs_slot; sv.slot_gpos = dpo.slot_gpos;
  sv.ent_groups = dpo.ent_groups; sv.ent_pt = dpo.ent_pt; sv.ent_mask = dpo.ent_mask;
  NVG = dpo.nvgroups; NS = N + NVG * NPF;
  sv.ngroups = dpo.ngroups; pt_total = dpo.group_doubles;
  tp_I.swap(dpo.tp_I); tp_J.swap(dpo.tp_J); tp_ptr.swap(dpo.tp_ptr);
  nent = tp_ptr.back();
  products_part[0] = dpo.products;
  return check_group_doubles();
}

// ---- tile graph of S, fill-reducing / parallelism-exposing ordering, symbolic factorisation ----
void PlanBuild::order_and_symbolic() {
  std::vector<std::vector<int32_t>> adj(nt);
  for (int t = 0; t < ntp; ++t) if (tp_I[t] != tp_J[t]) { adj[tp_I[t]].push_back(tp_J[t]); adj[tp_J[t]].push_back(tp_I[t]); }
  tick("entries");
  // Nested dissection by BFS level structures (tile_order.hpp).  A sharded solve (several ranks, one tile layout: the co-visibility
  // structure of all ranks is installed) asks for the top of the tree to be cut into one part per rank; whether THIS rank's points
  // respect the cut — rsba_partition_points places them so — is checked below (sharded plan).
  std::vector<double> tile_weight(nt, 0.0);
  for (int f = 0; f < FR; ++f) tile_weight[f / FT] += (double)(h->frame_obs_total.empty() ? frame_ptr[f + 1] - frame_ptr[f] : h->frame_obs_total[f]);
  tord = nested_dissection(nt, adj, plan_leaf_size(plan_votes ? h->world : 1, nt), plan_votes ? h->world : 1, &tile_weight);
  tick("ordering");
  chol_symbolic(nt, adj, tord, &hp);
  sv.nslots = hp.nslots;
  tick("symbolic");
}

// ---- sharded factorisation: does every rank's share of the points respect the cut? ----
// (part of a column = the rank whose subtree it belongs to, -1 = a separator the ranks share.)  Every kind of block the solver takes
// is in (rounds 4 - 6): motion priors are shared out like the frames (below), GoodPosePrior / SphericalPrior terms go to the rank whose
// part holds the pose, a free interFrameRatio has its column's forward solve run part by part — and SEVERAL intrinsics blocks (a 9-block
// per frame, CeresHandler.h:256-264,273-280; round 6) need nothing of their own: a block's pseudo frames sit in a tile that is adjacent to the
// tiles of exactly the frames seen through it, so the dissection puts it in those frames' part or in a separator, every point seen through
// the block is owned by that part's rank (rsba_partition_points builds the same graph and follows the pseudo tiles too: the vote below
// checks both), and the tile's replicated terms — damping, identity padding, the gradient after exchange (1) — follow frame_lead like
// any frame tile's.
int32_t PlanBuild::vote() {
  sharded = plan_votes && tord.parts_ok && sw.sharded;   // (the switch: A/B)
  if (plan_votes) {
    double bad = sharded ? 0.0 : 1.0;
    // an observation adds to its frame's tile and to the pseudo frames' tiles of the block its frame is seen through: every one of them
    // must be this rank's or a separator (a point seen in separator frames only may still reach a block whose pseudo tile is in a part)
    auto foreign = [&](int t) { const int p = tord.part_of[t]; return p >= 0 && p != h->rank; };
    for (int64_t i = 0; i < N && bad == 0.0; ++i) {
      if (foreign(lay.frame_tile(of[i]))) bad = 1.0;
      for (int v = 0; v < NPF && NIB > 0; ++v) if (foreign(lay.pseudo_tile(intr_of(of[i]), v))) bad = 1.0;
    }
    if (local_fail) bad = 2.0;   // this rank cannot build its plan at all: every rank gives up together
    // every rank must take the same form: one all-reduce (max) of the verdicts — through the handle's cost slot (allocated with the
    // handle, rewritten by every evaluation): no allocation here that could fail on one rank and leave the others waiting
    double* d_bad = h->d_cost2;
    hipError_t e = hipMemcpyAsync(d_bad, &bad, sizeof bad, hipMemcpyHostToDevice, h->stream);
    const int32_t rcx = exchange(h, d_bad, 1, 1, RSBA_EXCHANGE_SETUP);
    if (e == hipSuccess && rcx == RSBA_OK) e = hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && rcx == RSBA_OK) e = hipStreamSynchronize(h->stream);
    if (rcx) return rcx;
    if (e != hipSuccess) return rsba_set_error(e == hipErrorOutOfMemory ? RSBA_ERR_OUT_OF_MEMORY : RSBA_ERR_HIP, hipGetErrorString(e));
    if (local_fail) return rsba_set_error(local_fail, local_why.c_str());
    if (bad >= 2.0) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "another rank could not build its plan (its own call says why)");
    sharded = bad == 0.0;
  }
  return RSBA_OK;
}

int32_t PlanBuild::split_motion_priors() {
  if (sharded && !h->prior_frames.empty() && !h->prior_split) {
    // The prior between frames f and f - 1 (CeresHandler.h:147-185) adds to U_f, U_f-1, the (f, f-1) block and both gradients: it
    // belongs to the rank that owns the part either frame is in (two adjacent frames are never in two different parts: their tiles
    // are the same or neighbours), rank 0 when both sit in separators — so every tile of a part's columns stays complete on its rank.
    auto part_of_frame = [&](int f) { return tord.part_of[f / FT]; };
    std::vector<int32_t> own((size_t)FR + 1, 0);
    int mine = 0;
    for (int32_t f : h->prior_frames) {
      int r = part_of_frame(f);
      if (r < 0) r = part_of_frame(f - 1);
      if (r < 0) r = 0;
      if (r == h->rank) { own[f] = 1; ++mine; }
    }
    int32_t* d_own = nullptr;
    if (int32_t rc_ = s_upload(s, &d_own, own)) return rc_;
    h->prior_of_all = h->dp.prior_of; h->prior_invalid_all = h->prior_invalid;   // (d_own belongs to this plan: rsba_destroy_solver restores the handle's own table)
    h->dp.prior_of = d_own;
    if (h->prior_invalid > 0) h->prior_invalid = mine;
    h->prior_split = true;
  }
  return RSBA_OK;
}

// ---- the task graph: items, chunking, ticket orders (chol_plan.hpp) ----
void PlanBuild::task_graph() {
  CholTaskInput tin;
  tin.order = &tord; tin.sharded = sharded; tin.rank = h->rank; tin.pair_I = &tp_I; tin.pair_J = &tp_J;
  tin.two_rhs = h->prior_free && !h->prior_frames.empty();   // a free interFrameRatio: its column of the normal equations rides through the factorisation
  tin.opt.fuse_last = sw.chol_fuse;
  // (the defaults: swept on C4 / C5 after the look-ahead — fewer, longer UPDATE tasks and a short own share, 2.45 -> 2.36 ms per C4 iteration)
  tin.opt.tail = sw.chol_tail; tin.opt.chunk = sw.chol_chunk;   // tuning aids
  chol_tasks(tin, &hp);
  two_rhs = hp.two_rhs;
  tick("tasks");
}

// Chunks of the Schur kernel (one workgroup each): at most kSchurChunk consecutive entries of one tile pair, numbered tile
// pair by tile pair in (I, J) order — the pairs of one tile row, which read the same A_j(I) groups, next to each other; the
// kernel's blockIdx -> chunk map keeps consecutive chunks on one XCD.  What was measured around this choice (C4, round 3):
//   * this numbering: 40 % L2 hits, 2.5 GB from the fabric per launch, 4 975 chunks, kernel 0.53 ms — its MFMA loops run at
//     88 % of the matrix pipe (two waves per SIMD), the rest is tables / epilogue (14 %) and the ramp-down of the launch;
//   * point-block-major (RSBA_SCHUR_BLOCK=<points>: every tile pair cut at the same blocks of consecutive points, all pairs of
//     a block next to each other — rsba numbers tracks in the order the video first sees them, so a block spans a few tiles
//     and an XCD's L2 holds its records): 80 % L2 hits, 0.76 GB from the fabric, but 8 700 shorter chunks: 0.60 ms;
//   * equal parts of up to 1024 entries launched longest first, wherever their records are: 3 100 chunks, 0.67 ms — the
//     loops then wait for memory (2.2 us per group of four entries instead of 1.5).
// Per tile pair the chunk ids are listed in entry order for the merge kernel.
//   * round 4, 4k cameras (1 001 tile columns, 29 678 chunks): there the kernel pulls 20.5 GB from the fabric in 3.6 ms — the
//     point-block-major numbering with blocks of 2 048 points is worth 3 % (3.59 -> 3.47 ms, 35 502 chunks), so it is the default
//     above 500 tile columns — as long as it does not multiply the chunks (point numbers that do not follow the video would).
void PlanBuild::number_chunks(int64_t kBlock) {
  chunk_tp.clear(); chunk_n.clear(); chunk_e0.clear();
  for (auto& pc : pair_chunks) pc.clear();
  if (dev_plan && kBlock < M) {
    // the device plan's segments — maximal runs of one tile pair's entries inside one block of points, in entry order — in the order of
    // the walk below: block by block, inside a block the pairs in (I, J) order, every segment cut into chunks
    const size_t nseg = dpo.seg_pair.size();
    std::vector<int32_t> order(nseg);
    for (size_t q = 0; q < nseg; ++q) order[q] = (int32_t)q;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return dpo.seg_block[a] != dpo.seg_block[b] ? dpo.seg_block[a] < dpo.seg_block[b] : dpo.seg_pair[a] < dpo.seg_pair[b]; });
    for (int32_t q : order) {
      const int tp_ = dpo.seg_pair[q];
      const int64_t q0 = dpo.seg_start[q], q1 = ((size_t)q + 1 < nseg && dpo.seg_pair[q + 1] == tp_) ? dpo.seg_start[q + 1] : tp_ptr[tp_ + 1];
      for (int64_t a = q0; a < q1; a += kSchurChunk) {
        pair_chunks[tp_].push_back((int32_t)chunk_tp.size());
        chunk_tp.push_back(tp_); chunk_e0.push_back(a); chunk_n.push_back((int32_t)std::min<int64_t>(kSchurChunk, q1 - a));
      }
    }
    return;
  }
  // per tile pair the cursor into its entry list (entries are in point order); pairs that still have entries, in (I, J) order
  std::vector<int64_t> cursor(tp_ptr.begin(), tp_ptr.end() - 1);
  std::vector<int32_t> live; live.reserve(64);
  int next_pair = 0;           // pairs enter `live` when the block reaches their first point
  std::vector<int32_t> by_first(ntp);
  for (int t = 0; t < ntp; ++t) by_first[t] = t;
  // (the device plan brings the entries' points to the host only for a numbering by point blocks: without them every pair is live from the first — and only — block)
  auto first_point = [&](int t) { return tp_ptr[t] < tp_ptr[t + 1] ? (ent_pt.empty() ? 0 : (ent_pt[tp_ptr[t]] & 0x7fffffff)) : std::numeric_limits<int32_t>::max(); };
  std::stable_sort(by_first.begin(), by_first.end(), [&](int a, int b) { return first_point(a) < first_point(b); });
  for (int64_t p0 = 0; p0 < M; p0 += kBlock) {
    const int64_t p1 = std::min<int64_t>(p0 + kBlock, M);
    while (next_pair < ntp && first_point(by_first[next_pair]) < p1) live.push_back(by_first[next_pair++]);
    std::sort(live.begin(), live.end());   // (I, J) order inside the block: the pairs of one tile row next to each other
    size_t keep = 0;
    for (size_t x = 0; x < live.size(); ++x) {
      const int tp_ = live[x];
      int64_t q = cursor[tp_];
      const int64_t qend = tp_ptr[tp_ + 1];
      if (p1 >= M) q = qend;
      else q = std::lower_bound(ent_pt.begin() + q, ent_pt.begin() + qend, (int32_t)p1, [](int32_t e, int32_t p) { return (e & 0x7fffffff) < p; }) - ent_pt.begin();   // (a pair's entries are in point order)
      for (int64_t q0 = cursor[tp_]; q0 < q; q0 += kSchurChunk) {
        pair_chunks[tp_].push_back((int32_t)chunk_tp.size());
        chunk_tp.push_back(tp_); chunk_e0.push_back(q0); chunk_n.push_back((int32_t)std::min<int64_t>(kSchurChunk, q - q0));
      }
      cursor[tp_] = q;
      if (q < qend) live[keep++] = tp_;
    }
    live.resize(keep);
  }
}

int32_t PlanBuild::schur_chunks() {
  pair_chunks.resize((size_t)ntp);
  {
    int64_t pair_major = 0;
    for (int t = 0; t < ntp; ++t) pair_major += (tp_ptr[t + 1] - tp_ptr[t] + kSchurChunk - 1) / kSchurChunk;
    const bool by_size = sw.schur_block == PlanSwitches::kSchurBlockUnset;   // (RSBA_SCHUR_BLOCK: tuning aid, 0 = tile pair by tile pair)
    const int64_t kBlock = by_size ? (nt > 500 ? 2048 : std::max<int64_t>(M, 1)) : sw.schur_block > 0 ? sw.schur_block : std::max<int64_t>(M, 1);
    number_chunks(kBlock);
    if (kBlock < M && by_size && (int64_t)chunk_tp.size() > pair_major + pair_major / 3) number_chunks(std::max<int64_t>(M, 1));
  }
  // A pair with very many chunks (the diagonal pair of the intrinsics pseudo tile has one per 512 points of the whole
  // problem) would be summed by a single workgroup of the merge kernel: its chunk list is pre-reduced in groups of
  // kMergeGroup, one workgroup each, into the partial tile of the group's first chunk, and only those heads go to the merge.
  const int kMergeGroup = 32;
  tp_chunk0.assign(ntp + 1, 0);
  for (int t = 0; t < ntp; ++t) {
    tp_chunk0[t] = (int32_t)tp_chunk_list.size();
    const std::vector<int32_t>& pc = pair_chunks[t];
    if ((int)pc.size() <= kMergeGroup) { tp_chunk_list.insert(tp_chunk_list.end(), pc.begin(), pc.end()); continue; }
    for (size_t g = 0; g < pc.size(); g += kMergeGroup) {
      const size_t g1 = std::min(pc.size(), g + kMergeGroup);
      tp_chunk_list.push_back(pc[g]);
      if (g1 - g > 1) { pm_list.insert(pm_list.end(), pc.begin() + g, pc.begin() + g1); pm_ptr.push_back((int32_t)pm_list.size()); }
    }
  }
  tp_chunk0[ntp] = (int32_t)tp_chunk_list.size();
  sv.npremerge = (int)pm_ptr.size() - 1;
  sv.nchunk = (int)chunk_tp.size(); sv.ntp = ntp; sv.FT = FT;
  sv.schur_linear = sw.schur_linear;
  sv.schur_variant = sw.schur_variant;   // (4 / 5: ablations, instrumented build only)
  sv.schur_trace = nullptr;
  if (sw.schur_trace) { if (int32_t rc_ = s_alloc(s, &sv.schur_trace, 8 * (size_t)std::max(sv.nchunk, 1))) return rc_; }
  return RSBA_OK;
}

// where every tile pair goes in the packed tiles of S, and which J^T J blocks enter it
void PlanBuild::pair_tiles() {
  has_prior.assign((size_t)FR + 1, 0);
  for (int32_t f : h->prior_frames) has_prior[f] = 1;
  ucross_base = ((int64_t)FR + (int64_t)NPF * FR + (int64_t)NIB * NPF * NPF) * CD * CD;   // behind the J^T J blocks in sv.U
  tp_dst.assign(ntp, 0); tp_trans.assign(ntp, 0);
  tp_add.assign((size_t)ntp * FT * FT, -1);
  for (int t = 0; t < ntp; ++t) {
    const int I = tp_I[t], J = tp_J[t], pI = hp.iperm[I], pJ = hp.iperm[J];
    // tile of the pair in the permuted order; if the ordering swapped the two tiles it is stored transposed
    if (pI >= pJ) tp_dst[t] = hp.slot_of(pI, pJ); else { tp_dst[t] = hp.slot_of(pJ, pI); tp_trans[t] = 1; }
    // which J^T J block enters block (a,b) of this tile: U layout [frames][pseudo x frames][pseudo x pseudo]
    for (int x = 0; x < FT; ++x) for (int y = 0; y < FT; ++y) {
      const int a = I * FT + x, b = J * FT + y;
      if (a >= F || b >= F || a < b) continue;
      int64_t add = -1;
      if (a < FR) {
        if (a == b) add = (int64_t)a * CD * CD;
        else if (b == a - 1 && has_prior[a]) add = ucross_base + (int64_t)a * CD * CD;   // motion prior block (a, a-1)
      }
      else {
        const int ca = (a - FR) / NPF, va = (a - FR) % NPF;     // pseudo frame va of intrinsics block ca
        if (b < FR) { if (intr_of(b) == ca) add = ((int64_t)FR + (int64_t)va * FR + b) * CD * CD; }   // only with the frames that use the block
        else if ((b - FR) / NPF == ca) add = ((int64_t)FR + (int64_t)NPF * FR + ((int64_t)ca * NPF + va) * NPF + (b - FR) % NPF) * CD * CD;
      }
      tp_add[((size_t)t * FT + x) * FT + y] = add;
    }
  }
  tick("chunks");
}

// which coordinates belong to the reduced program (for |x| and |step|): blocks that are not constant
// and are touched by at least one residual block
void PlanBuild::reduced_program() {
  inprog_pose.assign((size_t)FR * CD, 0.0); inprog_intr.assign((size_t)std::max(NIB * NPF, 1) * CD, 0.0);
  std::vector<double>& inprog_point = scr.inprog_point; inprog_point.assign((size_t)M * 3, 0.0);
  int nfree = 0;
  sv.lead = lead;
  std::vector<uint8_t> has_pose_prior((size_t)FR, 0);
  for (int32_t b : h->pp_blocks) has_pose_prior[b / dp.P] = 1;
  if (dp.pp_spherical >= 0) has_pose_prior[dp.pp_spherical / dp.P] = 1;
  auto frame_has_obs = [&](int f) {
    if (has_prior[f] || has_prior[f + 1] || has_pose_prior[f]) return true;   // touched by a motion prior / pose prior block
    return h->frame_obs_total.empty() ? frame_ptr[f + 1] > frame_ptr[f] : h->frame_obs_total[f] > 0;
  };
  {
    // an intrinsics block is part of the program when it is not constant and a residual block touches it
    std::vector<uint8_t> touched((size_t)std::max(NIB, 1), 0);
    for (int f = 0; f < FR && NIB > 0; ++f) if (h->frame_obs_total.empty() ? frame_ptr[f + 1] > frame_ptr[f] : h->frame_obs_total[f] > 0) touched[intr_of(f)] = 1;
    for (int c = 0; c < NIB; ++c) if (lead && touched[c] && h->mask_intr[(size_t)c * 9] != 0.0)
      for (int k = 0; k < 9; ++k) { inprog_intr[((size_t)c * NPF + k / CD) * CD + k % CD] = 1.0; ++nfree; }
  }
  for (int f = 0; f < FR; ++f) for (int q = 0; q < dp.P; ++q) {
    bool any_free = false;
    for (int k = 0; k < 6; ++k) any_free = any_free || h->mask_pose[((size_t)f * dp.P + q) * 6 + k] != 0.0;
    if (lead && any_free && frame_has_obs(f)) for (int k = 0; k < 6; ++k) { inprog_pose[((size_t)f * dp.P + q) * 6 + k] = 1.0; nfree += h->mask_pose[((size_t)f * dp.P + q) * 6 + k] != 0.0; }
  }
  for (int j = 0; j < M; ++j) if (h->mask_point[(size_t)j * 3] != 0.0 && point_ptr[j + 1] > point_ptr[j]) { for (int k = 0; k < 3; ++k) inprog_point[(size_t)j * 3 + k] = 1.0; nfree += 3; }
  s->num_reduced_params = nfree;
  {
    // residual blocks whose parameter blocks are all constant leave the program: every observation of a free point stays; those
    // of a constant point stay where the frame's poses or its intrinsics block are free (per point, not per observation)
    std::vector<uint8_t> frame_const((size_t)FR, 1);
    for (int f = 0; f < FR; ++f) {
      bool c = NIB == 0 || h->mask_intr[(size_t)intr_of(f) * 9] == 0.0;
      for (int k = 0; k < CD && c; ++k) c = h->mask_pose[(size_t)f * CD + k] == 0.0;
      frame_const[f] = c;
    }
    int64_t nred = 0;
    for (int j = 0; j < M; ++j) {
      if (h->mask_point[(size_t)j * 3] != 0.0) { nred += point_ptr[j + 1] - point_ptr[j]; continue; }
      for (int64_t x = point_ptr[j]; x < point_ptr[j + 1]; ++x) nred += !frame_const[slot_frame()[x]];
    }
    s->num_priors_reduced = 0;
    if (lead) for (int32_t f : h->prior_frames) {
      bool all_const = !h->prior_free;
      for (int k = 0; k < 24 && all_const; ++k) all_const = h->mask_pose[(size_t)(f - 1) * CD + k] == 0.0;
      s->num_priors_reduced += !all_const;
    }
    if (lead) {   // per-pose priors: a GoodPosePrior always keeps its free priorPoses block; a SphericalPrior on a constant pose is dropped
      s->num_priors_reduced += (int)h->pp_blocks.size();
      nfree += 6 * (int)h->pp_blocks.size();
      s->num_reduced_params = nfree;
      if (dp.pp_spherical >= 0) { bool all_const = true; for (int k = 0; k < 6; ++k) all_const = all_const && h->mask_pose[(size_t)dp.pp_spherical * 6 + k] == 0.0; s->num_priors_reduced += !all_const; }
    }
    s->num_reduced_blocks = (int)nred;
  }
}

int32_t PlanBuild::uploads() {
  std::vector<double>& inprog_point = scr.inprog_point;
  int32_t rc;
  sv.tile_factored = nullptr;
  if (factored) up->upload_const(&sv.tile_factored, tile_factored);
  sv.all_real_factored = factored ? 1 : 0;
  for (int t = 0; t < nt && (int64_t)t * FT < FR; ++t) if (!tile_factored[t]) sv.all_real_factored = 0;
  sv.fused_sweep = 0;   // (set once the plan knows its virtual groups, below)
  up->upload_const(&sv.tp_I, tp_I);
  up->upload_const(&sv.tp_J, tp_J);
  up->upload_const(&sv.tp_ptr, tp_ptr);
  up->upload_const(&sv.inprog_pose, inprog_pose);
  up->upload_const_ref(&sv.inprog_point, inprog_point);
  up->upload_const(&sv.inprog_intr, inprog_intr);
  std::vector<int32_t> ifp((size_t)NIB + 1, 0), ifl;       // (alive until the uploads have finished)
  std::vector<int64_t> point_vgroup((NIB == 1 && !dev_plan) ? (size_t)M : 0, -1);
  {
    for (int f = 0; f < FR && NIB > 0; ++f) ifp[intr_of(f) + 1]++;
    for (int c = 0; c < NIB; ++c) ifp[c + 1] += ifp[c];
    ifl.resize(NIB > 0 ? FR : 0);
    { std::vector<int32_t> fill(ifp.begin(), ifp.end() - 1); for (int f = 0; f < FR && NIB > 0; ++f) ifl[fill[intr_of(f)]++] = f; }
    up->upload_const(&sv.intr_frame_ptr, ifp);
    up->upload_const(&sv.intr_frame_list, ifl);
    if (dev_plan) { sv.vgroup_point = dpo.vgroup_point; sv.vgroup_intr = dpo.vgroup_intr; sv.point_vgroup = dpo.point_vgroup; }
    else {
      up->upload_const_ref(&sv.vgroup_point, vgroup_point);
      up->upload_const_ref(&sv.vgroup_intr, vgroup_intr);
      for (int j = 0; j < M && NIB == 1; ++j) if (vgroup_ptr[j + 1] > vgroup_ptr[j]) point_vgroup[j] = vgroup_ptr[j];
      up->upload_const(&sv.point_vgroup, point_vgroup);
    }
  }
  up->upload_const(&sv.chunk_tp, chunk_tp);
  up->upload_const(&sv.chunk_e0, chunk_e0);
  up->upload_const(&sv.tp_chunk0, tp_chunk0);
  up->upload_const(&sv.tp_chunk_list, tp_chunk_list);
  up->upload_const(&sv.chunk_n, chunk_n);
  std::vector<int4> chunk_info(chunk_tp.size());
  for (size_t c = 0; c < chunk_tp.size(); ++c) {
    const int I_ = tp_I[chunk_tp[c]], J_ = tp_J[chunk_tp[c]];
    chunk_info[c] = int4{(int)(uint32_t)(chunk_e0[c] & 0xffffffff), (int)(chunk_e0[c] >> 32), chunk_n[c], (I_ == J_ ? 1 : 0) | (tile_factored[I_] ? 2 : 0) | (tile_factored[J_] ? 4 : 0)};
  }
  up->upload_const(&sv.chunk_info, chunk_info);
  up->upload_const(&sv.pm_ptr, pm_ptr);
  up->upload_const(&sv.pm_list, pm_list);
  up->upload_const(&sv.tp_dst, tp_dst);
  std::vector<int32_t> exch_slots(tp_dst);   // (a tile pair has a packed tile of its own: distinct slots; ascending = the order they sit in memory)
  std::sort(exch_slots.begin(), exch_slots.end());
  s->exch_tiles = (int)exch_slots.size();
  if (h->allreduce) {
    up->upload(&s->exch_slots, exch_slots);
    if ((rc = s_alloc(s, &s->exch_buf, (size_t)exch_slots.size() * kTile * kTile + (size_t)sv.npad))) return rc;
  }
  up->upload_const(&sv.tp_trans, tp_trans);
  up->upload_const(&sv.tp_add, tp_add);
  {
    // one 64-byte line per pair for the merge kernel (kernels_schur.hip, PairDesc): what it used to collect from five arrays in two dependent rounds
    std::vector<int32_t> tp_desc((size_t)ntp * 16, 0);
    for (int t = 0; t < ntp; ++t) {
      int32_t* d = tp_desc.data() + (size_t)t * 16;
      d[0] = tp_I[t]; d[1] = tp_J[t]; d[2] = tp_dst[t];
      d[3] = (tp_trans[t] ? 1 : 0) | (tile_factored[tp_I[t]] ? 2 : 0) | (tile_factored[tp_J[t]] ? 4 : 0);
      d[4] = tp_chunk0[t]; d[5] = tp_chunk0[t + 1];
      for (int u = 0; u < 8; ++u) d[8 + u] = tp_chunk0[t] + u < tp_chunk0[t + 1] ? tp_chunk_list[(size_t)tp_chunk0[t] + u] : -1;
    }
    up->upload_const(&sv.tp_desc, tp_desc);
  }
  if ((rc = s_alloc(s, &sv.schur_part, (size_t)std::max(sv.nchunk, 1) * (kTile * kTile + kTile)))) return rc;
  // the write-once cells of the persistent Cholesky driver — factor tiles | partial tiles | W | z, y | published X — live in ONE
  // allocation: one memset re-arms them before a launch (five launches before)
  {
    const size_t nLf = (size_t)sv.nslots * kTile * kTile, nPart = (size_t)std::max(hp.nparts, 1) * (kTile * kTile + kTile), nW = (size_t)nt * kTile * kTile, nZ = 3 * (size_t)sv.npad + 8;   // z | y | z2 | {s eta}
    s->ncells = nLf + nPart + nW + nZ + nW;
    s->cell_off[0] = 0; s->cell_off[1] = nLf; s->cell_off[2] = nLf + nPart; s->cell_off[3] = nLf + nPart + nW; s->cell_off[4] = nLf + nPart + nW + nZ;
    for (int b = 0; b < 2; ++b) {
      if ((rc = s_alloc(s, &s->cells[b], s->ncells))) return rc;
      RSBA_HIP_TRY(hipMemsetAsync(s->cells[b], 0xFF, s->ncells * sizeof(double), h->stream));   // both sets start out armed
    }
    RSBA_HIP_TRY(dev_stream_acquire(&s->mstream));
    for (int b = 0; b < 2; ++b) RSBA_HIP_TRY(dev_event_acquire(&s->ev_armed[b], false));
    RSBA_HIP_TRY(dev_event_acquire(&s->ev_released, false));
    RSBA_HIP_TRY(dev_event_acquire(&s->ev_fork, false));
    RSBA_HIP_TRY(dev_event_acquire(&s->ev_join, false));
    double* cells = s->cells[0];
    sv.Lf = cells; sv.chol_part = cells + nLf; sv.Winv = sv.chol_part + nPart; sv.zv = sv.Winv + nW; sv.yv = sv.zv + sv.npad; sv.Xpub = sv.zv + nZ;
    sv.zv2 = nullptr; sv.ceta = nullptr; sv.border2 = nullptr; sv.rt = nullptr;   // (set with the border, below)
  }
  if ((rc = s_alloc(s, &s->d_dag_sync, 4))) return rc;
  RSBA_HIP_TRY(hipMemsetAsync(s->d_dag_sync, 0, 4 * sizeof(unsigned int), h->stream));   // (the persistent kernel leaves its counters at zero behind every launch)
  if ((rc = s_alloc(s, &s->zy2, 2 * (size_t)sv.npad))) return rc;
  for (size_t i = 0; i < kNumPlanLists; ++i) if (sharded || (kPlanLists[i].plans & kPlanRep)) up->upload_ref(&s->d_plan_lists[i], hp.*kPlanLists[i].host);

  // ---- sharded factorisation: what the exchange between the two launches needs ----
  std::vector<double> frame_lead;   // (alive until the uploads have finished)
  sv.frame_lead = nullptr;
  if (sharded) {
    s->ntop_slots = (int)hp.top_slots.size(); s->ntop_tiles = (int)hp.top_tiles.size(); s->ntop_fill = (int)hp.top_fill.size();
    // who adds the replicated terms (damping, gradient, identity padding) of a camera-side frame to its partial S: the rank that
    // owns the frame's part, rank 0 for the separators
    frame_lead.assign((size_t)nt * FT, 0.0);
    for (int a = 0; a < nt * FT; ++a) frame_lead[a] = hp.row_mine[a / FT] ? 1.0 : 0.0;
    up->upload_ref(&s->d_top_slots, hp.top_slots); up->upload_ref(&s->d_top_info, hp.top_info); up->upload_ref(&s->d_asm_ptr, hp.asm_ptr); up->upload_ref(&s->d_asm_list, hp.asm_list);
    up->upload_ref(&s->d_top_tiles, hp.top_tiles); up->upload_ref(&s->d_row_mine, hp.row_mine); up->upload_ref(&s->d_top_fill, hp.top_fill);
    up->upload_ref(&s->d_row_check, hp.row_check); up->upload_ref(&s->d_row_sep, hp.row_sep);
    up->upload_const(&sv.frame_lead, frame_lead);
    // (+ with a second right-hand side: the parts' share of the separators' rows of it, and of the two dots — behind the tiles and the rhs rows)
    if ((rc = s_alloc(s, &s->topx_buf, (size_t)s->ntop_slots * kTile * kTile + (size_t)s->ntop_tiles * kTile + (two_rhs ? (size_t)s->ntop_tiles * kTile + 8 : 0)))) return rc;
    if ((rc = s_alloc(s, &s->ybuf, (size_t)sv.npad))) return rc;
    if (two_rhs) RSBA_HIP_TRY(hipMemsetAsync(s->topx_buf + (size_t)s->ntop_slots * kTile * kTile + (size_t)s->ntop_tiles * kTile, 0, ((size_t)s->ntop_tiles * kTile + 8) * sizeof(double), h->stream));
  }
  RSBA_HIP_TRY(up->finish());
  tick("uploads");
  return RSBA_OK;
}

int32_t PlanBuild::allocations() {
  int32_t rc;
  const size_t REC = 2 + 2 * (size_t)dp.K;
  h->dp.obs_slot = s->d_obs_slot;
  // The point-side passes recompute the records (lm_record.hpp) from the observations in slot order; problems with several
  // intrinsics parameter blocks (per-frame f.cam) keep the point-major copy.  RSBA_RECORDS=1 forces the copy.
  sv.slot_xy = nullptr; h->dp.rec = nullptr; h->dp.rec_alt = nullptr; h->dp.rec_candidate = 0;   // (recompute: settled with the group layout above)
  if (recompute) {
    double2* sxy = nullptr;
    if ((rc = s_alloc(s, &sxy, (size_t)N))) return rc;
    RSBA_HIP_TRY(launch_slot_xy(h->dp, sxy, h->stream));
    sv.slot_xy = sxy;
  } else {
    if ((rc = s_alloc(s, &h->dp.rec, (size_t)N * REC))) return rc;
    // ... and a second set for a candidate's records (device_state.hpp: rec_alt): with it the candidate is evaluated in LM mode like everybody
    // else's, and problems that keep records — several intrinsics blocks (per-frame f.cam, CeresHandler.h:260,277) — run the loop whose
    // decisions are taken on the device.  RSBA_RECORDS_ALT=0: one set, candidates residual-only, the host decides (round 5's form; A/B)
    if (sw.records_alt) { if ((rc = s_alloc(s, &h->dp.rec_alt, (size_t)N * REC))) return rc; }
  }
  sv.fused_sweep = sv.slot_xy && !h->dp.calibrated && sv.CD == 12 && sv.all_real_factored != 0 && sv.NPF > 0 && sv.nvgroups > 0 && sv.NIB == 1 && !sw.no_fused_sweep;
  if (N > 0) {
    // camera (and intrinsics border) blocks inside the evaluation kernel: per (64-observation wave, frame it touches)
    // the 16 x 16 blocks on and below the diagonal of [Ji | Jc | r]^T [Ji | Jc | r]
    const int64_t nwaves = (int64_t)eval_num_blocks(N) * (kEvalBlock / 64);
    std::vector<int32_t> wave_seg_base((size_t)nwaves + 1, 0), frame_rank(FR, 0);
    { int rk = 0; for (int f = 0; f < FR; ++f) { frame_rank[f] = rk; if (frame_ptr[f + 1] > frame_ptr[f]) ++rk; } }
    for (int64_t w = 0; w < nwaves; ++w) {
      const int64_t a = w * 64, b = std::min<int64_t>(a + 64, N);
      wave_seg_base[w + 1] = wave_seg_base[w] + (a < N ? frame_rank[of[b - 1]] - frame_rank[of[a]] + 1 : 0);
    }
    int32_t *d_base = nullptr, *d_rank = nullptr;
    if ((rc = s_upload(s, &d_base, wave_seg_base))) return rc;
    if ((rc = s_upload(s, &d_rank, frame_rank))) return rc;
    const int nblk = cam_part_blocks((dp.K - 3) + 1);   // (device_state.hpp)
    if ((rc = s_alloc(s, &h->dp.cam_part, (size_t)std::max(wave_seg_base[nwaves], 1) * nblk * 256))) return rc;
    h->dp.wave_seg_base = d_base; h->dp.frame_rank = d_rank;
  }
  const size_t ucross_len = h->prior_frames.empty() ? 0 : (size_t)FR * CD * CD;
  if ((rc = s_alloc(s, &sv.U, (size_t)ucross_base + ucross_len))) return rc;
  if (ucross_len) { s->ucross = sv.U + ucross_base; s->ucross_len = ucross_len; RSBA_HIP_TRY(hipMemset(s->ucross, 0, ucross_len * sizeof(double))); }   // stays zero on the other ranks
  if (ucross_len && h->prior_free) {   // the ratio is one more camera-side unknown: a 1-wide dense border of S, handled by a second solve
    if ((rc = s_alloc(s, &s->border, (size_t)sv.npad))) return rc;
    if ((rc = s_alloc(s, &s->ratio4, kRtSize))) return rc;
    RSBA_HIP_TRY(hipMemset(s->ratio4, 0, kRtSize * sizeof(double)));
    RSBA_HIP_TRY(hipMemset(s->border, 0, (size_t)sv.npad * sizeof(double)));
    sv.zv2 = sv.zv + 2 * sv.npad; sv.ceta = sv.zv + 3 * sv.npad; sv.border2 = s->border; sv.rt = s->ratio4;
    if (lead) s->num_reduced_params += 1;
  }
  if ((rc = s_alloc(s, &sv.gc, (size_t)F * CD))) return rc;
  if ((rc = s_alloc(s, &sv.intr_part, (size_t)FR * 54))) return rc;
  if ((rc = s_alloc(s, &sv.trial_intr, 9 * (size_t)std::max(dp.NI, 1)))) return rc;
  RSBA_HIP_TRY(hipMemcpy(sv.trial_intr, dp.intr, 9 * (size_t)dp.NI * sizeof(double), hipMemcpyDeviceToDevice));
  if ((rc = s_alloc(s, &sv.V, (size_t)M * 6))) return rc;
  if ((rc = s_alloc(s, &sv.gp, (size_t)M * 3))) return rc;
  if ((rc = s_alloc(s, &sv.diag_c, (size_t)F * CD))) return rc;
  if ((rc = s_alloc(s, &sv.diag_p, (size_t)M * 3))) return rc;
  if ((rc = s_alloc(s, &sv.Linv, (size_t)M * 6))) return rc;
  if ((rc = s_alloc(s, &sv.z, (size_t)M * 3))) return rc;
  const size_t pm_doubles = (size_t)pt_total + kGroupFull;   // (+ the all-zero group)
  sv.zero_off = (uint32_t)pt_total;
  sv.lerp_rot = dp.interp_rotation && dp.shutter != 0;
  if ((rc = s_alloc(s, &sv.Pm, pm_doubles))) return rc;
  RSBA_HIP_TRY(hipMemsetAsync(sv.Pm, 0, pm_doubles * sizeof(double), h->stream));   // rows of frames that do not see the point stay zero for good: nothing ever writes them
  if ((rc = s_alloc(s, &sv.schur_next, 9 * 16))) return rc;
  RSBA_HIP_TRY(hipMemsetAsync(sv.schur_next, 0, 9 * 16 * sizeof(unsigned), h->stream));   // (every launch leaves the counters at zero: its last workgroup)
  if ((rc = s_alloc(s, &sv.schur_mfma_count, 1))) return rc;
  RSBA_HIP_TRY(hipMemsetAsync(sv.schur_mfma_count, 0, sizeof(unsigned long long), h->stream));

  if ((rc = s_alloc(s, &sv.S, (size_t)sv.nslots * kTile * kTile + (size_t)sv.npad))) return rc;
  sv.rhs = sv.S + (size_t)sv.nslots * kTile * kTile;   // one buffer = exchange payload (2)
  RSBA_HIP_TRY(hipMemsetAsync(sv.S, 0, ((size_t)sv.nslots * kTile * kTile + (size_t)sv.npad) * sizeof(double), h->stream));   // fill-only tiles stay zero for good
  if ((rc = s_alloc(s, &sv.udiag, (size_t)F * CD))) return rc;
  if ((rc = s_alloc(s, &sv.xbuf, 2 * (size_t)F * CD + 3 + kMaxRankSlots))) return rc;   // (+ the ranks' gradient maxima)
  if ((rc = s_alloc(s, &sv.yp, (size_t)M * 3))) return rc;
  if ((rc = s_alloc(s, &sv.trial_poses, (size_t)FR * CD))) return rc;
  if ((rc = s_alloc(s, &sv.trial_points, (size_t)M * 3))) return rc;
  const size_t nb = std::max<size_t>((N + 255) / 256, ((size_t)sv.n + 3 * (size_t)M + 255) / 256);
  if ((rc = s_alloc(s, &sv.partial, 2 * std::max(nb, ((size_t)M + 15) / 16 + 1) + 2))) return rc;   // (the point sweeps leave one partial per workgroup: 16 - 64 points)
  if ((rc = s_alloc(s, &sv.partial_c, 2 * (((size_t)sv.n + 3 * (size_t)M + 255) / 256) + 2))) return rc;
  if ((rc = s_alloc(s, &sv.scalars, 16))) return rc;
  if ((rc = s_alloc(s, &s->d_ctl, kCtlSize))) return rc;
  RSBA_HIP_TRY(hipMemset(s->d_ctl, 0, kCtlSize * sizeof(double)));
  sv.ctl = s->d_ctl;   // (in the device copies of the plan: the persistent Cholesky looks at the status word — zero while the host decides; launches by value get null then)
  if ((rc = s_alloc(s, &sv.chol_fail, 1))) return rc;
  if ((rc = s_alloc(s, &s->d_gpose, (size_t)F * CD))) return rc;
  if ((rc = s_alloc(s, &s->d_gpoint, (size_t)M * 3))) return rc;
  if (h->allreduce && h->world > 1) { if ((rc = s_alloc(s, &s->merge_buf, 4 * (size_t)M))) return rc; }
  if (dp.pp_count > 0) {
    const size_t n6 = 6 * (size_t)dp.pp_count;
    if ((rc = s_alloc(s, &s->pp.v0, n6))) return rc;
    if ((rc = s_alloc(s, &s->pp.g0, n6))) return rc;
    if ((rc = s_alloc(s, &s->pp.cross, n6))) return rc;
    if ((rc = s_alloc(s, &s->pp.diag, n6))) return rc;
    std::vector<int32_t> tds(nt);
    for (int t = 0; t < nt; ++t) tds[t] = hp.slot_base[hp.iperm[t]];
    if ((rc = s_upload_const(s, &s->pp.tile_diag_slot, tds))) return rc;
  }
  RSBA_HIP_TRY(hipMemset(sv.scalars, 0, 16 * sizeof(double)));
  RSBA_HIP_TRY(hipMemset(sv.chol_fail, 0, sizeof(int)));
  pl.ntasks = (int)(hp.tasks.size() / 2); pl.ndiag = (int)(hp.diag_info.size() / 4);
  pl.ticket = s->d_dag_sync;
  pl.nslots = sv.nslots; pl.nparts = hp.nparts;
  if (sharded) {
    s->plan_a = pl; s->plan_a.ntasks = (int)(hp.tasks_a.size() / 2);
    s->plan_b = pl; s->plan_b.ntasks = (int)(hp.tasks_b.size() / 2);
    if (two_rhs) {
      double* tail = s->topx_buf + (size_t)s->ntop_slots * kTile * kTile + (size_t)s->ntop_tiles * kTile;
      s->plan_a.fwd2_partial = tail; s->plan_a.eta_tiles = s->d_row_check; s->plan_a.eta_partial = tail + (size_t)s->ntop_tiles * kTile;
      s->plan_b.fwd2_minus = tail; s->plan_b.eta_tiles = s->d_row_sep; s->plan_b.eta_extra = tail + (size_t)s->ntop_tiles * kTile;
    }
  }
  {
    CholPlan* const plans[3] = {&s->plan, &s->plan_a, &s->plan_b};
    for (size_t i = 0; i < kNumPlanLists; ++i) for (int b = 0; b < (sharded ? 3 : 1); ++b) if (kPlanLists[i].plans & (1u << b)) plans[b]->*kPlanLists[i].field = s->d_plan_lists[i];
  }
  int cus = 0;
  RSBA_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
  // One persistent workgroup per CU — or two, for a WIDE task graph.  Claimed tasks that wait for their inputs hold a workgroup and the
  // schedule is short of them (192 instead of 256 workgroups cost 5 % at C4); the kernel is built so that two fit a CU (78 KB of LDS,
  // <= 256 registers per lane).  Through round 4 two per CU slowed the solve down by orders of magnitude: twice the waves polling AND every
  // operand load going to the memory side.  With the operand tiles looked ahead at through L2 (chol_tasks.hpp, Frag::load) that is gone:
  // 512 workgroups are stable (C5 7.54 - 7.64 ms per LM iteration in six runs against 7.86 - 7.96 with 256, 384 in between) where a level of
  // the elimination tree holds more tasks than there are CUs (C5: 380 per level), and change nothing where the chain dominates (C4: 116 per
  // level, 1.62 ms either way).  RSBA_CHOL_WGS overrides, capped at two per CU.
  s->dag_workgroups = std::max(1, std::min(pl.ntasks, std::max(cus, 1)));
  const int64_t my_tasks = sharded ? (int64_t)s->plan_a.ntasks + s->plan_b.ntasks : (int64_t)pl.ntasks;   // (what THIS rank runs)
  if (hp.nlev > 0 && my_tasks > (int64_t)hp.nlev * std::max(cus, 1)) { s->dag_workgroups = std::max(1, std::min(pl.ntasks, 2 * std::max(cus, 1))); s->dag_one_per_cu = false; }
  // A small plan (100 cameras: 267 tasks, ~15 per elimination level) is served better by a quarter as many workgroups as tasks — fewer
  // pollers around the chain: 0.428 -> 0.418 ms per iteration, three runs each — and leaves the rest of the chip to other streams.
  if (pl.ntasks <= 512) s->dag_workgroups = std::max(1, std::min(s->dag_workgroups, std::max(64, pl.ntasks / 4)));
  if (sw.chol_wgs) { s->dag_workgroups = std::max(1, std::min(std::min(pl.ntasks, 2 * std::max(cus, 1)), *sw.chol_wgs)); s->dag_one_per_cu = s->dag_workgroups <= cus; }
  if (sw.chol_trace) {
    if ((rc = s_alloc(s, &s->d_trace, 8 * (size_t)pl.ntasks))) return rc;
    RSBA_HIP_TRY(hipMemset(s->d_trace, 0, 8 * (size_t)pl.ntasks * sizeof(long long)));
  }
  pl.trace = s->d_trace;
  tick("allocations");
  return RSBA_OK;
}

// ---- the arguments of the persistent Cholesky driver, one device copy per set of cells ----
int32_t PlanBuild::dag_arguments() {
  int32_t rc;
  if (dbg_plan)
    std::fprintf(stderr, "[rsba plan] tiles %d, factor tiles %d, levels %d, tasks %d (partials %d); tile pairs %d, entries %lld, schur chunks %d\n", nt, sv.nslots,
                 hp.nlev, pl.ntasks, hp.nparts, sv.ntp, (long long)s->num_pairs, sv.nchunk);
  s->use_levels = sw.chol_levels_before_solve;   // (for covariance calls before any solve: rsba_solve settles it again)
  DagArgs host_args{sv, pl};
  if ((rc = s_upload(s, &s->d_slot_tiles, hp.slot_tiles))) return rc;
  if ((rc = s_alloc(s, &s->d_verify, 2 * (size_t)sv.npad))) return rc;
  if ((rc = s_alloc(s, &s->verify_b, (size_t)sv.npad))) return rc;
  RSBA_HIP_TRY(dev_stream_acquire(&s->vstream));
  RSBA_HIP_TRY(dev_event_acquire(&s->ev_solved, false));
  RSBA_HIP_TRY(dev_event_acquire(&s->ev_verified, false));
  RSBA_HIP_TRY(hipMemset(s->d_verify, 0, 2 * (size_t)sv.npad * sizeof(double)));   // the check kernel leaves it zero again
  s->test_corrupt_once = sw.test_chol_corrupt;
  for (int b = 0; b < 2; ++b) {   // one device copy of {sv, plan} per set of cells
    double* c = s->cells[b];
    host_args.sv.Lf = c + s->cell_off[0]; host_args.sv.chol_part = c + s->cell_off[1]; host_args.sv.Winv = c + s->cell_off[2];
    host_args.sv.zv = c + s->cell_off[3]; host_args.sv.yv = host_args.sv.zv + sv.npad; host_args.sv.Xpub = c + s->cell_off[4];
    if (sv.zv2) { host_args.sv.zv2 = host_args.sv.zv + 2 * sv.npad; host_args.sv.ceta = host_args.sv.zv + 3 * sv.npad; }
    if ((rc = s_alloc(s, &s->d_dag_args2[b], 1))) return rc;
    RSBA_HIP_TRY(hipMemcpy(s->d_dag_args2[b], &host_args, sizeof host_args, hipMemcpyHostToDevice));
    if (sharded) {
      DagArgs a = host_args, bb = host_args;
      a.pl = s->plan_a; bb.pl = s->plan_b;
      if ((rc = s_alloc(s, &s->d_dag_args_a[b], 1))) return rc;
      if ((rc = s_alloc(s, &s->d_dag_args_b[b], 1))) return rc;
      RSBA_HIP_TRY(hipMemcpy(s->d_dag_args_a[b], &a, sizeof a, hipMemcpyHostToDevice));
      RSBA_HIP_TRY(hipMemcpy(s->d_dag_args_b[b], &bb, sizeof bb, hipMemcpyHostToDevice));
    }
  }
  s->d_dag_args = s->d_dag_args2[0];
  return RSBA_OK;
}

void PlanBuild::statistics() {
  rsba_plan_stats& ps = s->stats;
  ps.tiles = nt; ps.factor_tiles = sv.nslots; ps.levels = hp.nlev; ps.tasks = pl.ntasks;
  ps.schur_entries = nent; ps.schur_chunks = sv.nchunk;
  // block products of the Schur complement that are not structurally zero: per entry (frames present on the I side) x (on the J side),
  // summed in the pass that forms the entries' block masks
  ps.schur_block_products = 0;
  for (int64_t v : products_part) ps.schur_block_products += v;
  ps.cholesky_flops = hp.cholesky_flops;
  ps.exchange_doubles = (int64_t)s->exch_tiles * kTile * kTile + sv.npad;   // exchange (2) of a sharded solve: the plan's tile pairs | rhs (the fill-in tiles of the factor's layout stay home)
  ps.schur_groups = sv.ngroups;
  ps.schur_group_bytes = pt_total * (int64_t)sizeof(double);
  ps.schur_factored_groups = dev_plan ? dpo.factored_groups : 0;
  for (int64_t g = 0; g < sv.ngroups && !dev_plan; ++g) ps.schur_factored_groups += tile_factored[g_tile[(size_t)g]];
  ps.sharded_factorisation = sharded ? 1 : 0;
  if (sharded) {   // ... or, when every rank factors its own part: the separators' tiles | their rows of the rhs, and the gather of the step
    ps.exchange_doubles = (int64_t)s->ntop_slots * kTile * kTile + (int64_t)s->ntop_tiles * kTile + sv.npad;
    ps.separator_tiles = s->ntop_tiles; ps.separator_factor_tiles = s->ntop_slots;
    ps.local_tasks = (int64_t)(hp.tasks_a.size() / 2); ps.separator_tasks = (int64_t)(hp.tasks_b.size() / 2);
    ps.local_levels = hp.local_levels; ps.separator_levels = hp.separator_levels;
  }
}

int32_t build_solver_impl(rsba_handle* h) {
  Solver* s = new Solver();
  h->solver = s;   // owned by the handle from here on (freed by rsba_destroy_solver)
  s->sw = PlanSwitches::read();   // the environment, once: every stage reads the fields (switches.hpp)
  s->solve_sw = SolveSwitches::read(Solver::kCtlRing);   // (what a step called before any solve goes by)
  PlanBuild b(h, s);
  int32_t rc;
  b.settle_switches();
  if ((rc = b.dev_plan ? b.lists_on_device() : b.lists_on_host())) return rc;
  b.sv.nvgroups = b.NVG;
  b.ntp = (int)b.tp_I.size();
  s->num_pairs = b.nent;
  b.order_and_symbolic();
  if ((rc = b.vote()) || (rc = b.split_motion_priors())) return rc;
  b.task_graph();
  if ((rc = b.schur_chunks())) return rc;
  b.pair_tiles();
  b.reduced_program();
  if ((rc = b.uploads()) || (rc = b.allocations()) || (rc = b.dag_arguments())) return rc;
  b.statistics();
  b.sv.ctl = nullptr;
  b.tick("statistics");
  RSBA_HIP_TRY(hipStreamSynchronize(h->stream));   // the plan's one-time fills and scatters are done whatever stream the solves will run on
  b.tick("device fills");
  if (b.dbg_plan) std::fprintf(stderr, "[rsba plan] host phases:%s\n", b.phases.c_str());
  return RSBA_OK;
}

}  // namespace

// A plan that failed half-way (out of memory, an unsupported size) must not be taken for a finished one by the next call: the
// half-built solver is torn down again, so that a retry builds — and fails — afresh instead of launching kernels on null tables.
int32_t rsba::build_solver(rsba_handle* h) {
  if (h->solver) return RSBA_OK;
  const int32_t rc = build_solver_impl(h);
  if (rc != RSBA_OK) {
    const std::string why = rsba_last_error();   // (the teardown must not lose what went wrong)
    rsba_destroy_solver(h);
    return rsba_set_error(rc, why.c_str());
  }
  return RSBA_OK;
}

void rsba_release_plan_scratch() {
  std::lock_guard<std::mutex> lk(g_plan_scratch_mutex);
  g_plan_scratch.reset();
}

void rsba_destroy_solver(rsba_handle* h) {
  if (!h || !h->solver) return;
  const bool dbg = h->solver->sw.debug_plan;
  const double td0 = dbg ? now_s() : 0.0;
  // streams, events and the pinned block go back to the pool (devmem.hpp): idle first — the main stream too, whose last waits name these events
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->solver->vstream) { (void)hipStreamSynchronize(h->solver->vstream); dev_stream_release(h->solver->vstream); }
  if (h->solver->mstream) { (void)hipStreamSynchronize(h->solver->mstream); dev_stream_release(h->solver->mstream); }
  for (hipEvent_t e : {h->solver->ev_armed[0], h->solver->ev_armed[1], h->solver->ev_released, h->solver->ev_solved, h->solver->ev_verified, h->solver->ev_fork, h->solver->ev_join}) dev_event_release(e, false);
  dev_pinned_release(h->solver->h_ctl);
  if (h->solver->sv.schur_trace && h->solver->sw.schur_trace) {   // debugging aid: stamps of the last Schur launch
    std::vector<long long> tr(8 * (size_t)h->solver->sv.nchunk);
    if (hipMemcpy(tr.data(), h->solver->sv.schur_trace, tr.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess)
      if (FILE* f = std::fopen(h->solver->sw.schur_trace->c_str(), "wb")) { std::fwrite(tr.data(), sizeof(long long), tr.size(), f); std::fclose(f); }
  }
  const double td1 = dbg ? now_s() : 0.0;
  if (h->stream) (void)hipStreamSynchronize(h->stream);   // (the side streams above are idle too: the blocks go back to the cache, devmem.hpp)
  const double td2 = dbg ? now_s() : 0.0;
  for (void* p : h->solver->allocs) dev_free(p);
  for (double* p : {h->solver->cov.sigma, h->solver->cov.g, h->solver->cov.live, h->solver->cov.vdev}) if (p) dev_free(p);
  const double td3 = dbg ? now_s() : 0.0;
  delete h->solver;
  if (dbg) std::fprintf(stderr, "[rsba destroy] plan: streams + events to the pool %.2f ms; stream sync %.2f ms; blocks to the cache %.2f ms; host state %.2f ms\n", 1e3 * (td1 - td0), 1e3 * (td2 - td1), 1e3 * (td3 - td2), 1e3 * (now_s() - td3));
  h->solver = nullptr;
  if (h->prior_split) { h->dp.prior_of = h->prior_of_all; h->prior_invalid = h->prior_invalid_all; h->prior_split = false; }   // the rank's share of the priors was a table of the plan
  h->dp.rec = nullptr; h->dp.rec_alt = nullptr; h->dp.rec_candidate = 0; h->dp.obs_slot = nullptr; h->dp.cam_part = nullptr; h->dp.wave_seg_base = nullptr; h->dp.frame_rank = nullptr;
}
