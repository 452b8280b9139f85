// rsba_partition_points (include/rsba_amd.h): which rank of a sharded solve owns which point — host only, no device.
// The reference is single-process (/root/reference/src/rsba/CeresHandler.h:394-426); the partition is the cut SURVEY §8e derives for
// the path — by point, cameras replicated — placed so that the reduced camera system can be FACTORED where it is formed: along the
// top separators of the nested dissection of its tile graph (tile_order.hpp).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "handle.hpp"
#include "solver_state.hpp"
#include "tile_order.hpp"
#include "chol_plan.hpp"

using namespace rsba;

namespace {

// the cut (part_of: per tile column, -1 = a separator) and the owners of the points
int32_t partition(const rsba_problem_desc* d, int32_t world, int32_t* owner, int32_t* num_top_tiles, std::vector<int32_t>& part_of) {
  if (!d || !owner || world < 1) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad partition arguments");
  const int P = d->poses_per_frame;
  if (P != 1 && P != 2) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "poses_per_frame must be 1 or 2");
  const TileLayout lay(P, d->num_frames, d->calibrated != 0, d->num_intrinsics);
  const int FR = lay.FR, M = d->num_points, NIB = lay.NIB, NPF = lay.NPF, nt = lay.nt;
  const int64_t N = d->num_observations;
  if (num_top_tiles) *num_top_tiles = 0;
  if (world == 1 || N == 0) { std::fill(owner, owner + M, 0); part_of.assign(nt, 0); return RSBA_OK; }
  for (int64_t i = 0; i < N; ++i)
    if (d->obs_frame[i] < 0 || d->obs_frame[i] >= FR || d->obs_point[i] < 0 || d->obs_point[i] >= M) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "observation index out of range");
  auto intr_of = [&](int f) { return (NIB > 1 && d->frame_intrinsics) ? d->frame_intrinsics[f] : 0; };
  // the tiles every point is seen in (real frames and, with intrinsics as parameter blocks, the pseudo frames of the blocks it is seen through)
  std::vector<int64_t> ptr((size_t)M + 1, 0);
  for (int64_t i = 0; i < N; ++i) ptr[d->obs_point[i] + 1]++;
  for (int j = 0; j < M; ++j) ptr[j + 1] += ptr[j];
  std::vector<int32_t> fr((size_t)N);
  { std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1); for (int64_t i = 0; i < N; ++i) fr[fill[d->obs_point[i]]++] = d->obs_frame[i]; }
  std::vector<uint8_t> pair((size_t)nt * nt, 0);
  std::vector<double> weight(nt, 0.0);
  for (int64_t i = 0; i < N; ++i) weight[lay.frame_tile(d->obs_frame[i])] += 1.0;
  std::vector<int32_t> tiles;
  auto tiles_of = [&](int j) {
    tiles.clear();
    for (int64_t x = ptr[j]; x < ptr[j + 1]; ++x) {
      tiles.push_back(lay.frame_tile(fr[x]));
      for (int v = 0; v < NPF; ++v) tiles.push_back(lay.pseudo_tile(intr_of(fr[x]), v));
    }
    std::sort(tiles.begin(), tiles.end()); tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
  };
  for (int j = 0; j < M; ++j) {
    tiles_of(j);
    for (size_t a = 0; a < tiles.size(); ++a) for (size_t b = 0; b < a; ++b) pair[(size_t)tiles[a] * nt + tiles[b]] = 1;
  }
  for (int f = 0; f < FR && NIB > 0; ++f) for (int v = 0; v < NPF; ++v) { const int a = lay.pseudo_tile(intr_of(f), v), b = lay.frame_tile(f); if (a != b) pair[(size_t)std::max(a, b) * nt + std::min(a, b)] = 1; }
  for (int c = 0; c < NIB; ++c) for (int v = 0; v < NPF; ++v) for (int w = 0; w < v; ++w) { const int a = lay.pseudo_tile(c, v), b = lay.pseudo_tile(c, w); if (a != b) pair[(size_t)std::max(a, b) * nt + std::min(a, b)] = 1; }
  std::vector<std::vector<int32_t>> adj(nt);
  for (int a = 0; a < nt; ++a) for (int b = 0; b < a; ++b) if (pair[(size_t)a * nt + b]) { adj[a].push_back(b); adj[b].push_back(a); }
  for (auto& l : adj) std::sort(l.begin(), l.end());
  const TileOrder ord = nested_dissection(nt, adj, plan_leaf_size(world, nt), world, &weight);
  if (!ord.parts_ok) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "the co-visibility graph cannot be cut into that many parts (too few frames, or not connected)");
  int ntop = 0;
  for (int t = 0; t < nt; ++t) ntop += ord.part_of[t] < 0;
  if (num_top_tiles) *num_top_tiles = ntop;
  // a point belongs to the part of any of its tiles — real frames' and the pseudo frames' of the blocks it is seen through — that has
  // one (its tiles are a clique of the graph cut above, so at most one part is among them); points whose tiles are all separator
  // tiles touch only what every rank shares, so any rank may own them: they go, in point order, to whoever holds the fewest
  // observations so far.  (A point seen in separator frames only may still be seen through a block whose pseudo tile is in a part.)
  std::vector<int64_t> load(world, 0);
  for (int j = 0; j < M; ++j) {
    int own = -1;
    tiles_of(j);
    for (int32_t t : tiles) {
      const int p = ord.part_of[t];
      if (p < 0) continue;
      if (own >= 0 && own != p) return rsba_set_error(RSBA_ERR_HIP, "internal: a point is seen on both sides of a separator");
      own = p;
    }
    owner[j] = own;
    if (own >= 0) load[own] += ptr[j + 1] - ptr[j];
  }
  for (int j = 0; j < M; ++j) if (owner[j] < 0) {
    const int own = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    owner[j] = own; load[own] += ptr[j + 1] - ptr[j];
  }
  part_of = ord.part_of;
  return RSBA_OK;
}

}  // namespace

extern "C" int32_t rsba_partition_points(const rsba_problem_desc* d, int32_t world, int32_t* owner, int32_t* num_top_tiles) {
  std::vector<int32_t> part_of;
  return partition(d, world, owner, num_top_tiles, part_of);
}

#ifdef RSBA_TEST_HOOKS
// instrumented build only (not part of include/rsba_amd.h): the part of every tile column (-1 = a separator) of the cut
// rsba_partition_points computes — real frames' tiles first, then the intrinsics blocks' pseudo frames'.  part_of == NULL: only
// *num_tiles; otherwise part_of holds *num_tiles entries (the tile count of the problem; the caller asks for it first).
extern "C" int32_t rsba_debug_partition_tiles(const rsba_problem_desc* d, int32_t world, int32_t* part_of, int32_t* num_tiles) {
  if (!d || !num_tiles || d->num_points < 0 || (d->poses_per_frame != 1 && d->poses_per_frame != 2)) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad partition arguments");
  const int nt = TileLayout(d->poses_per_frame, d->num_frames, d->calibrated != 0, d->num_intrinsics).nt;
  if (!part_of) { *num_tiles = nt; return RSBA_OK; }
  if (*num_tiles != nt) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "num_tiles is not the problem's tile count");
  std::vector<int32_t> owner((size_t)std::max(d->num_points, 1)), parts;
  if (const int32_t rc = partition(d, world, owner.data(), nullptr, parts)) return rc;
  std::copy(parts.begin(), parts.end(), part_of);
  return RSBA_OK;
}

// ... and the Cholesky plan (chol_plan.hpp) of a tile graph given as nt tiles and num_edges pairs {a, b}, as rank `rank` of `world`
// ranks would build it: ordered as the solver orders it (the leaf size from RSBA_CHOL_LEAF), sharded when the graph can be cut into
// `world` parts, every tile pair of the graph a tile pair of S.  emit(ctx, name, data, count) is called once per list — and once
// with "meta" = {sharded, levels, partial tiles, packed slots}; the data does not outlive the call.
namespace {
int32_t debug_plan_of_graph(int32_t nt, int32_t num_edges, const int32_t* edges, int32_t world, int32_t rank, int32_t two_rhs, const CholPlanOptions& opt, CholHostPlan* out) {
  std::vector<std::vector<int32_t>> adj(nt);
  std::vector<int32_t> pair_I, pair_J;
  for (int t = 0; t < nt; ++t) { pair_I.push_back(t); pair_J.push_back(t); }
  for (int e = 0; e < num_edges; ++e) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if (a < 0 || a >= nt || b < 0 || b >= nt || a == b) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad edge");
    adj[a].push_back(b); adj[b].push_back(a);
  }
  for (int t = 0; t < nt; ++t) {
    std::sort(adj[t].begin(), adj[t].end()); adj[t].erase(std::unique(adj[t].begin(), adj[t].end()), adj[t].end());
    for (int32_t u : adj[t]) if (u < t) { pair_I.push_back(t); pair_J.push_back(u); }
  }
  const TileOrder ord = nested_dissection(nt, adj, plan_leaf_size(world, nt), world);
  CholHostPlan& hp = *out;
  chol_symbolic(nt, adj, ord, &hp);
  CholTaskInput in;
  in.order = &ord; in.sharded = world > 1 && ord.parts_ok; in.rank = rank; in.two_rhs = two_rhs != 0; in.pair_I = &pair_I; in.pair_J = &pair_J;
  in.opt = opt;
  chol_tasks(in, &hp);
  return RSBA_OK;
}
}  // namespace

extern "C" int32_t rsba_debug_chol_plan(int32_t nt, int32_t num_edges, const int32_t* edges, int32_t world, int32_t rank, int32_t two_rhs, int32_t chunk, int32_t tail,
                                        int32_t fuse_last, void (*emit)(void* ctx, const char* name, const int32_t* data, int64_t count), void* ctx) {
  if (nt < 1 || num_edges < 0 || (num_edges && !edges) || world < 1 || rank < 0 || rank >= world || tail < 1 || chunk < tail || !emit) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad plan arguments");
  CholPlanOptions opt;
  opt.chunk = chunk; opt.tail = tail; opt.fuse_last = fuse_last != 0;
  CholHostPlan hp;
  if (const int32_t rc = debug_plan_of_graph(nt, num_edges, edges, world, rank, two_rhs, opt, &hp)) return rc;
  const std::vector<int32_t> meta{hp.sharded, hp.nlev, hp.nparts, hp.nslots};
  emit(ctx, "meta", meta.data(), (int64_t)meta.size());
  auto bytes = [&](const char* name, const std::vector<uint8_t>& v) { const std::vector<int32_t> w(v.begin(), v.end()); emit(ctx, name, w.data(), (int64_t)w.size()); };
#define RSBA_EMIT(x) emit(ctx, #x, hp.x.data(), (int64_t)hp.x.size())
  RSBA_EMIT(perm); RSBA_EMIT(slot_tiles); RSBA_EMIT(level); RSBA_EMIT(cpart); RSBA_EMIT(lev_diag_ptr); RSBA_EMIT(lev_sub_ptr); RSBA_EMIT(lev_upd_ptr);
  RSBA_EMIT(upd); RSBA_EMIT(upd_owner); RSBA_EMIT(diag_info); RSBA_EMIT(diag_ptr); RSBA_EMIT(diag_list); RSBA_EMIT(diag_own); RSBA_EMIT(diag_fuse);
  RSBA_EMIT(sub_info); RSBA_EMIT(sub_ptr); RSBA_EMIT(sub_list); RSBA_EMIT(sub_own); RSBA_EMIT(sub_col); RSBA_EMIT(sub_pub);
  RSBA_EMIT(back_info); RSBA_EMIT(back_ptr); RSBA_EMIT(back_list); RSBA_EMIT(tasks); RSBA_EMIT(fwd_full); RSBA_EMIT(diag_toprow);
  RSBA_EMIT(tasks_a); RSBA_EMIT(tasks_b); RSBA_EMIT(fwd_a); RSBA_EMIT(fwd_b); RSBA_EMIT(diag_info_sh); RSBA_EMIT(sub_info_sh);
  RSBA_EMIT(top_slots); RSBA_EMIT(top_info); RSBA_EMIT(asm_ptr); RSBA_EMIT(asm_list); RSBA_EMIT(top_tiles); RSBA_EMIT(top_fill);
#undef RSBA_EMIT
  bytes("row_mine", hp.row_mine); bytes("row_check", hp.row_check); bytes("row_sep", hp.row_sep);
  return RSBA_OK;
}

// ... and the selected-inverse plan (chol_plan.hpp: selinv_plan) over the replicated Cholesky plan of the same tile graph, one rank: the
// lists by name, "meta" = {levels, packed slots, tiles}, and what a check needs of the Cholesky plan beside them (perm, slot_tiles, level).
extern "C" int32_t rsba_debug_selinv_plan(int32_t nt, int32_t num_edges, const int32_t* edges,
                                          void (*emit)(void* ctx, const char* name, const int32_t* data, int64_t count), void* ctx) {
  if (nt < 1 || num_edges < 0 || (num_edges && !edges) || !emit) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad plan arguments");
  CholHostPlan hp;
  if (const int32_t rc = debug_plan_of_graph(nt, num_edges, edges, 1, 0, 0, CholPlanOptions{}, &hp)) return rc;
  SelinvHostPlan sp;
  int bi = -1, bk = -1;
  if (!selinv_plan(hp, &sp, &bi, &bk)) return rsba_set_error(RSBA_ERR_UNSUPPORTED, ("selected inverse: tile (" + std::to_string(bi) + ", " + std::to_string(bk) + ") of the fill pattern has no slot").c_str());
  const std::vector<int32_t> meta{sp.nlev, hp.nslots, hp.nt};
  emit(ctx, "meta", meta.data(), (int64_t)meta.size());
#define RSBA_EMIT(o, x) emit(ctx, #x, o.x.data(), (int64_t)o.x.size())
  RSBA_EMIT(hp, perm); RSBA_EMIT(hp, slot_tiles); RSBA_EMIT(hp, level);
  RSBA_EMIT(sp, lev_g_ptr); RSBA_EMIT(sp, lev_off_ptr); RSBA_EMIT(sp, lev_diag_ptr); RSBA_EMIT(sp, g_info);
  RSBA_EMIT(sp, off_info); RSBA_EMIT(sp, off_ptr); RSBA_EMIT(sp, off_list); RSBA_EMIT(sp, diag_info); RSBA_EMIT(sp, diag_ptr); RSBA_EMIT(sp, diag_list);
#undef RSBA_EMIT
  return RSBA_OK;
}
#endif
