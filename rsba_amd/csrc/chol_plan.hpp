// The tile Cholesky of the reduced camera system as the HOST plans it: the symbolic factorisation of the ordered tile graph and the
// task graph the device runs over it (cholesky.hip, chol_tasks.hpp) — which UPDATE / DIAG / SUB / BACK / FWD2 / ETA items exist, who owns them, in
// what ticket order, which contributors are chunked or fused.  Index arithmetic only: no device, no handle, no environment — the
// caller (solver_plan.hip) reads the switches and passes values in, and the lists can be checked without a GPU (tests/test_chol_plan.py).
//
// Two calls, because the ranks of a sharded solve vote on the form of the plan between them (the vote needs part_of):
//   chol_symbolic  — col / row after fill, the packed tile slots
//   chol_tasks     — levels, items, chunking, ticket orders; for a sharded plan the two launches' orders and the separators' tables
#pragma once
#include <cstdint>
#include <vector>

#include "tile_order.hpp"

namespace rsba {

// FWD2: item = DIAG item whose column's z2 it forms; FWD2P: the same item's sum over THIS rank's part only (sharded: what travels)
enum : int { kTaskUpdate = 0, kTaskDiag = 1, kTaskSub = 2, kTaskBack = 3, kTaskFwd2 = 4, kTaskEta = 5, kTaskFwd2P = 6 };

struct CholPlanOptions {
  int chunk = 12, tail = 2;   // contributors per UPDATE item; contributors the owner of a tile keeps for itself (1 <= tail <= chunk)
  bool fuse_last = true;      // the DIAG task forms the product with its last contributor itself (look-ahead on the critical chain)
};

struct CholTaskInput {
  const TileOrder* order = nullptr;   // the order chol_symbolic was given
  bool sharded = false;               // every rank factors its own part, then all of them the separators (order->part_of)
  int rank = 0;                       // ... and this is the plan of that rank
  bool two_rhs = false;               // a second right-hand side rides through the factorisation (FWD2 / ETA tasks)
  const std::vector<int32_t>*pair_I = nullptr, *pair_J = nullptr;   // sharded: the Schur tile pairs (old numbering) — a separator tile without one is fill only
  CholPlanOptions opt;
};

struct CholHostPlan {
  // ---- chol_symbolic ----
  int nt = 0, nslots = 0;
  std::vector<int32_t> perm, iperm;             // perm[new] = old tile and its inverse
  std::vector<std::vector<int32_t>> col, row;   // new order: col[k] = rows i > k of column k (after fill), row[j] = columns k < j of row j
  std::vector<int32_t> slot_base;               // [nt + 1] packed tile slots, column by column: (k, k) first, then the tiles of col[k]
  std::vector<int32_t> slot_tiles;              // [nslots][2] {row tile, column tile} (old numbering) of every packed tile
  // slot of tile (i, k), new indices, i >= k; -1 if the tile is structurally zero
  int32_t slot_of(int i, int k) const;

  // ---- chol_tasks ----
  bool sharded = false, two_rhs = false;
  int nlev = 0, nparts = 0;                     // elimination levels; partial tiles of the UPDATE items
  std::vector<int32_t> level, cpart;            // per column (new order): its level; the rank whose part holds it, -1 = a separator / not sharded
  std::vector<int32_t> lev_diag_ptr, lev_sub_ptr, lev_upd_ptr;   // [nlev + 1] ranges of DIAG / SUB / UPDATE items per level
  // The items.  {part0, n} = the partial tiles that arrive from the item's UPDATE items; *_own = the first contributor the owner multiplies itself.
  std::vector<int32_t> upd, upd_owner;          // {kind 0 diag / 1 sub, list begin, list end, partial tile}; rank that runs it (-1: every rank)
  std::vector<int32_t> diag_info, diag_ptr, diag_list, diag_own;   // per column: {slot_jj, old tile, part0, n}; contributors {slot_jk, old tile k}
  std::vector<int32_t> diag_fuse;               // per column j: SUB item of tile (j, k*), k* = its last contributor, which the DIAG task forms itself (-1: none)
  std::vector<int32_t> sub_info, sub_ptr, sub_list, sub_own;       // per tile (i, j): {slot_ij, slot_jj, part0, n}; contributors {slot_ik, slot_jk}
  std::vector<int32_t> sub_col;                 // per SUB item: old tile of its column (W_j, z_j)
  std::vector<int32_t> sub_pub;                 // per SUB item: DIAG item that wants its X = S_ij - updates published, -1: nobody
  std::vector<int32_t> back_info, back_ptr, back_list;             // per column: {slot_jj, old tile}; tiles {slot_ij, old tile i}, bottom-up
  std::vector<int32_t> tasks;                   // {kind, item} in a topological order, backward solve last
  std::vector<int32_t> fwd_full, diag_toprow;   // second right-hand side, per DIAG item: contributor range a FWD2 task sums over; index of its column among the separators' (-1: a part's)
  // sharded: launch A = this rank's part, forward; launch B = the separators, forward and backward, then this rank's part backward
  std::vector<int32_t> tasks_a, tasks_b, fwd_a, fwd_b;
  std::vector<int32_t> diag_info_sh, sub_info_sh;   // {.., part0, n} of the separators' items without the parts' partials (the exchange has summed those in)
  // ... and what the exchange between the launches needs, separator tile by separator tile (column by column):
  std::vector<int32_t> top_slots, top_info;     // its slot; {has a tile pair (else: fill only, zero in S), index among top_tiles of its row of the rhs or -1}
  std::vector<int32_t> asm_ptr, asm_list;       // THIS rank's partial tiles that subtract from it
  std::vector<int32_t> top_tiles, top_fill;     // the separators' tile columns (old numbering, ascending new order); the slots that are fill only
  std::vector<uint8_t> row_mine, row_check, row_sep;   // [nt] old tiles whose rows of y this rank contributes (its part; rank 0: the separators) / can check (its part) / separators
  // statistics (rsba_plan_stats)
  int64_t cholesky_flops = 0;
  int local_levels = 0, separator_levels = 0;   // sharded: the two dependency chains — levels inside this rank's part, levels that hold a separator column
};

void chol_symbolic(int nt, const std::vector<std::vector<int32_t>>& adj, const TileOrder& order, CholHostPlan* hp);
void chol_tasks(const CholTaskInput& in, CholHostPlan* hp);   // (hp: what chol_symbolic left)

// The selected inverse: every tile of Sigma = S^-1 ON THE FACTOR'S OWN PATTERN from the factor (W_j = L_jj^-1 on the diagonal, L_ij
// below), by the Takahashi recurrence — with J = col[j], the sub-diagonal row tiles of column j after fill:
//   G    per tile (k, j), k in J:   G_kj     = L_kj W_j
//   OFF  per tile (i, j), i in J:   Sigma_ij = - sum_{k in J} Sigma_ik G_kj      (Sigma_ik from slot (i, k) if i >= k, else slot (k, i) transposed)
//   DIAG per column j:              Sigma_jj = W_j^T W_j - sum_{k in J} Sigma_kj^T G_kj      (then symmetrised)
// Columns are taken level by level, DESCENDING: the columns of one level are not ancestors of each other, an OFF item reads Sigma
// tiles of higher levels only, a DIAG item those and the OFF outputs of its own column — one launch per (level, kind), nobody waits
// for anybody inside one (kernels_selinv.hip).  The sums run in the order of col[j]: fixed, so two runs agree bit for bit.
// Position p of the lev_*_ptr tables is elimination level nlev - 1 - p.  Sigma and G tiles use the factor's packed slots.
struct SelinvHostPlan {
  int nlev = 0;
  std::vector<int32_t> lev_g_ptr, lev_off_ptr, lev_diag_ptr;   // [nlev + 1] ranges of the G / OFF / DIAG items per position
  std::vector<int32_t> g_info;                                 // per G item: {slot_kj (of L, and of G), old tile of j (W_j)}
  std::vector<int32_t> off_info, off_ptr, off_list;            // per OFF item: {slot_ij, old tile of j}; terms {slot of Sigma_ik or Sigma_ki, 1 = read it transposed, slot_kj of G}
  std::vector<int32_t> diag_info, diag_ptr, diag_list;         // per DIAG item: {slot_jj, old tile of j}; terms {slot_kj of Sigma and of G}
  int64_t flops = 0;                                           // 2 T^3 per tile product
};
// false (and *bad_i, *bad_k = the new indices of the pair, when given) if some (i, k), i, k in col[j], has no slot: fill closure says
// it has one, the plan checks instead of assuming it
bool selinv_plan(const CholHostPlan& hp, SelinvHostPlan* sp, int* bad_i = nullptr, int* bad_k = nullptr);   // (hp: what chol_tasks left)

}  // namespace rsba
