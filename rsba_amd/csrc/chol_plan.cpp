// Symbolic factorisation and task graph of the tile Cholesky (chol_plan.hpp).  Host only: no HIP header reaches this file.
#include "chol_plan.hpp"

#include <algorithm>

namespace rsba {

int32_t CholHostPlan::slot_of(int i, int k) const {
  if (i == k) return slot_base[k];
  auto it = std::lower_bound(col[k].begin(), col[k].end(), i);
  return (it != col[k].end() && *it == i) ? slot_base[k] + 1 + (int32_t)(it - col[k].begin()) : -1;
}

void chol_symbolic(int nt, const std::vector<std::vector<int32_t>>& adj, const TileOrder& order, CholHostPlan* hp) {
  hp->nt = nt;
  hp->perm = order.perm;
  const std::vector<int32_t>& perm = hp->perm;
  std::vector<int32_t>& iperm = hp->iperm;
  iperm.resize(nt);
  for (int k = 0; k < nt; ++k) iperm[perm[k]] = k;
  // symbolic factorisation in the new order: col[k] = rows i > k of column k (after fill), row[j] = columns k < j of row j
  std::vector<std::vector<int32_t>>&col = hp->col, &row = hp->row;
  col.assign(nt, {}); row.assign(nt, {});
  {
    std::vector<std::vector<uint8_t>> mark(nt);
    for (int k = 0; k < nt; ++k) mark[k].assign(nt - k, 0);       // mark[k][i-k] for i >= k
    for (int t = 0; t < nt; ++t) for (int u : adj[t]) { const int i = std::max(iperm[t], iperm[u]), k = std::min(iperm[t], iperm[u]); mark[k][i - k] = 1; }
    for (int k = 0; k < nt; ++k) {
      for (int i = k + 1; i < nt; ++i) if (mark[k][i - k]) col[k].push_back(i);
      for (size_t u = 0; u < col[k].size(); ++u) for (size_t v = u; v < col[k].size(); ++v) mark[col[k][u]][col[k][v] - col[k][u]] = 1;
      for (int32_t i : col[k]) row[i].push_back(k);
    }
  }
  // packed tile slots, column by column: (k,k) first, then the sub-diagonal tiles of column k
  hp->slot_base.assign(nt + 1, 0);
  for (int k = 0; k < nt; ++k) hp->slot_base[k + 1] = hp->slot_base[k] + 1 + (int32_t)col[k].size();
  hp->nslots = hp->slot_base[nt];
  hp->slot_tiles.resize(2 * (size_t)hp->nslots);
  for (int k = 0; k < nt; ++k) {
    int32_t* st = hp->slot_tiles.data() + 2 * (size_t)hp->slot_base[k];
    st[0] = perm[k]; st[1] = perm[k];
    for (size_t u = 0; u < col[k].size(); ++u) { st[2 * (u + 1)] = perm[col[k][u]]; st[2 * (u + 1) + 1] = perm[k]; }
  }
}

void chol_tasks(const CholTaskInput& in, CholHostPlan* hp) {
  CholHostPlan& s = *hp;
  const int nt = s.nt, kChunk = in.opt.chunk, kTail = in.opt.tail;
  const bool sharded = in.sharded, two_rhs = in.two_rhs;
  const std::vector<int32_t>&perm = s.perm, &slot_base = s.slot_base, &part_of = in.order->part_of;
  const std::vector<std::vector<int32_t>>&col = s.col, &row = s.row;
  auto slot_of = [&](int i, int k) { return s.slot_of(i, k); };
  s.sharded = sharded; s.two_rhs = two_rhs;
  // part of a column = the rank whose subtree it belongs to, -1 = a separator the ranks share
  std::vector<int32_t>& cpart = s.cpart;
  cpart.assign(nt, -1);
  if (sharded) for (int j = 0; j < nt; ++j) cpart[j] = part_of[perm[j]];
  // level schedule: column j is ready once every column of row[j] is done
  std::vector<int32_t>& level = s.level;
  level.assign(nt, 0);
  int nlev = 0;
  for (int j = 0; j < nt; ++j) { int l = 0; for (int32_t k : row[j]) l = std::max(l, level[k] + 1); level[j] = l; nlev = std::max(nlev, l + 1); }
  s.nlev = nlev;
  std::vector<std::vector<int32_t>> lev_cols(nlev);
  for (int j = 0; j < nt; ++j) lev_cols[level[j]].push_back(j);
  // flattened work lists
  //   diag item d: column j -> {slot_jj, old tile of j}, contributors k in row[j]: {slot_jk, old tile of k}
  //   sub  item t: tile (i,j) -> {slot_ij, slot_jj}, contributors k in row[j] & row[i]: {slot_ik, slot_jk}
  //   back item  : column j -> {slot_jj, old tile of j}, tiles i in col[j]: {slot_ij, old tile of i}
  // A tile with many contributors (separator rows are dense across their segments) would serialise dozens
  // of 48^3 products in one workgroup; its contributor list is cut into chunks of kChunk that separate
  // workgroups reduce to partial tiles (fixed split, fixed order: still deterministic), summed by the
  // factor kernels.  upd items: {kind 0 diag / 1 sub, list begin, list end, scratch slot}.
  // The owner of a tile keeps the last kTail contributors — the ones from the latest levels, the list being sorted by
  // level — for itself: on the critical path a freshly finished tile is then multiplied by its consumer directly
  // instead of passing through a partial tile in HBM (two memory round trips less per level).
  // An UPDATE task becomes runnable one level after its last contributor, which is where it enters the ticket order.
  // Look-ahead on the critical path: the LAST contributor k* of column j finishes one level before j and would reach the
  // DIAG task through the SUB task of tile (j, k*) — W_k* out, L_jk* = X W_k*^T back, two hand-offs through memory.  The DIAG
  // task takes X = S_jk* - (older updates) — which the SUB task publishes as soon as it has it, long before W_k* exists — and
  // multiplies by W_k* itself the moment it lands (one hand-off).  The SUB task still writes L_jk* for everyone else; both
  // follow the same arithmetic, bit for bit.
  std::vector<int32_t> sub_base(nt, 0);   // first SUB item of each column (items of a column follow col[] order)
  s.lev_diag_ptr.assign(1, 0); s.lev_sub_ptr.assign(1, 0); s.lev_upd_ptr.assign(1, 0);
  s.diag_ptr.assign(1, 0); s.sub_ptr.assign(1, 0); s.back_ptr.assign(1, 0);
  int parts = 0;
  std::vector<std::vector<int32_t>> upd_by_level(nlev);
  std::vector<int32_t> klev;   // level of each contributor of the list being built
  std::vector<int32_t>& upd_owner = s.upd_owner;
  std::vector<int32_t> diag_colnew, sub_colnew; int cur_part = -1;   // column (new order) of each DIAG / SUB item
  std::vector<std::vector<int32_t>> asm_of_slot(sharded ? (size_t)s.nslots : 0);   // per separator tile of a sharded plan: {part, partial tile} of the parts' UPDATE items that subtract from it
  for (int l = 0; l < nlev; ++l) {
    // contributors [p0, p1) of the list being built (levels in klev, klev[0] belonging to list position lbase); the first nb of them
    // — sharded plans, separator items only — are the columns of the ranks' parts, grouped by part (pk = their parts): each part's
    // share is cut into UPDATE items that ITS rank runs, whatever their number; {part0, nparts} covers every partial tile of the item
    // — what the replicated factorisation subtracts —, info_sh the ones of the separators' own columns only — what is left to
    // subtract after the exchange has summed the rest in (assemble_top)
    auto chunk_it = [&](int kind, int32_t p0, int32_t p1, std::vector<int32_t>& info, std::vector<int32_t>& own, int32_t lbase, int nb, const std::vector<int32_t>& pk,
                        std::vector<int32_t>* info_sh, int32_t tile_slot) {
      const int32_t first_part = parts;
      int cnt = 0;
      for (int32_t q = p0; q < p0 + nb;) {   // the parts' shares
        int32_t qe = q; while (qe < p0 + nb && pk[qe - p0] == pk[q - p0]) ++qe;
        for (int32_t c = q; c < qe; c += kChunk) {
          const int32_t c1 = std::min(c + kChunk, qe);
          upd_by_level[klev[c1 - 1 - lbase] + 1].push_back((int32_t)(s.upd.size() / 4));
          upd_owner.push_back(pk[q - p0]); asm_of_slot[tile_slot].push_back(pk[q - p0]); asm_of_slot[tile_slot].push_back(parts);
          s.upd.push_back(kind); s.upd.push_back(c); s.upd.push_back(c1); s.upd.push_back(parts++); ++cnt;
        }
        q = qe;
      }
      const int nbparts = cnt;
      p0 += nb;
      if (p1 - p0 <= kChunk) own.push_back(p0);
      else {
        const int32_t own0 = p1 - kTail;
        for (int32_t q = p0; q < own0; q += kChunk) {
          const int32_t q1 = std::min(q + kChunk, own0);
          upd_by_level[klev[q1 - 1 - lbase] + 1].push_back((int32_t)(s.upd.size() / 4));
          upd_owner.push_back(cur_part);
          s.upd.push_back(kind); s.upd.push_back(q); s.upd.push_back(q1); s.upd.push_back(parts++); ++cnt;
        }
        own.push_back(own0);
      }
      info.push_back(cnt ? first_part : 0); info.push_back(cnt);
      if (info_sh) { info_sh->push_back(cnt - nbparts ? first_part + nbparts : 0); info_sh->push_back(cnt - nbparts); }
    };
    // contributors of a separator item of a sharded plan: the parts' columns first, part by part, then the separators' own — each
    // group in the order its columns finish
    auto split_parts = [&](std::vector<int32_t>& ks, std::vector<int32_t>& pk) {
      std::stable_sort(ks.begin(), ks.end(), [&](int32_t x, int32_t y) { const unsigned px = (unsigned)cpart[x], py = (unsigned)cpart[y]; return px < py; });   // (-1 = separators: last)
      pk.clear();
      for (int32_t k : ks) if (cpart[k] >= 0) pk.push_back(cpart[k]);
      return (int)pk.size();
    };
    for (int32_t j : lev_cols[l]) {
      std::vector<int32_t> rj(row[j]);   // contributors in the order they finish
      std::stable_sort(rj.begin(), rj.end(), [&](int32_t x, int32_t y) { return level[x] < level[y]; });
      const bool topcol = sharded && cpart[j] < 0;
      cur_part = cpart[j];
      std::vector<int32_t> pk;
      const int nbj = topcol ? split_parts(rj, pk) : 0;
      s.diag_info.push_back(slot_base[j]); s.diag_info.push_back(perm[j]);
      if (sharded) { s.diag_info_sh.push_back(slot_base[j]); s.diag_info_sh.push_back(perm[j]); }
      diag_colnew.push_back(j);
      const int32_t dp0 = (int32_t)(s.diag_list.size() / 2);
      klev.clear();
      for (int32_t k : rj) { s.diag_list.push_back(slot_of(j, k)); s.diag_list.push_back(perm[k]); klev.push_back(level[k]); }
      s.diag_ptr.push_back((int32_t)(s.diag_list.size() / 2));
      {
        // the contributors a second right-hand side's forward task sums over (FWD2 / FWD2P, chol_tasks.hpp): all of them; in a sharded plan a
        // separator column takes THIS rank's part in launch A (its share travels) and the separators' own columns in launch B
        const int32_t dp1 = (int32_t)(s.diag_list.size() / 2);
        s.fwd_full.push_back(dp0); s.fwd_full.push_back(dp1);
        if (sharded) {
          int32_t lo = dp0, hi = dp0;
          if (topcol) { int q = 0; while (q < nbj && pk[q] != in.rank) ++q; lo = dp0 + q; while (q < nbj && pk[q] == in.rank) ++q; hi = dp0 + q; }
          else { lo = dp0; hi = dp1; }
          s.fwd_a.push_back(lo); s.fwd_a.push_back(hi);
          s.fwd_b.push_back(topcol ? dp0 + nbj : dp0); s.fwd_b.push_back(topcol ? dp1 : dp0);
        }
      }
      chunk_it(0, dp0, (int32_t)(s.diag_list.size() / 2), s.diag_info, s.diag_own, dp0, nbj, pk, sharded ? &s.diag_info_sh : nullptr, slot_base[j]);
      if (in.opt.fuse_last && !rj.empty() && (!topcol || cpart[rj.back()] < 0)) {   // (a separator column of a sharded plan never takes a part's column by the hand: it lives on another rank)
        const int32_t ks = rj.back();
        const int32_t fs = sub_base[ks] + (int32_t)(std::lower_bound(col[ks].begin(), col[ks].end(), j) - col[ks].begin());
        s.diag_fuse.push_back(fs);
        s.sub_pub[fs] = (int32_t)(s.diag_info.size() / 4) - 1;
      } else s.diag_fuse.push_back(-1);
      sub_base[j] = (int32_t)(s.sub_info.size() / 4);
      s.back_info.push_back(slot_base[j]); s.back_info.push_back(perm[j]);
      for (auto it = col[j].rbegin(); it != col[j].rend(); ++it) { s.back_list.push_back(slot_of(*it, j)); s.back_list.push_back(perm[*it]); }   // bottom-up: the order the y_i arrive in
      s.back_ptr.push_back((int32_t)(s.back_list.size() / 2));
      for (int32_t i : col[j]) {
        s.sub_info.push_back(slot_of(i, j)); s.sub_info.push_back(slot_base[j]); s.sub_col.push_back(perm[j]); s.sub_pub.push_back(-1);
        if (sharded) { s.sub_info_sh.push_back(slot_of(i, j)); s.sub_info_sh.push_back(slot_base[j]); }
        sub_colnew.push_back(j);
        const int32_t sp0 = (int32_t)(s.sub_list.size() / 2);
        // k in row[j] with tile (i,k) present (rj: for a separator column of a sharded plan the parts' columns first, part by part)
        klev.clear(); pk.clear();
        for (int32_t k : rj) { const int32_t sik = slot_of(i, k); if (sik >= 0) { s.sub_list.push_back(sik); s.sub_list.push_back(slot_of(j, k)); klev.push_back(level[k]); if (topcol && cpart[k] >= 0) pk.push_back(cpart[k]); } }
        s.sub_ptr.push_back((int32_t)(s.sub_list.size() / 2));
        chunk_it(1, sp0, (int32_t)(s.sub_list.size() / 2), s.sub_info, s.sub_own, sp0, (int)pk.size(), pk, sharded ? &s.sub_info_sh : nullptr, slot_of(i, j));
      }
    }
    s.lev_diag_ptr.push_back((int32_t)(s.diag_info.size() / 4));
    s.lev_sub_ptr.push_back((int32_t)(s.sub_info.size() / 4));
    s.lev_upd_ptr.push_back((int32_t)(s.upd.size() / 4));
  }
  s.nparts = parts;
  // A free interFrameRatio brings a second right-hand side (its column of the normal equations): z2 = L^-1 b is formed by FWD2 tasks
  // right behind the DIAG tasks of their columns — light tasks for workgroups the factorisation leaves idle — and ONE ETA task between
  // the forward and the backward phase turns both forward solves into the ratio's step (solver_state.hpp; chol_tasks.hpp: task_eta)
  auto push = [](std::vector<int32_t>& t, int kind, int item) { t.push_back(kind); t.push_back(item); };
  for (int l = 0; l < nlev; ++l) {
    for (int32_t u : upd_by_level[l]) push(s.tasks, kTaskUpdate, u);
    for (int d = s.lev_diag_ptr[l]; d < s.lev_diag_ptr[l + 1]; ++d) push(s.tasks, kTaskDiag, d);
    if (two_rhs) for (int d = s.lev_diag_ptr[l]; d < s.lev_diag_ptr[l + 1]; ++d) push(s.tasks, kTaskFwd2, d);
    for (int t = s.lev_sub_ptr[l]; t < s.lev_sub_ptr[l + 1]; ++t) push(s.tasks, kTaskSub, t);
  }
  if (two_rhs) push(s.tasks, kTaskEta, 0);
  for (int l = nlev - 1; l >= 0; --l)
    for (int d = s.lev_diag_ptr[l]; d < s.lev_diag_ptr[l + 1]; ++d) push(s.tasks, kTaskBack, d);
  // second right-hand side: per DIAG item the index of its column among the separators' tile columns (ascending new order: the order of top_tiles below)
  s.diag_toprow.assign(diag_colnew.size(), -1);
  // tile factorisation: per DIAG item its contributors (lower half of L L^T: T^3 each) + potrf and inverse (T^3 / 3 each);
  // per SUB item 2 T^3 per contributor + the product with W (T^3); forward / backward solve 2 T^2 per factor tile, twice
  const int64_t T3 = (int64_t)kTile * kTile * kTile;
  s.cholesky_flops = T3 * ((int64_t)(s.diag_list.size() / 2) + 2 * (int64_t)(s.sub_list.size() / 2) + (int64_t)(s.sub_info.size() / 4)) +
                     2 * T3 / 3 * (int64_t)(s.diag_info.size() / 4) + 4 * (int64_t)kTile * kTile * ((int64_t)s.nslots + nt);
  s.row_mine.assign((size_t)nt, 1);
  if (!sharded) return;

  // launch A: this rank's part, forward (the parts' UPDATE items of the separators' tiles included); launch B: the separators,
  // forward and backward, then this rank's part backward
  const int me = in.rank;
  auto mine_or_top = [&](int col_new, int kind, int item) { const int p = cpart[col_new]; if (p == me) push(s.tasks_a, kind, item); else if (p < 0) push(s.tasks_b, kind, item); };
  for (int l = 0; l < nlev; ++l) {
    for (int32_t u : upd_by_level[l]) { if (upd_owner[u] == me) push(s.tasks_a, kTaskUpdate, u); else if (upd_owner[u] < 0) push(s.tasks_b, kTaskUpdate, u); }
    for (int d = s.lev_diag_ptr[l]; d < s.lev_diag_ptr[l + 1]; ++d) mine_or_top(diag_colnew[d], kTaskDiag, d);
    if (two_rhs) for (int d = s.lev_diag_ptr[l]; d < s.lev_diag_ptr[l + 1]; ++d) mine_or_top(diag_colnew[d], kTaskFwd2, d);
    for (int t = s.lev_sub_ptr[l]; t < s.lev_sub_ptr[l + 1]; ++t) mine_or_top(sub_colnew[t], kTaskSub, t);
  }
  if (two_rhs) {
    // launch A ends with what travels: this rank's part's share of every separator column's second right-hand side, and of the two dots;
    // launch B's ETA task sits between its forward and its backward phase
    for (int d = 0; d < (int)diag_colnew.size(); ++d) if (cpart[diag_colnew[d]] < 0) push(s.tasks_a, kTaskFwd2P, d);
    push(s.tasks_a, kTaskEta, 0);
    push(s.tasks_b, kTaskEta, 0);
  }
  for (int l = nlev - 1; l >= 0; --l)
    for (int d = s.lev_diag_ptr[l]; d < s.lev_diag_ptr[l + 1]; ++d) { const int p = cpart[diag_colnew[d]]; if (p == me || p < 0) push(s.tasks_b, kTaskBack, d); }
  {
    std::vector<int32_t> trow_of_col((size_t)nt, -1);
    int32_t cnt = 0;
    for (int j = 0; j < nt; ++j) if (cpart[j] < 0) trow_of_col[j] = cnt++;
    for (size_t d = 0; d < diag_colnew.size(); ++d) s.diag_toprow[d] = trow_of_col[diag_colnew[d]];
  }
  // ---- what the exchange between the two launches needs ----
  std::vector<uint8_t> has_pair((size_t)s.nslots, 0);
  for (size_t t = 0; t < in.pair_I->size(); ++t) { const int a = s.iperm[(*in.pair_I)[t]], b = s.iperm[(*in.pair_J)[t]]; has_pair[slot_of(std::max(a, b), std::min(a, b))] = 1; }
  // the separators' tiles, column by column: {slot, has a tile pair (else: fill only, zero in S), index among the separator tiles of its row of the rhs or -1}
  s.asm_ptr.assign(1, 0);
  for (int j = 0; j < nt; ++j) if (cpart[j] < 0) {
    const int trow = (int)s.top_tiles.size();
    s.top_tiles.push_back(perm[j]);
    auto add = [&](int32_t slot, int rhs_row) {
      s.top_slots.push_back(slot); s.top_info.push_back(has_pair[slot]); s.top_info.push_back(rhs_row);
      const std::vector<int32_t>& a = asm_of_slot[slot];
      for (size_t q = 0; q + 1 < a.size(); q += 2) if (a[q] == me) s.asm_list.push_back(a[q + 1]);   // this rank's partial tiles, in list order
      s.asm_ptr.push_back((int32_t)s.asm_list.size());
      if (!has_pair[slot]) s.top_fill.push_back(slot);
    };
    add(slot_base[j], trow);
    for (size_t u = 0; u < col[j].size(); ++u) add(slot_base[j] + 1 + (int32_t)u, -1);   // (rows below a separator column are separators too: fill only reaches ancestors)
  }
  // rows of y this rank contributes to the gather (and whose residual it can check: every tile of those rows is complete here):
  // its own part; the separators' rows come from rank 0
  s.row_check.assign((size_t)nt, 0); s.row_sep.assign((size_t)nt, 0);
  for (int t = 0; t < nt; ++t) { const int p = part_of[t]; s.row_mine[t] = p == me || (p < 0 && me == 0); s.row_check[t] = p == me; s.row_sep[t] = p < 0; }
  // the two dependency chains: elimination levels inside this rank's part, and levels that hold a separator column
  int lmax = -1; std::vector<uint8_t> sep_level((size_t)nlev, 0);
  for (int j = 0; j < nt; ++j) { if (cpart[j] == me) lmax = std::max(lmax, level[j]); else if (cpart[j] < 0) sep_level[level[j]] = 1; }
  s.local_levels = lmax + 1; s.separator_levels = 0;
  for (uint8_t b : sep_level) s.separator_levels += b;
}

bool selinv_plan(const CholHostPlan& hp, SelinvHostPlan* sp, int* bad_i, int* bad_k) {
  SelinvHostPlan& p = *sp;
  p = SelinvHostPlan{};
  const int nt = hp.nt, nlev = hp.nlev;
  p.nlev = nlev;
  std::vector<std::vector<int32_t>> lev_cols((size_t)nlev);
  for (int j = 0; j < nt; ++j) lev_cols[hp.level[j]].push_back(j);
  p.lev_g_ptr.assign(1, 0); p.lev_off_ptr.assign(1, 0); p.lev_diag_ptr.assign(1, 0);
  p.off_ptr.assign(1, 0); p.diag_ptr.assign(1, 0);
  for (int l = nlev - 1; l >= 0; --l) {
    for (int32_t j : lev_cols[l]) {
      const std::vector<int32_t>& J = hp.col[j];
      const int32_t tile_j = hp.perm[j];
      for (size_t u = 0; u < J.size(); ++u) { p.g_info.push_back(hp.slot_base[j] + 1 + (int32_t)u); p.g_info.push_back(tile_j); }
      for (size_t a = 0; a < J.size(); ++a) {
        const int32_t i = J[a];
        p.off_info.push_back(hp.slot_base[j] + 1 + (int32_t)a); p.off_info.push_back(tile_j);
        for (size_t u = 0; u < J.size(); ++u) {
          const int32_t k = J[u];
          const int32_t s = i >= k ? hp.slot_of(i, k) : hp.slot_of(k, i);
          if (s < 0) { if (bad_i) *bad_i = i; if (bad_k) *bad_k = k; return false; }
          p.off_list.push_back(s); p.off_list.push_back(i < k ? 1 : 0); p.off_list.push_back(hp.slot_base[j] + 1 + (int32_t)u);
        }
        p.off_ptr.push_back((int32_t)(p.off_list.size() / 3));
      }
      p.diag_info.push_back(hp.slot_base[j]); p.diag_info.push_back(tile_j);
      for (size_t u = 0; u < J.size(); ++u) p.diag_list.push_back(hp.slot_base[j] + 1 + (int32_t)u);
      p.diag_ptr.push_back((int32_t)p.diag_list.size());
    }
    p.lev_g_ptr.push_back((int32_t)(p.g_info.size() / 2));
    p.lev_off_ptr.push_back((int32_t)(p.off_info.size() / 2));
    p.lev_diag_ptr.push_back((int32_t)(p.diag_info.size() / 2));
  }
  const int64_t T3 = (int64_t)kTile * kTile * kTile;
  p.flops = 2 * T3 * ((int64_t)(p.g_info.size() / 2) + (int64_t)(p.off_list.size() / 3) + (int64_t)(p.diag_info.size() / 2) + (int64_t)p.diag_list.size());
  return true;
}

}  // namespace rsba
