// Host side of the iterative reduced solve (pcg.hpp): the gather list of every row tile and the blocks of the preconditioner.
#include "pcg.hpp"

#include <algorithm>
#include <array>

namespace rsba {

namespace {
constexpr int kT = 48;   // the tile of the reduced camera system (tile_order.hpp: kTile)
}

bool pcg_build_plan(const std::vector<int32_t>& slot_tiles, int nt, int F, int CD, int NIB, int NPF, PcgHostPlan* out) {
  const int nslots = (int)(slot_tiles.size() / 2);
  // row tile -> {column tile, slot, transposed}: tile (i, j) serves row tile i as it is stored and row tile j transposed
  std::vector<std::vector<std::array<int32_t, 3>>> rows((size_t)nt);
  std::vector<int32_t> diag_slot((size_t)nt, -1);
  for (int s = 0; s < nslots; ++s) {
    const int i = slot_tiles[2 * (size_t)s], j = slot_tiles[2 * (size_t)s + 1];
    if (i < 0 || j < 0 || i >= nt || j >= nt) return false;
    if (i == j) { diag_slot[(size_t)i] = s; rows[(size_t)i].push_back({j, s, 0}); continue; }
    rows[(size_t)i].push_back({j, s, 0});
    rows[(size_t)j].push_back({i, s, 1});
  }
  out->row_ptr.assign((size_t)nt + 1, 0);
  out->row_list.clear();
  for (int i = 0; i < nt; ++i) {
    if (diag_slot[(size_t)i] < 0) return false;
    std::sort(rows[(size_t)i].begin(), rows[(size_t)i].end());
    for (const auto& e : rows[(size_t)i]) { out->row_list.push_back(e[1]); out->row_list.push_back(e[0] * 2 + e[2]); }
    out->row_ptr[(size_t)i + 1] = (int32_t)(out->row_list.size() / 2);
  }
  // blocks: frames, then per intrinsics block its 9 coordinates and the padding behind them one row each, then the padding of the last tile
  const int npad = nt * kT;
  out->blk_row.clear(); out->blk_size.clear();
  auto add = [&](int row, int size) { out->blk_row.push_back(row); out->blk_size.push_back(size); };
  for (int f = 0; f < F; ++f) add(f * CD, CD);
  int row = F * CD;
  for (int c = 0; c < NIB; ++c) {
    add(row, 9);
    for (int k = 9; k < NPF * CD; ++k) add(row + k, 1);
    row += NPF * CD;
  }
  for (; row < npad; ++row) add(row, 1);
  const size_t nblk = out->blk_row.size();
  out->blk_slots.assign(3 * nblk, -1);
  for (size_t b = 0; b < nblk; ++b) {
    const int t0 = out->blk_row[b] / kT, t1 = (out->blk_row[b] + out->blk_size[b] - 1) / kT;
    if (t1 >= nt || t1 > t0 + 1) return false;
    out->blk_slots[3 * b] = diag_slot[(size_t)t0];
    if (t1 == t0) continue;
    out->blk_slots[3 * b + 1] = diag_slot[(size_t)t1];
    for (int s = 0; s < nslots; ++s) {
      const int i = slot_tiles[2 * (size_t)s], j = slot_tiles[2 * (size_t)s + 1];
      if (i == t1 && j == t0) out->blk_slots[3 * b + 2] = 2 * s;
      else if (i == t0 && j == t1) out->blk_slots[3 * b + 2] = 2 * s + 1;
    }
  }
  return true;
}

}  // namespace rsba
