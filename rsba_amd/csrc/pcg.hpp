// Iterative solve of the reduced camera system: block-Jacobi preconditioned conjugate gradients over the packed tiles of S
// (kernels_pcg.hip; the rule is stated in include/rsba_amd.h at rsba_set_linear_solver).  The host side of the plan — which tiles
// a row tile gathers, in which order, and where the blocks of the preconditioner sit — is pcg_plan.cpp.
#pragma once
#include <cstdint>
#include <vector>

namespace rsba {

constexpr int kPcgBlockMax = 12;   // widest block of the preconditioner: a two-pose frame (9 for an intrinsics block, 6 for a one-pose frame, 1 for a padding row)

// Work lists of one problem, host side.  Nothing here depends on the order of the packed slots except the slot numbers themselves:
// a row tile's list is sorted by column tile, the blocks are numbered by their first row.
struct PcgHostPlan {
  std::vector<int32_t> row_ptr;    // [nt + 1] into row_list
  std::vector<int32_t> row_list;   // [.][2] {packed slot, column tile << 1 | read transposed}, ascending column tile
  std::vector<int32_t> blk_row;    // [nblk] first row of the block
  std::vector<int32_t> blk_size;   // [nblk] 1 .. kPcgBlockMax
  std::vector<int32_t> blk_slots;  // [nblk][3] packed slot of the diagonal tile of the block's first row | of its last row | of the tile between the two
                                   //   (second and third -1: the block lies in one tile; third: << 1 | stored as (first row's tile, last row's tile))
};
// slot_tiles [nslots][2] {row tile, column tile}; F frames of CD unknowns, then NIB intrinsics blocks of 9 unknowns at the front of NPF pseudo frames each
// returns false when a diagonal tile has no slot (cannot happen for a plan of this library)
bool pcg_build_plan(const std::vector<int32_t>& slot_tiles, int nt, int F, int CD, int NIB, int NPF, PcgHostPlan* out);

#ifdef __HIPCC__
struct SolverDev;
// device state of the iteration
struct PcgDev {
  const int32_t *row_ptr, *row_list, *blk_row, *blk_size, *blk_slots;
  int nblk, nbw;          // blocks, workgroups of the per-block kernels (kPcgBlockThreads blocks each)
  double* fac;            // [kPcgBlockMax * (kPcgBlockMax + 1) / 2][nblk] Cholesky factors of the blocks, lower, row-major packed, diagonal inverted; block index fastest
  double *y, *r, *z, *q;  // [npad]
  double* p[2];           // [npad] the search direction of the last and of this iteration (the product kernel forms p = z + beta p_old as it reads)
  double* part_pq;        // [nt] partial sums p.q of the product kernel
  double* part;           // [3][nbw] partial sums r.z | r.r | y.(rhs + r) of the update kernel
  double* sc;             // [kPcgScSize] scalars of the iteration (PcgSlot)
};
enum PcgSlot : int {
  kPcgDone = 0,      // != 0: the solve is over — 1 a stopping test held, 2 the cap, 3 failed; every kernel looks here first
  kPcgK = 1,         // iterations done
  kPcgRz = 2, kPcgBeta = 3, kPcgQ = 4, kPcgB2 = 5,   // r.z, beta of the next direction, Q_k, |rhs|^2
  kPcgRel = 6,       // |r_k| / |rhs|
  kPcgZeta = 7,      // k (Q_k - Q_k-1) / Q_k of the last iteration
  kPcgScSize = 8
};
struct PcgRule { int32_t min_iterations, max_iterations; double eta, r_tolerance; };
constexpr int kPcgBlockThreads = 64;

hipError_t launch_pcg_begin(const SolverDev& sv, const PcgDev& pc, hipStream_t st);   // factors of the blocks of M; y = 0, r = rhs, z = M^-1 r, the first scalars
hipError_t launch_pcg_iteration(const SolverDev& sv, const PcgDev& pc, const PcgRule& rule, int flip, hipStream_t st);   // flip: p[flip] is read, p[flip ^ 1] written
#endif

}  // namespace rsba
