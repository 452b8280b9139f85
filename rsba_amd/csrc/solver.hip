// Host side of rsba_solve: the steps of an iteration and the trust-region loop (the symbolic phase is solver_plan.hip, the covariance
// entry points are solver_cov.hip; what the three share is solver.hpp).
//
// The loop is a rule-for-rule restatement of Ceres-Solver 1.9's TrustRegionMinimizer +
// LevenbergMarquardtStrategy with an exact Schur-complement linear solve — what
// ceres::Solve(SPARSE_SCHUR) runs for CeresHandler.h:394-426 (SURVEY
// Appendix C.5).  Every array lives on the device; per iteration the host reads back a few scalars
// (costs, model decrease, step / parameter norms, gradient max-norm, failure flags) and decides.
#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "solver.hpp"
#include "test_hooks.hpp"

using namespace rsba;

namespace rsba {

int32_t reset_scales(rsba_handle* h) {
  const DeviceProblem& dp = h->dp;
  RSBA_HIP_TRY(hipMemcpyAsync(dp.scale_pose, h->d_mask_pose, h->mask_pose.size() * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  RSBA_HIP_TRY(hipMemcpyAsync(dp.scale_point, h->d_mask_point, h->mask_point.size() * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  RSBA_HIP_TRY(hipMemcpyAsync(dp.scale_intr, h->d_mask_intr, h->mask_intr.size() * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (dp.pp_count > 0) {   // the priorPoses blocks are always free: scale 1
    static const std::vector<double> ones(1 << 16, 1.0);
    for (size_t o = 0; o < 6 * (size_t)dp.pp_count; o += ones.size())
      RSBA_HIP_TRY(hipMemcpyAsync(dp.pp_scale + o, ones.data(), std::min(ones.size(), 6 * (size_t)dp.pp_count - o) * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  return RSBA_OK;
}

// all-reduce across the ranks of a point-partitioned solve (no-op for a single GPU); kind: RSBA_EXCHANGE_* (statistics)
int32_t exchange(rsba_handle* h, double* buf, int64_t count, int op, int kind) {
  if (!h->allreduce) return RSBA_OK;   // (a one-rank exchange still goes through its transport: identity, but the path is exercised)
  (void)rsba_set_error(RSBA_OK, "");   // a transport that fails says why through rsba_set_error (the RCCL one: the ncclResult string); keep what it said
  ++h->x_calls[kind]; h->x_doubles[kind] += count;
  PhaseTimer* xt = h->solver && h->solver->xtimer.on ? &h->solver->xtimer : nullptr;
  hipEvent_t a = nullptr;
  if (xt) { a = xt->get(); (void)hipEventRecord(a, h->stream); }
  const int failed = h->allreduce(h->allreduce_ctx, buf, count, op, h->stream);
  if (xt) { hipEvent_t b = xt->get(); (void)hipEventRecord(b, h->stream); xt->pending.push_back({kind, a, b}); }
  if (failed != 0) {
    const std::string why = rsba_last_error();
    char where[112];
    std::snprintf(where, sizeof where, " (all-reduce %s of %lld doubles, op %d, rank %d of %d)", rsba_exchange_name(kind), (long long)count, op, h->rank, h->world);
    return rsba_set_error(RSBA_ERR_COMM, ((why.empty() ? std::string("the all-reduce callback reported a failure") : why) + where).c_str());
  }
  return RSBA_OK;
}

// The ratio's column of the normal equations (and its own h, g) is formed by EVERY rank over ALL priors, from replicated poses — also where
// a sharded plan has shared the priors' blocks out (h->prior_split: dp.prior_of then lists this rank's share).
DeviceProblem all_priors(const rsba_handle* h) {
  DeviceProblem d = h->dp;
  if (h->prior_split) d.prior_of = h->prior_of_all;
  return d;
}

// r, J (loss-corrected, masked, scaled) and the normal-equation blocks at the current parameters;
// exchange (1): per-camera gradient blocks + diag(U) + cost scalars.  Results: sv.gc / sv.udiag global,
// scalars[kCost, kFixedCost, kEvalFailed].
// have_eval: the LM-mode evaluation at these parameters (per-wave camera blocks, cost incl. the prior blocks' in d_cost2) has just
// been run — the trust-region loop evaluates its candidates that way when nothing would be lost by it (see rsba_solve).
// exchange (1) of a linearisation on several ranks: the camera gradient, diag(U) and the cost scalars, summed over the ranks — with
// ride, every rank's gradient maximum over its points behind the payload and the cameras' maximum taken from the summed gradient
static int32_t exchange_camera_gradient(rsba_handle* h, bool ride) {
  Solver* s = h->solver;
  RSBA_HIP_TRY(launch_pack_linearize(h->dp, s->sv, h->d_cost2, h->stream, ride ? h->world : 0));
  if (ride) RSBA_HIP_TRY(launch_gradient_max_points(h->dp, s->sv, h->rank, h->stream));
  if (int32_t rc = exchange(h, s->sv.xbuf, 2 * s->sv.n + 3 + (ride ? h->world : 0), 0, RSBA_EXCHANGE_CAMERA)) return rc;
  RSBA_HIP_TRY(launch_unpack_linearize(h->dp, s->sv, h->stream));
  if (ride) RSBA_HIP_TRY(launch_gradient_max_cameras(h->dp, s->sv, h->world, h->stream));
  return RSBA_OK;
}

int32_t linearize(rsba_handle* h, bool have_eval, bool want_gradmax) {
  Solver* s = h->solver;
  if (!have_eval) {
    PhaseScope ps(h, RSBA_PHASE_EVAL_LM);
    RSBA_HIP_TRY(launch_eval(h->dp, kLmJacobian, h->stream));   // (the cost reduction overwrites dp.fail_count: nothing to clear)
    RSBA_HIP_TRY(launch_cost_reduce(h->dp, h->d_cost2, h->stream));
  }
  {
    PhaseScope ps(h, RSBA_PHASE_CAMERA_BLOCKS);
    RSBA_HIP_TRY(launch_camera_blocks(h->dp, s->sv, h->stream));
    RSBA_HIP_TRY(launch_intr_blocks(h->dp, s->sv, h->stream));
  }
  const bool my_priors = owns_motion_priors(h);
  if (my_priors || s->border) {
    PhaseScope ps(h, RSBA_PHASE_PRIORS);
    if (my_priors) {
      if (!have_eval) RSBA_HIP_TRY(launch_prior_cost(h->dp, h->d_cost2, h->prior_invalid, h->stream));
      RSBA_HIP_TRY(launch_prior_blocks(h->dp, s->sv, s->ucross, h->stream));
    }
    if (s->border) RSBA_HIP_TRY(launch_prior_border(all_priors(h), s->sv, s->border, s->ratio4, h->stream));   // every rank: from replicated poses
  }
  if (h->dp.pp_count > 0 || h->dp.pp_spherical >= 0) {   // per-pose priors: replicated terms, contributed by the lead rank;
    PhaseScope ps(h, RSBA_PHASE_PRIORS);                   // the linearisation of the priorPoses coordinates (v0, g0, cross) on every rank: each one steps them itself
    if (s->sv.lead && !have_eval) RSBA_HIP_TRY(launch_pose_prior_cost(h->dp, h->d_cost2, h->stream));
    RSBA_HIP_TRY(launch_pose_prior_blocks(h->dp, s->sv, s->pp, h->stream));
  }
  {
    PhaseScope ps(h, RSBA_PHASE_POINT_BLOCKS);
    RSBA_HIP_TRY(launch_point_blocks(h->dp, s->sv, h->stream));
  }
  PhaseScope ps(h, RSBA_PHASE_EXCHANGE);
  s->gradmax_done = false;
  if (!h->allreduce) { RSBA_HIP_TRY(launch_local_linearize(h->dp, s->sv, h->d_cost2, h->stream)); return RSBA_OK; }   // one rank: nothing to sum
  // max |g_i| (the gradient test that follows an accepted step) rides in this exchange instead of taking a MAX all-reduce of its own —
  // every collective is tens of microseconds of latency on a node: each rank's maximum over ITS points (they are nobody else's) in a
  // slot of its own behind the payload, the other ranks' slots zero, so the SUM delivers all of them; the cameras' maximum is taken
  // from the summed gradient behind the exchange.  (Not with per-pose priors: their blocks' maximum is the lead rank's alone.)
  const bool ride = want_gradmax && h->world <= kMaxRankSlots && h->dp.pp_count == 0;   // (a SphericalPrior has no coordinates of its own: its gradient is part of the summed camera gradient)
  if (int32_t rc = exchange_camera_gradient(h, ride)) return rc;
  s->gradmax_done = ride;
  return RSBA_OK;
}

int32_t gradient_max(rsba_handle* h) {
  Solver* s = h->solver;
  if (s->gradmax_done) { s->gradmax_done = false; return RSBA_OK; }   // (came with the camera exchange of the linearisation just before)
  PhaseScope ps(h, RSBA_PHASE_OTHER);
  RSBA_HIP_TRY(launch_gradient_max(h->dp, s->sv, h->stream));
  if (s->sv.lead) RSBA_HIP_TRY(launch_pose_prior_gradmax(h->dp, s->sv, s->pp, h->stream));
  return exchange(h, s->sv.scalars + kGradMax, 1, 1, RSBA_EXCHANGE_SCALARS);
}

// reduced camera system S and rhs at the given trust-region radius (point elimination), summed over the ranks
int32_t reduce_system(rsba_handle* h, double radius) {
  Solver* s = h->solver; const SolverDev& sv = s->sv; hipStream_t st = h->stream;
  { PhaseScope ps(h, RSBA_PHASE_POINT_FACTOR); RSBA_HIP_TRY(launch_point_factor(h->dp, sv, radius, st, s->clamp_with_factor ? s->clamp_lo_hi : nullptr)); }
  {
    PhaseScope ps(h, RSBA_PHASE_PROJECT);
    // A shared intrinsics block at scale (4k cameras: projection 1.03 ms of stores, virtual-record sweep 0.57 ms of fp64): the two passes
    // read the same point factors and write different records — side by side, the sweep on the arming stream (idle here), two events.
    const bool beside = sv.NPF > 0 && sv.nvgroups > 0 && s->mstream && s->ev_fork && h->dp.N >= 2000000 && !s->solve_sw.no_side_sweep && !project_covers_virtual_records(h->dp, sv);   // (round 5: one fused sweep does both where it applies)
    if (beside) {
      RSBA_HIP_TRY(hipEventRecord(s->ev_fork, st));
      RSBA_HIP_TRY(hipStreamWaitEvent(s->mstream, s->ev_fork, 0));
      RSBA_HIP_TRY(launch_virtual_records(h->dp, sv, s->mstream));
      RSBA_HIP_TRY(hipEventRecord(s->ev_join, s->mstream));
    }
    RSBA_HIP_TRY(launch_project(h->dp, sv, st));
    if (beside) RSBA_HIP_TRY(hipStreamWaitEvent(st, s->ev_join, 0));
    else RSBA_HIP_TRY(launch_virtual_records(h->dp, sv, st));
  }
  {
    PhaseScope ps(h, RSBA_PHASE_SCHUR);
    // (S needs no clearing: the merge kernel overwrites every tile a tile pair maps to, and the fill-only tiles — zeroed when the
    // plan was built — are never written by anyone: the factorisation keeps its own tiles, the multi-GPU exchange adds zeros)
    RSBA_HIP_TRY(launch_schur_blocks(h->dp, sv, radius, st));
    ++s->schur_launches;
    if (sv.lead || sv.frame_lead) RSBA_HIP_TRY(launch_pose_prior_reduce(h->dp, sv, s->pp, radius, st));   // the priorPoses blocks leave the system like points (each on the rank that holds its pose's tile)
  }
  // exchange (2): partial reduced camera systems -> the full one on every rank (then factored redundantly) — unless every rank
  // factors its own part: then only the separators travel, between the two launches of the factorisation (solve_reduced_system)
  if (s->hp.sharded && !s->sharded_off && !s->use_levels) return RSBA_OK;
  PhaseScope ps(h, RSBA_PHASE_EXCHANGE);
  if (s->hp.sharded && s->ntop_fill) RSBA_HIP_TRY(launch_zero_tiles(sv.S, s->d_top_fill, s->ntop_fill, st));   // (a sharded solve left its reduced values in the fill-only separator tiles)
  if (h->allreduce && s->exch_slots) {   // only the tiles that can be non-zero travel (the fill-in tiles of the layout are zero on every rank)
    const int64_t count = (int64_t)s->exch_tiles * kTile * kTile + sv.npad;
    RSBA_HIP_TRY(launch_exchange_pack(sv, s->exch_slots, s->exch_tiles, s->exch_buf, false, st));
    if (int32_t rc = exchange(h, s->exch_buf, count, 0, RSBA_EXCHANGE_SYSTEM)) return rc;
    RSBA_HIP_TRY(launch_exchange_pack(sv, s->exch_slots, s->exch_tiles, s->exch_buf, true, st));
    return RSBA_OK;
  }
  return exchange(h, sv.S, (int64_t)sv.nslots * kTile * kTile + sv.npad, 0, RSBA_EXCHANGE_SYSTEM);
}

// S y = rhs: left-looking tile Cholesky (forward solve rides along), then the backward solve: one persistent DAG
// launch, or — the schedule it is checked against — one launch per (level, kind).  S and rhs are left as they are
// (the factor has its own tiles); y lands in sv.yv.
// the solver's stream waits for a verification still running beside it (before its flag is read, and before the cells it reads are re-armed)
int32_t await_verification(rsba_handle* h) {
  Solver* s = h->solver;
  if (s->verify_pending) { RSBA_HIP_TRY(hipStreamWaitEvent(h->stream, s->ev_verified, 0)); s->verify_pending = false; }
  return RSBA_OK;
}
int32_t solve_reduced_system(rsba_handle* h, bool rhs_stays) {
  Solver* s = h->solver; SolverDev& sv = s->sv; hipStream_t st = h->stream;
  PhaseScope ps(h, RSBA_PHASE_CHOLESKY);
  if (int32_t rc = await_verification(h)) return rc;
  if (!s->use_levels) {
    // The set of cells the last solve used is released here — everything that reads it has been enqueued on this stream or has been
    // waited for above — and re-armed (every cell empty: all ones) on the side stream while THIS solve runs on the other set.
    const int used = s->cur_cells, now = used ^ 1;
    RSBA_HIP_TRY(hipEventRecord(s->ev_released, st));
    RSBA_HIP_TRY(hipStreamWaitEvent(s->mstream, s->ev_released, 0));
    RSBA_HIP_TRY(hipMemsetAsync(s->cells[used], 0xFF, s->ncells * sizeof(double), s->mstream));
    RSBA_HIP_TRY(hipEventRecord(s->ev_armed[used], s->mstream));
    s->arm_pending[used] = true;
    if (s->arm_pending[now]) { RSBA_HIP_TRY(hipStreamWaitEvent(st, s->ev_armed[now], 0)); s->arm_pending[now] = false; }
    s->cur_cells = now;
    double* c = s->cells[now];
    sv.Lf = c + s->cell_off[0]; sv.chol_part = c + s->cell_off[1]; sv.Winv = c + s->cell_off[2]; sv.zv = c + s->cell_off[3]; sv.yv = sv.zv + sv.npad; sv.Xpub = c + s->cell_off[4];
    if (sv.zv2) { sv.zv2 = sv.zv + 2 * sv.npad; sv.ceta = sv.zv + 3 * sv.npad; }
    s->d_dag_args = s->d_dag_args2[now];
    if (s->hp.sharded && !s->sharded_off) {
      // launch A: the columns of this rank's part, from its own partial S — complete for them: every point that sees one of its tiles is here
      RSBA_HIP_TRY(launch_chol_dag(sv, s->plan_a, s->d_dag_args_a[now], std::min(s->dag_workgroups, std::max(1, s->plan_a.ntasks)), s->dag_one_per_cu, st));
      // exchange (2'): the separators' tiles, each rank's share less what its part subtracts from them, summed over the ranks
      const int64_t count = (int64_t)s->ntop_slots * kTile * kTile + (int64_t)s->ntop_tiles * kTile + (s->hp.two_rhs ? (int64_t)s->ntop_tiles * kTile + 8 : 0);   // (+ the second right-hand side's share: launch A left it behind the rows of the first)
      ps.stop();
      {
        PhaseScope pe(h, RSBA_PHASE_EXCHANGE);
        RSBA_HIP_TRY(launch_top_assemble(sv, s->d_top_slots, s->d_top_info, s->d_asm_ptr, s->d_asm_list, s->d_top_tiles, s->ntop_slots, s->topx_buf, st));
        if (int32_t rc = exchange(h, s->topx_buf, count, 0, RSBA_EXCHANGE_SYSTEM)) return rc;
        RSBA_HIP_TRY(launch_top_unpack(sv, s->d_top_slots, s->d_top_info, s->d_top_tiles, s->ntop_slots, s->topx_buf, st));
      }
      ps.start();
      // launch B: the separators (every rank alike), forward and backward, then this rank's part backward
      RSBA_HIP_TRY(launch_chol_dag(sv, s->plan_b, s->d_dag_args_b[now], std::min(s->dag_workgroups, std::max(1, s->plan_b.ntasks)), s->dag_one_per_cu, st));
      // exchange (4): the camera step — every rank contributes the rows of its part, rank 0 the separators'
      ps.stop();
      {
        PhaseScope pe(h, RSBA_PHASE_EXCHANGE);
        RSBA_HIP_TRY(launch_step_rows(sv.yv, s->d_row_mine, sv.npad, s->ybuf, st));
        if (int32_t rc = exchange(h, s->ybuf, sv.npad, 0, RSBA_EXCHANGE_STEP)) return rc;
        RSBA_HIP_TRY(hipMemcpyAsync(sv.yv, s->ybuf, (size_t)sv.npad * sizeof(double), hipMemcpyDeviceToDevice, st));
      }
      ps.start();
    } else
    RSBA_HIP_TRY(launch_chol_dag(sv, s->plan, s->d_dag_args, s->dag_workgroups, s->dag_one_per_cu, st));
    if (s->test_corrupt_once) { s->test_corrupt_once = false; RSBA_HIP_TRY(hipMemsetAsync(sv.yv + (sv.n / 2 / 6) * 6 + 1, 0, sizeof(double), st)); }   // test hook: one entry of the solution (a pose coordinate in mid-video) lost
    if (s->sw.chol_verify) {
      // (rhs_stays: nobody writes sv.rhs before the check has been waited for — the LM iteration without a free ratio; otherwise the check gets a copy)
      const double* b_rhs = sv.rhs;
      if (s->hp.two_rhs) { RSBA_HIP_TRY(launch_border_combine(s->verify_b, sv.rhs, s->border, 0.0, sv.npad, st, s->ratio4 + kRtC)); b_rhs = s->verify_b; }   // what was solved for: g - (s eta) b
      else if (!rhs_stays) { RSBA_HIP_TRY(hipMemcpyAsync(s->verify_b, sv.rhs, (size_t)sv.npad * sizeof(double), hipMemcpyDeviceToDevice, st)); b_rhs = s->verify_b; }
      RSBA_HIP_TRY(hipEventRecord(s->ev_solved, st));
      RSBA_HIP_TRY(hipStreamWaitEvent(s->vstream, s->ev_solved, 0));
      RSBA_HIP_TRY(launch_chol_verify(sv, s->d_slot_tiles, b_rhs, s->d_verify, s->d_verify + sv.npad, 1e-7, sv.scalars + kDagSuspect, s->vstream,
                                 s->hp.sharded && !s->sharded_off ? s->d_row_check : nullptr));   // (a rank of a sharded factorisation holds the whole of its part's rows of S, nothing else)
      RSBA_HIP_TRY(hipEventRecord(s->ev_verified, s->vstream));
      s->verify_pending = true;
    }
  } else {
    for (int l = 0; l < s->hp.nlev; ++l) {
      const int d0 = s->hp.lev_diag_ptr[l], d1 = s->hp.lev_diag_ptr[l + 1], t0 = s->hp.lev_sub_ptr[l], t1 = s->hp.lev_sub_ptr[l + 1];
      const int u0 = s->hp.lev_upd_ptr[l], u1 = s->hp.lev_upd_ptr[l + 1];
      RSBA_HIP_TRY(launch_chol_level(sv, s->plan, kTaskUpdate, u0, u1 - u0, st));
      RSBA_HIP_TRY(launch_chol_level(sv, s->plan, kTaskDiag, d0, d1 - d0, st));
      if (s->hp.two_rhs) RSBA_HIP_TRY(launch_chol_level(sv, s->plan, kTaskFwd2, d0, d1 - d0, st));
      RSBA_HIP_TRY(launch_chol_level(sv, s->plan, kTaskSub, t0, t1 - t0, st));
    }
    if (s->hp.two_rhs) RSBA_HIP_TRY(launch_chol_level(sv, s->plan, kTaskEta, 0, 1, st));
    for (int l = s->hp.nlev - 1; l >= 0; --l) {
      const int d0 = s->hp.lev_diag_ptr[l], d1 = s->hp.lev_diag_ptr[l + 1];
      RSBA_HIP_TRY(launch_chol_level(sv, s->plan, kTaskBack, d0, d1 - d0, st));
    }
  }
  return RSBA_OK;
}

// S v = b2 for one more right-hand side, through the factor tiles the last solve_reduced_system left: forward and backward
// substitution only (cholesky.hip chol_solve_kernel).  *v_out points at the solution ([npad], valid until the next call).  The result
// is checked like the first one (same sticky flag), here on the solver's own stream: the check is 20 us, the solve 0.2 ms.
int32_t solve_again(rsba_handle* h, const double* b2, const double** v_out) {
  Solver* s = h->solver; const SolverDev& sv = s->sv; hipStream_t st = h->stream;
  PhaseScope ps(h, RSBA_PHASE_CHOLESKY);
  if (!s->use_levels) RSBA_HIP_TRY(launch_chol_solve(sv, s->plan, s->d_dag_args, b2, s->zy2, s->d_dag_sync + 2, s->dag_workgroups, st));
  else {   // the same tasks, one launch per level: no polling (what a suspect persistent result is redone with)
    for (int l = 0; l < s->hp.nlev; ++l) RSBA_HIP_TRY(launch_chol_solve_level(sv, s->plan, false, s->hp.lev_diag_ptr[l], s->hp.lev_diag_ptr[l + 1] - s->hp.lev_diag_ptr[l], b2, s->zy2, st));
    for (int l = s->hp.nlev - 1; l >= 0; --l) RSBA_HIP_TRY(launch_chol_solve_level(sv, s->plan, true, s->hp.lev_diag_ptr[l], s->hp.lev_diag_ptr[l + 1] - s->hp.lev_diag_ptr[l], b2, s->zy2, st));
  }
  *v_out = s->zy2 + sv.npad;
  if (!s->use_levels && s->sw.chol_verify) {
    if (int32_t rc = await_verification(h)) return rc;   // (the accumulators of the check are shared)
    SolverDev sv2 = sv;
    sv2.yv = s->zy2 + sv.npad;
    RSBA_HIP_TRY(launch_chol_verify(sv2, s->d_slot_tiles, b2, s->d_verify, s->d_verify + sv.npad, 1e-7, sv.scalars + kDagSuspect, st));
  }
  return RSBA_OK;
}

// S y = rhs by preconditioned conjugate gradients over the packed tiles (kernels_pcg.hip): the lists and vectors on first use, ...
int32_t ensure_pcg(rsba_handle* h) {
  Solver* s = h->solver; const SolverDev& sv = s->sv;
  if (s->pcg.ready) return RSBA_OK;
  if (!pcg_build_plan(s->hp.slot_tiles, sv.nt, sv.F, sv.CD, sv.NIB, sv.NPF, &s->pcg.hp)) return rsba_set_error(RSBA_ERR_UNSUPPORTED, "iterative linear solver: the tile layout of the reduced camera system has no diagonal tile for some row");
  PcgDev& pc = s->pcg.dev; const PcgHostPlan& hp = s->pcg.hp;
  int32_t rc;
  if ((rc = s_upload_const(s, &pc.row_ptr, hp.row_ptr))) return rc;
  if ((rc = s_upload_const(s, &pc.row_list, hp.row_list))) return rc;
  if ((rc = s_upload_const(s, &pc.blk_row, hp.blk_row))) return rc;
  if ((rc = s_upload_const(s, &pc.blk_size, hp.blk_size))) return rc;
  if ((rc = s_upload_const(s, &pc.blk_slots, hp.blk_slots))) return rc;
  pc.nblk = (int)hp.blk_row.size(); pc.nbw = (pc.nblk + kPcgBlockThreads - 1) / kPcgBlockThreads;
  if ((rc = s_alloc(s, &pc.fac, (size_t)(kPcgBlockMax * (kPcgBlockMax + 1) / 2) * pc.nblk))) return rc;
  double* v = nullptr;
  if ((rc = s_alloc(s, &v, 6 * (size_t)sv.npad))) return rc;
  pc.y = v; pc.r = v + sv.npad; pc.z = v + 2 * sv.npad; pc.q = v + 3 * sv.npad; pc.p[0] = v + 4 * sv.npad; pc.p[1] = v + 5 * sv.npad;
  if ((rc = s_alloc(s, &pc.part_pq, (size_t)sv.nt))) return rc;
  if ((rc = s_alloc(s, &pc.part, 3 * (size_t)pc.nbw))) return rc;
  if ((rc = s_alloc(s, &pc.sc, (size_t)kPcgScSize))) return rc;
  s->pcg.ready = true;
  return RSBA_OK;
}
// ... then the iterations, enqueued in chunks: after each the host reads the scalars once (the flag every kernel of the iteration looks at
// first: launches behind the end of the solve return at once).  The step stays in s->pcg.dev.y.
static int32_t solve_reduced_pcg(rsba_handle* h) {
  Solver* s = h->solver; const SolverDev& sv = s->sv; hipStream_t st = h->stream;
  PhaseScope ps(h, RSBA_PHASE_CHOLESKY);
  if (int32_t rc = ensure_pcg(h)) return rc;
  const PcgDev& pc = s->pcg.dev;
  const rsba_linear_solver_options& lo = h->lin_opt;
  const PcgRule rule{lo.min_iterations, lo.max_iterations, lo.eta, lo.r_tolerance};
  RSBA_HIP_TRY(launch_pcg_begin(sv, pc, st));
  double sc[kPcgScSize] = {};
  int enqueued = 0, flip = 0, chunk = 8;
  for (;;) {
    const int n = std::min(chunk, lo.max_iterations - enqueued);
    for (int k = 0; k < n; ++k) { RSBA_HIP_TRY(launch_pcg_iteration(sv, pc, rule, flip, st)); flip ^= 1; }
    enqueued += n;
    RSBA_HIP_TRY(hipMemcpyAsync(sc, pc.sc, sizeof sc, hipMemcpyDeviceToHost, st));
    RSBA_HIP_TRY(hipStreamSynchronize(st));
    if (sc[kPcgDone] != 0.0 || enqueued >= lo.max_iterations) break;
    chunk = std::min(2 * chunk, 64);
  }
  rsba_linear_solver_stats& ls = h->lin_stats;
  const int iters = (int)sc[kPcgK];
  ++ls.num_linear_solves; ls.total_iterations += iters; ls.max_iterations = std::max(ls.max_iterations, iters);
  if (sc[kPcgDone] == 2.0) ++ls.num_solves_at_cap;
  if (sc[kPcgDone] == 3.0) ++ls.num_failed_solves;
  ls.last_iterations = iters; ls.last_relative_residual = sc[kPcgRel];
  return RSBA_OK;
}

// ratio (free interFrameRatio only): in {h_s + D/radius, g_s, scale of the ratio}, out the ratio's scaled step eta.
// The ratio's column b of the damped normal equations is a 1-wide dense border of S.  With S = L L^T, z = L^-1 g, z2 = L^-1 b:
//   eta = (g_s - s z2.z) / (h_s + D - s^2 z2.z2),   L^T y = z - (s eta) z2
// — both forward solves inside the factorisation's own launch (FWD2 tasks beside the DIAG tasks, chol_tasks.hpp), the ETA task between
// the phases, ONE backward solve.  (Until round 4 the second right-hand side took a launch of its own: S u = g, S v = b, y = u - s eta v.)
// ratio == nullptr with a two-column plan: the device-side loop — the ratio's scalars are on the device already (ratio_prepare_ctl).
int32_t factor_and_solve(rsba_handle* h, double radius, RatioStep* ratio) {
  Solver* s = h->solver; const SolverDev& sv = s->sv; hipStream_t st = h->stream;
  if (ratio) RSBA_HIP_TRY(launch_ratio_prepare(s->ratio4, ratio->diag, ratio->gs, ratio->scale, st));
  int32_t rc = reduce_system(h, radius);
  if (rc) return rc;
  if (s->pcg.on) {   // the iterative solver: no factor, no verification — its own residual is its check
    if ((rc = solve_reduced_pcg(h))) return rc;
    s->sv.step = s->pcg.dev.y;
    PhaseScope ps(h, RSBA_PHASE_BACK_SUBSTITUTE);
    RSBA_HIP_TRY(launch_back_substitute(h->dp, sv, st));
    return RSBA_OK;
  }
  if ((rc = solve_reduced_system(h, /*rhs_stays=*/!s->hp.two_rhs))) return rc;
  if (ratio) {
    RSBA_HIP_TRY(hipMemcpyAsync(&ratio->eta, s->ratio4 + kRtEta, sizeof(double), hipMemcpyDeviceToHost, st));
    RSBA_HIP_TRY(hipStreamSynchronize(st));
  }
  s->sv.step = sv.yv;   // the camera step is read where the solve left it (the cells of this solve stay armed until the next one)
  PhaseScope ps(h, RSBA_PHASE_BACK_SUBSTITUTE);
  RSBA_HIP_TRY(launch_back_substitute(h->dp, sv, st));
  return RSBA_OK;
}

}  // namespace rsba

// rsba_set_loss: the (f, f-1) blocks of the motion priors are dense under a general loss and 2 x 2 per coordinate otherwise — the kernel
// of the second kind writes its own entries only, so what the first kind left elsewhere goes here
int32_t rsba_solver_loss_changed(rsba_handle* h) {
  if (!h || !h->solver || !h->solver->ucross) return RSBA_OK;
  RSBA_HIP_TRY(hipSetDevice(h->device));
  RSBA_HIP_TRY(hipMemsetAsync(h->solver->ucross, 0, h->solver->ucross_len * sizeof(double), h->stream));
  return RSBA_OK;
}

// gradient of Problem::Evaluate: loss-corrected J^T r on the masked tangent space, [F*P*6 | M*3 | NI*9]
int32_t rsba_gradient(rsba_handle* h, double* g) {
  int32_t rc = build_solver(h);
  if (rc) return rc;
  Solver* s = h->solver; const DeviceProblem& dp = h->dp;
  if ((rc = reset_scales(h))) return rc;
  if ((rc = linearize(h))) return rc;
  RSBA_HIP_TRY(launch_unscaled_gradient(dp, s->sv, s->d_gpose, s->d_gpoint, h->stream));
  const size_t npose = (size_t)dp.F * dp.P * 6, npt = (size_t)dp.M * 3;
  RSBA_HIP_TRY(hipMemcpyAsync(g, s->d_gpose, npose * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  RSBA_HIP_TRY(hipMemcpyAsync(g + npose, s->d_gpoint, npt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  std::fill(g + npose + npt, g + npose + npt + (size_t)dp.NI * 9, 0.0);
  for (int c = 0; c < s->sv.NIB; ++c)   // the 9 coordinates of block c sit at the front of its pseudo frames
    RSBA_HIP_TRY(hipMemcpyAsync(g + npose + npt + (size_t)c * 9, s->d_gpose + npose + (size_t)c * s->sv.NPF * s->sv.CD, 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  RSBA_HIP_TRY(hipStreamSynchronize(h->stream));
  return RSBA_OK;
}

extern "C" int32_t rsba_set_exchange(rsba_handle* h, rsba_allreduce_fn fn, void* ctx, int32_t rank, int32_t world) {
  if (!h || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "bad exchange arguments");
  if (h->solver) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "rsba_set_exchange must precede the first solve / gradient call");
  h->allreduce = fn; h->allreduce_ctx = ctx; h->rank = rank; h->world = world;
  return RSBA_OK;
}

extern "C" int32_t rsba_get_block_structure(rsba_handle* h, uint8_t* mask, int64_t* frame_obs_count) {
  if (!h || !mask) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  const int F = h->dp.F; const int64_t N = h->dp.N;
  std::fill(mask, mask + (size_t)F * F, (uint8_t)0);
  if (frame_obs_count) std::fill(frame_obs_count, frame_obs_count + F, (int64_t)0);
  // observations grouped by point: frames of one point pairwise share it
  std::vector<int64_t> ptr((size_t)h->dp.M + 1, 0);
  for (int64_t i = 0; i < N; ++i) ptr[h->obs_point[i] + 1]++;
  for (int j = 0; j < h->dp.M; ++j) ptr[j + 1] += ptr[j];
  std::vector<int32_t> fr(N);
  { std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1); for (int64_t i = 0; i < N; ++i) fr[fill[h->obs_point[i]]++] = h->obs_frame[i]; }
  for (int j = 0; j < h->dp.M; ++j)
    for (int64_t x = ptr[j]; x < ptr[j + 1]; ++x) for (int64_t y = ptr[j]; y <= x; ++y) {
      const int a = std::max(fr[x], fr[y]), b = std::min(fr[x], fr[y]);
      mask[(size_t)a * F + b] = 1;
    }
  if (frame_obs_count) for (int64_t i = 0; i < N; ++i) frame_obs_count[h->obs_frame[i]]++;
  return RSBA_OK;
}

extern "C" int32_t rsba_set_block_structure(rsba_handle* h, const uint8_t* mask, const int64_t* frame_obs_count) {
  if (!h || !mask) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  if (h->solver) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "rsba_set_block_structure must precede the first solve / gradient call");
  const int F = h->dp.F;
  h->union_mask.assign(mask, mask + (size_t)F * F);
  if (frame_obs_count) h->frame_obs_total.assign(frame_obs_count, frame_obs_count + F); else h->frame_obs_total.clear();
  return RSBA_OK;
}

extern "C" int32_t rsba_get_phase_times(rsba_handle* h, rsba_phase_times* out) {
  if (!h || !out) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  std::memset(out, 0, sizeof *out);
  if (!h->solver) return RSBA_OK;
  for (int p = 0; p < RSBA_NUM_PHASES; ++p) { out->ms[p] = h->solver->timer.ms[p]; out->calls[p] = h->solver->timer.calls[p]; }
  return RSBA_OK;
}
extern "C" const char* rsba_exchange_name(int32_t kind) {
  static const char* names[RSBA_NUM_EXCHANGES] = {"setup", "(1) camera blocks", "(2) reduced system", "(3) step scalars", "(4) camera step", "point merge"};
  return kind >= 0 && kind < RSBA_NUM_EXCHANGES ? names[kind] : "?";
}
extern "C" int32_t rsba_get_exchange_stats(rsba_handle* h, rsba_exchange_stats* out) {
  if (!h || !out) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  std::memset(out, 0, sizeof *out);
  out->rank = h->rank; out->world = h->world;
  for (int k = 0; k < RSBA_NUM_EXCHANGES; ++k) { out->calls[k] = h->x_calls[k]; out->doubles[k] = h->x_doubles[k]; if (h->solver) out->ms[k] = h->solver->xtimer.ms[k]; }
  return RSBA_OK;
}
extern "C" const char* rsba_phase_name(int32_t phase) {
  static const char* names[RSBA_NUM_PHASES] = {"eval_lm", "camera_blocks", "point_blocks", "point_factor", "project", "schur", "cholesky",
                                               "back_substitute", "candidate", "eval_trial", "priors", "exchange", "other"};
  return phase >= 0 && phase < RSBA_NUM_PHASES ? names[phase] : "?";
}
extern "C" int32_t rsba_get_plan_stats(rsba_handle* h, rsba_plan_stats* out) {
  if (!h || !out) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  RSBA_HIP_TRY(hipSetDevice(h->device));
  int32_t rc = build_solver(h);
  if (rc) return rc;
  *out = h->solver->stats;
  unsigned long long issued = 0;
  RSBA_HIP_TRY(hipMemcpyAsync(&issued, h->solver->sv.schur_mfma_count, sizeof issued, hipMemcpyDeviceToHost, h->stream));
  RSBA_HIP_TRY(hipStreamSynchronize(h->stream));
  out->schur_mfma_issued = (int64_t)issued; out->schur_launches = h->solver->schur_launches;
  return RSBA_OK;
}

extern "C" int32_t rsba_sync_block_structure(rsba_handle* h) {
  if (!h) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null handle");
  if (h->solver) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "rsba_sync_block_structure must precede the first solve / gradient call");
  if (!h->allreduce) return RSBA_OK;
  RSBA_HIP_TRY(hipSetDevice(h->device));
  const size_t F = (size_t)h->dp.F, M = (size_t)h->dp.M, count = F * F + F + M;
  std::vector<uint8_t> mask(F * F); std::vector<int64_t> cnt(F);
  int32_t rc = rsba_get_block_structure(h, mask.data(), cnt.data());
  if (rc) return rc;
  // one all-reduce (sum) of [mask | per-frame counts | per-point "observed here" flags], as doubles: the exchange's type
  std::vector<double> host(count, 0.0);
  for (size_t i = 0; i < F * F; ++i) host[i] = mask[i];
  for (size_t f = 0; f < F; ++f) host[F * F + f] = (double)cnt[f];
  for (int64_t i = 0; i < h->dp.N; ++i) host[F * F + F + (size_t)h->obs_point[i]] = 1.0;
  double* dev = nullptr;
  RSBA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dev), count * sizeof(double)));
  hipError_t e = hipMemcpyAsync(dev, host.data(), count * sizeof(double), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) { rc = exchange(h, dev, (int64_t)count, 0, RSBA_EXCHANGE_SETUP); if (rc) { (void)hipFree(dev); return rc; } }
  if (e == hipSuccess) e = hipMemcpyAsync(host.data(), dev, count * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(dev);
  if (e != hipSuccess) return rsba_set_error(RSBA_ERR_HIP, hipGetErrorString(e));
  for (size_t j = 0; j < M; ++j)
    if (host[F * F + F + j] > 1.0) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "a point has observations on more than one rank: partition the observations by point");
  for (size_t i = 0; i < F * F; ++i) mask[i] = host[i] != 0.0;
  for (size_t f = 0; f < F; ++f) cnt[f] = (int64_t)host[F * F + f];
  return rsba_set_block_structure(h, mask.data(), cnt.data());
}

extern "C" int32_t rsba_normal_equations(rsba_handle* h, double* U, double* gc, double* V, double* gp) {
  if (!h) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null handle");
  RSBA_HIP_TRY(hipSetDevice(h->device));
  int32_t rc = build_solver(h);
  if (rc) return rc;
  Solver* s = h->solver; const DeviceProblem& dp = h->dp; const int CD = s->sv.CD;
  if ((rc = reset_scales(h))) return rc;
  if ((rc = linearize(h))) return rc;
  if (U) RSBA_HIP_TRY(hipMemcpyAsync(U, s->sv.U, (size_t)dp.F * CD * CD * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (gc) RSBA_HIP_TRY(hipMemcpyAsync(gc, s->sv.gc, (size_t)dp.F * CD * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  std::vector<double> v6;
  if (V) { v6.resize((size_t)dp.M * 6); RSBA_HIP_TRY(hipMemcpyAsync(v6.data(), s->sv.V, v6.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream)); }
  if (gp) RSBA_HIP_TRY(hipMemcpyAsync(gp, s->sv.gp, (size_t)dp.M * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  RSBA_HIP_TRY(hipStreamSynchronize(h->stream));
  if (V) for (int j = 0; j < dp.M; ++j) {
    const double* v = &v6[(size_t)j * 6]; double* o = V + (size_t)j * 9;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[1]; o[4] = v[3]; o[5] = v[4]; o[6] = v[2]; o[7] = v[4]; o[8] = v[5];
  }
  return RSBA_OK;
}

namespace {

// One call of rsba_solve: the state of the trust-region loop, shared by its two forms — the decisions taken on the device
// (run_device_loop) or on the host (run_host_loop, also what a device loop hands over to after a suspect factorisation).
struct LmRun {
  rsba_handle* const h; const rsba_solver_options* const opt; rsba_solver_summary* const sum; rsba_iteration* const trace; const int32_t trace_cap;
  const double t_start;
  Solver* const s; SolverDev& sv; DeviceProblem& dp; const hipStream_t st;
  bool done = false;                // finish() has run: the call returns
  int ntrace = 0;                   // the trace cursor
  double host_sc[16]; double cost2[2]; int nfail = 0, cfail = 0;   // what read_back() brought
  // free interFrameRatio (the reference's default for the motion priors, CeresHandler.h:161,172,175): one more unknown of
  // the LM, kept on the host — value, Jacobi scale, LM diagonal, and {h, g} = its column's J^T J and J^T r from the device.
  // The candidate is projected onto the lower bound (ParameterBlock::Plus); Ceres' projected line search is not restated.
  const bool free_ratio; const double ratio_lb;
  double ratio, ratio_scale = 1.0, ratio_diag = 0.0, ratio_hg[2] = {0.0, 0.0}, ratio_new;
  double cost = 0.0, fixed = 0.0, gmax = 0.0, radius, decrease_factor = 2.0; bool reuse_diagonal = false;
  int invalid_streak = 0, iteration = 0;
  bool any_rank_needs_host = false, speculate = false;
  const bool has_pp;

  LmRun(rsba_handle* h_, const rsba_solver_options* opt_, rsba_solver_summary* sum_, rsba_iteration* trace_, int32_t trace_cap_, double t_start_)
      : h(h_), opt(opt_), sum(sum_), trace(trace_), trace_cap(trace_cap_), t_start(t_start_), s(h_->solver), sv(h_->solver->sv), dp(h_->dp), st(h_->stream),
        free_ratio(h_->solver->border != nullptr), ratio_lb(h_->dp.prior_kind == 2 ? 2.220446049250313e-16 : 0.0), ratio(h_->dp.prior_ratio), ratio_new(h_->dp.prior_ratio),
        radius(opt_->initial_trust_region_radius), has_pp(h_->dp.pp_count > 0 || h_->dp.pp_spherical >= 0) {}

  void push(const rsba_iteration& it) {
      if (trace && ntrace < trace_cap) trace[ntrace] = it;
      ++ntrace; sum->num_iterations = ntrace;
      if (opt->minimizer_progress_to_stdout)
        std::printf("%4d  cost % .6e  change % .3e  |grad| %.3e  |step| %.3e  rho % .3e  radius %.3e  %s\n", it.iteration, it.cost, it.cost_change,
                    it.gradient_max_norm, it.step_norm, it.relative_decrease, it.trust_region_radius, it.step_is_successful ? "ok" : (it.iteration ? "rejected" : ""));
  }
  // the record of an iteration as it ends, ...
  void record(rsba_iteration& it) { it.cost = cost + fixed; it.trust_region_radius = radius; push(it); }
  // ... and of the one the solve ends with
  int32_t terminate(rsba_iteration& it, int32_t term) { record(it); return finish(term); }
  double with_ratio_gradient(double g) const { return free_ratio ? std::max(g, std::fabs(ratio - std::max(ratio_lb, ratio - ratio_hg[1]))) : g; }
  // current <-> candidate parameter buffers (intrinsics only when they are a parameter block)
  void swap_params() {
      std::swap(dp.poses, sv.trial_poses); std::swap(dp.points, sv.trial_points);
      if (sv.NPF > 0) std::swap(dp.intr, sv.trial_intr);
      if (dp.pp_count > 0) std::swap(dp.pp_value, dp.pp_trial);
  }
  // The persistent driver's solution does not satisfy the system it was given: this iteration is repeated, and the problem finished, on
  // the level schedule (a sharded factorisation goes back to the replicated one: the level schedule needs the whole of S on every rank)
  void fall_back_to_levels() { s->use_levels = true; ++s->dag_fallbacks; ++sum->num_dag_fallbacks; s->sharded_off = true; }
  int32_t read_back();
  int32_t finish(int32_t term);
  int32_t refuse_unsupported_pcg();
  int32_t exchange_problem_size();
  int32_t initial_evaluation();
  bool choose_device_loop();
  int32_t enqueue_device_iteration(const LmRules& R, int cap, int enqueued);
  int32_t run_device_loop();
  int32_t run_host_loop();
};

int32_t LmRun::read_back() {
  RSBA_HIP_TRY(hipMemcpyAsync(host_sc, sv.scalars, sizeof host_sc, hipMemcpyDeviceToHost, st));
  if (free_ratio) RSBA_HIP_TRY(hipMemcpyAsync(ratio_hg, s->ratio4, sizeof ratio_hg, hipMemcpyDeviceToHost, st));
  RSBA_HIP_TRY(hipStreamSynchronize(st));
  if (s->timer.on) s->timer.resolve();
  if (s->xtimer.on) s->xtimer.resolve();
  cost2[0] = host_sc[kCost]; cost2[1] = host_sc[kFixedCost];
  nfail = host_sc[kEvalFailed] != 0.0; cfail = host_sc[kSolveFailed] != 0.0;
  return RSBA_OK;
}

int32_t LmRun::finish(int32_t term) {
  done = true;
  sum->termination_type = term;
  sum->is_solution_usable = term != RSBA_FAILURE;
  (void)reset_scales(h);
  const size_t npose = (size_t)dp.F * dp.P * 6, npt = (size_t)dp.M * 3;
  if (h->allreduce && h->world > 1) {   // every rank leaves with the complete point array: each point from its owner
    RSBA_HIP_TRY(launch_own_points(dp, sv, s->merge_buf, st));
    int32_t rc2 = exchange(h, s->merge_buf, 4 * (int64_t)dp.M, 0, RSBA_EXCHANGE_POINTS);
    if (rc2) return rc2;
    RSBA_HIP_TRY(launch_merge_points(dp, s->merge_buf, st));
  }
  RSBA_HIP_TRY(hipMemcpyAsync(h->desc.poses, dp.poses, npose * sizeof(double), hipMemcpyDeviceToHost, st));
  RSBA_HIP_TRY(hipMemcpyAsync(h->desc.points, dp.points, npt * sizeof(double), hipMemcpyDeviceToHost, st));
  if (!dp.calibrated) RSBA_HIP_TRY(hipMemcpyAsync(h->desc.intrinsics, dp.intr, (size_t)dp.NI * 9 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (dp.pp_count > 0 && h->pp_host) RSBA_HIP_TRY(hipMemcpyAsync(h->pp_host, dp.pp_value, 6 * (size_t)dp.pp_count * sizeof(double), hipMemcpyDeviceToHost, st));
  RSBA_HIP_TRY(hipStreamSynchronize(st));
  if (s->timer.on) { s->timer.resolve(); s->timer.on = false; }
  if (s->xtimer.on) { s->xtimer.resolve(); s->xtimer.on = false; }
  h->prior_ratio_result = dp.prior_ratio;
  sum->total_time_s = now_s() - t_start;
  if (Solver* sl = h->solver; sl->d_trace && sl->sw.chol_trace) {   // debugging aid, off by default
    std::vector<long long> tr(8 * (size_t)sl->plan.ntasks);
    RSBA_HIP_TRY(hipMemcpy(tr.data(), sl->d_trace, tr.size() * sizeof(long long), hipMemcpyDeviceToHost));
    if (FILE* f = std::fopen(sl->sw.chol_trace->c_str(), "wb")) {
      const int32_t n = sl->plan.ntasks;
      std::fwrite(&n, sizeof(n), 1, f);
      std::fwrite(sl->hp.tasks.data(), sizeof(int32_t), sl->hp.tasks.size(), f);
      std::fwrite(tr.data(), sizeof(long long), tr.size(), f);
      std::fclose(f);
    }
  }
  return RSBA_OK;
}

// The iterative linear solver (rsba_set_linear_solver): what it does not take is refused before anything of the solve has run
int32_t LmRun::refuse_unsupported_pcg() {
  s->pcg.on = h->lin_opt.type == RSBA_LINEAR_SOLVER_PCG;
  h->lin_stats = rsba_linear_solver_stats{};
  if (s->pcg.on) {
    const char* why = s->border ? "a free interFrameRatio (its border column needs a second solve)"
                    : h->allreduce ? "a handle with an exchange attached (one rank only)"
                    : opt->level_scheduled_cholesky ? "options.level_scheduled_cholesky (there is no factorisation to schedule)" : nullptr;
    if (why) { s->pcg.on = false; return rsba_set_error(RSBA_ERR_UNSUPPORTED, (std::string("the iterative linear solver does not take ") + why).c_str()); }
  }
  return RSBA_OK;
}

// problem-size figures of the whole (all-rank) problem
int32_t LmRun::exchange_problem_size() {
  int32_t rc;
  const double npri = sv.lead ? (double)h->prior_frames.size() + (double)h->pp_blocks.size() + (dp.pp_spherical >= 0 ? 1.0 : 0.0) : 0.0;
  // (+ how many ranks cannot run the loop without the host — no observations, or phase timers on: every rank must take the same form of the loop)
  const bool host_form_only = dp.N == 0 || s->timer.on || s->pcg.on || s->solve_sw.test_device_lm_off_on_this_rank;   // (the iterative linear solver reads its convergence flag on the host)
  double cnt[4] = {(double)dp.N + npri, (double)(s->num_reduced_blocks + s->num_priors_reduced), (double)s->num_reduced_params, host_form_only ? 1.0 : 0.0};
  if (h->allreduce) {
    RSBA_HIP_TRY(hipMemcpyAsync(sv.scalars + 8, cnt, sizeof cnt, hipMemcpyHostToDevice, st));
    if ((rc = exchange(h, sv.scalars + 8, 4, 0, RSBA_EXCHANGE_SETUP))) return rc;
    RSBA_HIP_TRY(hipMemcpyAsync(cnt, sv.scalars + 8, sizeof cnt, hipMemcpyDeviceToHost, st));
    RSBA_HIP_TRY(hipMemsetAsync(sv.scalars + 8, 0, 4 * sizeof(double), st));   // slots 8-11 ride in the per-iteration sum from here on
    RSBA_HIP_TRY(hipStreamSynchronize(st));
  }
  sum->num_residual_blocks = (int32_t)cnt[0]; sum->num_residual_blocks_reduced = (int32_t)cnt[1]; sum->num_parameters_reduced = (int32_t)cnt[2];
  any_rank_needs_host = cnt[3] != 0.0;
  return RSBA_OK;
}

// ---- iteration 0: initial evaluation ----
int32_t LmRun::initial_evaluation() {
  int32_t rc;
  double t0 = now_s();
  if ((rc = reset_scales(h))) return rc;
  if ((rc = linearize(h, false, true))) return rc;
  if ((rc = gradient_max(h))) return rc;
  if ((rc = read_back())) return rc;
  sum->residual_jacobian_time_s += now_s() - t0;
  if (nfail) { sum->termination_type = RSBA_FAILURE; (void)finish(RSBA_FAILURE); return rsba_set_error(RSBA_ERR_EVALUATION_FAILED, "initial residual and Jacobian evaluation failed"); }
  cost = cost2[0]; fixed = cost2[1];
  gmax = with_ratio_gradient(host_sc[kGradMax]);
  sum->fixed_cost = fixed; sum->initial_cost = cost + fixed; sum->final_cost = cost + fixed;
  rsba_iteration it; std::memset(&it, 0, sizeof it);
  it.cost = cost + fixed; it.gradient_max_norm = gmax; it.trust_region_radius = radius;
  if (gmax <= opt->gradient_tolerance) return terminate(it, RSBA_CONVERGENCE);
  if (opt->jacobi_scaling) {
    // EstimateScale from the first Jacobian, then the Jacobian is column-scaled for good; here the
    // scales feed the evaluation kernel, so re-linearise once with them
    RSBA_HIP_TRY(launch_jacobi_scale(dp, sv, st));
    RSBA_HIP_TRY(launch_pose_prior_scale(dp, s->pp, st));
    if (free_ratio) ratio_scale = 1.0 / (1.0 + std::sqrt(ratio_hg[0]));
    if ((rc = linearize(h))) return rc;
  }
  push(it);
  // A candidate is evaluated in LM mode straight away (residuals, Jacobian, per-wave camera blocks) when the problem keeps no
  // records (they would be overwritten and a rejected step needs the old ones): an accepted step — the rule — then re-uses that
  // evaluation for its linearisation instead of evaluating twice, a rejected one has computed Jacobians for nothing.
  speculate = (dp.rec == nullptr || dp.rec_alt != nullptr) && s->solve_sw.speculate;   // (records: only with a second set for the candidate's)
  return RSBA_OK;
}

// ---- trust-region control on the device ----
// The loop body below, decisions included, as a sequence of launches that never waits for the host: radius, accept / reject and the
// convergence tests live in HBM (s->d_ctl), two single-thread kernels take the decisions by the same rules in the same order, the
// kernels of an iteration read the radius there and skip themselves where the host form would not have launched them (a rejected
// candidate is not linearised).  What the reference calls per frame — windowedBA over ~100 cameras (VideoSfMClient.cc:241-246) —
// is where this counts: an iteration there is 0.5 ms, and the host form's 22 dependent launches, two read-backs and their gaps were
// 0.09 ms of it.  Here an iteration is 13 launches on this stream (the small steps share launches: kernels_lm.hip) and no wait.
// Every problem this call takes, on one rank or several (every rank takes the same form: settled with the problem-size exchange) — rounds 3 - 6
// added them kind by kind: motion priors, a free interFrameRatio, GoodPosePrior blocks, the SphericalPrior, several intrinsics blocks (their
// candidates' records go to a second set), GoodPosePrior blocks on several ranks.  What goes through the host form: phase timing, a rank that
// asks for it (no observations), RSBA_DEVICE_LM=0 / RSBA_RECORDS_ALT=0, and a suspect factorisation (the level schedule repeats the iteration).
bool LmRun::choose_device_loop() {
  const bool device_ctl = speculate && !s->use_levels && !any_rank_needs_host && opt->max_num_iterations > 0 && s->solve_sw.device_lm;   // (the switch: A/B, 0 = the host decides)
  if (device_ctl) ++s->stats.device_loop_solves; else ++s->stats.host_loop_solves;
  return device_ctl;
}

// One iteration of the device-side loop, enqueued: thirteen launches on this stream; the steps the host form spreads over twenty-two, in its
// order: kernels_lm.hip, "the same steps in fewer launches".  The diagonal's clamp rides in the point factor's launch — after a rejected
// step it recomputes what is there.
int32_t LmRun::enqueue_device_iteration(const LmRules& R, int cap, int enqueued) {
  int32_t rc;
  const bool multi = h->allreduce != nullptr;   // several ranks: the same loop with the three exchanges of an iteration enqueued between its kernels (RCCL: stream-ordered, no host wait)
  if (free_ratio) RSBA_HIP_TRY(launch_ratio_prepare_ctl(s->ratio4, s->d_ctl, opt->min_lm_diagonal, opt->max_lm_diagonal, st));   // the ratio's damped pivot and gradient for the ETA task of the factorisation
  if (dp.pp_count > 0) RSBA_HIP_TRY(launch_pose_prior_clamp(dp, s->pp, opt->min_lm_diagonal, opt->max_lm_diagonal, st));   // (the priorPoses coordinates' LM diagonal: recomputed from what the last accepted linearisation left — the same numbers after a rejected step)
  if ((rc = factor_and_solve(h, 1.0))) return rc;   // (the radius argument is ignored: the kernels read ctl)
  if (free_ratio) RSBA_HIP_TRY(launch_ratio_candidate(s->ratio4, s->d_ctl, st));
  RSBA_HIP_TRY(launch_candidate_and_model_cost(dp, sv, st));
  if (owns_motion_priors(h)) RSBA_HIP_TRY(launch_prior_model(dp, sv, sv.scalars + kModelCostChange, 0.0, st, free_ratio ? s->ratio4 + kRtC : nullptr));   // motion priors: their share of the model cost change (a free ratio's step included) ...
  if (has_pp) RSBA_HIP_TRY(launch_pose_prior_step(dp, sv, s->pp, 1.0, st));   // per-pose priors: the candidate priorPoses values, their share of the three sums (the lead rank's to add)
  swap_params();
  { DeviceProblem dq = dp; dq.rec_candidate = 1; RSBA_HIP_TRY(launch_eval(dq, kLmJacobian, st)); }   // (a problem that keeps records: the candidate's go to the other set)
  const bool extra_cost = s->ucross != nullptr || has_pp;   // prior blocks add their cost behind the observations': the cost is reduced by a launch of its own then
  if (extra_cost) {                                                                                // ... their cost at the candidate, behind the observations' ...
    RSBA_HIP_TRY(launch_cost_reduce(dp, h->d_cost2, st));
    if (owns_motion_priors(h)) {
      DeviceProblem dq = dp;
      if (free_ratio) dq.prior_ratio_ptr = s->ratio4 + kRtRatioEval;   // (... at the candidate's ratio)
      RSBA_HIP_TRY(launch_prior_cost(dq, h->d_cost2, h->prior_invalid, st));
    }
    if (has_pp && sv.lead) RSBA_HIP_TRY(launch_pose_prior_cost(dp, h->d_cost2, st));   // (replicated blocks: the lead rank's share of the summed cost)
  }
  swap_params();
  if ((rc = await_verification(h))) return rc;
  const bool my_priors = owns_motion_priors(h);
  if (!multi) RSBA_HIP_TRY(launch_lm_verdict_step(dp, sv, h->d_cost2, s->d_ctl, R, s->d_trace_it, cap, st, /*cost_reduced=*/extra_cost));
  else {   // several ranks: the scalars of the step are summed over the ranks between the reduction and the decision — exchange (3), enqueued like a kernel
    if (!extra_cost) RSBA_HIP_TRY(launch_cost_reduce(dp, h->d_cost2, st));
    RSBA_HIP_TRY(launch_pack_trial(dp, sv, h->d_cost2, st));
    if ((rc = exchange(h, sv.scalars, 12, 0, RSBA_EXCHANGE_SCALARS))) return rc;
    RSBA_HIP_TRY(launch_lm_decide_step(sv, s->d_ctl, R, s->d_trace_it, cap, st));
  }
  bool fused = false;
  RSBA_HIP_TRY(launch_linearize_blocks(dp, sv, st, &fused));   // camera blocks, the accepted candidate's copy over x, point blocks: side by side in one launch
  if (!fused) RSBA_HIP_TRY(launch_camera_blocks(dp, sv, st, /*take_candidate=*/true, /*padding_is_zero=*/true));   // (the initial linearisation zeroed the pseudo frames' padding)
  if (my_priors) RSBA_HIP_TRY(launch_prior_blocks(dp, sv, s->ucross, st));                             // ... and their blocks of an accepted step's linearisation
  if (free_ratio) RSBA_HIP_TRY(launch_prior_border(all_priors(h), sv, s->border, s->ratio4, st));      // (the ratio's column at the accepted point: every rank, from replicated poses)
  if (has_pp) { RSBA_HIP_TRY(launch_pose_prior_take(dp, sv, st)); RSBA_HIP_TRY(launch_pose_prior_blocks(dp, sv, s->pp, st)); }   // per-pose priors: the accepted values, their blocks
  RSBA_HIP_TRY(launch_intr_blocks(dp, sv, st));
  if (!fused) RSBA_HIP_TRY(launch_point_blocks(dp, sv, st));
  s->ctl_seq += 1.0;
  double* const slot = s->h_ctl_dev + (size_t)(enqueued % Solver::kCtlRing) * kCtlSize;   // (where the last kernel of this iteration leaves the state for the host)
  if (!multi) {
    RSBA_HIP_TRY(launch_lm_linearize_gradient(dp, sv, h->d_cost2, st));
    const int ngm = (int)((sv.n + 3 * (int64_t)dp.M + 255) / 256);
    if (dp.pp_count > 0) RSBA_HIP_TRY(launch_pose_prior_gradmax(dp, sv, s->pp, st, sv.partial + ngm));   // (one more partial maximum for the verdict)
    RSBA_HIP_TRY(launch_lm_verdict_gradient(dp, sv, s->d_ctl, R, s->d_trace_it, cap, slot, s->ctl_seq, st, false, dp.pp_count > 0 ? 1 : 0));
  } else {   // exchange (1): the camera gradient, diag(U), the cost — and every rank's gradient maximum over its points — whether or not the candidate
             // was accepted (the host does not know): the unpacking skips itself after a rejected one, the maximum comes out as it was
    const bool ride = h->world <= kMaxRankSlots && dp.pp_count == 0;   // (the priorPoses blocks' maximum is the lead rank's alone: a MAX exchange of its own then, as in the host form)
    if ((rc = exchange_camera_gradient(h, ride))) return rc;
    if (!ride) {
      RSBA_HIP_TRY(launch_gradient_max(dp, sv, st));
      if (sv.lead) RSBA_HIP_TRY(launch_pose_prior_gradmax(dp, sv, s->pp, st));
      if ((rc = exchange(h, sv.scalars + kGradMax, 1, 1, RSBA_EXCHANGE_SCALARS))) return rc;
    }
    RSBA_HIP_TRY(launch_lm_verdict_gradient(dp, sv, s->d_ctl, R, s->d_trace_it, cap, slot, s->ctl_seq, st, /*gradmax_done=*/true));
  }
  return RSBA_OK;
}

int32_t LmRun::run_device_loop() {
  int32_t rc;
  const int cap = opt->max_num_iterations + 2;
  if (cap > s->trace_it_cap) { if ((rc = s_alloc(s, &s->d_trace_it, (size_t)cap))) return rc; s->trace_it_cap = cap; }
  const LmRules R{opt->max_num_iterations, opt->max_num_consecutive_invalid_steps, opt->max_trust_region_radius, opt->min_trust_region_radius, opt->min_relative_decrease,
                  opt->function_tolerance, opt->gradient_tolerance, opt->parameter_tolerance};
  if (!s->h_ctl) {
    static_assert((size_t)(Solver::kCtlRing + 1) * kCtlSize * sizeof(double) <= 4096, "one pooled pinned block");
    RSBA_HIP_TRY(dev_pinned_acquire(reinterpret_cast<void**>(&s->h_ctl), (size_t)(Solver::kCtlRing + 1) * kCtlSize * sizeof(double)));
    RSBA_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&s->h_ctl_dev), s->h_ctl, 0));
    std::fill(s->h_ctl, s->h_ctl + (size_t)(Solver::kCtlRing + 1) * kCtlSize, 0.0);
  }
  double* const hc0 = s->h_ctl + (size_t)Solver::kCtlRing * kCtlSize;   // the initial state (pinned: the upload does not wait for the host)
  std::fill(hc0, hc0 + kCtlSize, 0.0);
  hc0[kCtlRadius] = radius; hc0[kCtlDecrease] = decrease_factor; hc0[kCtlCost] = cost; hc0[kCtlFixed] = fixed; hc0[kCtlGmax] = gmax; hc0[kCtlFinalCost] = sum->final_cost;
  RSBA_HIP_TRY(hipMemcpyAsync(s->d_ctl, hc0, kCtlSize * sizeof(double), hipMemcpyHostToDevice, st));
  struct CtlGuard {   // whichever way this block is left, the host form finds the state it expects: nobody skips, the radius (and the ratio) come by value
    rsba_handle* h; Solver* s;
    ~CtlGuard() { (void)hipStreamSynchronize(h->stream); s->sv.ctl = nullptr; h->dp.ctl = nullptr; h->dp.prior_ratio_ptr = nullptr; s->clamp_with_factor = false; (void)hipMemsetAsync(s->d_ctl, 0, kCtlSize * sizeof(double), h->stream); }
  } ctl_guard{h, s};
  sv.ctl = s->d_ctl; dp.ctl = s->d_ctl;
  if (free_ratio) {   // the ratio joins the state on the device: value, Jacobi scale, lower bound ({h, g} of the last linearisation are there)
    RSBA_HIP_TRY(launch_ratio_init(s->ratio4, ratio, ratio_scale, ratio_lb, st));
    dp.prior_ratio_ptr = s->ratio4 + kRtRatio;
  }
  s->clamp_with_factor = true; s->clamp_lo_hi[0] = opt->min_lm_diagonal; s->clamp_lo_hi[1] = opt->max_lm_diagonal;
  RSBA_HIP_TRY(launch_begin_solve(sv, st));   // (from here on the last kernel of an iteration clears the two flags for the next)
  // The last kernel of an iteration writes the state to a slot of pinned host memory and stamps it; the host polls the stamp (no
  // event, no copy in the stream) and enqueues the next iteration the moment it shows.  RSBA_LM_AHEAD = k keeps k iterations
  // enqueued beyond the one whose outcome the host has seen (those behind a termination fall through: every kernel looks at the
  // status word); measured at 100 and 1 000 cameras the queue does not need it — 0.492 / 0.498 / 0.500 ms per iteration for
  // k = 0 / 1 / 2 (profiles/r04/iteration_gaps.txt) — so the default enqueues nothing that might not be wanted.
  const int ahead = s->solve_sw.lm_ahead;
  const double* hc = hc0;
  int enqueued = 0, looked = 0;
  bool stopped = false;
  const double t0 = now_s();
  const double seq0 = s->ctl_seq;
  auto look = [&]() -> int32_t {   // the state behind iteration `looked`: wait for its stamp (the deciding kernel writes it last)
    const double* slot = s->h_ctl + (size_t)(looked % Solver::kCtlRing) * kCtlSize;
    const double want = seq0 + (double)(looked + 1);
    for (unsigned spins = 0;; ++spins) {
      if (__atomic_load_n(reinterpret_cast<const uint64_t*>(slot + kCtlSeq), __ATOMIC_ACQUIRE) == *reinterpret_cast<const uint64_t*>(&want)) break;
      if ((spins & 0xFFFu) == 0xFFFu) {   // now and then: is the stream still alive?  (an idle stream whose stamp never came is an error, not a wait)
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) { if (__atomic_load_n(reinterpret_cast<const uint64_t*>(slot + kCtlSeq), __ATOMIC_ACQUIRE) == *reinterpret_cast<const uint64_t*>(&want)) break; return rsba_set_error(RSBA_ERR_HIP, "the trust-region state of an iteration never reached the host"); }
        if (q != hipErrorNotReady) return rsba_set_error(RSBA_ERR_HIP, hipGetErrorString(q));
      }
      __builtin_ia32_pause();
    }
    hc = slot;
    ++looked;
    stopped = hc[kCtlStatus] != 0.0;
    return RSBA_OK;
  };
  while (!stopped && enqueued < opt->max_num_iterations) {
    if ((rc = enqueue_device_iteration(R, cap, enqueued))) return rc;
    ++enqueued;
    if (enqueued - looked > ahead) { if ((rc = look())) return rc; }
  }
  while (!stopped && looked < enqueued) { if ((rc = look())) return rc; }
  // (iterations enqueued behind the termination fall through; the stream is drained below, before anything of the loop is read or torn down)
  {
    const int have = std::min((int)hc[kCtlNumTrace], cap);
    std::vector<rsba_iteration> recs((size_t)std::max(have, 1));
    if (have > 0) RSBA_HIP_TRY(hipMemcpyAsync(recs.data(), s->d_trace_it, (size_t)have * sizeof(rsba_iteration), hipMemcpyDeviceToHost, st));
    RSBA_HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < have; ++k) push(recs[(size_t)k]);
  }
  sum->linear_solver_time_s += now_s() - t0;
  if (free_ratio) {   // the ratio's state back to the host (the stream is idle)
    double rt[kRtSize];
    RSBA_HIP_TRY(hipMemcpy(rt, s->ratio4, sizeof rt, hipMemcpyDeviceToHost));
    ratio = rt[kRtRatio]; ratio_new = ratio; ratio_diag = rt[kRtDiag]; ratio_hg[0] = rt[kRtH]; ratio_hg[1] = rt[kRtG];
    dp.prior_ratio = ratio;
  }
  radius = hc[kCtlRadius]; decrease_factor = hc[kCtlDecrease]; cost = hc[kCtlCost]; gmax = hc[kCtlGmax];
  if (dp.rec_alt && hc[kCtlRecSel] != 0.0) std::swap(dp.rec, dp.rec_alt);   // (the set that holds the current point's records is dp.rec again, as the host form has it)
  iteration = (int)hc[kCtlIteration]; invalid_streak = (int)hc[kCtlInvalidStreak];
  sum->num_successful_steps = (int)hc[kCtlSuccessful]; sum->num_unsuccessful_steps = (int)hc[kCtlUnsuccessful]; sum->final_cost = hc[kCtlFinalCost];
  const double status = hc[kCtlStatus];
  if (status > 0.0) return finish((int32_t)status - 1);
  if (status == -2.0) { (void)finish(RSBA_FAILURE); return rsba_set_error(RSBA_ERR_EVALUATION_FAILED, "residual and Jacobian evaluation failed"); }
  // status -1: the persistent driver's solution of the last iteration does not satisfy its system.  Nothing of that iteration has
  // touched x or the state: the host form repeats it, and finishes the problem, on the level schedule.
  fall_back_to_levels();
  reuse_diagonal = true;   // (the diagonal is in place)
  return RSBA_OK;
}

int32_t LmRun::run_host_loop() {
  int32_t rc;
  rsba_iteration it;
  double t0;
  while (true) {
    if (iteration >= opt->max_num_iterations) return finish(RSBA_NO_CONVERGENCE);
    t0 = now_s();
    if (!reuse_diagonal) {
      PhaseScope ps(h, RSBA_PHASE_OTHER);
      RSBA_HIP_TRY(launch_clamp_diagonal(dp, sv, opt->min_lm_diagonal, opt->max_lm_diagonal, st));
      RSBA_HIP_TRY(launch_pose_prior_clamp(dp, s->pp, opt->min_lm_diagonal, opt->max_lm_diagonal, st));
      ratio_diag = std::min(std::max(ratio_scale * ratio_scale * ratio_hg[0], opt->min_lm_diagonal), opt->max_lm_diagonal);
    }
    RSBA_HIP_TRY(launch_begin_solve(sv, st));   // chol_fail = 0 and the sticky verification flag of the DAG Cholesky = 0 (any solve of this iteration may raise it): one launch
    RatioStep rs{ratio_scale * ratio_scale * ratio_hg[0] + ratio_diag / radius, ratio_scale * ratio_hg[1], ratio_scale, 0.0};
    if ((rc = factor_and_solve(h, radius, free_ratio ? &rs : nullptr))) return rc;
    reuse_diagonal = true;
    const double ratio_step = free_ratio ? ratio_scale * rs.eta : 0.0;      // the ratio's step in its own units is -ratio_step
    ratio_new = free_ratio ? std::max(ratio_lb, ratio - ratio_step) : ratio;
    { PhaseScope ps(h, RSBA_PHASE_BACK_SUBSTITUTE); RSBA_HIP_TRY(launch_model_cost_change(dp, sv, st)); }
    if (owns_motion_priors(h)) { PhaseScope ps(h, RSBA_PHASE_PRIORS); RSBA_HIP_TRY(launch_prior_model(dp, sv, sv.scalars + kModelCostChange, std::isfinite(ratio_step) ? ratio_step : 0.0, st)); }
    { PhaseScope ps(h, RSBA_PHASE_CANDIDATE); RSBA_HIP_TRY(launch_candidate(dp, sv, st)); }
    if (dp.pp_count > 0 || dp.pp_spherical >= 0) { PhaseScope ps(h, RSBA_PHASE_PRIORS); RSBA_HIP_TRY(launch_pose_prior_step(dp, sv, s->pp, radius, st)); }   // every rank: candidate priorPoses values (scalars from the lead rank only)
    // residuals only at the candidate (T = double path)
    swap_params();
    {
      PhaseScope ps(h, RSBA_PHASE_EVAL_TRIAL);
      { DeviceProblem dq = dp; dq.rec_candidate = 1; RSBA_HIP_TRY(launch_eval(dq, speculate ? kLmJacobian : kResidualOnly, st)); }
      RSBA_HIP_TRY(launch_cost_reduce(dp, h->d_cost2, st));
    }
    if (owns_motion_priors(h)) {
      PhaseScope ps(h, RSBA_PHASE_PRIORS);
      dp.prior_ratio = std::isfinite(ratio_new) ? ratio_new : ratio;
      RSBA_HIP_TRY(launch_prior_cost(dp, h->d_cost2, h->prior_invalid, st));
      dp.prior_ratio = ratio;
    }
    if (sv.lead) RSBA_HIP_TRY(launch_pose_prior_cost(dp, h->d_cost2, st));
    swap_params();
    // exchange (3): model decrease, |step|^2, |x|^2, (skip the max slot), trial cost, -, failure flags
    {
      PhaseScope ps(h, RSBA_PHASE_EXCHANGE);
      if ((rc = await_verification(h))) return rc;   // (its flag rides in the scalars below)
      RSBA_HIP_TRY(launch_pack_trial(dp, sv, h->d_cost2, st));
      if ((rc = exchange(h, sv.scalars, 12, 0, RSBA_EXCHANGE_SCALARS))) return rc;   // one sum: ... and the verification flag of the Cholesky driver (every rank decides alike); slot kGradMax comes back as it was (pack_trial: the lead rank's copy, zeros from the others)
    }
    if ((rc = read_back())) return rc;
    if (host_sc[kDagSuspect] != 0.0 && !s->use_levels) {
      // the persistent driver's solution does not satisfy the system it was given: nothing of this iteration has touched
      // x yet — repeat it, and finish this problem, on the level schedule
      fall_back_to_levels();
      continue;   // (the flag is cleared at the top of the iteration)
    }
    cost2[1] = 0.0;   // the trial evaluation reports the total in kCost
    sum->linear_solver_time_s += now_s() - t0;
    ++iteration;
    std::memset(&it, 0, sizeof it); it.iteration = iteration;
    if (free_ratio) { host_sc[kStepSq] += (ratio - ratio_new) * (ratio - ratio_new); host_sc[kXSq] += ratio * ratio; }
    const double model_cost_change = host_sc[kModelCostChange];
    const bool solved = !cfail && std::isfinite(model_cost_change) && std::isfinite(host_sc[kStepSq]);
    const bool valid = solved && model_cost_change >= 0.0;
    it.model_cost_change = solved ? model_cost_change : 0.0;
    if (!valid) {
      if (++invalid_streak >= opt->max_num_consecutive_invalid_steps) return terminate(it, RSBA_FAILURE);
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;   // StepIsInvalid == StepRejected(0)
      ++sum->num_unsuccessful_steps;
      it.gradient_max_norm = gmax;
    } else {
      invalid_streak = 0; it.step_is_valid = 1;
      const double new_cost = nfail ? std::numeric_limits<double>::max() : (cost2[0] + cost2[1]) - fixed;
      it.step_norm = std::sqrt(host_sc[kStepSq]);
      const double x_norm = std::sqrt(host_sc[kXSq]);
      if (it.step_norm <= opt->parameter_tolerance * (x_norm + opt->parameter_tolerance)) return terminate(it, RSBA_CONVERGENCE);
      it.cost_change = cost - new_cost;
      if (std::fabs(it.cost_change) < opt->function_tolerance * cost) return terminate(it, RSBA_CONVERGENCE);
      it.relative_decrease = it.cost_change / model_cost_change;
      if (it.relative_decrease > opt->min_relative_decrease) {
        it.step_is_successful = 1; ++sum->num_successful_steps;
        const double t3 = 2.0 * it.relative_decrease - 1.0;   // (the cube by two multiplications — what the deciding kernel of the device-side loop computes, bit for bit)
        radius = radius / std::max(1.0 / 3.0, 1.0 - t3 * t3 * t3);
        radius = std::min(opt->max_trust_region_radius, radius); decrease_factor = 2.0; reuse_diagonal = false;
        swap_params();   // x = x_plus_delta
        if (speculate && dp.rec_alt) std::swap(dp.rec, dp.rec_alt);   // ... and its records, where the problem keeps them
        if (free_ratio) { ratio = ratio_new; dp.prior_ratio = ratio; }
        if (sv.NPF > 0) RSBA_HIP_TRY(hipMemcpyAsync(sv.trial_intr, dp.intr, 9 * (size_t)dp.NI * sizeof(double), hipMemcpyDeviceToDevice, st));   // constant coordinates stay in sync
        t0 = now_s();
        if ((rc = linearize(h, speculate, true))) return rc;
        if ((rc = gradient_max(h))) return rc;
        if ((rc = read_back())) return rc;
        sum->residual_jacobian_time_s += now_s() - t0;
        if (nfail) { push(it); (void)finish(RSBA_FAILURE); return rsba_set_error(RSBA_ERR_EVALUATION_FAILED, "residual and Jacobian evaluation failed"); }
        cost = cost2[0]; gmax = with_ratio_gradient(host_sc[kGradMax]);
        it.gradient_max_norm = gmax;
        sum->final_cost = std::min(sum->final_cost, cost + fixed);
        if (gmax <= opt->gradient_tolerance) return terminate(it, RSBA_CONVERGENCE);
      } else {
        ++sum->num_unsuccessful_steps; it.gradient_max_norm = gmax;
        radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;
      }
    }
    record(it);
    if (radius < opt->min_trust_region_radius) return finish(RSBA_CONVERGENCE);
  }
}

}  // namespace

extern "C" int32_t rsba_solve(rsba_handle* h, const rsba_solver_options* opt, rsba_solver_summary* sum, rsba_iteration* trace, int32_t trace_cap) {
  if (!h || !opt || !sum) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "null argument");
  RSBA_HIP_TRY(hipSetDevice(h->device));
  const double t_start = now_s();
  std::memset(sum, 0, sizeof *sum);
  int32_t rc = build_solver(h);
  if (rc) return rc;
  Solver* s = h->solver;
  s->solve_sw = SolveSwitches::read(Solver::kCtlRing);   // (once per solve: the loop and its steps read the fields)
  s->cov.valid = false;   // (rsba_covariance_compute: the parameters move)
  LmRun run(h, opt, sum, trace, trace_cap, t_start);
  if ((rc = run.refuse_unsupported_pcg())) return rc;
  sum->termination_type = RSBA_NO_CONVERGENCE;
  s->timer.on = opt->profile_phases != 0;
  if (s->timer.on) s->timer.reset();
  s->xtimer.on = s->timer.on && h->allreduce;
  if (s->xtimer.on) s->xtimer.reset();
  struct TimerGuard {   // whichever way this call returns, later rsba_gradient / covariance calls must not keep queueing phase records
    PhaseTimer& t; PhaseTimer& x;
    ~TimerGuard() { for (PhaseTimer* q : {&t, &x}) if (q->on) { q->on = false; q->pending.clear(); q->next = 0; } }
  } timer_guard{s->timer, s->xtimer};
  s->use_levels = opt->level_scheduled_cholesky != 0 || s->solve_sw.chol_levels;
  if ((rc = run.exchange_problem_size())) return rc;
  if ((rc = run.initial_evaluation()) || run.done) return rc;
  if (run.choose_device_loop()) { if ((rc = run.run_device_loop()) || run.done) return rc; }
  return run.run_host_loop();
}
