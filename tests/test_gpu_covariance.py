"""Row f4 of SURVEY §8f: the pose covariance blocks VideoSfMHandler::BA prints (VideoSfMHandler.cc:602-621,
ceres::Covariance on (p0,p0), (p0,p1), (p1,p1)) — the device path (one solve per unit vector through the tile
Cholesky of the undamped reduced camera system) against the oracle's dense inverse.  fp64: entries within 1e-8 of
the largest entry of the block (the systems are solved by different factorisations).

The second half of this file holds the same path to the extended-precision inverse of the whole undamped J^T J
(tests/lm_step_reference.py: covariance_blocks — nothing eliminated, one fp64 factorisation of the symmetrically scaled matrix, every
column refined against the long-double system; its own error is below 2e-3 of the unit on every case).  Unit of an entry:
u_ab = kappa^ * 2^-53 * sqrt(C_aa C_bb), kappa^ the condition number of the scaled J^T J; the ratio of a block is max |got_ab - C_ab| / u_ab
over its free coordinates, |got - got^T| is held to the same unit, fixed coordinates and the data slot of a one-pose frame must be
exactly zero.  Frames asked per case: lm_step_cases.cov_frames (first free, both sides of a tile edge, three middle tiles of a video
longer than a leaf, last, one-pose, constant / empty).

Worst ratio of the CPU oracle (Schur elimination + dense fp64 Cholesky), measured on a development host, per family (kappa^):
  frame counts and tile edges (rs_Fp1, gs_F2p1, rs_F2p1: 6.7e3 - 1.6e7) 0.36; structural edges (rs_far_pair, rs_twice, rs_dense_point,
  rs_empty_frame: 1.3e6 - 9.1e7) 0.30; masks and constant blocks (rs_const_frame, rs_const_points, rs_rotation_only: 2.1e3 - 2.8e4) 1.98
  (rs_const_points; rs_const_frame 1.85); intrinsics blocks (shared, run3, perframe, mixed, const: 2.2e7 - 2.9e9) 0.84; Huber 0.11;
  motion priors (rs_vel_r0, rs_acc_free, rs_prior_subset, rs_prior_nt, rs_free_huber: 1.2e5 - 5.3e5) 0.21; GoodPosePrior blocks
  (rs_pp_some, gs_pp_all, rs_pp_all_huber) 0.20; priors beside per-frame intrinsics 0.05; one-pose frames in a two-pose session 0.26;
  25 tiles (rs_nt25, gs_nt25) 0.13; C2 0.34.
Worst ratio of the device, per family: NOT MEASURED YET — no MI355X run of these tests has been recorded; every test below prints
its ratio ("device covariance ratio ...", run with -s), and the table belongs here.
C_COV is the smallest power of two >= 4 x the larger of the two worst ratios (the margin C_TOL = 64 has over the oracle's 18 on the
LM step): from the oracle's 1.98 alone, 8.  A device ratio above 2 raises it by that rule; one that would take it above 64 is a finding
to explain from the code or fix, not a bound to raise.  tests/test_lm_step_reference.py shows, without a GPU, that a 1e-9 relative error in one 48 x 48 tile of J^T J (7e4 x
the unit), a constant ratio, constant priorPoses blocks and a missing corrector exceed it.

rs_single_view is not in the case list but among the refusals: its single-view points have V_j of rank 2, so the undamped J^T J is
singular, like rs_F1's."""
import numpy as np
import pytest

from rsba_amd.problem import apply_gauge_masks
from rsba_amd.scene import make_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    return capi


def gauge_fixed_scene(rolling=True, huber=0.0, frames=14, points=600, seed=61, **kw):
    p = make_scene(frames, points, rolling=rolling, seed=seed, outlier_ratio=0.05 if huber else 0.0, **kw).problem
    p.huber_a = huber
    apply_gauge_masks(p, fix_first_n_cameras=1, fix_scale=False)
    p.pose_fixed_mask[-1, -1] |= 0b111000      # position of the last pose: fixes the scale, J^T J is regular
    return p


def check(capi, oracle, p, frames):
    with capi.DeviceProblem(p) as dp:
        for f in frames:
            got = dp.pose_covariance(f)
            ref, ok = oracle.pose_covariance(p, f)
            assert ok
            scale = np.abs(ref).max()
            assert scale > 0
            assert np.abs(got - ref).max() <= 1e-8 * scale, (f, np.abs(got - ref).max() / scale)
            assert np.allclose(got, got.T, rtol=0, atol=1e-9 * scale)
            # the blocks rsba prints
            pp, pe, ee = got[:6, :6], got[:6, 6:], got[6:, 6:]
            assert pp.shape == (6, 6) and (p.poses_per_frame == 1 or (pe.shape == (6, 6) and ee.shape == (6, 6)))


@pytest.mark.parametrize("rolling", [True, False])
@pytest.mark.parametrize("huber", [0.0, 2.0])
def test_covariance_blocks_match_the_oracle(capi, oracle, rolling, huber):
    p = gauge_fixed_scene(rolling=rolling, huber=huber)
    check(capi, oracle, p, [1, 5, p.num_frames - 2])


def test_fixed_coordinates_have_zero_covariance(capi, oracle):
    p = gauge_fixed_scene()
    with capi.DeviceProblem(p) as dp:
        c0 = dp.pose_covariance(0)                       # constant block (fixFirstNCameras = 1)
        cl = dp.pose_covariance(p.num_frames - 1)        # last frame: position of its second pose fixed
    assert np.all(c0 == 0)
    ref, ok = oracle.pose_covariance(p, p.num_frames - 1)
    assert ok and np.all(cl[9:, :] == 0) and np.all(cl[:, 9:] == 0) and np.abs(cl[:9, :9]).max() > 0
    assert np.abs(cl - ref).max() <= 1e-8 * np.abs(ref).max()


def test_covariance_after_a_solve_and_with_shared_intrinsics(capi, oracle):
    p = gauge_fixed_scene(frames=12, points=500, seed=62)
    p.calibrated = False
    with capi.DeviceProblem(p) as dp:
        dp.solve(capi.default_options(max_num_iterations=10))
        got = dp.pose_covariance(4)
    ref, ok = oracle.pose_covariance(p, 4)               # p holds the adjusted parameters now
    # (intrinsics in the problem make J^T J much worse conditioned: two different factorisations agree to ~3e-7 here)
    assert ok and np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max()


def test_rank_deficient_problem_is_refused(capi, oracle):
    p = make_scene(8, 200, rolling=True, seed=63).problem      # no gauge fixed at all
    with capi.DeviceProblem(p) as dp:
        with pytest.raises(capi.RsbaError):
            dp.pose_covariance(3)


@pytest.mark.parametrize("kind", [1, 2])
def test_covariance_with_the_free_inter_frame_ratio(capi, oracle, kind):
    """The reference's default with motion priors: the interFrameRatio is a free parameter block coupled to every pose, so
    ceres::Covariance inverts J^T J including its column.  The device path adds the bordered correction
    S^-1 + v v^T / (h - b.v); the constant-ratio covariance of the same scene is measurably different."""
    p = gauge_fixed_scene(frames=12, points=500, seed=64)
    p.prior_kind, p.prior_scale, p.inter_frame_ratio, p.ratio_free = kind, 9.0, 1.0, True
    p.prior_frames = np.arange(1, p.num_frames, dtype=np.int32)
    check(capi, oracle, p, [1, 6, p.num_frames - 1])
    q = p.copy(); q.ratio_free = False
    with capi.DeviceProblem(p) as dp, capi.DeviceProblem(q) as dq:
        a, b = dp.pose_covariance(6), dq.pose_covariance(6)
    assert np.abs(a - b).max() > 1e-6 * np.abs(a).max()


# ---- against the extended-precision inverse of the whole J^T J (tests/lm_step_reference.py: covariance_blocks) ---------------------

import lm_step_cases as LC                                                        # noqa: E402
import lm_step_reference as R                                                     # noqa: E402
from test_gpu_lm_step import KNOBS, _knob_id                                      # noqa: E402
from test_lm_step_reference import C_COV, covariance_reference, covariance_worst  # noqa: E402


def device_blocks(capi, p, frames):
    """({frame: block}, plan stats) of a fresh handle on p."""
    with capi.DeviceProblem(p) as dp:
        got = {f: dp.pose_covariance(f) for f in frames}
        return got, dp.plan_stats()


def check_case(capi, oracle, name):
    p, frames, ref = covariance_reference(oracle, name)
    assert ref.ok
    got, st = device_blocks(capi, p, frames)
    worst = covariance_worst(ref, got)          # (inf where a fixed coordinate, or the data slot of a one-pose frame, is not exactly zero)
    print(f"{name}: device covariance ratio {worst:.3f}, kappa^ {ref.kappa:.2e}, tiles {st['tiles']}, levels {st['levels']}")
    assert worst <= C_COV, (name, worst, ref.kappa)
    return p, frames, ref, got, st


@pytest.mark.parametrize("name", LC.COV_CASES)
def test_device_covariance_matches_the_reference(capi, oracle, name):
    p, frames, ref, got, st = check_case(capi, oracle, name)
    F, FT = p.num_frames, 48 // (6 * p.poses_per_frame)
    assert all(f in frames for f in (FT - 1, FT, F - 1) if f < F)
    assert not got[0].any()                                          # frame 0 is constant in every case
    if name in ("rs_const_frame", "rs_empty_frame"):                 # a constant / unobserved frame in mid-video
        assert FT + 1 in frames and not got[FT + 1].any()
    if p.frame_global is not None:                                   # a one-pose frame of a two-pose session: the second slot is data
        f = int(np.flatnonzero(p.frame_global)[0])
        assert got[f][:6, :6].any() and not got[f][6:, :].any() and not got[f][:, 6:].any()
    if (F + FT - 1) // FT > 8:                                       # longer than a leaf: a dissection, not a chain of tile columns
        assert st["levels"] < st["tiles"], st


@pytest.mark.parametrize("name", ["rs_far_pair", "gs_intr_run3", "rs_nt25", "rs_free_huber", "rs_pp_some"])
@pytest.mark.parametrize("knob", [k for k in KNOBS if k[0] != "RSBA_DEVICE_LM"], ids=_knob_id)
def test_plan_and_kernel_knobs_keep_the_covariance(capi, oracle, monkeypatch, knob, name):
    """Every plan / kernel knob the covariance path reads (RSBA_DEVICE_LM picks the form of the trust-region loop, which a
    covariance call never enters).  RSBA_CHOL_LEAF=2 on the 25 tiles of rs_nt25 is the deep dissection: no three consecutive tiles
    of a band fit in leaves of two, so one of the three middle tiles asked for is a separator's."""
    for kv in (knob if "=" in knob[0] else ["=".join(knob)]):
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)
    _, _, _, _, st = check_case(capi, oracle, name)
    if name == "rs_nt25" and knob[0] != "RSBA_CHOL_LEVELS":
        assert st["levels"] < st["tiles"], st


@pytest.mark.parametrize("name", LC.COV_REFUSED)
def test_rank_deficient_covariance_is_refused(capi, oracle, name):
    """No covariance where J^T J is rank deficient, as ceres::Covariance::Compute returns false:
      * free_gauge: nothing fixed, S has the 7-dimensional gauge null space — a pivot of the tile Cholesky is not positive;
      * rs_F1, rs_single_view: points seen once have V_j of rank 2.  Without damping (radius 1e300) the last pivot of the point's
        3 x 3 Cholesky is a rounding residue of either sign: where it is not positive the point factor raises the failure flag;
        where it is positive, L_j^-1 is of the order of 1 / eps and the point's share of S swamps its frame's block, whose tile
        Cholesky then fails.  Either way the call must not return numbers;
      * rs_spherical: the prior's second residual puts 1e40 s s^T (s = +-1 on the three position coordinates) on one pose.  After the
        first of them is eliminated the other two pivots are what fp64 leaves of U - 1e40 + 1e40: rounding of 1e40, either sign."""
    p = LC.cov_case(name)
    _, _, ref = covariance_reference(oracle, name)
    assert not ref.ok
    with capi.DeviceProblem(p) as dp:
        for f in LC.cov_frames(p)[:2] if name != "rs_F1" else [0]:
            with pytest.raises(capi.RsbaError):
                dp.pose_covariance(f)


def _solve_bits(s, tr, q):
    return (s.final_cost, s.num_iterations, [t.cost for t in tr], q.poses.tobytes(), q.points.tobytes(), float(q.inter_frame_ratio))


@pytest.mark.parametrize("name", ["rs_far_pair", "rs_free_huber", "rs_pp_some"])
def test_covariance_calls_leave_the_handle_as_they_found_it(capi, oracle, name):
    """On one handle: covariance of frame a, of frame b, of a again (bit-equal to the first); then a solve (bit-equal to the same
    solve on a fresh handle: costs, iterations, poses, points); then a covariance at the solved parameters, against the reference
    linearised there."""
    p, frames, ref = covariance_reference(oracle, name)
    a, b = frames[1], frames[-1]
    opts = capi.default_options(max_num_iterations=4)
    q, fresh = p.copy(), p.copy()
    with capi.DeviceProblem(q) as dp:
        c1, c2, c3 = dp.pose_covariance(a), dp.pose_covariance(b), dp.pose_covariance(a)
        assert np.array_equal(c1, c3)
        assert covariance_worst(ref, {a: c1, b: c2}) <= C_COV
        s, tr = dp.solve(opts)
        after = {f: dp.pose_covariance(f) for f in (a, b)}
    with capi.DeviceProblem(fresh) as dp:
        s0, tr0 = dp.solve(opts)
    assert _solve_bits(s, tr, q) == _solve_bits(s0, tr0, fresh)
    assert s.num_iterations > 1 and not np.array_equal(q.poses, p.poses)
    r, J, ok = oracle.evaluate_blocks(q)
    assert ok.all()
    ref1 = R.covariance_blocks(q, r, J, [a, b])
    worst = covariance_worst(ref1, after)
    print(f"{name}: covariance after a solve, ratio {worst:.3f}, kappa^ {ref1.kappa:.2e}")
    assert ref1.ok and worst <= C_COV, worst


def test_a_lost_entry_of_a_covariance_solve_is_redone_on_the_level_schedule(capi, oracle, tmp_path):
    """RSBA_CHOL_TEST_CORRUPT=1 (instrumented library): the first persistent-driver solve of the handle — column 0 of the asked block —
    loses entry (n / 2 / 6) * 6 + 1 of its result, which lies inside the block of the frame asked for: uncaught, entry (1, 0) of the
    block would be exactly zero.  The sticky verification flag must notice, the CD solves are repeated on the level schedule inside
    the call, the block is the level schedule's bit for bit and within the bound of the reference; a later solve on the handle runs
    and ends where it ends on an untouched handle."""
    from test_gpu_solve import run_hook_case
    out = run_hook_case("corrupt_covariance", tmp_path)
    p, _, _ = covariance_reference(oracle, "C2")
    f = out["frame"]
    assert f == 50 and out["entry"] == 1 and p.num_frames * 12 == 1200                   # entry 601 of the 1200 camera unknowns
    blk = {m: np.array(out[m]["cov"]) for m in ("corrupt", "levels", "plain")}
    assert np.array_equal(blk["corrupt"], blk["levels"])
    assert blk["corrupt"][1, 0] != 0.0                                                   # the lost entry did not reach the block
    # the switch arms ONE loss per handle: the solve after the covariance call found it spent (tests/test_gpu_solve.py shows that a
    # solve that meets it reports one fallback), so the covariance call is where the entry was lost — and redone
    assert all(out[m]["solve_fallbacks"] == 0 for m in blk)
    assert out["corrupt"]["final_cost"] == out["plain"]["final_cost"] and out["corrupt"]["iters"] == out["plain"]["iters"]
    r, J, ok = oracle.evaluate_blocks(p)
    ref = R.covariance_blocks(p, r, J, [f])
    for m in blk:
        assert covariance_worst(ref, {f: blk[m]}) <= C_COV, m
