"""rsba_covariance_compute and its getters: the covariance blocks of every frame, of pairs of frames, of points and of the intrinsics
blocks from ONE selected inverse of the reduced camera system on the device (kernels_selinv.hip), against the extended-precision inverse
of the whole J^T J (tests/cov_reference.py: full_covariance, nothing eliminated).

Per case (the cases, pairs, points and references of tests/test_cov_reference.py, computed once a session): every (f, f) block, the
(f, f + 1) and (f + 1, f) blocks of adjacent frames, one co-visible pair that is not adjacent, every intrinsics block, and the block of
every point (gs_intr_perframe: 64 sampled points; rs_nt25: 64 sampled points and 64 of those across the top separator).  Unit of an entry: u_ab = kappa^ * 2^-53 * sqrt(C_aa C_bb); a block's ratio is
max |got_ab - C_ab| / u_ab over its unknowns, the asymmetry of a diagonal block is held to the same unit, and rows and columns that are
no unknowns (fixed coordinates, the data slot of a one-pose frame, constant blocks, constant points) must be exactly zero.  Every (f, f)
block asked is also within 2 C_COVP units of rsba_pose_covariance(f) on the same handle (two routes through one factorisation, each
within C_COVP of the truth).

C_COVP comes from tests/test_cov_reference.py: derived from the fp64 restatement of the algorithm on the host, not from the device.
A device ratio above it is a finding to explain from the code, not a bound to raise.  What the device reached is in
profiles/cov/README.md; every test prints its ratios ("device covariance blocks ...", run with -s).

The cases: rs_Fp1 two tiles; gs_F2p1 CD = 6 and padding rows; rs_far_pair a tile far off the band; rs_intr_shared, gs_intr_perframe
intrinsics blocks (with CD = 6 a block crosses a tile edge: two pseudo frames; per-frame blocks: the records kept, virtual records);
rs_acc_free the border column of a free interFrameRatio; rs_pp_some priorPoses blocks; rs_scanline a one-pose frame in a two-pose
session; rs_const_points, rs_const_frame exact zeros; rs_nt25 under RSBA_CHOL_LEAF=2 a dissection with fill and separators."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_reference as CR                                      # noqa: E402
import lm_step_cases as LC                                      # noqa: E402
import test_cov_reference as TR                                 # noqa: E402
from helpers import HOOKS_LIB                                   # noqa: E402
from test_cov_reference import C_COVP, CASES, pairs_of          # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = [("RSBA_CHOL_LEVELS=1",), ("RSBA_CHOL_LEAF=2",), ("RSBA_CHOL_CHUNK=1", "RSBA_CHOL_TAIL=1"), ("RSBA_RECORDS=1",)]


@pytest.fixture(scope="module")
def hooks():
    return C.CDLL(HOOKS_LIB)                                     # (the instrumented library: the plan of the reference's point sample)


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    return capi


_ref_cache = {}


def reference(oracle, hooks, name, p=None, key=None):
    """(problem, pairs, points, intrinsics blocks, reference): the session's reference of the case (tests/test_cov_reference.py), or, for
    a problem p of the caller's (the case after a solve), one of its own with every 7th point."""
    if p is None:
        p, _, _, pairs, points, intr, ref, _ = TR.case_of(name, oracle, hooks, sample_across=64)
        return p, pairs, points, intr, ref
    if key not in _ref_cache:
        r, J, ok = oracle.evaluate_blocks(p)
        assert ok.all()
        intr = [] if p.calibrated else list(range(p.num_intrinsics))
        pairs, points = pairs_of(p), list(range(0, p.num_points, 7))
        _ref_cache[key] = (p, pairs, points, intr, CR.full_covariance(p, r, J, pairs, points, intr))
    return _ref_cache[key]


def device_blocks(dp, pairs, points, intr):
    dp.covariance_compute()
    got = dp.covariance_frame_blocks(pairs)
    allp = len(points) == dp.prob.num_points
    pb = dp.covariance_point_blocks(None if allp else points)
    return ({q: got[k] for k, q in enumerate(pairs)}, {c: dp.covariance_intrinsics_block(c) for c in intr},
            {int(j): pb[k] for k, j in enumerate(points)})


def check_blocks(name, ref, fb, ib, pb, bound=C_COVP):
    w = TR.worst_ratios(ref, fb, ib, pb)
    print(f"{name}: device covariance blocks, worst ratio (f, f) {w['diag']:.3f}, (f, g) {w['cross']:.3f}, intrinsics {w['intr']:.3f}, "
          f"points {w['point']:.3f} ({len(pb)}), asymmetry {w['asym']:.3f}, kappa^ {ref.kappa:.2e}, reference error {ref.error:.1e}")
    assert max(w.values()) <= bound, (name, w, ref.kappa)
    for (a, b), blk in fb.items():
        if a > b:
            assert np.array_equal(blk, fb[(b, a)].T), (a, b)                # the transpose of (b, a), bit for bit


@pytest.mark.parametrize("name", CASES)
def test_blocks_match_the_reference(capi, oracle, hooks, monkeypatch, name):
    p, pairs, points, intr, ref = reference(oracle, hooks, name)
    if name in TR.LEAF:
        monkeypatch.setenv("RSBA_CHOL_LEAF", TR.LEAF[name])
    assert ref.ok
    F, CD = p.num_frames, 6 * p.poses_per_frame
    with capi.DeviceProblem(p) as dp:
        fb, ib, pb = device_blocks(dp, pairs, points, intr)
        mem = dp.covariance_memory()
        one = {f: dp.pose_covariance(f) for f in sorted({a for a, b in pairs if a == b})}   # every (f, f) block asked
        assert np.array_equal(dp.covariance_point_blocks(points[:3]), np.stack([pb[j] for j in points[:3]]))   # pose_covariance leaves the getters alone
        st = dp.plan_stats()
        dp.covariance_release()
        assert 0 < dp.covariance_memory() < mem and mem >= 2 * st["factor_tiles"] * 48 * 48 * 8
    check_blocks(name, ref, fb, ib, pb)
    assert any(blk.any() for blk in pb.values())
    if p.point_constant is not None and p.point_constant.any():
        const = [j for j in points if p.point_constant[j]]
        assert const and all(not pb[j].any() for j in const)
    # exact zeros: frame 0 is constant in every case, the last pose's position is fixed
    assert not fb[(0, 0)].any() and not fb[(0, 1)].any() and not fb[(1, 0)].any()
    assert any(not m.all() and m.any() for g, m in ref.free.items() if g[0] == "f")
    if name == "rs_const_frame":
        FT = 48 // CD
        assert not fb[(FT + 1, FT + 1)].any() and not fb[(FT, FT + 1)].any()
    if p.frame_global is not None:
        f = int(np.flatnonzero(p.frame_global)[0])
        assert fb[(f, f)][:6, :6].any() and not fb[(f, f)][6:, :].any() and not fb[(f, f)][:, 6:].any()
    if intr:
        assert all(ib[c].any() for c in intr)
    if name == "rs_nt25":
        assert st["levels"] < st["tiles"], st
    # against the one-block path on the same handle
    for f, blk in one.items():
        g = ("f", f)
        assert CR.block_ratio(ref, g, g, np.asarray(blk, dtype=np.longdouble), fb[(f, f)]) <= 2 * C_COVP, f


@pytest.mark.parametrize("name", ["rs_nt25", "rs_far_pair"])
@pytest.mark.parametrize("knob", KNOBS, ids="+".join)
def test_plan_and_kernel_knobs_keep_the_blocks(capi, oracle, hooks, monkeypatch, knob, name):
    p, pairs, points, intr, ref = reference(oracle, hooks, name)
    for kv in knob:
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)
    with capi.DeviceProblem(p) as dp:
        fb, ib, pb = device_blocks(dp, pairs, points, intr)
        fb2, _, pb2 = device_blocks(dp, pairs, points, intr)
    check_blocks(f"{name} {'+'.join(knob)}", ref, fb, ib, pb)
    assert all(np.array_equal(fb[q], fb2[q]) for q in pairs) and all(np.array_equal(pb[j], pb2[j]) for j in points), "two computes on one handle differ"


@pytest.mark.parametrize("name", LC.COV_REFUSED)
def test_rank_deficient_problems_are_refused(capi, name):
    p = LC.cov_case(name)
    with capi.DeviceProblem(p) as dp:
        with pytest.raises(capi.RsbaError):
            dp.covariance_compute()
        with pytest.raises(capi.RsbaError, match="no covariance computed"):
            dp.covariance_frame_blocks([(0, 0)])
        with pytest.raises(capi.RsbaError, match="no covariance computed"):
            dp.covariance_point_blocks([0])


def test_getters_refuse_without_a_computed_covariance(capi, monkeypatch):
    monkeypatch.delenv("RSBA_CHOL_LEAF", raising=False)
    p = LC.cov_case("rs_nt25").copy()
    F = p.num_frames
    with capi.DeviceProblem(p) as dp:
        def refused():
            with pytest.raises(capi.RsbaError, match="no covariance computed") as e:
                dp.covariance_frame_blocks([(1, 1)])
            assert e.value.status == 1                                      # RSBA_ERR_INVALID_ARGUMENT
            with pytest.raises(capi.RsbaError, match="no covariance computed"):
                dp.covariance_point_blocks([0])
        refused()                                                           # before the first compute
        dp.covariance_compute()
        a = dp.covariance_frame_blocks([(1, 1)])
        # 25 tiles are more than a leaf of the dissection: tiles 1 and 23 lie in different parts of the elimination tree and no point
        # links them, so the factor has no tile for frames 4 and F - 5 — refused by name, and the handle and the computed covariance
        # stay usable
        with pytest.raises(capi.RsbaError, match=f"frames 4 and {F - 5} ") as e:
            dp.covariance_frame_blocks([(1, 1), (4, F - 5)])
        assert e.value.status == 6                                          # RSBA_ERR_UNSUPPORTED
        with pytest.raises(capi.RsbaError, match="out of range"):
            dp.covariance_frame_blocks([(1, F)])
        with pytest.raises(capi.RsbaError, match="out of range"):
            dp.covariance_point_blocks([p.num_points])
        assert np.array_equal(a, dp.covariance_frame_blocks([(1, 1)]))
        with pytest.raises(capi.RsbaError):
            dp.covariance_intrinsics_block(0)                               # a calibrated problem has none
        dp.solve(capi.default_options(max_num_iterations=1))
        refused()                                                           # after a solve
        dp.covariance_compute()
        dp.covariance_frame_blocks([(1, 1)])
        dp.upload_parameters()
        refused()                                                           # after new parameters
        dp.covariance_compute()
        dp.covariance_release()
        refused()                                                           # after the release
        dp.covariance_compute()                                             # ... and a compute after it allocates again
        assert dp.covariance_frame_blocks([(1, 1)]).any()


def test_a_handle_with_an_exchange_is_refused(capi):
    from rsba_amd.distributed import ALLREDUCE_FN
    p = LC.cov_case("rs_Fp1")
    fn = ALLREDUCE_FN(lambda _ctx, _ptr, _count, _op, _stream: 0)           # one rank: the identity
    with capi.DeviceProblem(p) as dp:
        capi._check(capi.lib().rsba_set_exchange(dp._h, fn, None, C.c_int32(0), C.c_int32(1)))
        with pytest.raises(capi.RsbaError, match="exchange") as e:
            dp.covariance_compute()
        assert e.value.status == 6                                          # RSBA_ERR_UNSUPPORTED


def _solve_bits(s, tr, q):
    return (s.final_cost, s.num_iterations, [t.cost for t in tr], q.poses.tobytes(), q.points.tobytes(), float(q.inter_frame_ratio))


@pytest.mark.parametrize("name", ["rs_far_pair", "rs_acc_free"])
def test_the_calls_leave_the_handle_as_they_found_it(capi, oracle, hooks, name):
    """pose_covariance before and after a compute: bit-equal.  Compute, getters, then a 4-iteration solve: bit-equal to the solve on a
    fresh handle.  Then compute and the getters at the solved parameters, against the reference linearised there."""
    p, pairs, points, intr, ref = reference(oracle, hooks, name)
    opts = capi.default_options(max_num_iterations=4)
    q, fresh = p.copy(), p.copy()
    with capi.DeviceProblem(q) as dp:
        c0 = dp.pose_covariance(1)
        fb, ib, pb = device_blocks(dp, pairs, points, intr)
        assert np.array_equal(c0, dp.pose_covariance(1))
        check_blocks(name, ref, fb, ib, pb)
        s, tr = dp.solve(opts)
        points1 = list(range(0, p.num_points, 7))
        fb1, ib1, pb1 = device_blocks(dp, pairs, points1, intr)
        c1 = dp.pose_covariance(1)
    with capi.DeviceProblem(fresh) as dp:
        s0, tr0 = dp.solve(opts)
        c1_fresh = dp.pose_covariance(1)
    assert _solve_bits(s, tr, q) == _solve_bits(s0, tr0, fresh)
    assert np.array_equal(c1, c1_fresh)
    assert s.num_iterations > 1 and not np.array_equal(q.poses, p.poses)
    _, _, pts1, _, ref1 = reference(oracle, hooks, name, p=q, key=name + " solved")
    assert ref1.ok and pts1 == points1
    check_blocks(name + " after a solve", ref1, fb1, ib1, pb1)


def test_the_facade_serves_two_frame_point_and_intrinsics_blocks(capi, tmp_path):
    """examples/covariance_blocks: ceres::Covariance on the pose pairs of ONE frame keeps its path (rsba_pose_covariance: the blocks of
    the Python binding's pose_covariance, bit for bit); a request with pose pairs of two frames and the intrinsics block goes through one
    rsba_covariance_compute and gives the Python getters' blocks bit for bit, the block of a point among them, and (B, A), which was not
    asked for, as the transpose of (A, B); a pose against a point is still refused."""
    import subprocess
    from helpers import write_scene_file
    from rsba_amd.problem import apply_gauge_masks
    from rsba_amd.scene import make_scene
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "covariance_blocks")
    p = make_scene(10, 400, rolling=True, seed=44).problem
    p.calibrated = False
    A, B, CD = 3, 7, 12
    write_scene_file(tmp_path / "s.bin", p, fix_first_n=1, fix_scale=True)
    r = subprocess.run([exe, str(tmp_path / "s.bin"), str(tmp_path / "o.bin"), str(A), str(B)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(tmp_path / "o.bin", dtype="<f8")
    assert list(raw[:3]) == [1.0, 1.0, 0.0], r.stdout
    same1, same2, cross = (raw[3 + k * CD * CD: 3 + (k + 1) * CD * CD].reshape(CD, CD) for k in range(3))
    intr = raw[3 + 3 * CD * CD: 3 + 3 * CD * CD + 81].reshape(9, 9)
    rest = raw[3 + 3 * CD * CD + 81:]
    track, point, back = int(rest[0]), rest[1:10].reshape(3, 3), rest[10:].reshape(CD, CD)
    apply_gauge_masks(p, fix_first_n_cameras=1, fix_scale=True)
    with capi.DeviceProblem(p) as dp:
        one = dp.pose_covariance(A)
        dp.covariance_compute()
        got = dp.covariance_frame_blocks([(A, A), (A, B)])
        gi = dp.covariance_intrinsics_block(0)
        gp = dp.covariance_point_blocks([track])[0]
    upper = np.kron(np.triu(np.ones((2, 2))), np.ones((6, 6))).astype(bool)      # the 6 x 6 blocks the request names: (p0,p0), (p0,p1), (p1,p1)
    assert np.array_equal(same1[upper], one[upper]) and one.any()
    assert np.array_equal(same2, got[0]) and np.array_equal(cross, got[1]) and np.array_equal(intr, gi)
    assert track >= 0 and np.array_equal(point, gp) and point.any() and np.array_equal(point, point.T)
    assert np.array_equal(back, cross.T)
    assert cross.any() and intr.any()
