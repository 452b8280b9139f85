"""The minimal solver of the global-shutter RANSAC on the device (rsba_pnp_p3p, rsba_pnp_gs_hypotheses_p3p) against the extended-precision
reference of tests/p3p_reference.py, on the case list test_p3p_reference.py fixes, and the third attempt of new_frame.hpp's solveRsPnP.

The bound: tests/golden/p3p_bound.json records the host fp64 p3p_pose's worst |pose_k - reference_k| / unit_k over these cases (half_turn and
sliver apart: tests/golden/make_p3p_bound.py says why); the kernel restates the same arithmetic in another operation order, so it gets that
figure times 4.  Nothing here comes from device output."""
import ctypes as C

import numpy as np
import pytest

import p3p_reference as R
from helpers import build_host_program, load_golden
from rsba_amd.problem import GLOBAL
from test_gpu_new_frame import F, Sess, exe, run  # noqa: F401  (exe: the fixture that builds examples/new_frame)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    return capi


def device_bound(name):
    rec = load_golden("p3p_bound.json")
    return rec["host_worst_error_" + name if name in ("half_turn", "sliver") else "host_worst_error"] * rec["device_factor"]


@pytest.mark.parametrize("name", list(R.cases()))
def test_p3p_matches_the_extended_precision_reference(capi, name):
    """status and num_solutions = the reference's for every subset; accepted poses within the bound; declined slots untouched; two calls
    agree bit for bit.  main_*: 24 points, 65 subsets (a full wave and one lane); single: num_tasks = 1, n = 4."""
    c, ref = R.cases()[name], R.reference(name)
    T = len(c["subsets"])
    poses = np.full((T, 6), SENTINEL)
    out = capi.pnp_p3p(c["cam"], c["X"], c["xy"], c["subsets"], poses_out=poses)
    assert list(out["status"]) == [r["status"] for r in ref]
    assert list(out["num_solutions"]) == [r["num_solutions"] for r in ref]
    for t, r in enumerate(ref):
        if r["status"] == 0:
            assert np.all(poses[t] == SENTINEL), (name, t)
    bound, worst = device_bound(name), R.worst_error(ref, out["status"], poses)
    print(f"{name}: device worst |pose - reference| in units = {worst:.4g} (bound {bound:.4g})")
    assert worst <= bound, (name, worst, bound)
    again = capi.pnp_p3p(c["cam"], c["X"], c["xy"], c["subsets"], poses_out=np.full((T, 6), SENTINEL))
    assert np.array_equal(again["status"], out["status"]) and np.array_equal(again["num_solutions"], out["num_solutions"]) and again["poses"].tobytes() == poses.tobytes()


def test_results_do_not_depend_on_where_a_subset_sits_in_the_launch(capi):
    """the 65 subsets reversed and repeated (195 tasks, four workgroups): every copy gives the bytes of the first call"""
    c = R.cases()["main_distorted"]
    base = capi.pnp_p3p(c["cam"], c["X"], c["xy"], c["subsets"])
    subs = np.concatenate([c["subsets"][::-1], c["subsets"], c["subsets"][::-1]])
    out = capi.pnp_p3p(c["cam"], c["X"], c["xy"], subs)
    for lo, order in ((0, slice(None, None, -1)), (65, slice(None)), (130, slice(None, None, -1))):
        assert np.ascontiguousarray(out["poses"][lo:lo + 65]).tobytes() == np.ascontiguousarray(base["poses"][order]).tobytes()
        assert np.array_equal(out["status"][lo:lo + 65], base["status"][order]) and np.array_equal(out["num_solutions"][lo:lo + 65], base["num_solutions"][order])


def test_gs_hypotheses_p3p_equal_the_two_step_form(capi, oracle, tmp_path):
    """rsba_pnp_gs_hypotheses_p3p against host p3p_pose starts -> rsba_pnp_tasks(GLOBAL, 5 iterations, m = 4) over the accepted subsets.
    Same statuses, same winner, inlier counts within one borderline point, the winner's pose within 1e-6: the tolerances of
    test_gpu_pnp_dlt.py::test_gs_hypotheses_equal_the_two_step_form for the same comparison."""
    from test_gpu_pnp import CAM, pnp_scene, random_subsets
    sc = pnp_scene(oracle, GLOBAL, n=220, outliers=0.3, seed=8)
    subs = random_subsets(np.random.default_rng(4), len(sc["X"]), 60, 4)
    subs[7] = subs[7][[0, 1, 2, 0]]                              # one degenerate subset: declined by both
    err = 6.0
    ok, _, starts = R.run_host(build_host_program("p3p_host", tmp_path), tmp_path, [dict(cam=CAM, X=sc["X"], xy=sc["xy"], subsets=subs)])[0]
    acc = np.flatnonzero(ok)
    two = capi.pnp_tasks(CAM, GLOBAL, sc["scan"], sc["X"], sc["xy"], subs[acc], np.concatenate([starts[acc], starts[acc]], axis=1),
                         max_num_iterations=5, reprojection_error=err, drop_coincident=False)
    status2 = np.zeros(60, dtype=np.uint8); status2[acc] = two["status"]
    count2 = np.zeros(60, dtype=np.int32); count2[acc] = two["num_inliers"]
    one = capi.pnp_gs_hypotheses_p3p(CAM, sc["X"], sc["xy"], subs, max_num_iterations=5, reprojection_error=err)
    assert one["status"][7] == 0 and ok[7] == 0
    assert np.array_equal(one["status"], status2)
    usable = np.flatnonzero(status2)
    w1 = usable[np.argmax(one["num_inliers"][usable])]; w2 = usable[np.argmax(count2[usable])]
    assert w1 == w2
    assert np.max(np.abs(one["num_inliers"].astype(int) - count2)) <= 1
    p1, p2 = one["poses"][w1], two["poses"][list(acc).index(w2), 0]
    assert np.max(np.abs(p1 - p2)) <= 1e-6
    assert one["num_inliers"][7] == 0 and one["final_cost"][7] == 0 and np.all(one["poses"][7] == 0)
    again = capi.pnp_gs_hypotheses_p3p(CAM, sc["X"], sc["xy"], subs, max_num_iterations=5, reprojection_error=err)
    assert again["poses"].tobytes() == one["poses"].tobytes() and np.array_equal(again["num_inliers"], one["num_inliers"])


def test_sixty_percent_outliers(capi, oracle):
    """200 points, 60 % outliers, 500 four-point subsets: about 500 * 0.4^4 = 13 are clean (none: (1 - 0.0256)^500 < 1e-5), and the winner
    holds at least 0.8 of the true inliers"""
    from test_gpu_pnp import CAM, pnp_scene, random_subsets
    sc = pnp_scene(oracle, GLOBAL, n=200, outliers=0.6, seed=12)
    subs = random_subsets(np.random.default_rng(6), len(sc["X"]), 500, 4)
    out = capi.pnp_gs_hypotheses_p3p(CAM, sc["X"], sc["xy"], subs, max_num_iterations=5, reprojection_error=6.0)
    usable = np.flatnonzero(out["status"])
    best = usable[np.argmax(out["num_inliers"][usable])]
    true_inliers = int((~sc["outlier"]).sum())
    clean = int(sum(not sc["outlier"][s].any() for s in subs))
    print(f"true inliers {true_inliers}, clean subsets {clean}, winner {best} with {out['num_inliers'][best]} inliers")
    assert out["num_inliers"][best] >= 0.8 * true_inliers
    assert np.max(np.abs(out["poses"][best] - sc["poses"][0])) <= 0.05       # the tolerance of the PnP tests on scenes with this noise


def test_the_example_program_runs_the_p3p_ransac(capi, oracle, tmp_path):
    """examples/pnp_ransac in its p3p mode (solveGsPnPRansacP3P, subsets from the restated cv::RNG) on the scene with 60 % outliers: the
    winner holds at least 0.8 of the true inliers, and the pose it writes has that many inliers when rsba_pnp_inliers counts them (one
    borderline point may move: the pose went through rvec / tvec and back).  The winner was refined on its own four points only, so its
    pose is as good as four observations with 0.4 px of noise make it: the inliers are the check, not a distance to the true pose."""
    import os
    import struct
    import subprocess
    from test_gpu_pnp import CAM, pnp_scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = os.path.join(root, "examples", "pnp_ransac")
    if not os.path.exists(prog):
        import __graft_entry__ as G
        G.build()
    sc = pnp_scene(oracle, GLOBAL, n=200, outliers=0.6, seed=12)
    with open(tmp_path / "problem.bin", "wb") as f:
        f.write(struct.pack("<7ifQ", len(sc["X"]), int(GLOBAL), 0, 1, 500, 0, 4, 6.0, 0x9e3779b97f4a7c15)); f.write(np.asarray(CAM, dtype="<f8").tobytes())
        f.write(np.zeros(12, dtype="<f8").tobytes()); f.write(sc["X"].astype("<f4").tobytes()); f.write(sc["xy"].astype("<f4").tobytes())
    r = subprocess.run([prog, str(tmp_path / "problem.bin"), str(tmp_path / "out.bin"), "p3p"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    buf = (tmp_path / "out.bin").read_bytes()
    assert len(buf) == 12 * 8 + 4
    v = np.frombuffer(buf[:96]); count = struct.unpack("<i", buf[96:])[0]
    assert count >= 0.8 * int((~sc["outlier"]).sum())
    rot = R._rodrigues(v[:3])
    pose = np.concatenate([v[:3], -rot.T @ v[3:6]])                           # rvec / tvec -> rsba's (angle-axis, camera centre)
    mask = capi.pnp_inliers(CAM, GLOBAL, sc["scan"], sc["X"], sc["xy"], np.concatenate([pose, pose]), 6.0)
    print(f"the example's winner: {count} inliers, recounted {mask.sum()}, distance to the true pose {np.max(np.abs(pose - sc['poses'][0])):.3g}")
    assert abs(int(mask.sum()) - count) <= 1 and np.array_equal(v[:6], v[6:])


def test_a_frame_with_five_correspondences_is_localised(exe, oracle, tmp_path):  # noqa: F811
    """a global-shutter session whose last frame reaches exactly five 3-D points: the extrinsic-guess attempt and the DLT attempt need six, the
    minimal-solver attempt localises it (minReprojections above the frame's key keeps the direct PnP, which would write poses of its own,
    out of it) and all five points reproject within the RANSAC threshold 2 sqrt(sqrdThreshold) = 8 px"""
    s = Sess(rolling=False)
    assert s.rs == GLOBAL
    linked = []
    for o in s.frames[F - 1]["obs"]:
        tracks = [s.frames[pf]["obs"][pk]["track"] for pf, pk, _ in o["matches"]]
        tracks = [t for t in tracks if t is not None]
        if tracks:
            if len(linked) < 5:
                linked.append((o, tracks[0]))
            else:
                o["matches"] = []
    assert len(linked) == 5
    got = run(exe, tmp_path, s, "solveGsPnP=1", "solveRsPnP=0", "reuseLastPose=0", "minReprojections=100")
    rep = got["report"][0]
    assert rep["key"] == F - 1 and rep["localised"] == 1 and len(got["poses"][F - 1]) == 1
    for o, t in linked:
        ok, p = oracle.reproject(s.cam, np.array(got["poses"][F - 1]), s.rs, s.scan, np.array(s.tracks[t]["pt"]), 1e12)
        assert ok and np.hypot(p[0] - o["x"], p[1] - o["y"]) < 8.0, (t, p, o["x"], o["y"])


def test_bad_arguments_are_errors_and_leave_the_outputs_untouched(capi):
    lib = capi.lib()
    cam = np.ascontiguousarray(R.CAM_DIST); X = np.zeros((8, 3), dtype=np.float32); xy = np.zeros((8, 2), dtype=np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def both(n, sub, T, cam_=cam, X_=X, null_out=False, device=0):
        poses = np.full((max(T, 1), 6), SENTINEL); status = np.full(max(T, 1), 77, dtype=np.uint8); nsol = np.full(max(T, 1), 77, dtype=np.int32)
        cost = np.full(max(T, 1), SENTINEL); inl = np.full(max(T, 1), 77, dtype=np.int32)
        a = lib.rsba_pnp_p3p(C.c_int32(device), ptr(cam_), ptr(X_), ptr(xy), C.c_int32(n), ptr(sub), C.c_int32(T), None if null_out else ptr(poses), ptr(status), ptr(nsol))
        b = lib.rsba_pnp_gs_hypotheses_p3p(C.c_int32(device), ptr(cam_), ptr(X_), ptr(xy), C.c_int32(n), ptr(sub), C.c_int32(T), C.c_int32(5), C.c_float(3.0),
                                           None if null_out else ptr(poses), ptr(status), ptr(cost), ptr(inl))
        assert np.all(poses == SENTINEL) and np.all(status == 77) and np.all(nsol == 77) and np.all(cost == SENTINEL) and np.all(inl == 77)
        return a, b

    def dlt(n, sub, m, T, cam_=cam, X_=X, null_out=False, device=0):
        """the code the DLT call returns for the same mistake"""
        poses = np.zeros((max(T, 1), 6)); status = np.zeros(max(T, 1), dtype=np.uint8)
        return lib.rsba_pnp_dlt(C.c_int32(device), ptr(cam_), ptr(X_), ptr(xy), C.c_int32(n), ptr(sub), C.c_int32(m), C.c_int32(T), None if null_out else ptr(poses), ptr(status))

    four = np.arange(4, dtype=np.int32)[None, :]; six = np.arange(6, dtype=np.int32)[None, :]
    code = dlt(8, six, 6, 0)
    assert code != 0
    assert both(3, np.array([[0, 1, 2, 0]], dtype=np.int32), 1) == (dlt(5, six, 6, 1),) * 2 == (code, code)                 # n < 4 | n < m
    assert both(8, np.array([[0, 1, 2, 8]], dtype=np.int32), 1) == (dlt(8, np.array([[0, 1, 2, 3, 4, 8]], dtype=np.int32), 6, 1),) * 2 == (code, code)   # index out of range
    assert both(8, np.array([[0, 1, 2, -1]], dtype=np.int32), 1) == (code, code)
    assert both(8, four, 0) == (dlt(8, six, 6, 0),) * 2                                                                     # no tasks
    assert both(8, four, -3) == (code, code)
    assert both(8, None, 1) == (dlt(8, None, 6, 1),) * 2 == (code, code)                                                    # null pointers
    assert both(8, four, 1, cam_=None) == (dlt(8, six, 6, 1, cam_=None),) * 2 == (code, code)
    assert both(8, four, 1, X_=None) == (dlt(8, six, 6, 1, X_=None),) * 2 == (code, code)
    assert both(8, four, 1, null_out=True) == (dlt(8, six, 6, 1, null_out=True),) * 2 == (code, code)
    bad_device = dlt(8, six, 6, 1, device=99)                                                                               # no such device
    assert bad_device != 0 and both(8, four, 1, device=99) == (bad_device, bad_device)
    # num_solutions may be NULL
    poses = np.zeros((1, 6)); status = np.zeros(1, dtype=np.uint8)
    c = R.cases()["single"]
    assert lib.rsba_pnp_p3p(C.c_int32(0), ptr(np.ascontiguousarray(c["cam"])), ptr(c["X"]), ptr(c["xy"]), C.c_int32(4), ptr(c["subsets"]), C.c_int32(1), ptr(poses), ptr(status), None) == 0
    assert status[0] == 1
    with pytest.raises(capi.RsbaError):
        capi.pnp_p3p(cam, X, xy, np.array([[0, 1, 2, 8]], dtype=np.int32))
