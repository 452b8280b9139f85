"""The five-point solver on the device (rsba_epipolar_five_point, rsba_epipolar_hypotheses_five_point, findEssentialRansac and
initializeTwoView with TwoViewOptions::solver = FivePoint through examples/two_view) against the extended-precision reference of
tests/five_point_reference.py and the host definitions of include/rsba/two_view.hpp (tests/five_point_host.cpp), on the case list, the
outlier scenes and the planar scene test_five_point_reference.py fixes.

The bound: tests/golden/five_point_bound.json records the host fp64 code's worst error in the reference's units over the cases; the kernel
restates the same arithmetic, so it gets that figure times 4 — and, on every case but sideways_no_rotation (whose vanishing units set the
first figure, see make_five_point_bound.py), the general figure times 4 as well.  Nothing here comes from device output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import five_point_reference as F
import two_view_reference as R
from helpers import build_host_program, load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.678
FB = 4


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    return capi


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as G
    path = os.path.join(ROOT, "examples", "two_view")
    if not os.path.exists(path):
        G.build()
    return path


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("five_point_gpu")
    return build_host_program("five_point_host", d), d


@pytest.fixture(scope="module")
def scoring(host):
    """the frames (0, 4) global-shutter outlier scene, the first 64 five-point subsets of the RANSAC and what the host chain makes of them"""
    exe_host, d = host
    s = R.outlier_scene(FB, False)
    subsets = F.distinct_subsets(len(s["xy_a"]), 5, 64, R.RANSAC["rng_state"])
    return s, subsets, F.run_host_hypotheses(exe_host, d, s, 64)


@pytest.mark.parametrize("name", list(F.cases()))
def test_five_point_matches_the_extended_precision_reference(capi, name):
    """status and count = the reference's for every subset; every solution (up to sign) and the pose the chain makes of the chosen one
    within the bound; declined tasks and the slots past the count untouched; two calls agree bit for bit.  main_*: 65 subsets."""
    c, ref = F.cases()[name], F.reference(name)
    args = (c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"])
    n_tasks = len(c["subsets"])
    E = np.full((n_tasks, 10, 9), SENTINEL)
    out = capi.epipolar_five_point(*args, c["subsets"], E_out=E)
    assert list(out["status"]) == [r["status"] for r in ref]
    assert list(out["num_solutions"]) == [len(r["E"]) for r in ref]
    E1 = np.full((n_tasks, 9), SENTINEL); poses = np.full((n_tasks, 6), SENTINEL)
    chain = capi.epipolar_hypotheses_five_point(*args, c["subsets"], threshold_px=F.THRESHOLD_PX, E_out=E1, poses_out=poses)
    assert list(chain["status"]) == [r["status"] for r in ref] and np.array_equal(chain["num_solutions"], out["num_solutions"])
    for t, r in enumerate(ref):
        assert np.all(E[t, len(r["E"]):] == SENTINEL), (name, t)
        if r["status"] == 0:
            assert np.all(E1[t] == SENTINEL) and np.all(poses[t] == SENTINEL) and chain["num_inliers"][t] == 0 and not chain["num_front"][t].any(), (name, t)
        else:
            assert E1[t].tobytes() == E[t, r["chosen"]].tobytes(), (name, t)
    rec = load_golden("five_point_bound.json")
    bound = rec["device_factor"] * rec["host_worst_error"]
    general = rec["device_factor"] * rec["host_worst_error_general"]
    worst = F.worst_error(ref, out["status"], out["num_solutions"], E, poses)
    print(f"{name}: device worst |value - reference| in units = {worst:.4g} (bound {bound:.4g}, general {general:.4g})")
    assert worst <= bound, (name, worst, bound)
    assert name == "sideways_no_rotation" or worst <= general, (name, worst, general)
    again = capi.epipolar_five_point(*args, c["subsets"], E_out=np.full((n_tasks, 10, 9), SENTINEL))
    assert np.array_equal(again["status"], out["status"]) and np.array_equal(again["num_solutions"], out["num_solutions"]) and again["E"].tobytes() == E.tobytes()


def test_results_do_not_depend_on_where_a_subset_sits_in_the_launch(capi):
    """the 65 subsets reversed and repeated (195 tasks, several workgroups): every copy gives the bytes of the first call"""
    c = F.cases()["main_distorted"]
    args = (c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"])
    base = capi.epipolar_five_point(*args, c["subsets"])
    out = capi.epipolar_five_point(*args, np.concatenate([c["subsets"][::-1], c["subsets"], c["subsets"][::-1]]))
    for lo, order in ((0, slice(None, None, -1)), (65, slice(None)), (130, slice(None, None, -1))):
        assert np.ascontiguousarray(out["E"][lo:lo + 65]).tobytes() == np.ascontiguousarray(base["E"][order]).tobytes()
        assert np.array_equal(out["status"][lo:lo + 65], base["status"][order]) and np.array_equal(out["num_solutions"][lo:lo + 65], base["num_solutions"][order])


def pick(five, sc):
    """the tie rule in numpy: per task the scored slot with the most inliers, then the most in front, then the first"""
    H = len(five["status"])
    best = np.full(H, -1)
    for t in range(H):
        for s in range(10):
            k = t * 10 + s
            if s >= five["num_solutions"][t] or not sc["status"][k]:
                continue
            key = (sc["num_inliers"][k], sc["num_front"][k].max())
            if best[t] < 0 or key > (sc["num_inliers"][t * 10 + best[t]], sc["num_front"][t * 10 + best[t]].max()):
                best[t] = s
    return best


def test_hypotheses_is_its_parts_in_one_call(capi, scoring):
    s, subsets, _ = scoring
    args = (s["cam"], s["cam"], s["xy_a"], s["xy_b"])
    thr = R.RANSAC["threshold_px"]
    five = capi.epipolar_five_point(*args, subsets)
    sc = capi.epipolar_score(*args, five["E"].reshape(-1, 9), threshold_px=thr)   # (an empty slot is a zero matrix: declined)
    best = pick(five, sc)
    both = capi.epipolar_hypotheses_five_point(*args, subsets, threshold_px=thr)
    assert five["status"].sum() >= 60 and np.array_equal(both["status"], (best >= 0).astype(np.uint8)) and np.array_equal(both["num_solutions"], five["num_solutions"])
    for t in range(64):
        if best[t] < 0:
            continue
        k = t * 10 + best[t]
        assert both["num_inliers"][t] == sc["num_inliers"][k] and np.array_equal(both["num_front"][t], sc["num_front"][k]), t
        assert both["E"][t].tobytes() == five["E"][t, best[t]].tobytes() and both["poses"][t].tobytes() == sc["poses"][k].tobytes(), t
    again = capi.epipolar_hypotheses_five_point(*args, subsets, threshold_px=thr)
    assert all(again[k].tobytes() == both[k].tobytes() for k in both)
    # a declined subset (a repeated index) beside them: zero counts, its slots untouched
    subs = subsets.copy(); subs[3, 4] = subs[3, 0]
    E = np.full((64, 9), SENTINEL); poses = np.full((64, 6), SENTINEL)
    out = capi.epipolar_hypotheses_five_point(*args, subs, threshold_px=thr, E_out=E, poses_out=poses)
    assert out["status"][3] == 0 and out["num_inliers"][3] == 0 and not out["num_front"][3].any() and out["num_solutions"][3] == 0
    assert np.all(E[3] == SENTINEL) and np.all(poses[3] == SENTINEL)
    keep = np.arange(64) != 3
    assert E[keep].tobytes() == both["E"][keep].tobytes() and np.array_equal(out["num_inliers"][keep], both["num_inliers"][keep])


def test_the_device_counts_what_the_host_chain_counts(capi, scoring):
    """64 hypotheses on the frames (0, 4) outlier scene (n ~ 440): the host's matrices scored on the device give the host's counts, and the
    device chain gives the host chain's status, solution count, counts and matrix"""
    s, subsets, hst = scoring
    args = (s["cam"], s["cam"], s["xy_a"], s["xy_b"])
    thr = R.RANSAC["threshold_px"]
    assert hst["status"].sum() >= 60
    sc = capi.epipolar_score(*args, hst["E"], threshold_px=thr)
    dev = capi.epipolar_hypotheses_five_point(*args, subsets, threshold_px=thr)
    assert np.array_equal(dev["status"], hst["status"]) and np.array_equal(dev["num_solutions"], hst["num_solutions"])
    for t in range(64):
        if not hst["status"][t]:
            continue
        assert sc["status"][t] == 1 and sc["num_inliers"][t] == hst["num_inliers"][t] and list(sc["num_front"][t]) == list(hst["num_front"][t]), t
        assert dev["num_inliers"][t] == hst["num_inliers"][t] and list(dev["num_front"][t]) == list(hst["num_front"][t]), t
        assert np.max(np.abs(dev["E"][t] - hst["E"][t])) <= 1e-12 and np.max(np.abs(dev["poses"][t] - hst["poses"][t])) <= 1e-9, t


def run_ransac(exe, d, scene, on_host, name):
    path = os.path.join(str(d), name + ".bin")
    R.write_scene_file(path, scene)
    o = R.RANSAC
    r = subprocess.run([exe, "ransac", path, str(o["iterations"]), str(o["threshold_px"]), str(o["refits"]), str(o["min_inliers"]), str(o["rng_state"]), str(int(on_host)),
                        "five_point"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [[float(x) for x in line.split()] for line in r.stdout.strip().split("\n")]
    head = [int(v) for v in rows[0]]
    return dict(ok=bool(head[0]), winner_task=head[1], num_inliers=head[2], num_front=head[3], refits_adopted=head[4], E=np.array(rows[1]), pose=np.array(rows[2]),
                mask=np.array(rows[3]).astype(bool))


def check_loop(exe, d, s, what, min_found):
    dev = run_ransac(exe, d, s, False, "dev5")
    hst = run_ransac(exe, d, s, True, "hst5")
    found = int((dev["mask"] & s["true_inlier"]).sum())
    good = R.reprojecting_inliers(s, dev["pose"], dev["mask"])
    rot, base = R.distance_to_truth(dev["pose"], s)
    print(f"{what}: winner task {dev['winner_task']} (host {hst['winner_task']}), refits adopted {dev['refits_adopted']} (host {hst['refits_adopted']}), inliers "
          f"{dev['num_inliers']} ({found} true), in front {dev['num_front']}, reprojecting {good}, rotation {rot:.3f} deg, baseline {base:.3f} deg, "
          f"|pose - host| {np.max(np.abs(dev['pose'] - hst['pose'])):.2e}")
    assert dev["ok"] and found >= min_found
    assert dev["num_front"] >= 0.9 * dev["num_inliers"] and good >= 0.9 * dev["num_inliers"]
    assert dev["winner_task"] == hst["winner_task"]
    assert np.max(np.abs(dev["pose"] - hst["pose"])) <= 1e-12


@pytest.mark.parametrize("fb,rolling", R.OUTLIER_SCENES)
def test_find_essential_ransac_five_point_on_an_outlier_scene(exe, host, fb, rolling):
    """findEssentialRansac with solver = FivePoint, the hypotheses on the device: the host loop's winner task, its pose within 1e-12, and the
    acceptance ratios of the host test"""
    s = R.outlier_scene(fb, rolling)
    check_loop(exe, host[1], s, f"frames (0, {fb}) rolling={rolling}", 0.9 * s["true_inlier"].sum())


def test_find_essential_ransac_five_point_on_a_planar_scene(exe, host):
    check_loop(exe, host[1], F.planar_scene(0), "planar scene, seed 0", 0.9 * 60)


@pytest.mark.parametrize("rolling", [True, False])
def test_two_frames_of_a_session_get_their_poses_and_tracks_from_five_point_subsets(exe, tmp_path, rolling):
    """examples/two_view solver=five_point on the sessions of test_gpu_two_view.py, under that test's criteria"""
    from test_gpu_two_view import Sess, run
    sess = Sess(rolling)
    kv = ("a=0", f"b={FB}", "ba=0", f"rolling={int(rolling)}", "solver=five_point")
    got = run(exe, tmp_path, sess, *kv)
    rep = got["report"]
    slots = 2 if rolling else 1
    print(f"rolling={rolling}: {rep}")
    assert rep["ok"] == 1 and rep["correspondences"] >= 400 and rep["front"] >= 0.9 * rep["inliers"] >= 0.9 * 0.9 * rep["correspondences"]
    assert len(got["poses"][0]) == slots and not np.any(np.array(got["poses"][0]))
    assert len(got["poses"][FB]) == slots and all(p == got["poses"][FB][0] for p in got["poses"][FB])
    assert abs(np.linalg.norm(got["poses"][FB][0][3:]) - 1.0) <= 1e-9
    assert rep["tracks"] == len(got["tracks"]) >= 0.9 * rep["inliers"]
    for f in range(12):
        if f not in (0, FB):
            assert got["poses"][f] == [] and not any(o[1] for o in got["frames"][f])
    assert all(sorted(r[0] for r in tr[2]) == [0, FB] for tr in got["tracks"])
    again = run(exe, tmp_path, sess, *kv, name="again")
    assert again["bytes"] == got["bytes"]


def test_bad_arguments_are_errors_and_leave_the_outputs_untouched(capi):
    lib = capi.lib()
    cam = np.ascontiguousarray(R.CAM_DIST); xy = np.zeros((16, 2), dtype=np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    five = np.arange(5, dtype=np.int32)[None, :]
    eight = np.arange(8, dtype=np.int32)[None, :]

    def both(n, sub, tasks, cam_=cam, xy_=xy, null_out=False, device=0):
        k = max(tasks, 1)
        E10 = np.full((k, 10, 9), SENTINEL); E = np.full((k, 9), SENTINEL); poses = np.full((k, 6), SENTINEL); status = np.full(k, 77, dtype=np.uint8)
        count = np.full(k, 77, dtype=np.int32); inl = np.full(k, 77, dtype=np.int32); front = np.full((k, 4), 77, dtype=np.int32)
        codes = (lib.rsba_epipolar_five_point(device, ptr(cam_), ptr(cam), ptr(xy_), ptr(xy), n, ptr(sub), tasks, None if null_out else ptr(E10), ptr(count), ptr(status)),
                 lib.rsba_epipolar_hypotheses_five_point(device, ptr(cam_), ptr(cam), ptr(xy_), ptr(xy), n, ptr(sub), tasks, 4.0, None if null_out else ptr(E), ptr(poses),
                                                         ptr(status), ptr(inl), ptr(front), ptr(count)))
        assert np.all(E10 == SENTINEL) and np.all(E == SENTINEL) and np.all(poses == SENTINEL) and np.all(status == 77) and np.all(count == 77)
        assert np.all(inl == 77) and np.all(front == 77)
        return codes

    def eight_point(n, sub, m, tasks, cam_=cam, null_out=False, device=0):
        """the code the eight-point call returns for the same mistake"""
        E = np.zeros((max(tasks, 1), 9)); status = np.zeros(max(tasks, 1), dtype=np.uint8)
        return lib.rsba_epipolar_eight_point(C.c_int32(device), ptr(cam_), ptr(cam), ptr(xy), ptr(xy), C.c_int32(n), ptr(sub), C.c_int32(m), C.c_int32(tasks),
                                             None if null_out else ptr(E), ptr(status))

    code = eight_point(7, eight, 8, 1)
    assert code != 0
    assert both(4, five, 1) == (code,) * 2                                                   # n = 4
    bad = five.copy(); bad[0, 4] = 16
    assert both(16, bad, 1) == (code,) * 2                                                   # an index out of range
    bad[0, 4] = -1
    assert both(16, bad, 1) == (code,) * 2
    assert both(16, five, 1, null_out=True) == (eight_point(16, eight, 8, 1, null_out=True),) * 2 == (code,) * 2   # NULL outputs
    assert both(16, None, 1) == (code,) * 2 and both(16, five, 1, cam_=None) == (code,) * 2 and both(16, five, 1, xy_=None) == (code,) * 2
    assert both(16, five, 0) == (eight_point(16, eight, 8, 0),) * 2 == (code,) * 2           # num_tasks = 0
    assert both(16, five, -3) == (code,) * 2
    bad_device = eight_point(16, eight, 8, 1, device=99)
    assert bad_device != 0 and both(16, five, 1, device=99) == (bad_device,) * 2
    with pytest.raises(capi.RsbaError):
        capi.epipolar_five_point(cam, cam, xy, xy, bad)
