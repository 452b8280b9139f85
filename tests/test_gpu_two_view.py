"""The two-view bootstrap on the device (rsba_epipolar_eight_point, rsba_epipolar_score, rsba_epipolar_hypotheses, rsba_epipolar_inliers,
findEssentialRansac and initializeTwoView through examples/two_view) against the extended-precision reference of tests/two_view_reference.py
and the host definitions of include/rsba/two_view.hpp (tests/two_view_host.cpp), on the case list and the outlier scenes
test_two_view_reference.py fixes.

The bounds: tests/golden/two_view_bound.json records the host fp64 code's worst error in the reference's units over the cases, and the host
loop's distance to the true relative pose per outlier scene; the kernels restate the same arithmetic in another operation order, so they get
the first figure times 4 and the second times 2.  Nothing here comes from device output."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import thrift_encode as T
import two_view_reference as R
from helpers import build_host_program, load_golden
from rsba_amd.scene import make_scene
from test_gpu_new_frame import average_reprojection_error

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.678
FB = 4   # the second frame of the sessions and of the scoring scene


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
    d = tmp_path_factory.mktemp("two_view_gpu")
    return build_host_program("two_view_host", d), d


@pytest.fixture(scope="module")
def scoring(host):
    """the frames (0, 4) global-shutter outlier scene, its first 64 RANSAC subsets and what the host definitions make of them"""
    exe_host, d = host
    s = R.outlier_scene(FB, False)
    out = subprocess.run([exe_host, "subsets", str(len(s["xy_a"])), "8", "64", str(R.RANSAC["rng_state"])], check=True, capture_output=True, text=True).stdout
    subsets = np.array([[int(x) for x in line.split()] for line in out.strip().split("\n")], dtype=np.int32)
    return s, subsets, R.run_host_hypotheses(exe_host, d, s, 64)


@pytest.mark.parametrize("name", list(R.cases()))
def test_eight_point_matches_the_extended_precision_reference(capi, name):
    """status = the reference's for every subset; accepted E (up to sign) and the pose rsba_epipolar_score makes of it within the bound;
    declined slots untouched; two calls agree bit for bit.  main_*: 24 correspondences, 65 subsets (a full wave and one lane)."""
    c, ref = R.cases()[name], R.reference(name)
    n_tasks = len(c["subsets"])
    E = np.full((n_tasks, 9), SENTINEL)
    out = capi.epipolar_eight_point(c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"], c["subsets"], E_out=E)
    assert list(out["status"]) == [r["status"] for r in ref]
    poses = np.full((n_tasks, 6), SENTINEL)
    sc = capi.epipolar_score(c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"], E, threshold_px=R.THRESHOLD_PX, poses_out=poses)
    assert list(sc["status"]) == [r["status"] for r in ref]                        # (a sentinel matrix has rank one: declined)
    for t, r in enumerate(ref):
        if r["status"] == 0:
            assert np.all(E[t] == SENTINEL) and np.all(poses[t] == SENTINEL) and sc["num_inliers"][t] == 0 and not sc["num_front"][t].any(), (name, t)
    rec = load_golden("two_view_bound.json")
    bound, worst = rec["device_factor"] * rec["host_worst_error"], R.worst_error(ref, out["status"], E, poses)
    print(f"{name}: device worst |value - reference| in units = {worst:.4g} (bound {bound:.4g})")
    assert worst <= bound, (name, worst, bound)
    again = capi.epipolar_eight_point(c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"], c["subsets"], E_out=np.full((n_tasks, 9), SENTINEL))
    assert np.array_equal(again["status"], out["status"]) and again["E"].tobytes() == E.tobytes()


def test_results_do_not_depend_on_where_a_subset_sits_in_the_launch(capi):
    """the 65 subsets reversed and repeated (195 tasks, four workgroups): every copy gives the bytes of the first call"""
    c = R.cases()["main_distorted"]
    args = (c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"])
    base = capi.epipolar_eight_point(*args, c["subsets"])
    out = capi.epipolar_eight_point(*args, np.concatenate([c["subsets"][::-1], c["subsets"], c["subsets"][::-1]]))
    for lo, order in ((0, slice(None, None, -1)), (65, slice(None)), (130, slice(None, None, -1))):
        assert np.ascontiguousarray(out["E"][lo:lo + 65]).tobytes() == np.ascontiguousarray(base["E"][order]).tobytes()
        assert np.array_equal(out["status"][lo:lo + 65], base["status"][order])


def same_counts(dev, hst, tasks):
    """counts, winner and pose of the device against the host definitions, over the tasks no correspondence of which is within 1e-9
    relative of the threshold"""
    for t in tasks:
        assert dev["status"][t] == hst["scored"][t], t
        if not hst["scored"][t]:
            assert dev["num_inliers"][t] == 0 and not dev["num_front"][t].any()
            continue
        assert hst["margin"][t] > 1e-9, t          # the CPU test has shown that the scene has no such correspondence for the final E; nor here
        assert dev["num_inliers"][t] == hst["num_inliers"][t] and list(dev["num_front"][t]) == list(hst["num_front"][t]), t
        assert int(np.argmax(dev["num_front"][t])) == hst["winner"][t], t
        assert np.max(np.abs(dev["poses"][t] - hst["poses"][t])) <= 1e-9, t


def test_score_counts_what_the_host_definition_counts(capi, scoring):
    """the host's E matrices of 64 subsets on the frames (0, 4) outlier scene (n ~ 440): the five counts, the winning candidate and its pose"""
    s, _, hst = scoring
    dev = capi.epipolar_score(s["cam"], s["cam"], s["xy_a"], s["xy_b"], hst["E"], threshold_px=R.RANSAC["threshold_px"])
    assert hst["scored"].sum() >= 60
    same_counts(dev, hst, range(64))
    mask = capi.epipolar_inliers(s["cam"], s["cam"], s["xy_a"], s["xy_b"], hst["E"][int(np.argmax(hst["num_inliers"]))], threshold_px=R.RANSAC["threshold_px"])
    assert int(mask.sum()) == int(hst["num_inliers"].max())


def test_hypotheses_is_the_two_steps_in_one_call(capi, scoring):
    s, subsets, _ = scoring
    args = (s["cam"], s["cam"], s["xy_a"], s["xy_b"])
    thr = R.RANSAC["threshold_px"]
    one = capi.epipolar_eight_point(*args, subsets)
    two = capi.epipolar_score(*args, one["E"], threshold_px=thr)
    both = capi.epipolar_hypotheses(*args, subsets, threshold_px=thr)
    assert np.array_equal(both["status"], one["status"] & two["status"])
    assert np.array_equal(both["num_inliers"], two["num_inliers"]) and np.array_equal(both["num_front"], two["num_front"])
    assert both["E"].tobytes() == one["E"].tobytes() and both["poses"].tobytes() == two["poses"].tobytes()
    again = capi.epipolar_hypotheses(*args, subsets, threshold_px=thr)
    assert all(again[k].tobytes() == both[k].tobytes() for k in both)
    # a declined subset (a repeated index) beside them: zero counts, its slots untouched
    subs = subsets.copy(); subs[3, 7] = subs[3, 0]
    E = np.full((64, 9), SENTINEL); poses = np.full((64, 6), SENTINEL)
    out = capi.epipolar_hypotheses(*args, subs, threshold_px=thr, E_out=E, poses_out=poses)
    assert out["status"][3] == 0 and out["num_inliers"][3] == 0 and not out["num_front"][3].any() and np.all(E[3] == SENTINEL) and np.all(poses[3] == SENTINEL)
    keep = np.arange(64) != 3
    assert E[keep].tobytes() == both["E"][keep].tobytes() and np.array_equal(out["num_inliers"][keep], both["num_inliers"][keep])


def run_ransac(exe, d, scene, on_host, name):
    path = os.path.join(str(d), name + ".bin")
    R.write_scene_file(path, scene)
    o = R.RANSAC
    r = subprocess.run([exe, "ransac", path, str(o["iterations"]), str(o["threshold_px"]), str(o["refits"]), str(o["min_inliers"]), str(o["rng_state"]), str(int(on_host))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [[float(x) for x in line.split()] for line in r.stdout.strip().split("\n")]
    head = [int(v) for v in rows[0]]
    return dict(ok=bool(head[0]), winner_task=head[1], num_inliers=head[2], num_front=head[3], refits_adopted=head[4], E=np.array(rows[1]), pose=np.array(rows[2]),
                mask=np.array(rows[3]).astype(bool))


@pytest.mark.parametrize("fb,rolling", R.OUTLIER_SCENES)
def test_find_essential_ransac_on_an_outlier_scene(exe, host, fb, rolling):
    """findEssentialRansac with the hypotheses on the device: the two 0.9 conditions, the distance to the truth within twice the recorded host
    figure, the winner task of the host loop, the final pose within 1e-6 of the host loop's (test_gpu_pnp_dlt.py's tolerance for the same
    kind of comparison)"""
    _, d = host
    s = R.outlier_scene(fb, rolling)
    dev = run_ransac(exe, d, s, False, "dev")
    hst = run_ransac(exe, d, s, True, "hst")
    true, found = int(s["true_inlier"].sum()), int((dev["mask"] & s["true_inlier"]).sum())
    good = R.reprojecting_inliers(s, dev["pose"], dev["mask"])
    rot, base = R.distance_to_truth(dev["pose"], s)
    print(f"frames (0, {fb}) rolling={rolling}: winner task {dev['winner_task']} (host {hst['winner_task']}), inliers {dev['num_inliers']} ({found} of {true} true), "
          f"in front {dev['num_front']}, reprojecting {good}, rotation {rot:.3f} deg, baseline {base:.3f} deg, |pose - host| {np.max(np.abs(dev['pose'] - hst['pose'])):.2e}")
    assert dev["ok"] and found >= 0.9 * true and good >= 0.9 * dev["num_inliers"]
    rec = load_golden("two_view_bound.json")["ransac"]
    assert rot <= rec["device_factor"] * rec["scenes"][R.scene_name(fb, rolling)]["rotation_deg"]
    assert base <= rec["device_factor"] * rec["scenes"][R.scene_name(fb, rolling)]["baseline_deg"]
    assert dev["winner_task"] == hst["winner_task"]
    assert np.max(np.abs(dev["pose"] - hst["pose"])) <= 1e-6


# ---------------------------------------------------------------- sessions through examples/two_view ----------------------------------------------------------------
class Sess:
    """the scene of test_gpu_new_frame.py's helper with 600 points: true geometry, 0.3 px of noise; no poses, no tracks.  Matches are
    key-frame matches: every observation is matched to its point's earlier observations in frames 0, 4 and 8 — frame 4 reaches frame 0 and
    nothing else, as createTracks requires of a frame whose other neighbours have no poses yet (it refuses a match into a frame without
    poses, as the reference does).  frames: which frames of the scene the session holds"""
    def __init__(self, rolling, frames=tuple(range(12))):
        self.sc = sc = make_scene(12, 600, rolling=rolling, seed=5, noise_px=0.3, rot_noise=0.0, pos_noise=0.0, pt_noise=0.0)
        p = sc.problem
        self.cam, self.rs, self.scan = p.intrinsics[0], int(p.shutter), list(p.scanlines)
        self.frames = [dict(obs=[], poses=None, prior=None) for _ in frames]
        index = {f: i for i, f in enumerate(frames)}
        seen = {}
        for i in np.argsort(p.obs_frame, kind="stable"):
            f, j = int(p.obs_frame[i]), int(p.obs_point[i])
            if f not in index:
                continue
            k = len(self.frames[index[f]]["obs"])
            self.frames[index[f]]["obs"].append(dict(x=float(p.obs_xy[i, 0]), y=float(p.obs_xy[i, 1]), matches=[(pf, pk, False) for pf, pk in seen.get(j, [])], track=None))
            if f % 4 == 0:
                seen.setdefault(j, []).append((index[f], k))
        self.tracks = []

    def cache(self):
        frames = [T.frame([T.observation(o["x"], o["y"], track=o["track"], matches=o["matches"] or None) for o in fr["obs"]], poses=fr["poses"], prior_poses=fr["prior"])
                  for fr in self.frames]
        return T.file_events(T.session(self.cam, frames, [], self.rs, self.scan, 1280, 720), np.random.default_rng(1), max_event=4096)


def run(exe, tmp_path, sess, *kv, name="o"):
    (tmp_path / "s.cache").write_bytes(sess.cache())
    out = tmp_path / (name + ".bin")
    r = subprocess.run([exe, str(tmp_path / "s.cache"), str(out), *kv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    buf = out.read_bytes()
    pos = 0

    def q():
        nonlocal pos
        v = struct.unpack_from("<q", buf, pos)[0]; pos += 8; return v

    def d(n):
        nonlocal pos
        v = struct.unpack_from(f"<{n}d", buf, pos); pos += 8 * n; return list(v)
    report = dict(ok=q(), correspondences=q(), inliers=q(), front=q(), tracks=q())
    poses, frames, tracks = [], [], []
    for _ in range(q()):
        poses.append([d(6) for _ in range(q())])
        frames.append([(q(), bool(q()), [bool(q()) for _ in range(q())]) for _ in range(q())])
    for _ in range(q()):
        pt = d(3); valid = bool(q())
        tracks.append((pt, valid, [[q(), q(), bool(q())] for _ in range(q())]))
    assert pos == len(buf)
    return dict(report=report, poses=poses, frames=frames, tracks=tracks, bytes=buf)


def rodrigues(w):
    return R._rodrigues(np.asarray(w, dtype=np.float64))


@pytest.mark.parametrize("rolling", [True, False])
def test_two_frames_of_a_session_get_their_poses_and_tracks(exe, tmp_path, rolling):
    sess = Sess(rolling)
    kv = ("a=0", f"b={FB}", "ba=0", f"rolling={int(rolling)}")
    got = run(exe, tmp_path, sess, *kv)
    rep = got["report"]
    slots = 2 if rolling else 1
    print(f"rolling={rolling}: {rep}")
    assert rep["ok"] == 1 and rep["correspondences"] >= 400 and rep["front"] >= 0.9 * rep["inliers"] >= 0.9 * 0.9 * rep["correspondences"]
    assert len(got["poses"][0]) == slots and not np.any(np.array(got["poses"][0]))
    assert len(got["poses"][FB]) == slots and all(p == got["poses"][FB][0] for p in got["poses"][FB])
    assert abs(np.linalg.norm(got["poses"][FB][0][3:]) - 1.0) <= 1e-9                         # the unit baseline
    assert rep["tracks"] == len(got["tracks"]) >= 0.9 * rep["inliers"]                         # tracks for at least 0.9 of the inliers
    for f in range(12):
        if f not in (0, FB):                                                                  # every other frame is untouched
            assert got["poses"][f] == [] and not any(o[1] for o in got["frames"][f])
    assert all(sorted(r[0] for r in tr[2]) == [0, FB] for tr in got["tracks"])
    again = run(exe, tmp_path, sess, *kv, name="again")
    assert again["bytes"] == got["bytes"]                                                     # two runs, the same bytes
    # frame A where it is: the zero-pose result moved by that pose
    pa = [0.03, -0.02, 0.05, 0.4, -0.3, 0.2]
    moved = Sess(rolling)
    moved.frames[0]["poses"] = [pa] * slots
    kept = run(exe, tmp_path, moved, *kv, "keepPoseA=1", name="kept")
    assert kept["report"] == rep and kept["poses"][0] == [pa] * slots
    Ra, Rrel = rodrigues(pa[:3]), rodrigues(got["poses"][FB][0][:3])
    Rb = rodrigues(kept["poses"][FB][0][:3])
    assert np.max(np.abs(Rb - Rrel @ Ra)) <= 1e-9
    assert np.max(np.abs(np.array(kept["poses"][FB][0][3:]) - (np.array(pa[3:]) + Ra.T @ np.array(got["poses"][FB][0][3:])))) <= 1e-9


def test_two_frame_session_with_a_bundle_adjustment(exe, oracle, tmp_path):
    """frames 0 and 4 of the global-shutter scene as a two-frame session, ba=20 fixFirstN=1: the bundle adjustment is usable, and the final
    average reprojection error is not above that of the same createTracks and bundle adjustment started from the true relative geometry
    (unit baseline) by more than 2 % — the reasoning and the margin of test_three_frames_re_added_with_a_windowed_ba: both runs end in the
    same bundle adjustment over (nearly) the same observations, so once the recovered pose is in the basin of the true one the two errors
    differ by what the capped iterations leave between two starts, a small fraction of the error the 0.3 px noise sets, while a wrong
    relative pose costs pixels."""
    sess = Sess(False, frames=(0, FB))
    kv = ("a=0", "b=1", "ba=20", "fixFirstN=1", "minReprojections=2", "rolling=0")
    got = run(exe, tmp_path, sess, *kv)
    assert got["report"]["ok"] == 1 and len(got["poses"][1]) == 1 and sum(1 for t in got["tracks"] if t[1]) >= 0.9 * got["report"]["inliers"]
    true = Sess(False, frames=(0, FB))
    tp = sess.sc.true_poses
    Ra, Rb = rodrigues(tp[0, 0, :3]), rodrigues(tp[FB, 0, :3])
    rel_c = Ra @ (tp[FB, 0, 3:] - tp[0, 0, 3:])
    w = R._np_log(Rb @ Ra.T)
    true.frames[0]["poses"] = [[0.0] * 6]
    true.frames[1]["poses"] = [[*w, *(rel_c / np.linalg.norm(rel_c))]]
    ref = run(exe, tmp_path, true, *kv, "keepPoses=1", name="ref")
    assert ref["report"]["ok"] == 1
    e_got, n_got = average_reprojection_error(oracle, sess, got)
    e_ref, n_ref = average_reprojection_error(oracle, sess, ref)
    print(f"average reprojection error: two-view start {e_got:.6f} px over {n_got} observations, from the true relative geometry {e_ref:.6f} px over {n_ref}")
    assert n_got >= 0.98 * n_ref
    assert e_got <= 1.02 * e_ref


def test_bad_arguments_are_errors_and_leave_the_outputs_untouched(capi):
    lib = capi.lib()
    cam = np.ascontiguousarray(R.CAM_DIST); xy = np.zeros((16, 2), dtype=np.float32); X = np.zeros((16, 3), dtype=np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    eight = np.arange(8, dtype=np.int32)[None, :]; six = np.arange(6, dtype=np.int32)[None, :]

    def all_four(n, sub, m, tasks, cam_=cam, xy_=xy, null_out=False, device=0, calls=4):
        """the codes of the first `calls` entry points (the mistakes of a subset concern the first two, of the task count the first three)"""
        k = max(tasks, 1)
        E = np.full((k, 9), SENTINEL); poses = np.full((k, 6), SENTINEL); status = np.full(k, 77, dtype=np.uint8)
        inl = np.full(k, 77, dtype=np.int32); front = np.full((k, 4), 77, dtype=np.int32); mask = np.full(16, 77, dtype=np.uint8)
        dev, i32, thr = C.c_int32(device), C.c_int32, C.c_double(4.0)
        fns = (lambda: lib.rsba_epipolar_eight_point(dev, ptr(cam_), ptr(cam), ptr(xy_), ptr(xy), i32(n), ptr(sub), i32(m), i32(tasks), None if null_out else ptr(E), ptr(status)),
               lambda: lib.rsba_epipolar_hypotheses(dev, ptr(cam_), ptr(cam), ptr(xy_), ptr(xy), i32(n), ptr(sub), i32(m), i32(tasks), thr, None if null_out else ptr(E), ptr(poses),
                                                    ptr(status), ptr(inl), ptr(front)),
               lambda: lib.rsba_epipolar_score(dev, ptr(cam_), ptr(cam), ptr(xy_), ptr(xy), i32(n), ptr(np.ones((k, 9))), i32(tasks), thr, ptr(inl), ptr(front),
                                               None if null_out else ptr(poses), ptr(status)),
               lambda: lib.rsba_epipolar_inliers(dev, ptr(cam_), ptr(cam), ptr(xy_), ptr(xy), i32(n), ptr(np.ones(9)), thr, None if null_out else ptr(mask)))
        codes = tuple(f() for f in fns[:calls])
        assert np.all(E == SENTINEL) and np.all(poses == SENTINEL) and np.all(status == 77) and np.all(inl == 77) and np.all(front == 77) and np.all(mask == 77)
        return codes

    def dlt(n, sub, m, tasks, cam_=cam, X_=X, null_out=False, device=0):
        """the code the DLT call returns for the same mistake"""
        poses = np.zeros((max(tasks, 1), 6)); status = np.zeros(max(tasks, 1), dtype=np.uint8)
        return lib.rsba_pnp_dlt(C.c_int32(device), ptr(cam_), ptr(X_), ptr(xy), C.c_int32(n), ptr(sub), C.c_int32(m), C.c_int32(tasks), None if null_out else ptr(poses), ptr(status))

    code = dlt(16, six, 6, 0)
    assert code != 0
    assert all_four(7, eight, 8, 1) == (dlt(5, six, 6, 1),) * 4 == (code,) * 4                                              # n < 8 | n < 6
    assert all_four(16, np.arange(7, dtype=np.int32)[None, :], 7, 1, calls=2) == (dlt(16, six[:, :5], 5, 1),) * 2 == (code,) * 2   # m < 8 | m < 6
    bad = eight.copy(); bad[0, 7] = 16
    assert all_four(16, bad, 8, 1, calls=2) == (dlt(16, np.array([[0, 1, 2, 3, 4, 16]], dtype=np.int32), 6, 1),) * 2 == (code,) * 2   # index out of range
    bad[0, 7] = -1
    assert all_four(16, bad, 8, 1, calls=2) == (code,) * 2
    assert all_four(16, eight, 8, 0, calls=3) == (dlt(16, six, 6, 0),) * 3                                                       # no tasks
    assert all_four(16, eight, 8, -3, calls=3) == (code,) * 3
    assert all_four(16, None, 8, 1, calls=2) == (dlt(16, None, 6, 1),) * 2 == (code,) * 2                                        # null pointers
    assert all_four(16, eight, 8, 1, cam_=None) == (dlt(16, six, 6, 1, cam_=None),) * 4 == (code,) * 4
    assert all_four(16, eight, 8, 1, xy_=None) == (dlt(16, six, 6, 1, X_=None),) * 4 == (code,) * 4
    assert all_four(16, eight, 8, 1, null_out=True) == (dlt(16, six, 6, 1, null_out=True),) * 4 == (code,) * 4
    bad_device = dlt(16, six, 6, 1, device=99)                                                                              # no such device
    assert bad_device != 0 and all_four(16, eight, 8, 1, device=99) == (bad_device,) * 4
    with pytest.raises(capi.RsbaError):
        capi.epipolar_eight_point(cam, cam, xy, xy, bad)
