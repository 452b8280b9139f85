"""The batched degeneracy test (rsba_two_view_classify_pairs; classifyPairs through examples/classify_pairs) against the single-pair path:
findHomographyRansac on each pair alone plus the host parallax counts (homo_detail::parallax_counts), run pair by pair by the same example.

One call of 19 pairs, 64 subsets each (homography_reference.py): the five classification pairs (n = 178 .. 196, no multiple of 64; they take
refits), the planar and the general scoring scene (200), pairs of 3, 4, 5 and 7 correspondences in the middle of the list, two pairs with
a distorted and a pinhole camera, the classification pairs once more, and a pair whose pair_status is forced to 0.  The essential results
come from rsba_epipolar_ransac_pairs (five-point subsets) — before and after the new call, which must leave that path's bytes alone.

Everything is compared for equality — the counts, the masks, and H bit for bit: the batched call runs the single-pair calls' compiled DLT
and score kernels (the refits through the same DLT kernel with a list per task), and its own kernels move integers and copies."""
import os
import subprocess

import numpy as np
import pytest

import homography_reference as H
import verify_pairs_common as V
from helpers import build_host_program
from p3p_reference import CAM_DIST, CAM_PLAIN, project

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.678
TASKS, MIN_INLIERS, DEG = 64, 16, 2.0
COS_MIN = float(np.cos(np.radians(DEG)))


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    return capi


@pytest.fixture(scope="module")
def example():
    import __graft_entry__ as G
    path = os.path.join(ROOT, "examples", "classify_pairs")
    if not os.path.exists(path):
        G.build()
    return path


def pair_list():
    cls = H.classification_pairs()
    planar, general = H.scoring_scene(), H.scoring_scene(planar=False)
    scenes = [V.pair(s["cam_a"], s["cam_b"], s["xy_a"], s["xy_b"], name) for s, name in ((planar, "scoring_planar"), (general, "scoring_general"))]
    few = H.cases()["plane_distorted"]          # noise-free points of a plane: four of them have their homography
    short = [V.pair(few["cam_a"], few["cam_b"], few["xy_a"][:n], few["xy_b"][:n], f"short_{n}") for n in (3, 4, 5, 7)]
    rng = np.random.default_rng(41)
    X = H.R._cloud(rng, 37)
    pose = H.R._unit_centre(H.R.POSE_B)
    two = [V.pair(CAM_DIST, CAM_PLAIN, project(CAM_DIST, np.zeros(6), X), project(CAM_PLAIN, pose, X), "two_cameras"),
           V.pair(CAM_PLAIN, CAM_DIST, project(CAM_PLAIN, np.zeros(6), X), project(CAM_DIST, pose, X), "two_cameras_swapped")]
    again = [dict(p, name=p["name"] + "_again") for p in cls]
    forced = [dict(cls[0], name="status_forced_to_0")]
    return [V.pair(p["cam_a"], p["cam_b"], p["xy_a"], p["xy_b"], p["name"]) for p in cls[:3] + scenes[:1] + short[:2] + cls[3:] + short[2:] + scenes[1:] + two + again + forced]


@pytest.fixture(scope="module")
def call(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("classify_pairs_gpu")
    host = build_host_program("homography_host", d)
    pairs = pair_list()
    P = len(pairs)
    cams, index = [], {}
    for p in pairs:
        for side in ("cam_a", "cam_b"):
            if p[side].tobytes() not in index:
                index[p[side].tobytes()] = len(cams); cams.append(p[side])
    drawn = {}

    def subsets(n, m, least):
        if n < least:
            return np.full((TASKS, m), 10 ** 6, dtype=np.int32)     # (never read: any index would be out of range)
        if (n, m) not in drawn:
            out = subprocess.run([host, "subsets", str(n), str(m), str(TASKS), str(H.RNG_STATE)], check=True, capture_output=True, text=True).stdout
            drawn[(n, m)] = np.array([[int(x) for x in line.split()] for line in out.strip().split("\n")], dtype=np.int32)
        return drawn[(n, m)]
    sizes = [len(p["xy_a"]) for p in pairs]
    assert P == 19 and sizes[4:6] == [3, 4] and sizes[8:10] == [5, 7] and len(cams) == 2 and any(p["cam_a"].tobytes() != p["cam_b"].tobytes() for p in pairs)
    path = d / "pairs.bin"
    H.write_pairs_file(path, pairs)
    c = dict(pairs=pairs, P=P, dir=d, host=host, path=path, cams=np.array(cams), cam_a=np.array([index[p["cam_a"].tobytes()] for p in pairs], dtype=np.int32),
             cam_b=np.array([index[p["cam_b"].tobytes()] for p in pairs], dtype=np.int32), offset=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
             xy_a=np.concatenate([p["xy_a"] for p in pairs]), xy_b=np.concatenate([p["xy_b"] for p in pairs]),
             sub5=np.stack([subsets(n, 5, 8) for n in sizes]), sub4=np.stack([subsets(n, 4, 4) for n in sizes]))
    c["essential"] = essential(capi, c)
    front = c["essential"]["num_front"].max(axis=1)
    c["pair_status"] = ((c["essential"]["status"] == 1) & (front >= MIN_INLIERS)).astype(np.uint8)
    c["essential_ok"] = c["pair_status"].copy()
    c["pair_status"][P - 1] = 0
    return c


def essential(capi, c):
    return capi.epipolar_ransac_pairs(c["cams"], c["cam_a"], c["cam_b"], c["offset"], c["xy_a"], c["xy_b"], c["sub5"], threshold_px=H.THRESHOLD_PX, refits=3)


def classify(capi, c, order=None, max_tasks=0):
    """the C call over the pairs in `order` (None: an empty pair, n = 0, whose subsets are never read; it is given pair 0's essential result)"""
    order = list(range(c["P"])) if order is None else order
    empty = [k for k, p in enumerate(order) if p is None]
    known = [0 if p is None else p for p in order]
    sizes = [0 if p is None else c["offset"][p + 1] - c["offset"][p] for p in order]
    points = np.concatenate([np.zeros(0)] + [np.arange(c["offset"][p], c["offset"][p + 1]) for p in order if p is not None]).astype(np.int64)
    subsets = c["sub4"][known]
    subsets[empty] = 10 ** 6
    e = c["essential"]
    out = capi.two_view_classify_pairs(c["cams"], c["cam_a"][known], c["cam_b"][known], np.concatenate([[0], np.cumsum(sizes)]), c["xy_a"][points], c["xy_b"][points],
                                       e["E"][known], e["poses"][known], c["pair_status"][known], subsets, threshold_px=H.THRESHOLD_PX, refits=3,
                                       cos_min_parallax=COS_MIN, max_tasks_per_launch=max_tasks, H_out=np.full((len(order), 9), SENTINEL))
    out["offset"] = np.concatenate([[0], np.cumsum(sizes)])
    return out


def pair_bytes(out, k):
    lo, hi = out["offset"][k], out["offset"][k + 1]
    return b"".join(np.ascontiguousarray(out[key][k]).tobytes() for key in ("H", "status", "winner_task", "refits_adopted", "num_inliers", "num_front", "num_parallax")) + out["mask"][lo:hi].tobytes()


def run_example(example, c, mode, max_tasks=0, tasks=TASKS):
    r = subprocess.run([example, "pairs", str(c["path"]), mode, str(tasks), str(H.THRESHOLD_PX), "3", str(MIN_INLIERS), str(H.RNG_STATE), "0", "five_point", str(DEG), str(max_tasks)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    rows = []
    for p in range(c["P"]):
        v = lines[3 * p].split()
        rows.append(dict(essential_ok=int(v[0]), kind=v[1], h_ok=int(v[2]), winner_task=int(v[3]), refits_adopted=int(v[4]), num_inliers=int(v[5]), num_front=int(v[6]),
                         num_parallax=int(v[7]), H=np.array([float(x) for x in lines[3 * p + 1].split()]), mask=np.array([int(x) for x in lines[3 * p + 2].split()], dtype=bool)))
    return r.stdout, rows


_SEQUENTIAL = {}


def sequential(example, c):
    if not _SEQUENTIAL:
        _SEQUENTIAL["out"] = run_example(example, c, "sequential")
    return _SEQUENTIAL["out"]


def test_every_pair_equals_the_single_pair_path(capi, example, call):
    c = call
    _, ref = sequential(example, c)
    out = classify(capi, c)
    names = [p["name"] for p in c["pairs"]]
    # the host parallax counts decide nothing within 1e-9 of a threshold, so the device's may be compared for equality
    par = H.run_host_parallax(c["host"], c["dir"], c["pairs"], c["essential"]["E"], c["essential"]["poses"], c["pair_status"], COS_MIN)
    print("parallax margins:", [f"{m:.2g}" for m in par["margin"]])
    assert all(m > 1e-9 for m, s in zip(par["margin"], c["pair_status"]) if s)
    for k, r in enumerate(ref):
        lo, hi = c["offset"][k], c["offset"][k + 1]
        assert out["status"][k] == r["h_ok"], (k, names[k])
        assert out["winner_task"][k] == r["winner_task"] and out["refits_adopted"][k] == r["refits_adopted"] and out["num_inliers"][k] == r["num_inliers"], (k, names[k])
        assert np.array_equal(out["mask"][lo:hi], r["mask"]), (k, names[k])
        assert (out["num_front"][k], out["num_parallax"][k]) == (par["num_front"][k], par["num_parallax"][k]), (k, names[k])
        if k < c["P"] - 1:
            assert r["essential_ok"] == c["essential_ok"][k] and (out["num_front"][k], out["num_parallax"][k]) == (r["num_front"], r["num_parallax"]), (k, names[k])
        if out["status"][k]:
            assert np.array_equal(out["H"][k], r["H"]), (k, names[k], np.abs(out["H"][k] - r["H"]).max())
        else:
            assert np.all(out["H"][k] == SENTINEL) and out["num_inliers"][k] == 0 and not out["mask"][lo:hi].any() and out["winner_task"][k] == -1 and out["refits_adopted"][k] == 0
    declined = {names[k] for k in range(c["P"]) if not out["status"][k]}
    assert "short_3" in declined and out["status"][5] == 1, declined        # three correspondences: no homography; four: one
    last = c["P"] - 1
    assert c["essential_ok"][last] == 1 and out["num_front"][last] == 0 and out["num_parallax"][last] == 0 and out["num_front"][0] > 0   # pair_status 0: no counts
    assert pair_bytes(out, last)[:72] == pair_bytes(out, 0)[:72]                # ... and the same homography as the pair it repeats
    assert out["refits_adopted"].max() >= 1
    kinds = {names[k]: r["kind"] for k, r in enumerate(ref)}
    print(kinds)
    assert kinds["b_narrow_general"] == "LowParallax" and kinds["a_wide_general"] == "General" and kinds["e_pure_rotation"] != "General" and kinds["short_7"] == "Unverified"
    assert kinds["scoring_general"] == "General" or not c["essential_ok"][names.index("scoring_general")]


def test_the_bytes_depend_neither_on_the_chunking_nor_on_the_order(capi, call):
    c = call
    base = classify(capi, c)
    for max_tasks in (3 * TASKS, TASKS, 10 ** 6):     # three pairs per launch; one per launch; all in one
        other = classify(capi, c, max_tasks=max_tasks)
        assert all(other[k].tobytes() == base[k].tobytes() for k in base), max_tasks
    order = list(range(c["P"]))[::-1]
    rev = classify(capi, c, order=order, max_tasks=5 * TASKS)
    for k, p in enumerate(order):
        assert pair_bytes(rev, k) == pair_bytes(base, p), p
    one = classify(capi, c, order=[1])
    assert pair_bytes(one, 0) == pair_bytes(base, 1)


def is_untouched_empty(out, k):
    return (out["status"][k] == 0 and out["winner_task"][k] == -1 and out["refits_adopted"][k] == 0 and out["num_inliers"][k] == 0 and out["num_front"][k] == 0
            and out["num_parallax"][k] == 0 and np.all(out["H"][k] == SENTINEL) and out["offset"][k] == out["offset"][k + 1])


def test_empty_pairs_are_declined_and_change_nothing_around_them(capi, call):
    """pairs of n = 0 (with pair_status 1) between three of the pairs: in the middle of a chunk and first in one (three pairs per launch),
    last in a chunk (two per launch), all in one launch; then a call of empty pairs only (no correspondences at all)"""
    c = call
    order = [0, 5, 11]
    assert [c["pairs"][p]["name"] for p in order[1:]] == ["short_4", "two_cameras"] and c["pair_status"][0] == 1
    base = classify(capi, c, order=order)
    assert base["status"].all()
    mixed = [0, None, 5, None, 11]
    for max_tasks in (3 * TASKS, 2 * TASKS, 0):
        out = classify(capi, c, order=mixed, max_tasks=max_tasks)
        assert is_untouched_empty(out, 1) and is_untouched_empty(out, 3), max_tasks
        assert [pair_bytes(out, k) for k in (0, 2, 4)] == [pair_bytes(base, k) for k in range(3)], max_tasks
    for max_tasks in (0, TASKS):
        none = classify(capi, c, order=[None, None, None], max_tasks=max_tasks)
        assert len(none["mask"]) == 0 and all(is_untouched_empty(none, k) for k in range(3))


def test_a_second_stride_of_the_winner_kernel(capi, example, call, tmp_path):
    """65 subsets per pair — one stride of the wave over a pair's tasks and a single lane of the next, in the winner kernel the homography shares
    with the essential matrix (which the other tests run at 100 tasks) — for three of the pairs, against the pair-by-pair path as above"""
    c = call
    tasks, order = 65, [0, 5, 11]
    pairs = [c["pairs"][p] for p in order]
    sizes = [len(p["xy_a"]) for p in pairs]

    def subsets(n, m):
        out = subprocess.run([c["host"], "subsets", str(n), str(m), str(tasks), str(H.RNG_STATE)], check=True, capture_output=True, text=True).stdout
        return np.array([[int(x) for x in line.split()] for line in out.strip().split("\n")], dtype=np.int32)
    offset = np.concatenate([[0], np.cumsum(sizes)])
    xy_a, xy_b = np.concatenate([p["xy_a"] for p in pairs]), np.concatenate([p["xy_b"] for p in pairs])
    sub5 = np.stack([subsets(n, 5) if n >= 8 else np.full((tasks, 5), 10 ** 6, dtype=np.int32) for n in sizes])
    e = capi.epipolar_ransac_pairs(c["cams"], c["cam_a"][order], c["cam_b"][order], offset, xy_a, xy_b, sub5, threshold_px=H.THRESHOLD_PX, refits=3)
    pair_status = ((e["status"] == 1) & (e["num_front"].max(axis=1) >= MIN_INLIERS)).astype(np.uint8)
    out = capi.two_view_classify_pairs(c["cams"], c["cam_a"][order], c["cam_b"][order], offset, xy_a, xy_b, e["E"], e["poses"], pair_status,
                                       np.stack([subsets(n, 4) for n in sizes]), threshold_px=H.THRESHOLD_PX, refits=3, cos_min_parallax=COS_MIN,
                                       H_out=np.full((3, 9), SENTINEL))
    path = tmp_path / "three.bin"
    H.write_pairs_file(path, pairs)
    _, ref = run_example(example, dict(path=path, P=3), "sequential", tasks=tasks)
    for k, r in enumerate(ref):
        lo, hi = offset[k], offset[k + 1]
        assert out["status"][k] == r["h_ok"] == 1 and r["essential_ok"] == pair_status[k], k
        assert out["winner_task"][k] == r["winner_task"] and out["refits_adopted"][k] == r["refits_adopted"] and out["num_inliers"][k] == r["num_inliers"], k
        assert np.array_equal(out["mask"][lo:hi], r["mask"]) and np.array_equal(out["H"][k], r["H"]), k
        assert (out["num_front"][k], out["num_parallax"][k]) == (r["num_front"], r["num_parallax"]), k
    print("winner tasks of 65:", out["winner_task"].tolist())


def test_the_new_call_leaves_the_essential_path_alone(capi, call):
    c = call
    classify(capi, c)
    after = essential(capi, c)
    assert all(after[k].tobytes() == c["essential"][k].tobytes() for k in after)


def test_classify_pairs_prints_what_the_sequential_calls_print(example, call):
    """the C++ function (its own draw of the subsets, its conversion to PairGeometry, the kind rule) against the pair-by-pair path: the same
    text, with the default chunking and with a few pairs per launch"""
    text, _ = sequential(example, call)
    assert run_example(example, call, "batched")[0] == text
    assert run_example(example, call, "batched", max_tasks=200)[0] == text


def test_bad_arguments_are_errors(capi, call):
    c = call
    e = c["essential"]
    args = lambda **kw: dict(dict(cams=c["cams"], a=c["cam_a"], b=c["cam_b"], off=c["offset"], sub=c["sub4"], cos=COS_MIN, refits=3, max_tasks=0), **kw)

    def run(**kw):
        a = args(**kw)
        return capi.two_view_classify_pairs(a["cams"], a["a"], a["b"], a["off"], c["xy_a"], c["xy_b"], e["E"], e["poses"], c["pair_status"], a["sub"], refits=a["refits"],
                                            cos_min_parallax=a["cos"], max_tasks_per_launch=a["max_tasks"])
    run()
    bad = c["sub4"].copy(); bad[0, 5, 2] = c["offset"][1]
    cam = c["cam_b"].copy(); cam[2] = 2
    off = c["offset"].copy(); off[1], off[2] = off[2], off[1]
    for kw in (dict(sub=bad), dict(b=cam), dict(off=off), dict(cos=1.5), dict(cos=float("nan")), dict(refits=-1), dict(max_tasks=-1)):
        with pytest.raises(capi.RsbaError):
            run(**kw)
    free = c["sub4"].copy(); free[4] = 10 ** 6      # the subsets of the pair of 3 are not read
    run(sub=free)
