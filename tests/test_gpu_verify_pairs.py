"""The batched essential-matrix RANSAC (rsba_epipolar_ransac_pairs; findEssentialRansacPairs through examples/verify_matches) against the
existing path: findEssentialRansac on each pair alone, run pair by pair by the same example over the single-pair entry points.

One call of 67 pairs, assembled by repetition from the scenes the two-view tests use (verify_pairs_common.py): the four outlier scenes
(n = 436 .. 449, no multiple of 64; they take refits), the case list (n = 8, 12, 24, 48), the planar scene (60), the pure-rotation and
coincident-point pairs (n = 8, every hypothesis declined), two pairs with a distorted and a pinhole camera, a pair of 7 in the middle and
next to it the sparse pair (n = 10, six correspondences and four gross outliers: a winner under the refit size, so the compaction of the
first round ends the pair with a non-zero count — test_verify_pairs_host.py checks that on the host).
67 pairs: the refit runs one lane per pair, so the call crosses a 64-lane workgroup.  100 subsets per pair, both solvers.

Everything is compared for equality — the counts, the masks, and E and the pose bit for bit: the batched call runs the single-pair calls'
compiled eight-point and score kernels (the refits through the same eight-point kernel with a list per task), and its own kernels move
integers and copies."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import verify_pairs_common as V
from helpers import build_host_program

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.678
P, TASKS, MIDDLE, SPARSE = 67, 100, 33, 34


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    return capi


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as G
    path = os.path.join(ROOT, "examples", "verify_matches")
    if not os.path.exists(path):
        G.build()
    return path


@pytest.fixture(scope="module")
def call(tmp_path_factory):
    """the 67 pairs, the arrays of the C call, and the subsets per solver: distinct_subsets(n_p, m, 100, rng_state) through
    tests/two_view_host.cpp — the draw findEssentialRansac makes for the pair alone"""
    d = tmp_path_factory.mktemp("verify_pairs_gpu")
    host = build_host_program("two_view_host", d)
    base = V.outlier_pairs() + V.small_pairs()
    pairs = [base[i % len(base)] for i in range(P)]
    pairs[MIDDLE] = V.short_pair()
    pairs[SPARSE] = V.sparse_pair()
    cams, index = [], {}
    for p in pairs:
        for side in ("cam_a", "cam_b"):
            if p[side].tobytes() not in index:
                index[p[side].tobytes()] = len(cams); cams.append(p[side])
    drawn = {}

    def subsets(n, m):
        if n < 8:
            return np.full((TASKS, m), 10 ** 6, dtype=np.int32)     # (never read: any index would be out of range)
        if (n, m) not in drawn:
            out = subprocess.run([host, "subsets", str(n), str(m), str(TASKS), str(V.OPTIONS["rng_state"])], check=True, capture_output=True, text=True).stdout
            drawn[(n, m)] = np.array([[int(x) for x in line.split()] for line in out.strip().split("\n")], dtype=np.int32)
        return drawn[(n, m)]
    sizes = [len(p["xy_a"]) for p in pairs]
    assert 8 in sizes and sizes[MIDDLE] == 7 and any(n % 64 for n in sizes if n > 64) and len(cams) >= 3
    assert any(p["cam_a"].tobytes() != p["cam_b"].tobytes() for p in pairs)
    path = d / "pairs.bin"
    V.write_pairs_file(path, pairs)
    return dict(pairs=pairs, dir=d, path=path, cams=np.array(cams), cam_a=np.array([index[p["cam_a"].tobytes()] for p in pairs], dtype=np.int32),
                cam_b=np.array([index[p["cam_b"].tobytes()] for p in pairs], dtype=np.int32), offset=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                xy_a=np.concatenate([p["xy_a"] for p in pairs]), xy_b=np.concatenate([p["xy_b"] for p in pairs]),
                subsets={m: np.stack([subsets(n, m) for n in sizes]) for m in (8, 5)})


def solver_name(m):
    return "five_point" if m == 5 else "eight_point"


def run_example(exe, path, mode, m, count, max_tasks=0):
    o = V.OPTIONS
    r = subprocess.run([exe, "pairs", str(path), mode, str(o["iterations"]), str(o["threshold_px"]), str(o["refits"]), str(o["min_inliers"]), str(o["rng_state"]), "0",
                        solver_name(m), str(max_tasks)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, V.parse_results(r.stdout, count)


_REFERENCE = {}


def reference(exe, call, m):
    """findEssentialRansac pair by pair, once per solver"""
    if m not in _REFERENCE:
        _REFERENCE[m] = run_example(exe, call["path"], "sequential", m, P)
    return _REFERENCE[m]


def batched(capi, call, m, order=None, max_tasks=0):
    """the C call over the pairs in `order` (None: an empty pair, n = 0, whose subsets are never read), the outputs that a pair without a
    winner must not touch filled with a sentinel"""
    order = list(range(P)) if order is None else order
    empty = [k for k, p in enumerate(order) if p is None]
    known = [0 if p is None else p for p in order]
    sizes = [0 if p is None else call["offset"][p + 1] - call["offset"][p] for p in order]
    points = np.concatenate([np.zeros(0)] + [np.arange(call["offset"][p], call["offset"][p + 1]) for p in order if p is not None]).astype(np.int64)
    subsets = call["subsets"][m][known]
    subsets[empty] = 10 ** 6
    E = np.full((len(order), 9), SENTINEL); poses = np.full((len(order), 6), SENTINEL)
    out = capi.epipolar_ransac_pairs(call["cams"], call["cam_a"][known], call["cam_b"][known], np.concatenate([[0], np.cumsum(sizes)]), call["xy_a"][points], call["xy_b"][points],
                                     subsets, threshold_px=V.OPTIONS["threshold_px"], refits=V.OPTIONS["refits"], max_tasks_per_launch=max_tasks,
                                     E_out=E, poses_out=poses)
    out["offset"] = np.concatenate([[0], np.cumsum(sizes)])
    return out


def pair_bytes(out, k):
    lo, hi = out["offset"][k], out["offset"][k + 1]
    return b"".join(np.ascontiguousarray(out[key][k]).tobytes() for key in ("E", "poses", "status", "winner_task", "refits_adopted", "num_inliers", "num_front")) + out["mask"][lo:hi].tobytes()


@pytest.mark.parametrize("m", [8, 5])
def test_every_pair_equals_find_essential_ransac_on_the_pair_alone(capi, exe, call, m):
    _, ref = reference(exe, call, m)
    out = batched(capi, call, m)
    names = [p["name"] for p in call["pairs"]]
    for k, r in enumerate(ref):
        lo, hi = call["offset"][k], call["offset"][k + 1]
        assert out["status"][k] == (1 if r["winner_task"] >= 0 else 0), (k, names[k])
        assert out["winner_task"][k] == r["winner_task"] and out["refits_adopted"][k] == r["refits_adopted"] and out["num_inliers"][k] == r["num_inliers"], (k, names[k])
        assert int(out["num_front"][k].max()) == r["num_front"], (k, names[k])
        assert np.array_equal(out["mask"][lo:hi], r["mask"]), (k, names[k])
        if out["status"][k]:
            assert np.array_equal(out["E"][k], r["E"]) and np.array_equal(out["poses"][k], r["pose"]), (k, names[k], np.abs(out["E"][k] - r["E"]).max(), np.abs(out["poses"][k] - r["pose"]).max())
        else:   # declined: zero counts, a zero mask, the sentinel where it was
            assert np.all(out["E"][k] == SENTINEL) and np.all(out["poses"][k] == SENTINEL) and not out["num_front"][k].any() and out["num_inliers"][k] == 0, (k, names[k])
            assert not out["mask"][lo:hi].any() and out["winner_task"][k] == -1 and out["refits_adopted"][k] == 0
    declined = {names[k] for k in range(P) if not out["status"][k]}
    assert declined >= {"seven", "pure_rotation", "coincident"}, declined   # (m = 8 declines every minimal sample of the planar scene too)
    print(f"m={m}: {int(out['status'].sum())} of {P} pairs with a winner, refits adopted {np.bincount(out['refits_adopted'][out['status'] == 1]).tolist()} (pairs per count)")
    assert out["refits_adopted"].max() >= 1            # the refit rounds ran, and not for nothing
    assert out["status"][64:].any() and out["refits_adopted"][64:].max() >= 1   # ... past the 64th lane of the refit too


@pytest.mark.parametrize("m", [8, 5])
def test_the_bytes_depend_neither_on_the_chunking_nor_on_the_order(capi, call, m):
    base = batched(capi, call, m)
    for max_tasks in (700, 50, 6700):     # seven pairs per launch; a budget under one pair's tasks: every pair a chunk of its own; all in one
        other = batched(capi, call, m, max_tasks=max_tasks)
        assert all(other[k].tobytes() == base[k].tobytes() for k in base), max_tasks
    order = list(range(P))[::-1]
    rev = batched(capi, call, m, order=order, max_tasks=1000)
    for k, p in enumerate(order):
        assert pair_bytes(rev, k) == pair_bytes(base, p), p


@pytest.mark.parametrize("m", [8, 5])
def test_one_pair(capi, exe, call, m):
    """P = 1 against the single-pair call, for a pair that takes refits, the pair of 8 and the pair of 7"""
    _, ref = reference(exe, call, m)
    base = batched(capi, call, m)
    for p in (0, [q["name"] for q in call["pairs"]].index("single"), MIDDLE):
        one = batched(capi, call, m, order=[p])
        assert pair_bytes(one, 0) == pair_bytes(base, p), p
        assert one["winner_task"][0] == ref[p]["winner_task"] and np.array_equal(one["mask"], ref[p]["mask"])
        if one["status"][0]:
            assert np.array_equal(one["E"][0], ref[p]["E"]) and np.array_equal(one["poses"][0], ref[p]["pose"])


@pytest.mark.parametrize("m", [8, 5])
def test_find_essential_ransac_pairs_prints_what_the_sequential_calls_print(exe, call, m):
    """the C++ function (its own draw of the subsets, its conversion to TwoViewResult) against findEssentialRansac pair by pair: the same text,
    with the default chunking and with a few pairs per launch"""
    text, _ = reference(exe, call, m)
    assert run_example(exe, call["path"], "batched", m, P)[0] == text
    assert run_example(exe, call["path"], "batched", m, P, max_tasks=900)[0] == text


def is_untouched_empty(out, k):
    return (out["status"][k] == 0 and out["winner_task"][k] == -1 and out["refits_adopted"][k] == 0 and out["num_inliers"][k] == 0 and not out["num_front"][k].any()
            and np.all(out["E"][k] == SENTINEL) and np.all(out["poses"][k] == SENTINEL) and out["offset"][k] == out["offset"][k + 1])


@pytest.mark.parametrize("m", [8, 5])
def test_empty_pairs_are_declined_and_change_nothing_around_them(capi, call, m):
    """pairs of n = 0 between main_pinhole, main_distorted and single: in the middle of a chunk and first in one (three pairs per launch), last
    in a chunk (two per launch), all in one launch; then a call of empty pairs only (no correspondences at all)"""
    order = [4, 5, 6]
    base = batched(capi, call, m, order=order)
    assert base["status"].all()
    mixed = [4, None, 5, None, 6]
    for max_tasks in (3 * TASKS, 2 * TASKS, 0):
        out = batched(capi, call, m, order=mixed, max_tasks=max_tasks)
        assert is_untouched_empty(out, 1) and is_untouched_empty(out, 3), max_tasks
        assert [pair_bytes(out, k) for k in (0, 2, 4)] == [pair_bytes(base, k) for k in range(3)], max_tasks
    for max_tasks in (0, TASKS):
        none = batched(capi, call, m, order=[None, None, None], max_tasks=max_tasks)
        assert len(none["mask"]) == 0 and all(is_untouched_empty(none, k) for k in range(3))


def test_bad_arguments_are_errors_and_leave_the_outputs_untouched(capi, call):
    lib = capi.lib()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    order = [4, MIDDLE, 5]                      # n = 24 (main_pinhole), 7, 24
    assert [call["pairs"][p]["name"] for p in order] == ["main_pinhole", "seven", "main_distorted"]
    sizes = [len(call["pairs"][p]["xy_a"]) for p in order]
    good = dict(cams=call["cams"].copy(), num_cams=len(call["cams"]), cam_a=call["cam_a"][order].copy(), cam_b=call["cam_b"][order].copy(),
                offset=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), num_pairs=3,
                xy_a=np.concatenate([call["pairs"][p]["xy_a"] for p in order]), xy_b=np.concatenate([call["pairs"][p]["xy_b"] for p in order]),
                subsets=np.ascontiguousarray(call["subsets"][8][order]), m=8, tasks=TASKS, refits=3, max_tasks=0, null_out=None, device=0)
    outs = ("E", "poses", "status", "winner", "adopted", "inl", "front", "mask")

    def code(**change):
        a = dict(good, **change)
        o = dict(E=np.full((3, 9), SENTINEL), poses=np.full((3, 6), SENTINEL), status=np.full(3, 77, dtype=np.uint8), winner=np.full(3, 77, dtype=np.int32),
                 adopted=np.full(3, 77, dtype=np.int32), inl=np.full(3, 77, dtype=np.int32), front=np.full((3, 4), 77, dtype=np.int32), mask=np.full(sum(sizes), 77, dtype=np.uint8))
        rc = lib.rsba_epipolar_ransac_pairs(a["device"], ptr(a["cams"]), a["num_cams"], ptr(a["cam_a"]), ptr(a["cam_b"]), ptr(a["offset"]), a["num_pairs"], ptr(a["xy_a"]), ptr(a["xy_b"]),
                                            ptr(a["subsets"]), a["m"], a["tasks"], 4.0, a["refits"], a["max_tasks"], *[None if a["null_out"] == k else ptr(o[k]) for k in outs])
        if rc != 0:
            assert np.all(o["E"] == SENTINEL) and np.all(o["poses"] == SENTINEL) and all(np.all(o[k] == 77) for k in outs[2:]), change
        return rc, o

    rc, o = code()
    assert rc == 0 and list(o["status"]) == [1, 0, 1] and np.all(o["E"][1] == SENTINEL)
    invalid = lib.rsba_epipolar_hypotheses(0, None, None, None, None, 16, None, 8, 1, C.c_double(4.0), None, None, None, None, None)   # what the sibling returns for a null pointer
    assert invalid != 0
    for key in ("cams", "cam_a", "cam_b", "offset", "xy_a", "xy_b", "subsets"):
        assert code(**{key: None})[0] == invalid, key
    for key in outs:
        assert code(null_out=key)[0] == invalid, key
    down = good["offset"].copy(); down[1], down[2] = down[2], down[1]
    assert code(offset=down)[0] == invalid                                   # a decreasing pair_offset
    shifted = good["offset"].copy(); shifted[0] = 1
    assert code(offset=shifted)[0] == invalid
    for bad in (len(call["cams"]), -1):
        cam = good["cam_b"].copy(); cam[2] = bad
        assert code(cam_b=cam)[0] == invalid                                 # a camera index out of range
    six = np.ascontiguousarray(good["subsets"][:, :, :6])
    assert code(subsets=six, m=6)[0] == invalid                              # m = 6
    for bad in (sizes[2], -1):
        sub = good["subsets"].copy(); sub[2, 99, 7] = bad
        assert code(subsets=sub)[0] == invalid                               # an index >= n_p in a pair with n_p >= 8
    sub = good["subsets"].copy(); sub[1] = 10 ** 6
    assert code(subsets=sub)[0] == 0                                         # ... while the subsets of the pair of 7 are not read
    assert code(num_pairs=0)[0] == invalid and code(tasks=0)[0] == invalid and code(refits=-1)[0] == invalid and code(max_tasks=-1)[0] == invalid and code(num_cams=0)[0] == invalid
    no_device = lib.rsba_epipolar_hypotheses(99, ptr(good["cams"]), ptr(good["cams"]), ptr(good["xy_a"]), ptr(good["xy_b"]), 24, ptr(np.arange(8, dtype=np.int32)), 8, 1, C.c_double(4.0),
                                             ptr(np.zeros(9)), ptr(np.zeros(6)), ptr(np.zeros(1, dtype=np.uint8)), ptr(np.zeros(1, dtype=np.int32)), ptr(np.zeros(4, dtype=np.int32)))
    assert no_device != 0 and code(device=99)[0] == no_device
    # a repeated index is a declined task, not an error: the other 99 tasks decide as before
    sub = good["subsets"].copy(); sub[0, 3, 7] = sub[0, 3, 0]
    rc2, o2 = code(subsets=sub)
    assert rc2 == 0 and o2["status"][0] == 1
    with pytest.raises(capi.RsbaError):
        capi.epipolar_ransac_pairs(good["cams"], good["cam_a"], good["cam_b"], down, good["xy_a"], good["xy_b"], good["subsets"])
