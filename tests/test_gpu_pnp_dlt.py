"""DLT start poses of the RANSAC hypotheses on the device (rsba_pnp_dlt, rsba_pnp_gs_hypotheses) against the extended-precision
restatement of tests/pnp_dlt_reference.py, on the case list test_pnp_dlt_reference.py fixes.

The bound: tests/golden/pnp_dlt_bound.json records the host fp64 dlt_pose's worst |pose - reference| / (kappa eps) over these cases;
the kernel applies the same rotations in another operation order, so it gets that ratio times 4.  Nothing here comes from device output."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import pnp_dlt_reference as R
from helpers import build_host_program, load_golden
from rsba_amd.problem import GLOBAL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    return capi


def device_bound():
    rec = load_golden("pnp_dlt_bound.json")
    return rec["host_worst_error_over_kappa_eps"] * rec["device_factor"]


@pytest.mark.parametrize("name", list(R.cases()))
def test_dlt_matches_the_extended_precision_reference(capi, name):
    """status = the reference's branch for every subset; accepted poses within the bound; declined slots untouched; two calls agree
    bit for bit.  main_*: 40 points, 65 subsets (a full wave and one lane); single: num_tasks = 1, m = n = 6."""
    c, ref = R.cases()[name], R.reference(name)
    T = len(c["subsets"])
    poses = np.full((T, 6), SENTINEL)
    out = capi.pnp_dlt(c["cam"], c["X"], c["xy"], c["subsets"], poses_out=poses)
    assert list(out["status"]) == [r["branch"] for r in ref]
    bound, worst = device_bound(), 0.0
    for t, r in enumerate(ref):
        if r["branch"] == 0:
            assert np.all(poses[t] == SENTINEL), (name, t)
        else:
            ratio = float(np.max(np.abs(poses[t] - np.array(r["pose"])))) / (r["kappa"] * R.EPS)
            worst = max(worst, ratio)
    print(f"{name}: device worst |pose - reference| / (kappa eps) = {worst:.4g} (bound {bound:.4g})")
    assert worst <= bound, (name, worst, bound)
    again = capi.pnp_dlt(c["cam"], c["X"], c["xy"], c["subsets"], poses_out=np.full((T, 6), SENTINEL))
    assert np.array_equal(again["status"], out["status"]) and again["poses"].tobytes() == poses.tobytes()


def test_results_do_not_depend_on_where_a_subset_sits_in_the_launch(capi):
    """the 65 subsets reversed and repeated (195 tasks, four workgroups): every copy gives the bytes of the first call"""
    c = R.cases()["main_distorted"]
    base = capi.pnp_dlt(c["cam"], c["X"], c["xy"], c["subsets"])
    subs = np.concatenate([c["subsets"][::-1], c["subsets"], c["subsets"][::-1]])
    out = capi.pnp_dlt(c["cam"], c["X"], c["xy"], subs)
    for part, order in ((out["poses"][:65], slice(None, None, -1)), (out["poses"][65:130], slice(None)), (out["poses"][130:], slice(None, None, -1))):
        assert np.ascontiguousarray(part).tobytes() == np.ascontiguousarray(base["poses"][order]).tobytes()
    assert np.array_equal(out["status"][65:130], base["status"])


def host_dlt(tmp_path, cam, X, xy, subs):
    """(accepted [T], poses [T,6]) of the C++ pnp_detail::dlt_pose (tests/pnp_dlt_host.cpp, host code only)"""
    exe = build_host_program("pnp_dlt_host", tmp_path)
    T, m = subs.shape
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", 1)); f.write(struct.pack("<3i", len(X), m, T)); f.write(np.asarray(cam, dtype="<f8").tobytes())
        f.write(X.astype("<f4").tobytes()); f.write(xy.astype("<f4").tobytes()); f.write(subs.astype("<i4").tobytes())
    rows = np.array([[float(x) for x in line.split()] for line in subprocess.run([exe, str(tmp_path / "cases.bin")], check=True, capture_output=True, text=True).stdout.strip().split("\n")])
    return rows[:, 0].astype(int), rows[:, 1:]


def test_gs_hypotheses_equal_the_two_step_form(capi, oracle, tmp_path):
    """rsba_pnp_gs_hypotheses against what it replaces: host dlt_pose starts -> rsba_pnp_tasks(GLOBAL, 5 iterations) over the accepted
    subsets.  Same statuses, same winner, its inlier set within one borderline point, its pose within 1e-6 (the tolerances of
    test_gpu_pnp.py::test_ransac_host_program_matches_sequential_oracle_replay for the same comparison)."""
    from test_gpu_pnp import CAM, pnp_scene, random_subsets
    sc = pnp_scene(oracle, GLOBAL, n=220, outliers=0.3, seed=8)
    subs = random_subsets(np.random.default_rng(4), len(sc["X"]), 60, 6)
    subs[7] = subs[7][[0, 1, 2, 3, 4, 0]]                        # one degenerate subset: declined by both
    err = 6.0
    ok, starts = host_dlt(tmp_path, CAM, sc["X"], sc["xy"], subs)
    acc = np.flatnonzero(ok)
    two = capi.pnp_tasks(CAM, GLOBAL, sc["scan"], sc["X"], sc["xy"], subs[acc], np.concatenate([starts[acc], starts[acc]], axis=1),
                         max_num_iterations=5, reprojection_error=err, drop_coincident=False)
    status2 = np.zeros(60, dtype=np.uint8); status2[acc] = two["status"]
    count2 = np.zeros(60, dtype=np.int32); count2[acc] = two["num_inliers"]
    one = capi.pnp_gs_hypotheses(CAM, sc["X"], sc["xy"], subs, max_num_iterations=5, reprojection_error=err)
    assert one["status"][7] == 0 and ok[7] == 0
    assert np.array_equal(one["status"], status2)
    usable = np.flatnonzero(status2)
    w1 = usable[np.argmax(one["num_inliers"][usable])]; w2 = usable[np.argmax(count2[usable])]
    assert w1 == w2
    assert np.max(np.abs(one["num_inliers"].astype(int) - count2)) <= 1
    p1, p2 = one["poses"][w1], two["poses"][list(acc).index(w2), 0]
    assert np.max(np.abs(p1 - p2)) <= 1e-6
    m1 = capi.pnp_inliers(CAM, GLOBAL, sc["scan"], sc["X"], sc["xy"], np.concatenate([p1, p1]), err)
    m2 = capi.pnp_inliers(CAM, GLOBAL, sc["scan"], sc["X"], sc["xy"], np.concatenate([p2, p2]), err)
    assert (m1 != m2).sum() <= 1 and m1.sum() == one["num_inliers"][w1]
    assert m1.sum() >= 0.8 * (~sc["outlier"]).sum()              # and the winner is the pose
    # status 2 keeps the DLT pose; declined subsets report nothing
    assert one["num_inliers"][7] == 0 and one["final_cost"][7] == 0 and np.all(one["poses"][7] == 0)
    again = capi.pnp_gs_hypotheses(CAM, sc["X"], sc["xy"], subs, max_num_iterations=5, reprojection_error=err)
    assert again["poses"].tobytes() == one["poses"].tobytes() and np.array_equal(again["num_inliers"], one["num_inliers"])


def test_bad_arguments_are_errors_and_leave_the_outputs_untouched(capi):
    lib = capi.lib()
    cam = np.ascontiguousarray(R.CAM_DIST); X = np.zeros((8, 3), dtype=np.float32); xy = np.zeros((8, 2), dtype=np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def both(n, sub, m, T, cam_=cam, X_=X, null_out=False):
        poses = np.full((max(T, 1), 6), SENTINEL); status = np.full(max(T, 1), 77, dtype=np.uint8)
        cost = np.full(max(T, 1), SENTINEL); inl = np.full(max(T, 1), 77, dtype=np.int32)
        a = lib.rsba_pnp_dlt(C.c_int32(0), ptr(cam_), ptr(X_), ptr(xy), C.c_int32(n), ptr(sub), C.c_int32(m), C.c_int32(T), None if null_out else ptr(poses), ptr(status))
        b = lib.rsba_pnp_gs_hypotheses(C.c_int32(0), ptr(cam_), ptr(X_), ptr(xy), C.c_int32(n), ptr(sub), C.c_int32(m), C.c_int32(T), C.c_int32(5), C.c_float(3.0),
                                       None if null_out else ptr(poses), ptr(status), ptr(cost), ptr(inl))
        assert np.all(poses == SENTINEL) and np.all(status == 77) and np.all(cost == SENTINEL) and np.all(inl == 77)
        return a, b

    six = np.arange(6, dtype=np.int32)[None, :]
    tasks_code = lib.rsba_pnp_tasks(C.c_int32(0), ptr(cam), C.c_int32(0), ptr(np.array([0, 1], dtype=np.int32)), ptr(X), ptr(xy), C.c_int32(8),
                                    ptr(np.array([[0, 1, 2, 3, 4, 8]], dtype=np.int32)), C.c_int32(6), C.c_int32(1), ptr(np.zeros(12)), C.c_int32(0), C.c_int32(5), C.c_int32(0),
                                    C.c_float(3.0), ptr(np.zeros(12)), ptr(np.zeros(1, dtype=np.uint8)), None, None)
    assert tasks_code != 0
    assert both(8, np.arange(5, dtype=np.int32)[None, :], 5, 1) == (tasks_code, tasks_code)                    # m < 6
    assert both(5, six, 6, 1) == (tasks_code, tasks_code)                                                     # n < m
    assert both(8, np.array([[0, 1, 2, 3, 4, 8]], dtype=np.int32), 6, 1) == (tasks_code, tasks_code)           # index out of range
    assert both(8, np.array([[0, 1, 2, 3, 4, -1]], dtype=np.int32), 6, 1) == (tasks_code, tasks_code)
    assert both(8, six, 6, 0) == (tasks_code, tasks_code)                                                     # no tasks
    assert both(8, None, 6, 1) == (tasks_code, tasks_code)                                                    # null pointers
    assert both(8, six, 6, 1, cam_=None) == (tasks_code, tasks_code)
    assert both(8, six, 6, 1, X_=None) == (tasks_code, tasks_code)
    assert both(8, six, 6, 1, null_out=True) == (tasks_code, tasks_code)
    # no such device: the code rsba_pnp_tasks returns for it
    poses = np.full((1, 6), SENTINEL); status = np.full(1, 77, dtype=np.uint8)
    t = lib.rsba_pnp_tasks(C.c_int32(99), ptr(cam), C.c_int32(0), ptr(np.array([0, 1], dtype=np.int32)), ptr(X), ptr(xy), C.c_int32(8), ptr(six), C.c_int32(6), C.c_int32(1),
                           ptr(np.zeros(12)), C.c_int32(0), C.c_int32(5), C.c_int32(0), C.c_float(3.0), ptr(np.zeros(12)), ptr(np.zeros(1, dtype=np.uint8)), None, None)
    d = lib.rsba_pnp_dlt(C.c_int32(99), ptr(cam), ptr(X), ptr(xy), C.c_int32(8), ptr(six), C.c_int32(6), C.c_int32(1), ptr(poses), ptr(status))
    g = lib.rsba_pnp_gs_hypotheses(C.c_int32(99), ptr(cam), ptr(X), ptr(xy), C.c_int32(8), ptr(six), C.c_int32(6), C.c_int32(1), C.c_int32(5), C.c_float(3.0), ptr(poses), ptr(status), None, None)
    assert t != 0 and d == t and g == t and np.all(poses == SENTINEL) and status[0] == 77
    with pytest.raises(capi.RsbaError):
        capi.pnp_dlt(cam, X, xy, np.array([[0, 1, 2, 3, 4, 8]], dtype=np.int32))
