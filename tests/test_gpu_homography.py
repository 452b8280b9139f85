"""The homography kernels (rsba_homography_dlt, rsba_homography_score, rsba_homography_inliers, rsba_homography_hypotheses) and
findHomographyRansac on the device, against the extended-precision reference and the host definitions (homography_reference.py,
tests/homography_host.cpp) with the bound of tests/golden/homography_bound.json: status equal for every subset, an accepted H within
device_factor x host_worst_error units, counts equal for all 64 hypotheses of the scoring scene (test_homography_reference.py asserts that
none of its correspondences is within 1e-9 of a deciding threshold)."""
import os
import subprocess

import numpy as np
import pytest

import homography_reference as H
from helpers import build_host_program, load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    return capi


@pytest.fixture(scope="module")
def bound():
    return load_golden("homography_bound.json")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("homography_gpu")


@pytest.fixture(scope="module")
def host(workdir):
    return build_host_program("homography_host", workdir)


@pytest.fixture(scope="module")
def example():
    import __graft_entry__ as G
    path = os.path.join(ROOT, "examples", "classify_pairs")
    if not os.path.exists(path):
        G.build()
    return path


def dlt(capi, c, subsets=None):
    sub = c["subsets"] if subsets is None else subsets
    out = np.full((len(sub), 9), SENTINEL)
    return capi.homography_dlt(c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"], sub, H_out=out)


@pytest.mark.parametrize("name", list(H.cases()))
def test_dlt_against_the_reference(capi, bound, name):
    c, ref = H.cases()[name], H.reference(name)
    got = dlt(capi, c)
    assert got["status"].tolist() == [r["status"] for r in ref], [r["why"] for r in ref]
    worst = H.worst_error(ref, got["status"], got["H"])
    limit = bound["device_factor"] * bound["host_worst_error"]
    print(f"{name}: {int(got['status'].sum())} of {len(ref)} accepted, worst error {worst:.3g} units (host {bound['per_case'][name]}, bound {limit:.3g})")
    assert worst <= limit
    assert np.all(got["H"][got["status"] == 0] == SENTINEL)      # a declined slot is untouched
    again = dlt(capi, c)
    assert again["H"].tobytes() == got["H"].tobytes() and again["status"].tobytes() == got["status"].tobytes()


def test_a_subset_s_bytes_do_not_depend_on_its_place_in_the_call(capi):
    """the 65 subsets reversed and repeated: 195 tasks, four workgroups"""
    c = H.cases()["plane_distorted"]
    first = dlt(capi, c)
    sub = np.concatenate([c["subsets"][::-1], c["subsets"], c["subsets"][::-1]])
    many = dlt(capi, c, sub)
    for lo, order in ((0, -1), (65, 1), (130, -1)):
        assert many["H"][lo:lo + 65][::order].tobytes() == first["H"].tobytes() and many["status"][lo:lo + 65][::order].tobytes() == first["status"].tobytes()


@pytest.fixture(scope="module")
def scoring(host, workdir):
    s = H.scoring_scene()
    return s, H.run_host_hypotheses(host, workdir, s, H.SCORING["T"])


def test_score_counts_equal_the_host_s_for_all_64(capi, scoring, bound):
    s, hyp = scoring
    got = capi.homography_score(s["cam_a"], s["cam_b"], s["xy_a"], s["xy_b"], hyp["H"], threshold_px=H.THRESHOLD_PX)
    # a declined host slot holds zeros: a singular matrix, which the score declines too
    assert got["status"].tolist() == hyp["status"].tolist() == bound["scoring"]["status"]
    assert got["num_inliers"].tolist() == hyp["num_inliers"].tolist() == bound["scoring"]["num_inliers"]
    best = int(np.argmax(hyp["num_inliers"]))
    mask = capi.homography_inliers(s["cam_a"], s["cam_b"], s["xy_a"], s["xy_b"], hyp["H"][best], threshold_px=H.THRESHOLD_PX)
    assert mask.sum() == hyp["num_inliers"][best] and len(mask) == 200
    assert not capi.homography_inliers(s["cam_a"], s["cam_b"], s["xy_a"], s["xy_b"], np.zeros(9)).any()


def test_hypotheses_equal_the_two_calls_chained(capi, host, scoring):
    s, _ = scoring
    sub = H.run_host_subsets(host, 200, H.SCORING["T"])
    a = capi.homography_dlt(s["cam_a"], s["cam_b"], s["xy_a"], s["xy_b"], sub, H_out=np.full((64, 9), SENTINEL))
    b = capi.homography_score(s["cam_a"], s["cam_b"], s["xy_a"], s["xy_b"], np.where(a["status"][:, None] == 1, a["H"], 0.0), threshold_px=H.THRESHOLD_PX)
    both = capi.homography_hypotheses(s["cam_a"], s["cam_b"], s["xy_a"], s["xy_b"], sub, threshold_px=H.THRESHOLD_PX, H_out=np.full((64, 9), SENTINEL))
    assert both["status"].tolist() == (a["status"] & b["status"]).tolist() and both["num_inliers"].tolist() == b["num_inliers"].tolist()
    assert both["H"].tobytes() == a["H"].tobytes()
    assert both["status"].sum() >= 16


def test_find_homography_ransac_on_the_device_against_the_host_loop(example, host, workdir, scoring, bound):
    """findHomographyRansac with device hypotheses (examples/classify_pairs, sequential) on the scoring scene: winner, refits adopted, count and
    mask equal the host loop's, H within the bound"""
    s, _ = scoring
    want = H.run_host_ransac(host, workdir, s, H.SCORING["iterations"], H.SCORING["refits"])
    path = os.path.join(str(workdir), "scoring_pair.bin")
    H.write_pairs_file(path, [s])
    r = subprocess.run([example, "pairs", path, "sequential", str(H.SCORING["iterations"]), str(H.THRESHOLD_PX), str(H.SCORING["refits"]), "16", str(H.RNG_STATE), "0", "eight_point", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    head = lines[0].split()
    got = dict(ok=bool(int(head[2])), winner_task=int(head[3]), refits_adopted=int(head[4]), num_inliers=int(head[5]), H=np.array([float(v) for v in lines[1].split()]),
               mask=np.array([int(v) for v in lines[2].split()], dtype=bool))
    assert got["ok"] and got["winner_task"] == want["winner_task"] and got["refits_adopted"] == want["refits_adopted"] and got["num_inliers"] == want["num_inliers"]
    assert np.array_equal(got["mask"], want["mask"])
    # the final H is the DLT over the indices the host loop names (the inliers before the last adopted refit): its reference and units
    ref = H.solve_one(s["cam_a"], s["cam_b"], s["xy_a"], s["xy_b"], want["fitted_to"])
    assert ref["status"] == 1 and not ref["leave_out"] and len(want["fitted_to"]) >= 100
    worst = H.worst_error([ref], [1], got["H"][None, :])
    print(f"findHomographyRansac: winner {got['winner_task']}, {got['num_inliers']} inliers, {got['refits_adopted']} refits; H fitted to {len(want['fitted_to'])} points, "
          f"{worst:.3g} units from the reference (host {H.worst_error([ref], [1], want['H'][None, :]):.3g})")
    assert worst <= bound["device_factor"] * bound["host_worst_error"]


def test_bad_arguments(capi):
    import ctypes as C
    c = H.cases()["plane_pinhole"]
    lib = capi.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ca, a, b = np.ascontiguousarray(c["cam_a"], dtype=np.float64), c["xy_a"], c["xy_b"]
    out, st = np.full(9, SENTINEL), np.full(1, 77, dtype=np.uint8)
    three = np.arange(3, dtype=np.int32)
    bad = np.array([0, 1, 2, 24], dtype=np.int32)
    invalid = lib.rsba_homography_dlt(0, None, None, None, None, 24, None, 4, 1, None, None)
    assert invalid != 0
    assert lib.rsba_homography_dlt(0, ptr(ca), ptr(ca), ptr(a), ptr(b), 24, ptr(three), 3, 1, ptr(out), ptr(st)) == invalid      # m < 4
    assert lib.rsba_homography_dlt(0, ptr(ca), ptr(ca), ptr(a), ptr(b), 3, ptr(bad), 4, 1, ptr(out), ptr(st)) == invalid        # n < 4
    assert lib.rsba_homography_dlt(0, ptr(ca), ptr(ca), ptr(a), ptr(b), 24, ptr(bad), 4, 1, ptr(out), ptr(st)) == invalid       # an index out of range
    assert lib.rsba_homography_dlt(0, ptr(ca), ptr(ca), ptr(a), ptr(b), 24, ptr(bad), 4, 0, ptr(out), ptr(st)) == invalid
    assert np.all(out == SENTINEL) and st[0] == 77
    with pytest.raises(capi.RsbaError):
        capi.homography_dlt(ca, ca, a, b, bad[None, :])
