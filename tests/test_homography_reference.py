"""The host definitions of the two-view degeneracy test (include/rsba/pair_geometry.hpp: homo_detail::dlt, score, parallax_counts, host_ransac,
classifyPairs and pickBootstrapPair on the host path) against the extended-precision reference of homography_reference.py.  No device: the
C++ is compiled into a stand-alone program (tests/homography_host.cpp) that links nothing of the library.  The device tests
(test_gpu_homography.py, test_gpu_classify_pairs.py) hold the kernels to the same reference with the bound recorded here
(tests/golden/homography_bound.json, written by tests/golden/make_homography_bound.py)."""
import subprocess

import numpy as np
import pytest

import homography_reference as H
from helpers import build_host_program, load_golden


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("homography_host")


@pytest.fixture(scope="module")
def exe(workdir):
    return build_host_program("homography_host", workdir)


@pytest.fixture(scope="module")
def host_cases(exe, workdir):
    cs = H.cases()
    return dict(zip(cs, H.run_host(exe, workdir, list(cs.values()))))


@pytest.fixture(scope="module")
def bound():
    return load_golden("homography_bound.json")


@pytest.mark.parametrize("name", list(H.cases()))
def test_host_dlt_against_the_reference(host_cases, bound, name):
    ref, got = H.reference(name), host_cases[name]
    assert [r["status"] for r in ref] == got["status"].tolist(), [r["why"] for r in ref]
    worst = H.worst_error(ref, got["status"], got["H"])
    print(f"{name}: {int(got['status'].sum())} of {len(ref)} accepted, worst error {worst:.3g} units (recorded {bound['per_case'][name]})")
    assert worst <= bound["per_case"][name] <= bound["host_worst_error"]
    assert not any(r["leave_out"] for r in ref)              # no subset of these cases is too ill-conditioned to compare
    for r, s, h in zip(ref, got["status"], got["H"]):
        if not s:
            assert not h.any()                               # a declined slot is untouched
        else:
            assert abs(np.linalg.norm(h) - 1.0) < 1e-14


def test_the_cases_are_the_ones_the_rules_name(host_cases):
    c = H.cases()
    assert len(c["plane_pinhole"]["subsets"]) == len(c["plane_distorted"]["subsets"]) == 65 and len(c["plane_pinhole"]["xy_a"]) == 24   # a full wave and one lane
    assert c["refit_24_exact"]["subsets"].shape[1] == 24 and c["refit_100_noisy"]["subsets"].shape[1] == 100
    why = [r["why"] for r in H.reference("declined")]
    assert why == list(H.DECLINED) and not host_cases["declined"]["status"].any()   # one subset per way to be declined
    # the pure rotation: every subset accepted, and H is the rotation (up to scale) — which the eight-point rule declines
    rot = host_cases["pure_rotation"]
    assert rot["status"].all()
    Rm = H.R._rodrigues(H.R.POSE_B[:3])
    for h in rot["H"]:
        assert np.max(np.abs(h.reshape(3, 3) / np.linalg.norm(h) - Rm / np.linalg.norm(Rm))) < 1e-4   # (pixels rounded to float, a minimal sample's conditioning)


def test_a_seeded_error_exceeds_the_device_bound(host_cases, bound):
    """a relative error of 1e-6 in one entry of one H is far outside device_factor x host_worst_error: the bound can fail"""
    ref, got = H.reference("plane_distorted"), host_cases["plane_distorted"]
    t = int(np.flatnonzero(got["status"])[7])
    k = int(np.argmax(np.abs(got["H"][t])))
    seeded = got["H"].copy()
    seeded[t, k] *= 1.0 + 1e-6
    assert H.worst_error(ref, got["status"], got["H"]) <= bound["device_factor"] * bound["host_worst_error"] < H.worst_error(ref, got["status"], seeded)


@pytest.fixture(scope="module")
def scoring(exe, workdir):
    s = H.scoring_scene()
    return s, H.run_host_hypotheses(exe, workdir, s, H.SCORING["T"])


def test_scoring_scene_counts_equal_the_reference(scoring, bound):
    """the planar scene with 200 correspondences (three full waves and a tail of 8), 25 % gross outliers, 0.5 px noise: the host form's counts
    of all 64 hypotheses equal the extended-precision rule's, and no correspondence of any scored task is within 1e-9 of a deciding
    threshold — so the device test may compare all 64 counts"""
    s, hyp = scoring
    assert len(s["xy_a"]) == 200 and int((~s["true_inlier"]).sum()) == 50 and len(hyp["status"]) == 64
    nrm = H.normalised_points(s["cam_a"], s["cam_b"], s["xy_a"], s["xy_b"])
    f = H.mean_focal(s["cam_a"], s["cam_b"])
    margins = []
    for t in range(64):
        if not hyp["status"][t]:
            assert hyp["num_inliers"][t] == 0
            continue
        st, count, _, margin, depth = H.score(hyp["H"][t], nrm, f)
        margins.append((min(margin, float(hyp["margin"][t])), min(depth, float(hyp["depth"][t]))))
        assert st == 1 and count == hyp["num_inliers"][t], t
    assert len(margins) >= 16 and max(hyp["num_inliers"]) >= 0.9 * s["true_inlier"].sum()
    print("margins per scored task (relative to the threshold, smallest depth):", [(f"{m:.2g}", f"{d:.2g}") for m, d in margins])
    assert min(m for m, _ in margins) > 1e-9 and min(d for _, d in margins) > 1e-9
    assert hyp["status"].tolist() == bound["scoring"]["status"] and hyp["num_inliers"].tolist() == bound["scoring"]["num_inliers"]


def test_host_loop_on_the_scoring_scene(exe, workdir, scoring, bound):
    s, hyp = scoring
    r = H.run_host_ransac(exe, workdir, s, H.SCORING["iterations"], H.SCORING["refits"])
    best = int(np.argmax(np.where(hyp["status"] == 1, hyp["num_inliers"], -1)))
    assert r["ok"] and r["winner_task"] == best and r["num_inliers"] >= hyp["num_inliers"][best] and r["mask"].sum() == r["num_inliers"]
    assert r["refits_adopted"] >= 1
    assert (r["mask"] & ~s["true_inlier"]).sum() <= 2 and r["num_inliers"] >= 0.95 * s["true_inlier"].sum()   # it found the plane
    assert {k: r[k] for k in ("winner_task", "num_inliers", "refits_adopted")} == bound["scoring"]["loop"]


@pytest.fixture(scope="module")
def classified(exe, workdir):
    pairs = H.classification_pairs()
    rows, pick = H.run_host_classify(exe, workdir, pairs)
    return pairs, rows, pick


def test_classification_of_the_four_pairs_and_the_pure_rotation(classified, bound):
    """one cloud of 200 points, 20 % outliers and 0.5 px noise per pair; min_parallax_deg = 2; the host path"""
    pairs, rows, pick = classified
    a, b, c, d, e = rows
    ratio = lambda r: r["num_h_inliers"] / r["num_inliers"]
    for p, r in zip(pairs, rows):
        print(p["name"], len(p["xy_a"]), r, f"ratio {ratio(r):.3f}" if r["num_inliers"] else "")
    assert all(r["ok"] for r in (a, b, c, d))
    assert a["kind"] == "General"
    assert b["kind"] == "LowParallax" and ratio(b) > 0.8
    assert c["kind"] == "Planar" and ratio(c) > 0.8
    assert d["kind"] == "General" and ratio(d) < 0.8
    assert e["kind"] != "General"
    assert bool(e["ok"]) == bound["classify"]["pure_rotation_accepted_by_the_essential_ransac"]
    # (b) shares (a)'s cloud and loses fewer points to the image border: the plain pick prefers the pair without a baseline
    assert len(pairs[1]["xy_a"]) > len(pairs[0]["xy_a"]) and b["essential_front"] > a["essential_front"]
    assert pick == [1, 0]
    assert {p["name"]: r for p, r in zip(pairs, rows)} == bound["classify"]["pairs"]


def test_parallax_counts_equal_the_reference(exe, workdir, classified):
    """the host parallax counts of the true geometry of pairs (a) and (b) against the extended-precision rule, no comparison within 1e-9 of
    its threshold"""
    pairs, _, _ = classified
    cos_min = float(np.cos(np.radians(H.CLASSIFY["min_parallax_deg"])))
    E, poses = [], []
    for scale in (0.3, 0.01):
        pose = np.concatenate([H.ROTATION, scale * H.MEAN_DEPTH * H.DIRECTION])
        Rm = H.R._rodrigues(pose[:3]); t = -Rm @ pose[3:]; t /= np.linalg.norm(t)
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        E.append((tx @ Rm).reshape(-1)); poses.append(np.concatenate([pose[:3], pose[3:] / np.linalg.norm(pose[3:])]))
    got = H.run_host_parallax(exe, workdir, pairs[:2], E, poses, [1, 1], cos_min)
    for k, p in enumerate(pairs[:2]):
        nrm = H.normalised_points(p["cam_a"], p["cam_b"], p["xy_a"], p["xy_b"])
        front, par, margin = H.parallax_counts(E[k], poses[k], nrm, H.mean_focal(p["cam_a"], p["cam_b"]), cos_min)
        print(p["name"], front, par, f"margin {margin:.3g} (host {got['margin'][k]:.3g})")
        assert min(margin, got["margin"][k]) > 1e-9
        assert (front, par) == (got["num_front"][k], got["num_parallax"][k])
    assert got["num_parallax"][0] > 0.9 * got["num_front"][0] and got["num_parallax"][1] == 0   # 0.3 of the depth against 0.01 of it, at 2 degrees
    none = H.run_host_parallax(exe, workdir, pairs[:1], E[:1], poses[:1], [0], cos_min)
    assert none["num_front"][0] == 0 and none["num_parallax"][0] == 0


def test_host_program_under_the_sanitizers(workdir, tmp_path):
    """the host definitions once more with -fsanitize=address,undefined, run as a stand-alone program over the case file, the scoring scene
    and the classification pairs: a clean exit"""
    exe = build_host_program("homography_host", tmp_path, extra_flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    cs = H.cases()
    H.run_host(exe, tmp_path, list(cs.values()))
    s = H.scoring_scene()
    H.run_host_hypotheses(exe, tmp_path, s, 8)
    H.run_host_ransac(exe, tmp_path, s, 16, 2)
    H.run_host_classify(exe, tmp_path, H.classification_pairs()[:2], dict(H.CLASSIFY, iterations=20))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "ERROR" not in r.stderr
