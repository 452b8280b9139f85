"""The host definitions of the five-point solver (include/rsba/two_view.hpp: epi_detail::five_point, five_point_hypothesis, host_ransac with
solver = FivePoint) against the extended-precision reference of tests/five_point_reference.py, on the case list the device test shares, and
the host RANSAC loop on the outlier scenes and on a planar scene.  No GPU.

What is recorded (tests/golden/five_point_bound.json, written by tests/golden/make_five_point_bound.py): the host fp64 code's worst
|value_k - reference_k| / unit_k, unit_k = (kappa_k + |value_k|) 2^-52, over every solution (up to sign) of every accepted subset and the
pose of the chosen one; the host loop's distance to the true relative pose per outlier scene; and on how many of the 32 runs each loop ends
with 0.9 of the true inliers.  The device bound is the first figure times 4; nothing in it comes from device output.

The case list is two_view_reference.cases() cut to the first five indices, with one change: sideways_no_rotation is drawn from seed 26, not
17.  With exact data and no rotation the subsets have spurious solutions close to a double root, and on seed 17 two of the five subsets
have kappa above 1e6 (1.4e6, 1.1e6); on seed 22 one subset has its true solution at infinity in the solver's chart (no component along the
fourth null vector, which exact data can do and noisy data cannot), which the rule declines as not finite.  Seed 26 has neither."""
import numpy as np
import pytest

import five_point_reference as F
import two_view_reference as R
from helpers import build_host_program, load_golden

MODES = {1: "the factor 1/2 of the trace term dropped", 2: "E transposed", 3: "the Newton steps and the polish removed"}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """mode -> {case name: per-subset results} from tests/five_point_host.cpp, compiled here"""
    d = tmp_path_factory.mktemp("five_point")
    exe = build_host_program("five_point_host", d)
    cs = F.cases()
    return {mode: dict(zip(cs, F.run_host(exe, d, list(cs.values()), mode))) for mode in (0, 1, 2, 3)}, exe, d


def test_the_case_list_covers_what_it_must():
    cs = F.cases()
    for name in R.RANDOM_CASES:
        assert cs[name]["subsets"].shape == (65, 5) and len(cs[name]["xy_a"]) == 24 and cs[name]["xy_a"].dtype == np.float32
    assert cs["single"]["subsets"].shape == (1, 5) and len(cs["single"]["xy_a"]) == 5 and F.reference("single")[0]["status"] == 1
    # a repeated index, five coplanar points (accepted), a pure rotation, coincident points, five ordinary points
    assert [r["status"] for r in F.reference("degenerate")] == [0, 1, 0, 0, 1]
    for name in cs:
        for t, r in enumerate(F.reference(name)):
            assert not r["leave_out"], (name, t, r["kappa_max"])                           # no subset is left out of the accuracy check
            # no subset sits on a threshold that decides its status (1e-7 both): accepted ones two orders above, declined ones two below
            assert r["rank_gap"] is None or not 1e-9 < r["rank_gap"] < 1e-5, (name, t, r["rank_gap"])
            assert r["elim_gap"] is None or not 1e-9 < r["elim_gap"] < 1e-5, (name, t, r["elim_gap"])
            if r["status"]:
                assert len(r["E"]) in (2, 4, 6, 8, 10), (name, t)
                assert r["root_gap"] > 1e-3, (name, t, r["root_gap"])                      # no double root, real or about to be
                assert r["key_gap"] is None or r["key_gap"] > 1e-4, (name, t, r["key_gap"])   # the order of the solutions is not in doubt


def test_the_generating_motion_is_among_the_solutions():
    """noise-free data rounded to float: within 1.7e-4 (Frobenius, unit norm, up to sign).  (It need not be the chosen one: a second
    solution may keep all 24 correspondences within 4 px too, and the tie goes to the first.)"""
    cs = F.cases()
    for name in F.NOISE_FREE:
        truth = F.essential_of(cs[name]["pose"])
        for t, r in enumerate(F.reference(name)):
            assert r["status"] == 1, (name, t)
            dist = [min(np.linalg.norm(np.array(e) - truth), np.linalg.norm(np.array(e) + truth)) for e in r["E"]]
            assert min(dist) <= 1.7e-4, (name, t, min(dist))


def test_host_gives_the_reference_status_and_count_everywhere(host):
    results = host[0][0]
    for name in F.cases():
        ref = F.reference(name)
        assert list(results[name]["status"]) == [r["status"] for r in ref], name
        assert list(results[name]["count"]) == [len(r["E"]) for r in ref], name
        assert list(results[name]["chain"]) == [r["status"] for r in ref], name
        assert list(results[name]["chosen"]) == [r["chosen"] if r["status"] else -1 for r in ref], name


def _per_case(results):
    return {name: F.worst_error(F.reference(name), results[name]["status"], results[name]["count"], results[name]["E"], results[name]["poses"]) for name in F.cases()}


def test_host_error_is_on_record(host):
    per_case = _per_case(host[0][0])
    print("host five_point / five_point_hypothesis, worst error in units per case:", {k: float(f"{v:.3g}") for k, v in per_case.items()})
    rec = load_golden("five_point_bound.json")
    worst = max(per_case.values())
    general = max(v for k, v in per_case.items() if k != "sideways_no_rotation")
    # the record is what this host code measures (other compilers / maths libraries move the last digits, not the size)
    assert worst <= rec["host_worst_error"] <= 2.0 * worst, (worst, rec)
    assert general <= rec["host_worst_error_general"] <= 2.0 * general, (general, rec)
    assert rec["device_factor"] == 4


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_seeded_error_exceeds_the_device_bound(host, mode):
    """against the bound of every case, and — for what only the cases with a meaningful unit can show — against the general one"""
    results = host[0][mode]
    rec = load_golden("five_point_bound.json")
    over = []
    for name in F.cases():
        ref = F.reference(name)
        h = results[name]
        same = np.array([r["status"] == h["status"][t] and len(r["E"]) == h["count"][t] for t, r in enumerate(ref)])
        w = F.worst_error(ref, h["status"], h["count"], h["E"])
        bound = rec["device_factor"] * (rec["host_worst_error"] if name == "sideways_no_rotation" else rec["host_worst_error_general"])
        if w > bound or not same.all():
            over.append((name, float(f"{w:.3g}"), int((~same).sum())))
    print(MODES[mode], "-> cases above the device bound (worst in units, subsets with another status or count):", over)
    assert over, MODES[mode]
    if mode != 3:   # these two are wrong by the size of E itself: also above the bound that sideways_no_rotation sets
        assert any(w > rec["device_factor"] * rec["host_worst_error"] or bad for _, w, bad in over)


@pytest.fixture(scope="module")
def loops(host):
    """(scene, five-point result, eight-point result) per (fb, rolling, draw)"""
    _, exe, d = host
    out = {}
    for fb, rolling in R.OUTLIER_SCENES:
        for draw in range(8):
            s = F.outlier_draw(fb, rolling, draw)
            out[(fb, rolling, draw)] = (s, F.run_host_ransac(exe, d, s, 5), F.run_host_ransac(exe, d, s, 8))
    return out


def _succeeds(s, r):
    return bool(r["ok"] and (r["mask"] & s["true_inlier"]).sum() >= 0.9 * s["true_inlier"].sum())


def test_the_five_point_loop_succeeds_at_least_as_often_as_the_eight_point_loop(loops):
    """four outlier scenes x eight draws of the 40 % outliers, 1000 subsets each, the refits what they are"""
    five = sum(_succeeds(s, r5) for s, r5, _ in loops.values())
    eight = sum(_succeeds(s, r8) for s, _, r8 in loops.values())
    print(f"runs of 32 that end with 0.9 of the true inliers: five-point {five}, eight-point {eight}; five-point misses:",
          [k for k, (s, r5, _) in loops.items() if not _succeeds(s, r5)])
    rec = load_golden("five_point_bound.json")["ransac"]
    assert five >= eight
    assert (five, eight) == (rec["five_point_successes"], rec["eight_point_successes"])


@pytest.mark.parametrize("fb,rolling", R.OUTLIER_SCENES)
def test_host_five_point_ransac_on_an_outlier_scene(loops, fb, rolling):
    """draw 0, the committed scenes: everything test_two_view_reference.py asks of the eight-point loop there"""
    s, r, _ = loops[(fb, rolling, 0)]
    true = int(s["true_inlier"].sum())
    found = int((r["mask"] & s["true_inlier"]).sum())
    good = R.reprojecting_inliers(s, r["pose"], r["mask"])
    rot, base = R.distance_to_truth(r["pose"], s)
    print(f"frames (0, {fb}) rolling={rolling}: n {len(s['xy_a'])}, true inliers {true}, winner task {r['winner_task']}, refits adopted {r['refits_adopted']}, "
          f"inliers {r['num_inliers']} ({found} true), in front {r['num_front']}, reprojecting {good}, rotation {rot:.3f} deg, baseline {base:.3f} deg, "
          f"nearest to the threshold {np.min(np.abs(r['ratio'] - 1.0)):.2e}")
    assert r["ok"] and r["num_inliers"] == int(r["mask"].sum())
    assert found >= 0.9 * true
    assert good >= 0.9 * r["num_inliers"]
    assert r["num_front"] >= 0.9 * r["num_inliers"]
    assert np.min(np.abs(r["ratio"] - 1.0)) > 1e-9
    rec = load_golden("five_point_bound.json")["ransac"]["scenes"][R.scene_name(fb, rolling)]
    assert rot <= rec["rotation_deg"] <= 2.0 * max(rot, 1e-3) and base <= rec["baseline_deg"] <= 2.0 * max(base, 1e-3)


@pytest.mark.parametrize("seed", range(6))
def test_host_five_point_ransac_on_a_planar_scene(host, seed):
    """60 noisy correspondences of one plane: the eight-point rule declines every sample, the five-point loop starts the video.  A plane
    admits a twin motion, so the pose is not compared with the truth."""
    _, exe, d = host
    s = F.planar_scene(seed)
    r = F.run_host_ransac(exe, d, s, 5, name="planar")
    r8 = F.run_host_ransac(exe, d, s, 8, name="planar")
    good = R.reprojecting_inliers(s, r["pose"], r["mask"])
    rot, base = R.distance_to_truth(r["pose"], s)
    print(f"planar seed {seed}: five-point ok {r['ok']}, inliers {r['num_inliers']} of 60, in front {r['num_front']}, reprojecting {good}, refits adopted "
          f"{r['refits_adopted']}, rotation {rot:.2f} deg, baseline {base:.2f} deg; eight-point ok {r8['ok']}, winner task {r8['winner_task']}, inliers {r8['num_inliers']}")
    assert r["ok"]
    assert r["num_inliers"] >= 0.9 * 60
    assert r["num_front"] >= 0.9 * r["num_inliers"]
    assert good >= 0.9 * r["num_inliers"]
