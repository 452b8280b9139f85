"""The host minimal solver (include/rsba/solve_rs_pnp.hpp: pnp_detail::p3p_pose) against the extended-precision reference of
tests/p3p_reference.py, on the case list the device test shares.  No GPU.

What is recorded (tests/golden/p3p_bound.json, written by tests/golden/make_p3p_bound.py): the host fp64 code's worst
|pose_k - reference_k| / unit_k, unit_k = (kappa_k + |pose_k|) 2^-52, over every accepted subset of every case — half_turn apart, see the
script.  The device bound is that figure times 4; nothing in it comes from device output."""
import subprocess

import numpy as np
import pytest

import p3p_reference as R
from helpers import build_host_program, load_golden

RANDOM_CASES = ("main_pinhole", "main_distorted")
APART = ("half_turn", "sliver")   # recorded apart in p3p_bound.json (tests/golden/make_p3p_bound.py says why)


def record(name):
    rec = load_golden("p3p_bound.json")
    return rec["host_worst_error_" + name] if name in APART else rec["host_worst_error"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """mode -> {case name: (status, num_solutions, poses)} from tests/p3p_host.cpp, compiled here"""
    d = tmp_path_factory.mktemp("p3p")
    exe = build_host_program("p3p_host", d)
    cs = R.cases()
    return {mode: dict(zip(cs, R.run_host(exe, d, list(cs.values()), mode))) for mode in (0, 1, 2, 3)}, exe, d


def test_the_case_list_covers_what_it_must():
    cs = R.cases()
    for name in RANDOM_CASES:
        ref = R.reference(name)
        assert cs[name]["subsets"].shape == (65, 4) and len(cs[name]["X"]) == 24
        left = [t for t, r in enumerate(ref) if r["leave_out"]]
        assert len(left) <= 3, (name, left)                                                # the cap on what the accuracy check may leave out
        assert all(r["status"] == 1 for r in ref)
        # noise-free data: the chosen solution is the pose that made the observations (float32 coordinates; kappa of a few thousand)
        for t, r in enumerate(ref):
            if not r["leave_out"]:
                assert np.max(np.abs(np.array(r["pose"]) - cs[name]["pose"])) <= 1e-3, (name, t)
    assert any(cs["main_distorted"]["cam"][2:7] != 0) and not any(cs["main_pinhole"]["cam"][2:7] != 0)
    assert cs["single"]["subsets"].shape == (1, 4) and len(cs["single"]["X"]) == 4 and R.reference("single")[0]["status"] == 1
    assert all(r["status"] == 1 and np.max(np.abs(r["pose"][:3])) <= 1e-12 for r in R.reference("identity"))           # the small-angle branch
    assert all(r["status"] == 1 and abs(np.linalg.norm(r["pose"][:3]) - np.pi) <= 1e-6 for r in R.reference("half_turn"))
    assert all(r["num_solutions"] == 4 for r in R.reference("four_roots"))
    deg = R.reference("degenerate")
    assert [r["status"] for r in deg] == [0, 0, 0, 0, 0, 0, 1, 0, 1] and all(r["num_solutions"] == 0 for r in deg if not r["status"])
    # the two subsets declined for the fourth point: their triple has solutions with positive depths, every one puts the fourth point behind
    c = cs["degenerate"]
    for t in (5, 7):
        swapped = R.solve_one(c["cam"], c["X"], c["xy"], list(c["subsets"][t][:3]) + [3], want_kappa=False)
        assert swapped["status"] == 1 and swapped["num_solutions"] >= 1
    assert all(r["status"] == 1 for r in R.reference("lost_leading_coefficient"))
    # the collinearity threshold, 1e-4 on the singular values of the centred triple, from either side
    sl = cs["sliver"]
    ratios = [np.linalg.svd((lambda P: P - P.mean(axis=0))(sl["X"][s[:3]].astype(np.float64)), compute_uv=False) for s in sl["subsets"]]
    assert 0.6e-4 < ratios[0][1] / ratios[0][0] < 0.8e-4 and 1.4e-4 < ratios[1][1] / ratios[1][0] < 1.6e-4
    assert [r["status"] for r in R.reference("sliver")] == [0, 1]
    # no case outside the random ones leans on the leave-out rule
    assert not any(r["leave_out"] for name in cs if name not in RANDOM_CASES for r in R.reference(name))


def test_the_leading_coefficient_is_lost_where_the_header_says():
    """A4 = ((a^2 - c^2) / b^2 - 1)^2 - 4 (c^2 / b^2) cos(alpha)^2 of the first four subsets of the case, from the case's own floats"""
    c = R.cases()["lost_leading_coefficient"]
    for t in range(4):
        idx = c["subsets"][t]
        P = [[R.mpf(float(c["X"][i, k])) for k in range(3)] for i in idx[:3]]
        J = [R._bearing(*R.normalise(c["cam"], c["xy"][i, 0], c["xy"][i, 1])) for i in idx[:3]]
        a2, b2, c2, ca, cb, cg = R._triangle(P, J)
        A4 = ((a2 - c2) / b2 - 1) ** 2 - 4 * c2 / b2 * ca * ca
        A0 = ((a2 - c2) / b2 + 1) ** 2 - 4 * a2 / b2 * cg * cg
        assert (a2 - c2) / b2 == 1 and abs(A4) <= 1e-12 * abs(A0), (t, float(A4), float(A0))


def test_host_gives_the_reference_status_and_solution_count_everywhere(host):
    results = host[0][0]
    for name in R.cases():
        status, nsol, _ = results[name]
        ref = R.reference(name)
        assert list(status) == [r["status"] for r in ref], name
        assert list(nsol) == [r["num_solutions"] for r in ref], name


def test_host_error_is_on_record(host):
    results = host[0][0]
    per_case = {name: R.worst_error(R.reference(name), results[name][0], results[name][2]) for name in R.cases()}
    print("host p3p_pose, worst error in units per case:", {k: float(f"{v:.3g}") for k, v in per_case.items()})
    rec = load_golden("p3p_bound.json")
    regular = max(v for k, v in per_case.items() if k not in APART)
    # the record is what this host code measures (other compilers / maths libraries move the last digits, not the size)
    assert regular <= rec["host_worst_error"] <= 2.0 * regular, (regular, rec)
    for name in APART:
        assert per_case[name] <= rec["host_worst_error_" + name] <= 2.0 * max(per_case[name], 1.0), (name, per_case[name], rec)
    assert rec["device_factor"] == 4


@pytest.mark.parametrize("mode,what", [(1, "the runner-up solution chosen"), (2, "the polish of the depths dropped"), (3, "the bearing (x, y, 1) not normalised")])
def test_a_seeded_error_exceeds_the_device_bound(host, mode, what):
    results = host[0][mode]
    rec = load_golden("p3p_bound.json")
    over = []
    for name in R.cases():
        status, _, poses = results[name]
        w = R.worst_error(R.reference(name), status, poses)
        if w > rec["device_factor"] * record(name):
            over.append((name, float(f"{w:.3g}")))
    print(what, "-> cases above the device bound:", over)
    assert over, what


def test_the_subset_generator_is_the_restated_one(host):
    """solveGsPnPRansacP3P scores through the device, so only its sampling is checked here: hyp_detail::distinct_subsets against cv::RNG's
    multiply-with-carry and the distinct-index loop of solveGsPnPRansac, restated"""
    _, exe, _ = host
    for n, m, it, state in ((5, 4, 40, 0x9e3779b97f4a7c15), (200, 4, 500, 0x9e3779b97f4a7c15), (24, 6, 30, 0xffffffff)):
        out = subprocess.run([exe, "subsets", str(n), str(m), str(it), str(state)], check=True, capture_output=True, text=True).stdout
        got = np.array([[int(x) for x in line.split()] for line in out.strip().split("\n")])
        s, want = state, []
        for _ in range(it):
            pick = []
            while len(pick) < m:
                s = ((s & 0xffffffff) * 4164903690 + (s >> 32)) & 0xffffffffffffffff
                c = (s & 0xffffffff) % n
                if c not in pick:
                    pick.append(c)
            want.append(pick)
        assert np.array_equal(got, np.array(want)), (n, m)
        assert all(len(set(r)) == m for r in got.tolist())

