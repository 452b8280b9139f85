"""The host DLT start pose (include/rsba/solve_rs_pnp.hpp: pnp_detail::dlt_pose) against the extended-precision restatement of
tests/pnp_dlt_reference.py, on the case list the device test shares.  No GPU.

What is recorded: the host fp64 code's worst |pose - reference| / (kappa eps) over every accepted subset of every case, kappa =
gap[2] / gap[1] of the reference's 12 x 12 eigenproblem (the planar branch: the homography's), eps = 2^-52.  The figure lives in
tests/golden/pnp_dlt_bound.json (RSBA_RECORD_PNP_DLT_BOUND=1 makes this test rewrite it; otherwise the test checks that the record
is what it measures).  The device kernel applies the same rotations in another operation order (symmetric update on the triangle, fused
multiply-adds), so its bound is that ratio times 4 — derived from the host code and the reference, never from device output."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import pnp_dlt_reference as R
from helpers import GOLDEN, build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_FILE = os.path.join(GOLDEN, "pnp_dlt_bound.json")


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    """name -> [(accepted, pose)] from the C++ dlt_pose, compiled here (host code only: nothing of the library is linked)"""
    d = tmp_path_factory.mktemp("pnp_dlt")
    exe = build_host_program("pnp_dlt_host", d)
    cs = R.cases()
    with open(d / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs.values():
            T, m = c["subsets"].shape
            f.write(struct.pack("<3i", len(c["X"]), m, T)); f.write(np.asarray(c["cam"], dtype="<f8").tobytes())
            f.write(c["X"].astype("<f4").tobytes()); f.write(c["xy"].astype("<f4").tobytes()); f.write(c["subsets"].astype("<i4").tobytes())
    lines = subprocess.run([exe, str(d / "cases.bin")], check=True, capture_output=True, text=True).stdout.split("\n")
    out, k = {}, 0
    for name, c in cs.items():
        rows = [lines[k + t].split() for t in range(len(c["subsets"]))]
        k += len(c["subsets"])
        out[name] = [(int(r[0]), np.array([float(x) for x in r[1:]])) for r in rows]
    return out


def test_every_tested_ratio_is_a_factor_two_from_its_threshold():
    """no case sits where fp64 and extended precision could legitimately take different branches; no case is excluded"""
    seen = set()
    for name in R.cases():
        for t, ref in enumerate(R.reference(name)):
            for key, value in ref["ratios"].items():
                thr = R.THRESHOLDS[key]
                assert value >= 2 * thr or value <= 0.5 * thr, (name, t, key, value)
            seen.add(ref["branch"])
    assert seen == {0, 1, 2}


def test_the_case_list_covers_what_it_must():
    cs = R.cases()
    main = R.reference("main_distorted")
    assert cs["main_distorted"]["subsets"].shape == (65, 6) and len(cs["main_distorted"]["X"]) == 40
    assert all(r["branch"] == 1 for r in main[:48]) and all(r["branch"] == 2 for r in main[48:54])
    assert all(r["branch"] == 0 and list(r["ratios"]) == ["val1/val2"] for r in main[54:57])          # the line: declined on the scatter
    assert all(r["branch"] == 0 and "gap1/gap2" in r["ratios"] for r in main[57:61])                   # a point named twice: a second null direction
    assert cs["m12"]["subsets"].shape[1] == 12 and cs["m_all"]["subsets"].shape == (1, 40) and cs["single"]["subsets"].shape == (1, 6)
    assert all(r["branch"] == 1 for name in ("m12", "m_all", "single") for r in R.reference(name))
    assert any(cs["main_distorted"]["cam"][2:7] != 0) and not any(cs["main_plain"]["cam"][2:7] != 0)
    for c, ref in zip(("main_distorted", "main_plain", "m12", "m_all", "half_turn"), map(R.reference, ("main_distorted", "main_plain", "m12", "m_all", "half_turn"))):
        for r in ref:   # noise-free data: every accepted subset recovers the pose that made the observations (float32 coordinates: ~1e-7 kappa)
            if r["branch"]:
                assert np.max(np.abs(np.array(r["pose"]) - cs[c]["pose"])) <= 1e-7 * r["kappa"], (c, r)
    half = R.reference("half_turn")
    assert all(r["branch"] == 1 and abs(np.linalg.norm(r["pose"][:3]) - np.pi) <= 1e-12 for r in half)


def measured_ratio(host_results):
    worst = 0.0
    for name in R.cases():
        for t, (ref, (ok, pose)) in enumerate(zip(R.reference(name), host_results[name])):
            assert ok == (ref["branch"] != 0), (name, t, ok, ref)          # the same branch everywhere (the host reports accepted / declined)
            if ok:
                worst = max(worst, float(np.max(np.abs(pose - np.array(ref["pose"])))) / (ref["kappa"] * R.EPS))
    return worst


def test_host_dlt_takes_the_reference_branches_and_its_error_is_on_record(host_results):
    worst = measured_ratio(host_results)
    print(f"host dlt_pose: worst |pose - reference| / (kappa eps) = {worst:.4g}")
    if os.environ.get("RSBA_RECORD_PNP_DLT_BOUND"):
        with open(BOUND_FILE, "w") as f:
            json.dump({"host_worst_error_over_kappa_eps": float(f"{worst * 1.005:.3g}"), "device_factor": 4,
                       "what": "worst |pose - reference| / (kappa eps) of the host fp64 pnp_detail::dlt_pose over tests/pnp_dlt_reference.py cases()"}, f, indent=1)
            f.write("\n")
    with open(BOUND_FILE) as f:
        rec = json.load(f)
    # the record is what this host code measures (other compilers / maths libraries move the last digits, not the size)
    assert worst <= rec["host_worst_error_over_kappa_eps"] <= 2.0 * worst, (worst, rec)
    assert rec["device_factor"] == 4
