#!/usr/bin/env python3
"""Writes tests/golden/five_point_bound.json, measured on the CPU — no device output is read:
  host_worst_error   the worst error of the host fp64 epi_detail::five_point / five_point_hypothesis (include/rsba/two_view.hpp) against the
                     extended-precision reference of tests/five_point_reference.py over the case list, in the reference's units
                     (kappa_k + |value_k|) 2^-52, over every solution (up to sign) and the chosen solution's pose.  The device kernel
                     restates the same arithmetic, so it gets that figure times device_factor = 4.
                     The figure is set by sideways_no_rotation alone: with exact data and no rotation the true E = [t]x has entries that
                     are zero and whose first derivative in every input is zero too (E00 = t0 w0 - t.w for a small rotation w), so their
                     unit is some 1e-26 and a last-bit error of 1e-17 counts as 1e9 units.  Every other case stays below a hundred:
  host_worst_error_general   the same maximum over the cases other than sideways_no_rotation, which the device test holds those cases
                     to as well (times device_factor): the bound that sees a missing polish.
  ransac             the host five-point loop's distance to the true relative pose on the four outlier scenes (draw 0), and on how many of
                     the 32 runs (four scenes x eight draws of the outliers) each loop ends with at least 0.9 of the true inliers."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import five_point_reference as F  # noqa: E402
import two_view_reference as R  # noqa: E402
from helpers import build_host_program  # noqa: E402


def successes(exe, d, solver):
    """per (scene, draw): the run ends ok with at least 0.9 of the true inliers"""
    out = {}
    for fb, rolling in R.OUTLIER_SCENES:
        for draw in range(8):
            s = F.outlier_draw(fb, rolling, draw)
            r = F.run_host_ransac(exe, d, s, solver)
            out[(fb, rolling, draw)] = bool(r["ok"] and (r["mask"] & s["true_inlier"]).sum() >= 0.9 * s["true_inlier"].sum())
    return out


def measure():
    cs = F.cases()
    with tempfile.TemporaryDirectory() as d:
        exe = build_host_program("five_point_host", d)
        got = F.run_host(exe, d, list(cs.values()))
        per_case = {name: F.worst_error(F.reference(name), h["status"], h["count"], h["E"], h["poses"]) for name, h in zip(cs, got)}
        ransac = {}
        for fb, rolling in R.OUTLIER_SCENES:
            s = R.outlier_scene(fb, rolling)
            ransac[R.scene_name(fb, rolling)] = R.distance_to_truth(F.run_host_ransac(exe, d, s, 5)["pose"], s)
        counts = {solver: sum(successes(exe, d, solver).values()) for solver in (8, 5)}
    return per_case, ransac, counts


def main():
    per_case, ransac, counts = measure()
    general = max(v for k, v in per_case.items() if k != "sideways_no_rotation")
    rec = {"host_worst_error": float(f"{max(per_case.values()) * 1.005:.3g}"),
           "host_worst_error_general": float(f"{general * 1.005:.3g}"),
           "device_factor": 4,
           "per_case": {k: float(f"{v:.3g}") for k, v in per_case.items()},
           "ransac": {"device_factor": 2, "runs": 32, "eight_point_successes": counts[8], "five_point_successes": counts[5],
                      "scenes": {k: {"rotation_deg": float(f"{v[0] * 1.005:.3g}"), "baseline_deg": float(f"{v[1] * 1.005:.3g}")} for k, v in ransac.items()}},
           "what": "host_worst_error: worst |value_k - reference_k| / ((kappa_k + |value_k|) 2^-52) of the host fp64 epi_detail::five_point and "
                   "five_point_hypothesis over tests/five_point_reference.py cases(), every solution up to sign and the chosen one's pose; "
                   "host_worst_error_general: the same without sideways_no_rotation; ransac: the host five-point loop's distance to the true "
                   "relative pose on the outlier scenes, and the runs of 32 that end with 0.9 of the true inliers per loop"}
    with open(os.path.join(HERE, "five_point_bound.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
