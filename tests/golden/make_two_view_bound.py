#!/usr/bin/env python3
"""Writes tests/golden/two_view_bound.json, measured on the CPU — no device output is read:
  host_worst_error   the worst error of the host fp64 epi_detail::eight_point / score (include/rsba/two_view.hpp) against the
                     extended-precision reference of tests/two_view_reference.py over the case list, in the reference's units
                     (kappa_k + |value_k|) 2^-52, over E (up to sign) and the pose.  The figure is thousands of units, not tens: kappa is the
                     conditioning of the null vector in the constraint matrix, the host code takes it from the Gram matrix, whose eigenvalue
                     gap is the square of the singular-value gap — an eight-point subset with kappa in the thousands loses that factor again.
                     It is first order in the rounding all the same, so no case is recorded apart.
                     The device kernel restates the same arithmetic in another operation order (the symmetric Jacobi update, fused
                     multiply-adds), so it gets that figure times device_factor = 4.
  ransac             the host loop's distance to the true relative pose on the four outlier scenes: rotation angle and angle between the
                     baseline directions, degrees.  The device loop sees the same noisy data; and borderline inliers differ:
                     truth_factor = 2."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import two_view_reference as R  # noqa: E402
from helpers import build_host_program  # noqa: E402


def measure():
    cs = R.cases()
    with tempfile.TemporaryDirectory() as d:
        exe = build_host_program("two_view_host", d)
        got = R.run_host(exe, d, list(cs.values()))
        per_case = {name: R.worst_error(R.reference(name), h["status"], h["E"], h["poses"]) for name, h in zip(cs, got)}
        ransac = {}
        for fb, rolling in R.OUTLIER_SCENES:
            s = R.outlier_scene(fb, rolling)
            ransac[R.scene_name(fb, rolling)] = R.distance_to_truth(R.run_host_ransac(exe, d, s)["pose"], s)
    return per_case, ransac


def main():
    per_case, ransac = measure()
    rec = {"host_worst_error": float(f"{max(per_case.values()) * 1.005:.3g}"),
           "device_factor": 4,
           "per_case": {k: float(f"{v:.3g}") for k, v in per_case.items()},
           "ransac": {"device_factor": 2,
                      "scenes": {k: {"rotation_deg": float(f"{v[0] * 1.005:.3g}"), "baseline_deg": float(f"{v[1] * 1.005:.3g}")} for k, v in ransac.items()}},
           "what": "host_worst_error: worst |value_k - reference_k| / ((kappa_k + |value_k|) 2^-52) of the host fp64 epi_detail::eight_point and score over "
                   "tests/two_view_reference.py cases(), E up to sign and the pose; ransac: the host loop's distance to the true relative pose on the outlier scenes"}
    with open(os.path.join(HERE, "two_view_bound.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
