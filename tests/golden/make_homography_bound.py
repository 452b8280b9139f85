#!/usr/bin/env python3
"""Writes tests/golden/homography_bound.json, measured on the CPU — no device output is read:
  host_worst_error   the worst error of the host fp64 homo_detail::dlt (include/rsba/pair_geometry.hpp) against the extended-precision
                     reference of tests/homography_reference.py over the case list, in the reference's units (kappa_k + |value_k|) 2^-52,
                     H at unit Frobenius norm and the rule's sign; per case and overall.  Thousands of units for the minimal samples, as
                     for the eight-point rule and for the same reason: kappa is the conditioning of the null vector in the constraint
                     matrix, the host code takes it from the Gram matrix, whose eigenvalue gap is the square of the singular-value gap.
                     The device kernel restates the same arithmetic in another operation order (the symmetric Jacobi update, fused
                     multiply-adds), so it gets that figure times device_factor = 4, the eight-point kernels' factor.
  scoring            the host form's counts of the 64 hypotheses of the scoring scene, the smallest margin of any correspondence of any
                     scored task to a deciding threshold, and the host loop's result on that scene
  classify           what the host path makes of the five classification pairs (five-point essential subsets), both picks, and — recorded,
                     not prescribed — whether the essential RANSAC accepts the exact pure rotation, and the kinds with the default
                     eight-point subsets (the plane of pair (c) then has no stable E: its kind is not Planar)."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import homography_reference as H  # noqa: E402
from helpers import build_host_program  # noqa: E402


def measure():
    cs = H.cases()
    with tempfile.TemporaryDirectory() as d:
        exe = build_host_program("homography_host", d)
        got = H.run_host(exe, d, list(cs.values()))
        per_case = {name: H.worst_error(H.reference(name), h["status"], h["H"]) for name, h in zip(cs, got)}
        s = H.scoring_scene()
        hyp = H.run_host_hypotheses(exe, d, s, H.SCORING["T"])
        loop = H.run_host_ransac(exe, d, s, H.SCORING["iterations"], H.SCORING["refits"])
        scoring = {"status": hyp["status"].tolist(), "num_inliers": hyp["num_inliers"].tolist(), "min_margin": float(f"{hyp['margin'][hyp['status'] == 1].min():.3g}"),
                   "min_depth": float(f"{hyp['depth'][hyp['status'] == 1].min():.3g}"),
                   "loop": {"winner_task": loop["winner_task"], "num_inliers": loop["num_inliers"], "refits_adopted": loop["refits_adopted"]}}
        pairs = H.classification_pairs()
        rows, pick = H.run_host_classify(exe, d, pairs)
        rows8, pick8 = H.run_host_classify(exe, d, pairs, dict(H.CLASSIFY, solver=8))
        classify = {"pairs": {p["name"]: r for p, r in zip(pairs, rows)}, "pick_plain": pick[0], "pick_geometry": pick[1],
                    "pure_rotation_accepted_by_the_essential_ransac": bool(rows[4]["ok"]),
                    "eight_point_subsets": {"kinds": {p["name"]: r["kind"] for p, r in zip(pairs, rows8)}, "pick_plain": pick8[0], "pick_geometry": pick8[1]}}
    return per_case, scoring, classify


def main():
    per_case, scoring, classify = measure()
    rec = {"host_worst_error": float(f"{max(per_case.values()) * 1.01:.3g}"),
           "device_factor": 4,
           "per_case": {k: float(f"{v * 1.01:.3g}") for k, v in per_case.items()},
           "scoring": scoring,
           "classify": classify,
           "what": "host_worst_error: worst |value_k - reference_k| / ((kappa_k + |value_k|) 2^-52) of the host fp64 homo_detail::dlt over "
                   "tests/homography_reference.py cases(), H at unit Frobenius norm and the rule's sign; scoring, classify: the host path on the scoring scene "
                   "and the classification pairs"}
    with open(os.path.join(HERE, "homography_bound.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
