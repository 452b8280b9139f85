#!/usr/bin/env python3
"""Writes tests/golden/p3p_bound.json: the worst error of the host fp64 pnp_detail::p3p_pose against the extended-precision reference of
tests/p3p_reference.py over the case list, in the reference's units (kappa_k + |pose_k|) 2^-52, measured on the CPU — no device output
is read.  The device kernel restates the same arithmetic in another operation order (fused multiply-adds, the world triangle's triad
hoisted), so it gets that figure times device_factor = 4.
The half_turn case is recorded apart and bounds only itself: pose_from_rt takes the angle from acos of the trace, and one unit of rounding
in the trace of a rotation by pi is sqrt(2 * 1.1e-16) = 1.5e-8 in the angle — seven orders above every other case.  Letting it set the
bound of all cases would make their check empty.  So is the sliver case: its solved triple is 1.5e-4 from collinear in singular values,
the two admissible roots lie 7e-6 apart (just outside the 1e-6 at which a random subset may be left out), and so close to a double root
the error is no longer first order in the rounding, which is all kappa measures; the case is there for its statuses, which pin the
collinearity threshold.  Each of the three figures is never above the worst over the whole list."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import p3p_reference as R  # noqa: E402
from helpers import build_host_program  # noqa: E402


APART = ("half_turn", "sliver")   # recorded apart, each bounds only itself


def measure():
    cs = R.cases()
    with tempfile.TemporaryDirectory() as d:
        got = R.run_host(build_host_program("p3p_host", d), d, list(cs.values()))
    return {name: R.worst_error(R.reference(name), st, poses) for name, (st, _, poses) in zip(cs, got)}


def main():
    per_case = measure()
    rec = {"host_worst_error": float(f"{max(v for k, v in per_case.items() if k not in APART) * 1.005:.3g}"),
           "host_worst_error_half_turn": float(f"{per_case['half_turn'] * 1.005:.3g}"),
           "host_worst_error_sliver": float(f"{per_case['sliver'] * 1.005:.3g}"),
           "device_factor": 4,
           "per_case": {k: float(f"{v:.3g}") for k, v in per_case.items()},
           "what": "worst |pose_k - reference_k| / ((kappa_k + |pose_k|) 2^-52) of the host fp64 pnp_detail::p3p_pose over tests/p3p_reference.py cases(): "
                   "every case but half_turn and sliver; half_turn (the angle of a half turn from acos of the trace); sliver (next to a double root)"}
    with open(os.path.join(HERE, "p3p_bound.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
