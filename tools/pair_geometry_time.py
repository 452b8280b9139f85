#!/usr/bin/env python3
"""Times the batched degeneracy test (classifyPairs / rsba_two_view_classify_pairs: the homography RANSAC and the parallax counts of many
frame pairs) beside the batched essential-matrix RANSAC of the same pairs (rsba_epipolar_ransac_pairs, eight-point subsets) and beside P
sequential findHomographyRansac calls, in the same process on the same box (tools/pair_geometry_time.cpp).  The shapes of
tools/verify_pairs_time.py: P = 1, 16, 256 pairs x 1 024 subsets x 500 correspondences, three refits; three warm-ups, ten timed
repetitions, the median with min .. max; the batched homographies are compared with the sequential ones pair by pair on the way.
Builds the program when it is missing (g++ over the C ABI), runs it, prints its JSON lines and, with --out, writes them to a file.
Needs a GPU: there is no fallback."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def build(force=False):
    exe = os.path.join(TOOLS, "pair_geometry_time")
    if force or not os.path.exists(exe):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-L" + os.path.join(ROOT, "rsba_amd", "_lib"), "-lrsba_amd",
                        "-Wl,-rpath,$ORIGIN/../rsba_amd/_lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--rebuild", action="store_true")
    a = ap.parse_args()
    exe = build(a.rebuild)
    if a.build_only:
        return 0
    r = subprocess.run([exe], capture_output=True, text=True, timeout=560)
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        return r.returncode
    print(r.stdout.strip())
    if a.out:
        with open(a.out, "w") as f:
            f.write(r.stdout.strip() + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
