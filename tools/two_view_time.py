#!/usr/bin/env python3
"""Times the essential-matrix hypotheses of the two-view bootstrap on the device, for 1 024 and 16 384 eight-point subsets of 500 and 8 000
correspondences (tools/two_view_time.hip): the eight-point and the score kernel alone in HIP-event time, the whole
rsba_epipolar_hypotheses call, and beside it the same batch from the host definitions on the same box — three warm-ups, ten timed
repetitions, the median with min .. max.  Then the five-point chain on the same views: the five-point kernel, the score kernel over the
ten solution slots per subset and the pick kernel alone, the whole rsba_epipolar_hypotheses_five_point call, the host chain.
Builds the program when it is missing (hipcc), runs it, prints its JSON lines and, with --out, writes them to a file.
Needs a GPU: there is no fallback."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def build(force=False):
    exe = os.path.join(TOOLS, "two_view_time")
    if force or not os.path.exists(exe):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-Wno-unused-function", "-Wno-unused-result",
                        "-I" + os.path.join(ROOT, "include"), "-I" + TOOLS, exe + ".hip", "-L" + os.path.join(ROOT, "rsba_amd", "_lib"), "-lrsba_amd",
                        "-Wl,-rpath,$ORIGIN/../rsba_amd/_lib", "-o", exe], check=True)
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
