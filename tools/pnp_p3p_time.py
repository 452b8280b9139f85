#!/usr/bin/env python3
"""Times the minimal-solver hypotheses of the global-shutter RANSAC on the device, for 500, 1 000 and 16 384 subsets of 2 000 points
(tools/pnp_p3p_time.hip over the scene of tools/pnp_time_scene.hpp): the P3P kernel alone, the whole rsba_pnp_gs_hypotheses_p3p call and,
beside it, the whole rsba_pnp_gs_hypotheses call (the DLT form) at the same counts, all in HIP-event time after a warm-up.
Builds the program when it is missing (hipcc), runs it, prints its JSON lines and, with --out, writes them to a file.
Needs a GPU: there is no fallback."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def build(force=False):
    exe = os.path.join(TOOLS, "pnp_p3p_time")
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
    r = subprocess.run([exe], capture_output=True, text=True, timeout=110)
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
