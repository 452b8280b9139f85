#!/usr/bin/env python3
"""Times the DLT start poses of the global-shutter RANSAC hypotheses on the device against the host loop they replace, for 500, 1 000
and 16 384 six-point subsets of 2 000 points:
  * the host pnp_detail::dlt_pose loop's wall time and the device kernels' HIP-event time (tools/pnp_dlt_time.hip),
  * the wall time of solveGsPnPRansac with hypotheses_on_device off and on (tools/pnp_gs_e2e.cpp, over librsba_amd).
Builds the two programs when they are missing (hipcc / g++), runs them, prints their JSON lines and, with --out, writes them to a file.
Needs a GPU: there is no fallback."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def build(force=False):
    k, e = os.path.join(TOOLS, "pnp_dlt_time"), os.path.join(TOOLS, "pnp_gs_e2e")
    if force or not os.path.exists(k):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-Wno-unused-function", "-Wno-unused-result",
                        "-I" + os.path.join(ROOT, "include"), "-I" + TOOLS, k + ".hip", "-o", k], check=True)
    if force or not os.path.exists(e):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + TOOLS, e + ".cpp", "-L" + os.path.join(ROOT, "rsba_amd", "_lib"),
                        "-lrsba_amd", "-Wl,-rpath,$ORIGIN/../rsba_amd/_lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", e], check=True)
    return k, e


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--rebuild", action="store_true")
    a = ap.parse_args()
    programs = build(a.rebuild)
    if a.build_only:
        return 0
    lines = []
    for p in programs:
        r = subprocess.run([p], capture_output=True, text=True, timeout=600)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            return r.returncode
        lines += r.stdout.strip().split("\n")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
