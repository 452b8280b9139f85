#!/usr/bin/env python3
"""What rsba_covariance_compute costs against rsba_pose_covariance frame by frame, for the bench configurations (default C2 and C4):
wall-clock time of a compute (median of --repeat, after one warm-up that allocates the tile arrays and uploads the plan's lists), its
split into the G / OFF / DIAG launches, the point kernel (every point) and the gather of every (f, f) block by HIP events
(rsba_covariance_times), 8 rsba_pose_covariance calls scaled to F, and the device memory the covariance holds (rsba_covariance_memory).
One JSON line per configuration.  rsba_pose_covariance is the same code on the parent commit: its time there is this column.  What the
kernels move is a counters-only pass' job."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["RSBA_COV_TIMES"] = "1"   # the library takes its HIP-event times only where asked (rsba_covariance_times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    from rsba_amd import capi
    from rsba_amd.scene import make_config
    for cfg in args.configs.split(","):
        p = make_config(cfg).problem              # (gauge fixed: frame 0 and the position of the last pose)
        F = p.num_frames
        with capi.DeviceProblem(p) as dp:
            st = dp.plan_stats()
            dp.covariance_compute()
            t_compute, t_gather = [], []
            pairs = np.stack([np.arange(F), np.arange(F)], axis=1)
            for _ in range(args.repeat):
                t0 = time.perf_counter(); dp.covariance_compute(); t1 = time.perf_counter()
                blocks = dp.covariance_frame_blocks(pairs); t2 = time.perf_counter()
                t_compute.append(t1 - t0); t_gather.append(t2 - t1)
            t0 = time.perf_counter(); pts = dp.covariance_point_blocks(); t_points = time.perf_counter() - t0
            ev, mem = dp.covariance_times(), dp.covariance_memory()
            frames = np.linspace(1, F - 1, 8).astype(int)
            dp.pose_covariance(int(frames[0]))
            t0 = time.perf_counter()
            one = [dp.pose_covariance(int(f)) for f in frames]
            t_one = (time.perf_counter() - t0) / len(frames)
            scale = max(float(np.abs(b).max()) for b in one)
            diff = max(float(np.abs(blocks[int(f)] - b).max()) for f, b in zip(frames, one))
        print(json.dumps(dict(config=cfg, frames=F, tiles=st["tiles"], factor_tiles=st["factor_tiles"], levels=st["levels"],
                              compute_ms=1e3 * float(np.median(t_compute)), gather_all_frames_ms=1e3 * float(np.median(t_gather)),
                              pose_covariance_ms_per_frame=1e3 * t_one, pose_covariance_all_frames_ms=1e3 * t_one * F,
                              points=int(p.num_points), point_blocks_all_points_ms=1e3 * t_points, points_finite=bool(np.isfinite(pts).all()),
                              extra_device_bytes=mem, **ev,
                              max_abs_difference_to_pose_covariance=diff, largest_entry=scale)), flush=True)


if __name__ == "__main__":
    main()
