"""Track-creation geometry (rsba_track_candidates) at C4 size: every observation matched to its point's two previous
observations (about 4 M candidates).  One triangulation call over all frames, as the batched createTracks makes it, and one
reprojection-check call over the same candidates against the scene's points.  Wall times include the host staging, upload
and download; run under rocprofv3 --kernel-trace --stats for the kernel times.  Then the end-to-end batched
createTracks(sess, 0, F - 1, opt) through the C++ host side on the same scene (tools/tracks_e2e, built by build()), with its
breakdown.   usage: python tools/tracks_time.py [C4] [--no-e2e]"""
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from rsba_amd import capi  # noqa: E402
from rsba_amd.scene import make_config  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
name = args[0] if args else "C4"
p = make_config(name).problem
order = np.lexsort((p.obs_frame, p.obs_point))                     # by point, then frame
pts, frs = p.obs_point[order], p.obs_frame[order]
ca, cb = [], []
for back in (1, 2):                                                  # the point's previous observations
    same = np.zeros(len(order), dtype=bool)
    same[back:] = pts[back:] == pts[:-back]
    ca.append(order[same]); cb.append(order[np.nonzero(same)[0] - back])
ca = np.concatenate(ca).astype(np.int32); cb = np.concatenate(cb).astype(np.int32)
n = len(ca)
frame_poses = [p.poses[f] for f in range(p.num_frames)]
args = (p.intrinsics[0], None, frame_poses, p.shutter, p.scanlines, p.obs_frame, p.obs_xy, ca, cb)
tri = np.full(n, capi.TRACK_TRIANGULATE, dtype=np.uint8)
rep = np.full(n, capi.TRACK_REPROJECT, dtype=np.uint8)
track_pt = p.points[p.obs_point[cb]]
for _ in range(2):
    capi.track_candidates(*args, tri)
    capi.track_candidates(*args, rep, track_pt)
K = 5
t = time.perf_counter()
for _ in range(K):
    ok, pt, _ = capi.track_candidates(*args, tri)
tt = (time.perf_counter() - t) / K
t = time.perf_counter()
for _ in range(K):
    _, _, rok = capi.track_candidates(*args, rep, track_pt)
tr = (time.perf_counter() - t) / K
print(f"{name}: {p.num_observations} observations, {n} candidates")
print(f"triangulate: {tt * 1e3:.2f} ms per call incl. staging, upload, download ({n / tt:.3g} candidates/s), tri_ok {ok.mean():.3f}")
print(f"reprojection check: {tr * 1e3:.2f} ms per call incl. staging, upload, download ({n / tr:.3g} candidates/s), reproj_ok {rok.mean():.3f}")

if "--no-e2e" not in sys.argv:
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tracks_e2e")
    with tempfile.TemporaryDirectory() as d:
        np.array([p.num_frames, p.poses.shape[1], p.num_points, p.num_observations, p.shutter, p.scanlines[0], p.scanlines[1]], dtype=np.int64).tofile(f"{d}/header.bin")
        np.ascontiguousarray(p.intrinsics[0], dtype=np.float64).tofile(f"{d}/cam.bin")
        np.ascontiguousarray(p.poses, dtype=np.float64).tofile(f"{d}/poses.bin")
        np.ascontiguousarray(p.points, dtype=np.float64).tofile(f"{d}/points.bin")
        np.ascontiguousarray(p.obs_xy, dtype=np.float64).tofile(f"{d}/xy.bin")
        np.ascontiguousarray(p.obs_frame, dtype=np.int32).tofile(f"{d}/frame.bin")
        np.ascontiguousarray(p.obs_point, dtype=np.int32).tofile(f"{d}/point.bin")
        r = subprocess.run([exe, d], capture_output=True, text=True)
        print(r.stdout.strip())
        if r.returncode:
            print(r.stderr.strip())
            sys.exit(r.returncode)
