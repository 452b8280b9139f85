"""Timing of the descriptor matcher (rsba_match_descriptors): one frame of n SIFT-like descriptors against five earlier frames
of n, the shape of parseFrame's loop (VideoSfMClient.cc:196-201), for n = 2048 and n = 8192.

Reported per workload, after warm-up calls, over repeated calls (median, min .. max):
  kernel      HIP events around the three passes of kernels_match.hip (rsba_match_last_kernel_ms)
  call        wall clock of rsba_match_descriptors itself — staging copy, upload, kernels, download — called through ctypes on
              arrays prepared beforehand (the Python wrapper's concatenation and allocations are outside the clock)
  check       every workload's result is compared with the integer restatement (tests/match_reference.py) on a sample of
              queries per pair, bit for bit: the timing run doubles as a correctness check at the large shapes
  TFLOP/s     2 * n_q * n_t * 128 * pairs over the kernel time, and its share of the fp32-matrix peak (157.3 TFLOP/s)
  CPU         the same search on this box's host: numpy sgemm in the form |q|^2 + |t|^2 - 2 q.t, argpartition for the k best —
              the labelled baseline, with the CPU model and the thread count of numpy's BLAS (threadpoolctl where installed)

    python tools/match_time.py [--sizes 2048,8192] [--repeats 10] [--warmup 3] [--k 2] [--no-cpu] [--check 64] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TFLOPS = 157.3   # fp32-input matrix peak of the MI355X


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return ", ".join(f"{i.get('internal_api')} {i.get('num_threads')}" for i in threadpool_info() if i.get("user_api") == "blas") or "no BLAS pool found"
    except ImportError:
        return "OMP_NUM_THREADS=" + os.environ.get("OMP_NUM_THREADS", "unset") + " (threadpoolctl not installed)"


def gpu_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:
        return "unknown"


def cpu_search(frames, pairs, k):
    t0 = time.perf_counter()
    for fq, ft in pairs:
        q, t = frames[fq], frames[ft]
        d2 = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2.0 * (q @ t.T)
        part = np.argpartition(d2, k, axis=1)[:, :k]
        np.take_along_axis(d2, part, 1).sort(axis=1)
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--check", type=int, default=64, help="queries per pair compared with the integer restatement")
    ap.add_argument("--out")
    a = ap.parse_args()
    from rsba_amd import capi
    import match_reference as M
    lib = capi.lib()
    results = {"host": socket.gethostname(), "gpu": gpu_name(), "date": time.strftime("%Y-%m-%d"), "cpu_model": cpu_model(),
               "cpu_blas_threads": blas_threads(), "k": a.k, "workloads": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(n)
        frames = [rng.integers(0, 256, (n, 128)).astype(np.float32) for _ in range(6)]
        pairs = [(5, 5 - i) for i in range(1, 6)]
        # the C call's arguments, prepared once
        desc = np.ascontiguousarray(np.concatenate(frames))
        off = np.arange(7, dtype=np.int64) * n
        pq = np.array([p[0] for p in pairs], dtype=np.int32); pt = np.array([p[1] for p in pairs], dtype=np.int32)
        out = np.arange(len(pairs) + 1, dtype=np.int64) * n * a.k
        idx = np.empty(len(pairs) * n * a.k, dtype=np.int32); dist = np.empty(len(pairs) * n * a.k, dtype=np.float32)
        cnt = np.empty(len(pairs) * n, dtype=np.int32)

        def call():
            capi._check(lib.rsba_match_descriptors(C.c_int32(0), capi._ptr(desc), C.c_int32(128), capi._ptr(off), C.c_int32(6), capi._ptr(pq), capi._ptr(pt),
                                                   C.c_int64(len(pairs)), C.c_int32(a.k), capi._ptr(out), capi._ptr(idx), capi._ptr(dist), capi._ptr(cnt)))
        for _ in range(a.warmup):
            call()
        kern, wall = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(capi.match_last_kernel_ms())
        # a sample of queries of every pair against the integer restatement, bit for bit
        checked = 0
        for p, (fq, ft) in enumerate(pairs):
            rows = rng.choice(n, min(a.check, n), replace=False)
            wi, wd, wc = M.knn_int(frames[fq][rows], frames[ft], a.k)
            gi = idx[out[p]:out[p + 1]].reshape(n, a.k)[rows]; gd = dist[out[p]:out[p + 1]].reshape(n, a.k)[rows]
            if not (np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(cnt[p * n:(p + 1) * n][rows], wc)):
                raise SystemExit(f"n = {n}, pair {p}: the device result differs from the integer restatement")
            checked += len(rows)
        flop = 2.0 * n * n * 128 * len(pairs)
        w = {"n": n, "pairs": len(pairs), "kernel_ms": spread(kern), "call_ms": spread(wall), "repeats": a.repeats, "warmup": a.warmup, "queries_checked": checked}
        w["tflops"] = flop / (w["kernel_ms"]["median"] * 1e-3) / 1e12
        w["share_of_fp32_matrix_peak"] = w["tflops"] / PEAK_TFLOPS
        if not a.no_cpu:
            cpu_search(frames, pairs[:1], a.k)
            w["cpu_numpy_sgemm_ms"] = spread([cpu_search(frames, pairs, a.k) for _ in range(3)])
        results["workloads"].append(w)
        print(f"n = {n}: kernel {w['kernel_ms']['median']:.3f} ms ({w['kernel_ms']['min']:.3f} .. {w['kernel_ms']['max']:.3f}), "
              f"call {w['call_ms']['median']:.3f} ms ({w['call_ms']['min']:.3f} .. {w['call_ms']['max']:.3f}), "
              f"{w['tflops']:.1f} TFLOP/s = {100 * w['share_of_fp32_matrix_peak']:.1f} % of {PEAK_TFLOPS}"
              + ("" if a.no_cpu else f"; CPU numpy sgemm {w['cpu_numpy_sgemm_ms']['median']:.1f} ms ({results['cpu_model']}, BLAS threads: {results['cpu_blas_threads']})")
              + f"; {checked} queries bit-equal to the restatement")
    print(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
