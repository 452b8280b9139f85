"""Shared helpers for the parity tests."""
import json
import os

import numpy as np

from rsba_amd.problem import BAProblem, GLOBAL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def build_host_program(name, directory, extra_flags=()):
    """compiles tests/<name>.cpp over the headers of include/ (host code only: nothing of the library is linked) into `directory`
    -> the program's path"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(directory), name)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", *extra_flags, "-I" + os.path.join(root, "include"), os.path.join(root, "tests", name + ".cpp"), "-o", exe], check=True)
    return exe


def problem_from_case(c) -> BAProblem:
    """One-observation problem for a per_observation.json case."""
    poses = [c["pose0"]] if c["pose1"] is None else [c["pose0"], c["pose1"]]
    return BAProblem(poses=np.array([poses]), points=np.array([c["point"]]), intrinsics=np.array([c["cam"]]),
                     obs_xy=np.array([c["obs"]]), obs_frame=np.array([0]), obs_point=np.array([0]),
                     shutter=c["shutter"], scanlines=tuple(c["scanlines"]),
                     interpolate_rotation=c["interpolate_rotation"], calibrated=c["calibrated"])


def batch_cases(cases):
    """Group per-observation cases that share a model into multi-observation problems so a device
    launch sees many of them at once.  Yields (problem, [case indices])."""
    groups = {}
    for idx, c in enumerate(cases):
        key = (c["pose1"] is None, c["shutter"], tuple(c["scanlines"]), c["interpolate_rotation"], c["calibrated"])
        groups.setdefault(key, []).append(idx)
    for key, idxs in groups.items():
        cs = [cases[i] for i in idxs]
        poses = np.array([[c["pose0"]] if c["pose1"] is None else [c["pose0"], c["pose1"]] for c in cs])
        prob = BAProblem(poses=poses, points=np.array([c["point"] for c in cs]), intrinsics=np.array([c["cam"] for c in cs]),
                         obs_xy=np.array([c["obs"] for c in cs]), obs_frame=np.arange(len(cs)), obs_point=np.arange(len(cs)),
                         shutter=key[1], scanlines=key[2], interpolate_rotation=key[3], calibrated=key[4],
                         frame_intrinsics=np.arange(len(cs), dtype=np.int32))
        yield prob, idxs


def problem_from_solve_case(c) -> BAProblem:
    poses = np.array(c["poses"])
    prob = BAProblem(poses=poses, points=np.array(c["points"]), intrinsics=np.array([c["cam"]]),
                     obs_xy=np.array(c["obs_xy"]), obs_frame=np.array(c["obs_frame"]), obs_point=np.array(c["obs_point"]),
                     shutter=c["shutter"], scanlines=tuple(c["scanlines"]), interpolate_rotation=True, calibrated=True,
                     huber_a=c["huber_a"])
    F, P = poses.shape[:2]
    mask = np.zeros((F, P), dtype=np.uint8)
    mask[0, :] = 0x3F
    mask[-1, -1] |= 0b111000
    prob.pose_fixed_mask = mask
    if c.get("prior_kind"):
        prob.prior_kind, prob.prior_scale, prob.inter_frame_ratio = c["prior_kind"], c["prior_scale"], c["inter_frame_ratio"]
        prob.prior_frames = np.array(c["prior_frames"], dtype=np.int32)
        prob.ratio_free = bool(c.get("ratio_free", False))
    return prob


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def write_scene_file(path, prob, *, fix_first_n=1, fix_scale=False, max_iter=20, revalidate=0.0, cov_frame=-1,
                     const_frame_velocity=0.0, const_frame_acceleration=0.0, inter_frame_ratio=1.0):
    """Binary scene file read by examples/ba_session.cpp (layout documented there)."""
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<11i", prob.num_frames, prob.poses_per_frame, prob.num_points, int(prob.shutter), int(prob.scanlines[0]),
                            int(prob.scanlines[1]), int(prob.calibrated), int(prob.interpolate_rotation), fix_first_n, int(fix_scale), max_iter))
        f.write(struct.pack("<q", prob.num_observations))
        f.write(struct.pack("<ddd", float(prob.huber_a), float(revalidate), float(cov_frame)))
        f.write(struct.pack("<ddd", float(const_frame_velocity), float(const_frame_acceleration), float(inter_frame_ratio)))
        f.write(prob.intrinsics[0].astype("<f8").tobytes())
        f.write(prob.poses.astype("<f8").tobytes())
        f.write(prob.points.astype("<f8").tobytes())
        f.write(prob.obs_xy.astype("<f8").tobytes())
        f.write(prob.obs_frame.astype("<i4").tobytes())
        f.write(prob.obs_point.astype("<i4").tobytes())


def read_result_file(path, prob):
    raw = np.fromfile(path, dtype="<f8")
    head = raw[:6]
    npose = prob.poses.size
    poses = raw[6:6 + npose].reshape(prob.poses.shape)
    points = raw[6 + npose:6 + npose + prob.points.size].reshape(-1, 3)
    rest = raw[6 + npose + prob.points.size:]
    return dict(initial_cost=head[0], final_cost=head[1], iterations=int(head[2]), reduced=int(head[3]), termination=int(head[4]),
                usable=bool(head[5]), poses=poses, points=points, covariance=rest[:108].reshape(3, 6, 6) if rest.size >= 108 else None)


# ---- the cut of a sharded solve (rsba_partition_points) restated on the host ----

HOOKS_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rsba_amd", "_lib", "librsba_amd_hooks.so")


def partition_tiles(prob: BAProblem, world: int) -> np.ndarray:
    """part_of[tile column] of the cut rsba_partition_points computes (-1 = a separator): rsba_debug_partition_tiles, which only the
    instrumented library (-DRSBA_TEST_HOOKS) exports.  Host only."""
    import ctypes as C

    from rsba_amd import capi
    L = C.CDLL(HOOKS_LIB)
    d = capi.make_desc(prob)
    nt = C.c_int32(0)
    assert L.rsba_debug_partition_tiles(C.byref(d), C.c_int32(world), None, C.byref(nt)) == 0
    part_of = np.full(nt.value, -2, dtype=np.int32)
    rc = L.rsba_debug_partition_tiles(C.byref(d), C.c_int32(world), part_of.ctypes.data_as(C.c_void_p), C.byref(nt))
    if rc != 0:
        L.rsba_last_error.restype = C.c_char_p
        raise capi.RsbaError(rc, L.rsba_last_error().decode())
    return part_of


def observation_tiles(prob: BAProblem):
    """Per observation, the tile columns of the reduced camera system it adds to: its frame's tile (real, [N]) and the tiles of the
    pseudo frames of the intrinsics block its frame is seen through (pseudo, [N, NPF]; NPF = 0 when calibrated).  A tile holds 48
    unknowns: 4 two-pose frames or 8 one-pose frames; a 9-block of intrinsics takes ceil(9 / unknowns per frame) pseudo frames,
    numbered behind the real frames block by block."""
    CD = 6 * prob.poses_per_frame
    FT, FR = 48 // CD, prob.num_frames
    NIB = 0 if prob.calibrated else prob.num_intrinsics
    NPF = 0 if prob.calibrated else (9 + CD - 1) // CD
    fi = prob.frame_intrinsics if (NIB > 1 and prob.frame_intrinsics is not None) else np.zeros(FR, dtype=np.int32)
    real = prob.obs_frame.astype(np.int64) // FT
    pseudo = (FR + fi[prob.obs_frame].astype(np.int64)[:, None] * NPF + np.arange(NPF)[None, :]) // FT
    nt = (FR + NIB * NPF + FT - 1) // FT
    return real, pseudo, nt


def points_off_the_cut(prob: BAProblem, owner: np.ndarray, part_of: np.ndarray, pseudo_only: bool = False) -> np.ndarray:
    """The points that reach a tile of a part other than their owner's (separator tiles, -1, are everyone's) — through a real frame's
    tile or an intrinsics block's pseudo tile (pseudo_only: through the pseudo tiles alone)."""
    real, pseudo, _ = observation_tiles(prob)
    own = np.asarray(owner)[prob.obs_point][:, None]
    tiles = pseudo if pseudo_only else np.concatenate([real[:, None], pseudo], axis=1)
    p = part_of[tiles]
    off = ((p >= 0) & (p != own)).any(axis=1)
    return np.unique(prob.obs_point[off])


def owners_from_real_tiles(prob: BAProblem, world: int, part_of: np.ndarray) -> np.ndarray:
    """An owner rule that looks at the real frames' tiles only (what rsba_partition_points did before it followed the pseudo tiles
    too): a point goes to the part of its frames' tiles, points seen in separator frames only to whichever rank holds the fewest
    observations so far, in point order."""
    real, _, _ = observation_tiles(prob)
    M = prob.num_points
    p = part_of[real]
    owner = np.full(M, -1, dtype=np.int32)
    inpart = p >= 0
    owner[prob.obs_point[inpart]] = p[inpart]
    nobs = np.bincount(prob.obs_point, minlength=M)
    load = np.bincount(owner[owner >= 0], weights=nobs[owner >= 0], minlength=world).astype(np.int64)
    for j in np.flatnonzero(owner < 0):
        r = int(np.argmin(load))
        owner[j] = r; load[r] += nobs[j]
    return owner
