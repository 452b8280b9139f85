"""Small scenes for the one-step checks (tests/test_lm_step_reference.py, tests/test_gpu_lm_step.py): make_scene plus edits that
put something at a structural edge of the device solve — the last partial tile of FT frames (two-pose frames: CD 12, FT 4; one-pose
frames: CD 6, FT 8), a pseudo tile of an intrinsics block, a far tile pair, an empty or constant frame, masked coordinates.

``case(name)`` -> (problem, solver options as keywords).  Every case has its gauge fixed or damped enough that the scaled, damped
matrix keeps kappa <= 1e9."""
from __future__ import annotations

import numpy as np

from rsba_amd.problem import apply_gauge_masks
from rsba_amd.scene import make_scene, project

# the solve stops after one iteration whatever the tolerances say: the step is applied if the cost goes down
ONE_STEP = dict(max_num_iterations=1, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0)


def _gauge(p, *, fix_first=True):
    apply_gauge_masks(p, fix_first_n_cameras=1 if fix_first else 0)
    p.pose_fixed_mask[-1, -1] |= 0b111000
    return p


def _sorted(p, obs_frame, obs_point, obs_xy):
    order = np.lexsort((obs_point, obs_frame))
    p.obs_frame = np.ascontiguousarray(obs_frame[order], dtype=np.int32)
    p.obs_point = np.ascontiguousarray(obs_point[order], dtype=np.int32)
    p.obs_xy = np.ascontiguousarray(obs_xy[order], dtype=np.float64)
    return p


def base(frames, *, rolling=True, per_frame=45, seed=11, **kw):
    p = make_scene(frames, per_frame * frames, rolling=rolling, seed=seed, **kw).problem
    return _gauge(p)


def one_frame(rolling=True):
    """F = 1: frame 1 of a small scene on its own, free; every other point constant, the others seen once (V_j of rank 2: only the
    damping makes it invertible)."""
    p = make_scene(6, 300, rolling=rolling, seed=12).problem
    k = p.obs_frame == 1
    pts, inv = np.unique(p.obs_point[k], return_inverse=True)
    p.poses = np.ascontiguousarray(p.poses[1:2])
    p.points = np.ascontiguousarray(p.points[pts])
    p.obs_xy = np.ascontiguousarray(p.obs_xy[k])
    p.obs_frame = np.zeros(int(k.sum()), dtype=np.int32)
    p.obs_point = inv.astype(np.int32)
    apply_gauge_masks(p)
    p.point_constant[::2] = 1
    return p


def _observe(p, frame, X):
    """A new observation of point X from ``frame`` through its first pose (close to the rolling-shutter projection)."""
    xy, _ = project(p.intrinsics[0], p.poses[frame, :1], X[None, :])
    return xy[0] + 0.3


def case(name):
    opts = dict(ONE_STEP)
    rolling = not name.startswith("gs_")
    key = name[3:] if name.startswith(("rs_", "gs_")) else name
    FT = 4 if rolling else 8
    if key == "F1":
        return one_frame(rolling), opts
    if key.startswith("F"):                      # F in {FT - 1, FT, FT + 1, 2 FT + 1} given as an offset: "Fm1", "F0", "Fp1", "F2p1"
        F = {"Fm1": FT - 1, "F0": FT, "Fp1": FT + 1, "F2p1": 2 * FT + 1}[key]
        return base(F, rolling=rolling), opts
    if key == "nt25":                            # 25 tiles, the last one partial (two-pose: 99 frames; one-pose: 199)
        return base(25 * FT - 1, rolling=rolling, per_frame=25), opts
    if key == "single_view":                     # points seen by exactly one frame: every observation but the first dropped
        p = base(10, rolling=rolling)
        pick = np.arange(3, p.num_points, 17)
        first = np.full(p.num_points, -1)
        for i in range(p.num_observations - 1, -1, -1):
            first[p.obs_point[i]] = i
        drop = np.isin(p.obs_point, pick) & (np.arange(p.num_observations) != first[p.obs_point])
        return _sorted(p, p.obs_frame[~drop], p.obs_point[~drop], p.obs_xy[~drop]), opts
    if key == "twice":                           # some points seen twice in one frame
        p = base(10, rolling=rolling)
        dup = np.arange(0, p.num_observations, 13)
        return _sorted(p, np.concatenate([p.obs_frame, p.obs_frame[dup]]), np.concatenate([p.obs_point, p.obs_point[dup]]),
                       np.concatenate([p.obs_xy, p.obs_xy[dup] + 0.25])), opts
    if key == "far_pair":                        # points that link the first and the last tile
        p = base(4 * FT + 1, rolling=rolling)
        F = p.num_frames
        sel = np.unique(p.obs_point[p.obs_frame == 1])[:3]
        xy = np.stack([_observe(p, F - 1, p.points[j]) for j in sel])
        return _sorted(p, np.concatenate([p.obs_frame, np.full(len(sel), F - 1)]), np.concatenate([p.obs_point, sel]),
                       np.concatenate([p.obs_xy, xy])), opts
    if key == "dense_point":                     # one point seen by every frame: a dense S
        p = base(3 * FT + 2, rolling=rolling, all_visible=True)
        X = p.points.mean(axis=0)
        j = p.num_points
        p.points = np.concatenate([p.points, X[None, :]])
        p.point_constant = np.concatenate([p.point_constant, [0]]).astype(np.uint8)
        F = p.num_frames
        xy = np.stack([_observe(p, f, X) for f in range(F)])
        return _sorted(p, np.concatenate([p.obs_frame, np.arange(F)]), np.concatenate([p.obs_point, np.full(F, j)]),
                       np.concatenate([p.obs_xy, xy])), opts
    if key == "empty_frame":                     # a frame without observations (not a parameter block of the program)
        p = base(2 * FT + 3, rolling=rolling)
        k = p.obs_frame != FT + 1
        return _sorted(p, p.obs_frame[k], p.obs_point[k], p.obs_xy[k]), opts
    if key == "const_frame":                     # a fully constant frame in the middle
        p = base(2 * FT + 3, rolling=rolling)
        p.pose_fixed_mask[FT + 1] = 0x3F
        return p, opts
    if key in ("rotation_only", "position_only"):
        p = make_scene(2 * FT + 1, 45 * (2 * FT + 1), rolling=rolling, seed=13).problem
        apply_gauge_masks(p, fix_first_n_cameras=1, fix_position=key == "rotation_only", fix_rotation=key == "position_only")
        return p, opts
    if key == "const_points":
        p = base(2 * FT + 1, rolling=rolling)
        p.point_constant[::4] = 1
        return p, opts
    if key in ("intr_shared", "intr_perframe", "intr_mixed", "intr_run3", "intr_const"):
        p = base(2 * FT + 1, rolling=rolling, seed=14)
        p.calibrated = False
        F = p.num_frames
        rng = np.random.default_rng(3)
        jitter = 1.0 + 1e-3 * rng.normal(size=(F, 9)) * np.array([[1, 1, 20, 20, 10, 10, 10, 0.5, 0.5]])
        if key != "intr_shared":
            p.intrinsics = np.ascontiguousarray(np.tile(p.intrinsics[:1], (F, 1)) * jitter)
            p.frame_intrinsics = np.arange(F, dtype=np.int32)
        if key == "intr_mixed":                  # every third frame its own block, the others share block 0
            own = np.arange(F) % 3 == 1
            p.frame_intrinsics = np.where(own, np.cumsum(own), 0).astype(np.int32)
            p.intrinsics = np.ascontiguousarray(p.intrinsics[: int(own.sum()) + 1])
        if key == "intr_run3":                   # one block per run of three frames: a pseudo tile beside several frames' tiles
            p.frame_intrinsics = (np.arange(F) // 3).astype(np.int32)
            p.intrinsics = np.ascontiguousarray(p.intrinsics[: int(p.frame_intrinsics.max()) + 1])
        if key == "intr_const":                  # every other block constant
            p.intrinsics_constant = np.zeros(p.num_intrinsics, dtype=np.uint8)
            p.intrinsics_constant[::2] = 1
        return p, opts
    if key == "huber":                           # 10 % outliers
        p = base(2 * FT + 1, rolling=rolling, outlier_ratio=0.1, seed=15)
        p.huber_a = 2.0
        opts["initial_trust_region_radius"] = 1e2   # (at 1e4 the first two-pose step overshoots and is rejected)
        return p, opts
    if key.startswith("radius"):                 # radius1e-3, radius1e4, radius1e10
        opts["initial_trust_region_radius"] = float(key[6:])
        return base(2 * FT + 1, rolling=rolling, seed=16), opts
    raise KeyError(name)


SHAPES = ["F1", "Fm1", "F0", "Fp1", "F2p1", "single_view", "twice", "far_pair", "dense_point", "empty_frame", "const_frame",
          "rotation_only", "position_only", "const_points", "intr_shared", "intr_perframe", "intr_mixed", "intr_run3", "intr_const",
          "huber", "radius1e-3", "radius1e4", "radius1e10"]
CASES = [f"rs_{s}" for s in SHAPES] + [f"gs_{s}" for s in SHAPES] + ["rs_nt25", "gs_nt25"]
