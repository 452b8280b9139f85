"""Small scenes for the one-step checks (tests/test_lm_step_reference.py, tests/test_gpu_lm_step.py): make_scene plus edits that
put something at a structural edge of the device solve — the last partial tile of FT frames (two-pose frames: CD 12, FT 4; one-pose
frames: CD 6, FT 8), a pseudo tile of an intrinsics block, a far tile pair, an empty or constant frame, masked coordinates.

``case(name)`` -> (problem, solver options as keywords).  Every case has its gauge fixed or damped enough that the scaled, damped
matrix keeps kappa <= 1e9.

``PRIOR_CASES``: the prior blocks of CeresHandler::Add on such scenes — motion priors at a constant ratio (both kinds, the
velocity prior's ratio <= eps branch), with Huber, on some frames, next to constant frames, across tile edges; a free ratio
(the border column of the reduced system), once pushed onto its lower bound by the step; GoodPosePrior blocks (eliminated in
closed form by the device); the SphericalPrior; one-pose frames in a two-pose session (frame_global); intrinsics blocks."""
from __future__ import annotations

import numpy as np

from rsba_amd.problem import apply_gauge_masks, lower_scanline_poses
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
    if name in PRIOR_CASES:
        return prior_case(name)
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


def with_motion_priors(p, kind, scale, ratio, frames=None, free=False):
    p.prior_kind, p.prior_scale, p.inter_frame_ratio, p.ratio_free = kind, scale, ratio, free
    p.prior_frames = np.arange(1, p.num_frames, dtype=np.int32) if frames is None else np.asarray(frames, dtype=np.int32)
    return p


def with_pose_priors(p, blocks=None, rotation=3.0, position=5.0, sigma=0.01, seed=5):
    """GoodPosePrior blocks on the given pose blocks f * P + q (default: every pose block of frames >= 1), priorPoses near the poses."""
    rng = np.random.default_rng(seed)
    P = p.poses_per_frame
    p.pose_prior_block = np.arange(P, P * p.num_frames, dtype=np.int32) if blocks is None else np.asarray(blocks, dtype=np.int32)
    p.pose_prior_values = p.poses.reshape(-1, 6)[p.pose_prior_block] + rng.normal(0, sigma, (len(p.pose_prior_block), 6))
    p.pose_prior_rotation, p.pose_prior_position = rotation, position
    return p


def with_spherical(p):
    """The SphericalPrior of a session that starts at the origin (CeresHandler.h:121-130): frame 0 at zero, frame 1 at zero plus
    1e-4 in position, the prior on frame 1's first pose."""
    p.poses[0] = 0.0
    p.poses[1] = 0.0
    p.poses[1, :, 3:] += 1e-4
    p.spherical_pose_block = p.poses_per_frame
    return p


def scanline_session(rolling=True, *, one_pose=(2, 5, 6), seed=17):
    """A two-pose session in which the frames ``one_pose`` carry one pose (lowered with lower_scanline_poses: frame_global, the
    second slot data).  The second slot of those frames is set far from the first, so that touching it would show."""
    s = make_scene(10, 450, rolling=rolling, seed=seed).problem
    fp = [s.poses[f, :1].copy() if f in one_pose else s.poses[f].copy() for f in range(s.num_frames)]
    p, blocks = lower_scanline_poses(fp, s.obs_frame, s.obs_point, s.obs_xy, points=s.points, intrinsics=s.intrinsics,
                                     scanlines=s.scanlines)
    assert np.array_equal(blocks[:, 0], np.arange(s.num_frames)) and p.frame_global is not None
    p.poses[p.frame_global == 1, 1] += 0.5
    p.pose_fixed_mask[0] = 0x3F
    p.pose_fixed_mask[-1, 0 if p.frame_global[-1] else 1] |= 0b111000
    p.point_constant = np.zeros(p.num_points, dtype=np.uint8)
    return p


HUBER_PRIOR_SCALE = 10.0   # some 12-vectors of the Huber cases beyond a = 2, some within


def prior_case(name):
    """Cases with prior blocks: "rs_<what>" (two-pose frames: FT = 4) or "gs_<what>" (one-pose frames, no motion prior)."""
    opts = dict(ONE_STEP)
    rolling = not name.startswith("gs_")
    key = name[3:]
    FT = 4 if rolling else 8
    kinds = {"vel": (1, 6.0), "acc": (2, 25.0)}
    if key[:4] in ("vel_", "acc_") and key[4] == "r":        # constant ratio: "vel_r0.8", "acc_r2.5", "vel_r0" (the ratio <= eps branch)
        kind, scale = kinds[key[:3]]
        return with_motion_priors(base(2 * FT + 1, seed=21), kind, scale, float(key[5:])), opts
    if key in ("vel_free", "acc_free"):                      # the reference's default: a free, lower-bounded ratio (a border column)
        kind, scale = kinds[key[:3]]
        return with_motion_priors(base(2 * FT + 1, seed=22), kind, scale, 1.0, free=True), opts
    if key == "vel_free_bound":                              # frames that overlap in time (read-out 3 frames long: a negative gap) and a
        p = make_scene(2 * FT + 1, 45 * (2 * FT + 1), seed=23, intra_frame=3.0).problem   # ratio that starts at 8: the model step takes
        return with_motion_priors(_gauge(p), 1, 6.0, 8.0, free=True), opts                # the ratio to -0.07, the candidate is projected
    # (the acceleration prior's bound is DBL_EPSILON: a candidate projected there has 1 / ratio = 4.5e15 in its residuals, and no such
    # first step is accepted — none is here)
    if key in ("prior_huber", "free_huber"):                 # Huber on the reprojections and on the 12-vectors, some priors beyond it
        p = base(2 * FT + 1, outlier_ratio=0.1, seed=15)
        p.huber_a = 2.0
        opts["initial_trust_region_radius"] = 1e2
        return with_motion_priors(p, 2, HUBER_PRIOR_SCALE, 1.0 if key == "free_huber" else 1.25, free=key == "free_huber"), opts
    if key == "prior_subset":                                # priors on some frames only: (f, f - 1) blocks inside and across tiles
        return with_motion_priors(base(3 * FT + 1, seed=24), 1, 10.0, 2.5, frames=[2, 3, FT, 2 * FT + 1, 3 * FT]), opts
    if key in ("prior_fix3", "free_fix3"):                   # fixFirstNCameras = 3: the priors of frames 1, 2 are all constant (with a
        p = base(2 * FT + 1, seed=25)                        # constant ratio), frame 3's is half constant
        apply_gauge_masks(p, fix_first_n_cameras=3)
        p.pose_fixed_mask[-1, -1] |= 0b111000
        return with_motion_priors(p, 2, 25.0, 1.0 if key == "free_fix3" else 0.8, free=key == "free_fix3"), opts
    if key.startswith("prior_F"):                            # F = 2 FT - 1, 2 FT, 2 FT + 1, 3 FT - 1: (f, f - 1) blocks across tile edges,
        F = {"Fm1": 2 * FT - 1, "F0": 2 * FT, "Fp1": 2 * FT + 1, "F3m1": 3 * FT - 1}[key[6:]]   # the last tile partial or not
        return with_motion_priors(base(F, seed=26), 2, 25.0, 1.25), opts
    if key == "prior_nt":                                    # 7 tiles, the last partial, a free ratio
        return with_motion_priors(base(7 * FT - 2, per_frame=30, seed=27), 2, 25.0, 1.0, free=True), opts
    if key.startswith("pp_"):                                # GoodPosePrior blocks: on every pose of frames >= 1, or on some
        p = base(2 * FT + 1, outlier_ratio=0.1 if key.endswith("huber") else 0.0, seed=28)
        if key.endswith("huber"):
            p.huber_a = 2.0
            opts["initial_trust_region_radius"] = 1e2
        P = p.poses_per_frame
        blocks = None if "_all" in key else [P, P + 1 if P == 2 else 3, 5, 2 * FT * P - 1, (2 * FT + 1) * P - 1]
        return with_pose_priors(p, blocks), opts
    if key == "spherical":                                   # the SphericalPrior alone
        return with_spherical(base(2 * FT + 1, seed=29)), opts
    if key == "spherical_pp":                                # ... with GoodPosePriors (not on the spherical pose)
        p = with_spherical(base(2 * FT + 1, seed=29))
        P = p.poses_per_frame
        return with_pose_priors(p, np.arange(P + 1, P * p.num_frames, 2)), opts
    if key == "spherical_all":                               # ... with GoodPosePriors and motion priors, a free ratio
        p = with_pose_priors(with_spherical(base(2 * FT + 1, seed=29)), np.arange(3, 2 * (2 * FT + 1), 3))
        return with_motion_priors(p, 1, 6.0, 1.0, free=True), opts
    if key == "scanline":                                    # one-pose frames in a two-pose session
        return scanline_session(), opts
    if key == "scanline_priors":                             # ... with motion priors between two-pose frames and GoodPosePriors
        p = scanline_session()
        two = np.flatnonzero(p.frame_global == 0)
        frames = [f for f in range(1, p.num_frames) if f in two and f - 1 in two]
        return with_pose_priors(with_motion_priors(p, 2, 25.0, 1.0, frames=frames, free=True), [2 * 2, 2 * 5, 2 * 7, 2 * 7 + 1]), opts
    if key in ("prior_intr_shared", "prior_intr_perframe"):  # intrinsics blocks beside the priors
        p, _ = case(f"rs_intr_{key[11:]}")
        return with_pose_priors(with_motion_priors(p, 2, 25.0, 1.0, free=True), [3, 8, 11]), opts
    raise KeyError(name)


PRIOR_CASES = ["rs_vel_r0.8", "rs_vel_r1.25", "rs_vel_r2.5", "rs_vel_r0", "rs_acc_r0.8", "rs_acc_r1.25", "rs_acc_r2.5",
               "rs_vel_free", "rs_acc_free", "rs_vel_free_bound", "rs_prior_huber", "rs_free_huber", "rs_prior_subset", "rs_prior_fix3",
               "rs_free_fix3", "rs_prior_Fm1", "rs_prior_F0", "rs_prior_Fp1", "rs_prior_F3m1", "rs_prior_nt",
               "rs_pp_all", "rs_pp_some", "rs_pp_all_huber", "rs_pp_some_huber", "gs_pp_all", "gs_pp_some",
               "rs_spherical", "gs_spherical", "rs_spherical_pp", "gs_spherical_pp", "rs_spherical_all",
               "rs_scanline", "rs_scanline_priors", "rs_prior_intr_shared", "rs_prior_intr_perframe"]


SHAPES = ["F1", "Fm1", "F0", "Fp1", "F2p1", "single_view", "twice", "far_pair", "dense_point", "empty_frame", "const_frame",
          "rotation_only", "position_only", "const_points", "intr_shared", "intr_perframe", "intr_mixed", "intr_run3", "intr_const",
          "huber", "radius1e-3", "radius1e4", "radius1e10"]
CASES = [f"rs_{s}" for s in SHAPES] + [f"gs_{s}" for s in SHAPES] + ["rs_nt25", "gs_nt25"]


# ---- pose covariance (tests/test_lm_step_reference.py, tests/test_gpu_covariance.py) ------------------------------------------------

# the scenes the covariance unit was first measured on (the CPU oracle against the extended-precision inverse) ...
COV_TABLE = ["rs_Fp1", "gs_F2p1", "rs_huber", "rs_intr_shared", "rs_intr_run3", "gs_intr_perframe", "rs_prior_intr_perframe", "rs_acc_free",
             "rs_vel_r0", "rs_pp_some", "gs_pp_all", "rs_scanline", "rs_far_pair", "rs_twice", "rs_const_frame", "rs_nt25"]
# ... and the rest of the list: structural edges, masks, more intrinsics layouts, priors across tiles, 25 one-pose tiles, C2
COV_CASES = COV_TABLE + ["rs_F2p1", "rs_dense_point", "rs_empty_frame", "rs_const_points", "rs_rotation_only",
                         "rs_intr_mixed", "rs_intr_const", "rs_prior_subset", "rs_prior_nt", "rs_free_huber", "rs_pp_all_huber",
                         "rs_scanline_priors", "gs_nt25", "C2"]
# J^T J without damping is rank deficient: points seen once (two residuals for three unknowns: V_j of rank 2 — every other point of
# rs_F1, every 17th of rs_single_view), the SphericalPrior (1e20 on three coordinates: their columns are parallel to fp64), nothing
# fixed (the 7-dimensional gauge)
COV_REFUSED = ["rs_F1", "rs_single_view", "rs_spherical", "free_gauge"]


def cov_case(name):
    """The problem of a covariance case (undamped: the solver options of case() do not matter here)."""
    if name == "C2":
        from rsba_amd.scene import make_config
        return make_config("C2").problem
    if name == "free_gauge":
        return make_scene(8, 200, rolling=True, seed=63).problem
    return case(name)[0]


def cov_frames(p):
    """The frames a covariance case asks for: the first free frame, one on each side of the first tile edge (FT - 1, FT), the first
    frame of each of the three middle tiles when the video is longer than a leaf of the dissection (8 tiles: the top separator of
    a band of tiles is its middle BFS level, see tile_order.hpp), the last frame, the first one-pose frame of a two-pose session,
    and every constant or empty frame (all zeros)."""
    F, P = p.num_frames, p.poses_per_frame
    FT = 48 // (6 * P)
    mask = np.zeros((F, P), dtype=np.uint8) if p.pose_fixed_mask is None else p.pose_fixed_mask.reshape(F, P).copy()
    if p.frame_global is not None:
        mask[p.frame_global.astype(bool), 1:] = 0x3F
    seen = np.bincount(p.obs_frame, minlength=F) > 0
    dead = np.all(mask == 0x3F, axis=1) | ~seen
    out = {int(np.flatnonzero(~dead)[0]), F - 1} | {int(f) for f in np.flatnonzero(dead)}
    out |= {f for f in (FT - 1, FT) if f < F}
    nt = (F + FT - 1) // FT
    if nt > 8:
        out |= {t * FT for t in (nt // 2 - 1, nt // 2, nt // 2 + 1)}
    if p.frame_global is not None and p.frame_global.any():
        out.add(int(np.flatnonzero(p.frame_global)[0]))
    return sorted(out)
