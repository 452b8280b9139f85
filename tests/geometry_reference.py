"""An mpmath model (50 digits) of the geometry either side of the solve, written from the meaning of the reference's
struct/VideoSfM.cc (getPose, reproject, validate), mat/cam.h (distort, undistort, c2direction, triangulate, w2i, validate) and
solveRSpnp.cpp (project3dPoints' float roundings, one LevenbergMarquardt step of Ceres' TrustRegionMinimizer at its defaults).
It imports neither the oracle nor the product; only mp_rotate / mp_residual of tests/golden/make_golden.py, which are as
independent.  The device kernels (kernels_filter.hip, kernels_tracks.hip, kernels_pnp.hip) and the CPU oracle are both compared
with it, by tests/test_geometry_reference.py (no GPU) and tests/test_gpu_geometry.py.

Every function that makes a comparison also returns that comparison's MARGIN, the relative distance |a - b| / max(|a|, |b|)
between the two sides (named in a dict), so that a caller can leave out the items whose outcome fp64 rounding may decide:
an item is *decided* when every comparison the model made for it clears the caller's rule.

The second half of the file builds the input sets of the two test files (parts A - E of their docstrings) and evaluates the
model on them once per process (functools.lru_cache)."""
import functools
import importlib.util
import os

import mpmath as mp
import numpy as np

_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py"))
_mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mg)
mp_rotate, mp_residual = _mg.mp_rotate, _mg.mp_residual

mp.mp.dps = 50
M = mp.mpf
GLOBAL, HORIZONTAL, VERTICAL = 0, 1, 2
DBL_EPS = M(2) ** -52
EPS53 = 2.0 ** -53
Z_GATE = M("1e-8")
INF = float("inf")
CAM = np.array([800.0, 800.0, -0.05, 0.01, 1e-3, -1e-3, 2e-3, 640.0, 360.0])    # the camera of tests/test_gpu_tracks.py


def mpv(v):
    """doubles -> mpf, exactly"""
    return [M(float(x)) for x in np.asarray(v, dtype=np.float64).ravel()]


def rel(a, b):
    """relative distance of the two sides of a comparison"""
    s = max(abs(a), abs(b))
    return float(abs(a - b) / s) if s != 0 else 0.0


def norm(v):
    return mp.sqrt(mp.fsum(x * x for x in v))


def contraction(moves):
    """Of a fixed-point replay's successive move lengths: L, the largest ratio of successive moves, and the factor by which the
    replay can amplify a rounding error u made in every step, e' = r e + u along the replay's own ratios: at most 1 / (1 - L) when
    L < 1, and still defined when an iteration first runs away and then settles at a clamped pose (ratios above 1, then 0)."""
    ratios = [float(b / a) for a, b in zip(moves, moves[1:]) if a > 0]
    amp = 1.0
    for r in ratios:
        amp = 1.0 + r * amp
    return max(ratios + [0.0]), amp


# ---------------------------------------------------------------- poses ----------------------------------------------------------------
def scanline_index(line, n):
    """the pose a frame with more than two poses lends to a scan line: clamped to [0, n - 1], then std::round (halves away from
    zero; the clamped line is not negative)"""
    line = min(max(line, M(0)), M(n - 1))
    return int(mp.floor(line + M(1) / 2)), line


def get_pose(poses, shutter, scan, obs, interp=True, index=scanline_index):
    """getPose's three cases.  poses: list of 6-lists of mpf.  -> (pose, margins); the only discontinuous choice is the scan-line
    index, whose margin is the distance of the clamped line from the nearest half"""
    n = len(poses)
    if n == 1:
        return list(poses[0]), {}
    if n == 2:
        if shutter == GLOBAL:
            return list(poses[0]), {}
        coord = obs[1] if shutter == VERTICAL else obs[0]
        tau = (coord - scan[0]) / M(scan[1] - scan[0])
        tau = min(max(tau, M(0)), M(1))
        p0, p1 = poses
        return [p0[k] if (k < 3 and not interp) else p0[k] + (p1[k] - p0[k]) * tau for k in range(6)], {}
    k, line = index(obs[0] if shutter == HORIZONTAL else obs[1], n)
    frac = line - mp.floor(line)
    return list(poses[k]), {"line": float(abs(frac - M(1) / 2))}


# -------------------------------------------------------------- the camera --------------------------------------------------------------
def distort(cam, p):
    k1, k2, p1, p2, k3 = cam[2:7]
    x, y = p
    r2 = x * x + y * y
    d = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return [d * x + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), d * y + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y]


def w2i(cam, pose, X, gate=True):
    """world -> image.  With the gate a point whose camera-frame z is below 1e-8 fails; without it only a z that is numerically
    zero is moved to DBL_EPSILON.  -> (ok, xy or None, z)"""
    pc = mp_rotate(pose[:3], [X[i] - pose[3 + i] for i in range(3)])
    z = pc[2]
    if z < Z_GATE:
        if gate:
            return False, None, z
        if abs(z) < DBL_EPS:
            z = DBL_EPS
    d = distort(cam, [pc[0] / z, pc[1] / z])
    return True, [cam[0] * d[0] + cam[7], cam[1] * d[1] + cam[8]], pc[2]


def undistort_replay(cam, pn, max_iter=200, stop_early=0):
    """The reference's fixed-point undistortion p_u -= distort(p_u) - p_n: leaves (invalid) when the error exceeds |p_n|, ends
    (valid) when it falls below |p_n| 0.001 / fx, at most 200 steps.  stop_early = 1 ends one step sooner (a wrong replay, for
    the discrimination check).  -> dict(ok, p, steps, L, margins)"""
    nrm = norm(pn)
    tol = nrm * M("0.001") / cam[0]
    pu, ok, dists, margin = list(pn), False, [], INF
    if stop_early:
        max_iter = undistort_replay(cam, pn)["steps"] - stop_early
    for it in range(max_iter):
        pd = distort(cam, pu)
        err = [pd[0] - pn[0], pd[1] - pn[1]]
        dist = norm(err)
        margin = min(margin, rel(dist, nrm))
        if dist > nrm:
            break
        pu = [pu[0] - err[0], pu[1] - err[1]]
        dists.append(dist)
        margin = min(margin, rel(dist, tol))
        if dist < tol:
            ok = True
            break
    if stop_early:
        ok = True
    L, amp = contraction(dists)
    return dict(ok=ok, p=pu, steps=len(dists), L=L, amp=amp, tol=tol, margins={"undistort": margin})


def undistort_newton(cam, pn, steps=60):
    """the inverse of distort by Newton's method (Jacobian by differences in mp), independent of the replay"""
    pu, h = list(pn), M("1e-25")
    for _ in range(steps):
        f = distort(cam, pu)
        r = [f[0] - pn[0], f[1] - pn[1]]
        if norm(r) < M("1e-45"):
            break
        fx = distort(cam, [pu[0] + h, pu[1]]); fy = distort(cam, [pu[0], pu[1] + h])
        a, c = (fx[0] - f[0]) / h, (fx[1] - f[1]) / h
        b, d = (fy[0] - f[0]) / h, (fy[1] - f[1]) / h
        det = a * d - b * c
        pu = [pu[0] - (d * r[0] - b * r[1]) / det, pu[1] - (a * r[1] - c * r[0]) / det]
    return pu


def c2direction(pose, p):
    """camera-frame point -> unit direction in the world frame (the inverse rotation)"""
    d = mp_rotate([-pose[0], -pose[1], -pose[2]], list(p))
    n = norm(d)
    return [x / n for x in d]


def pixel_ray(cam, pose, xy, stop_early=0):
    """direction of a pixel: centre and normalise, undistort (must be valid), rotate into the world frame"""
    pn = [(xy[0] - cam[7]) / cam[0], (xy[1] - cam[8]) / cam[1]]
    u = undistort_replay(cam, pn, stop_early=stop_early)
    ray = c2direction(pose, [u["p"][0], u["p"][1], M(1)]) if u["ok"] else None
    return ray, u


def triangulate(c1, a, c2, b):
    """the midpoint of two rays: A p = Pa c1 + Pb c2 with Pa = I - a a^T, A = Pa + Pb, through lu_solve.
    -> (p or None when A is singular to 50 digits, det(A), cond_2(A))"""
    eye = mp.eye(3)
    va, vb = mp.matrix(a), mp.matrix(b)
    Pa, Pb = eye - va * va.T, eye - vb * vb.T
    A = Pa + Pb
    det = mp.det(A)
    ev = sorted(abs(e) for e in mp.eigsy(A, eigvals_only=True))
    if ev[0] < M("1e-40"):
        return None, det, INF
    y = Pa * mp.matrix(c1) + Pb * mp.matrix(c2)
    p = mp.lu_solve(A, y)
    return [p[0], p[1], p[2]], det, float(ev[2] / ev[0])


# ----------------------------------------------------------- reproject, validate -----------------------------------------------------------
def reproject(cam, poses, shutter, scan, X, interp=True, limit=50, stop=M("1e-6"), index=scanline_index):
    """The reference's fixed point for the pixel of a point in a rolling-shutter frame: from the principal point, take the pose at
    the iterate, project with the gate, until the squared move is <= 1e-6 (or the frame has one pose); `--limit < 1` before every
    step fails the 50th.  -> dict(ok, xy, reason, steps, L, margins)"""
    proj, moves = [cam[7], cam[8]], []
    m = {"move": INF, "z": INF, "line": INF}
    n = len(poses)
    out = dict(ok=False, xy=None, reason=None, steps=0, L=0.0, margins=m, zmin=INF)
    while True:
        limit -= 1
        if limit < 1:
            out["reason"] = "limit"
            break
        prev = proj
        pose, pm = get_pose(poses, shutter, scan, prev, interp, index)
        m["line"] = min(m["line"], pm.get("line", INF))
        ok, proj, z = w2i(cam, pose, X)
        m["z"] = min(m["z"], rel(z, Z_GATE))
        out["zmin"] = min(out["zmin"], float(z))
        out["steps"] += 1
        if not ok:
            out["reason"] = "gate"
            break
        mv2 = (prev[0] - proj[0]) ** 2 + (prev[1] - proj[1]) ** 2
        if n > 1:
            m["move"] = min(m["move"], rel(mv2, stop))
            moves.append(mp.sqrt(mv2))
        if not (n > 1 and mv2 > stop):
            out["ok"], out["xy"] = True, proj
            break
    out["L"], out["amp"] = contraction(moves)
    return out


def validate(cam, poses, shutter, scan, X, obs, sq_threshold, min_distance, interp=True, index=scanline_index):
    """vision::sfm::validate: the pose at the observation itself, the camera no nearer than min_distance, the gated projection
    within the squared threshold.  -> (flag, margins, squared error or None)"""
    pose, _ = get_pose(poses, shutter, scan, obs, interp, index)
    dist = norm([pose[3 + i] - X[i] for i in range(3)])
    m = {"dist": rel(dist, M(min_distance)) if min_distance != 0 else INF}
    far = dist >= M(min_distance)
    ok, proj, z = w2i(cam, pose, X)
    m["z"] = rel(z, Z_GATE)
    if not ok:
        return False, m, None
    e2 = (proj[0] - obs[0]) ** 2 + (proj[1] - obs[1]) ** 2
    m["err"] = rel(e2, M(sq_threshold))
    return bool(far and e2 < M(sq_threshold)), m, e2


def decided(margins, **rule):
    """every comparison made clears its rule (a margin that was not made is absent or infinite)"""
    return all(margins.get(k, INF) > v for k, v in rule.items())


# ------------------------------------------------------------- PnP scoring -------------------------------------------------------------
def f32(x):
    return float(np.float32(float(x)))


def pnp_score(cam, poses, shutter, scan, X, ixy, threshold, tau_from_x=False):
    """project3dPoints' inlier rule for one float32 point / observation and a pose pair: tau from the TRUE observation (x for
    HORIZONTAL, y for VERTICAL), no z gate, the projection rounded to float32, float32 differences, their norm in double against
    (double)(float)threshold.  -> (inlier, |dist - thr|, dist)"""
    ix, iy = float(np.float32(ixy[0])), float(np.float32(ixy[1]))
    src = ix if (tau_from_x or shutter != VERTICAL) else iy
    pose, _ = get_pose(poses, HORIZONTAL if shutter != GLOBAL else GLOBAL, scan, [M(src), M(src)], True)
    ok, proj, _ = w2i(cam, pose, [M(float(v)) for v in X], gate=False)
    dx = float(np.float32(ix) - np.float32(f32(proj[0])))
    dy = float(np.float32(iy) - np.float32(f32(proj[1])))
    dist = mp.sqrt(M(dx) * dx + M(dy) * dy)
    thr = M(f32(threshold))
    return bool(dist < thr), float(abs(dist - thr)), float(dist)


# ------------------------------------------------------------ one LM step ------------------------------------------------------------
def pnp_rows(cam, x, shutter, scan, X, obs, tau_from_x_always=True, h=M("1e-20"), jac=True):
    """residual (2) and Jacobian (2 x 12, central differences) of one float32 point / observation at the pose pair x (12 mpf);
    the functor takes tau from x for a VERTICAL shutter too, and has no z gate (the inputs keep z far above it)"""
    Xm, om = [M(float(v)) for v in X], [M(float(v)) for v in obs]

    def res(x):
        r = mp_residual(cam, x[:6], x[6:], Xm, om, shutter, scan, True, tau_from_x_always=tau_from_x_always)
        assert r is not None
        return r
    r = res(x)
    if not jac:
        return r, None
    J = [[M(0)] * 12, [M(0)] * 12]
    for a in range(12 if shutter != GLOBAL else 6):
        xp, xm = list(x), list(x)
        xp[a] += h; xm[a] -= h
        rp, rm = res(xp), res(xm)
        J[0][a], J[1][a] = (rp[0] - rm[0]) / (2 * h), (rp[1] - rm[1]) / (2 * h)
    return r, J


def lm_step(cam, shutter, scan, X, xy, subset, init, radius=M("1e4"), clamp_lo=M("1e-6"), tau_from_x_always=True, rows=None):
    """The first iteration of Ceres' trust-region loop at its defaults on the two pose blocks: H = J^T J, g = J^T r, the Jacobi
    scale s = 1 / (1 + sqrt(diag H)), D = clamp(s^2 diag H, 1e-6, 1e32), (S H S + D / radius) y = S g, delta = -S y.
    rows: a cache {point index: (r, J)} at `init`, shared by the hypotheses that start from the same poses.
    -> dict(delta [12] mpf, kappa, cost0, cost1, rho, step_ratio, cost_ratio, gmax, valid)"""
    x = mpv(init)
    rows = {} if rows is None else rows
    Hm, g, cost0 = mp.zeros(12, 12), [M(0)] * 12, M(0)
    for i in subset:
        i = int(i)
        if i not in rows:
            rows[i] = pnp_rows(cam, x, shutter, scan, X[i], xy[i], tau_from_x_always)
        r, J = rows[i]
        cost0 += r[0] * r[0] + r[1] * r[1]
        for a in range(12):
            g[a] += J[0][a] * r[0] + J[1][a] * r[1]
            for b in range(a + 1):
                Hm[a, b] += J[0][a] * J[0][b] + J[1][a] * J[1][b]
    for a in range(12):
        for b in range(a):
            Hm[b, a] = Hm[a, b]
    cost0 /= 2
    s = [1 / (1 + mp.sqrt(Hm[a, a])) for a in range(12)]
    D = [s[a] * s[a] * Hm[a, a] for a in range(12)]
    D = [min(max(d, clamp_lo) if clamp_lo is not None else d, M("1e32")) for d in D]
    A = mp.matrix(12, 12)
    for a in range(12):
        for b in range(12):
            A[a, b] = s[a] * s[b] * Hm[a, b] + (D[a] / radius if a == b else 0)
    live = [a for a in range(12) if Hm[a, a] > 0]
    out = dict(cost0=cost0, valid=True, gmax=float(max(abs(v) for v in g)))
    if any(A[a, a] == 0 for a in range(12)):
        # a zero pivot: the factorisation fails, the step is invalid, and with one iteration the poses stay where they were
        out.update(valid=False, delta=[M(0)] * 12, kappa=INF)
        return out
    y = mp.lu_solve(A, mp.matrix([s[a] * g[a] for a in range(12)]))
    delta = [-s[a] * y[a] for a in range(12)]
    Af = np.array([[float(A[a, b]) for b in live] for a in live])
    kappa = float(np.linalg.cond(Af))
    xn = [x[a] + delta[a] for a in range(12)]
    cost1 = M(0)
    for i in subset:
        r, _ = pnp_rows(cam, xn, shutter, scan, X[int(i)], xy[int(i)], tau_from_x_always, jac=False)
        cost1 += r[0] * r[0] + r[1] * r[1]
    cost1 /= 2
    Hd = Hm * mp.matrix(delta)
    model_change = -mp.fsum(g[a] * delta[a] for a in range(12)) - mp.fsum(delta[a] * Hd[a] for a in range(12)) / 2
    out.update(delta=delta, kappa=kappa, cost1=cost1, rho=float((cost0 - cost1) / model_change),
               step_ratio=float(norm(delta) / (M("1e-8") * (norm(x) + M("1e-8")))), cost_ratio=float(abs(cost0 - cost1) / (M("1e-6") * cost0)),
               xn=xn)
    return out


# ======================================================================================================================================
# The input sets.  Item counts come from {1, 255, 256, 257, 600} (one lane per item in 256-thread blocks), hypothesis counts from
# {1, 63, 64, 65} (64-thread blocks).  Inputs are made with the model itself where an observation has to sit at a chosen place
# (on a threshold, at a chosen parallax): the model then evaluates the rounded doubles / floats like everything else.
# ======================================================================================================================================
def fl(v):
    return np.array([float(x) for x in v])


def c2w(pose, pc):
    """camera-frame point -> world"""
    r = mp_rotate([-pose[0], -pose[1], -pose[2]], list(pc))
    return [r[i] + pose[3 + i] for i in range(3)]


def backproject(cam, pose, pixel, depth):
    """the world point at camera-frame depth `depth` that projects to `pixel` under `pose`"""
    pu = undistort_newton(cam, [(pixel[0] - cam[7]) / cam[0], (pixel[1] - cam[8]) / cam[1]])
    return c2w(pose, [pu[0] * depth, pu[1] * depth, depth])


def scaled_cam(k):
    c = CAM.copy()
    c[[2, 3, 6]] *= k
    return c


def two_poses(rng, sep, axis=0, rot=0.02):
    p0 = np.concatenate([rng.normal(0, rot, 3), rng.normal(0, 0.1, 3)])
    d = np.array([0.05, 0.05, -0.04]); d[axis] = sep
    return np.stack([p0, p0 + np.concatenate([rng.normal(0, 0.01, 3), d])])


# ---- part A: reproject -------------------------------------------------------------------------------------------------------------
SEPS = (0.35, 5.0, 10.0, 13.0, 20.0)
A_HANDLE = [(GLOBAL, True, 255, (17, 1203)), (GLOBAL, False, 1, (1280, 0)), (HORIZONTAL, True, 600, (17, 1203)), (HORIZONTAL, False, 257, (1280, 0)),
            (VERTICAL, True, 256, (1280, 0)), (VERTICAL, False, 600, (17, 1203))]
A_FRAME = [("lines33", HORIZONTAL, 257), ("lines33", VERTICAL, 255), ("lines33", GLOBAL, 256), ("two", HORIZONTAL, 256), ("one", HORIZONTAL, 1), ("edge", HORIZONTAL, 255)]
CAM32 = np.array([30.0, 60.0, -0.05, 0.01, 1e-3, -1e-3, 2e-3, 16.0, 16.0])   # a 32 x 32 image: a pose per scan line is 33 poses


@functools.lru_cache(maxsize=None)
def reproject_handle_case(shutter, interp, n, scan):
    """A two-pose session of five frames whose poses lie 0.35, 5, 10, 13 and 20 apart along the shutter's axis (x; y for VERTICAL,
    whose tau follows y), points at depth 7 - 9 that project inside and on both sides of the scan range, some behind the camera"""
    rng = np.random.default_rng(1000 + 10 * shutter + interp)
    axis = 1 if shutter == VERTICAL else 0
    poses = np.stack([two_poses(rng, s, axis) for s in SEPS])
    frames = (np.arange(n) % len(SEPS)).astype(np.int32) if n > 1 else np.array([1], dtype=np.int32)
    z = rng.uniform(7, 9, n)
    a, b = rng.uniform(-1.05, 1.05, n), rng.uniform(-0.5, 0.5, n)
    if axis == 1:
        a, b = rng.uniform(-0.8, 0.8, n), rng.uniform(-0.6, 1.3, n)
    X = poses[frames, 0, 3:] + np.stack([a * z, b * z, z], 1)
    X[11::23, 2] = -3.0
    order = np.argsort(frames, kind="stable")
    prob = dict(poses=poses, points=X, intrinsics=CAM[None], obs_xy=np.tile([640.0, 360.0], (n, 1)), obs_frame=frames[order],
                obs_point=order.astype(np.int32), shutter=shutter, scanlines=scan, interpolate_rotation=interp)
    items = [(CAM, poses[f], X[j]) for j, f in enumerate(frames)]
    return dict(prob=prob, frames=frames, points=np.arange(n, dtype=np.int32), items=items, shutter=shutter, scan=scan, interp=interp,
                sep=[SEPS[f] for f in frames])


@functools.lru_cache(maxsize=None)
def reproject_frame_case(kind, shutter, n):
    """one frame, no handle: 33 poses (one per scan line of a 32-pixel image), two poses 10 apart, or one pose"""
    rng = np.random.default_rng(1100 + shutter + n)
    if kind == "lines33":
        cam, scan = CAM32, (0, 32)
        t = np.linspace(0, 1, 33)[:, None]
        p = two_poses(rng, 1.5, 1 if shutter != HORIZONTAL else 0)
        poses = p[0] * (1 - t) + p[1] * t
        z = rng.uniform(6, 10, n)
        X = poses[0, 3:] + np.stack([rng.uniform(-0.7, 0.7, n) * z, rng.uniform(-0.35, 0.35, n) * z, z], 1)
        X[:, 1 if shutter != HORIZONTAL else 0] += 0.75
    elif kind == "edge":
        # a contraction factor of about 0.775 spends the limit exactly: the items converge in 47 - 52 projections, and the 50th fails
        cam, scan = CAM, (0, 1280)
        poses = two_poses(rng, 10.0, rot=0.0)
        z = rng.uniform(7.8, 8.2, n)
        X = poses[0, 3:] + np.stack([rng.uniform(0.45, 0.75, n) * z, rng.uniform(-0.1, 0.1, n) * z, z], 1)
    else:
        cam, scan = CAM, (0, 1280)
        poses = two_poses(rng, 10.0)[: 2 if kind == "two" else 1]
        z = rng.uniform(7, 9, n)
        X = poses[0, 3:] + np.stack([rng.uniform(-0.8, 0.8, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)
    if kind != "edge":
        X[5::17, 2] = -4.0
    return dict(cam=cam, poses=poses, X=X, items=[(cam, poses, x) for x in X], shutter=shutter, scan=scan, interp=True)


@functools.lru_cache(maxsize=None)
def reproject_model(case_fn, *key, **variant):
    case = case_fn(*key)
    out = []
    for cam, poses, X in case["items"]:
        out.append(reproject(mpv(cam), [mpv(p) for p in poses], case["shutter"], case["scan"], mpv(X), case["interp"], **dict(variant)))
    return out


# ---- part B: validate --------------------------------------------------------------------------------------------------------------
B_HANDLE = [(GLOBAL, True, 255), (HORIZONTAL, True, 600), (HORIZONTAL, False, 256), (VERTICAL, True, 257), (VERTICAL, False, 600)]
B_FRAME = [(HORIZONTAL, 257), (VERTICAL, 256), (GLOBAL, 255), (HORIZONTAL, 1)]
B_THR, B_MIN = 25.0, 9.0
BAND = 64


def on_threshold(cam, poses, shutter, scan, interp, obs, depth, angle, sq_threshold, factor):
    """a point whose squared reprojection error against `obs` is sq_threshold * factor: back-project a pixel sqrt(sq_threshold)
    away, then slide the point along that image-plane direction"""
    pose, _ = get_pose(poses, shutter, scan, obs, interp)
    c, s = mp.cos(angle), mp.sin(angle)
    r = mp.sqrt(M(sq_threshold))
    X0 = backproject(cam, pose, [obs[0] + r * c, obs[1] + r * s], M(depth))
    u = mp_rotate([-pose[0], -pose[1], -pose[2]], [c, s, M(0)])
    target = M(sq_threshold) * factor

    def f(t):
        _, proj, _ = w2i(cam, pose, [X0[i] + t * u[i] for i in range(3)])
        return (proj[0] - obs[0]) ** 2 + (proj[1] - obs[1]) ** 2 - target
    t = mp.findroot(f, (M(0), M("1e-6")), tol=M("1e-30"), solver="secant")
    return fl([X0[i] + t * u[i] for i in range(3)])


@functools.lru_cache(maxsize=None)
def validate_handle_case(shutter, interp, n):
    """A two-pose session of six frames with two intrinsics blocks and (rolling shutters) a one-pose frame; n - 64 observations with
    pixel noise about the threshold and depths about min_distance, then the band: 64 observations whose squared error is
    threshold (1 +- 2^-20)"""
    rng = np.random.default_rng(2000 + 10 * shutter + interp)
    F = 6
    scan = (0, 1280) if shutter != VERTICAL else (0, 720)
    poses = np.stack([two_poses(rng, 0.35, 1 if shutter == VERTICAL else 0) + np.array([0, 0, 0, 0.5 * f, 0, 0]) for f in range(F)])
    cams = np.stack([CAM, CAM * np.array([1.1, 1.05, 1, 1, 1, 1, 1, 1, 1])])
    fcam = (np.arange(F) % 2).astype(np.int32)
    fglobal = np.zeros(F, dtype=np.uint8)
    if shutter != GLOBAL:
        fglobal[4] = 1
    frames = np.sort(np.arange(n) % F).astype(np.int32)
    X, xy = np.zeros((n, 3)), np.zeros((n, 2))
    for i in range(n):
        f = frames[i]
        cam = mpv(cams[fcam[f]])
        ps = [mpv(poses[f, 0])] if fglobal[f] else [mpv(p) for p in poses[f]]
        obs = mpv(rng.uniform([40, 40], [1240, 680]))
        if i >= n - BAND:
            k = i - (n - BAND)
            X[i] = on_threshold(cam, ps, shutter, scan, interp, obs, rng.uniform(10, 12), M(float(rng.uniform(0, 6.28))), B_THR,
                                1 + (M(2) ** -20) * (1 if k % 2 else -1))
            xy[i] = fl(obs)
        else:
            pose, _ = get_pose(ps, shutter, scan, obs, interp)
            X[i] = fl(backproject(cam, pose, obs, M(float(rng.uniform(6, 12)))))
            xy[i] = fl(obs) + rng.normal(0, 3.5, 2)
            if i % 29 == 7:
                X[i] = poses[f, 0, 3:] + np.array([0.3, 0.2, -5.0])
    perm = rng.permutation(n) if (shutter == HORIZONTAL and interp) else np.arange(n)       # one case is not frame-major
    frames, X, xy = frames[perm], X[perm], xy[perm]
    prob = dict(poses=poses, points=X, intrinsics=cams, obs_xy=xy, obs_frame=frames, obs_point=np.arange(n, dtype=np.int32), shutter=shutter,
                scanlines=scan, interpolate_rotation=interp, frame_intrinsics=fcam, frame_global=fglobal if fglobal.any() else None)
    items = [(cams[fcam[f]], poses[f, :1] if fglobal[f] else poses[f], X[i], xy[i]) for i, f in enumerate(frames)]
    band = np.zeros(n, dtype=bool); band[n - BAND:] = True
    return dict(prob=prob, items=items, shutter=shutter, scan=scan, interp=interp, thr=B_THR, min_dist=B_MIN, band=band[perm], half=np.zeros(n, dtype=bool))


@functools.lru_cache(maxsize=None)
def validate_frame_case(shutter, n):
    """one frame with 33 poses 0.4 apart: observations whose line coordinate is exactly k + 0.5 (the neighbouring pose shifts the
    projection by 1.5 px against a threshold of 1 px), one with a negative line coordinate, one beyond the last pose"""
    rng = np.random.default_rng(2100 + shutter + n)
    cam, scan, thr, min_dist = CAM32, (0, 32), 1.0, 8.0
    base = np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3)])
    poses = base + np.arange(33)[:, None] * np.array([0.0005, 0, 0, 0.4, 0, 0.0])
    ax = 0 if shutter == HORIZONTAL else 1
    X, xy, half = np.zeros((n, 3)), np.zeros((n, 2)), np.zeros(n, dtype=bool)
    for i in range(n):
        o = rng.uniform([2, 2], [30, 30])
        depth, noise = rng.uniform(6, 10), (0.3 if i % 10 < 7 else 2.0)
        if n > 1 and i % 6 == 0 and i // 6 < 40:
            o[ax], depth, noise, half[i] = (i // 6) % 32 + 0.5, rng.uniform(8.5, 10), 0.2, True
        if i == 1:
            o[ax] = -1.25
        if i == 2:
            o[ax] = 33.75
        pose, _ = get_pose([mpv(p) for p in poses], shutter, scan, mpv(o), True)
        th = rng.uniform(0, 6.28)
        X[i] = fl(backproject(mpv(cam), pose, mpv(o + noise * np.array([np.cos(th), np.sin(th)])), M(float(depth))))
        xy[i] = o
    X[9::31, 2] = -4.0
    return dict(cam=cam, poses=poses, X=X, xy=xy, items=[(cam, poses, X[i], xy[i]) for i in range(n)], shutter=shutter, scan=scan, interp=True,
                thr=thr, min_dist=min_dist, half=half, band=np.zeros(n, dtype=bool))


@functools.lru_cache(maxsize=None)
def validate_model(case_fn, *key, floor_index=False):
    case = case_fn(*key)
    index = (lambda line, n: (int(mp.floor(min(max(line, M(0)), M(n - 1)))), min(max(line, M(0)), M(n - 1)))) if floor_index else scanline_index
    return [validate(mpv(cam), [mpv(p) for p in poses], case["shutter"], case["scan"], mpv(X), mpv(obs), case["thr"], case["min_dist"],
                     case["interp"], index) for cam, poses, X, obs in case["items"]]


# ---- part C: track rays and triangulation ----------------------------------------------------------------------------------------------
C_CASES = [(HORIZONTAL, True, 600, 257), (VERTICAL, False, 256, 600), (GLOBAL, True, 255, 255), (HORIZONTAL, False, 257, 256), (VERTICAL, True, 1, 1)]
C_THR, C_MIN = 16.0, 4.0
ANGLES = (None, 1e-1, 1e-2, 1e-3, 1e-4, 3e-5)
C_NP = (1, 1, 1, 2, 5, 2, 1, 5, 2)                      # poses per frame; frames 0 and 1 are bitwise equal, frame 2 differs from them by a -0.0 (no solve between 0 and 1, one between 0 and 2)
C_FCAM = (0, 0, 0, 0, 1, 0, 2, 1, 3)                    # CAM, and CAM with (k1, k2, k3) times 8, 12 and (frame 8, a handful of items) 16


def _project_into(cams, fcam, fposes, f, shutter, scan, interp, X):
    r = reproject(mpv(cams[fcam[f]]), [mpv(p) for p in fposes[f]], shutter, scan, mpv(X), interp)
    return fl(r["xy"]) if r["ok"] else None


@functools.lru_cache(maxsize=None)
def tracks_case(shutter, interp, n_obs, n_cand):
    """Nine frames with 1, 2 and 5 poses and four cameras.  Observations come in pairs, the two views of one point: ordinary points
    (depth 2 - 12, 1.5 px of noise) and points at the distance that gives the pair of rays a parallax of 1e-1 ... 3e-5 (no noise).
    The first candidates are those pairs, the others random pairs of observations (false matches, equal poses, one frame twice)."""
    rng = np.random.default_rng(3000 + 10 * shutter + interp)
    scan = (0, 1280) if shutter != VERTICAL else (0, 720)
    cams = np.stack([CAM, scaled_cam(8), scaled_cam(12), scaled_cam(16)])
    fposes = []
    for f, k in enumerate(C_NP):
        c = np.array([0.3 * f, 0.02 * np.sin(f), 0.0]) if f > 2 else np.array([0.5, 0.1, 0.25])   # (not the origin: a solve between frames 0 and 2 writes a point that is not 0)
        w = rng.normal(0, 0.02, 3) if f > 2 else np.zeros(3)
        fposes.append(np.stack([np.concatenate([w + q * rng.normal(0, 0.002, 3), c + q * np.array([0.01, 0.003, 0.0])]) for q in range(k)]))
    fposes[2][0, 2] = -0.0
    of, oxy, opt = [], [], []
    while len(of) < n_obs:
        j = len(of) // 2
        fa, fb = rng.choice(np.arange(3, 8), 2, replace=False)
        if j % 9 == 4:
            fa, fb = rng.choice(3, 2, replace=False)            # among the three frames that share a centre
        if j % 40 == 7:
            fb = 8
        ang = ANGLES[j % len(ANGLES)]
        ca, cb = fposes[fa][0, 3:], fposes[fb][0, 3:]
        if ang is None or np.allclose(ca, cb):
            X = np.array([rng.uniform(-1, 3), rng.uniform(-1.5, 1.5), rng.uniform(2, 12)])
            noise = 1.5
        else:
            d = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), 1.0]); d /= np.linalg.norm(d)
            b = cb - ca
            X = (ca + cb) / 2 + d * np.linalg.norm(b - d * (b @ d)) / ang
            noise = 0.0
        for f in (fa, fb):
            xy = _project_into(cams, C_FCAM, fposes, f, shutter, scan, interp, X)
            if xy is None or not (0 < xy[0] < 1280 and 0 < xy[1] < 720) or (C_FCAM[f] >= 2 and j % 3 == 0):
                xy = rng.uniform([0, 0], [1280, 720])          # (strong distortion: any pixel, up to the fold where the undistortion crawls or fails)
            of.append(int(f)); oxy.append(xy + rng.normal(0, noise, 2) if noise else xy); opt.append(X)
    of, oxy, opt = np.array(of[:n_obs], dtype=np.int32), np.array(oxy[:n_obs]), np.array(opt[:n_obs])
    npair = min(n_obs // 2, n_cand)
    ca = np.concatenate([2 * np.arange(npair), rng.integers(0, n_obs, n_cand - npair)]).astype(np.int32)
    cb = np.concatenate([2 * np.arange(npair) + 1, rng.integers(0, n_obs, n_cand - npair)]).astype(np.int32)
    if n_obs == 1:
        ca = cb = np.zeros(1, dtype=np.int32)
    request = rng.integers(1, 4, n_cand).astype(np.uint8)
    request[:npair] |= 1
    track_pt = opt[ca] + rng.normal(0, 0.01, (n_cand, 3))
    return dict(cams=cams, fcam=np.array(C_FCAM, dtype=np.int32), fposes=fposes, shutter=shutter, scan=scan, interp=interp, of=of, oxy=oxy, ca=ca, cb=cb,
                request=request, track_pt=track_pt, thr=C_THR, min_dist=C_MIN, angle=[ANGLES[(int(a) // 2) % len(ANGLES)] if c < npair else None for c, a in enumerate(ca)])


@functools.lru_cache(maxsize=None)
def parallel_case():
    """the same pixel in two frames that share the camera and a zero rotation but not the centre: exactly parallel rays, det(A) about
    0 — undecided by design"""
    rng = np.random.default_rng(3100)
    fposes = [np.zeros((1, 6)), np.array([[0, 0, 0, 0.5, 0.1, 0.0]])]
    oxy = np.repeat(rng.uniform([100, 100], [1180, 620], (32, 2)), 2, axis=0)
    of = np.tile([0, 1], 32).astype(np.int32)
    return dict(cams=CAM[None], fcam=np.zeros(2, dtype=np.int32), fposes=fposes, shutter=GLOBAL, scan=(0, 1280), interp=True, of=of, oxy=oxy,
                ca=(2 * np.arange(32)).astype(np.int32), cb=(2 * np.arange(32) + 1).astype(np.int32), request=np.ones(32, dtype=np.uint8),
                track_pt=np.zeros((32, 3)), thr=C_THR, min_dist=0.0)


def _selected_rows(case, f, xy):
    """the input pose rows getPose reads for this observation (for the bitwise comparison of two poses)"""
    P = case["fposes"][f]
    if len(P) == 1 or (len(P) == 2 and case["shutter"] == GLOBAL):
        return P[0].tobytes()
    if len(P) > 2:
        k, _ = scanline_index(M(float(xy[0] if case["shutter"] == HORIZONTAL else xy[1])), len(P))
        return P[k].tobytes()
    return None


def tracks_model(case, C_C, stop_early=0):
    """per candidate: dict(tri_ok, solved, p, reproj_ok, det, cond, amp, bound, decided_tri, decided_rep).  C_C enters the margins of
    the tests made ON the triangulated point: they must clear the error that point may carry."""
    cams = [mpv(c) for c in case["cams"]]
    sh, scan, interp, thr, mind = case["shutter"], case["scan"], case["interp"], case["thr"], case["min_dist"]
    obs = []
    for f, xy in zip(case["of"], case["oxy"]):
        cam, xym = cams[case["fcam"][f]], mpv(xy)
        pose, _ = get_pose([mpv(p) for p in case["fposes"][f]], sh, scan, xym, interp)
        ray, u = pixel_ray(cam, pose, xym, stop_early=stop_early)
        obs.append(dict(cam=cam, pose=pose, xy=xym, ray=ray, u=u, rows=_selected_rows(case, f, xy), f=int(f)))
    out = []
    for c in range(len(case["ca"])):
        a, b, rq = obs[case["ca"][c]], obs[case["cb"][c]], int(case["request"][c])
        r = dict(tri_ok=False, solved=False, p=None, reproj_ok=False, det=None, cond=None, amp=None, bound=None, decided_tri=True, decided_rep=True)
        if rq & 2:
            X = mpv(case["track_pt"][c])
            d = norm([a["pose"][3 + i] - X[i] for i in range(3)])
            ok, proj, z = w2i(a["cam"], a["pose"], X)
            e2 = (proj[0] - a["xy"][0]) ** 2 + (proj[1] - a["xy"][1]) ** 2 if ok else None
            r["reproj_ok"] = bool(not (d < mind) and ok and e2 < thr)
            r["decided_rep"] = rel(d, M(mind)) > 1e-12 and rel(z, Z_GATE) > 1e-6 and (not ok or rel(e2, M(thr)) > 1e-9)
        if rq & 1:
            if a["rows"] is not None and b["rows"] is not None:
                same = a["rows"] == b["rows"]
            else:
                same = a["f"] == b["f"] and all(x == y for x, y in zip(a["pose"], b["pose"]))
            dec = True
            if not same:
                dec = a["u"]["margins"]["undistort"] > 1e-5 and b["u"]["margins"]["undistort"] > 1e-5
            if not same and a["ray"] is not None and b["ray"] is not None:
                p, det, cond = triangulate(a["pose"][3:], a["ray"], b["pose"][3:], b["ray"])
                r.update(det=float(det), cond=cond)
                dec = dec and abs(det - DBL_EPS) > M("1e-12")
                if det >= DBL_EPS and p is not None:
                    amp = max(a["u"]["amp"], b["u"]["amp"])
                    scale = max(abs(v) for v in a["pose"][3:]) + max(abs(v) for v in b["pose"][3:]) + max(abs(v) for v in p)
                    unit = cond * EPS53 * float(scale) * amp
                    r.update(solved=True, p=fl(p), amp=amp, unit=unit, bound=C_C * unit)
                    ok = True
                    for o in (a, b):
                        d = norm([o["pose"][3 + i] - p[i] for i in range(3)])
                        dec = dec and abs(d - mind) > 2 * r["bound"] + M("1e-12") * d
                        ok = ok and not (d < mind)
                    for o in (a, b) if ok else ():             # (a point too near a camera is refused before any projection is made)
                        good, proj, z = w2i(o["cam"], o["pose"], p)
                        dec = dec and abs(z - Z_GATE) > 2 * r["bound"]
                        if not good:
                            ok = False
                            continue
                        e = mp.sqrt((proj[0] - o["xy"][0]) ** 2 + (proj[1] - o["xy"][1]) ** 2)
                        dec = dec and abs(e - mp.sqrt(M(thr))) > 4 * (o["cam"][0] + o["cam"][1]) * r["bound"] / z + M("1e-9")
                        ok = ok and e * e < thr
                    r["tri_ok"] = bool(ok)
            r["decided_tri"] = bool(dec)
        out.append(r)
    return out, obs


# ---- part D: PnP scoring ---------------------------------------------------------------------------------------------------------------
D_CASES = [(HORIZONTAL, 257, 65), (VERTICAL, 256, 1), (GLOBAL, 255, 65), (VERTICAL, 1, 1), (HORIZONTAL, 255, 1)]
D_THR = 8.0


def pnp_truth(rng, shutter):
    scan = (0, 1280) if shutter != VERTICAL else (0, 720)
    pose0 = np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.3, 3)])
    pose1 = pose0 + np.concatenate([rng.normal(0, 0.01, 3), [0.35, 0.05, -0.04]])
    return scan, np.stack([pose0, pose1])


def pnp_observe(rng, shutter, scan, poses, n, noise):
    """n float32 points in view of the frame and their float32 observations (the model's fixed point plus noise)"""
    X, xy = [], []
    cam, ps = mpv(CAM), [mpv(p) for p in poses]
    while len(X) < n:
        x = np.array([rng.uniform(-5, 5), rng.uniform(-3, 3), rng.uniform(6, 14)]).astype(np.float32)
        r = reproject(cam, ps, shutter, scan, mpv(x))
        if r["ok"] and 0 < r["xy"][0] < 1280 and 0 < r["xy"][1] < 720:
            X.append(x); xy.append(fl(r["xy"]) + rng.normal(0, noise, 2))
    return np.array(X, dtype=np.float32), np.array(xy).astype(np.float32)


@functools.lru_cache(maxsize=None)
def score_case(shutter, n, H):
    """n points against H given pose pairs (per-task initial poses, zero iterations).  The first min(32, n) observations sit in the
    image's corner (|ix|, |iy| < 8, where the float32 grid is fine enough) at a distance thr (1 +- 16 * 2^-24) from their projection
    under pose pair 0; the rest carry 5 px of noise against thr = 8; a few points lie behind the camera (no z gate here)."""
    rng = np.random.default_rng(4000 + 10 * shutter + n + H)
    scan, poses = pnp_truth(rng, shutter)
    inits = poses.reshape(1, 12) + np.concatenate([np.zeros((1, 12)), rng.normal(0, 1, (H - 1, 12)) * np.tile([0.002] * 3 + [0.03] * 3, 2)])
    X, xy = pnp_observe(rng, shutter, scan, poses, n, 5.0)
    for i in range(40, n, 37):
        X[i, 2] = -5.0
    cam, ps, thr = mpv(CAM), [mpv(p) for p in inits[0].reshape(2, 6)], M(f32(D_THR))
    nb = min(32, n)
    fixed = 1 if shutter == VERTICAL else 0            # the coordinate that sets tau stays put; the other one is tuned
    for i in range(nb):
        o = np.array(rng.uniform(1, 7, 2), dtype=np.float32)
        pose, _ = get_pose(ps, HORIZONTAL if shutter != GLOBAL else GLOBAL, scan, [M(float(o[fixed]))] * 2, True)
        q = [M(0), M(0)]
        q[fixed] = M(float(o[fixed])) + M(float(rng.uniform(-0.5, 0.5)))
        q[1 - fixed] = M(float(rng.uniform(-7.5, -2.0)))
        X[i] = fl(backproject(cam, pose, q, M(float(rng.uniform(6, 14))))).astype(np.float32)
        target = thr * (1 + (1 if i % 2 else -1) * 16 * M(2) ** -24)
        _, proj, _ = w2i(cam, pose, mpv(X[i]), gate=False)
        o[1 - fixed] = np.float32(float(proj[1 - fixed] + mp.sqrt(target ** 2 - (proj[fixed] - M(float(o[fixed]))) ** 2)))
        best = None
        for _ in range(200):
            d = pnp_score(cam, ps, shutter, scan, X[i], o, D_THR)[2]
            if best is None or abs(d - target) < best[0]:
                best = (abs(d - target), o.copy())
            elif abs(d - target) > best[0]:
                break
            o[1 - fixed] = np.nextafter(o[1 - fixed], np.float32(100.0 if d < target else -100.0))
        xy[i] = best[1]
    subs = np.stack([rng.choice(n, 6, replace=False) for _ in range(H)]).astype(np.int32) if n >= 6 else np.zeros((H, 1), dtype=np.int32)
    return dict(shutter=shutter, scan=scan, X=X, xy=xy, inits=inits, subs=subs, thr=D_THR, band=nb)


@functools.lru_cache(maxsize=None)
def score_model(shutter, n, H, tau_from_x=False):
    """[H][n] of (inlier, |dist - thr|, dist)"""
    c = score_case(shutter, n, H)
    cam = mpv(CAM)
    return [[pnp_score(cam, [mpv(p) for p in init.reshape(2, 6)], shutter, c["scan"], c["X"][i], c["xy"][i], c["thr"], tau_from_x) for i in range(n)]
            for init in c["inits"]]


def score_decided(case, row):
    lim = np.array([4 * 2.0 ** -24 * max(abs(float(ix)), abs(float(iy)), f32(case["thr"])) for ix, iy in case["xy"]])
    return np.array([r[1] for r in row]) > lim


# ---- part E: one LM step of the hypothesis kernel ----------------------------------------------------------------------------------------
E_CALLS = [(1, 64), (63, 6), (64, 7), (65, 20)]            # (hypotheses, subset size); plus three per-task initial poses with m = 6
E_N = 80


@functools.lru_cache(maxsize=None)
def step_scene(shutter):
    rng = np.random.default_rng(5000 + shutter)
    scan, poses = pnp_truth(rng, shutter)
    X, xy = pnp_observe(rng, shutter, scan, poses, E_N, 0.4)
    init = poses + np.concatenate([rng.normal(0, 0.01, (2, 3)), rng.normal(0, 0.08, (2, 3))], axis=1)
    return dict(shutter=shutter, scan=scan, X=X, xy=xy, init=init.reshape(12), poses=poses, rows={})


@functools.lru_cache(maxsize=None)
def step_call(shutter, H, m, per_task=False):
    sc = step_scene(shutter)
    rng = np.random.default_rng(5100 + 10 * shutter + H + m)
    subs = np.stack([rng.choice(E_N, m, replace=False) for _ in range(H)]).astype(np.int32)
    if H > 2:
        subs[H - 1] = subs[0]                            # two hypotheses of a call may share a subset; not all do
    inits = sc["init"][None]
    if per_task:
        inits = sc["init"][None] + rng.normal(0, 1, (H, 12)) * np.tile([0.003] * 3 + [0.03] * 3, 2)
    return dict(sc, subs=subs, inits=inits, per_task=per_task)


@functools.lru_cache(maxsize=None)
def step_model(shutter, H, m, per_task=False, **variant):
    c = step_call(shutter, H, m, per_task)
    cam, out, done = mpv(CAM), [], {}
    share = step_scene(shutter)["rows"] if not (per_task or variant) else None
    for h in range(H):
        key = (c["subs"][h].tobytes(), h if per_task else 0)
        if key not in done:
            done[key] = lm_step(cam, shutter, c["scan"], c["X"], c["xy"], c["subs"][h], c["inits"][h if per_task else 0], rows=share, **variant)
        out.append(done[key])
    return out
