"""Extended-precision restatement of the DLT start pose of a RANSAC hypothesis (include/rsba/solve_rs_pnp.hpp:
hyp_detail::normalised_point and pnp_detail::dlt_pose with what it calls), in mpmath at 60 digits, and the fixed case list the host
test (test_pnp_dlt_reference.py) and the device test (test_gpu_pnp_dlt.py) share.  It shares no code with the C++: the
eigen-decompositions are mpmath's (eigsy), not cyclic Jacobi; the nearest rotation is the limit of R <- (R + R^-T) / 2.
Where the C++ computes in float because its operands are (the quotients point / m that make the centroid), so does this: the
planar branch drops each point's component along the plane's normal, so its pose depends on the centroid at that level.

dlt(...) returns per subset
  branch   0 declined, 1 general DLT, 2 planar branch (the status rsba_pnp_dlt reports)
  pose     rsba's 6-vector (angle-axis world->camera, camera centre), floats; None when declined
  ratios   the tested quantities that were reached, by name: 'val1/val2' (declined below 1e-4), 'val0/val1' (planar below
           1e-3), 'gap1/gap2' (declined below 1e-9), 'gap0/gap1' (declined above 0.05)
  kappa    gap[2] / gap[1] of the 12 x 12 eigenproblem that produced the pose (the planar branch: the homography's)
"""
import numpy as np
from mpmath import mp, mpf, matrix, eigsy, sqrt, acos, sin, cos

mp.dps = 60
EPS = 2.0 ** -52
THRESHOLDS = {"val1/val2": 1e-4, "val0/val1": 1e-3, "gap1/gap2": 1e-9, "gap0/gap1": 0.05}


def _normalise(cam, u, v):
    fx, fy, k1, k2, p1, p2, k3, cx, cy = [mpf(float(c)) for c in cam]
    pn = ((mpf(float(u)) - cx) / fx, (mpf(float(v)) - cy) / fy)
    x, y = pn
    for _ in range(20):
        r2 = x * x + y * y
        d = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = d * x + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = d * y + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = x - (dx - pn[0]), y - (dy - pn[1])
    return x, y


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _smallest(A):
    """(eigenvector of the smallest eigenvalue, [smallest, second, largest]) of a symmetric mp matrix"""
    E, Q = eigsy(A)
    order = sorted(range(len(E)), key=lambda i: E[i])
    b = order[0]
    return [Q[k, b] for k in range(A.rows)], [E[order[0]], E[order[1]], E[order[-1]]]


def _nearest_rotation(R):
    for _ in range(30):
        if abs(mp.det(R)) <= mpf("1e-12"):
            return None
        R = (R + (R ** -1).T) / 2
    return R if mp.det(R) > 0 else None


def _rotate(w, p):
    th2 = sum(x * x for x in w)
    wxp = _cross(w, p)
    if th2 > mpf(2.220446049250313e-16):
        th = sqrt(th2)
        k = [x / th for x in w]
        kxp = [x / th for x in wxp]
        kp = sum(a * b for a, b in zip(k, p)) * (1 - cos(th))
        return [p[i] * cos(th) + kxp[i] * sin(th) + k[i] * kp for i in range(3)]
    return [p[i] + wxp[i] for i in range(3)]


def _pose_from_rt(R, tvec):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cs = min(mpf(1), max(mpf(-1), (tr - 1) / 2))
    th = acos(cs)
    ax = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    sn = sqrt(sum(a * a for a in ax)) / 2
    if sn > mpf("1e-8"):
        rvec = [a * th / (2 * sn) for a in ax]
    elif cs > 0:
        rvec = [a / 2 for a in ax]
    else:   # a half turn: the axis from the diagonal, its first component positive
        d = [sqrt(max(mpf(0), (R[i, i] + 1) / 2)) for i in range(3)]
        rvec = [th * d[0], th * d[1] * (1 if R[0, 1] + R[1, 0] >= 0 else -1), th * d[2] * (1 if R[0, 2] + R[2, 0] >= 0 else -1)]
    centre = _rotate([-r for r in rvec], [-t for t in tvec])
    return [float(x) for x in rvec + centre]


def dlt_one(cam, X, xy, idx):
    """One subset.  X [n,3] float32, xy [n,2] float32, idx the subset's indices (repeats allowed)."""
    m = len(idx)
    out = dict(branch=0, pose=None, ratios={}, kappa=None)
    if m < 6:
        return out
    P = [[mpf(float(X[i, k])) for k in range(3)] for i in idx]
    uv = [_normalise(cam, xy[i, 0], xy[i, 1]) for i in idx]
    # (the object points are float and so is each quotient point / m of the centroid: a float32 division, part of the definition)
    c = [sum(mpf(float(np.float32(X[i, k]) / np.float32(m))) for i in idx) for k in range(3)]
    scale = sum(sqrt(sum((p[k] - c[k]) ** 2 for k in range(3))) for p in P) / m
    if not scale > 0:
        return out
    D = [[(p[k] - c[k]) / scale for k in range(3)] for p in P]
    S = matrix(3, 3)
    for d in D:
        for a in range(3):
            for b in range(3):
                S[a, b] += d[a] * d[b]
    E, Q = eigsy(S)
    order = sorted(range(3), key=lambda i: E[i])
    val = [E[i] for i in order]
    vec = [[Q[r, i] for r in range(3)] for i in order]
    out["ratios"]["val1/val2"] = float(val[1] / val[2])
    if not val[1] > mpf(1e-4) * val[2]:
        return out
    out["ratios"]["val0/val1"] = float(val[0] / val[1])
    planar = val[0] < mpf(1e-3) * val[1]
    A = matrix(12, 12)
    if planar:
        e1, e2 = vec[2], vec[1]
        nrm = _cross(e1, e2)
        cu, cv = sum(p[0] for p in uv) / m, sum(p[1] for p in uv) / m
        su = sum(sqrt((p[0] - cu) ** 2 + (p[1] - cv) ** 2) for p in uv) / m
        if not su > 0:
            return out
        su /= sqrt(mpf(2))
        for d, p in zip(D, uv):
            x, y = sum(d[k] * e1[k] for k in range(3)), sum(d[k] * e2[k] for k in range(3))
            u, v = (p[0] - cu) / su, (p[1] - cv) / su
            for row in ([x, y, 1, 0, 0, 0, -u * x, -u * y, -u], [0, 0, 0, x, y, 1, -v * x, -v * y, -v]):
                for a in range(9):
                    for b in range(9):
                        A[a, b] += row[a] * row[b]
        big = sum(A[a, a] for a in range(9))
        if not big > 0:
            return out
        for a in range(9, 12):
            A[a, a] = 2 * big
    else:
        for d, p in zip(D, uv):
            Xh = d + [mpf(1)]
            r0 = Xh + [mpf(0)] * 4 + [-p[0] * x for x in Xh]
            r1 = [mpf(0)] * 4 + Xh + [-p[1] * x for x in Xh]
            for row in (r0, r1):
                for a in range(12):
                    for b in range(12):
                        A[a, b] += row[a] * row[b]
    h, gap = _smallest(A)
    out["ratios"]["gap1/gap2"] = float(gap[1] / gap[2])
    if not gap[1] > mpf(1e-9) * gap[2]:
        return out
    out["ratios"]["gap0/gap1"] = float(gap[0] / gap[1])
    if not gap[0] < mpf(0.05) * gap[1]:
        return out
    out["kappa"] = float(gap[2] / gap[1])
    if planar:
        H = matrix(3, 3)
        for k in range(3):
            H[0, k] = su * h[k] + cu * h[6 + k]; H[1, k] = su * h[3 + k] + cv * h[6 + k]; H[2, k] = h[6 + k]
        if H[2, 2] < 0:
            H = -H
        n1 = sqrt(sum(H[r, 0] ** 2 for r in range(3))); n2 = sqrt(sum(H[r, 1] ** 2 for r in range(3)))
        if not (n1 > 0 and n2 > 0):
            return out
        r1 = [H[r, 0] / n1 for r in range(3)]; r2 = [H[r, 1] / n2 for r in range(3)]; r3 = _cross(r1, r2)
        lam = (n1 + n2) / 2
        tp = [H[r, 2] / lam for r in range(3)]
        Rp = _nearest_rotation(matrix([[r1[r], r2[r], r3[r]] for r in range(3)]))
        if Rp is None:
            return out
        R = Rp * matrix([e1, e2, nrm])
        tvec = [scale * tp[r] - sum(R[r, k] * c[k] for k in range(3)) for r in range(3)]
    else:
        M = matrix([[h[4 * r + k] for k in range(3)] for r in range(3)])
        t = [h[4 * r + 3] for r in range(3)]
        if t[2] < 0:
            M = -M; t = [-x for x in t]
        lam = sum(sqrt(sum(M[r, k] ** 2 for k in range(3))) for r in range(3)) / 3
        if not lam > 0:
            return out
        R = _nearest_rotation(M / lam)
        if R is None:
            return out
        tvec = [scale * t[r] / lam - sum(R[r, k] * c[k] for k in range(3)) for r in range(3)]
    out["pose"] = _pose_from_rt(R, tvec)
    out["branch"] = 2 if planar else 1
    return out


# ---------------------------------------------------------------- the shared cases ----------------------------------------------------------------
CAM_DIST = np.array([800.0, 800.0, -0.05, 0.01, 1e-3, -1e-3, 2e-3, 640.0, 360.0])
CAM_PLAIN = np.array([800.0, 800.0, 0.0, 0.0, 0.0, 0.0, 0.0, 640.0, 360.0])
CAM_EXACT = np.array([768.0, 768.0, 0.0, 0.0, 0.0, 0.0, 0.0, 640.0, 360.0])


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def project(cam, pose, X):
    """pinhole + the radial / tangential distortion of the sfm intrinsics, global shutter"""
    fx, fy, k1, k2, p1, p2, k3, cx, cy = cam
    pc = (np.asarray(X, dtype=np.float64) - pose[3:]) @ _rodrigues(pose[:3]).T
    x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    r2 = x * x + y * y
    d = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = d * x + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = d * y + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def _main_scene(cam, seed):
    """40 points seen from one pose: 0..23 a general cloud, 24..33 on a tilted plane, 34..39 on a line; 65 six-point subsets:
    0..47 general, 48..53 from the plane, 54..56 the line, 57..60 one point named twice, 61..64 plane and cloud mixed"""
    rng = np.random.default_rng(seed)
    pose = np.array([0.08, -0.12, 0.05, 0.4, -0.3, 0.2])
    X = np.zeros((40, 3))
    X[:24] = np.stack([rng.uniform(-4, 4, 24), rng.uniform(-2.5, 2.5, 24), rng.uniform(7, 14, 24)], axis=1)
    ab = rng.uniform(-3, 3, (10, 2))
    X[24:34] = np.stack([ab[:, 0], ab[:, 1], 10 + 0.3 * ab[:, 0] - 0.2 * ab[:, 1]], axis=1)
    s = np.linspace(-3, 3, 6)
    X[34:] = np.array([0.5, -0.2, 9.0]) + s[:, None] * np.array([1.0, 0.4, 0.7])
    X = X.astype(np.float32)
    xy = project(cam, pose, X).astype(np.float32)
    subs = [rng.choice(24, 6, replace=False) for _ in range(48)]
    subs += [24 + rng.choice(10, 6, replace=False) for _ in range(6)]
    subs += [34 + rng.permutation(6) for _ in range(3)]
    for _ in range(4):
        s5 = rng.choice(24, 5, replace=False)
        subs.append(np.concatenate([s5, s5[:1]]))
    subs += [np.concatenate([24 + rng.choice(10, 3, replace=False), rng.choice(24, 3, replace=False)]) for _ in range(4)]
    return dict(cam=cam, X=X, xy=xy, subsets=np.array(subs, dtype=np.int32), pose=pose)


def _half_turn_scene():
    """A camera a half turn (about (1, 2, 2) / 3) away from the identity, with EXACT data: integer camera-frame points at depths
    3 * 2^k seen through fx = fy = 768, so that every float32 image and object coordinate is exact and the recovered rotation is
    symmetric to rounding — pose_from_rt takes its half-turn branch, well conditioned because no axis component is small."""
    N = np.array([[-7, 4, 4], [4, -1, 8], [4, 8, -1]])          # 9 R, R = 2 a a^T - I
    t = np.array([1, -2, 3])
    pts = []
    rng = np.random.default_rng(5)
    while len(pts) < 12:
        z = int(rng.choice([3, 6, 12, 24])); x = int(rng.integers(-z // 2, z // 2 + 1)); y = int(rng.integers(-z // 3, z // 3 + 1))
        d = np.array([x, y, z]) - t
        if (d[0] + 2 * d[1] + 2 * d[2]) % 9 == 0 and (x, y, z) not in pts:
            pts.append((x, y, z))
    Pc = np.array(pts)
    X = ((Pc - t) @ N.T) // 9                                     # X = R^T (Pc - t), R symmetric; exact integers
    assert np.array_equal(X @ N.T + 9 * t, 9 * Pc)
    xy = np.stack([768.0 * Pc[:, 0] / Pc[:, 2] + 640.0, 768.0 * Pc[:, 1] / Pc[:, 2] + 360.0], axis=1)
    assert np.array_equal(xy.astype(np.float32).astype(np.float64), xy)
    subs = [rng.choice(12, 6, replace=False) for _ in range(3)] + [np.arange(12)[:6], np.arange(12)[6:]]
    a = np.array([1.0, 2.0, 2.0]) / 3.0
    R = 2 * np.outer(a, a) - np.eye(3)
    pose = np.concatenate([np.pi * a, -R.T @ t])
    return dict(cam=CAM_EXACT, X=X.astype(np.float32), xy=xy.astype(np.float32), subsets=np.array(subs, dtype=np.int32), pose=pose)


def cases():
    """name -> dict(cam, X [n,3] float32, xy [n,2] float32, subsets [T,m] int32, pose)"""
    out = {}
    out["main_distorted"] = _main_scene(CAM_DIST, 11)             # 40 points, 65 subsets: one full wave and one lane
    out["main_plain"] = _main_scene(CAM_PLAIN, 12)
    rng = np.random.default_rng(21)
    base = out["main_distorted"]
    out["m12"] = dict(base, subsets=np.array([rng.choice(24, 12, replace=False) for _ in range(4)], dtype=np.int32))
    out["m_all"] = dict(base, subsets=np.arange(40, dtype=np.int32)[None, :])                                   # m = n = 40
    out["half_turn"] = _half_turn_scene()
    out["single"] = dict(base, X=base["X"][:6], xy=base["xy"][:6], subsets=np.arange(6, dtype=np.int32)[None, :])   # num_tasks = 1, m = n = 6
    return out


_REFERENCE = {}


def reference(name):
    """the extended-precision results of one case, computed once per process"""
    if name not in _REFERENCE:
        c = cases()[name]
        _REFERENCE[name] = [dlt_one(c["cam"], c["X"], c["xy"], list(s)) for s in c["subsets"]]
    return _REFERENCE[name]
