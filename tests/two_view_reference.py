"""Extended-precision reference of the two-view bootstrap (include/rsba_amd.h: rsba_epipolar_eight_point / rsba_epipolar_score; host form
epi_detail::eight_point / score in include/rsba/two_view.hpp), in mpmath at 60 digits, and the fixed case list the host test
(test_two_view_reference.py) and the device test (test_gpu_two_view.py) share.  It shares no code with the C++ and takes another way to
every number: the null vector is the last right singular vector of mpmath's SVD of the m x 9 constraint matrix itself (no Gram matrix, no
Jacobi), the manifold projection and the decomposition come from mpmath's SVD of the 3 x 3 matrix, the depths from the exact 2 x 2 solve.

solve_one(...) returns per subset
  status     0 declined, 1 solved
  E          the essential matrix (row-major, b^T E a = 0, sign: largest entry positive), floats; None when declined
  pose       rsba's 6-vector of camera B in A's frame (unit baseline) for the candidate with the most inliers in front over ALL the case's
             correspondences at THRESHOLD_PX, floats
  unit_E, unit_pose   the error unit per component, (kappa_k + |value_k|) 2^-52, kappa_k = sum_j |d value_k / d x_j| |x_j| over the 4 m
             normalised image coordinates of the subset.  kappa needs two digits, not sixty: central differences (h = 1e-6) of an fp64
             numpy restatement of the same map (numpy's SVD), aligned to the reference's sign and candidate
  gap        second-smallest eigenvalue of the Gram matrix over the value the gap test compares it with (declined below 1; None: declined earlier)
  kappa_max, leave_out   the subset may be left out of the ACCURACY check (never of the status check): kappa_max > 1e6
"""
import numpy as np
from mpmath import mp, mpf, matrix, sqrt, svd_r

from p3p_reference import CAM_DIST, CAM_EXACT, CAM_PLAIN, _pose_from_rt, _rodrigues, normalise, project

mp.dps = 60
EPS = 2.0 ** -52
THRESHOLD_PX = 4.0
W = matrix([[0, -1, 0], [1, 0, 0], [0, 0, 1]])


def _hartley(pts):
    m = len(pts)
    cx, cy = sum(p[0] for p in pts) / m, sum(p[1] for p in pts) / m
    s = sum(sqrt((p[0] - cx) ** 2 + (p[1] - cy) ** 2) for p in pts) / m
    return cx, cy, s / sqrt(mpf(2))


def _det3(M):
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
            + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))


def _essential(pa, pb):
    """the eight-point matrix of the normalised points pa, pb (lists of mp pairs); None: declined"""
    m = len(pa)
    ax, ay, sa = _hartley(pa)
    bx, by, sb = _hartley(pb)
    if not sa > 0 or not sb > 0:
        return None
    rows = []
    for (xa, ya), (xb, yb) in zip(pa, pb):
        xa, ya, xb, yb = (xa - ax) / sa, (ya - ay) / sa, (xb - bx) / sb, (yb - by) / sb
        rows.append([xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, mpf(1)])
    rows += [[mpf(0)] * 9] * max(0, 9 - m)
    _, S, V = svd_r(matrix(rows))
    sv = sorted(((S[i], i) for i in range(9)), key=lambda p: -p[0])
    trace = sum(s * s for s, _ in sv)
    _essential.gap = float(sv[7][0] ** 2 / (mpf(1e-9) * 2 * trace))   # how far the subset is from the gap test that declines it (1 = on it)
    if not sv[7][0] ** 2 > mpf(1e-9) * 2 * trace or not sv[8][0] ** 2 < mpf(0.05) * sv[7][0] ** 2:
        return None
    e = [V[sv[8][1], k] for k in range(9)]
    Fn = matrix(3, 3)
    for r in range(3):
        for k in range(3):
            Fn[r, k] = e[3 * r + k]
    Ta = matrix([[1 / sa, 0, -ax / sa], [0, 1 / sa, -ay / sa], [0, 0, 1]])
    Tb = matrix([[1 / sb, 0, -bx / sb], [0, 1 / sb, -by / sb], [0, 0, 1]])
    F = Tb.T * Fn * Ta
    U, S, V = svd_r(F)
    order = sorted(range(3), key=lambda i: -S[i])
    if not S[order[1]] > mpf(1e-6) * S[order[0]]:
        return None
    E = matrix(3, 3)
    for i in order[:2]:
        E += U[:, i] * V[i, :]
    flat = [E[r, k] for r in range(3) for k in range(3)]
    lead = max(range(9), key=lambda k: abs(flat[k]))
    return E * (-1 if flat[lead] < 0 else 1)


def _candidates(E):
    U, S, V = svd_r(E)
    order = sorted(range(3), key=lambda i: -S[i])
    U = matrix([[U[r, i] for i in order] for r in range(3)])
    V = matrix([[V[i, k] for k in range(3)] for i in order])   # rows v_i^T
    if _det3(U) < 0:
        U[:, 2] = -U[:, 2]
    if _det3(V) < 0:
        V[2, :] = -V[2, :]
    t = [U[r, 2] for r in range(3)]
    return [(R, [sg * x for x in t]) for R in (U * W * V, U * W.T * V) for sg in (1, -1)]


def _in_front(R, t, a, b):
    p = [R[r, 0] * a[0] + R[r, 1] * a[1] + R[r, 2] for r in range(3)]
    q = [b[0], b[1], mpf(1)]
    M = matrix([[sum(x * x for x in p), -sum(x * y for x, y in zip(p, q))], [-sum(x * y for x, y in zip(p, q)), sum(x * x for x in q)]])
    rhs = matrix([-sum(x * y for x, y in zip(p, t)), sum(x * y for x, y in zip(q, t))])
    z = M ** -1 * rhs
    return z[0] > 0 and z[1] > 0


def _sampson(E, a, b):
    l = [E[r, 0] * a[0] + E[r, 1] * a[1] + E[r, 2] for r in range(3)]
    mm = [E[0, k] * b[0] + E[1, k] * b[1] + E[2, k] for k in range(2)]
    r = b[0] * l[0] + b[1] * l[1] + l[2]
    return r * r / (l[0] ** 2 + l[1] ** 2 + mm[0] ** 2 + mm[1] ** 2)


# ---- the fp64 restatement that kappa is differentiated through ----
def _np_hartley(p):
    c = p.mean(axis=0)
    s = np.mean(np.hypot(p[:, 0] - c[0], p[:, 1] - c[1])) / np.sqrt(2.0)
    return (p - c) / s, np.array([[1 / s, 0, -c[0] / s], [0, 1 / s, -c[1] / s], [0, 0, 1]])


def _np_log(R):
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn, cs = 0.5 * np.linalg.norm(ax), 0.5 * (np.trace(R) - 1.0)
    return 0.5 * ax if sn < 1e-8 else ax * (np.arctan2(sn, cs) / (2.0 * sn))


def _np_map(x, m, E_ref, pose_ref):
    pa, pb = x[:2 * m].reshape(m, 2), x[2 * m:].reshape(m, 2)
    (ha, Ta), (hb, Tb) = _np_hartley(pa), _np_hartley(pb)
    A = np.stack([hb[:, 0] * ha[:, 0], hb[:, 0] * ha[:, 1], hb[:, 0], hb[:, 1] * ha[:, 0], hb[:, 1] * ha[:, 1], hb[:, 1], ha[:, 0], ha[:, 1], np.ones(m)], axis=1)
    F = Tb.T @ np.linalg.svd(A, full_matrices=True)[2][-1].reshape(3, 3) @ Ta
    U, _, Vt = np.linalg.svd(F)
    E = U @ np.diag([1.0, 1.0, 0.0]) @ Vt
    if np.sum(E.reshape(-1) * E_ref) < 0:
        E = -E
    U, _, Vt = np.linalg.svd(E)
    U[:, 2] *= np.sign(np.linalg.det(U)); Vt[2] *= np.sign(np.linalg.det(Vt))
    Wn = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    best = None
    for R in (U @ Wn @ Vt, U @ Wn.T @ Vt):
        for sg in (1.0, -1.0):
            pose = np.concatenate([_np_log(R), -R.T @ (sg * U[:, 2])])
            if best is None or np.linalg.norm(pose - pose_ref) < np.linalg.norm(best - pose_ref):
                best = pose
    return np.concatenate([E.reshape(-1), best])


def solve_one(cam_a, cam_b, xy_a, xy_b, idx, want_kappa=True, normalised=None):
    """One subset.  xy_a, xy_b [n,2] float32, idx its m indices.  normalised: ((xa, ya), (xb, yb)) per correspondence, where already known."""
    out = dict(status=0, E=None, pose=None, unit_E=None, unit_pose=None, kappa_max=None, leave_out=False, gap=None)
    idx = [int(i) for i in idx]
    if len(idx) < 8 or len(set(idx)) < len(idx):
        return out
    n = len(xy_a)
    nrm = normalised or [(normalise(cam_a, xy_a[i, 0], xy_a[i, 1]), normalise(cam_b, xy_b[i, 0], xy_b[i, 1])) for i in range(n)]
    _essential.gap = None
    E = _essential([nrm[i][0] for i in idx], [nrm[i][1] for i in idx])
    out["gap"] = _essential.gap
    if E is None:
        return out
    f = (mpf(float(cam_a[0])) + mpf(float(cam_a[1])) + mpf(float(cam_b[0])) + mpf(float(cam_b[1]))) / 4
    inliers = [i for i in range(n) if _sampson(E, *nrm[i]) * f * f <= mpf(THRESHOLD_PX) ** 2]
    cands = _candidates(E)
    counts = [sum(1 for i in inliers if _in_front(R, t, *nrm[i])) for R, t in cands]
    R, t = cands[max(range(4), key=lambda c: (counts[c], -c))]
    pose = _pose_from_rt(R, t)
    out.update(status=1, E=[float(E[r, k]) for r in range(3) for k in range(3)], pose=[float(p) for p in pose])
    if want_kappa:
        m = len(idx)
        x0 = np.array([float(v) for i in idx for v in nrm[i][0]] + [float(v) for i in idx for v in nrm[i][1]])
        E_ref, pose_ref = np.array(out["E"]), np.array(out["pose"])
        kappa = np.zeros(15)
        for j in range(4 * m):
            h = 1e-6 * max(abs(x0[j]), 1.0)
            xp, xm = x0.copy(), x0.copy(); xp[j] += h; xm[j] -= h
            kappa += np.abs((_np_map(xp, m, E_ref, pose_ref) - _np_map(xm, m, E_ref, pose_ref)) / (2 * h)) * abs(x0[j])
        out["unit_E"] = list((kappa[:9] + np.abs(E_ref)) * EPS)
        out["unit_pose"] = list((kappa[9:] + np.abs(pose_ref)) * EPS)
        out["kappa_max"] = float(kappa.max())
        out["leave_out"] = bool(out["kappa_max"] > 1e6)
    return out


# ---------------------------------------------------------------- the shared cases ----------------------------------------------------------------
MAIN_SEEDS = {"main_pinhole": 3, "main_distorted": 4}
NOISY_CASES = ("overdetermined_noisy",)   # their solution is not the generating pose
RANDOM_CASES = tuple(MAIN_SEEDS)
POSE_B = np.array([0.05, -0.12, 0.04, 0.9, 0.1, 0.42])


def _unit_centre(pose):
    pose = np.array(pose, dtype=np.float64)
    if np.linalg.norm(pose[3:]) > 0:
        pose[3:] /= np.linalg.norm(pose[3:])
    return pose


def _scene(cam, pose_b, X, subsets, m=8):
    """camera A at the origin, camera B at pose_b (unit baseline); noise-free projections rounded to float"""
    pose_b = _unit_centre(pose_b)
    X = np.asarray(X, dtype=np.float64)
    return dict(cam_a=cam, cam_b=cam, xy_a=project(cam, np.zeros(6), X).astype(np.float32), xy_b=project(cam, pose_b, X).astype(np.float32),
                subsets=np.asarray(subsets, dtype=np.int32).reshape(-1, m), pose=pose_b)


def _cloud(rng, n):
    return np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(5, 11, n)], axis=1)


def _main_scene(cam, seed):
    """24 points between 5 and 11 m in front of camera A; 65 random eight-point subsets"""
    rng = np.random.default_rng(seed)
    X = _cloud(rng, 24)
    return _scene(cam, POSE_B, X, [rng.choice(24, 8, replace=False) for _ in range(65)])


def _sideways_scene():
    """no rotation and EXACT data (integer camera-frame points at depths 3 * 2^k through fx = fy = 768, the baseline one unit along x): the
    recovered rotation is the identity to rounding and pose_from_rt takes its small-angle branch"""
    rng = np.random.default_rng(17)
    pts = set()
    while len(pts) < 12:
        z = int(rng.choice([3, 6, 12, 24]))
        pts.add((int(rng.integers(-z // 2, z // 2 + 1)), int(rng.integers(-z // 3, z // 3 + 1)), z))
    X = np.array(sorted(pts), dtype=np.float64)
    sc = _scene(CAM_EXACT, np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0]), X, [rng.choice(12, 8, replace=False) for _ in range(5)])
    assert np.array_equal(project(CAM_EXACT, sc["pose"], X), sc["xy_b"].astype(np.float64)) and np.array_equal(project(CAM_EXACT, np.zeros(6), X), sc["xy_a"].astype(np.float64))
    return sc


def _forward_scene():
    """camera B one unit ahead of A, almost along the optical axis: the epipole lies inside the image"""
    rng = np.random.default_rng(23)
    return _scene(CAM_PLAIN, np.array([0.02, 0.03, -0.01, 0.05, -0.03, 1.0]), _cloud(rng, 24), [rng.choice(24, 8, replace=False) for _ in range(6)])


def _degenerate_scene():
    """0..23 the distorted main scene; 24..31 eight points of one scene plane; 32..39 eight points seen by a camera B that only turned (no
    baseline); 40..47 one correspondence eight times"""
    base = _main_scene(CAM_DIST, MAIN_SEEDS["main_distorted"])
    rng = np.random.default_rng(31)
    P = _cloud(rng, 8); P[:, 2] = 7.0 + 0.3 * P[:, 0] - 0.2 * P[:, 1]
    Q = _cloud(rng, 8)
    plane = _scene(CAM_DIST, POSE_B, P, np.arange(8))
    turned = dict(xy_a=project(CAM_DIST, np.zeros(6), Q).astype(np.float32), xy_b=project(CAM_DIST, np.array([*POSE_B[:3], 0, 0, 0]), Q).astype(np.float32))
    same = _scene(CAM_DIST, POSE_B, np.repeat(Q[:1], 8, axis=0), np.arange(8))
    subs = [[0, 1, 2, 3, 4, 5, 6, 0], list(range(24, 32)), list(range(32, 40)), list(range(40, 48)), list(range(8))]
    return dict(base, xy_a=np.concatenate([base["xy_a"], plane["xy_a"], turned["xy_a"], same["xy_a"]]),
                xy_b=np.concatenate([base["xy_b"], plane["xy_b"], turned["xy_b"], same["xy_b"]]), subsets=np.array(subs, dtype=np.int32))


def cases():
    """name -> dict(cam_a, cam_b, xy_a [n,2] float32, xy_b [n,2] float32, subsets [T,m] int32, pose: the generating pose of B, unit baseline)"""
    out = {}
    out["main_pinhole"] = _main_scene(CAM_PLAIN, MAIN_SEEDS["main_pinhole"])       # 65 subsets: one full wave and one lane
    out["main_distorted"] = _main_scene(CAM_DIST, MAIN_SEEDS["main_distorted"])
    base = out["main_distorted"]
    out["single"] = dict(base, xy_a=base["xy_a"][:8], xy_b=base["xy_b"][:8], subsets=np.arange(8, dtype=np.int32)[None, :])   # n = 8, one task
    out["overdetermined"] = dict(base, subsets=np.array([np.arange(24), np.random.default_rng(2).permutation(24)], dtype=np.int32))   # m = 24
    noisy = base["xy_b"].astype(np.float64) + np.random.default_rng(6).normal(0.0, 0.1, base["xy_b"].shape)   # 0.1 px of noise: no exact null vector, so the fit depends on the normalisation
    out["overdetermined_noisy"] = dict(base, xy_b=noisy.astype(np.float32), subsets=np.arange(24, dtype=np.int32)[None, :])
    out["sideways_no_rotation"] = _sideways_scene()
    out["forward_motion"] = _forward_scene()
    out["degenerate"] = _degenerate_scene()
    return out


_REFERENCE = {}


def reference(name):
    """the extended-precision results of one case, computed once per process"""
    if name not in _REFERENCE:
        c = cases()[name]
        nrm = [(normalise(c["cam_a"], c["xy_a"][i, 0], c["xy_a"][i, 1]), normalise(c["cam_b"], c["xy_b"][i, 0], c["xy_b"][i, 1])) for i in range(len(c["xy_a"]))]
        _REFERENCE[name] = [solve_one(c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"], s, normalised=nrm) for s in c["subsets"]]
    return _REFERENCE[name]


# ---- the outlier scenes of the RANSAC tests: frames (0, fb) of the 12-frame, 600-point scene, 40 % of frame B's observations replaced ----
OUTLIER_SCENES = ((1, False), (4, False), (1, True), (4, True))   # (frame B, rolling shutter)
RANSAC = dict(iterations=1000, threshold_px=4.0, refits=3, min_inliers=16, rng_state=0x9e3779b97f4a7c15)


def scene_name(fb, rolling):
    return f"frames_0_{fb}_{'rolling' if rolling else 'global'}"


def outlier_scene(fb, rolling):
    """-> dict(cam, xy_a, xy_b [n,2] float32, true_inlier [n] bool, R, t: camera B's first pose slot relative to A's (t a unit vector), sc)"""
    from rsba_amd.scene import make_scene
    sc = make_scene(12, 600, rolling=rolling, seed=5, noise_px=0.3, rot_noise=0.0, pos_noise=0.0, pt_noise=0.0)
    p = sc.problem
    at = lambda f: {int(j): p.obs_xy[i] for i, j in zip(np.nonzero(p.obs_frame == f)[0], p.obs_point[p.obs_frame == f])}
    a, b = at(0), at(fb)
    pts = sorted(set(a) & set(b))
    xy_a, xy_b = np.array([a[j] for j in pts]), np.array([b[j] for j in pts])
    rng = np.random.default_rng(0)   # (the draw matters: see test_two_view_reference.py on how often the loop as defined misses 0.9)
    bad = rng.random(len(pts)) < 0.4
    xy_b[bad] = np.stack([rng.uniform(0, 1280, bad.sum()), rng.uniform(0, 720, bad.sum())], axis=1)
    Ra, Rb = _rodrigues(sc.true_poses[0, 0, :3]), _rodrigues(sc.true_poses[fb, 0, :3])
    R = Rb @ Ra.T
    t = Rb @ (sc.true_poses[0, 0, 3:] - sc.true_poses[fb, 0, 3:])
    return dict(cam=p.intrinsics[0], xy_a=xy_a.astype(np.float32), xy_b=xy_b.astype(np.float32), true_inlier=~bad, R=R, t=t / np.linalg.norm(t), points=np.array(pts), sc=sc)


def distance_to_truth(pose, scene):
    """(rotation angle, angle between the baseline directions) in degrees between a pose of B in A's frame and the scene's true geometry"""
    R = _rodrigues(np.asarray(pose[:3]))
    t = -R @ np.asarray(pose[3:])
    ang = np.degrees(np.arccos(np.clip(0.5 * (np.trace(R @ scene["R"].T) - 1.0), -1.0, 1.0)))
    return float(ang), float(np.degrees(np.arccos(np.clip(np.dot(t / np.linalg.norm(t), scene["t"]), -1.0, 1.0))))


def undistort(cam, xy):
    """normalised, undistorted points [n,2] (fp64: for the triangulation check, which needs pixels, not ulps)"""
    pn = (np.asarray(xy, dtype=np.float64) - cam[7:9]) / cam[0:2]
    u = pn.copy()
    for _ in range(20):
        x, y = u[:, 0], u[:, 1]; r2 = x * x + y * y
        d = 1 + r2 * (cam[2] + r2 * (cam[3] + r2 * cam[6]))
        u = u - (np.stack([d * x + 2 * cam[4] * x * y + cam[5] * (r2 + 2 * x * x), d * y + cam[4] * (r2 + 2 * y * y) + 2 * cam[5] * x * y], axis=1) - pn)
    return u


def reprojecting_inliers(scene, pose, mask, sq_threshold=16.0):
    """how many of the flagged correspondences, triangulated from the two views (midpoint of the two rays), lie in front of both cameras and
    reproject within sq_threshold px^2 in both frames — what createTracks asks of a new track, with identical pose slots"""
    from rsba_amd.scene import project as project_pose
    cam = scene["cam"]
    R = _rodrigues(np.asarray(pose[:3])); c = np.asarray(pose[3:])
    na, nb = undistort(cam, scene["xy_a"][mask]), undistort(cam, scene["xy_b"][mask])
    da = np.concatenate([na, np.ones((len(na), 1))], axis=1); db = np.concatenate([nb, np.ones((len(nb), 1))], axis=1) @ R   # rays in A's frame
    count = 0
    for i in range(len(da)):
        A = np.stack([da[i], -db[i]], axis=1)
        z = np.linalg.lstsq(A, c, rcond=None)[0]
        X = 0.5 * (z[0] * da[i] + c + z[1] * db[i])
        pa, za = project_pose(cam, np.zeros((1, 6)), X[None]); pb, zb = project_pose(cam, np.asarray(pose, dtype=np.float64)[None], X[None])
        if za[0] > 0 and zb[0] > 0 and np.sum((pa[0] - scene["xy_a"][mask][i]) ** 2) <= sq_threshold and np.sum((pb[0] - scene["xy_b"][mask][i]) ** 2) <= sq_threshold:
            count += 1
    return count


# ------------------------------------------- the host program (tests/two_view_host.cpp), for the tests and make_two_view_bound.py -------------------------------------------
def write_case_file(path, case_list):
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(case_list)))
        for c in case_list:
            f.write(struct.pack("<3i", len(c["xy_a"]), len(c["subsets"]), c["subsets"].shape[1]))
            f.write(np.asarray(c["cam_a"], dtype="<f8").tobytes()); f.write(np.asarray(c["cam_b"], dtype="<f8").tobytes())
            f.write(c["xy_a"].astype("<f4").tobytes()); f.write(c["xy_b"].astype("<f4").tobytes()); f.write(np.asarray(c["subsets"]).astype("<i4").tobytes())


def write_scene_file(path, scene):
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(scene["xy_a"])))
        f.write(np.asarray(scene["cam"], dtype="<f8").tobytes()); f.write(np.asarray(scene["cam"], dtype="<f8").tobytes())
        f.write(scene["xy_a"].astype("<f4").tobytes()); f.write(scene["xy_b"].astype("<f4").tobytes())


def _rows(text):
    return [[float(x) for x in line.split()] for line in text.strip().split("\n")]


def _per_subset(r):
    r = np.array(r)
    return dict(status=r[:, 0].astype(int), E=r[:, 1:10], scored=r[:, 10].astype(int), num_inliers=r[:, 11].astype(int), num_front=r[:, 12:16].astype(int),
                winner=r[:, 16].astype(int), poses=r[:, 17:23], margin=r[:, 23])


def run_host(exe, directory, case_list, mode=0):
    """per case: dict(status [T], E [T,9], scored, num_inliers, num_front [T,4], winner, poses [T,6], margin) of the C++ host definitions"""
    import os
    import subprocess
    path = os.path.join(str(directory), "cases.bin")
    write_case_file(path, case_list)
    rows = _rows(subprocess.run([exe, path, str(mode), str(THRESHOLD_PX)], check=True, capture_output=True, text=True).stdout)
    out, k = [], 0
    for c in case_list:
        out.append(_per_subset(rows[k:k + len(c["subsets"])])); k += len(c["subsets"])
    return out


def run_host_hypotheses(exe, directory, scene, T, name="scene"):
    import os
    import subprocess
    path = os.path.join(str(directory), name + ".bin")
    write_scene_file(path, scene)
    return _per_subset(_rows(subprocess.run([exe, "hypotheses", path, str(T), str(RANSAC["threshold_px"]), str(RANSAC["rng_state"])], check=True, capture_output=True, text=True).stdout))


def run_host_ransac(exe, directory, scene, name="scene"):
    """the whole host loop -> dict(ok, winner_task, num_inliers, num_front, refits_adopted, E, pose, mask [n] bool, ratio [n]: d^2 f^2 / thr^2)"""
    import os
    import subprocess
    path = os.path.join(str(directory), name + ".bin")
    write_scene_file(path, scene)
    o = RANSAC
    rows = _rows(subprocess.run([exe, "ransac", path, str(o["iterations"]), str(o["threshold_px"]), str(o["refits"]), str(o["min_inliers"]), str(o["rng_state"])],
                                check=True, capture_output=True, text=True).stdout)
    head = [int(v) for v in rows[0]]
    return dict(ok=bool(head[0]), winner_task=head[1], num_inliers=head[2], num_front=head[3], refits_adopted=head[4], E=np.array(rows[1]), pose=np.array(rows[2]),
                mask=np.array(rows[3]).astype(bool), ratio=np.array(rows[4]))


def worst_error(ref, status, E, poses):
    """worst |value_k - reference_k| / unit_k over E (up to sign) and the pose, over the subsets both accept and the reference does not leave out"""
    worst = 0.0
    for t, r in enumerate(ref):
        if r["status"] and status[t] and not r["leave_out"]:
            e = np.array(r["E"])
            sign = 1.0 if np.dot(E[t], e) >= 0 else -1.0
            worst = max(worst, float(np.max(np.abs(sign * E[t] - e) / np.array(r["unit_E"]))), float(np.max(np.abs(poses[t] - np.array(r["pose"])) / np.array(r["unit_pose"]))))
    return worst
