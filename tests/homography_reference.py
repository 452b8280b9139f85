"""Extended-precision reference of the two-view degeneracy test (include/rsba_amd.h: rsba_homography_dlt / rsba_homography_score and the
parallax rule; host form homo_detail::dlt / score / parallax_counts in include/rsba/pair_geometry.hpp), in mpmath at 60 digits, and the fixed
case list the host test (test_homography_reference.py) and the device tests (test_gpu_homography.py, test_gpu_classify_pairs.py) share.  It
shares no code with the C++ and reaches the null vector another way: the last right singular vector of mpmath's SVD of the 2m x 9
constraint matrix itself (no Gram matrix, no Jacobi); the inverse is mpmath's, the rotation of the parallax rule Rodrigues' formula.

solve_one(...) returns per subset
  status     0 declined, 1 solved
  H          the homography (row-major, b ~ H a, unit Frobenius norm, (H a)_z > 0 for the first index), floats; None when declined
  unit_H     the error unit per component, (kappa_k + |value_k|) 2^-52, kappa_k = sum_j |d value_k / d x_j| |x_j| over the 4 m normalised image
             coordinates of the subset: central differences (h = 1e-6) of an fp64 numpy restatement of the same map (numpy's SVD)
  gap        second-smallest eigenvalue of the Gram matrix over the value the gap test compares it with (declined below 1; None: declined earlier)
  why        what declined it: "repeated", "scale", "gap", "orientation", "det"
  kappa_max, leave_out   the subset may be left out of the ACCURACY check (never of the status check): kappa_max > 1e6
"""
import os
import struct
import subprocess

import numpy as np
from mpmath import mp, mpf, matrix, sqrt, svd_r

import two_view_reference as R
from p3p_reference import CAM_DIST, CAM_PLAIN, _rotate, normalise, project

assert mp.dps >= 50   # (60: what two_view_reference and p3p_reference set on import; one precision for every reference in a test process)
EPS = 2.0 ** -52
THRESHOLD_PX = 4.0
RNG_STATE = R.RANSAC["rng_state"]


def _homography(pa, pb):
    """the DLT matrix of the normalised points pa, pb (lists of mp pairs) as a flat list of 9; None: declined (_homography.why says by what)"""
    m = len(pa)
    ax, ay, sa = R._hartley(pa)
    bx, by, sb = R._hartley(pb)
    _homography.gap = None
    _homography.why = "scale"
    if not sa > 0 or not sb > 0:
        return None
    rows = []
    for (xa, ya), (xb, yb) in zip(pa, pb):
        xa, ya, xb, yb = (xa - ax) / sa, (ya - ay) / sa, (xb - bx) / sb, (yb - by) / sb
        rows.append([-xa, -ya, mpf(-1), 0, 0, 0, xb * xa, xb * ya, xb])
        rows.append([0, 0, 0, -xa, -ya, mpf(-1), yb * xa, yb * ya, yb])
    rows += [[mpf(0)] * 9] * max(0, 9 - 2 * m)
    _, S, V = svd_r(matrix(rows))
    sv = sorted(((S[i], i) for i in range(9)), key=lambda p: -p[0])
    trace = sum(s * s for s, _ in sv)
    _homography.gap = float(sv[7][0] ** 2 / (mpf(1e-9) * 2 * trace))
    _homography.why = "gap"
    if not sv[7][0] ** 2 > mpf(1e-9) * 2 * trace or not sv[8][0] ** 2 < mpf(0.05) * sv[7][0] ** 2:
        return None
    Hn = matrix(3, 3)
    for r in range(3):
        for k in range(3):
            Hn[r, k] = V[sv[8][1], 3 * r + k]
    Ta = matrix([[1 / sa, 0, -ax / sa], [0, 1 / sa, -ay / sa], [0, 0, 1]])
    Tbi = matrix([[sb, 0, bx], [0, sb, by], [0, 0, 1]])
    H = Tbi * Hn * Ta
    fro = sqrt(sum(H[r, k] ** 2 for r in range(3) for k in range(3)))
    H = H / fro
    z = [H[2, 0] * xa + H[2, 1] * ya + H[2, 2] for xa, ya in pa]
    if z[0] < 0:
        H, z = -H, [-v for v in z]
    _homography.why = "orientation"
    if not all(v > 0 for v in z):
        return None
    _homography.why = "det"
    if not abs(R._det3(H)) > mpf(1e-6):
        return None
    _homography.why = None
    return [H[r, k] for r in range(3) for k in range(3)]


def _np_map(x, m, H_ref):
    pa, pb = x[:2 * m].reshape(m, 2), x[2 * m:].reshape(m, 2)
    (ha, Ta), (hb, Tb) = R._np_hartley(pa), R._np_hartley(pb)
    A = np.zeros((2 * m, 9))
    A[0::2, 0:2] = -ha; A[0::2, 2] = -1; A[0::2, 6:8] = hb[:, :1] * ha; A[0::2, 8] = hb[:, 0]
    A[1::2, 3:5] = -ha; A[1::2, 5] = -1; A[1::2, 6:8] = hb[:, 1:] * ha; A[1::2, 8] = hb[:, 1]
    H = np.linalg.inv(Tb) @ np.linalg.svd(A, full_matrices=True)[2][-1].reshape(3, 3) @ Ta
    H = H.reshape(-1) / np.linalg.norm(H)
    return -H if np.dot(H, H_ref) < 0 else H


def solve_one(cam_a, cam_b, xy_a, xy_b, idx, want_kappa=True, normalised=None):
    """One subset.  xy_a, xy_b [n,2] float32, idx its m indices.  normalised: ((xa, ya), (xb, yb)) per correspondence, where already known."""
    out = dict(status=0, H=None, unit_H=None, kappa_max=None, leave_out=False, gap=None, why="repeated")
    idx = [int(i) for i in idx]
    if len(idx) < 4 or len(set(idx)) < len(idx):
        return out
    nrm = normalised or [(normalise(cam_a, xy_a[i, 0], xy_a[i, 1]), normalise(cam_b, xy_b[i, 0], xy_b[i, 1])) for i in range(len(xy_a))]
    H = _homography([nrm[i][0] for i in idx], [nrm[i][1] for i in idx])
    out["gap"], out["why"] = _homography.gap, _homography.why
    if H is None:
        return out
    out.update(status=1, H=[float(v) for v in H])
    if want_kappa:
        m = len(idx)
        x0 = np.array([float(v) for i in idx for v in nrm[i][0]] + [float(v) for i in idx for v in nrm[i][1]])
        H_ref = np.array(out["H"])
        kappa = np.zeros(9)
        for j in range(4 * m):
            h = 1e-6 * max(abs(x0[j]), 1.0)
            xp, xm = x0.copy(), x0.copy(); xp[j] += h; xm[j] -= h
            kappa += np.abs((_np_map(xp, m, H_ref) - _np_map(xm, m, H_ref)) / (2 * h)) * abs(x0[j])
        out["unit_H"] = list((kappa + np.abs(H_ref)) * EPS)
        out["kappa_max"] = float(kappa.max())
        out["leave_out"] = bool(out["kappa_max"] > 1e6)
    return out


def normalised_points(cam_a, cam_b, xy_a, xy_b):
    return [(normalise(cam_a, xy_a[i, 0], xy_a[i, 1]), normalise(cam_b, xy_b[i, 0], xy_b[i, 1])) for i in range(len(xy_a))]


def mean_focal(cam_a, cam_b):
    return (mpf(float(cam_a[0])) + mpf(float(cam_a[1])) + mpf(float(cam_b[0])) + mpf(float(cam_b[1]))) / 4


def score(H, nrm, f, threshold_px=THRESHOLD_PX):
    """the inlier rule of a given H (9 floats) in extended precision -> (status, count, flags, margin: the smallest relative distance of a
    correspondence in front both ways from the threshold, depth: the smallest |(H a)_z|, |(H^-1 b)_z|)"""
    Hm = matrix(3, 3)
    for r in range(3):
        for k in range(3):
            Hm[r, k] = mpf(float(H[3 * r + k]))
    if R._det3(Hm) == 0:
        return 0, 0, [False] * len(nrm), None, None
    Hi = Hm ** -1
    thr2 = mpf(float(threshold_px)) ** 2
    flags, margin, depth = [], None, None
    for (xa, ya), (xb, yb) in nrm:
        p = [Hm[r, 0] * xa + Hm[r, 1] * ya + Hm[r, 2] for r in range(3)]
        q = [Hi[r, 0] * xb + Hi[r, 1] * yb + Hi[r, 2] for r in range(3)]
        for w in (abs(p[2]), abs(q[2])):
            depth = w if depth is None or w < depth else depth
        if not (p[2] > 0 and q[2] > 0):
            flags.append(False)
            continue
        d2 = max((xb - p[0] / p[2]) ** 2 + (yb - p[1] / p[2]) ** 2, (xa - q[0] / q[2]) ** 2 + (ya - q[1] / q[2]) ** 2)
        rel = abs(d2 * f * f - thr2) / thr2
        margin = rel if margin is None or rel < margin else margin
        flags.append(bool(d2 * f * f <= thr2))
    return 1, sum(flags), flags, None if margin is None else float(margin), float(depth)


def parallax_counts(E, pose, nrm, f, cos_min, threshold_px=THRESHOLD_PX):
    """-> (num_front, num_parallax, margin: the smallest distance of a deciding comparison from changing sides, in the units of
    homography_host parallax)"""
    Em = matrix(3, 3)
    for r in range(3):
        for k in range(3):
            Em[r, k] = mpf(float(E[3 * r + k]))
    w, c = [mpf(float(v)) for v in pose[:3]], [mpf(float(v)) for v in pose[3:]]
    cols = [_rotate(w, [mpf(int(k == j)) for j in range(3)]) for k in range(3)]
    Rm = matrix([[cols[k][r] for k in range(3)] for r in range(3)])
    t = [-v for v in _rotate(w, c)]
    thr2, cm = mpf(float(threshold_px)) ** 2, mpf(float(cos_min))
    front = par = 0
    margin = None
    for a, b in nrm:
        d2 = R._sampson(Em, a, b) * f * f
        ms = [abs(d2 - thr2) / thr2]
        if d2 <= thr2:
            p = [Rm[r, 0] * a[0] + Rm[r, 1] * a[1] + Rm[r, 2] for r in range(3)]
            q = [b[0], b[1], mpf(1)]
            M = matrix([[sum(x * x for x in p), -sum(x * y for x, y in zip(p, q))], [-sum(x * y for x, y in zip(p, q)), sum(x * x for x in q)]])
            z = M ** -1 * matrix([-sum(x * y for x, y in zip(p, t)), sum(x * y for x, y in zip(q, t))])
            ms += [abs(z[0]), abs(z[1])]
            if z[0] > 0 and z[1] > 0:
                front += 1
                rb = [Rm[0, k] * b[0] + Rm[1, k] * b[1] + Rm[2, k] for k in range(3)]
                cosang = (a[0] * rb[0] + a[1] * rb[1] + rb[2]) / sqrt((a[0] ** 2 + a[1] ** 2 + 1) * sum(x * x for x in rb))
                ms.append(abs(cm - cosang))
                par += 1 if cosang <= cm else 0
        margin = min(ms) if margin is None else min(margin, *ms)
    return front, par, float(margin)


# ---------------------------------------------------------------- the shared cases ----------------------------------------------------------------
NOISY_CASES = ("refit_24_noisy", "refit_100_noisy")
DECLINED = ("repeated", "gap", "scale", "orientation", "det")   # the reason each subset of the "declined" case is declined for, in order


def _plane_points(rng, n, wide=3.0):
    X = np.stack([rng.uniform(-wide, wide, n), rng.uniform(-2, 2, n), np.zeros(n)], axis=1)
    X[:, 2] = 7.0 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    return X


def _plane_scene(cam, seed, n=24, T=65):
    """n points of one scene plane; T random four-point subsets"""
    rng = np.random.default_rng(seed)
    return R._scene(cam, R.POSE_B, _plane_points(rng, n), [rng.choice(n, 4, replace=False) for _ in range(T)], m=4)


def _rotation_scene():
    """a general cloud seen by a camera B that only turned: H = R, which the eight-point rule declines and the DLT must accept"""
    rng = np.random.default_rng(11)
    return R._scene(CAM_DIST, np.array([*R.POSE_B[:3], 0.0, 0.0, 0.0]), R._cloud(rng, 24), [rng.choice(24, 4, replace=False) for _ in range(8)], m=4)


def _refit_scene(n, noise, seed):
    rng = np.random.default_rng(seed)
    sc = R._scene(CAM_DIST, R.POSE_B, _plane_points(rng, n), [np.arange(n), rng.permutation(n)], m=n)
    if noise:
        sc["xy_b"] = (sc["xy_b"].astype(np.float64) + rng.normal(0.0, noise, sc["xy_b"].shape)).astype(np.float32)
    return sc


def _declined_scene():
    """0..23 the pinhole plane scene.  24..27 three points of one scene line and a fourth; 28..31 one correspondence four times; 32..35 a
    square whose image has two neighbouring corners exchanged (the homography exists and sends part of the square behind the camera);
    36..39 general points whose images are the same figure shrunk to 5e-4 of its size (a fraction of a pixel across): H = diag(s, s, 1),
    |det H| = s^2 at unit norm, which Hartley's normalisation fits without trouble and the determinant test declines"""
    cam = CAM_PLAIN
    base = _plane_scene(cam, 3)
    P = _plane_points(np.random.default_rng(31), 4)
    P[2, :2] = 0.5 * (P[0, :2] + P[1, :2]); P[2, 2] = 7.0 + 0.3 * P[2, 0] - 0.2 * P[2, 1]
    line = R._scene(cam, R.POSE_B, P, np.arange(4), m=4)
    same = R._scene(cam, R.POSE_B, np.repeat(P[:1], 4, axis=0), np.arange(4), m=4)
    px = lambda pts: (np.array(pts, dtype=np.float64) * cam[0] + cam[7:9]).astype(np.float32)
    square = [[-0.2, -0.2], [0.2, -0.2], [0.2, 0.2], [-0.2, 0.2]]
    twisted = [[-0.2, -0.2], [0.2, -0.2], [-0.2, 0.2], [0.2, 0.2]]
    general = np.array([[-0.3, -0.1], [0.25, -0.2], [0.1, 0.3], [-0.15, 0.2]])
    subs = [[0, 1, 2, 0], [24, 25, 26, 27], [28, 29, 30, 31], [32, 33, 34, 35], [36, 37, 38, 39]]
    return dict(base, xy_a=np.concatenate([base["xy_a"], line["xy_a"], same["xy_a"], px(square), px(general)]),
                xy_b=np.concatenate([base["xy_b"], line["xy_b"], same["xy_b"], px(twisted), px(5e-4 * general)]), subsets=np.array(subs, dtype=np.int32))


def cases():
    """name -> dict(cam_a, cam_b, xy_a [n,2] float32, xy_b [n,2] float32, subsets [T,m] int32)"""
    out = {}
    out["plane_pinhole"] = _plane_scene(CAM_PLAIN, 3)       # 65 subsets: one full wave and one lane
    out["plane_distorted"] = _plane_scene(CAM_DIST, 4)
    out["pure_rotation"] = _rotation_scene()
    out["refit_24_exact"] = _refit_scene(24, 0.0, 5)
    out["refit_24_noisy"] = _refit_scene(24, 0.5, 6)
    out["refit_100_exact"] = _refit_scene(100, 0.0, 7)
    out["refit_100_noisy"] = _refit_scene(100, 0.5, 8)
    out["declined"] = _declined_scene()
    return out


_REFERENCE = {}


def reference(name):
    """the extended-precision results of one case, computed once per process"""
    if name not in _REFERENCE:
        c = cases()[name]
        nrm = normalised_points(c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"])
        _REFERENCE[name] = [solve_one(c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"], s, normalised=nrm) for s in c["subsets"]]
    return _REFERENCE[name]


# ---- the scoring scene: the plane with 200 correspondences (three full waves and a tail of 8), 25 % gross outliers, 0.5 px of noise ----
SCORING = dict(n=200, T=64, seed=21, iterations=64, refits=3)


def _outlier_scene(cam, X, pose, rng, share, noise):
    xy_a, xy_b = project(cam, np.zeros(6), X), project(cam, pose, X) + rng.normal(0.0, noise, (len(X), 2))
    bad = np.zeros(len(X), dtype=bool)
    bad[rng.choice(len(X), int(round(share * len(X))), replace=False)] = True   # exactly that share
    xy_b[bad] = np.stack([rng.uniform(0, 1280, bad.sum()), rng.uniform(0, 720, bad.sum())], axis=1)
    return dict(cam=cam, cam_a=cam, cam_b=cam, xy_a=xy_a.astype(np.float32), xy_b=xy_b.astype(np.float32), true_inlier=~bad)


def scoring_scene(planar=True, seed=None):
    rng = np.random.default_rng(SCORING["seed"] if seed is None else seed)
    X = _plane_points(rng, SCORING["n"]) if planar else R._cloud(rng, SCORING["n"])
    return _outlier_scene(CAM_DIST, X, R._unit_centre(R.POSE_B), rng, 0.25, 0.5)


# ---- the classification pairs: one cloud of 200 points, 20 % outliers and 0.5 px of noise per pair, only what both 1280 x 720 images see ----
CLASSIFY = dict(iterations=200, threshold_px=4.0, refits=3, min_inliers=16, rng_state=RNG_STATE, min_parallax_deg=2.0, solver=5)   # five-point subsets: the eight-point rule has no stable E for the plane of pair (c)
CLOUD_SEED, MEAN_DEPTH = 51, 8.0
PAIR_SEEDS = (59, 1037, 58, 53, 56)   # the draws of noise and outliers; (b)'s is one of those that leave (b) more inliers in front than (a) has
ROTATION = np.array([0.02, 0.1, -0.03])
DIRECTION = np.array([1.0, 0.05, 0.1]) / np.linalg.norm([1.0, 0.05, 0.1])
PAIR_NAMES = ("a_wide_general", "b_narrow_general", "c_wide_plane", "d_wide_general", "e_pure_rotation")


def _visible_pair(cam, X, pose, rng, name):
    s = _outlier_scene(cam, X, pose, rng, 0.2, 0.5)
    clean_b = project(cam, pose, X)
    inside = lambda xy: (xy[:, 0] >= 0) & (xy[:, 0] < 1280) & (xy[:, 1] >= 0) & (xy[:, 1] < 720)
    keep = inside(s["xy_a"]) & inside(clean_b)
    return dict(cam_a=np.asarray(cam, dtype=np.float64), cam_b=np.asarray(cam, dtype=np.float64), xy_a=np.ascontiguousarray(s["xy_a"][keep]),
                xy_b=np.ascontiguousarray(s["xy_b"][keep]), name=name)


def classification_pairs():
    """(a) baseline 0.3 of the mean depth, the cloud; (b) the same rotation, baseline 0.01 of the mean depth, the cloud; (c) (a)'s motion, the
    cloud's (x, y) on a plane; (d) (a)'s motion, the cloud, another draw of noise and outliers; (e) an exact pure rotation"""
    rng = np.random.default_rng(CLOUD_SEED)
    X = np.stack([rng.uniform(-5, 5, 200), rng.uniform(-2.5, 2.5, 200), rng.uniform(5, 11, 200)], axis=1)
    plane = X.copy(); plane[:, 2] = MEAN_DEPTH + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    wide, narrow = np.concatenate([ROTATION, 0.3 * MEAN_DEPTH * DIRECTION]), np.concatenate([ROTATION, 0.01 * MEAN_DEPTH * DIRECTION])
    turned = np.concatenate([ROTATION, np.zeros(3)])
    draws = [np.random.default_rng(k) for k in PAIR_SEEDS]
    return [_visible_pair(CAM_DIST, X, wide, draws[0], PAIR_NAMES[0]), _visible_pair(CAM_DIST, X, narrow, draws[1], PAIR_NAMES[1]),
            _visible_pair(CAM_DIST, plane, wide, draws[2], PAIR_NAMES[2]), _visible_pair(CAM_DIST, X, wide, draws[3], PAIR_NAMES[3]),
            _visible_pair(CAM_DIST, X, turned, draws[4], PAIR_NAMES[4])]


# ------------------------------------------- the host program (tests/homography_host.cpp), for the tests and make_homography_bound.py -------------------------------------------
def write_pairs_file(path, pairs, E=None, poses=None, status=None):
    """the file homography_host parallax / classify and examples/classify_pairs read"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(pairs)))
        for k, p in enumerate(pairs):
            f.write(struct.pack("<ii", len(p["xy_a"]), 1 if status is None else int(status[k])))
            f.write(np.asarray(p["cam_a"], dtype="<f8").tobytes()); f.write(np.asarray(p["cam_b"], dtype="<f8").tobytes())
            f.write(np.asarray(np.zeros(9) if E is None else E[k], dtype="<f8").tobytes()); f.write(np.asarray(np.zeros(6) if poses is None else poses[k], dtype="<f8").tobytes())
            f.write(p["xy_a"].astype("<f4").tobytes()); f.write(p["xy_b"].astype("<f4").tobytes())


def _run(args):
    return subprocess.run([str(a) for a in args], check=True, capture_output=True, text=True).stdout


def run_host(exe, directory, case_list):
    """per case: dict(status [T], H [T,9]) of the C++ host definitions"""
    path = os.path.join(str(directory), "homography_cases.bin")
    R.write_case_file(path, case_list)
    rows = np.array(R._rows(_run([exe, path])))
    out, k = [], 0
    for c in case_list:
        r = rows[k:k + len(c["subsets"])]; k += len(c["subsets"])
        out.append(dict(status=r[:, 0].astype(int), H=r[:, 1:10]))
    return out


def run_host_hypotheses(exe, directory, scene, T, name="scoring"):
    path = os.path.join(str(directory), name + ".bin")
    R.write_scene_file(path, scene)
    r = np.array(R._rows(_run([exe, "hypotheses", path, T, THRESHOLD_PX, RNG_STATE])))
    return dict(status=r[:, 0].astype(int), H=r[:, 1:10], num_inliers=r[:, 10].astype(int), margin=r[:, 11], depth=r[:, 12])


def run_host_ransac(exe, directory, scene, iterations, refits, name="scoring"):
    path = os.path.join(str(directory), name + ".bin")
    R.write_scene_file(path, scene)
    lines = _run([exe, "ransac", path, iterations, THRESHOLD_PX, refits, RNG_STATE]).split("\n")
    head = [int(v) for v in lines[0].split()]
    return dict(ok=bool(head[0]), winner_task=head[1], num_inliers=head[2], refits_adopted=head[3], H=np.array([float(v) for v in lines[1].split()]),
                mask=np.array([int(v) for v in lines[2].split()], dtype=bool), fitted_to=np.array([int(v) for v in lines[3].split()], dtype=np.int32))


def run_host_subsets(exe, n, T):
    return np.array([[int(x) for x in line.split()] for line in _run([exe, "subsets", n, 4, T, RNG_STATE]).strip().split("\n")], dtype=np.int32)


def run_host_parallax(exe, directory, pairs, E, poses, status, cos_min, threshold_px=THRESHOLD_PX, name="parallax"):
    path = os.path.join(str(directory), name + ".bin")
    write_pairs_file(path, pairs, E, poses, status)
    r = np.array(R._rows(_run([exe, "parallax", path, threshold_px, repr(float(cos_min))])))
    return dict(num_front=r[:, 0].astype(int), num_parallax=r[:, 1].astype(int), margin=r[:, 2])


def run_host_classify(exe, directory, pairs, options=None, name="classify"):
    o = options or CLASSIFY
    path = os.path.join(str(directory), name + ".bin")
    write_pairs_file(path, pairs)
    lines = _run([exe, "classify", path, o["iterations"], o["threshold_px"], o["refits"], o["min_inliers"], o["rng_state"], o["min_parallax_deg"], o.get("solver", 8)]).strip().split("\n")
    keys = ("ok", "winner_task", "num_inliers", "essential_front", "kind", "h_ok", "h_winner_task", "h_refits_adopted", "num_h_inliers", "num_front", "num_parallax")
    rows = [{k: (v if k == "kind" else int(v)) for k, v in zip(keys, line.split())} for line in lines[:len(pairs)]]
    pick = [int(v) for v in lines[len(pairs)].split()[1:]]
    return rows, pick


def worst_error(ref, status, H):
    """worst |value_k - reference_k| / unit_k over H, over the subsets both accept and the reference does not leave out"""
    worst = 0.0
    for t, r in enumerate(ref):
        if r["status"] and status[t] and not r["leave_out"]:
            worst = max(worst, float(np.max(np.abs(H[t] - np.array(r["H"])) / np.array(r["unit_H"]))))
    return worst


# ---- the session of the classifyMatches tests: 5 frames over the classification cloud, every later frame matched into frame 0 ----
SESSION_BASELINES = (0.01, 0.015, 0.02, 0.3)   # of the mean depth, frames 1..4: three neighbours without a baseline to speak of, one wide pair
SESSION_SEED = 111   # a draw after which the pair without a baseline (frames 0, 1) has clearly the most inliers in front


def classify_session(seed=SESSION_SEED):
    """-> dict(cam, poses [5][6], frames: per frame a list of dict(x, y, matches [(frame, obs)])).  Frame 0 sees the cloud as it is; frame k
    sees it from ROTATION and its baseline with 0.5 px of noise, and matches each observation to frame 0's observation of the same point —
    every fifth to another point's, a gross outlier"""
    rng = np.random.default_rng(CLOUD_SEED)
    X = np.stack([rng.uniform(-5, 5, 200), rng.uniform(-2.5, 2.5, 200), rng.uniform(5, 11, 200)], axis=1)
    rng = np.random.default_rng(seed)
    cam = np.asarray(CAM_DIST, dtype=np.float64)
    inside = lambda xy: (xy[:, 0] >= 0) & (xy[:, 0] < 1280) & (xy[:, 1] >= 0) & (xy[:, 1] < 720)
    poses = [np.zeros(6)] + [np.concatenate([ROTATION, b * MEAN_DEPTH * DIRECTION]) for b in SESSION_BASELINES]
    xy0 = project(cam, poses[0], X)
    seen0 = np.flatnonzero(inside(xy0))
    where0 = {int(j): k for k, j in enumerate(seen0)}
    frames = [[dict(x=float(xy0[j, 0]), y=float(xy0[j, 1]), matches=[]) for j in seen0]]
    for pose in poses[1:]:
        clean = project(cam, pose, X)
        xy = clean + rng.normal(0.0, 0.5, clean.shape)
        frame, count = [], 0
        for j in np.flatnonzero(inside(clean)):
            o = dict(x=float(xy[j, 0]), y=float(xy[j, 1]), matches=[])
            if int(j) in where0:
                count += 1
                right = where0[int(j)]
                o["matches"].append((0, (right + 11) % len(seen0) if count % 5 == 0 else right))
            frame.append(o)
        frames.append(frame)
    return dict(cam=cam, poses=[p.tolist() for p in poses], frames=frames)


def session_cache_bytes(s):
    import thrift_encode as T
    frames = [T.frame([T.observation(o["x"], o["y"], track=None, matches=[(fa, oa, True) for fa, oa in o["matches"]] or None) for o in fr], poses=[s["poses"][k]], prior_poses=None)
              for k, fr in enumerate(s["frames"])]
    return T.file_events(T.session(s["cam"], frames, [], 0, [0, 720], 1280, 720), np.random.default_rng(1), max_event=4096)


def parse_classify_output(text):
    """what examples/classify_pairs prints for a session -> (rows, [plain pick, pick with the geometry], untouched)"""
    lines = text.strip().split("\n")
    count = int(lines[0].split()[1])
    keys = ("frameA", "frameB", "correspondences", "ok", "num_inliers", "essential_front", "kind", "h_ok", "num_h_inliers", "num_front", "num_parallax")
    rows = [{k: (v if k == "kind" else int(v)) for k, v in zip(keys, line.split())} for line in lines[1:1 + count]]
    return rows, [int(v) for v in lines[1 + count].split()[1:]], bool(int(lines[2 + count].split()[1]))
