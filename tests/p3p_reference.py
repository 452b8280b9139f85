"""Extended-precision reference of the minimal solver of the global-shutter RANSAC (include/rsba_amd.h: rsba_pnp_p3p; host form
pnp_detail::p3p_pose in include/rsba/solve_rs_pnp.hpp), in mpmath at 60 digits, and the fixed case list the host test
(test_p3p_reference.py) and the device test (test_gpu_pnp_p3p.py) share.  It shares no code with the C++ and takes another way to every
number: the quartic is the resultant of the two quadratics in u = s2 / s1 that the cosine laws leave, interpolated from five samples and
solved by mpmath.polyroots in v = s3 / s1 itself (an exactly vanishing leading coefficient is stripped); u is a root of one quadratic that
satisfies the other (no division by D); collinearity is read off mpmath's singular values; the rigid motion is M_cam M_world^-1 of the
edge-edge-normal matrices, not a product of triads.

solve_one(...) returns per subset
  status         0 declined, 1 solved
  num_solutions  admissible solutions: three depths above 1e-9 |P1 P3| and the fourth point in front of the camera
  pose           rsba's 6-vector of the chosen solution, floats; None when declined
  unit           the error unit per component, (kappa_k + |pose_k|) 2^-52, kappa_k = sum_j |d pose_k / d x_j| |x_j| over the 15 inputs of
                 the three solved points (9 world coordinates, 6 normalised image coordinates), by central differences of this solution
  runner_up      the fourth-point distance of the second-best admissible solution (None: there is none)
  closest_pair   the smallest relative distance between two admissible roots v (None: fewer than two)
  leave_out      the subset may be left out of the ACCURACY check (never of the status check): runner_up < 1e-4, max kappa > 1e6 or
                 closest_pair < 1e-6
"""
import numpy as np
from mpmath import mp, mpf, matrix, sqrt, acos, sin, cos, polyroots, lu_solve, svd_r

mp.dps = 60
EPS = 2.0 ** -52


def normalise(cam, u, v):
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


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _bearing(x, y, normalised_bearing=True):
    n = sqrt(x * x + y * y + 1) if normalised_bearing else mpf(1)
    return [x / n, y / n, 1 / n]


def _rotate(w, p):
    th2 = _dot(w, w)
    wxp = _cross(w, p)
    if th2 > mpf(2.220446049250313e-16):
        th = sqrt(th2)
        k = [x / th for x in w]
        kxp = [x / th for x in wxp]
        kp = _dot(k, p) * (1 - cos(th))
        return [p[i] * cos(th) + kxp[i] * sin(th) + k[i] * kp for i in range(3)]
    return [p[i] + wxp[i] for i in range(3)]


def _pose_from_rt(R, tvec):
    """hyp_detail::pose_from_rt with its three branches, in extended precision"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cs = min(mpf(1), max(mpf(-1), (tr - 1) / 2))
    th = acos(cs)
    ax = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    sn = sqrt(_dot(ax, ax)) / 2
    if sn > mpf("1e-8"):
        rvec = [a * th / (2 * sn) for a in ax]
    elif cs > 0:
        rvec = [a / 2 for a in ax]
    else:
        d = [sqrt(max(mpf(0), (R[i, i] + 1) / 2)) for i in range(3)]
        rvec = [th * d[0], th * d[1] * (1 if R[0, 1] + R[1, 0] >= 0 else -1), th * d[2] * (1 if R[0, 2] + R[2, 0] >= 0 else -1)]
    return rvec + _rotate([-r for r in rvec], [-t for t in tvec])


def _triangle(P, J):
    a2 = _dot(_sub(P[1], P[2]), _sub(P[1], P[2])); b2 = _dot(_sub(P[0], P[2]), _sub(P[0], P[2])); c2 = _dot(_sub(P[0], P[1]), _sub(P[0], P[1]))
    return a2, b2, c2, _dot(J[1], J[2]), _dot(J[0], J[2]), _dot(J[0], J[1])


def _depth_solutions(P, J):
    """every real (s1, s2, s3, v) of the three cosine laws with v = s3 / s1 > 0 and u = s2 / s1 > 0, ascending v"""
    a2, b2, c2, ca, cb, cg = _triangle(P, J)

    def quadratics(v):   # u^2 + p1 u + p0 (sides a and b), u^2 + q1 u + q0 (sides c and b)
        w = 1 + v * v - 2 * v * cb
        return -2 * v * ca, v * v - a2 / b2 * w, -2 * cg, 1 - c2 / b2 * w

    def resultant(v):
        p1, p0, q1, q0 = quadratics(v)
        return (p0 - q0) ** 2 - p1 * (p0 - q0) * (p1 - q1) + p0 * (p1 - q1) ** 2
    xs = [mpf(k) for k in range(5)]
    coef = lu_solve(matrix([[x ** k for k in range(5)] for x in xs]), matrix([resultant(x) for x in xs]))   # ascending powers
    coef = [coef[k] for k in range(5)]
    big = max(abs(c) for c in coef)
    while len(coef) > 1 and abs(coef[-1]) <= big * mpf("1e-50"):
        coef.pop()
    if len(coef) < 2:
        return []
    out = []
    for r in polyroots(coef[::-1], maxsteps=500, extraprec=400):
        if abs(r.imag) > mpf("1e-25") * (1 + abs(r.real)) or r.real <= 0:
            continue
        v = r.real
        p1, p0, q1, q0 = quadratics(v)
        disc = cg * cg - q0
        cands = [cg + sqrt(disc), cg - sqrt(disc)] if disc > 0 else [cg]
        if disc > 0 and abs(p1 - q1) > mpf("1e-20"):   # the common root of the two quadratics, the nearer of the two candidates
            common = -(p0 - q0) / (p1 - q1)
            cands = [min(cands, key=lambda u: abs(u - common))]
        for u in cands:
            if u > 0 and abs(u * u + p1 * u + p0) <= mpf("1e-20") * (1 + u * u):
                s1 = sqrt(b2 / (1 + v * v - 2 * v * cb))
                out.append((s1, u * s1, v * s1, v))
    return sorted(out, key=lambda s: s[3])


def _newton_depths(P, J, s):
    """the solution of the cosine laws next to s (three Newton steps: for the finite differences of kappa)"""
    a2, b2, c2, ca, cb, cg = _triangle(P, J)
    s = list(s)
    for _ in range(3):
        F = matrix([s[1] ** 2 + s[2] ** 2 - 2 * s[1] * s[2] * ca - a2, s[0] ** 2 + s[2] ** 2 - 2 * s[0] * s[2] * cb - b2, s[0] ** 2 + s[1] ** 2 - 2 * s[0] * s[1] * cg - c2])
        Jm = matrix([[0, 2 * s[1] - 2 * s[2] * ca, 2 * s[2] - 2 * s[1] * ca], [2 * s[0] - 2 * s[2] * cb, 0, 2 * s[2] - 2 * s[0] * cb], [2 * s[0] - 2 * s[1] * cg, 2 * s[1] - 2 * s[0] * cg, 0]])
        d = lu_solve(Jm, F)
        s = [s[k] - d[k] for k in range(3)]
    return s


def _rigid(P, J, s):
    Q = [[s[i] * J[i][k] for k in range(3)] for i in range(3)]

    def frame(A):
        e1, e2 = _sub(A[1], A[0]), _sub(A[2], A[0])
        n = _cross(e1, e2)
        return matrix([[e1[r], e2[r], n[r]] for r in range(3)])
    R = frame(Q) * frame(P) ** -1
    pc = [sum(P[i][k] for i in range(3)) / 3 for k in range(3)]; qc = [sum(Q[i][k] for i in range(3)) / 3 for k in range(3)]
    t = [qc[r] - sum(R[r, k] * pc[k] for k in range(3)) for r in range(3)]
    return R, t


def solve_one(cam, X, xy, idx, normalised_bearing=True, pick=0, want_kappa=True):
    """One subset.  X [n,3] float32, xy [n,2] float32, idx its four indices.  normalised_bearing=False and pick=1 are the seeded errors of
    test_p3p_reference.py (the bearing (x, y, 1) left unnormalised; the runner-up chosen)."""
    out = dict(status=0, num_solutions=0, pose=None, unit=None, runner_up=None, closest_pair=None, leave_out=False, kappa_max=None)
    idx = [int(i) for i in idx]
    if len(set(idx)) < 4:
        return out
    P = [[mpf(float(X[i, k])) for k in range(3)] for i in idx[:3]]
    if any(all(P[i][k] == P[j][k] for k in range(3)) for i in range(3) for j in range(i + 1, 3)):
        return out
    c = [sum(p[k] for p in P) / 3 for k in range(3)]
    sv = sorted(svd_r(matrix([_sub(p, c) for p in P]), compute_uv=False), reverse=True)
    if not sv[1] > mpf(1e-4) * sv[0]:
        return out
    uv = [normalise(cam, xy[i, 0], xy[i, 1]) for i in idx]
    J = [_bearing(x, y, normalised_bearing) for x, y in uv[:3]]
    P4 = [mpf(float(X[idx[3], k])) for k in range(3)]
    b = sqrt(_dot(_sub(P[0], P[2]), _sub(P[0], P[2])))
    adm = []
    for s1, s2, s3, v in _depth_solutions(P, J):
        if not min(s1, s2, s3) > mpf(1e-9) * b:
            continue
        R, t = _rigid(P, J, (s1, s2, s3))
        x4 = [sum(R[r, k] * P4[k] for k in range(3)) + t[r] for r in range(3)]
        if not x4[2] > 0:
            continue
        adm.append(dict(s=(s1, s2, s3), v=v, R=R, t=t, dist=sqrt((x4[0] / x4[2] - uv[3][0]) ** 2 + (x4[1] / x4[2] - uv[3][1]) ** 2)))
    if not adm:
        return out
    order = sorted(range(len(adm)), key=lambda i: (adm[i]["dist"], i))   # ties: the solution found first, ascending v
    best = adm[order[min(pick, len(order) - 1)]]
    pose = _pose_from_rt(best["R"], best["t"])
    out.update(status=1, num_solutions=len(adm), pose=[float(p) for p in pose])
    if len(order) > 1:
        out["runner_up"] = float(adm[order[1]]["dist"])
        vs = [a["v"] for a in adm]
        out["closest_pair"] = float(min(abs(vs[i] - vs[k]) / max(vs[i], vs[k]) for i in range(len(vs)) for k in range(i + 1, len(vs))))
    if want_kappa:
        x0 = [p[k] for p in P for k in range(3)] + [w for pt in uv[:3] for w in pt]

        def pose_of(x):
            Pp = [x[0:3], x[3:6], x[6:9]]
            Jp = [_bearing(x[9], x[10], normalised_bearing), _bearing(x[11], x[12], normalised_bearing), _bearing(x[13], x[14], normalised_bearing)]
            return _pose_from_rt(*_rigid(Pp, Jp, _newton_depths(Pp, Jp, best["s"])))
        kappa = [mpf(0)] * 6
        for jx in range(15):
            h = mpf("1e-25") * max(abs(x0[jx]), mpf(1))
            xp = list(x0); xm = list(x0); xp[jx] += h; xm[jx] -= h
            pp, pm = pose_of(xp), pose_of(xm)
            for k in range(6):
                kappa[k] += abs((pp[k] - pm[k]) / (2 * h)) * abs(x0[jx])
        out["unit"] = [float((kappa[k] + abs(pose[k])) * EPS) for k in range(6)]
        out["kappa_max"] = float(max(kappa))
        out["leave_out"] = bool((out["runner_up"] is not None and out["runner_up"] < 1e-4) or out["kappa_max"] > 1e6
                                or (out["closest_pair"] is not None and out["closest_pair"] < 1e-6))
    return out


# ---------------------------------------------------------------- the shared cases ----------------------------------------------------------------
CAM_DIST = np.array([800.0, 800.0, -0.05, 0.01, 1e-3, -1e-3, 2e-3, 640.0, 360.0])
CAM_PLAIN = np.array([800.0, 800.0, 0.0, 0.0, 0.0, 0.0, 0.0, 640.0, 360.0])
CAM_EXACT = np.array([768.0, 768.0, 0.0, 0.0, 0.0, 0.0, 0.0, 640.0, 360.0])
MAIN_SEEDS = {"main_pinhole": 3, "main_distorted": 4}


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


def _scene(cam, pose, X, subsets):
    X = np.asarray(X, dtype=np.float32)
    return dict(cam=cam, X=X, xy=project(cam, pose, X).astype(np.float32), subsets=np.asarray(subsets, dtype=np.int32).reshape(-1, 4), pose=np.asarray(pose, dtype=np.float64))


def _main_scene(cam, seed):
    """24 points in a 6 m cube seen from about 9 m, noise-free projections rounded to float; 65 random four-point subsets"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3, 3, (24, 3))
    subs = [rng.choice(24, 4, replace=False) for _ in range(65)]
    return _scene(cam, np.array([0.10, -0.15, 0.07, 0.5, -0.4, -9.0]), X, subs)


def _half_turn_scene():
    """the exact half-turn data of the DLT reference (integer camera-frame points, fx = fy = 768: every float coordinate exact)"""
    from pnp_dlt_reference import _half_turn_scene as dlt_scene
    sc = dlt_scene()
    rng = np.random.default_rng(9)
    return dict(sc, subsets=np.array([rng.choice(12, 4, replace=False) for _ in range(6)], dtype=np.int32))


def _identity_scene():
    """the camera at zero rotation with EXACT data (integer camera-frame points at depths 3 * 2^k through fx = fy = 768, an integer centre):
    the recovered rotation is the identity to rounding and pose_from_rt takes its small-angle branch"""
    rng = np.random.default_rng(17)
    pts = set()
    while len(pts) < 8:
        z = int(rng.choice([3, 6, 12, 24]))
        pts.add((int(rng.integers(-z // 2, z // 2 + 1)), int(rng.integers(-z // 3, z // 3 + 1)), z))
    centre = np.array([1.0, -2.0, -3.0])
    sc = _scene(CAM_EXACT, np.array([0.0, 0.0, 0.0, *centre]), np.array(sorted(pts), dtype=np.float64) + centre, [rng.choice(8, 4, replace=False) for _ in range(5)])
    assert np.array_equal(project(CAM_EXACT, sc["pose"], sc["X"]), sc["xy"].astype(np.float64))
    return sc


def _four_roots_scene():
    """Fischler and Bolles' example made scalene: a triangle with sides near 2 sqrt(3) seen from near its axis at leg length 4 has four
    solutions with positive depths ((4, 4, 4) and the three permutations of (1, 4, 4) in the symmetric limit, where two of them share
    v = 1 and D vanishes — hence the offsets); the fourth point lies next to the triangle, in front of the camera in all four."""
    X = np.array([[2.0, 0.1, 0.0], [-1.1, 1.8, 0.05], [-0.9, -1.7, -0.05], [0.15, 0.1, 0.3]])
    centre = np.array([0.12, -0.08, -3.4])
    return _scene(CAM_PLAIN, np.array([0.02, -0.03, 0.3, *centre]), X, [[0, 1, 2, 3], [1, 2, 0, 3], [2, 0, 1, 3]])


def _degenerate_scene():
    """point 5 repeats point 1; 6, 7, 8 lie on a line; 9 lies far behind the camera, beyond it on the line from the cloud through the camera;
    10, 11 and 12 or 13 (the subsets of the case `sliver`) make a sliver either side of the collinearity threshold: base 4, height h, singular values sqrt(8) and h sqrt(2 / 3),
    so h = 2.4e-4 is a ratio of 0.7e-4 (declined) and h = 5.2e-4 one of 1.5e-4 (solved)"""
    base = _main_scene(CAM_DIST, MAIN_SEEDS["main_distorted"])
    X = np.zeros((14, 3), dtype=np.float32)
    X[:5] = base["X"][:5]
    X[5] = X[1]
    X[6:9] = np.array([0.5, -0.2, 1.0]) + np.array([-1.5, 0.0, 2.0])[:, None] * np.array([1.0, 0.4, 0.7])
    c = base["pose"][3:]
    X[9] = c + 200.0 * (c - X[:5].mean(axis=0))
    X[10:] = [[-2.0, 0.5, 1.0], [2.0, 0.5, 1.0], [0.0, 0.5 + 2.4e-4, 1.0], [0.0, 0.5 + 5.2e-4, 1.0]]
    sc = _scene(CAM_DIST, base["pose"], X, [[0, 1, 2, 0], [0, 2, 2, 3], [0, 1, 5, 3], [5, 1, 2, 3], [6, 7, 8, 0], [0, 1, 2, 9], [1, 3, 4, 9], [0, 2, 4, 9], [0, 1, 2, 3]])
    sc["xy"][9] = (640.0, 360.0)
    return sc


def _lost_leading_coefficient_scene():
    """P2 P3 = -+(6, 2, 3) is a diameter of the sphere of radius 7 about the origin, and the camera centre (2, -3, -6) and P1 = (3, 6, 2)
    or (-3, 6, 2) lie on that sphere: the camera sees P2 P3 under a right angle, the triangle's angle at P1 (Thales, twice) — the quartic's
    leading coefficient vanishes.  Integer world points make K = (a^2 - c^2) / b^2 = 1 exactly; the image points are rounded to float, so
    cos(alpha) ~ 1e-8 and A4 = -4 (c^2 / b^2) cos(alpha)^2 ~ 1e-15 of the other coefficients.  The subsets that start at another
    vertex see the same triangles with the right angle elsewhere; (1, 2, 1), inside the sphere, makes ordinary triples for comparison."""
    X = np.array([[3.0, 6.0, 2.0], [-6.0, -2.0, -3.0], [6.0, 2.0, 3.0], [-3.0, 6.0, 2.0], [1.0, 2.0, 1.0], [1.0, 1.0, 2.0], [-1.0, 2.0, 4.0]])
    subs = [[0, 1, 2, 5], [3, 1, 2, 5], [0, 1, 2, 6], [3, 1, 2, 6], [1, 2, 0, 5], [2, 3, 1, 6], [4, 1, 2, 5], [4, 1, 2, 6]]
    return _scene(CAM_EXACT, np.array([0.05, 0.2, -0.3, 2.0, -3.0, -6.0]), X, subs)


def cases():
    """name -> dict(cam, X [n,3] float32, xy [n,2] float32, subsets [T,4] int32, pose)"""
    out = {}
    out["main_pinhole"] = _main_scene(CAM_PLAIN, MAIN_SEEDS["main_pinhole"])       # 65 subsets: one full wave and one lane
    out["main_distorted"] = _main_scene(CAM_DIST, MAIN_SEEDS["main_distorted"])
    base = out["main_distorted"]
    out["single"] = dict(base, X=base["X"][:4], xy=base["xy"][:4], subsets=np.arange(4, dtype=np.int32)[None, :])   # n = 4, one task
    out["identity"] = _identity_scene()
    out["half_turn"] = _half_turn_scene()
    out["four_roots"] = _four_roots_scene()
    out["degenerate"] = _degenerate_scene()
    out["sliver"] = dict(out["degenerate"], subsets=np.array([[10, 11, 12, 3], [10, 11, 13, 3]], dtype=np.int32))   # declined, solved: pins the threshold
    out["lost_leading_coefficient"] = _lost_leading_coefficient_scene()
    return out


_REFERENCE = {}


def reference(name):
    """the extended-precision results of one case, computed once per process"""
    if name not in _REFERENCE:
        c = cases()[name]
        _REFERENCE[name] = [solve_one(c["cam"], c["X"], c["xy"], s) for s in c["subsets"]]
    return _REFERENCE[name]


# ------------------------------------------- the host program (tests/p3p_host.cpp), for the tests and make_p3p_bound.py -------------------------------------------
def write_case_file(path, case_list):
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(case_list)))
        for c in case_list:
            f.write(struct.pack("<2i", len(c["X"]), len(c["subsets"]))); f.write(np.asarray(c["cam"], dtype="<f8").tobytes())
            f.write(c["X"].astype("<f4").tobytes()); f.write(c["xy"].astype("<f4").tobytes()); f.write(np.asarray(c["subsets"]).astype("<i4").tobytes())


def run_host(exe, directory, case_list, mode=0):
    """per case: (status [T], num_solutions [T], poses [T,6]) of the C++ p3p_pose (mode 0) or one of its seeded errors"""
    import os
    import subprocess
    path = os.path.join(str(directory), "cases.bin")
    write_case_file(path, case_list)
    rows = [[float(x) for x in line.split()] for line in subprocess.run([exe, path, str(mode)], check=True, capture_output=True, text=True).stdout.strip().split("\n")]
    out, k = [], 0
    for c in case_list:
        r = np.array(rows[k:k + len(c["subsets"])]); k += len(c["subsets"])
        out.append((r[:, 0].astype(int), r[:, 1].astype(int), r[:, 2:]))
    return out


def worst_error(ref, status, poses):
    """worst |pose_k - reference_k| / unit_k over the subsets both accept and the reference does not leave out"""
    worst = 0.0
    for t, r in enumerate(ref):
        if r["status"] and status[t] and not r["leave_out"]:
            worst = max(worst, float(np.max(np.abs(poses[t] - np.array(r["pose"])) / np.array(r["unit"]))))
    return worst
