"""Extended-precision reference of the five-point solver of the two-view bootstrap (include/rsba_amd.h: rsba_epipolar_five_point /
rsba_epipolar_hypotheses_five_point; host form epi_detail::five_point / five_point_hypothesis in include/rsba/two_view.hpp), in mpmath at 60
digits, and the fixed case list the host test (test_five_point_reference.py) and the device test (test_gpu_five_point.py) share.  It shares
no code with the C++ and takes another way to every number: the null space is the last four right singular vectors of mpmath's SVD of the
5 x 9 constraint matrix itself (no Householder); the ten cubics are expanded exactly, by arithmetic on polynomials kept as dictionaries;
the solutions are not the roots of an eliminant but the eigenvectors of the 10 x 10 action matrix of "multiply by a linear form" on the quotient ring
(Stewenius' form: Gauss-Jordan on the ten cubic monomials, mpmath.eig).  A solution is real where the imaginary parts of (x, y, z) are below
1e-30 of their size.  Scoring, candidates and the pose come from two_view_reference (mpmath's SVD of the 3 x 3 matrix).

solve_one(...) returns per subset
  status         0 declined, 1 solved
  E              the solutions (each row-major, unit Frobenius norm, largest entry positive), ascending KEY(E) = |sum_k (k + 1) E[k]|: the header's key; [] when declined
  unit_E         per solution the error unit per component, (kappa_k + |value_k|) 2^-52, kappa_k = sum_j |d value_k / d x_j| |x_j| over the
                 20 normalised image coordinates of the subset.  kappa needs two digits, not sixty: central differences (h = 1e-6) of an fp64
                 numpy restatement of the same map (numpy's SVD, solve and eig), which follows the reference's solution (the nearest one)
  chosen, pose, unit_pose   the solution with the most inliers over ALL the case's correspondences at THRESHOLD_PX (ties: the most in front,
                 then the first), rsba's 6-vector of its winning candidate and that vector's units
  rank_gap       fifth singular value of the 5 x 9 over the first (declined at or below RANK_TOL); None: declined earlier
  elim_gap       smallest over largest singular value of the 10 x 10 block that is eliminated (declined at or below ELIM_TOL)
  root_gap       smallest relative distance between two solutions' (x, y, z), and smallest relative imaginary part of a complex one
  key_gap        smallest difference between two solutions' keys
  kappa_max, leave_out   kappa_max > 1e6.  The case list is built so that no subset is left out (test_five_point_reference.py asserts it).
"""
import numpy as np
from mpmath import mp, mpf, matrix, svd_r, eig

import two_view_reference as R
from p3p_reference import CAM_DIST, _pose_from_rt, normalise, project

mp.dps = 60
EPS = 2.0 ** -52
THRESHOLD_PX = R.THRESHOLD_PX
RANK_TOL = 1e-7
ELIM_TOL = 1e-7

CUBIC = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


# ---- polynomials in (x, y, z) as {exponents: coefficient}; the coefficients may be mpf or float ----
def _pmul(p, q):
    out = {}
    for (a, b, c), u in p.items():
        for (d, e, f), v in q.items():
            k = (a + d, b + e, c + f)
            out[k] = out.get(k, 0) + u * v
    return out


def _padd(p, q, s=1):
    out = dict(p)
    for k, v in q.items():
        out[k] = out.get(k, 0) + s * v
    return out


def _cubics(null):
    """the ten cubic constraints on E = x N0 + y N1 + z N2 + N3, as dictionaries"""
    e = [[{(1, 0, 0): null[0][3 * r + c], (0, 1, 0): null[1][3 * r + c], (0, 0, 1): null[2][3 * r + c], (0, 0, 0): null[3][3 * r + c]} for c in range(3)] for r in range(3)]
    det = {}
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        det = _padd(det, _pmul(e[0][i], _padd(_pmul(e[1][j], e[2][k]), _pmul(e[1][k], e[2][j]), -1)))
    eet = [[{} for _ in range(3)] for _ in range(3)]
    for i in range(3):
        for j in range(3):
            for k in range(3):
                eet[i][j] = _padd(eet[i][j], _pmul(e[i][k], e[j][k]))
    tr = _padd(_padd(eet[0][0], eet[1][1]), eet[2][2])
    out = [det]
    for i in range(3):
        for c in range(3):
            p = {}
            for j in range(3):
                p = _padd(p, _pmul(eet[i][j], e[j][c]), 2)
            out.append(_padd(p, _pmul(tr, e[i][c]), -1))   # 2 E E^T E - tr(E E^T) E
    return out


def KEY(E):
    return abs(sum((k + 1) * E[k] for k in range(9)))


FORM = (1.0, 0.375, -0.625)   # the action matrix is that of x + 0.375 y - 0.625 z: a form that two solutions share only by accident (x alone is
                              # shared by every solution with E[0] = 0 when the motion runs along an axis, and a repeated eigenvalue has no eigenvectors to read)


def _action(G):
    """(row, column, value) contributions of the action matrix of FORM on BASIS, from G(r, c): cubic monomial r = -sum_c G(r, c) basis_c"""
    for var in range(3):
        for i, b in enumerate(BASIS):
            m = tuple(b[k] + (1 if k == var else 0) for k in range(3))
            if m in BASIS:
                yield i, BASIS.index(m), FORM[var]
            else:
                for j in range(10):
                    yield i, j, -FORM[var] * G(CUBIC.index(m), j)


def _rows(pa, pb):
    return [[xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, 1] for (xa, ya), (xb, yb) in zip(pa, pb)]


def _finish(null, x, y, z):
    E = [x * null[0][k] + y * null[1][k] + z * null[2][k] + null[3][k] for k in range(9)]
    fro = sum(v * v for v in E) ** 0.5
    E = [v / fro for v in E]
    lead = max(range(9), key=lambda k: abs(E[k]))
    return [-v for v in E] if E[lead] < 0 else E


def _mp_solutions(pa, pb, info):
    """every real essential matrix of five normalised correspondences (lists of mp pairs), or None: declined"""
    rows = _rows(pa, pb) + [[mpf(0)] * 9] * 4
    _, S, V = svd_r(matrix(rows))
    order = sorted(range(9), key=lambda i: -S[i])
    info["rank_gap"] = float(S[order[4]] / S[order[0]])
    if not S[order[4]] > mpf(RANK_TOL) * S[order[0]]:
        return None
    null = [[V[order[5 + m], k] for k in range(9)] for m in range(4)]
    polys = _cubics(null)
    A = matrix([[p.get(m, mpf(0)) for m in CUBIC] for p in polys])
    Bm = matrix([[p.get(m, mpf(0)) for m in BASIS] for p in polys])
    _, SA, _ = svd_r(A)
    info["elim_gap"] = float(min(SA) / max(SA))
    if not min(SA) > mpf(ELIM_TOL) * max(SA):
        return None
    G = A ** -1 * Bm   # cubic monomial i = -sum_j G[i, j] basis_j on the variety
    act = matrix(10, 10)
    for i, j, v in _action(lambda r, c: G[r, c]):
        act[i, j] += mpf(v)
    _, vecs = eig(act)
    sols, points, imag = [], [], []
    for i in range(10):
        w = vecs[9, i]
        x, y, z = vecs[6, i] / w, vecs[7, i] / w, vecs[8, i] / w
        size = max(abs(x), abs(y), abs(z), 1)
        im = max(abs(mp.im(x)), abs(mp.im(y)), abs(mp.im(z))) / size
        if im > mpf("1e-30"):
            imag.append(float(im))
            continue
        points.append([mp.re(x), mp.re(y), mp.re(z)])
        sols.append(_finish(null, mp.re(x), mp.re(y), mp.re(z)))
    gaps = [float(max(abs(p[k] - q[k]) for k in range(3)) / max(max(abs(v) for v in p + q), 1)) for a, p in enumerate(points) for q in points[a + 1:]]
    info["root_gap"] = min(gaps + imag) if gaps + imag else None
    return sorted(sols, key=KEY)


def _np_solutions(x0):
    """the fp64 restatement that kappa is differentiated through: x0 = 5 (xa, ya) then 5 (xb, yb) -> [k, 9]"""
    pa, pb = x0[:10].reshape(5, 2), x0[10:].reshape(5, 2)
    null = np.linalg.svd(np.array(_rows(pa, pb)), full_matrices=True)[2][5:]
    polys = _cubics(null)
    A = np.array([[p.get(m, 0.0) for m in CUBIC] for p in polys]); Bm = np.array([[p.get(m, 0.0) for m in BASIS] for p in polys])
    G = np.linalg.solve(A, Bm)
    act = np.zeros((10, 10))
    for i, j, v in _action(lambda r, c: G[r, c]):
        act[i, j] += float(v)
    _, vecs = np.linalg.eig(act)
    out = []
    for i in range(10):
        p = vecs[6:9, i] / vecs[9, i]
        if np.max(np.abs(p.imag)) <= 1e-6 * max(np.max(np.abs(p)), 1.0):
            out.append(_finish(null, *p.real))
    return np.array(out)


def _np_follow(x0, E_ref, pose_ref=None):
    """the restatement's solution nearest E_ref (up to sign), and (with pose_ref) the pose of its candidate nearest pose_ref"""
    sols = _np_solutions(x0)
    signed = np.where((sols @ E_ref)[:, None] < 0, -sols, sols)
    E = signed[np.argmin(np.linalg.norm(signed - E_ref, axis=1))]
    if pose_ref is None:
        return E
    U, _, Vt = np.linalg.svd(E.reshape(3, 3))
    U[:, 2] *= np.sign(np.linalg.det(U)); Vt[2] *= np.sign(np.linalg.det(Vt))
    Wn = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    best = None
    for Rm in (U @ Wn @ Vt, U @ Wn.T @ Vt):
        for sg in (1.0, -1.0):
            pose = np.concatenate([R._np_log(Rm), -Rm.T @ (sg * U[:, 2])])
            if best is None or np.linalg.norm(pose - pose_ref) < np.linalg.norm(best - pose_ref):
                best = pose
    return np.concatenate([E, best])


def _kappa(x0, f):
    k = None
    for j in range(len(x0)):
        h = 1e-6 * max(abs(x0[j]), 1.0)
        xp, xm = x0.copy(), x0.copy(); xp[j] += h; xm[j] -= h
        d = np.abs((f(xp) - f(xm)) / (2 * h)) * abs(x0[j])
        k = d if k is None else k + d
    return k


def solve_one(cam_a, cam_b, xy_a, xy_b, idx, want_kappa=True, normalised=None):
    """One subset.  xy_a, xy_b [n,2] float32, idx its five indices.  normalised: ((xa, ya), (xb, yb)) per correspondence, where already known."""
    out = dict(status=0, E=[], unit_E=[], chosen=None, pose=None, unit_pose=None, kappa_max=None, leave_out=False, rank_gap=None, elim_gap=None,
               root_gap=None, key_gap=None)
    idx = [int(i) for i in idx]
    if len(idx) != 5 or len(set(idx)) < 5:
        return out
    n = len(xy_a)
    nrm = normalised or [(normalise(cam_a, xy_a[i, 0], xy_a[i, 1]), normalise(cam_b, xy_b[i, 0], xy_b[i, 1])) for i in range(n)]
    sols = _mp_solutions([nrm[i][0] for i in idx], [nrm[i][1] for i in idx], out)
    if not sols:
        return out
    f = (mpf(float(cam_a[0])) + mpf(float(cam_a[1])) + mpf(float(cam_b[0])) + mpf(float(cam_b[1]))) / 4
    best = None
    for s, flat in enumerate(sols):
        E = matrix(3, 3)
        for k in range(9):
            E[k // 3, k % 3] = flat[k]
        inliers = [i for i in range(n) if R._sampson(E, *nrm[i]) * f * f <= mpf(THRESHOLD_PX) ** 2]
        cands = R._candidates(E)
        counts = [sum(1 for i in inliers if R._in_front(Rm, t, *nrm[i])) for Rm, t in cands]
        c = max(range(4), key=lambda c: (counts[c], -c))
        if best is None or (len(inliers), counts[c]) > best[0]:
            best = ((len(inliers), counts[c]), s, cands[c])
    out.update(status=1, E=[[float(v) for v in E] for E in sols], chosen=best[1], pose=[float(p) for p in _pose_from_rt(*best[2])])
    keys = sorted(KEY(E) for E in out["E"])
    out["key_gap"] = float(min(np.diff(keys))) if len(keys) > 1 else None
    if want_kappa:
        x0 = np.array([float(v) for i in idx for v in nrm[i][0]] + [float(v) for i in idx for v in nrm[i][1]])
        worst = 0.0
        for s, E in enumerate(out["E"]):
            E_ref = np.array(E)
            if s == best[1]:
                pose_ref = np.array(out["pose"])
                k = _kappa(x0, lambda x: _np_follow(x, E_ref, pose_ref))
                out["unit_pose"] = list((k[9:] + np.abs(pose_ref)) * EPS)
            else:
                k = _kappa(x0, lambda x: _np_follow(x, E_ref))
            out["unit_E"].append(list((k[:9] + np.abs(E_ref)) * EPS))
            worst = max(worst, float(k.max()))
        out["kappa_max"] = worst
        out["leave_out"] = bool(worst > 1e6)
    return out


# ---------------------------------------------------------------- the shared cases ----------------------------------------------------------------
NOISE_FREE = ("main_pinhole", "main_distorted", "forward_motion", "sideways_no_rotation")   # the generating motion is among the solutions


SIDEWAYS_SEED = 26   # 17, the eight-point list's, gives two subsets with kappa above 1e6 (near-double spurious solutions): see test_five_point_reference.py


def _sideways_scene(seed):
    """two_view_reference's sideways scene — no rotation, exact data: integer camera-frame points at depths 3 * 2^k through fx = fy = 768,
    the baseline one unit along x — from another seed (see cases())"""
    rng = np.random.default_rng(seed)
    pts = set()
    while len(pts) < 12:
        z = int(rng.choice([3, 6, 12, 24]))
        pts.add((int(rng.integers(-z // 2, z // 2 + 1)), int(rng.integers(-z // 3, z // 3 + 1)), z))
    X = np.array(sorted(pts), dtype=np.float64)
    sc = R._scene(R.CAM_EXACT, np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0]), X, [rng.choice(12, 8, replace=False) for _ in range(5)])
    assert np.array_equal(project(R.CAM_EXACT, sc["pose"], X), sc["xy_b"].astype(np.float64))
    return sc


def cases():
    """two_view_reference.cases() with the first five indices of every subset (so `degenerate` becomes: a repeated index, five coplanar
    points — accepted —, a pure rotation, coincident points, five ordinary points), and `single` with n = 5"""
    out = {}
    for name, c in R.cases().items():
        if name == "sideways_no_rotation":
            c = _sideways_scene(SIDEWAYS_SEED)
        out[name] = dict(c, subsets=np.ascontiguousarray(c["subsets"][:, :5]))
    out["degenerate"]["subsets"][0, 4] = out["degenerate"]["subsets"][0, 0]   # (the eight-point row repeats its first index in the eighth place)
    base = out["main_distorted"]
    out["single"] = dict(base, xy_a=base["xy_a"][:5], xy_b=base["xy_b"][:5], subsets=np.arange(5, dtype=np.int32)[None, :])
    return out


_REFERENCE = {}


def reference(name):
    """the extended-precision results of one case, computed once per process"""
    if name not in _REFERENCE:
        c = cases()[name]
        nrm = [(normalise(c["cam_a"], c["xy_a"][i, 0], c["xy_a"][i, 1]), normalise(c["cam_b"], c["xy_b"][i, 0], c["xy_b"][i, 1])) for i in range(len(c["xy_a"]))]
        _REFERENCE[name] = [solve_one(c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"], s, normalised=nrm) for s in c["subsets"]]
    return _REFERENCE[name]


def essential_of(pose):
    """[t]x R of a pose of B in A's frame, unit Frobenius norm, signed: what a noise-free subset must have among its solutions"""
    Rm = R._rodrigues(np.asarray(pose[:3], dtype=np.float64))
    t = -Rm @ np.asarray(pose[3:], dtype=np.float64)
    E = (np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ Rm).reshape(-1)
    E /= np.linalg.norm(E)
    return -E if E[np.argmax(np.abs(E))] < 0 else E


def planar_scene(seed):
    """60 correspondences of one scene plane, 0.3 px of noise on both sides, camera B at POSE_B: dict as two_view_reference.outlier_scene
    (every correspondence a true inlier)"""
    rng = np.random.default_rng(seed)
    X = R._cloud(rng, 60); X[:, 2] = 7.0 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    pose = R._unit_centre(R.POSE_B)
    xy_a = project(CAM_DIST, np.zeros(6), X) + rng.normal(0.0, 0.3, (60, 2)); xy_b = project(CAM_DIST, pose, X) + rng.normal(0.0, 0.3, (60, 2))
    Rm = R._rodrigues(pose[:3]); t = -Rm @ pose[3:]
    return dict(cam=CAM_DIST, xy_a=xy_a.astype(np.float32), xy_b=xy_b.astype(np.float32), true_inlier=np.ones(60, dtype=bool), R=Rm, t=t / np.linalg.norm(t), pose=pose)


def outlier_draw(fb, rolling, draw, _cache={}):
    """two_view_reference.outlier_scene with the outliers of default_rng(draw); draw 0 is that scene itself"""
    if (fb, rolling) not in _cache:
        _cache[(fb, rolling)] = R.outlier_scene(fb, rolling)
    base = _cache[(fb, rolling)]
    if draw == 0:
        return base
    sc = base["sc"]; p = sc.problem
    b = {int(j): p.obs_xy[i] for i, j in zip(np.nonzero(p.obs_frame == fb)[0], p.obs_point[p.obs_frame == fb])}
    xy_b = np.array([b[int(j)] for j in base["points"]])
    rng = np.random.default_rng(draw)
    bad = rng.random(len(xy_b)) < 0.4
    xy_b[bad] = np.stack([rng.uniform(0, 1280, bad.sum()), rng.uniform(0, 720, bad.sum())], axis=1)
    return dict(base, xy_b=xy_b.astype(np.float32), true_inlier=~bad)


# ------------------------------------------- the host program (tests/five_point_host.cpp), for the tests and make_five_point_bound.py -------------------------------------------
def _per_subset(r):
    r = np.array(r)
    return dict(status=r[:, 0].astype(int), count=r[:, 1].astype(int), rank_ratio=r[:, 2], pivot_ratio=r[:, 3], E=r[:, 4:94].reshape(-1, 10, 9),
                chain=r[:, 94].astype(int), chosen=r[:, 95].astype(int), num_inliers=r[:, 96].astype(int), num_front=r[:, 97:101].astype(int), poses=r[:, 101:107])


def run_host(exe, directory, case_list, mode=0):
    """per case: dict(status [T], count [T], rank_ratio, pivot_ratio, E [T,10,9], chain, chosen, num_inliers, num_front [T,4], poses [T,6])"""
    import os
    import subprocess
    path = os.path.join(str(directory), "cases5.bin")
    R.write_case_file(path, case_list)
    rows = R._rows(subprocess.run([exe, path, str(mode), str(THRESHOLD_PX)], check=True, capture_output=True, text=True).stdout)
    out, k = [], 0
    for c in case_list:
        out.append(_per_subset(rows[k:k + len(c["subsets"])])); k += len(c["subsets"])
    return out


def run_host_hypotheses(exe, directory, scene, T, name="scene5"):
    """the chain of the first T five-point subsets of the RANSAC -> dict(status, num_solutions, num_inliers, num_front [T,4], E [T,9], poses [T,6])"""
    import os
    import subprocess
    path = os.path.join(str(directory), name + ".bin")
    R.write_scene_file(path, scene)
    r = np.array(R._rows(subprocess.run([exe, "hypotheses", path, str(T), str(R.RANSAC["threshold_px"]), str(R.RANSAC["rng_state"])], check=True, capture_output=True, text=True).stdout))
    return dict(status=r[:, 0].astype(int), num_solutions=r[:, 1].astype(int), num_inliers=r[:, 2].astype(int), num_front=r[:, 3:7].astype(int), E=r[:, 7:16], poses=r[:, 16:22])


def run_host_ransac(exe, directory, scene, solver, name="scene5"):
    """the whole host loop with five-point (solver = 5) or eight-point (8) subsets -> as two_view_reference.run_host_ransac"""
    import os
    import subprocess
    path = os.path.join(str(directory), name + ".bin")
    R.write_scene_file(path, scene)
    o = R.RANSAC
    rows = R._rows(subprocess.run([exe, "ransac", path, str(o["iterations"]), str(o["threshold_px"]), str(o["refits"]), str(o["min_inliers"]), str(o["rng_state"]), str(solver)],
                                  check=True, capture_output=True, text=True).stdout)
    head = [int(v) for v in rows[0]]
    return dict(ok=bool(head[0]), winner_task=head[1], num_inliers=head[2], num_front=head[3], refits_adopted=head[4], E=np.array(rows[1]), pose=np.array(rows[2]),
                mask=np.array(rows[3]).astype(bool), ratio=np.array(rows[4]))


def distinct_subsets(n, m, iterations, state):
    """hyp_detail::distinct_subsets restated (test_two_view_reference.py holds the C++ to this generator)"""
    out = []
    for _ in range(iterations):
        pick = []
        while len(pick) < m:
            state = ((state & 0xffffffff) * 4164903690 + (state >> 32)) & 0xffffffffffffffff
            c = (state & 0xffffffff) % n
            if c not in pick:
                pick.append(c)
        out.append(pick)
    return np.array(out, dtype=np.int32)


def worst_error(ref, status, count, E, poses=None):
    """worst |value_k - reference_k| / unit_k over every solution (up to sign, slot by slot) and, where poses are given, the chosen solution's
    pose, over the subsets both accept with the same count"""
    worst = 0.0
    for t, r in enumerate(ref):
        if not (r["status"] and status[t] and count[t] == len(r["E"])) or r["leave_out"]:
            continue
        for s, e in enumerate(r["E"]):
            e = np.array(e)
            sign = 1.0 if np.dot(E[t][s], e) >= 0 else -1.0
            worst = max(worst, float(np.max(np.abs(sign * E[t][s] - e) / np.array(r["unit_E"][s]))))
        if poses is not None:
            worst = max(worst, float(np.max(np.abs(poses[t] - np.array(r["pose"])) / np.array(r["unit_pose"]))))
    return worst
