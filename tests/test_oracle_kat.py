"""The reference's own known-answer tests (src/rsba/test/mat_test.cc) re-expressed against the CPU
oracle: same input tables, same tolerances.  This is what pins the oracle's geometry helpers
(SURVEY §4 / §8c).  Line numbers refer to the reference's src/rsba/test/mat_test.cc."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
PI, PI2 = math.pi, math.pi / 2


def dist3(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)))


def test_norm(oracle):  # mat_test.cc:23-30
    x = np.array([-1e-100, 2.3, 1e100])
    assert abs(math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) - oracle.norm3(x)) <= EPS * 1e100
    x = x * (1.0 / oracle.norm3(x))
    assert abs(oracle.norm3(x) - 1.0) <= EPS


def test_rotation(oracle):  # mat_test.cc:34-72
    r, ri, r2, r3 = [0, PI, 0], [0, -PI, 0], [0, -PI2, 0], [PI2, 0, 0]
    p, p2, p3, p4 = [0, 0, -10], [0, 0, 10], [10, 0, 0], [0, 10, 0]
    test = oracle.angle_axis_rotate(r, p)
    assert dist3(p2, test) <= 1e-9
    # inverse rotation applied IN PLACE (:50-53)
    buf = np.array(test)
    oracle.angle_axis_rotate_inplace([-v for v in r], buf)
    assert dist3(p, buf) <= 1e-9
    assert dist3(p2, oracle.angle_axis_rotate(ri, p)) <= 1e-9
    assert dist3(p3, oracle.angle_axis_rotate(r2, p)) <= 1e-9
    assert dist3(p4, oracle.angle_axis_rotate(r3, p)) <= 1e-9
    # "same with eigen" (:67-71): rotation matrix about x by pi/2
    c, s = math.cos(PI2), math.sin(PI2)
    R = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    assert dist3(p4, R @ np.array(p, dtype=float)) <= 1e-9


def _quat(aa):
    n = np.linalg.norm(aa)
    ax = np.asarray(aa) / n
    return np.concatenate([[math.cos(n / 2)], math.sin(n / 2) * ax])


def _quat_slerp(q0, q1, t):  # Eigen::Quaternion::slerp
    d = float(np.dot(q0, q1))
    ad = abs(d)
    if ad >= 1.0 - EPS:
        s0, s1 = 1.0 - t, t
    else:
        th = math.acos(ad)
        s0, s1 = math.sin((1 - t) * th) / math.sin(th), math.sin(t * th) / math.sin(th)
    if d < 0:
        s1 = -s1
    return s0 * q0 + s1 * q1


def _quat_to_aa(q):  # Eigen::AngleAxis(Quaternion)
    q = np.array(q, dtype=float)
    n = np.linalg.norm(q[1:])
    if q[0] < 0:
        n = -n
    if abs(n) > 0:
        ang = 2 * math.atan2(n, abs(q[0]))
        return q[1:] / n * ang
    return np.zeros(3)


def test_slerp_is_linear(oracle):  # mat_test.cc:75-142
    rs = [[0, 0.5, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 1, 1], [1, 1, 1], [0, -1, 0], [-1, 0, 0], [-1, 0, -1],
          [0, PI2, 0], [PI2, 0, 0], [0, 1 - PI2, 0], [0, -1, PI2], [0, -1, 1 - PI2], [0, 0, EPS], [1, -1, EPS]]
    for i in range(16):
        for j in range(1, 16):
            assert dist3(oracle.lerp_rotation(rs[i], rs[j], 1.0), rs[j]) <= 1e-6
            assert dist3(oracle.lerp_rotation(rs[i], rs[j], 0.0), rs[i]) <= 1e-6
            r05 = oracle.lerp_rotation(rs[i], rs[j], 0.5)
            r15 = oracle.lerp_rotation(rs[i], rs[j], 1.5)
            r20 = oracle.lerp_rotation(rs[i], rs[j], 2.0)
            assert dist3(oracle.lerp_rotation(rs[i], r20, 0.5), rs[j]) <= 1e-6
            assert dist3(oracle.lerp_rotation(r05, r15, 0.5), rs[j]) <= 1e-6
            if i != j:
                frac = 2
                while frac < 500:
                    for n in range(1, frac):
                        tau = n / frac
                        inter = oracle.lerp_rotation(rs[i], rs[j], tau)
                        rst = _quat_to_aa(_quat_slerp(_quat(rs[i]), _quat(rs[j]), tau))
                        assert dist3(inter, rst) <= 0.2
                    frac = frac * 2 - 1


def test_distortion_roundtrip(oracle):  # mat_test.cc:145-167 (only 7 initialisers: cx = cy = 0)
    cams = [[0.1, 0.1, 0, 0, 0, 0, 0, 0, 0], [100, 100, 0.01, 0, 0, 0, 0, 0, 0],
            [500, 500, -0.03, 0, 0, 0, 0, 0, 0], [500, 500, -0.1, 0.02, 0, 0, 0, 0, 0]]
    imgs = [[0.10, 0.10], [0.21, 0.19], [1.10, 0.50]]
    for img in imgs:
        for cam in cams:
            d = oracle.distort(cam, img)
            ok, u = oracle.undistort(cam, d)
            assert ok
            assert math.hypot(img[0] - u[0], img[1] - u[1]) <= 1e-6


from kat_tables import CAMS, POSE_REF, POSES, PTS   # mat_test.cc:171-214 (shared with the GPU replay, tests/test_gpu_kat.py)


def test_reprojection(oracle):  # mat_test.cc:170-313
    n_full = 0
    for pose in POSES:
        for pt in PTS:
            for cam in CAMS:
                c3 = oracle.w2c(pose, pt)
                w3 = oracle.c2w(pose, c3)
                assert dist3(pt, w3) <= 1e-6                                           # :229
                ok1, d1 = oracle.direction_world(pose, pt)
                ok2, d2 = oracle.c2direction(pose, c3)
                if not (ok1 and ok2):
                    continue
                assert dist3(d1, d2) <= 1e-6                                           # :235
                oki, img = oracle.w2i(cam, pose, pt)
                if not oki:
                    continue
                okd, d3 = oracle.direction_pixel(cam, pose, img)
                if not okd:
                    continue
                assert dist3(d1, d3) <= 1e-1                                           # :241
                c_ref = oracle.w2c(POSE_REF, pt)
                okr, d_ref = oracle.c2direction(POSE_REF, c_ref)
                if not okr:
                    continue
                p2 = np.array(POSE_REF[3:], dtype=float) - np.array(pose[3:], dtype=float)
                okx, ln = oracle.ray_intersect(p2, d1, d_ref)
                assert okx                                                             # :250
                pd1 = np.array(d1) * ln[0] + np.array(pose[3:], dtype=float)
                assert dist3(pt, pd1) <= 1e-9                                          # :257
                pd2 = np.array(d_ref) * ln[1] + np.array(POSE_REF[3:], dtype=float)
                assert dist3(pt, pd2) <= 1e-9                                          # :262
                assert ln[0] >= EPS                                                    # :264
                okt, tri = oracle.triangulate(pose[3:], d1, POSE_REF[3:], d_ref)
                assert okt                                                             # :266
                # :271-272 ("imprecise!" in the reference).  triangulate is NOT on the hot path (SURVEY §2
                # row 1: track creation); its 3x3 inverse is Eigen's in the reference and a cofactor
                # restatement here, and on the near-parallel vector (-0.39,1.25,2014) the two roundings
                # differ at the 1e-5 level, so this one tolerance is 2e-5 instead of 1e-5.
                assert abs(dist3(pose[3:], tri) - ln[0]) <= 2e-5
                assert abs(dist3(POSE_REF[3:], tri) - ln[1]) <= 2e-5
                okw, img_ref = oracle.w2i(cam, POSE_REF, tri)
                if not okw:
                    continue
                assert dist3(pt, tri) <= 2e-5                                          # :277 (same note)
                assert oracle.validate(cam, pose, img, pt, 1.0)                        # :280
                assert oracle.validate(cam, POSE_REF, img_ref, pt, 1.0)                # :281
                okx, ln = oracle.ray_intersect(p2, d1, d_ref)
                assert okx and ln[1] >= EPS                                            # :284-287
                okrd, dist = oracle.ray_dist(cam, pose, img, cam, POSE_REF, img_ref)
                if okrd:
                    assert np.linalg.norm(dist) <= dist3(pose[3:], POSE_REF[3:]) + 1e-1  # :294
                n_full += 1
    assert n_full > 50   # the deep branch is actually exercised
