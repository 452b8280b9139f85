"""CPU tests of the mpmath model of tests/geometry_reference.py, and the calibration of the device checks of
tests/test_gpu_geometry.py: the check functions below are the ones the device results go through; here the CPU oracle goes through
them, the input sets are shown to stay inside their caps (at most 1 % of a set undecided, both outcomes present), and seven wrong
variants of the model are shown to be seen by them.

The constants, each 8 times the oracle's worst ratio on these inputs rounded up to a power of two (16 times for the cost):
  C_A   reproject:   |xy - xy_mp|_inf <= C_A * 2^-53 * (|xy|_inf + fx + fy) * amp
                     oracle's worst 11.4 -> C_A = 128.  (11.4 on the clamped items of the frame whose poses are 20 apart, which project
                     7000 - 18000 px outside the image, where the distortion polynomial multiplies the rounding of the normalised
                     point; 1.43 inside the image.)
  C_C   tri_pt:      |p - p_mp|_inf <= C_C * cond(A) * 2^-53 * (|c1|_inf + |c2|_inf + |p|_inf) * amp_u
                     oracle's triangulate alone, on exact rays: 0.89; the whole composition (direction_pixel, triangulate): 2.84 -> C_C = 32
  C_TOL one LM step: |delta - delta_mp|_inf <= C_TOL * kappa * 2^-53 * |delta_mp|_inf + 2 ulp(x)   (64, of test_lm_step_reference.py);
                     oracle's worst 2.4
  C_E   final_cost:  |cost - cost_mp(x + delta_mp)| <= C_E * cost0, oracle's worst 2.03e-14 (VERTICAL, m = 6, where the functor's
                     tau from x leaves a cost of 30 after 3300; at most 5.8e-16 under the other shutters) -> C_E = 16 * 2.03e-14 = 3.3e-13
amp is the factor by which a fixed-point replay amplifies a per-step rounding error along the model's own ratios of successive
moves (geometry_reference.contraction): at most 1 / (1 - L), and defined also where the iteration runs away before it settles at
a clamped pose.  The reprojection bound is far inside the 1e-9 max(1, |xy|) of tests/test_gpu_filter.py
(test_the_reprojection_bound_is_tighter_than_the_old_one).

Margin rules (an item is decided when every comparison the model made clears them):
  A  every squared move 1e-6 relative away from 1e-6, every z 1e-6 relative away from 1e-8, a scan-line coordinate 1e-9 away
     from a half
  B  squared error 1e-9 relative, camera distance 1e-12 relative, z 1e-6 relative
  C  undistortion stop tests 1e-5 relative (the error of |distort(p_u) - p_n|, a few 2^-53 |p_n|, is 1e-10 of the stopping
     tolerance 1.25e-6 |p_n|, times the replay's amplification); det(A) 1e-12 away from DBL_EPSILON (A has entries of size 1);
     the tests on the triangulated point by what its bound allows: distances 2 bound + 1e-12 relative, z 2 bound, pixel error
     4 (fx + fy) bound / z + 1e-9 away from the threshold's root; the reprojectMatches test as in B
  D  |dist - thr| > 4 * 2^-24 * max(|ix|, |iy|, thr)
  E  preconditions instead: the step is accepted (rho > 0.1) and no convergence test is within a factor 100 of its limit."""
import numpy as np
import pytest

import geometry_reference as G
from geometry_reference import GLOBAL, HORIZONTAL, VERTICAL, M, mpv
from test_lm_step_reference import C_TOL

C_A = 128
C_C = 32
C_E = 3.3e-13
RULE_A = dict(move=1e-6, z=1e-6, line=1e-9)
RULE_B = dict(err=1e-9, dist=1e-12, z=1e-6)
EPS = G.EPS53


def cap(undecided, n):
    """at most 1 % of a test's items may be undecided"""
    return undecided <= n // 100


def mp_inf(got, ref):
    """|got - ref|_inf, the difference taken in mp"""
    return float(max(abs(M(float(g)) - r) for g, r in zip(np.ravel(got), ref)))


# ================================================================ the checks ================================================================
def check_reproject(case, model, xy, ok):
    """part A.  -> (worst error in units of 2^-53 (|xy| + fx + fy) amp, undecided items)"""
    worst, undecided = 0.0, 0
    for i, r in enumerate(model):
        if not G.decided(r["margins"], **RULE_A):
            undecided += 1
            continue
        assert bool(ok[i]) == r["ok"], (i, r["reason"], r["margins"])
        if r["ok"]:
            cam = case["items"][i][0]
            unit = EPS * (float(max(abs(v) for v in r["xy"])) + cam[0] + cam[1]) * r["amp"]
            worst = max(worst, mp_inf(xy[i], r["xy"]) / unit)
    assert cap(undecided, len(model)), undecided
    assert worst <= C_A, worst
    return worst, undecided


def check_validate(case, model, flags):
    """part B.  -> undecided items"""
    dec = np.array([G.decided(m, **RULE_B) for _, m, _ in model])
    want = np.array([f for f, _, _ in model])
    bad = np.flatnonzero(dec & (np.asarray(flags, dtype=bool) != want))
    assert len(bad) == 0, (bad[:5], [model[i][1] for i in bad[:5]])
    assert dec[case["band"]].all()                           # the near-threshold band is decided, hence exact
    assert cap(int((~dec).sum()), len(model))
    return int((~dec).sum())


def check_tracks(case, model, tri_ok, tri_pt, rep_ok):
    """part C.  -> (worst error of tri_pt in units of cond 2^-53 scale amp, undecided flags)"""
    worst, undecided = 0.0, 0
    for c, r in enumerate(model):
        rq = int(case["request"][c])
        if not rq & 2:
            assert not rep_ok[c]
        elif r["decided_rep"]:
            assert bool(rep_ok[c]) == r["reproj_ok"], c
        if not rq & 1:
            assert not tri_ok[c] and not np.any(tri_pt[c])
        elif r["decided_tri"]:
            assert bool(tri_ok[c]) == r["tri_ok"], (c, r)
            if r["solved"] and r["unit"] == 0:
                assert np.array_equal(tri_pt[c], r["p"])     # both centres and the point at the origin: nothing to round
            elif r["solved"]:
                worst = max(worst, float(np.abs(tri_pt[c] - r["p"]).max()) / r["unit"])
            else:
                assert not np.any(tri_pt[c]), c              # no point written unless solved
        undecided += (not r["decided_rep"]) + (not r["decided_tri"])
    assert cap(undecided, len(model)), undecided
    assert worst <= C_C, worst
    return worst, undecided


def check_scores(case, model, num_inliers, mask0):
    """part D: num_inliers [H] of the given poses, mask0 the inlier flags of pose pair 0.  -> undecided (hypothesis, point) pairs"""
    undecided = 0
    for h, row in enumerate(model):
        dec = G.score_decided(case, row)
        inl = np.array([r[0] for r in row])
        assert abs(int(num_inliers[h]) - int((inl & dec).sum())) <= int((~dec).sum()) and int(num_inliers[h]) >= int((inl & dec).sum()), h
        assert cap(int((~dec).sum()), max(len(row), 100))
        undecided += int((~dec).sum())
        if h == 0:
            assert np.array_equal(np.asarray(mask0, dtype=bool)[dec], inl[dec])
            assert dec[:case["band"]].all()
    return undecided


def check_steps(call, model, poses_out, final_cost):
    """part E.  -> (worst step error in units of kappa 2^-53 |delta|_inf, worst cost error over cost0)"""
    worst, worst_cost = 0.0, 0.0
    for h, r in enumerate(model):
        x0 = call["inits"][h if call["per_task"] else 0]
        assert r["valid"] and r["rho"] > 0.1 and r["step_ratio"] > 100 and r["cost_ratio"] > 100 and r["gmax"] > 1e-8
        got = poses_out[h].reshape(12)
        dmax = float(max(abs(v) for v in r["delta"]))
        err = max(max(0.0, abs(float(M(float(got[a])) - M(float(x0[a])) - r["delta"][a])) - 2 * np.spacing(abs(got[a]))) for a in range(12))
        worst = max(worst, err / (r["kappa"] * EPS * dmax))
        if call["shutter"] == GLOBAL:
            assert got[6:].tobytes() == np.asarray(x0[6:], dtype=np.float64).tobytes()     # no Jacobian: bitwise where it started
        worst_cost = max(worst_cost, abs(float(M(float(final_cost[h])) - r["cost1"])) / float(r["cost0"]))
    assert worst <= C_TOL, worst
    assert worst_cost <= C_E, worst_cost
    return worst, worst_cost


# ============================================================ the oracle as a backend ============================================================
def oracle_reproject(oracle, case):
    out = [oracle.reproject(cam, poses, case["shutter"], case["scan"], X, 1.0, case["interp"]) for cam, poses, X in case["items"]]
    return np.array([xy for _, xy in out]), np.array([ok for ok, _ in out])


def oracle_validate(oracle, case):
    return np.array([oracle.validate_obs(cam, poses, case["shutter"], case["scan"], X, obs, case["thr"], case["min_dist"], case["interp"])
                     for cam, poses, X, obs in case["items"]])


def oracle_pose(oracle, case, f, xy):
    P = case["fposes"][f]
    if len(P) == 1:
        return P[0].copy()
    if len(P) == 2:
        return oracle.interpolate_rs(P[0], P[1], case["shutter"], case["scan"], xy, case["interp"])
    return P[oracle.scanline_pose_index(len(P), case["shutter"], xy)].copy()


def oracle_tracks(oracle, case):
    """the candidate pass composed of the oracle's scalar pieces"""
    n = len(case["ca"])
    tri_ok, tri_pt, rep_ok = np.zeros(n, dtype=bool), np.zeros((n, 3)), np.zeros(n, dtype=bool)
    obs = []
    for f, xy in zip(case["of"], case["oxy"]):
        cam, pose = case["cams"][case["fcam"][f]], oracle_pose(oracle, case, f, xy)
        obs.append((cam, pose, xy) + oracle.direction_pixel(cam, pose, xy))
    for c in range(n):
        (cama, pa, xa, oka, da), (camb, pb, xb, okb, db) = obs[case["ca"][c]], obs[case["cb"][c]]
        rq = int(case["request"][c])
        if rq & 2:
            X = case["track_pt"][c]
            rep_ok[c] = not (oracle.norm3(pa[3:] - X) < case["min_dist"]) and oracle.validate(cama, pa, xa, X, case["thr"])
        if rq & 1 and pa.tobytes() != pb.tobytes() and oka and okb:
            solved, p = oracle.triangulate(pa[3:], da, pb[3:], db)
            if solved:
                tri_pt[c] = p
                tri_ok[c] = (not (oracle.norm3(pa[3:] - p) < case["min_dist"]) and not (oracle.norm3(pb[3:] - p) < case["min_dist"])
                             and oracle.validate(cama, pa, xa, p, case["thr"]) and oracle.validate(camb, pb, xb, p, case["thr"]))
    return tri_ok, tri_pt, rep_ok


def oracle_scores(oracle, case):
    out = [oracle.pnp_task(G.CAM, case["shutter"], case["scan"], case["X"], case["xy"], case["subs"][h], case["inits"][h], 0, case["thr"])
           for h in range(len(case["inits"]))]
    assert all(np.array_equal(o["poses"].reshape(12), case["inits"][h]) for h, o in enumerate(out))
    return np.array([o["num_inliers"] for o in out]), out[0]["mask"]


def oracle_steps(oracle, call):
    out = [oracle.pnp_task(G.CAM, call["shutter"], call["scan"], call["X"], call["xy"], call["subs"][h], call["inits"][h if call["per_task"] else 0], 1, 8.0)
           for h in range(len(call["subs"]))]
    return np.array([o["poses"] for o in out]), np.array([o["final_cost"] for o in out])


# ================================================================== the tests ==================================================================
def test_scan_line_index_rounds_halves_away_from_zero_and_clamps():
    idx = lambda v, n=33: G.scanline_index(M(v), n)[0]
    assert [idx(v) for v in (-3.0, 0.0, 0.49, 0.5, 1.5, 2.5, 31.5, 32.49, 40.0)] == [0, 0, 0, 1, 2, 3, 32, 32, 32]
    poses = [mpv([0, 0, 0, k, 0, 0]) for k in range(5)]
    assert G.get_pose(poses, HORIZONTAL, (0, 4), mpv([2.5, 0.2]))[0][3] == 3 and G.get_pose(poses, VERTICAL, (0, 4), mpv([2.5, 0.2]))[0][3] == 0
    assert G.get_pose(poses, GLOBAL, (0, 4), mpv([0.2, 3.6]))[0][3] == 4                       # y unless HORIZONTAL, a GLOBAL session included
    two = [mpv([0.125, 0, 0, 0, 0, 0]), mpv([0.375, 0, 0, 2, 0, 0])]
    assert G.get_pose(two, VERTICAL, (0, 100), mpv([75.0, 25.0]), True)[0] == mpv([0.1875, 0, 0, 0.5, 0, 0])
    assert G.get_pose(two, HORIZONTAL, (100, 0), mpv([75.0, 25.0]), False)[0] == mpv([0.125, 0, 0, 0.5, 0, 0])
    assert G.get_pose(two, HORIZONTAL, (0, 100), mpv([175.0, 25.0]), True)[0][3] == 2 and G.get_pose(two, GLOBAL, (0, 100), mpv([75.0, 25.0]))[0][3] == 0


def test_the_gate_and_the_ungated_projection():
    cam, pose = mpv(G.CAM), mpv(np.zeros(6))
    assert not G.w2i(cam, pose, mpv([0.1, 0.1, 0.9e-8]))[0] and G.w2i(cam, pose, mpv([0.1, 0.1, 1.1e-8]))[0]
    ok, xy, z = G.w2i(cam, pose, mpv([1.0, 0.5, -5.0]), gate=False)
    assert ok and z == -5 and xy[0] < 640 and xy[1] < 360                # mirrored through the centre, not refused
    assert G.w2i(cam, pose, mpv([0.0, 0.0, 3.0]))[1] == [640, 360]


@pytest.mark.parametrize("scale", [1, 8, 12])
def test_the_replayed_undistortion_is_an_undistortion(scale):
    """the replay lands within L / (1 - L) * tol of the Newton inverse of distort (the a-posteriori bound of a contraction whose
    last step was shorter than tol)"""
    cam = mpv(G.scaled_cam(scale))
    rng = np.random.default_rng(scale)
    checked = 0
    for xy in rng.uniform([0, 0], [1280, 720], (80, 2)):
        pn = [(M(float(xy[0])) - cam[7]) / cam[0], (M(float(xy[1])) - cam[8]) / cam[1]]
        u = G.undistort_replay(cam, pn)
        if not u["ok"] or u["L"] >= 1:
            continue
        inv = G.undistort_newton(cam, pn)
        back = G.distort(cam, inv)
        assert abs(back[0] - pn[0]) + abs(back[1] - pn[1]) < M("1e-40")
        assert G.norm([u["p"][0] - inv[0], u["p"][1] - inv[1]]) <= u["L"] / (1 - u["L"]) * u["tol"] * M("1.001")
        checked += 1
    assert checked >= 40


def test_the_midpoint_is_the_least_squares_point_of_the_two_rays():
    rng = np.random.default_rng(0)
    c1, c2 = mpv(rng.normal(0, 1, 3)), mpv(rng.normal(0, 1, 3))
    X = mpv([0.3, -0.2, 7.0])
    a = [x / G.norm([X[i] - c1[i] for i in range(3)]) for x in [X[i] - c1[i] for i in range(3)]]
    b = [x / G.norm([X[i] - c2[i] for i in range(3)]) for x in [X[i] - c2[i] for i in range(3)]]
    p, det, cond = G.triangulate(c1, a, c2, b)
    assert max(abs(p[i] - X[i]) for i in range(3)) < M("1e-40")
    cosang = sum(x * y for x, y in zip(a, b))
    assert abs(det - 2 * (1 - cosang ** 2)) < M("1e-40") and abs(cond - float(2 / (1 - abs(cosang)))) < 1e-9 * cond


# ---- part A ----
@pytest.mark.parametrize("key", G.A_HANDLE, ids=str)
def test_oracle_reproject_through_the_session_inputs(oracle, key):
    case, model = G.reproject_handle_case(*key), G.reproject_model(G.reproject_handle_case, *key)
    worst, undecided = check_reproject(case, model, *oracle_reproject(oracle, case))
    print(f"reproject {key}: worst {worst:.2f}, undecided {undecided}")
    shutter, _, n, scan = key
    if n > 1:
        assert sum(r["reason"] == "gate" for r in model) >= 3 and sum(r["ok"] for r in model) >= n // 3
    if shutter != GLOBAL and n > 1:
        by_limit = [r for r, s in zip(model, case["sep"]) if r["reason"] == "limit"]
        assert all(r["zmin"] > 1.0 for r in by_limit)                                       # by the limit alone: z far from its gate
        assert scan[0] > scan[1] or sum(s >= 13 for r, s in zip(model, case["sep"]) if r["reason"] == "limit") >= 20
        # tau clamped on both sides among the converged items
        line = np.array([float(r["xy"][1 if shutter == VERTICAL else 0]) for r in model if r["ok"]])
        assert (line < min(scan)).sum() >= 3 and (line > max(scan)).sum() >= 3
        for sep, lo, hi in ((0.35, 0.01, 0.06), (5.0, 0.3, 0.6), (10.0, 0.6, 1.1)):
            if scan[0] < scan[1]:
                assert lo < max(r["L"] for r, s in zip(model, case["sep"]) if s == sep and r["ok"]) < hi


@pytest.mark.parametrize("key", G.A_FRAME, ids=str)
def test_oracle_reproject_through_the_frame_inputs(oracle, key):
    case, model = G.reproject_frame_case(*key), G.reproject_model(G.reproject_frame_case, *key)
    worst, undecided = check_reproject(case, model, *oracle_reproject(oracle, case))
    print(f"reproject_frame {key}: worst {worst:.2f}, undecided {undecided}")
    if key[0] in ("two", "edge"):
        assert sum(r["reason"] == "limit" and r["zmin"] > 1.0 for r in model) >= 20
    if key[0] == "edge":
        assert sum(r["ok"] and r["steps"] == 49 for r in model) >= 10                      # the last projection the limit allows


def test_the_reprojection_bound_is_tighter_than_the_old_one():
    for fn, keys in ((G.reproject_handle_case, G.A_HANDLE), (G.reproject_frame_case, G.A_FRAME)):
        for key in keys:
            for (cam, _, _), r in zip(fn(*key)["items"], G.reproject_model(fn, *key)):
                if r["ok"]:
                    top = float(max(abs(v) for v in r["xy"]))
                    assert C_A * EPS * (top + cam[0] + cam[1]) * r["amp"] < 0.01 * 1e-9 * max(1.0, top)


def test_a_reprojection_that_stops_at_1e_3_is_seen():
    key = (HORIZONTAL, True, 600, (17, 1203))
    case, model = G.reproject_handle_case(*key), G.reproject_model(G.reproject_handle_case, *key)
    wrong = G.reproject_model(G.reproject_handle_case, *key, stop=M("1e-3"))
    over = [mp_inf(G.fl(w["xy"]), r["xy"]) / (C_A * EPS * (float(max(abs(v) for v in r["xy"])) + 1600.0) * r["amp"])
            for r, w, s in zip(model, wrong, case["sep"]) if r["ok"] and w["ok"] and s in (5.0, 10.0) and r["L"] > 0.1]
    assert len(over) >= 50 and np.mean(np.array(over) >= 100) >= 0.5 and np.median(over) >= 1e4, (len(over), np.median(over))


def test_a_reprojection_limit_one_larger_is_seen():
    key = ("edge", HORIZONTAL, 255)
    model, wrong = G.reproject_model(G.reproject_frame_case, *key), G.reproject_model(G.reproject_frame_case, *key, limit=51)
    limit_items = [i for i, r in enumerate(model) if r["reason"] == "limit" and G.decided(r["margins"], **RULE_A)]
    flips = sum(wrong[i]["ok"] for i in limit_items)
    assert len(limit_items) >= 20 and flips >= max(2, len(limit_items) // 20), (flips, len(limit_items))


# ---- part B ----
def both_outcomes(case, model):
    flag = np.array([f for f, _, _ in model])
    near = np.array([m["dist"] != G.INF and e2 is not None and not f and e2 < case["thr"] for f, m, e2 in model])   # refused by the distance alone
    off = np.array([e2 is not None and e2 >= case["thr"] for _, _, e2 in model])                                   # refused by the error
    return flag.mean(), near.mean(), off.mean()


@pytest.mark.parametrize("key", G.B_HANDLE, ids=str)
def test_oracle_validate_through_the_session_inputs(oracle, key):
    case, model = G.validate_handle_case(*key), G.validate_model(G.validate_handle_case, *key)
    undecided = check_validate(case, model, oracle_validate(oracle, case))
    print(f"validate {key}: undecided {undecided}")
    good, near, off = both_outcomes(case, model)
    assert 0.2 <= good <= 0.8 and near >= 0.1 and off >= 0.1, (good, near, off)
    band = [m["err"] for (_, m, _), b in zip(model, case["band"]) if b]
    assert len(band) == 64 and 0.9 * 2.0 ** -20 < min(band) and max(band) < 1.1 * 2.0 ** -20
    assert sum(f for (f, _, _), b in zip(model, case["band"]) if b) == 32


@pytest.mark.parametrize("key", G.B_FRAME, ids=str)
def test_oracle_validate_through_the_scan_line_frames(oracle, key):
    case, model = G.validate_frame_case(*key), G.validate_model(G.validate_frame_case, *key)
    undecided = check_validate(case, model, oracle_validate(oracle, case))
    print(f"validate_frame {key}: undecided {undecided}")
    if key[1] > 1:
        good, near, off = both_outcomes(case, model)
        assert 0.2 <= good <= 0.8 and near >= 0.1 and off >= 0.1, (good, near, off)
        assert case["half"].sum() == 40


def test_floor_instead_of_round_is_seen_on_the_half_lines():
    for key in G.B_FRAME[:3]:
        case = G.validate_frame_case(*key)
        model, wrong = G.validate_model(G.validate_frame_case, *key), G.validate_model(G.validate_frame_case, *key, floor_index=True)
        dec = np.array([G.decided(m, **RULE_B) for _, m, _ in model]) & case["half"]
        flips = sum(model[i][0] != wrong[i][0] for i in np.flatnonzero(dec))
        assert dec.sum() >= 38 and flips >= dec.sum() // 2, (flips, dec.sum())


# ---- part C ----
@pytest.fixture(scope="module")
def tracks():
    return {key: G.tracks_model(G.tracks_case(*key), C_C) for key in G.C_CASES}


@pytest.mark.parametrize("key", G.C_CASES, ids=str)
def test_oracle_track_candidates(oracle, tracks, key):
    case, (model, obs) = G.tracks_case(*key), tracks[key]
    worst, undecided = check_tracks(case, model, *oracle_tracks(oracle, case))
    print(f"track_candidates {key}: worst {worst:.2f}, undecided {undecided}")
    if key[3] > 1:
        solved = [r for r in model if r["solved"]]
        assert min(r["det"] for r in solved) < 2.5e-9 and max(r["cond"] for r in solved) > 3e9
        for ang in G.ANGLES[1:]:
            assert sum(r["solved"] and r["decided_tri"] for r, a in zip(model, case["angle"]) if a == ang) >= 10
        assert sum(r["tri_ok"] for r in model) >= 50 and sum(r["solved"] and not r["tri_ok"] for r in model) >= 15
        assert sum(r["reproj_ok"] for r in model) >= 50
        assert sum(not r["solved"] for r, q in zip(model, case["request"]) if q & 1) >= 5     # equal poses, one frame twice
        assert max(o["u"]["steps"] for o in obs) >= 25
        # bitwise-equal poses are skipped; poses that differ by the sign of a zero are solved, and the point (their centre) is written
        fa, fb = case["of"][case["ca"]], case["of"][case["cb"]]
        tri = (case["request"] & 1) > 0
        assert sum(not r["solved"] for r, a, b, t in zip(model, fa, fb, tri) if t and {a, b} == {0, 1}) >= 2
        assert sum(r["solved"] and r["decided_tri"] and np.all(r["p"] != 0) for r, a, b, t in zip(model, fa, fb, tri) if t and a != b and 2 in (a, b) and a < 3 and b < 3) >= 2


def test_the_strongest_distortions_crawl_and_fail(tracks):
    _, obs = tracks[G.C_CASES[0]]
    assert max(o["u"]["steps"] for o in obs if o["ray"] is not None) >= 50 and sum(o["ray"] is None for o in obs) >= 1


def test_triangulate_alone_on_exact_rays(oracle, tracks):
    """the oracle's cofactor solve fed the model's rays rounded to double: within 0.95 of cond 2^-53 scale down to det = 1.4e-9"""
    case, (model, obs) = G.tracks_case(*G.C_CASES[0]), tracks[G.C_CASES[0]]
    worst = 0.0
    for c, r in enumerate(model):
        if r["solved"] and r["unit"] > 0:
            a, b = obs[case["ca"][c]], obs[case["cb"][c]]
            ok, p = oracle.triangulate(G.fl(a["pose"][3:]), G.fl(a["ray"]), G.fl(b["pose"][3:]), G.fl(b["ray"]))
            assert ok
            worst = max(worst, float(np.abs(p - r["p"]).max()) / (r["unit"] / r["amp"]))
    print(f"triangulate alone: worst {worst:.2f}")
    assert worst <= 0.95


def test_an_undistortion_that_stops_one_step_early_is_seen(tracks):
    case, (model, _) = G.tracks_case(*G.C_CASES[0]), tracks[G.C_CASES[0]]
    wrong, _ = G.tracks_model(case, C_C, stop_early=1)
    over = [float(np.abs(w["p"] - r["p"]).max()) / r["bound"] for r, w in zip(model, wrong) if r["solved"] and w["solved"] and r["unit"] > 0]
    # (the pairs of frames that share a centre triangulate to that centre whatever their rays are: the few that do not move)
    assert len(over) >= 200 and np.median(over) >= 100 and np.mean(np.array(over) > 1) >= 0.9, (len(over), np.median(over), min(over))


def test_parallel_rays_are_undecided_by_design():
    case = G.parallel_case()
    model, _ = G.tracks_model(case, C_C)
    assert all(abs(r["det"]) < 1e-12 and not r["decided_tri"] for r in model)


# ---- part D ----
@pytest.mark.parametrize("key", G.D_CASES, ids=str)
def test_oracle_scores(oracle, key):
    case, model = G.score_case(*key), G.score_model(*key)
    undecided = check_scores(case, model, *oracle_scores(oracle, case))
    print(f"pnp scoring {key}: undecided {undecided}")
    inl = np.array([r[0] for r in model[0]])
    if key[1] > 1:
        assert 0.2 <= inl.mean() <= 0.8 and inl[:case["band"]].sum() == case["band"] // 2
        lim = 16 * 2.0 ** -24 * G.f32(case["thr"])
        assert all(0.9 * lim < r[1] < 1.1 * lim for r in model[0][:case["band"]])


def test_scoring_with_tau_from_x_under_a_vertical_shutter_is_seen():
    key = G.D_CASES[1]
    case, model, wrong = G.score_case(*key), G.score_model(*key)[0], G.score_model(*key, tau_from_x=True)[0]
    dec = G.score_decided(case, model)
    flips = sum(model[i][0] != wrong[i][0] for i in np.flatnonzero(dec))
    assert flips >= dec.sum() // 20, (flips, dec.sum())


# ---- part E ----
E_KEYS = [(s, H, m, False) for s in (HORIZONTAL, VERTICAL, GLOBAL) for H, m in G.E_CALLS] + [(s, 3, 6, True) for s in (HORIZONTAL, VERTICAL, GLOBAL)]


@pytest.mark.parametrize("key", E_KEYS, ids=str)
def test_oracle_first_step(oracle, key):
    call, model = G.step_call(*key), G.step_model(*key)
    worst, worst_cost = check_steps(call, model, *oracle_steps(oracle, call))
    print(f"LM step {key}: worst {worst:.3f} of kappa eps |delta| (kappa {min(r['kappa'] for r in model):.1e} - {max(r['kappa'] for r in model):.1e}), cost {worst_cost:.1e} of cost0")
    assert len({call["subs"][h].tobytes() for h in range(key[1])}) >= min(key[1], 2)


def step_error(model, wrong):
    return max(max(abs(float(w["delta"][a] - r["delta"][a])) for a in range(12)) / (C_TOL * r["kappa"] * EPS * float(max(abs(v) for v in r["delta"])))
               for r, w in zip(model, wrong))


def test_a_functor_with_tau_from_y_under_a_vertical_shutter_is_seen():
    key = (VERTICAL, 3, 6, True)
    assert step_error(G.step_model(*key), G.step_model(*key, tau_from_x_always=False)) >= 100


def test_a_clamp_without_its_lower_bound_is_seen_under_a_global_shutter():
    """the second pose has no Jacobian: without the 1e-6 its pivot is zero, the step invalid, the poses unmoved"""
    key = (GLOBAL, 3, 6, True)
    wrong = G.step_model(*key, clamp_lo=None)
    assert not any(w["valid"] for w in wrong) and step_error(G.step_model(*key), wrong) >= 100
