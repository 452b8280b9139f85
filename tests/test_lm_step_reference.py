"""The host reference of one LM step (tests/lm_step_reference.py) against the CPU oracle's first step, and proof that the tolerance
tests/test_gpu_lm_step.py puts on the device step would see a one-tile error of the reduced camera system.

The oracle solves by Schur elimination and an envelope Cholesky of the reduced system; the reference by a dense (or sparse LU)
factorisation of the whole damped system refined in long double.  They share no code, so agreement to a few kappa * eps on every
scene shape of tests/lm_step_cases.py checks both.  Measured here: error / (kappa eps |delta|_inf) <= 18 (the intrinsics scenes;
below 3 elsewhere), the model cost change to <= 1e-13 relative.  With prior blocks (lm_step_cases.PRIOR_CASES): <= 7.7 (motion
priors beside shared intrinsics), below 1.6 elsewhere; the sharded modes' problems (tests/test_distributed.py) <= 15.

The prior blocks' closed forms are checked against mpmath (50 digits, central differences), and three errors a device could make
in them are shown to exceed the device tolerance: one prior's (f, f - 1) coupling missing from the reduced system, a 1e-9 error in
the free ratio's border column, and the priorPoses elimination without the block's LM diagonal."""
import numpy as np
import pytest

import mpmath

import lm_step_cases as LC
import lm_step_reference as R
from helpers import load_golden

C_TOL = 64          # (measured: oracle <= 18, device <= 1.5) the tolerance of the device step: |delta_gpu - delta_ref|_inf <= C_TOL * kappa * 2^-53 * |delta_ref|_inf (+ rounding)


def reference(oracle, name):
    p, opts = LC.case(name)
    r, J, ok = oracle.evaluate_blocks(p)
    assert ok.all()
    ref = R.lm_step(p, r, J, **{k: opts[k] for k in ("initial_trust_region_radius",) if k in opts})
    return p, opts, ref


def test_huber_rho_matches_the_goldens():
    for c in load_golden("huber.json"):
        rho = R.huber_rho(c["a"], np.array([c["s"]]))
        assert np.allclose([v[0] for v in rho], c["rho"], rtol=1e-15, atol=0.0), c


@pytest.mark.parametrize("name", LC.CASES + LC.PRIOR_CASES)
def test_reference_step_matches_the_oracles_first_step(oracle, name):
    p, opts, ref = reference(oracle, name)
    assert ref.kappa <= 1e9, ref.kappa
    assert ref.refinement[-1] <= 1e-16, ref.refinement          # the refined residual sits far below fp64 kappa * eps
    q = p.copy()
    s, tr = oracle.solve(q, oracle.default_options(**opts))
    assert len(tr) == 2 and tr[1].step_is_successful == 1         # a precondition of the case: the step is applied
    ratio, where = R.step_ratio(p, ref, *R.solved_blocks(q))
    print(f"{name}: step ratio {ratio:.3f} at {where}, kappa {ref.kappa:.2e}")
    assert ratio <= C_TOL, (ratio, where, ref.kappa)
    assert abs(tr[1].model_cost_change - ref.model_cost_change) <= 1e-12 * ref.model_cost_change
    nrm, allowed = R.step_norm_bound(p, ref, C_TOL)
    assert abs(tr[1].step_norm - nrm) <= allowed, (tr[1].step_norm, nrm, allowed)
    assert abs(tr[0].gradient_max_norm - ref.gradient_max_norm) <= 1e-13 * ref.gradient_max_norm
    # fixed coordinates and blocks outside the program do not move
    assert np.all(ref.poses[np.unpackbits(p.pose_fixed_mask[..., None], axis=-1, bitorder="little")[..., :6].astype(bool)] == 0)
    assert np.array_equal(q.poses[ref.poses == 0], p.poses[ref.poses == 0])


def _reduced(p, ref):
    """The reduced camera system of the reference's matrix: S, its solution, and the pieces for back-substitution."""
    H = ref.H.astype(np.float64).toarray()
    y = ref.y.astype(np.float64)
    cam = ref.free < ref.ncam
    c, q = np.flatnonzero(cam), np.flatnonzero(~cam)
    Hpp_inv = np.linalg.inv(H[np.ix_(q, q)])
    S = H[np.ix_(c, c)] - H[np.ix_(c, q)] @ Hpp_inv @ H[np.ix_(q, c)]
    CD = 6 * p.poses_per_frame
    tile = np.where(ref.free[c] < p.num_frames * CD, ref.free[c] // CD // (48 // CD), -1)   # 48 x 48 tiles of FT frames

    def moved(dS):
        """|delta' - delta|_inf when S becomes S + dS (exactly: (S + dS) dy = -dS y, then the points' back-substitution)."""
        dyc = np.linalg.solve(S + dS, -dS @ y[c])
        dy = np.zeros(len(y))
        dy[c], dy[q] = dyc, -Hpp_inv @ H[np.ix_(q, c)] @ dyc
        return float(np.max(np.abs(ref.scale * dy)))
    return H, S, c, q, tile, moved


@pytest.mark.parametrize("name", ["rs_far_pair", "gs_far_pair"])
def test_the_tolerance_sees_a_one_tile_error(oracle, name):
    """A 1e-9 relative error in ONE 48 x 48 off-diagonal tile of the reduced system, or one point's contribution missing from one
    tile pair, moves delta by more than the device test's tolerance (measured: 47x - 250x, and 1e8x, of it)."""
    p, _, ref = reference(oracle, name)
    H, S, c, q, tile, moved = _reduced(p, ref)
    tol = C_TOL * ref.kappa * R.EPS * R.delta_inf(ref)
    for I, J in ((2, 1), (3, 1)):
        a, b = np.flatnonzero(tile == I), np.flatnonzero(tile == J)
        assert len(a) == len(b) == 48 and np.count_nonzero(S[np.ix_(a, b)]) == 48 * 48
        dS = np.zeros_like(S)
        dS[np.ix_(a, b)] = 1e-9 * S[np.ix_(a, b)]
        dS[np.ix_(b, a)] = dS[np.ix_(a, b)].T
        assert moved(dS) > 10 * tol, (I, J, moved(dS), tol)
    # the smallest single-point contribution to tile pair (2, 1)
    a, b = np.flatnonzero(tile == 2), np.flatnonzero(tile == 1)
    pt_of = (ref.free[q] - ref.ncam) // 3
    smallest = None
    for j in np.unique(pt_of):
        qj = q[pt_of == j]
        Wa, Wb = H[np.ix_(c[a], qj)], H[np.ix_(c[b], qj)]
        if np.any(Wa) and np.any(Wb):
            C = Wa @ np.linalg.inv(H[np.ix_(qj, qj)]) @ Wb.T
            if smallest is None or np.max(np.abs(C)) < np.max(np.abs(smallest)):
                smallest = C
    assert smallest is not None
    dS = np.zeros_like(S)
    dS[np.ix_(a, b)] = smallest          # S = U - sum_j W_j V_j^-1 W_j^T: dropping point j's term adds it back
    dS[np.ix_(b, a)] = smallest.T
    assert moved(dS) > 10 * tol, (moved(dS), tol)


def test_the_bound_case_projects_the_ratio(oracle):
    """rs_vel_free_bound: the model step takes the ratio below 0; the candidate sits on the bound, step_norm counts the projected
    move, model_cost_change the model step."""
    p, _, ref = reference(oracle, "rs_vel_free_bound")
    x0 = p.inter_frame_ratio
    assert x0 + ref.ratio[0] < 0.0 and ref.apply(p)["ratio"][0] == 0.0
    d = ref.delta()
    d[R.layout(p)["iratio"]] = -x0                                        # the projected move of the ratio
    assert abs(ref.step_norm - np.linalg.norm(d)) <= 1e-14 * ref.step_norm
    assert abs(ref.step_norm - np.linalg.norm(ref.delta())) > 1e-3 * ref.step_norm


def test_one_pose_frames_keep_their_second_slot_out_of_the_system():
    """frame_global: the second slot of a one-pose frame is data — no Jacobian entry refers to it and it is not an unknown."""
    p, _ = LC.case("rs_scanline_priors")
    gcol, ncam, nparam, fixed = R.columns(p)
    glob = np.flatnonzero(p.frame_global)
    slot2 = (glob[:, None] * 12 + 6 + np.arange(6)[None, :]).reshape(-1)
    assert len(glob) == 3 and fixed[slot2].all()
    assert not np.isin(gcol, slot2).any()
    for _, _, g, _ in R.prior_blocks(p):
        assert not np.isin(g, slot2).any()
    q = p.copy(); q.pose_fixed_mask[glob, 1] = 0                        # even without the caller's mask
    assert R.columns(q)[3][slot2].all()


# ---- the prior blocks' closed forms against mpmath ------------------------------------------------------------------------------

mp = mpmath.mp


def _mp_motion(kind, scale, t, a, b, c, d):
    """The motion priors from their meaning, in mpmath: the frame's first pose against the previous frame's last pose moved on
    over the gap (gap = ratio x exposure), the frame's last pose against its first pose moved on over the exposure — at the previous
    velocity (kind 1; its second half at the previous frame's velocity when ratio <= eps) or at the mean of the previous and the
    current one (kind 2); rotation rows x 0.01, all x scale."""
    out = []
    for half in (0, 1):
        for i in range(6):
            if kind == 1 and half == 0:
                v = a[i] - (d[i] + t * (d[i] - c[i]))
            elif kind == 1:
                v = b[i] - (a[i] + ((a[i] - d[i]) / t if t > R.DBL_EPSILON else (d[i] - c[i])))
            elif half == 0:
                prev, now = t * (d[i] - c[i]), a[i] - d[i]
                v = a[i] - (d[i] + prev + (now - prev) / 2)
            else:
                prev, now = (a[i] - d[i]) / t, b[i] - a[i]
                v = b[i] - (a[i] + prev + (now - prev) / 2)
            out.append(v * scale * (mpmath.mpf("0.01") if i < 3 else 1))
    return out


def _mp_jacobian(fun, x, h=mpmath.mpf("1e-25")):
    cols = []
    for k in range(len(x)):
        xp, xm = list(x), list(x)
        xp[k] += h; xm[k] -= h
        cols.append([(u - v) / (2 * h) for u, v in zip(fun(xp), fun(xm))])
    return [[cols[k][i] for k in range(len(x))] for i in range(len(cols[0]))]


def _close(got, want, rtol):
    got = np.asarray(got, dtype=np.longdouble).astype(np.float64)
    want = np.array([[float(v) for v in row] for row in want]) if isinstance(want[0], list) else np.array([float(v) for v in want])
    scale = max(float(np.max(np.abs(want))), 1e-300)
    assert np.max(np.abs(got - want)) <= rtol * scale, (np.max(np.abs(got - want)) / scale)


@pytest.mark.parametrize("kind,t", [(1, 0.8), (1, 2.5), (1, 0.0), (1, 1e-17), (1, 3e-16), (2, 0.8), (2, 1.25), (2, 1e-3)])
def test_motion_prior_jacobians_against_mpmath(kind, t):
    rng = np.random.default_rng(7)
    a, b, c, d = rng.normal(size=(4, 6))
    scale = 7.0
    with mp.workdps(50):
        x = [mpmath.mpf(float(v)) for v in np.concatenate([a, b, c, d, [t]])]
        fun = lambda x: _mp_motion(kind, scale, x[24], x[0:6], x[6:12], x[12:18], x[18:24])   # noqa: E731
        r_mp, J_mp = fun(x), _mp_jacobian(fun, x)
    r, J = R.motion_prior_jacobian(kind, scale, t, a, b, c, d)
    _close(r[0], r_mp, 1e-17)
    _close(J[0], J_mp, 1e-17)
    if kind == 1 and t <= R.DBL_EPSILON:                       # the second half does not depend on the ratio there
        assert np.all(J[0, 6:, 24] == 0)


def test_pose_prior_jacobians_against_mpmath():
    rng = np.random.default_rng(8)
    prior, pose = rng.normal(size=(2, 6)) * 0.1
    with mp.workdps(50):
        x = [mpmath.mpf(float(v)) for v in np.concatenate([prior, pose])]
        W = [3, 3, 3, 5, 5, 5]
        fun = lambda x: [W[i] * (x[i] - x[6 + i]) for i in range(6)]   # noqa: E731
        r_mp, J_mp = fun(x), _mp_jacobian(fun, x)
    r, J = R.good_pose_prior(3.0, 5.0, prior, pose)
    _close(r[0], r_mp, 1e-17)
    _close(J[0], J_mp, 1e-17)


@pytest.mark.parametrize("signs", [(1, 1, 1), (-1, 1, -1), (1, -1, -1)])
def test_spherical_prior_jacobians_against_mpmath(signs):
    pose = np.array([0.1, -0.2, 0.05, 1e-4, 2e-4, 3e-4]) * np.array([1, 1, 1, *signs])
    with mp.workdps(60):
        x = [mpmath.mpf(float(v)) for v in pose]
        fun = lambda x: [x[0] ** 2 + x[1] ** 2 + x[2] ** 2, mpmath.mpf(10) ** 20 * (1 - abs(x[3]) - abs(x[4]) - abs(x[5]))]   # noqa: E731
        r_mp, J_mp = fun(x), _mp_jacobian(fun, x, h=mpmath.mpf("1e-30"))
    r, J = R.spherical_prior(pose)
    _close(r[0], r_mp, 1e-17)
    _close(J[0][0], J_mp[0], 1e-17)
    _close(J[0][1], J_mp[1], 1e-17)


# ---- sensitivity: errors in the prior terms that the device tolerance must see ----------------------------------------------------

def _moved(oracle, p, opts, ref, edit):
    """|delta' - delta|_inf when the reference's scaled, damped matrix is edited, and the device tolerance."""
    r, J, ok = oracle.evaluate_blocks(p)
    other = R.lm_step(p, r, J, want_kappa=False, edit=edit, **{k: opts[k] for k in ("initial_trust_region_radius",) if k in opts})
    tol = C_TOL * ref.kappa * R.EPS * R.delta_inf(ref)
    return float(np.max(np.abs(other.delta() - ref.delta()))), tol


@pytest.mark.parametrize("name,f", [("rs_acc_r1.25", 4), ("rs_acc_r1.25", 5), ("rs_free_huber", 8)])
def test_the_tolerance_sees_a_missing_prior_coupling(oracle, name, f):
    """Prior f's share of the (f, f - 1) block of the reduced system left out (f = FT: the block crosses a tile edge)."""
    p, opts, ref = reference(oracle, name)
    k = int(np.flatnonzero(p.prior_frames == f)[0])
    rp, Jp, g, _ = R.prior_blocks(p)[0]
    _, Jc = R.corrected(float(p.huber_a), rp.astype(np.float64)[k:k + 1], Jp.astype(np.float64)[k:k + 1])

    def edit(H, free, scale):
        pos = {int(c): i for i, c in enumerate(free)}
        H = H.tolil()
        for a in range(12):                       # columns of frame f
            for b in range(12, 24):               # columns of frame f - 1
                ia, ib = pos.get(int(g[k, a])), pos.get(int(g[k, b]))
                if ia is None or ib is None:
                    continue
                v = np.longdouble(scale[ia] * scale[ib] * float(Jc[0, :, a] @ Jc[0, :, b]))
                H[ia, ib] -= v
                H[ib, ia] -= v
        return H.tocsr()
    moved, tol = _moved(oracle, p, opts, ref, edit)
    print(f"{name} prior {f}: moved {moved:.3e}, tolerance {tol:.3e}, ratio {moved / tol:.3g}")
    assert moved > 10 * tol, (moved, tol)


@pytest.mark.parametrize("name", ["rs_vel_free", "rs_acc_free", "rs_free_huber"])
def test_the_tolerance_sees_a_ratio_border_error(oracle, name):
    """A 1e-9 relative error in the free ratio's border column of the system (every off-diagonal entry).  (Measured: 2x - 290x the
    tolerance.  It is the least sharp of these checks: on the 7-tile rs_prior_nt the same error moves delta by 0.9x the tolerance.)"""
    p, opts, ref = reference(oracle, name)
    ir = int(np.flatnonzero(ref.free == R.layout(p)["iratio"])[0])

    def edit(H, free, scale):
        H = H.tolil()
        row = H.getrow(ir)
        for j, v in zip(row.indices, row.data):
            if j != ir:
                H[ir, j] = v * np.longdouble(1 + 1e-9)
                H[j, ir] = H[ir, j]
        return H.tocsr()
    moved, tol = _moved(oracle, p, opts, ref, edit)
    print(f"{name} ratio border: moved {moved:.3e}, tolerance {tol:.3e}, ratio {moved / tol:.3g}")
    assert moved > tol, (moved, tol)


@pytest.mark.parametrize("name", ["rs_pp_all", "gs_pp_some", "rs_spherical_all"])
def test_the_tolerance_sees_a_prior_pose_elimination_without_its_diagonal(oracle, name):
    """The device eliminates each priorPoses coordinate in closed form: S_xx -= c^2 / V0' with V0' = V0 + D0 its damped diagonal.
    With c^2 / V0 instead (no LM diagonal), S_xx changes by c^2 / V0' - c^2 / V0: that changed S, the same back-substitution."""
    p, opts, ref = reference(oracle, name)
    L = R.layout(p)
    radius = opts.get("initial_trust_region_radius", 1e4)

    def edit(H, free, scale):
        H = H.tolil()
        for i in np.flatnonzero((free >= L["ipp"]) & (free < L["ipp"] + 6 * len(p.pose_prior_block))):
            row = H.getrow(i)
            tied = [j for j in row.indices if j != i]               # the pose coordinate it is tied to (W is diagonal), if that is free
            if not tied:
                continue
            (x,) = tied
            Vd = H[i, i]
            V0 = Vd / (1 + np.longdouble(1.0) / np.longdouble(radius))   # (V0 is inside [1e-6, 1e32]: D0 = V0 / radius)
            c = H[i, x]
            H[x, x] += c * c / Vd - c * c / V0
        return H.tocsr()
    moved, tol = _moved(oracle, p, opts, ref, edit)
    print(f"{name} priorPoses without D0: moved {moved:.3e}, tolerance {tol:.3e}, ratio {moved / tol:.3g}")
    assert moved > 10 * tol, (moved, tol)


# ---- pose covariance: the (frame, frame) blocks of (J^T J)^-1 ----------------------------------------------------------------------

# The unit of a covariance comparison is u_ab = kappa^ * 2^-53 * sqrt(C_aa C_bb): kappa^ the condition number of the symmetrically
# scaled J^T J, C the reference block (lm_step_reference.covariance_blocks: the whole unscaled, undamped J^T J, factored once, every
# column refined in long double — its own error is below 2e-3 of the unit).  Measured in that unit: the CPU oracle (Schur elimination,
# dense fp64 Cholesky) <= 1.98 over LC.COV_CASES (rs_const_points; rs_const_frame 1.85, below 0.85 elsewhere);
# tests/test_gpu_covariance.py has the tables.  C_COV is the smallest power of two >= 4 x the larger of the oracle's and the device's
# worst ratio — the margin C_TOL = 64 has over the oracle's 18 on the LM step: 4 x 1.98 = 7.9 -> 8.
C_COV = 8

_cov_cache = {}


def covariance_reference(oracle, name):
    """(problem, frames asked, reference) of a covariance case; one factorisation per case and session."""
    if name not in _cov_cache:
        p = LC.cov_case(name)
        r, J, ok = oracle.evaluate_blocks(p)
        assert ok.all()
        frames = LC.cov_frames(p)
        _cov_cache[name] = (p, frames, R.covariance_blocks(p, r, J, frames))
    return _cov_cache[name]


def covariance_worst(ref, blocks):
    """Worst ratio of {frame: block} against the reference, the asymmetry |got - got^T| in the same unit included."""
    return max(max(R.covariance_ratio(ref, f, c), R.covariance_asymmetry(ref, f, c)) for f, c in blocks.items())


@pytest.mark.parametrize("name", LC.COV_CASES)
def test_oracle_covariance_is_within_the_bound(oracle, name):
    p, frames, ref = covariance_reference(oracle, name)
    assert ref.ok and ref.error <= 2.0 ** -6, (ref.error, ref.refinement)
    got = {}
    for f in frames:
        got[f], ok = oracle.pose_covariance(p, f)
        assert ok
        assert np.array_equal(ref.blocks[f] != 0, np.outer(ref.free[f], ref.free[f]))    # free coordinates couple, the others are zero
    worst = covariance_worst(ref, got)
    print(f"{name}: oracle covariance ratio {worst:.3f}, kappa^ {ref.kappa:.2e}, refinement {ref.refinement}, reference error {ref.error:.1e}")
    assert worst <= C_COV, (worst, ref.kappa)
    if p.frame_global is not None:                   # the second slot of a one-pose frame is data
        f = int(np.flatnonzero(p.frame_global)[0])
        assert f in frames and not ref.free[f][6:].any() and ref.free[f][:6].all()


@pytest.mark.parametrize("name", LC.COV_REFUSED)
def test_rank_deficient_covariance_is_refused(oracle, name):
    """Points seen once (rs_F1, rs_single_view), the SphericalPrior (1e20 on three coordinates), no gauge fixed: no covariance."""
    p, _, ref = covariance_reference(oracle, name)
    assert not ref.ok
    if name != "free_gauge":                         # (the oracle's Cholesky gets through the free gauge's rounding-sized pivots)
        assert not oracle.pose_covariance(p, min(1, p.num_frames - 1))[1]


def _seeded(oracle, name, frames, **kw):
    """Worst ratio, over ``frames``, of a reference computed WITH a seeded error against the reference itself; and of the reference
    computed again without it (0: the expectation fails without the error)."""
    p = LC.cov_case(name)
    r, J, ok = oracle.evaluate_blocks(p)
    ref = R.covariance_blocks(p, r, J, frames)
    wrong = kw.pop("wrong", None)
    other = wrong(p, r, J) if wrong else R.covariance_blocks(p, r, J, frames, **kw)
    assert ref.ok and other.ok
    again = R.covariance_blocks(p, r, J, frames)
    as64 = lambda c: {f: c.blocks[f].astype(np.float64) for f in frames}   # noqa: E731
    return covariance_worst(ref, as64(other)), covariance_worst(ref, as64(again)), ref


@pytest.mark.parametrize("name,tile,frame", [("rs_nt25", 12, 49), ("rs_intr_run3", 1, 5)])
def test_the_covariance_bound_sees_a_one_tile_error(oracle, name, tile, frame):
    """A 1e-9 relative error in ONE 48 x 48 camera-camera block of J^T J (the diagonal tile of four two-pose frames)."""
    def edit(H, free):
        k = np.flatnonzero(free // 48 == tile)
        assert len(k) == 48
        H = H.tolil()
        H[np.ix_(k, k)] = H[np.ix_(k, k)].toarray() * np.longdouble(1 + 1e-9)
        return H.tocsr()
    seeded, clean, ref = _seeded(oracle, name, [frame], edit=edit)
    print(f"{name} tile {tile}: ratio {seeded:.3g} (kappa^ {ref.kappa:.2e})")
    assert clean <= 1e-3 and seeded > C_COV, (seeded, clean)


def test_the_covariance_bound_sees_a_constant_ratio(oracle):
    """The free interFrameRatio's column dropped: the covariance of the constant-ratio problem."""
    p = LC.cov_case("rs_acc_free")
    seeded, clean, ref = _seeded(oracle, "rs_acc_free", [1, 4, 8], constant=[R.layout(p)["iratio"]])
    print(f"rs_acc_free, constant ratio: ratio {seeded:.3g}")
    assert clean <= 1e-3 and seeded > C_COV, (seeded, clean)


def test_the_covariance_bound_sees_constant_prior_poses(oracle):
    """The priorPoses columns dropped: GoodPosePrior blocks treated as constants."""
    p = LC.cov_case("rs_pp_some")
    L = R.layout(p)
    seeded, clean, ref = _seeded(oracle, "rs_pp_some", [1, 7], constant=np.arange(L["ipp"], L["ipp"] + 6 * len(p.pose_prior_block)))
    print(f"rs_pp_some, constant priorPoses: ratio {seeded:.3g}")
    assert clean <= 1e-3 and seeded > C_COV, (seeded, clean)


def test_the_covariance_bound_sees_a_missing_corrector(oracle, monkeypatch):
    """The Huber corrector dropped from the Jacobian.  Its alpha term cannot be the seeded error: ceres::Corrector sets alpha = 0
    whenever rho'' <= 0 (corrector.cc), and HuberLoss has rho'' = -rho' / (2 s) < 0 beyond its threshold and 0 within — alpha is
    identically zero under this loss (asserted below), so dropping it changes nothing.  What the corrector does to J^T J here is the
    factor rho' = a / |r| on the outliers' blocks: that factor dropped (J left uncorrected) is the error seeded instead."""
    frames = [1, 4, 8]
    p = LC.cov_case("rs_huber")
    r, J, _ = oracle.evaluate_blocks(p)
    s = np.sum(r * r, axis=1)
    _, rho1, rho2 = R.huber_rho(float(p.huber_a), s)
    assert np.count_nonzero(rho1 < 1.0) > 10 and np.all(rho2 <= 0.0)             # outliers exist; alpha = 0 on every block
    rc, Jc = R.corrected(float(p.huber_a), r, J)
    assert np.array_equal(Jc, np.sqrt(rho1)[:, None, None] * J)

    def wrong(p, r, J):
        def plain(a, rr, JJ):
            JJ = np.asarray(JJ, dtype=np.float64)
            return np.asarray(rr, dtype=np.float64).reshape(JJ.shape[0], JJ.shape[1]).copy(), JJ.copy()
        with monkeypatch.context() as m:
            m.setattr(R, "corrected", plain)
            return R.covariance_blocks(p, r, J, frames)
    seeded, clean, ref = _seeded(oracle, "rs_huber", frames, wrong=wrong)
    print(f"rs_huber, no corrector: ratio {seeded:.3g}")
    assert clean <= 1e-3 and seeded > C_COV, (seeded, clean)
