"""The host reference of one LM step (tests/lm_step_reference.py) against the CPU oracle's first step, and proof that the tolerance
tests/test_gpu_lm_step.py puts on the device step would see a one-tile error of the reduced camera system.

The oracle solves by Schur elimination and an envelope Cholesky of the reduced system; the reference by a dense (or sparse LU)
factorisation of the whole damped system refined in long double.  They share no code, so agreement to a few kappa * eps on every
scene shape of tests/lm_step_cases.py checks both.  Measured here: error / (kappa eps |delta|_inf) <= 18 (the intrinsics scenes;
below 3 elsewhere), the model cost change to <= 1e-13 relative."""
import numpy as np
import pytest

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


@pytest.mark.parametrize("name", LC.CASES)
def test_reference_step_matches_the_oracles_first_step(oracle, name):
    p, opts, ref = reference(oracle, name)
    assert ref.kappa <= 1e9, ref.kappa
    assert ref.refinement[-1] <= 1e-16, ref.refinement          # the refined residual sits far below fp64 kappa * eps
    q = p.copy()
    s, tr = oracle.solve(q, oracle.default_options(**opts))
    assert len(tr) == 2 and tr[1].step_is_successful == 1         # a precondition of the case: the step is applied
    ratio, where = R.step_ratio(p, ref, q.poses, q.points, q.intrinsics)
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
