"""The general losses (rsba_set_loss: SOFT_L_ONE, CAUCHY, ARCTAN, TOLERANT, scaled) on the paths that tests/test_gpu_loss.py does not
reach — covariance, the iterative linear solver, plan / kernel knobs, several ranks: the cases, the conditions on them, the bounds and
the seeded faults, all on the host (no GPU).  The device tests (tests/test_gpu_loss_paths.py, tests/test_distributed.py) import the
cases, references and constants from here, so that they cannot pass by testing nothing.

Cases.  PAIRS = {rs_huber, rs_intr_shared, rs_acc_free, rs_prior_Fp1, rs_acc_r1.25, gs_intr_run3, rs_far_pair} x {cauchy10, tol100_25}
+ rs_huber x {soft10, arctan100, cauchy10_x0.25}: the scenes of tests/lm_step_cases.py with huber_a = 0 and the losses of
tests/test_gpu_loss.py, imported.  PCG_PAIRS = PAIRS without rs_acc_free (a free ratio is refused by the iterative solver).

Conditions, asserted per pair (test_conditions_on_the_cases prints them): rho1 < 0.5 and rho1 > 0.9 each on >= 5 % of the blocks that
take the loss, TOLERANT's rho2 > 1e-6 on >= 50 %, kappa of the damped step <= 1e9, the covariance references ok with their own error
<= 2^-6 unit.  Measured: rho1 < 0.5 on 29 - 66 %, rho1 > 0.9 on 5.3 - 53 %, rho2 > 1e-6 on 77 - 97 % (TOLERANT), step kappa
5.1e2 - 7.9e4, kappa^ of the scaled J^T J 5.9e4 - 5.4e7, reference error 6.2e-5 - 2.8e-4 (lm_step_reference.covariance_blocks) and
1.8e-4 - 1.2e-3 (cov_reference.full_covariance) of the unit.

Points of the covariance blocks (regime_points).  No scene here has eight points whose observations ALL have rho1 > 0.9: a point has
8 - 12 observations and 5 - 53 % of the observations are there, so 0 - 6 points of a scene qualify (rs_huber tol100_25: 6; every CAUCHY
pair: 0).  The points asked instead are the 12 with the LARGEST SHARE of observations at rho1 > 0.9 (at least eight have one: 164 - 765
points), 12 with an observation at rho1 < 0.5 (386 - 765 points have one), under TOLERANT 12 with one at rho2 > 1e-6 (every point has
one), 8 points of the frame of fault (d), and every 13th point: 52 - 89 points a pair.  None of the scenes has a constant point.

Bounds, none from device output.
  * step: C_TOL = 64 (tests/test_lm_step_reference.py); pose covariance: C_COV = 8 (there).
  * covariance blocks of the selected inverse: the rule of tests/test_cov_reference.py — the smallest power of two >= 4 x the worst ratio
    of cov_reference.selinv_fp64 against full_covariance, never below C_COV — run again under every pair, through the same plan
    lookup.  Worst ratio per family over the 17 pairs: (f, f) 0.693, (f, g) 0.687 (both gs_intr_run3 tol100_25), intrinsics 1.245,
    points 1.245 (both rs_intr_shared cauchy10, kappa^ 4.5e7), asymmetry 0.  4 x 1.245 = 4.98: the rule keeps C_COVP = 8, imported.
  * PCG, the rules of tests/test_gpu_pcg.py recomputed for PCG_PAIRS.  Distance of the fp64 restatement from the long-double iterates
    (R.step_ratio units), the first iteration within a factor 2 of the restatement's error floor, the converged restatement:
        pair                              k=1       k=2       k=3      floor at   N_CASE   converged
        rs_huber cauchy10               0.2092    0.2510    0.2712       35         45      0.335
        rs_huber tol100_25              0.1068    0.2886    0.3065       35         45      0.288
        rs_intr_shared cauchy10         0.0483    0.0757    0.1593       85         95      3.87
        rs_intr_shared tol100_25        0.0390    0.0750    0.1069       96        106      0.522
        rs_prior_Fp1 cauchy10           0.0036    0.0081    0.0092       44         54      0.201
        rs_prior_Fp1 tol100_25          0.0096    0.0137    0.0218       68         78      0.135
        rs_acc_r1.25 cauchy10           0.0058    0.0080    0.0124       46         56      0.0935
        rs_acc_r1.25 tol100_25          0.0109    0.0119    0.0169       64         74      0.146
        gs_intr_run3 cauchy10           0.0139    0.0386    0.0351      301        311      0.521
        gs_intr_run3 tol100_25          0.0664    0.0544    0.0332      323        333      0.0881
        rs_far_pair cauchy10            0.0048    0.0124    0.0146       63         73      0.102
        rs_far_pair tol100_25           0.0061    0.0044    0.0052       95        105      0.0475
        rs_huber soft10                 0.1190    0.8057    0.9259       35         45      0.805
        rs_huber arctan100              0.2577    0.2124    0.1845       34         44      0.443
        rs_huber cauchy10_x0.25         0.2949    0.3717    0.4118       35         45      0.378
    The worst is 0.92593873306839136 (rs_huber soft10, k = 3): 4 x it = 3.70 is above the 1.98 of tests/test_gpu_pcg.py, so
    C_ITER = 3.70 here, for the new tests only.  The converged restatement is within 3.87 units (rs_intr_shared cauchy10); 4 x 3.87 =
    15.5 is below C_TOL, so C_PCG = 64.  Stopping rule: the long-double run stops by its test on every pair (2 - 3 iterations with
    min_iterations 1, 3 with 3), and its criterion is nowhere within 1e-6 relative of eta = 0.1 (the nearest: 2.1e-2 relative, on
    rs_intr_shared tol100_25) — no pair had to be replaced.
  * the whole solve with the iterative solver, (rs_huber, cauchy10), 15 iterations: the reference loop has one rejected step (iteration
    5, relative decrease -0.141: the decision nearest to min_relative_decrease = 1e-3; the accepted steps have 0.55 - 1.71), so the
    pair stays.

Seeded faults, each "ratio > bound" on its pairs (measured):
  (a) the loss ignored (TRIVIAL weights), all 17 pairs: step 9.3e9 - 1.2e15 units against C_TOL, pose covariance 1.3e8 - 7.5e10 against
      C_COV;
  (b) TOLERANT with rho2 forced to 0, the seven tol100_25 pairs: step 1.1e11 - 3.8e12, pose covariance 1.7e8 - 9.1e10;
  (c) the (f, f - 1) block of every motion prior with its 2 x 2-per-coordinate entries only, rs_prior_Fp1 / rs_acc_r1.25 / rs_acc_free
      with tol100_25: step 1.3e9 / 2.9e9 / 2.1e10, pose covariance 9.1e8 / 4.9e8 / 2.1e9, the PCG iterate at k = 2 2.8e8 / 1.0e8 against
      C_ITER (rs_acc_free has a free ratio: the iterative solver refuses it, so the PCG iterate is checked on the other two).  Under
      CAUCHY the dropped entries are exactly zero (rho'' < 0: alpha = 0), asserted: only TOLERANT tests this fault;
  (d) the point rows of one frame (the first of the second tile) from the record of the no-loss instantiation, all 17 pairs, on the
      point blocks: 2.1e9 - 3.7e12 against C_COVP, while the points that frame does not see stay at 0.007 - 0.95.
No pair had to be replaced for any fault."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_reference as CR                                       # noqa: E402
import lm_step_cases as LC                                       # noqa: E402
import lm_step_reference as R                                    # noqa: E402
import loss_reference as L                                       # noqa: E402
import pcg_reference as PR                                       # noqa: E402
import test_cov_reference as TR                                  # noqa: E402
import test_gpu_loss as GL                                       # noqa: E402  (LOSSES, SCALED, the scenes with huber_a = 0: not restated)
import test_gpu_pcg as GP                                        # noqa: E402
from helpers import HOOKS_LIB                                    # noqa: E402
from test_lm_step_reference import C_COV, C_TOL, covariance_worst   # noqa: E402
from test_selinv_plan import plan as selinv_plan                 # noqa: E402

SCENES = ["rs_huber", "rs_intr_shared", "rs_acc_free", "rs_prior_Fp1", "rs_acc_r1.25", "gs_intr_run3", "rs_far_pair"]
PAIRS = [(s, k) for s in SCENES for k in ("cauchy10", "tol100_25")] + [("rs_huber", k) for k in ("soft10", "arctan100", "cauchy10_x0.25")]
PCG_PAIRS = [q for q in PAIRS if q[0] != "rs_acc_free"]          # a free ratio is refused by the iterative solver
TOL_PAIRS = [q for q in PAIRS if q[1] == "tol100_25"]
CROSS_PAIRS = [(s, "tol100_25") for s in ("rs_prior_Fp1", "rs_acc_r1.25", "rs_acc_free")]   # motion priors under rho'' > 0: dense (f, f - 1) blocks
assert all(GL.the_loss(k)[0] != L.TRIVIAL for _, k in PAIRS)

C_COVP = TR.C_COVP                                               # 8: the rule of tests/test_cov_reference.py keeps it here (docstring)
C_ITER = 4 * 0.92593873306839136                                 # 3.70: rs_huber soft10, k = 3 (docstring)
C_PCG = C_TOL
N_CASE = {("rs_huber", "cauchy10"): 45, ("rs_huber", "tol100_25"): 45, ("rs_intr_shared", "cauchy10"): 95, ("rs_intr_shared", "tol100_25"): 106,
          ("rs_prior_Fp1", "cauchy10"): 54, ("rs_prior_Fp1", "tol100_25"): 78, ("rs_acc_r1.25", "cauchy10"): 56, ("rs_acc_r1.25", "tol100_25"): 74,
          ("gs_intr_run3", "cauchy10"): 311, ("gs_intr_run3", "tol100_25"): 333, ("rs_far_pair", "cauchy10"): 73, ("rs_far_pair", "tol100_25"): 105,
          ("rs_huber", "soft10"): 45, ("rs_huber", "arctan100"): 44, ("rs_huber", "cauchy10_x0.25"): 45}
ETA = 0.1
WHOLE_PCG = ("rs_huber", "cauchy10")                             # the whole solve with the iterative solver
WHOLE_PCG_OPTS = dict(max_num_iterations=15)
MIN_POINTS = 8                                                   # points per regime whose blocks the device test asks for


@pytest.fixture(scope="module")
def hooks():
    import __graft_entry__ as G
    G.build()
    return C.CDLL(HOOKS_LIB)


def radius_of(opts):
    return {k: opts[k] for k in ("initial_trust_region_radius",) if k in opts}


def case(oracle, name, key):
    """(problem with huber_a = 0, the same with the corrector switched on for L.substituted, options, raw r, raw J, loss)"""
    p, opts, r, J = GL.scene(oracle, name)
    return p, L._with_loss(p), opts, r, J, GL.the_loss(key)


def regime_conditions(p, r, loss):
    """The regime conditions of a (problem, loss): asserted wherever a device test relies on them.  -> the three fractions."""
    r1, r2 = GL.regimes(p, r, loss)
    lo, hi, curved = float(np.mean(r1 < 0.5)), float(np.mean(r1 > 0.9)), float(np.mean(r2 > 1e-6))
    assert lo >= 0.05 and hi >= 0.05, (lo, hi)
    if loss[0] == L.TOLERANT:
        assert curved >= 0.5, curved
    return lo, hi, curved


_cache = {}


def cached(kind, name, key, make):
    if (kind, name, key) not in _cache:
        _cache[(kind, name, key)] = make()
    return _cache[(kind, name, key)]


def step_reference(oracle, name, key):
    p, q, opts, r, J, loss = case(oracle, name, key)
    return cached("step", name, key, lambda: L.lm_step(p, r, J, loss, **radius_of(opts)))


def pose_covariance_reference(oracle, name, key):
    """(frames of LC.cov_frames, R.covariance_blocks under the loss)"""
    p, q, opts, r, J, loss = case(oracle, name, key)

    def make():
        frames = LC.cov_frames(p)
        with L.substituted(loss):
            return frames, R.covariance_blocks(q, r, J, frames)
    return cached("cov", name, key, make)


def regime_points(p, r, loss, frame):
    """The points whose blocks are asked for, by regime of their observations at the first linearisation: the 12 with the largest
    share of observations at rho1 > 0.9 (see the module's docstring: no scene here has eight points whose observations are ALL there),
    12 with an observation at rho1 < 0.5, 12 with one at rho2 > 1e-6 (none but under TOLERANT), 8 seen by ``frame`` (the frame of the
    seeded record fault), the first constant point, and every 13th point.  -> (points, sizes of the three regime groups in the
    whole scene: an observation at rho1 > 0.9, one at rho1 < 0.5, one at rho2 > 1e-6; and of the group with ALL at rho1 > 0.9)."""
    N, M = p.num_observations, p.num_points
    r1, r2 = GL.regimes(p, r, loss)
    r1, r2 = r1[:N], r2[:N]
    j = p.obs_point.astype(np.int64)
    count = np.bincount(j, minlength=M)
    high = np.bincount(j, weights=(r1 > 0.9), minlength=M)
    any_low = np.bincount(j, weights=(r1 < 0.5), minlength=M) > 0
    any_curved = np.bincount(j, weights=(r2 > 1e-6), minlength=M) > 0
    free = np.ones(M, dtype=bool) if p.point_constant is None else ~p.point_constant.astype(bool)
    share = np.where(free & (count > 0), high / np.maximum(count, 1), 0.0)
    by_share = np.argsort(-share, kind="stable")
    groups = [by_share[: int(np.count_nonzero(share > 0))], np.flatnonzero(any_low & free), np.flatnonzero(any_curved & free)]
    out = {int(x) for g in groups for x in g[:12]} | {int(x) for x in np.unique(j[p.obs_frame == frame])[:8]} | set(range(0, M, 13))
    if not free.all():
        out.add(int(np.flatnonzero(~free)[0]))
    return sorted(out), [len(g) for g in groups] + [int(np.count_nonzero(share == 1.0))]


def fault_frame(p):
    return 48 // (6 * p.poses_per_frame)                          # the first frame of the second tile


def plan_of(hooks):
    def f(nt, edges):
        old = os.environ.pop("RSBA_CHOL_LEAF", None)
        try:
            return selinv_plan(hooks, nt, edges)
        finally:
            if old is not None:
                os.environ["RSBA_CHOL_LEAF"] = old
    return f


def blocks_reference(oracle, name, key):
    """(frame pairs of test_cov_reference.pairs_of, points of regime_points, intrinsics blocks, sizes of the regime groups,
    cov_reference.full_covariance under the loss)"""
    p, q, opts, r, J, loss = case(oracle, name, key)

    def make():
        pairs = TR.pairs_of(p)
        points, sizes = regime_points(p, r, loss, fault_frame(p))
        intr = [] if p.calibrated else list(range(p.num_intrinsics))
        with L.substituted(loss):
            return pairs, points, intr, sizes, CR.full_covariance(q, r, J, pairs, points, intr)
    return cached("blocks", name, key, make)


def pcg_reference(oracle, name, key):
    """(problem, options, LMStep, Reduced in long double, StepMaker, the first three iterates in long double) under the loss"""
    p, q, opts, r, J, loss = case(oracle, name, key)

    def make():
        ref = step_reference(oracle, name, key)
        with L.substituted(loss):
            red = PR.reduce_system(q, ref)
            sm = PR.StepMaker(q, r, J, ref)
        return p, opts, ref, red, sm, PR.pcg(red, max_iterations=3, **GP.OFF)
    return cached("pcg", name, key, make)


# ---- the conditions on the cases ------------------------------------------------------------------------------------------------

def test_the_case_list_is_the_issues():
    assert len(PAIRS) == 17 and len(set(PAIRS)) == 17 and len(PCG_PAIRS) == 15 and set(N_CASE) == set(PCG_PAIRS)
    assert {k for _, k in PAIRS} == {"cauchy10", "tol100_25", "soft10", "arctan100", "cauchy10_x0.25"}
    assert GL.the_loss("cauchy10") == L.loss(L.CAUCHY, 10) and GL.the_loss("tol100_25") == L.loss(L.TOLERANT, 100, 25)
    assert GL.the_loss("cauchy10_x0.25") == L.loss(L.CAUCHY, 10, scale=0.25)


@pytest.mark.parametrize("name,key", PAIRS)
def test_conditions_on_the_cases(oracle, name, key):
    p, q, opts, r, J, loss = case(oracle, name, key)
    assert p.huber_a == 0.0
    lo, hi, curved = regime_conditions(p, r, loss)
    ref = step_reference(oracle, name, key)
    frames, cov = pose_covariance_reference(oracle, name, key)
    print(f"LOSSPATH conditions {name} {key}: rho1 < 0.5 on {lo:.3f}, rho1 > 0.9 on {hi:.3f}, rho2 > 1e-6 on {curved:.3f}, kappa of the damped step "
          f"{ref.kappa:.2e}, kappa^ of scaled J^T J {cov.kappa:.2e}, covariance reference error {cov.error:.1e}")
    assert ref.kappa <= 1e9
    assert cov.ok and cov.error <= 2.0 ** -6
    assert (R.layout(p)["iratio"] >= 0) == (name == "rs_acc_free")


# ---- C_COVP: the selected inverse restated in fp64, under every pair --------------------------------------------------------------

@pytest.mark.parametrize("name,key", PAIRS)
def test_the_restated_selected_inverse_keeps_the_bound(oracle, hooks, name, key):
    p, q, opts, r, J, loss = case(oracle, name, key)
    pairs, points, intr, sizes, ref = blocks_reference(oracle, name, key)
    assert ref.ok and ref.error <= 2.0 ** -6
    assert sizes[0] >= MIN_POINTS and sizes[1] >= MIN_POINTS and (loss[0] != L.TOLERANT or sizes[2] >= MIN_POINTS), sizes
    with L.substituted(loss):
        got = CR.selinv_fp64(q, r, J, plan_of(hooks), pairs, points, intr)
    w = TR.worst_ratios(ref, got.frame_blocks, got.intr_blocks, got.point_blocks)
    print(f"LOSSPATH selinv_fp64 {name} {key}: worst ratio (f, f) {w['diag']:.3f}, (f, g) {w['cross']:.3f}, intrinsics {w['intr']:.3f}, points {w['point']:.3f} "
          f"({len(points)} of {p.num_points}; regime groups {sizes}), asymmetry {w['asym']:.3f}, kappa^ {ref.kappa:.2e}, reference error {ref.error:.1e}")
    assert 4 * max(w.values()) <= C_COVP, (name, key, w)
    assert C_COVP >= C_COV and C_COVP & (C_COVP - 1) == 0


# ---- C_ITER, C_PCG, N_CASE and the stopping rule ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,key", PCG_PAIRS)
def test_the_pcg_constants_are_four_times_the_restatement(oracle, name, key):
    p, opts, ref, red, sm, run = pcg_reference(oracle, name, key)
    q, loss = L._with_loss(p), GL.the_loss(key)
    red64 = PR.reduce_system(q, ref, np.float64)
    r64 = PR.pcg(red64, max_iterations=700, **GP.OFF)            # (the floor is reached by iteration 323 at the latest)
    d = []
    for k in (1, 2, 3):
        want = sm.step(PR.full_solution(red, ref, run.y[k]))
        got = sm.step(PR.full_solution(red64, ref, r64.y[k]))
        d.append(R.step_ratio(p, want, *PR.applied(p, got))[0])
    yc = np.asarray(ref.y)[red.cam].astype(np.float64)
    err = np.array([np.max(np.abs(np.asarray(y) - yc)) for y in r64.y])
    first = int(np.flatnonzero(err <= 2 * err.min())[0])
    got = sm.step(PR.full_solution(red64, ref, r64.y[N_CASE[(name, key)]]))
    conv, where = R.step_ratio(p, ref, *PR.applied(p, got))
    print(f"LOSSPATH pcg restatement {name} {key}: k=1 {d[0]:.4g} k=2 {d[1]:.4g} k=3 {d[2]:.4g}, first iteration within 2x of the floor {first}, "
          f"converged {conv:.3g} at {where}, kappa {ref.kappa:.2e}")
    assert max(d) <= C_ITER / 4 * (1 + 1e-9), d
    assert first + 10 == N_CASE[(name, key)], first
    assert conv <= C_PCG / 4, (conv, where)


@pytest.mark.parametrize("min_iterations", [1, 3])
@pytest.mark.parametrize("name,key", PCG_PAIRS)
def test_no_stopping_criterion_sits_on_eta(oracle, name, key, min_iterations):
    p, opts, ref, red, sm, _ = pcg_reference(oracle, name, key)
    run = PR.pcg(red, min_iterations=min_iterations, eta=ETA)
    near = min(abs(float(run.zeta[k]) - ETA) / ETA for k in range(max(min_iterations, 1), run.iterations + 1))
    print(f"LOSSPATH pcg stop {name} {key} min={min_iterations}: {run.iterations} iterations, zeta {float(run.zeta[run.iterations]):.4g}, nearest to eta {near:.3g} relative")
    assert run.reason == "test" and near > 1e-6


def test_the_whole_pcg_solves_reference_has_no_decision_on_the_edge(oracle):
    name, key = WHOLE_PCG
    p, q, opts, r, J, loss = case(oracle, name, key)
    want, _ = L.lm_loop(oracle, p, loss, **dict(radius_of(opts), **WHOLE_PCG_OPTS))
    for t in want[1:]:
        print(f"LOSSPATH whole {name} {key}: iteration {t['iteration']} accepted {t['step_is_successful']} relative_decrease {t['relative_decrease']:.4g} cost {t['cost']:.12e}")
        assert abs(t["relative_decrease"] - 1e-3) > 1e-6, t
    assert len(want) > 3


# ---- seeded faults: each exceeds the bound of the device test that is there for it ---------------------------------------------

@contextlib.contextmanager
def substituted_without_rho2(loss):
    """The loss with rho'' forced to 0: the corrector without its rank-one term."""
    saved = R.huber_rho

    def rho(a, s):
        r0, r1, r2 = L.rho(loss, s)
        return r0, r1, np.zeros_like(r2)
    R.huber_rho = rho
    try:
        yield
    finally:
        R.huber_rho = saved


def as64(cov, frames):
    return {f: cov.blocks[f].astype(np.float64) for f in frames}


def step_and_covariance_ratio(oracle, name, key, wrong_step, wrong_cov):
    p, q, opts, r, J, loss = case(oracle, name, key)
    ref = step_reference(oracle, name, key)
    frames, cov = pose_covariance_reference(oracle, name, key)
    other = wrong_cov(frames)
    assert other.ok
    return R.step_ratio(p, ref, *PR.applied(p, wrong_step()))[0], covariance_worst(cov, as64(other, frames))


@pytest.mark.parametrize("name,key", PAIRS)
def test_the_bounds_see_an_ignored_loss(oracle, name, key):
    """(a) TRIVIAL weights where the loss was asked for: the no-loss instantiation of every pass."""
    p, q, opts, r, J, loss = case(oracle, name, key)
    step, cov = step_and_covariance_ratio(oracle, name, key, lambda: R.lm_step(p, r, J, want_kappa=False, **radius_of(opts)),
                                          lambda frames: R.covariance_blocks(p, r, J, frames))
    print(f"LOSSPATH fault (a) {name} {key}: step {step:.3g} (bound {C_TOL}), covariance {cov:.3g} (bound {C_COV})")
    assert step > C_TOL and cov > C_COV


@pytest.mark.parametrize("name,key", TOL_PAIRS)
def test_the_bounds_see_a_dropped_rank_one_term(oracle, name, key):
    """(b) TOLERANT with rho'' forced to 0."""
    p, q, opts, r, J, loss = case(oracle, name, key)

    def wrong_step():
        with substituted_without_rho2(loss):
            return R.lm_step(q, r, J, want_kappa=False, **radius_of(opts))

    def wrong_cov(frames):
        with substituted_without_rho2(loss):
            return R.covariance_blocks(q, r, J, frames)
    step, cov = step_and_covariance_ratio(oracle, name, key, wrong_step, wrong_cov)
    print(f"LOSSPATH fault (b) {name} {key}: step {step:.3g} (bound {C_TOL}), covariance {cov:.3g} (bound {C_COV})")
    assert step > C_TOL and cov > C_COV


def sparse_prior_cross(p, H, free):
    """H without the entries of the motion priors' (f, f - 1) blocks that couple different pose coordinates: the block as sparse as it
    is without a loss (2 x 2 per coordinate).  Nothing else of H lies there: the points are not eliminated.  -> (H, largest dropped)"""
    F, CD = p.num_frames, 6 * p.poses_per_frame
    H = sp.coo_matrix(H)
    g = np.asarray(free)
    gi, gj = g[H.row], g[H.col]
    pose = (gi < F * CD) & (gj < F * CD)
    fi, fj = np.where(pose, gi // CD, -9), np.where(pose, gj // CD, -9)
    pf = np.zeros(F + 10, dtype=bool)
    pf[np.asarray(p.prior_frames, dtype=np.int64)] = True
    cross = pose & (((fi == fj + 1) & pf[fi]) | ((fj == fi + 1) & pf[fj]))
    drop = cross & (gi % 6 != gj % 6)
    worst = float(np.max(np.abs(H.data[drop]))) if drop.any() else 0.0
    return sp.csr_matrix((H.data[~drop], (H.row[~drop], H.col[~drop])), shape=H.shape), worst


@pytest.mark.parametrize("name,key", CROSS_PAIRS)
def test_the_bounds_see_a_sparse_prior_cross_block(oracle, name, key):
    """(c) the (f, f - 1) block of every motion prior keeps its 2 x 2-per-coordinate entries only: what a launcher that takes the
    no-loss prior kernel, or a cross block left from before the loss was set, gives.  In the step, in the covariance and — where the
    iterative solver takes the problem (no free ratio) — in the iterate after two CG iterations."""
    p, q, opts, r, J, loss = case(oracle, name, key)
    dropped = []

    def edit_step(H, free, scale):
        H, worst = sparse_prior_cross(p, H, free)
        dropped.append(worst)
        return H

    def wrong_step():
        with L.substituted(loss):
            return R.lm_step(q, r, J, want_kappa=False, edit=edit_step, **radius_of(opts))

    def wrong_cov(frames):
        with L.substituted(loss):
            return R.covariance_blocks(q, r, J, frames, edit=lambda H, free: sparse_prior_cross(p, H, free)[0])
    step, cov = step_and_covariance_ratio(oracle, name, key, wrong_step, wrong_cov)
    assert dropped[0] > 0.0                                      # the rank-one term does fill those entries
    print(f"LOSSPATH fault (c) {name} {key}: step {step:.3g} (bound {C_TOL}), covariance {cov:.3g} (bound {C_COV}), largest dropped entry of the scaled matrix {dropped[0]:.3g}")
    assert step > C_TOL and cov > C_COV
    if (name, key) in PCG_PAIRS:
        _, _, ref, red, sm, run = pcg_reference(oracle, name, key)
        D = PR.prior_cross_entries(q, ref, red)
        assert np.any(D != 0) and np.array_equal(D, D.T)
        bad = PR.pcg(red, max_iterations=3, drop_entries=D, **GP.OFF)
        want = sm.step(PR.full_solution(red, ref, run.y[2]))
        got = sm.step(PR.full_solution(red, ref, bad.y[2]))
        ratio = R.step_ratio(p, want, *PR.applied(p, got))[0]
        print(f"LOSSPATH fault (c) {name} {key}: PCG iterate k = 2 {ratio:.3g} (bound {C_ITER:.3g})")
        assert ratio > C_ITER


def test_a_loss_without_curvature_leaves_the_prior_cross_block_sparse(oracle):
    """The other side of (c): under CAUCHY (rho'' < 0: alpha = 0) those entries are exactly zero, which is why only TOLERANT tests it."""
    p, q, opts, r, J, loss = case(oracle, "rs_acc_r1.25", "cauchy10")
    ref = step_reference(oracle, "rs_acc_r1.25", "cauchy10")
    assert sparse_prior_cross(p, ref.H, ref.free)[1] == 0.0


@pytest.mark.parametrize("name,key", PAIRS)
def test_the_bound_sees_point_rows_from_the_no_loss_record(oracle, hooks, name, key):
    """(d) the point rows of one frame built from the record of the other instantiation (cov_reference.selinv_fp64, fault "record"):
    checked on the point blocks."""
    p, q, opts, r, J, loss = case(oracle, name, key)
    pairs, points, intr, sizes, ref = blocks_reference(oracle, name, key)
    f = fault_frame(p)
    with L.substituted(loss):
        got = CR.selinv_fp64(q, r, J, plan_of(hooks), pairs[:1], points, fault="record", fault_frame=f)
    hit = set(int(j) for j in p.obs_point[p.obs_frame == f])
    worst = max(CR.point_ratio(ref, j, got.point_blocks[j]) for j in points)
    clean = max([CR.point_ratio(ref, j, got.point_blocks[j]) for j in points if j not in hit] + [0.0])
    print(f"LOSSPATH fault (d) {name} {key}: frame {f}, points {worst:.3g} (bound {C_COVP}), points the frame does not see {clean:.3g}")
    assert worst > C_COVP and 4 * clean <= C_COVP
