"""The general losses on the device paths that tests/test_gpu_loss.py does not reach: rsba_pose_covariance, rsba_covariance_compute and
its getters, the invalidation of a computed covariance by rsba_set_loss, the iterative linear solver, and every plan / kernel knob —
each against the host reference of the same operation under that loss (loss_reference.substituted around lm_step_reference,
cov_reference and pcg_reference).

Cases, conditions, references and constants come from tests/test_loss_paths_reference.py (no GPU), which derives them and shows that
every bound sees the fault it is there for: the loss ignored, TOLERANT's rank-one term dropped, a motion prior's (f, f - 1) block left
as sparse as it is without a loss, a frame's point rows taken from the record of the no-loss instantiation.  The regime conditions
are asserted again wherever a test relies on them.

Constants.  Step C_TOL = 64 and pose covariance C_COV = 8 (tests/test_lm_step_reference.py); blocks of the selected inverse C_COVP = 8
(the fp64 restatement reaches 1.245 units under these pairs: 4 x 1.245 = 4.98); PCG early iterates C_ITER = 4 x 0.926 = 3.70 (the fp64
restatement's worst distance from the long-double iterates, rs_huber soft10 at k = 3), converged step C_PCG = 64 (restatement: 3.87)
after N_CASE iterations (first iteration within a factor 2 of the restatement's error floor, plus 10); the whole solve 1e-9 relative
(the project's trajectory bound); bit equality where two handles must do the same thing.

What the tests cover:
  * rsba_pose_covariance under every pair, frames of lm_step_cases.cov_frames (rs_acc_free: the free ratio's border under the loss);
  * rsba_covariance_compute and its getters under every pair: every (f, f), both blocks of adjacent frames, a co-visible pair, the
    intrinsics blocks, 52 - 89 points chosen by regime; (a, b) with a > b is the transpose of (b, a) bit for bit;
  * rsba_set_loss on a handle with a computed covariance: every getter returns RSBA_ERR_INVALID_ARGUMENT, and the next compute gives
    the blocks of a fresh handle created with that loss, bit for bit, along none -> TOLERANT -> none -> CAUCHY (rs_acc_r1.25,
    rs_acc_free; the third state is a handle that never had a loss: the priors' dense cross blocks are cleared); the same chain for one
    LM iteration with the exact and with the iterative solver;
  * covariance calls leave the handle as found: the iteration after them is a fresh handle's;
  * the iterative solver over PCG_PAIRS: iterates k = 1, 2, 3 against the long-double ones with model_cost_change, the converged step
    against loss_reference.lm_step, the stopping iteration for min_iterations 1 and 3, the refusal of a free ratio, and a whole solve of
    (rs_huber, cauchy10), its linear systems solved to r_tolerance 1e-13, against loss_reference.lm_loop;
  * every knob of tests/test_gpu_lm_step.py on (rs_acc_free, tol100_25), (gs_intr_run3, tol100_25) and (rs_intr_perframe, cauchy10: the
    path that keeps records) for the step, and all but RSBA_DEVICE_LM on (rs_far_pair, tol100_25) for rsba_pose_covariance.

Measured on an MI355X (every test prints its figure on a line that starts with LOSSPATH before it asserts), worst per family:
  pose covariance 0.157 units (rs_acc_r1.25 cauchy10; 0.015 - 0.157 over the 17 pairs);
  covariance blocks: (f, f) 0.169, (f, g) 0.164 (both rs_acc_r1.25 cauchy10), intrinsics 0.180, points 0.179 (both rs_intr_shared cauchy10),
    asymmetry 0;
  PCG early iterates 0.338 (rs_huber arctan100, k = 3; the scenes with kappa above 1e4 stay below 0.042), model_cost_change within 4.9e-15
    relative; PCG converged step 1.07 (rs_intr_shared cauchy10; 0.020 - 0.44 elsewhere); the stopping iteration equals the reference's
    in all 30 runs (2 - 3 iterations); the whole solve: 15 iterations as the reference, 689 CG iterations in 15 solves, none at the cap,
    final cost within 2.2e-14 relative;
  knobs: step 0.676 (rs_intr_perframe cauchy10 under RSBA_CHOL_FUSE=0; rs_acc_free tol100_25 at most 0.132, gs_intr_run3 tol100_25 0.058),
    model_cost_change within 6.1e-16 relative; pose covariance 0.076 (rs_far_pair tol100_25, 0.007 - 0.076 over the 15 knobs);
  the chains and the handle-as-found tests: bit-equal in every state.
The sharded runs on 2 and 4 ranks are tests/test_distributed.py's."""
import numpy as np
import pytest

import cov_reference as CR
import lm_step_cases as LC
import lm_step_reference as R
import loss_reference as L
import pcg_reference as PR
import test_cov_reference as TR
import test_gpu_loss as GL
import test_gpu_pcg as GP
import test_loss_paths_reference as T
from test_gpu_lm_step import KNOBS, _knob_id
from test_lm_step_reference import C_COV, C_TOL, covariance_worst
from test_loss_paths_reference import C_COVP, C_ITER, C_PCG, N_CASE, PAIRS, PCG_PAIRS

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNSUPPORTED = 1, 6
ANY_DECREASE = GL.ANY_DECREASE
TOL = dict(type=L.TOLERANT, a=100.0, b=25.0)
CAUCHY = dict(type=L.CAUCHY, a=10.0)
NONE = dict(type=L.TRIVIAL)
CHAIN = [None, TOL, NONE, CAUCHY]                                # none (never set) -> TOLERANT -> none -> CAUCHY


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    assert capi.device_count() >= 1
    assert (capi.LOSS_TRIVIAL, capi.LOSS_CAUCHY, capi.LOSS_TOLERANT) == (L.TRIVIAL, L.CAUCHY, L.TOLERANT)
    return capi


def set_env(monkeypatch, knob):
    for kv in (knob if "=" in knob[0] else ["=".join(knob)]):
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)


# ---- rsba_pose_covariance ----------------------------------------------------------------------------------------------------------

def pose_covariance_ratio(capi, oracle, name, key):
    p, q, opts, r, J, loss = T.case(oracle, name, key)
    T.regime_conditions(p, r, loss)
    frames, ref = T.pose_covariance_reference(oracle, name, key)
    assert ref.ok
    with capi.DeviceProblem(p.copy()) as dp:
        GL.set_loss(dp, loss)
        got = {f: dp.pose_covariance(f) for f in frames}
    assert any(blk.any() for blk in got.values())
    return covariance_worst(ref, got), ref


@pytest.mark.parametrize("name,key", PAIRS)
def test_pose_covariance_under_a_loss(capi, oracle, name, key):
    worst, ref = pose_covariance_ratio(capi, oracle, name, key)
    print(f"LOSSPATH pose covariance {name} {key}: ratio {worst:.3f}, kappa^ {ref.kappa:.2e}")
    assert worst <= C_COV, (worst, ref.kappa)


@pytest.mark.parametrize("knob", [k for k in KNOBS if k[0] != "RSBA_DEVICE_LM"], ids=_knob_id)
def test_knobs_keep_the_pose_covariance_under_a_loss(capi, oracle, monkeypatch, knob):
    set_env(monkeypatch, knob)
    worst, ref = pose_covariance_ratio(capi, oracle, "rs_far_pair", "tol100_25")
    print(f"LOSSPATH knob pose covariance rs_far_pair tol100_25 {_knob_id(knob)}: ratio {worst:.3f}, kappa^ {ref.kappa:.2e}")
    assert worst <= C_COV, (worst, ref.kappa)


# ---- rsba_covariance_compute and its getters ---------------------------------------------------------------------------------------

def device_blocks(dp, pairs, points, intr):
    dp.covariance_compute()
    fb = dp.covariance_frame_blocks(pairs)
    pb = dp.covariance_point_blocks(points)
    return ({q: fb[k] for k, q in enumerate(pairs)}, {c: dp.covariance_intrinsics_block(c) for c in intr}, {int(j): pb[k] for k, j in enumerate(points)})


@pytest.mark.parametrize("name,key", PAIRS)
def test_covariance_blocks_under_a_loss(capi, oracle, name, key):
    p, q, opts, r, J, loss = T.case(oracle, name, key)
    T.regime_conditions(p, r, loss)
    pairs, points, intr, sizes, ref = T.blocks_reference(oracle, name, key)
    assert ref.ok
    assert sizes[0] >= T.MIN_POINTS and sizes[1] >= T.MIN_POINTS and (loss[0] != L.TOLERANT or sizes[2] >= T.MIN_POINTS), sizes
    with capi.DeviceProblem(p.copy()) as dp:
        GL.set_loss(dp, loss)
        fb, ib, pb = device_blocks(dp, pairs, points, intr)
    w = TR.worst_ratios(ref, fb, ib, pb)
    print(f"LOSSPATH covariance blocks {name} {key}: worst ratio (f, f) {w['diag']:.3f}, (f, g) {w['cross']:.3f}, intrinsics {w['intr']:.3f}, "
          f"points {w['point']:.3f} ({len(pb)}), asymmetry {w['asym']:.3f}, kappa^ {ref.kappa:.2e}")
    assert max(w.values()) <= C_COVP, (name, key, w, ref.kappa)
    for (a, b), blk in fb.items():
        if a > b:
            assert np.array_equal(blk, fb[(b, a)].T), (a, b)     # the transpose of (b, a), bit for bit
    assert any(blk.any() for blk in pb.values()) and any(a != b and blk.any() for (a, b), blk in fb.items())
    assert (len(intr) > 0) == (not p.calibrated) and all(ib[c].any() for c in intr)
    if p.point_constant is not None and p.point_constant.any():
        const = [j for j in points if p.point_constant[j]]
        assert const and all(not pb[j].any() for j in const)


# ---- rsba_set_loss invalidates a computed covariance; the next one is a fresh handle's -------------------------------------------------

def all_blocks(dp, pairs):
    dp.covariance_compute()
    return dp.covariance_frame_blocks(pairs).tobytes(), dp.covariance_point_blocks(None).tobytes()


@pytest.mark.parametrize("name", ["rs_acc_r1.25", "rs_acc_free"])
def test_set_loss_invalidates_the_covariance_and_the_next_is_a_fresh_handles(capi, oracle, name):
    p, _, _, _ = GL.scene(oracle, name)
    pairs = TR.pairs_of(p)
    fresh = []
    for loss in CHAIN:
        with capi.DeviceProblem(p.copy()) as dp:
            if loss:
                dp.set_loss(**loss)
            fresh.append(all_blocks(dp, pairs))
    assert fresh[0] == fresh[2] and len({f[0] for f in fresh}) == 3 and len({f[1] for f in fresh}) == 3   # three losses, three covariances
    with capi.DeviceProblem(p.copy()) as dp:
        for k, loss in enumerate(CHAIN):
            if loss:
                dp.set_loss(**loss)
                for getter in (lambda: dp.covariance_frame_blocks(pairs[:1]), lambda: dp.covariance_point_blocks([0]), lambda: dp.covariance_point_blocks(None)):
                    with pytest.raises(capi.RsbaError, match="no covariance computed") as e:
                        getter()
                    assert e.value.status == INVALID_ARGUMENT
            got = all_blocks(dp, pairs)
            print(f"LOSSPATH invalidation {name} state {k}: frame blocks equal {got[0] == fresh[k][0]}, point blocks equal {got[1] == fresh[k][1]}")
            assert got == fresh[k], k                            # (k = 2: the dense prior cross blocks of TOLERANT are gone)


def test_set_loss_invalidates_the_intrinsics_getter_too(capi, oracle):
    p, _, _, _ = GL.scene(oracle, "rs_intr_shared")
    with capi.DeviceProblem(p.copy()) as dp:
        dp.covariance_compute()
        plain = dp.covariance_intrinsics_block(0)
        dp.set_loss(**TOL)
        with pytest.raises(capi.RsbaError, match="no covariance computed") as e:
            dp.covariance_intrinsics_block(0)
        assert e.value.status == INVALID_ARGUMENT
        dp.covariance_compute()
        assert not np.array_equal(plain, dp.covariance_intrinsics_block(0))


@pytest.mark.parametrize("solver", ["exact", "pcg"])
def test_set_loss_between_single_iterations_takes_effect(capi, oracle, solver):
    """none -> TOLERANT -> none -> CAUCHY on one handle, the parameters put back before each: every iteration is, bit for bit, that of a
    fresh handle created with the loss — under TOLERANT the (f, f - 1) blocks of the priors are dense, and they must be cleared after it."""
    p, opts, _, _ = GL.scene(oracle, "rs_acc_r1.25")

    def one(dp, q):
        if solver == "pcg":
            dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG)
        o = capi.default_options(**opts)
        o.min_relative_decrease = ANY_DECREASE
        s, tr = dp.solve(o)
        assert len(tr) == 2 and tr[1].step_is_valid == 1
        return GL.bits(q), GL.trace_bits(tr), (dp.linear_solver_stats()["last_iterations"] if solver == "pcg" else 0)
    fresh = []
    for loss in CHAIN:
        q = p.copy()
        with capi.DeviceProblem(q) as dp:
            if loss:
                dp.set_loss(**loss)
            fresh.append(one(dp, q))
    assert fresh[0] == fresh[2] and len({f[0][0] for f in fresh}) == 3
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        for k, loss in enumerate(CHAIN):
            if loss:
                dp.set_loss(**loss)
            for x, y in zip((q.poses, q.points, q.intrinsics), (p.poses, p.points, p.intrinsics)):
                x[...] = y
            dp.upload_parameters()
            got = one(dp, q)
            print(f"LOSSPATH chain {solver} state {k}: equal to a fresh handle {got == fresh[k]}")
            assert got == fresh[k], k


@pytest.mark.parametrize("name,key", [("rs_far_pair", "tol100_25"), ("rs_acc_free", "cauchy10")])
def test_covariance_calls_leave_the_handle_as_found_under_a_loss(capi, oracle, name, key):
    p, q_, opts, r, J, loss = T.case(oracle, name, key)
    frames = LC.cov_frames(p)

    def iteration(before):
        q = p.copy()
        with capi.DeviceProblem(q) as dp:
            GL.set_loss(dp, loss)
            before(dp)
            s, tr = dp.solve(capi.default_options(**opts))
            return GL.bits(q), GL.trace_bits(tr), GL.summary_bits(s), dp.inter_frame_ratio() if p.prior_kind else 0.0

    def blocks(dp):
        dp.covariance_compute()
        assert dp.covariance_frame_blocks([(1, 1)]).any() and dp.covariance_point_blocks([0]).any()
        dp.covariance_release()
    fresh = iteration(lambda dp: None)
    assert iteration(lambda dp: [dp.pose_covariance(f) for f in frames[:2]]) == fresh
    assert iteration(blocks) == fresh
    assert len(fresh[1]) == 2


# ---- the iterative linear solver ------------------------------------------------------------------------------------------------------

def device_step(capi, p, opts, loss, linear=None):
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        GL.set_loss(dp, loss)
        if linear is not None:
            dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG, **linear)
        o = capi.default_options(**opts)
        o.min_relative_decrease = ANY_DECREASE                   # (the step is what is under test: every valid one is applied, see tests/test_gpu_pcg.py)
        s, tr = dp.solve(o)
        st = dp.linear_solver_stats()
        ratio1 = dp.inter_frame_ratio() if R.layout(p)["iratio"] >= 0 else float(q.inter_frame_ratio)
    assert len(tr) == 2 and tr[1].step_is_valid == 1 and tr[1].step_is_successful == 1, (len(tr), tr[-1].step_is_valid, tr[-1].step_is_successful)
    return q, tr, st, ratio1


def blocks_of(q, ratio1):
    return q.poses, q.points, q.intrinsics, ratio1, q.pose_prior_values


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name,key", PCG_PAIRS)
def test_pcg_early_iterates_under_a_loss(capi, oracle, name, key, k):
    p, opts, ref, red, sm, run = T.pcg_reference(oracle, name, key)
    q, tr, st, ratio1 = device_step(capi, p, opts, GL.the_loss(key), dict(max_iterations=k, **GP.OFF))
    assert st["last_iterations"] == k and st["num_linear_solves"] == 1 and st["num_solves_at_cap"] == 1 and st["num_failed_solves"] == 0, st
    want = sm.step(PR.full_solution(red, ref, run.y[k]))
    ratio, where = R.step_ratio(p, want, *blocks_of(q, ratio1))
    rel = abs(tr[1].model_cost_change - want.model_cost_change) / abs(want.model_cost_change)
    print(f"LOSSPATH pcg early {name} {key} k={k}: ratio {ratio:.4g} at {where}, mcc_rel {rel:.3g}, kappa {ref.kappa:.3g}")
    assert ratio <= C_ITER, (ratio, where, ref.kappa)
    assert rel <= 1e-12, (tr[1].model_cost_change, want.model_cost_change)


@pytest.mark.parametrize("name,key", PCG_PAIRS)
def test_pcg_converged_step_under_a_loss(capi, oracle, name, key):
    p, opts, ref, red, sm, run = T.pcg_reference(oracle, name, key)
    n = N_CASE[(name, key)]
    q, tr, st, ratio1 = device_step(capi, p, opts, GL.the_loss(key), dict(eta=0.0, r_tolerance=0.0, max_iterations=n))
    ratio, where = R.step_ratio(p, ref, *blocks_of(q, ratio1))
    print(f"LOSSPATH pcg converged {name} {key} N={n}: iterations {st['last_iterations']}, ratio {ratio:.4g} at {where}, residual {st['last_relative_residual']:.3g}")
    assert st["num_failed_solves"] == 0
    assert ratio <= C_PCG, (ratio, where, ref.kappa)


@pytest.mark.parametrize("min_iterations", [1, 3])
@pytest.mark.parametrize("name,key", PCG_PAIRS)
def test_pcg_stopping_rule_under_a_loss(capi, oracle, name, key, min_iterations):
    p, opts, ref, red, sm, _ = T.pcg_reference(oracle, name, key)
    run = PR.pcg(red, min_iterations=min_iterations, eta=T.ETA)
    n = run.iterations
    assert run.reason == "test" and not any(abs(float(run.zeta[k]) - T.ETA) <= 1e-6 * T.ETA for k in range(max(min_iterations, 1), n + 1))
    q, tr, st, _ = device_step(capi, p, opts, GL.the_loss(key), dict(min_iterations=min_iterations))
    print(f"LOSSPATH pcg stop {name} {key} min={min_iterations}: device {st['last_iterations']} reference {n} zeta {float(run.zeta[n]):.4g}")
    assert st["last_iterations"] == n, (st, n, [float(z) for z in run.zeta[1:]])
    assert st["num_solves_at_cap"] == 0 and st["num_failed_solves"] == 0
    y = GP.camera_y(p, ref, red, q)                              # the step the device returned satisfies the inequality in long double
    res = red.rhs - red.S @ y
    Q = PR.LD(-0.5) * np.dot(y, red.rhs + res)
    zeta = n * (Q - run.Q[n - 1]) / Q
    assert zeta < T.ETA, (float(zeta), n)
    rel = float(np.sqrt(np.dot(res, res) / np.dot(red.rhs, red.rhs)))
    assert abs(st["last_relative_residual"] - rel) <= 1e-6 * rel + 1e-9, (st["last_relative_residual"], rel)


def test_pcg_still_refuses_a_free_ratio_under_a_loss(capi, oracle):
    p, opts, _, _ = GL.scene(oracle, "rs_acc_free")
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        dp.set_loss(**TOL)
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG)
        with pytest.raises(capi.RsbaError) as e:
            dp.solve(capi.default_options(**opts))
        assert e.value.status == UNSUPPORTED and "iterative linear solver" in str(e.value)
        assert GL.bits(q) == GL.bits(p)


def test_a_whole_pcg_solve_under_a_loss_follows_the_reference_loop(capi, oracle):
    name, key = T.WHOLE_PCG
    p, q_, opts, r, J, loss = T.case(oracle, name, key)
    o = dict(T.radius_of(opts), **T.WHOLE_PCG_OPTS)
    want, _ = L.lm_loop(oracle, p, loss, **o)
    assert all(abs(t["relative_decrease"] - 1e-3) > 1e-6 for t in want[1:])
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        GL.set_loss(dp, loss)
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG, eta=0.0, r_tolerance=1e-13, max_iterations=2000)   # (solved to the residual's floor: the reference loop takes exact steps)
        s, tr = dp.solve(capi.default_options(**o))
        st = dp.linear_solver_stats()
    err = abs(s.final_cost - want[-1]["cost"]) / want[-1]["cost"]
    print(f"LOSSPATH pcg whole {name} {key}: {len(tr) - 1} iterations (reference {len(want) - 1}), CG iterations {st['total_iterations']} in {st['num_linear_solves']} solves, "
          f"final cost {s.final_cost:.12e} (reference {want[-1]['cost']:.12e}), relative error {err:.2e}")
    assert st["num_solves_at_cap"] == 0 and st["num_failed_solves"] == 0 and st["num_linear_solves"] >= 3
    assert len(tr) == len(want)
    assert err <= 1e-9


# ---- plan and kernel knobs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,key", [("rs_acc_free", "tol100_25"), ("gs_intr_run3", "tol100_25"), ("rs_intr_perframe", "cauchy10")])
@pytest.mark.parametrize("knob", KNOBS, ids=_knob_id)
def test_knobs_keep_the_step_under_a_loss(capi, oracle, monkeypatch, knob, name, key):
    p, q_, opts, r, J, loss = T.case(oracle, name, key)
    T.regime_conditions(p, r, loss)
    ref = T.step_reference(oracle, name, key)
    assert ref.kappa <= 1e9
    set_env(monkeypatch, knob)
    q, tr, st, ratio1 = device_step(capi, p, opts, loss)
    ratio, where = R.step_ratio(p, ref, *blocks_of(q, ratio1))
    mcc = abs(tr[1].model_cost_change - ref.model_cost_change) / abs(ref.model_cost_change)
    print(f"LOSSPATH knob step {name} {key} {_knob_id(knob)}: ratio {ratio:.3f} at {where}, mcc_rel {mcc:.2e}, kappa {ref.kappa:.2e}")
    assert ratio <= C_TOL, (ratio, where, ref.kappa)
    assert mcc <= 1e-12
