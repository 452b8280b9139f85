"""The losses beyond Huber on the device (rsba_set_loss; the rule: include/rsba_amd.h) against the host reference of
tests/loss_reference.py: cost and gradient, the first LM step, whole solves, both forms of the trust-region loop, neutrality for
problems that do not ask for a loss, and the facade's lowering.

Scenes (tests/lm_step_cases.py): rs_huber (9 two-pose frames, 10 % outliers), rs_Fp1, gs_F2p1 (one pose per frame), rs_intr_shared
(the 24-column block), rs_intr_perframe (the path that keeps records), rs_acc_free (motion priors — 12-vectors under the loss — and a
free ratio).  Losses: SOFT_L_ONE(10), CAUCHY(10), ARCTAN(100), TOLERANT(150, 50), TOLERANT(100, 25); on rs_huber also CAUCHY(10) at
scale 0.25.  Every (scene, loss) has at least 5 % of its blocks at rho1 < 0.5 and 5 % at rho1 > 0.9, and TOLERANT has rho2 > 1e-6 on
at least half of them: conditions on the cases, asserted.

Bounds: cost and gradient 1e-12 relative (the project's parity bound for residuals); the step C_TOL = 64 units of kappa eps |delta_ref|
per parameter block (test_lm_step_reference.C_TOL: a plain fp64 direct solve of the same system sits 0.012 - 0.84 units from the
reference), model_cost_change 1e-12 and gradient_max_norm 1e-13 relative; iteration costs of whole solves 1e-9 relative (the
project's trajectory bound).

Measured on an MI355X, worst over the 31 (scene, loss) pairs: cost 5.7e-16, gradient 1.9e-15, cost of the golden observations
3.7e-16, model_cost_change 2.2e-15, gradient_max_norm 8.1e-16 (all relative); the step 1.67 units (rs_intr_shared SOFT_L_ONE, the
intrinsics block, kappa 7.2e4), with TOLERANT (the rank-one branch) 0.04 - 0.21.  On the host: rho1 < 0.5 on 6 - 75 % and rho1 > 0.9 on 6 - 53 %
of every pair's blocks, TOLERANT's rho2 > 1e-6 on 77 - 99.6 % (rs_intr_perframe: 11 - 74 %, 13 - 35 %, 92.5 - 98.3 %); the reference
loop of the two whole solves has no decision within 1e-6 of min_relative_decrease (rs_huber CAUCHY(10): one rejected step, at
relative_decrease -0.14; rs_acc_free TOLERANT(100, 25): none, converged by function_tolerance at iteration 9)."""
import ctypes
import os
import subprocess

import mpmath
import numpy as np
import pytest

import lm_step_cases as LC
import lm_step_reference as R
import loss_reference as L
from helpers import batch_cases, load_golden
from test_lm_step_reference import C_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENES = ["rs_huber", "rs_Fp1", "gs_F2p1", "rs_intr_shared", "rs_intr_perframe", "rs_acc_free"]
LOSSES = {"soft10": L.loss(L.SOFT_L_ONE, 10), "cauchy10": L.loss(L.CAUCHY, 10), "arctan100": L.loss(L.ARCTAN, 100),
          "tol150_50": L.loss(L.TOLERANT, 150, 50), "tol100_25": L.loss(L.TOLERANT, 100, 25)}
SCALED = L.loss(L.CAUCHY, 10, scale=0.25)
PAIRS = [(s, k) for s in SCENES for k in LOSSES] + [("rs_huber", "cauchy10_x0.25")]
ANY_DECREASE = -1e300      # min_relative_decrease: the step is applied whatever it does to the cost (as tests/test_gpu_pcg.py)
INVALID_ARGUMENT = 1


def the_loss(key):
    return SCALED if key == "cauchy10_x0.25" else LOSSES[key]


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    assert capi.device_count() >= 1
    return capi


_scene_cache = {}


def scene(oracle, name):
    """(problem with no loss of its own, solver options, raw residuals, raw Jacobians) — evaluated once per module, never changed"""
    if name not in _scene_cache:
        p, opts = LC.case(name)
        p.huber_a = 0.0
        r, J, ok = oracle.evaluate_blocks(p)
        assert ok.all()
        _scene_cache[name] = (p, opts, r, J)
    return _scene_cache[name]


def set_loss(dp, loss):
    dp.set_loss(type=loss[0], a=loss[1], b=loss[2], scale=loss[3])


def regimes(p, r, loss):
    """The blocks' rho1 and rho2 at the first linearisation: observations and the 12-vectors of the motion priors."""
    s = [np.sum(np.asarray(r, dtype=np.float64) ** 2, axis=1)]
    for rp, _, _, takes in R.prior_blocks(p):
        if takes:
            s.append(np.sum(rp.astype(np.float64).reshape(rp.shape[0], -1) ** 2, axis=1))
    _, r1, r2 = L.rho(loss, np.concatenate(s))
    return r1 / loss[3], r2 / loss[3]


@pytest.mark.parametrize("name,key", PAIRS)
def test_cases_reach_both_regimes(oracle, name, key):
    """(needs no device; kept here with the cases it is about)"""
    p, _, r, _ = scene(oracle, name)
    loss = the_loss(key)
    r1, r2 = regimes(p, r, loss)
    print(f"{name} {key}: rho1 < 0.5 on {np.mean(r1 < 0.5):.3f}, rho1 > 0.9 on {np.mean(r1 > 0.9):.3f}, rho2 > 1e-6 on {np.mean(r2 > 1e-6):.3f}")
    assert np.mean(r1 < 0.5) >= 0.05 and np.mean(r1 > 0.9) >= 0.05
    if loss[0] == L.TOLERANT:
        assert np.mean(r2 > 0) >= 0.5


def device_gradient(p, out):
    """rsba_evaluate's gradient in the global numbering of lm_step_reference.columns (no entry for the ratio or priorPoses blocks)."""
    Lo = R.layout(p)
    g = np.zeros(Lo["nparam"])
    F, P = p.num_frames, p.poses_per_frame
    g[: F * 6 * P] = out["gradient"]["poses"].reshape(-1)
    if not p.calibrated:
        g[Lo["intr"]: Lo["intr"] + 9 * p.num_intrinsics] = out["gradient"]["intrinsics"].reshape(-1)
    g[Lo["ncam"]:] = out["gradient"]["points"].reshape(-1)
    return g


@pytest.mark.parametrize("name,key", PAIRS)
def test_cost_and_gradient(capi, oracle, name, key):
    p, _, r, J = scene(oracle, name)
    loss = the_loss(key)
    cost, grad = L.cost_and_gradient(p, r, J, loss)
    with capi.DeviceProblem(p.copy()) as dp:
        set_loss(dp, loss)
        out = dp.evaluate(residuals=False, jacobians=False, gradient=True)
    got = device_gradient(p, out)
    _, _, _, fixed = R.columns(p)
    Lo = R.layout(p)
    keep = ~fixed
    if Lo["iratio"] >= 0:                         # the ratio has no entry in rsba_evaluate's gradient
        keep[Lo["iratio"]] = False
    want = grad.astype(np.float64)
    gerr = float(np.max(np.abs(got[keep] - grad[keep]))) / float(np.max(np.abs(want[keep])))
    cerr = abs(out["cost"] - float(cost)) / float(cost)
    print(f"{name} {key}: cost {out['cost']:.15e} (reference {float(cost):.15e}, relative error {cerr:.2e})")
    print(f"{name} {key}: gradient relative error {gerr:.2e}")
    assert cerr <= 1e-12
    assert gerr <= 1e-12


def mp_rho0(loss, s):
    kind, a, b, scale = loss
    a, b, s = mpmath.mpf(a), mpmath.mpf(b), mpmath.mpf(s)
    if kind == L.SOFT_L_ONE:
        v = 2 * a * a * (mpmath.sqrt(1 + s / (a * a)) - 1)
    elif kind == L.CAUCHY:
        v = a * a * mpmath.log(1 + s / (a * a))
    elif kind == L.ARCTAN:
        v = a * mpmath.atan2(s, a)
    else:
        c = b * mpmath.log(1 + mpmath.exp(-a / b))
        v = s - a - c if (s - a) / b > mpmath.mpf("36.7") else b * mpmath.log(1 + mpmath.exp((s - a) / b)) - c
    return scale * v


@pytest.mark.parametrize("key", list(LOSSES) + ["cauchy10_x0.25"])
def test_cost_of_the_golden_observations(capi, key):
    """The cost-only site of the raw evaluation on the inputs of tests/golden/per_observation.json (as test_gpu_eval.py batches
    them), against sum rho0 / 2 of the goldens' residuals in mpmath."""
    loss = the_loss(key)
    cases = load_golden("per_observation.json")
    mpmath.mp.dps = 50
    for prob, idxs in batch_cases(cases):
        want = sum(mp_rho0(loss, mpmath.mpf(cases[i]["residual"][0]) ** 2 + mpmath.mpf(cases[i]["residual"][1]) ** 2) for i in idxs if cases[i]["ok"]) / 2
        with capi.DeviceProblem(prob) as dp:
            set_loss(dp, loss)
            out = dp.evaluate(residuals=False, jacobians=False)
        err = float(abs(out["cost"] - want) / want)
        print(f"{key}: {len(idxs)} golden observations, cost {out['cost']:.15e}, relative error {err:.2e}")
        assert err <= 1e-12


@pytest.mark.parametrize("name,key", PAIRS)
def test_first_lm_step(capi, oracle, name, key):
    p, opts, r, J = scene(oracle, name)
    loss = the_loss(key)
    ref = L.lm_step(p, r, J, loss, **{k: opts[k] for k in ("initial_trust_region_radius",) if k in opts})
    assert ref.kappa <= 1e9, ref.kappa
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        set_loss(dp, loss)
        o = capi.default_options(**opts)
        o.min_relative_decrease = ANY_DECREASE
        s, tr = dp.solve(o)
        ratio1 = dp.inter_frame_ratio() if R.layout(p)["iratio"] >= 0 else float(q.inter_frame_ratio)
    assert len(tr) == 2 and tr[1].step_is_valid == 1 and tr[1].step_is_successful == 1
    ratio, where = R.step_ratio(p, ref, q.poses, q.points, q.intrinsics, ratio1, q.pose_prior_values)
    mcc = abs(tr[1].model_cost_change - ref.model_cost_change) / abs(ref.model_cost_change)
    gmx = abs(tr[0].gradient_max_norm - ref.gradient_max_norm) / ref.gradient_max_norm
    print(f"{name} {key}: step ratio {ratio:.3f} at {where}, kappa {ref.kappa:.2e}")
    print(f"{name} {key}: model_cost_change relative error {mcc:.2e}")
    print(f"{name} {key}: gradient_max_norm relative error {gmx:.2e}")
    assert ratio <= C_TOL, (ratio, where, ref.kappa)
    assert mcc <= 1e-12
    assert gmx <= 1e-13


WHOLE = [("rs_huber", "cauchy10"), ("rs_acc_free", "tol100_25")]
WHOLE_OPTS = dict(max_num_iterations=15)


def whole_opts(opts):
    return dict({k: v for k, v in opts.items() if k == "initial_trust_region_radius"}, **WHOLE_OPTS)


def bits(q):
    return [a.tobytes() for a in (q.poses, q.points, q.intrinsics)]


def trace_bits(tr):
    return [ctypes.string_at(ctypes.addressof(t), ctypes.sizeof(t)) for t in tr]


def summary_bits(s):
    return (s.termination_type, s.num_successful_steps, s.num_unsuccessful_steps, s.num_iterations, s.initial_cost, s.final_cost, s.fixed_cost)


@pytest.mark.parametrize("name,key", WHOLE)
def test_whole_solves_follow_the_reference_loop(capi, oracle, name, key):
    p, opts, _, _ = scene(oracle, name)
    loss = the_loss(key)
    o = whole_opts(opts)
    want, _ = L.lm_loop(oracle, p, loss, **o)
    for t in want[1:]:                                  # a precondition of the case: no decision on the edge of its threshold
        assert abs(t["relative_decrease"] - 1e-3) > 1e-6, t
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        set_loss(dp, loss)
        s, tr = dp.solve(capi.default_options(**o))
    print(f"{name} {key}: {len(tr) - 1} iterations (reference {len(want) - 1}), final cost {s.final_cost:.12e} (reference {want[-1]['cost']:.12e})")
    assert len(tr) == len(want)
    for t, w in zip(tr, want):
        print(f"  iteration {t.iteration}: accepted {t.step_is_successful} (reference {w['step_is_successful']}), cost {t.cost:.12e}, relative error {abs(t.cost - w['cost']) / w['cost']:.2e}")
        assert t.step_is_successful == w["step_is_successful"]
        assert abs(t.cost - w["cost"]) <= 1e-9 * w["cost"]


@pytest.mark.parametrize("name,key", WHOLE)
def test_host_and_device_form_of_the_loop_agree(capi, oracle, monkeypatch, name, key):
    p, opts, _, _ = scene(oracle, name)
    loss = the_loss(key)
    got = []
    for form in ("1", "0"):
        monkeypatch.setenv("RSBA_DEVICE_LM", form)
        q = p.copy()
        with capi.DeviceProblem(q) as dp:
            set_loss(dp, loss)
            s, tr = dp.solve(capi.default_options(**whole_opts(opts)))
            got.append((bits(q), trace_bits(tr), summary_bits(s), dp.inter_frame_ratio() if p.prior_kind else 0.0))
    assert got[0] == got[1]
    assert len(got[0][1]) > 3


def test_huber_through_set_loss_is_the_handle_created_with_it(capi):
    p, opts = LC.case("rs_huber")
    assert p.huber_a == 2.0
    o = dict(opts, max_num_iterations=8)
    a = p.copy()
    with capi.DeviceProblem(a) as dp:
        assert dp.loss() == dict(type=capi.LOSS_HUBER, a=2.0, b=0.0, scale=1.0)
        sa, ta = dp.solve(capi.default_options(**o))
    b = p.copy()
    b.huber_a = 0.0
    with capi.DeviceProblem(b) as dp:
        assert dp.loss() == dict(type=capi.LOSS_TRIVIAL, a=0.0, b=0.0, scale=1.0)
        dp.set_loss(type=capi.LOSS_HUBER, a=2.0)
        assert dp.loss() == dict(type=capi.LOSS_HUBER, a=2.0, b=0.0, scale=1.0)
        sb, tb = dp.solve(capi.default_options(**o))
    assert len(ta) > 3
    assert bits(a) == bits(b) and trace_bits(ta) == trace_bits(tb) and summary_bits(sa) == summary_bits(sb)


def test_trivial_through_set_loss_is_no_call_at_all(capi):
    p, opts = LC.case("rs_Fp1")
    o = dict(opts, max_num_iterations=5)
    a, b = p.copy(), p.copy()
    with capi.DeviceProblem(a) as dp:
        sa, ta = dp.solve(capi.default_options(**o))
    with capi.DeviceProblem(b) as dp:
        dp.set_loss(type=capi.LOSS_CAUCHY, a=10.0)
        dp.set_loss(type=capi.LOSS_TRIVIAL)
        sb, tb = dp.solve(capi.default_options(**o))
    assert bits(a) == bits(b) and trace_bits(ta) == trace_bits(tb) and summary_bits(sa) == summary_bits(sb)


@pytest.mark.parametrize("name", ["rs_huber", "rs_acc_r1.25"])
def test_set_loss_between_two_solves_takes_effect(capi, name):
    """One handle: a solve under TOLERANT (dense prior cross blocks where there are priors), the parameters put back, the loss taken
    away, a second solve — the bits of a handle that never had a loss; and the other way round."""
    p, opts = LC.case(name)
    p.huber_a = 0.0
    o = dict(opts, max_num_iterations=4)
    tol = dict(type=capi.LOSS_TOLERANT, a=100.0, b=25.0)

    def fresh(loss):
        q = p.copy()
        with capi.DeviceProblem(q) as dp:
            if loss:
                dp.set_loss(**loss)
            s, tr = dp.solve(capi.default_options(**o))
            return bits(q), trace_bits(tr), summary_bits(s)
    plain, robust = fresh(None), fresh(tol)
    assert plain[2][5] != robust[2][5]                    # the loss changes the solve
    for first, second, want in ((tol, None, plain), (None, tol, robust)):
        q = p.copy()
        with capi.DeviceProblem(q) as dp:
            dp.set_loss(**(first or dict(type=capi.LOSS_TRIVIAL)))
            dp.solve(capi.default_options(**o))
            for x, y in zip((q.poses, q.points, q.intrinsics), (p.poses, p.points, p.intrinsics)):
                x[...] = y
            dp.upload_parameters()
            dp.set_loss(**(second or dict(type=capi.LOSS_TRIVIAL)))
            s, tr = dp.solve(capi.default_options(**o))
            assert (bits(q), trace_bits(tr), summary_bits(s)) == want


def test_bad_arguments_are_refused_and_leave_the_loss(capi):
    p, _ = LC.case("rs_Fp1")
    with capi.DeviceProblem(p.copy()) as dp:
        dp.set_loss(type=capi.LOSS_CAUCHY, a=10.0, scale=0.25)
        kept = dp.loss()
        assert kept == dict(type=capi.LOSS_CAUCHY, a=10.0, b=0.0, scale=0.25)
        bad = [dict(type=capi.LOSS_CAUCHY, a=0.0), dict(type=capi.LOSS_CAUCHY, a=-1.0), dict(type=capi.LOSS_HUBER, a=float("nan")),
               dict(type=capi.LOSS_SOFT_L_ONE, a=float("inf")), dict(type=capi.LOSS_TOLERANT, a=1.0, b=0.0), dict(type=capi.LOSS_TOLERANT, a=1.0, b=float("nan")),
               dict(type=capi.LOSS_ARCTAN, a=1.0, scale=0.0), dict(type=capi.LOSS_TRIVIAL, scale=-2.0), dict(type=capi.LOSS_TRIVIAL, scale=float("inf")),
               dict(type=6, a=1.0), dict(type=-1, a=1.0)]
        for kw in bad:
            with pytest.raises(capi.RsbaError) as e:
                dp.set_loss(**kw)
            assert e.value.status == INVALID_ARGUMENT and "loss" in str(e.value), kw
            assert dp.loss() == kept
        dp.set_loss(type=capi.LOSS_TOLERANT, a=150.0, b=50.0)
        assert dp.loss() == dict(type=capi.LOSS_TOLERANT, a=150.0, b=50.0, scale=1.0)


# ---- the facade ---------------------------------------------------------------------------------------------------------------

def _facade(tmp_path, p, spec):
    import __graft_entry__ as G
    from helpers import write_scene_file
    exe = os.path.join(ROOT, "examples", "robust_loss")
    if not os.path.exists(exe):
        G.build()
    write_scene_file(tmp_path / "s.bin", p, fix_first_n=1, max_iter=12)
    return subprocess.run([exe, str(tmp_path / "s.bin"), str(tmp_path / "out.bin"), spec], capture_output=True, text=True), tmp_path / "out.bin"


@pytest.mark.parametrize("spec,loss", [("cauchy:10", L.loss(L.CAUCHY, 10)), ("scaled:0.5:tolerant:100:25", L.loss(L.TOLERANT, 100, 25, 0.5))])
def test_facade_lowers_the_loss(capi, tmp_path, spec, loss):
    from rsba_amd.problem import apply_gauge_masks
    from rsba_amd.scene import make_scene
    p = make_scene(14, 500, rolling=True, seed=41, outlier_ratio=0.1).problem
    r, out = _facade(tmp_path, p, spec)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.float64)
    q = p.copy()
    apply_gauge_masks(q, fix_first_n_cameras=1)
    with capi.DeviceProblem(q) as dp:
        set_loss(dp, loss)
        s, tr = dp.solve(capi.default_options(max_num_iterations=12))
    print(f"{spec}: facade final cost {raw[1]:.15e} ({int(raw[2])} records), C ABI {s.final_cost:.15e} ({len(tr)} records)")
    assert raw[5] == 1.0 and len(tr) > 3
    assert abs(raw[0] - s.initial_cost) <= 1e-12 * s.initial_cost
    assert abs(raw[1] - s.final_cost) <= 1e-12 * s.final_cost


@pytest.mark.parametrize("spec", ["user", "scaled:2:scaled:0.5:cauchy:10", "scaled:2:user"])
def test_facade_refuses_what_it_cannot_lower(tmp_path, spec):
    from rsba_amd.scene import make_scene
    p = make_scene(6, 120, rolling=True, seed=42).problem
    r, _ = _facade(tmp_path, p, spec)
    assert r.returncode == 1
    assert "unsupported loss function" in r.stderr and "CauchyLoss" in r.stderr and "ScaledLoss" in r.stderr
