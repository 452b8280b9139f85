"""The iterative linear solver of rsba_solve (rsba_set_linear_solver type 1: block-Jacobi preconditioned conjugate gradients on the
reduced camera system) against the host reference of tests/pcg_reference.py, on the smallest shapes of tests/lm_step_cases.py at
which its kernels can go wrong: tile edges and a partial last tile (rs_Fp1, rs_F2p1), five tiles with an off-diagonal tile used in
both directions (rs_far_pair), pseudo tiles of intrinsics blocks beside a partial tile (gs_intr_run3), a shared intrinsics block,
Huber, a constant frame, 25 row tiles with uneven tile lists (rs_nt25), motion priors at a constant ratio across a tile edge
(rs_prior_Fp1), GoodPosePriors with the SphericalPrior (rs_spherical_pp).

Units.  R.step_ratio measures a step, per parameter block, in kappa * 2^-53 * |delta_ref|_inf (kappa of the scaled, damped matrix,
beyond two ulps of x for the rounding of x0 + delta).

C_ITER (early iterates: the step after k = 1, 2, 3 CG iterations against the step that follows from the long-double y_k) is 4 x the
worst distance of the fp64 numpy restatement from the long-double one on these cases, measured on the CPU:
    case             k=1      k=2      k=3        case             k=1      k=2      k=3
    rs_Fp1           0.0077   0.0196   0.0322     rs_huber         0.167    0.454    0.495
    rs_F2p1          0.0051   0.0113   0.0144     rs_const_frame   0.052    0.138    0.154
    rs_far_pair      0.0031   0.0102   0.0149     rs_nt25          0.0008   0.0059   0.0062
    gs_intr_run3     0.0234   0.0739   0.0749     rs_prior_Fp1     0.0153   0.0278   0.0416
    rs_intr_shared   0.0295   0.0332   0.0638     rs_spherical_pp  0.123    1.9e10   1.8e9
rs_spherical_pp is taken on its own.  Its right-hand side carries three entries of 1e20 (the SphericalPrior's weight times a residual
of 0.9997) beside entries of order 1e3: after the first iteration the recurrence r -= alpha q leaves 1e20 * 2^-53 = 1e4 of rounding in
those three rows, more than everything the other rows hold, and NO fp64 conjugate-gradient recurrence resolves the rest of the step
(the restatement misses the long-double iterate by 1.9e10 units at k = 2 and its converged step misses lm_step's by 5.9e10; the exact
solver's elimination is immune because its errors are relative to each pivot).  One constant over all ten cases would be 7.7e10 and
would let every seeded error of tests/test_pcg_reference.py through, so the rule "4 x the restatement's worst" is applied twice:
C_ITER = 4 x 0.4951 = 1.98 from the nine cases an fp64 recurrence can follow, which is the bound for them and for k = 1 of
rs_spherical_pp (0.123), and C_ITER_SPHERICAL = 4 x 1.934e10, C_PCG_SPHERICAL = 4 x 5.862e10 from rs_spherical_pp itself for its
k = 2, 3 and its converged step — nowhere wider than the single constant, and saying no more about that case than fp64 allows.

C_PCG (converged step against lm_step's): N_CASE iterations with both tests off, N_CASE = the first iteration at which the fp64
restatement's error against LMStep.y is within a factor 2 of the smallest it ever reaches (it has stopped falling), plus 10.  The
restatement's step is then within 0.16 - 4.4 units (worst: rs_intr_shared); 4 x 4.4 = 17.7 is below the exact solver's
C_TOL = 64, so C_PCG = 64.

Stopping rule: the long-double reference stops at the same iteration for every case, with min_iterations 1 (2 - 4 iterations) and 3
(3 - 4); its criterion value at the stopping iteration is nowhere within 1e-6 relative of eta (the nearest: 0.1044 at k = 2 of
rs_F2p1, which goes on to k = 3), so no case may take the +-1 branch.

Whole solves (checked on the CPU with an inexact-LM loop over the restatement: Jacobi scales re-estimated per iteration, otherwise the
rules of rsba_solve): 12 frames 23 LM iterations, 582 CG iterations, at most 46 per solve; 30 frames with Huber 23 LM iterations,
1040 CG iterations, at most 80 — no solve reaches the cap of 500, both end within 4e-12 relative of the oracle's minimum (13 and 10
iterations of the exact solver).

Measured on an MI355X (every test prints its figure on a line that starts with PCGFIG before it asserts):
    early iterates   k=1      k=2      k=3        case             k=1      k=2      k=3
    rs_Fp1           0.0028   0.0068   0.0163     rs_huber         0.251    0.255    0.295
    rs_F2p1          0.0032   0.0073   0.0085     rs_const_frame   0.052    0.083    0.131
    rs_far_pair      0.0019   0.0045   0.0052     rs_nt25          0.0017   0.0031   0.0029
    gs_intr_run3     0.0148   0.0148   0.0113     rs_prior_Fp1     0.0031   0.0052   0.0101
    rs_intr_shared   0.0103   0.0105   0.0108     rs_spherical_pp  0.117    3.0e10   2.0e10
model_cost_change within 2.6e-15 relative everywhere.  Converged step: 0.056 - 0.28 units, rs_intr_shared 2.17, rs_spherical_pp 5.864e10
(its restatement: 5.862e10; bound 2.3e11).  Stopping rule: the device's count equals the reference's in all twenty runs (2 - 4 iterations).
Whole solves: 12 frames 24 LM iterations, 581 CG iterations at eta = 0.1 against 933 at r_tolerance 1e-13; 30 frames with Huber 26 and
1203 against 1274; no solve at the cap; final costs within 5e-12 relative of the oracle's.

The early iterates and the stopped steps of rs_intr_shared RAISE the cost (relative decrease of the reference's own y_1, y_2, y_3 on the
CPU: -8.7, -4.7, -3.0; the converged step lowers it), so LM rejects them, rightly, and x does not move.  The tests that read the step
from x1 - x0 therefore run with min_relative_decrease = -1e300: every valid step is applied, whatever it does to the cost.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lm_step_cases as LC
import lm_step_reference as R
import pcg_reference as PR
from test_lm_step_reference import C_TOL

CASES = ["rs_Fp1", "rs_F2p1", "rs_far_pair", "gs_intr_run3", "rs_intr_shared", "rs_huber", "rs_const_frame", "rs_nt25", "rs_prior_Fp1",
         "rs_spherical_pp"]
C_ITER = 4 * 0.49513741098098424
C_PCG = C_TOL
C_ITER_SPHERICAL, C_PCG_SPHERICAL = 4 * 1.9338035978791870e10, 4 * 5.8622471245605160e10


def c_iter(name, k):
    return C_ITER_SPHERICAL if name == "rs_spherical_pp" and k >= 2 else C_ITER


def c_pcg(name):
    return C_PCG_SPHERICAL if name == "rs_spherical_pp" else C_PCG
# first iteration at which the fp64 restatement's error is within a factor 2 of its floor, plus 10 (tools: tests/pcg_reference.py)
N_CASE = {"rs_Fp1": 47, "rs_F2p1": 65, "rs_far_pair": 82, "gs_intr_run3": 325, "rs_intr_shared": 99, "rs_huber": 43, "rs_const_frame": 52,
          "rs_nt25": 410, "rs_prior_Fp1": 56, "rs_spherical_pp": 12}
OFF = dict(eta=0.0, r_tolerance=-1.0)          # both stopping tests off: the cap ends the solve
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    assert capi.device_count() >= 1
    return capi


_REF = {}


def reference(oracle, name):
    """(problem, options, LMStep, Reduced in long double, StepMaker, the first iterates in long double) of a case: computed once, shared."""
    if name not in _REF:
        p, opts = LC.case(name)
        r, J, ok = oracle.evaluate_blocks(p)
        assert ok.all()
        ref = R.lm_step(p, r, J, **{k: opts[k] for k in ("initial_trust_region_radius",) if k in opts})
        red = PR.reduce_system(p, ref)
        _REF[name] = (p, opts, ref, red, PR.StepMaker(p, r, J, ref), PR.pcg(red, max_iterations=3, **OFF))
    return _REF[name]


ANY_DECREASE = -1e300


def device_step(capi, p, opts, min_relative_decrease=None, **linear):
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG, **linear)
        o = capi.default_options(**opts)
        if min_relative_decrease is not None:
            o.min_relative_decrease = min_relative_decrease
        s, tr = dp.solve(o)
        st = dp.linear_solver_stats()
    assert len(tr) == 2 and tr[1].step_is_valid == 1 and tr[1].step_is_successful == 1, (len(tr), tr[-1].step_is_valid, tr[-1].step_is_successful)
    return q, tr, st


@gpu
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", CASES)
def test_early_iterates(capi, oracle, name, k):
    p, opts, ref, red, sm, run = reference(oracle, name)
    # an iterate after k CG iterations need not lower the cost (the reference's own y_1 .. y_3 of rs_intr_shared raise it: relative
    # decrease -8.7, -4.7, -3.0 on the CPU) and LM is right to reject it; the step is what is under test here, so every valid one is applied
    q, tr, st = device_step(capi, p, opts, min_relative_decrease=ANY_DECREASE, max_iterations=k, **OFF)
    assert st["last_iterations"] == k and st["num_linear_solves"] == 1 and st["num_solves_at_cap"] == 1 and st["num_failed_solves"] == 0, st
    want = sm.step(PR.full_solution(red, ref, run.y[k]))
    ratio, where = R.step_ratio(p, want, *R.solved_blocks(q))
    rel = abs(tr[1].model_cost_change - want.model_cost_change) / abs(want.model_cost_change)
    print(f"PCGFIG early {name} k={k} ratio {ratio:.4g} at {where} mcc_rel {rel:.3g} kappa {ref.kappa:.3g}")
    assert ratio <= c_iter(name, k), (ratio, where, ref.kappa)
    assert rel <= 1e-12, (tr[1].model_cost_change, want.model_cost_change)


@gpu
@pytest.mark.parametrize("name", CASES)
def test_converged_step(capi, oracle, name):
    p, opts, ref, red, sm, run = reference(oracle, name)
    q, tr, st = device_step(capi, p, opts, eta=0.0, r_tolerance=0.0, max_iterations=N_CASE[name])
    ratio, where = R.step_ratio(p, ref, *R.solved_blocks(q))
    print(f"PCGFIG converged {name} N={N_CASE[name]} iterations {st['last_iterations']} ratio {ratio:.4g} at {where} residual {st['last_relative_residual']:.3g}")
    assert st["num_failed_solves"] == 0
    assert ratio <= c_pcg(name), (ratio, where, ref.kappa)


def camera_y(p, ref, red, q):
    """The camera-side y of the step a solve applied: -(x1 - x0) / scale over the unknowns of red.cam, in long double."""
    d = np.concatenate([(q.poses - p.poses).ravel(), np.zeros(0) if p.calibrated else (q.intrinsics - p.intrinsics).ravel()])
    return -(d[np.asarray(ref.free)[red.cam]].astype(PR.LD)) / ref.scale[red.cam].astype(PR.LD)


@gpu
@pytest.mark.parametrize("min_iterations", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_stopping_rule(capi, oracle, name, min_iterations):
    p, opts, ref, red, sm, _ = reference(oracle, name)
    eta = 0.1
    run = PR.pcg(red, min_iterations=min_iterations, eta=eta)
    assert run.reason == "test"
    n = run.iterations
    near = any(abs(float(run.zeta[k]) - eta) <= 1e-6 * eta for k in range(max(min_iterations, 1), n + 1))
    assert not near                              # (chosen so on the CPU: the count is exact for every case)
    q, tr, st = device_step(capi, p, opts, min_relative_decrease=ANY_DECREASE, min_iterations=min_iterations)   # (y is read from x1 - x0: the step has to be applied, see test_early_iterates)
    print(f"PCGFIG stop {name} min={min_iterations} device {st['last_iterations']} reference {n} zeta {float(run.zeta[n]):.4g}")
    assert st["last_iterations"] == n, (st, n, [float(z) for z in run.zeta[1:]])
    assert st["num_solves_at_cap"] == 0 and st["num_failed_solves"] == 0
    # the step the device returned satisfies the stopping inequality, evaluated in long double (Q_k-1: the reference's)
    y = camera_y(p, ref, red, q)
    res = red.rhs - red.S @ y
    Q = PR.LD(-0.5) * np.dot(y, red.rhs + res)
    zeta = n * (Q - run.Q[n - 1]) / Q
    assert zeta < eta, (float(zeta), n)
    rel = float(np.sqrt(np.dot(res, res) / np.dot(red.rhs, red.rhs)))
    assert abs(st["last_relative_residual"] - rel) <= 1e-6 * rel + 1e-9, (st["last_relative_residual"], rel)   # (y is known through x1 - x0 only: ulps of x)


def bits(q):
    return [a.tobytes() for a in (q.poses, q.points, q.intrinsics)] + [None if q.pose_prior_values is None else q.pose_prior_values.tobytes()]


def trace_bits(tr):
    return [ctypes.string_at(ctypes.addressof(t), ctypes.sizeof(t)) for t in tr]


@gpu
@pytest.mark.parametrize("name", CASES)
def test_two_solves_are_bit_equal(capi, name):
    p, opts = LC.case(name)
    opts = dict(opts, max_num_iterations=3)
    got = []
    for _ in range(2):
        q = p.copy()
        with capi.DeviceProblem(q) as dp:
            dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG)
            s, tr = dp.solve(capi.default_options(**opts))
            got.append((bits(q), trace_bits(tr), dp.linear_solver_stats(), s.final_cost))
    assert got[0] == got[1]
    assert got[0][2]["total_iterations"] > 0


# ---- whole solves -------------------------------------------------------------------------------------------------------------

def whole_scene(frames, huber):
    from rsba_amd.problem import apply_gauge_masks
    from rsba_amd.scene import make_scene
    # (no seeded outliers: with any, the exact solver itself is still creeping after 100 iterations at function_tolerance 1e-12 and has
    # no minimum to compare with; Huber at a = 2 acts on the tails of the 0.5 px noise)
    p = make_scene(frames, 40 * frames, rolling=True, seed=71 + frames).problem
    apply_gauge_masks(p, fix_first_n_cameras=1)
    p.pose_fixed_mask[-1, -1] |= 0b111000
    if huber:
        p.huber_a = 2.0
    return p


@gpu
@pytest.mark.parametrize("frames,huber", [(12, False), (30, True)])
def test_whole_solves(capi, oracle, frames, huber):
    """Inexact steps end at the oracle's minimum; with a tight residual tolerance the iteration costs are the exact solver's."""
    p = whole_scene(frames, huber)
    po = p.copy()
    so, tro = oracle.solve(po, oracle.default_options(max_num_iterations=100, function_tolerance=1e-12))
    qt = p.copy()
    with capi.DeviceProblem(qt) as dp:
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG, eta=0.0, r_tolerance=1e-13, max_iterations=2000)
        st_, trt = dp.solve(capi.default_options(max_num_iterations=100, function_tolerance=1e-12))
        tight = dp.linear_solver_stats()
    assert len(trt) >= 6 and len(tro) >= 6
    for k in range(6):                            # the initial cost and the first five iterations (SURVEY protocol C.6 (b))
        assert abs(trt[k].cost - tro[k].cost) <= 1e-9 * tro[k].cost, (k, trt[k].cost, tro[k].cost)
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG)
        s, tr = dp.solve(capi.default_options(max_num_iterations=100, function_tolerance=1e-12))
        loose = dp.linear_solver_stats()
    print(f"PCGFIG whole F={frames} huber={huber} oracle {so.final_cost:.12e} ({so.num_iterations} it) tight {st_.final_cost:.12e} ({st_.num_iterations} it, CG {tight['total_iterations']}) "
          f"eta=0.1 {s.final_cost:.12e} ({s.num_iterations} it, CG {loose['total_iterations']}, cap {loose['num_solves_at_cap']})")
    assert abs(s.final_cost - so.final_cost) <= 1e-6 * so.final_cost, (s.final_cost, so.final_cost)
    assert abs(st_.final_cost - so.final_cost) <= 1e-6 * so.final_cost, (st_.final_cost, so.final_cost)
    assert 0 < loose["total_iterations"] < tight["total_iterations"], (loose, tight)
    assert loose["num_failed_solves"] == 0 and tight["num_failed_solves"] == 0


# ---- refusals and neutrality ----------------------------------------------------------------------------------------------------

UNSUPPORTED = 6


@gpu
@pytest.mark.parametrize("what", ["free_ratio", "exchange", "levels"])
def test_refusals_leave_the_handle_usable(capi, what):
    from rsba_amd.distributed import ALLREDUCE_FN
    p, opts = LC.case("rs_vel_free" if what == "free_ratio" else "rs_Fp1")
    q, plain = p.copy(), p.copy()
    with capi.DeviceProblem(plain) as dp:
        s_plain, _ = dp.solve(capi.default_options(**opts))
    with capi.DeviceProblem(q) as dp:
        if what == "exchange":                   # the callback form on one rank: never called for a sum over one rank's share
            cb = ALLREDUCE_FN(lambda ctx, buf, count, op, stream: 0)
            capi._check(capi.lib().rsba_set_exchange(dp._h, cb, None, ctypes.c_int32(0), ctypes.c_int32(1)))
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG)
        o = capi.default_options(**opts)
        if what == "levels":
            o.level_scheduled_cholesky = 1
        with pytest.raises(capi.RsbaError) as e:
            dp.solve(o)
        assert e.value.status == UNSUPPORTED and "iterative linear solver" in str(e.value)
        assert bits(q) == bits(p)                # nothing was touched
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_EXACT)
        s_after, _ = dp.solve(o)
        assert dp.linear_solver_stats()["num_linear_solves"] == 0
    assert abs(s_after.final_cost - s_plain.final_cost) <= 1e-9 * s_plain.final_cost
    if what == "free_ratio":                     # (the same handle set-up as the plain one: the same bits; an exchange or the level schedule take other launches)
        assert bits(q) == bits(plain)


@gpu
@pytest.mark.parametrize("name", ["rs_F2p1", "gs_intr_run3"])
def test_exact_solver_is_untouched_by_the_option(capi, name):
    """A handle set to the iterative solver and back gives the bits of one that never heard of it — also after it has solved with it."""
    p, opts = LC.case(name)
    opts = dict(opts, max_num_iterations=4)
    plain = p.copy()
    with capi.DeviceProblem(plain) as dp:
        s0, tr0 = dp.solve(capi.default_options(**opts))
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG, eta=0.01)
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_EXACT)
        s1, tr1 = dp.solve(capi.default_options(**opts))
    assert bits(q) == bits(plain) and trace_bits(tr1) == trace_bits(tr0)
    q = p.copy()
    with capi.DeviceProblem(q) as dp:
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_PCG)
        dp.solve(capi.default_options(**opts))
        assert dp.linear_solver_stats()["total_iterations"] > 0
        for a, b in zip((q.poses, q.points, q.intrinsics), (p.poses, p.points, p.intrinsics)):
            a[...] = b
        dp.upload_parameters()
        dp.set_linear_solver(type=capi.LINEAR_SOLVER_EXACT)
        s2, tr2 = dp.solve(capi.default_options(**opts))
        assert dp.linear_solver_stats()["total_iterations"] == 0
    assert bits(q) == bits(plain) and trace_bits(tr2) == trace_bits(tr0)


# ---- the facade ---------------------------------------------------------------------------------------------------------------

def _facade_result(path, p):
    raw = np.fromfile(path, dtype=np.float64)
    npose, npt = p.poses.size, p.points.size
    assert raw.size == 7 + npose + npt
    return dict(initial_cost=raw[0], final_cost=raw[1], iterations=int(raw[2]), usable=raw[5] == 1.0, linear_iterations=int(raw[6]),
                poses=raw[7:7 + npose], points=raw[7 + npose:])


@gpu
def test_facade_routes_iterative_schur_and_only_that(oracle, tmp_path):
    """ceres::Solve through the facade: ITERATIVE_SCHUR reports conjugate-gradient iterations and ends at the oracle's cost;
    SPARSE_SCHUR reports none and returns what BA() (examples/ba_session, SPARSE_SCHUR with the same options) returns, bit for bit."""
    import __graft_entry__ as G
    from helpers import read_result_file, write_scene_file
    from rsba_amd.problem import apply_gauge_masks
    from rsba_amd.scene import make_scene
    exe, ba = os.path.join(ROOT, "examples", "iterative_schur"), os.path.join(ROOT, "examples", "ba_session")
    if not (os.path.exists(exe) and os.path.exists(ba)):
        G.build()
    p = make_scene(14, 500, rolling=True, seed=41).problem
    write_scene_file(tmp_path / "s.bin", p, fix_first_n=1, max_iter=20)
    runs = {}
    for kind in ("ITERATIVE_SCHUR", "SPARSE_SCHUR"):
        r = subprocess.run([exe, str(tmp_path / "s.bin"), str(tmp_path / f"{kind}.bin"), kind], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        runs[kind] = _facade_result(tmp_path / f"{kind}.bin", p)
        assert ("ITERATIVE_SCHUR" in r.stdout) == (kind == "ITERATIVE_SCHUR")
    r = subprocess.run([ba, str(tmp_path / "s.bin"), str(tmp_path / "ba.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    today = read_result_file(tmp_path / "ba.bin", p)
    exact, pcg = runs["SPARSE_SCHUR"], runs["ITERATIVE_SCHUR"]
    assert exact["linear_iterations"] == 0 and pcg["linear_iterations"] > 0
    assert exact["final_cost"] == today["final_cost"] and exact["iterations"] == today["iterations"]
    assert np.array_equal(exact["poses"], today["poses"].ravel()) and np.array_equal(exact["points"], today["points"].ravel())
    q = p.copy()
    apply_gauge_masks(q, fix_first_n_cameras=1)
    s_ref, _ = oracle.solve(q, oracle.default_options(max_num_iterations=20))
    # 20 LM iterations of inexact steps at function_tolerance 1e-6 (BA's options) promise a usable solution below the initial cost and
    # not below the minimum (the oracle's, itself converged to 1e-6), no more: the inexact whole solves above take 24 - 26 iterations
    # to the minimum at function_tolerance 1e-12, and that contract is test_whole_solves'
    print(f"PCGFIG facade initial {pcg['initial_cost']:.9e} ITERATIVE_SCHUR {pcg['final_cost']:.9e} ({pcg['iterations']} it, CG {pcg['linear_iterations']}) "
          f"SPARSE_SCHUR {exact['final_cost']:.9e} ({exact['iterations']} it) oracle {s_ref.final_cost:.9e}")
    assert pcg["usable"] and s_ref.final_cost * (1 - 1e-6) <= pcg["final_cost"] < pcg["initial_cost"], (pcg["final_cost"], s_ref.final_cost, pcg["initial_cost"])
