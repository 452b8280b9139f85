"""The losses beyond Huber without a GPU: the table of include/rsba_amd.h against 50-digit goldens (tests/golden/losses.json, written
by tests/golden/make_loss_golden.py with mpmath: rho1 and rho2 there are numerical derivatives of rho0), in the numpy forms of
tests/loss_reference.py and in the Evaluate of the facade's classes; the corrector's identities; and that the bound of the device
step (tests/test_gpu_loss.py) sees a corrector without its rank-one branch and a wrong rho1.

Bounds: rho1 and rho2 within 16 eps relative, rho0 within 16 eps (|rho0| + K), eps = 2^-53 and K the constant the form subtracts or
scales by (2 a^2 SOFT_L_ONE, a^2 CAUCHY and HUBER, a ARCTAN, b + c TOLERANT; times the scale): the forms cancel for small s, and the
forms are the definition.  Measured: numpy 1.5 / 2.1 / 3.9 units of eps (rho0 / rho1 / rho2).  A rho1 at its floor max(DBL_MIN, .) is
exempt (FLOORED lists them: none at these s)."""
import json
import os
import subprocess

import mpmath
import numpy as np
import pytest

import lm_step_cases as LC
import lm_step_reference as R
import loss_reference as L
from test_lm_step_reference import C_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = R.EPS
TINY = np.finfo(np.float64).tiny
mpmath.mp.dps = 50


def goldens():
    with open(os.path.join(ROOT, "tests", "golden", "losses.json")) as fh:
        return json.load(fh)["cases"]


def _check_rows(case, evaluate):
    """evaluate(s) -> (rho0, rho1, rho2) as floats; -> worst error of each in units of its bound / 16, the floored rows"""
    loss = L.loss(case["type"], case["a"], case["b"], case["scale"])
    K = L.knee(loss)[1] * case["scale"]
    worst, floored = [0.0, 0.0, 0.0], []
    for row in case["rows"]:
        s = float.fromhex(row["s"])
        got = evaluate(s)
        want = [mpmath.mpf(v) for v in row["rho"]]
        units = [abs(got[0] - want[0]) / (EPS * (abs(want[0]) + K)) if abs(want[0]) + K > 0 else mpmath.mpf(abs(got[0]))]
        if want[1] < TINY:
            floored.append((loss, s))
            assert got[1] == TINY * case["scale"]
        else:
            units.append(abs(got[1] - want[1]) / (EPS * abs(want[1])))
        if want[2] == 0:
            assert got[2] == 0.0, (loss, s, got)
        else:
            units.append(abs(got[2] - want[2]) / (EPS * abs(want[2])))
        for k, u in enumerate(units):
            assert u <= 16, (loss, s, k, float(u), got, [float(w) for w in want])
            worst[k] = max(worst[k], float(u))
    return worst, floored


def test_the_goldens_cover_every_loss_and_both_sides_of_the_tolerant_branch():
    cases = goldens()
    assert {c["type"] for c in cases} == set(range(6))
    assert any(c["scale"] != 1.0 for c in cases)
    for c in cases:
        assert len(c["rows"]) == (10 if c["type"] == L.TOLERANT else 8)
        if c["type"] == L.TOLERANT:
            x = [(float.fromhex(r["s"]) - c["a"]) / c["b"] for r in c["rows"][-2:]]
            assert x == [36.5, 37.0]                   # exact in binary64
            assert float(mpmath.mpf(c["rows"][-2]["rho"][2])) > 0 and float(mpmath.mpf(c["rows"][-1]["rho"][2])) == 0


FLOORED = []   # (loss, s) at which rho1 sits at its floor: none among the goldens' s


def test_numpy_forms_match_the_goldens():
    worst, floored = [0.0, 0.0, 0.0], []
    for c in goldens():
        loss = L.loss(c["type"], c["a"], c["b"], c["scale"])
        w, f = _check_rows(c, lambda s: [float(v[0]) for v in L.rho(loss, np.array([s]))])
        worst = [max(a, b) for a, b in zip(worst, w)]
        floored += f
    print(f"numpy forms: worst rho0 {worst[0]:.2f}, rho1 {worst[1]:.2f}, rho2 {worst[2]:.2f} units of eps")
    assert floored == FLOORED


def test_long_double_forms_match_the_goldens():
    """... and in np.longdouble, the dtype the device checks take their expected values in (the same bound: no looser)."""
    for c in goldens():
        loss = L.loss(c["type"], c["a"], c["b"], c["scale"])
        _check_rows(c, lambda s: [float(v[0]) for v in L.rho(loss, np.array([s]), L.LD)])


FACADE_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "rsba/ceres_facade.hpp"
using namespace rsba_amd::ceres;
// argv: type a b scale s...   ->  one line "rho0 rho1 rho2" (hex floats) per s
int main(int argc, char** argv) {
  const int type = std::atoi(argv[1]);
  const double a = std::strtod(argv[2], nullptr), b = std::strtod(argv[3], nullptr), scale = std::strtod(argv[4], nullptr);
  LossFunction* inner = nullptr;
  switch (type) {
    case 0: inner = new TrivialLoss; break;
    case 1: inner = new HuberLoss(a); break;
    case 2: inner = new SoftLOneLoss(a); break;
    case 3: inner = new CauchyLoss(a); break;
    case 4: inner = new ArctanLoss(a); break;
    case 5: inner = new TolerantLoss(a, b); break;
  }
  LossFunction* loss = scale == 1.0 ? inner : new ScaledLoss(inner, scale, TAKE_OWNERSHIP);
  for (int k = 5; k < argc; ++k) {
    double rho[3];
    loss->Evaluate(std::strtod(argv[k], nullptr), rho);
    std::printf("%a %a %a\n", rho[0], rho[1], rho[2]);
  }
  { double rho[3]; ScaledLoss none(nullptr, 3.0, TAKE_OWNERSHIP); none.Evaluate(2.0, rho); if (rho[0] != 6.0 || rho[1] != 3.0 || rho[2] != 0.0) return 3; }
  delete loss;
  return 0;
}
"""


def test_facade_classes_match_the_goldens(tmp_path):
    """Evaluate of the facade's loss classes (include/rsba/ceres_facade.hpp) on the goldens' s, in a program built here with g++.  It
    uses the loss classes only — none of the header's inline code that calls the C ABI is instantiated — so it links without the
    device library.  (-ffp-contract=off: the forms as written.)"""
    src = tmp_path / "loss_eval.cpp"
    src.write_text(FACADE_PROGRAM)
    exe = tmp_path / "loss_eval"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", f"-I{ROOT}/include", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for c in goldens():
        ss = [float.fromhex(row["s"]) for row in c["rows"]]
        r = subprocess.run([str(exe), str(c["type"]), repr(c["a"]), repr(c["b"]), repr(c["scale"])] + [s.hex() for s in ss], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr)
        table = {s: [float.fromhex(v) for v in line.split()] for s, line in zip(ss, r.stdout.splitlines())}
        assert len(table) == len(ss)
        _check_rows(c, lambda s: table[s])


@pytest.mark.parametrize("d,K", [(2, 15), (2, 24), (12, 25)])
def test_triggs_identities(d, K):
    """J~^T J~ = rho1 J^T J + 2 rho2 (J^T r)(J^T r)^T where the rank-one branch applies (rho2 > 0, D > 0), J~^T r~ = rho1 J^T r always:
    lm_step_reference.corrected restated in np.longdouble on random 2 x K and 12 x K blocks, every loss."""
    rng = np.random.default_rng(7 + d + K)
    n = 400
    r = (rng.normal(size=(n, d)) * np.exp(rng.uniform(-3, 6, size=(n, 1)))).astype(L.LD)
    J = rng.normal(size=(n, d, K)).astype(L.LD)
    r[0] = 0                                                # s == 0: the plain branch
    for loss in [L.loss(L.HUBER, 2), L.loss(L.SOFT_L_ONE, 10), L.loss(L.CAUCHY, 10), L.loss(L.ARCTAN, 100), L.loss(L.TOLERANT, 150, 50),
                 L.loss(L.TOLERANT, 100, 25, 0.5), L.loss(L.TOLERANT, 1, 0.5)]:
        s = np.sum(r * r, axis=1)
        _, r1, r2 = L.rho(loss, s, L.LD)
        plain = (s == 0) | (r2 <= 0)
        ss = np.where(plain, 1, s)
        D = np.where(plain, 1, 1 + 2 * ss * r2 / r1)
        assert np.all(D > 0)
        alpha = np.where(plain, 0, 1 - np.sqrt(D))
        rtj = np.einsum("nd,ndk->nk", r, J)
        Jc = np.sqrt(r1)[:, None, None] * (J - (alpha / ss)[:, None, None] * r[:, :, None] * rtj[:, None, :])
        rc = (np.sqrt(r1) / (1 - alpha))[:, None] * r
        # the fp64 corrector of the reference agrees with this restatement
        with L.substituted(loss):
            r64, J64 = R.corrected(1.0, r.astype(np.float64), J.astype(np.float64))
        assert np.allclose(J64, Jc.astype(np.float64), rtol=1e-12, atol=1e-12 * float(np.max(np.abs(Jc))))
        assert np.allclose(r64, rc.astype(np.float64), rtol=1e-12, atol=0)
        JtJ = np.einsum("ndk,ndl->nkl", Jc, Jc)
        want = r1[:, None, None] * np.einsum("ndk,ndl->nkl", J, J) + np.where(plain, 0, 2 * r2)[:, None, None] * rtj[:, :, None] * rtj[:, None, :]
        scale = np.max(np.abs(want), axis=(1, 2))
        assert np.all(np.max(np.abs(JtJ - want), axis=(1, 2)) <= 1e-16 * scale), float(np.max(np.max(np.abs(JtJ - want), axis=(1, 2)) / scale))
        g, gw = np.einsum("ndk,nd->nk", Jc, rc), r1[:, None] * rtj
        gs = np.maximum(np.max(np.abs(gw), axis=1), 1e-300)
        assert np.all(np.max(np.abs(g - gw), axis=1) <= 1e-16 * gs)
        if loss[0] == L.TOLERANT:
            assert np.mean(~plain) > 0.3                    # the branch is exercised
        else:
            assert plain.all()                              # of the set only TOLERANT takes it


def _step(oracle, name, loss, **kw):
    p, opts = LC.case(name)
    r, J, ok = oracle.evaluate_blocks(p)
    assert ok.all()
    radius = {k: opts[k] for k in ("initial_trust_region_radius",) if k in opts}
    return p, r, J, radius, L.lm_step(p, r, J, loss, **radius, **kw)


@pytest.mark.parametrize("name,loss", [("rs_Fp1", L.loss(L.TOLERANT, 1, 0.5)), ("rs_huber", L.loss(L.TOLERANT, 4, 2))])
def test_the_bound_sees_a_corrector_without_its_rank_one_branch(oracle, monkeypatch, name, loss):
    """rho2 taken as non-positive (today's corrector) under a loss with rho2 > 0: the step moves by far more than
    C_TOL kappa eps |delta|.  (Measured: 3.9e10 units on rs_Fp1 with TOLERANT(1, 0.5), 1.96e12 on rs_huber with TOLERANT(4, 2).)"""
    p, r, J, radius, ref = _step(oracle, name, loss)
    unit = ref.kappa * EPS * R.delta_inf(ref)
    monkeypatch.setattr(L, "rho", (lambda f: lambda l, s, dtype=np.float64: (lambda v: (v[0], v[1], -np.abs(v[2])))(f(l, s, dtype)))(L.rho))
    other = L.lm_step(p, r, J, loss, want_kappa=False, **radius)
    moved = float(np.max(np.abs(other.delta() - ref.delta()))) / unit
    print(f"{name} {loss}: without the rank-one branch the step moves by {moved:.3g} units")
    assert moved >= 1e6, moved


@pytest.mark.parametrize("name", ["rs_Fp1", "rs_huber"])
def test_the_bound_sees_hubers_rho1_under_cauchy(oracle, monkeypatch, name):
    loss = L.loss(L.CAUCHY, 10)
    p, r, J, radius, ref = _step(oracle, name, loss)
    unit = ref.kappa * EPS * R.delta_inf(ref)
    monkeypatch.setattr(L, "rho", (lambda f: lambda l, s, dtype=np.float64: (lambda v: (v[0], f(L.loss(L.HUBER, 10), s, dtype)[1], v[2]))(f(l, s, dtype)))(L.rho))
    other = L.lm_step(p, r, J, loss, want_kappa=False, **radius)
    moved = float(np.max(np.abs(other.delta() - ref.delta()))) / unit
    print(f"{name}: with Huber's rho1 under CAUCHY(10) the step moves by {moved:.3g} units")
    assert moved >= 1e6, moved


def test_a_trivial_or_huber_loss_is_the_existing_reference(oracle):
    """lm_step with HUBER(a) is lm_step_reference.lm_step with huber_a = a, and TRIVIAL the one without a loss, bit for bit."""
    p, opts = LC.case("rs_huber")
    r, J, _ = oracle.evaluate_blocks(p)
    kw = dict(initial_trust_region_radius=opts["initial_trust_region_radius"], want_kappa=False)
    assert np.array_equal(L.lm_step(p, r, J, L.loss(L.HUBER, p.huber_a), **kw).delta(), R.lm_step(p, r, J, **kw).delta())
    q = p.copy()
    q.huber_a = 0.0
    assert np.array_equal(L.lm_step(p, r, J, L.loss(L.TRIVIAL), **kw).delta(), R.lm_step(q, r, J, **kw).delta())
