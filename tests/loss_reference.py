"""Host reference of the problem's loss function (rsba_set_loss; the rule: include/rsba_amd.h): the six rho functions in numpy, the
first LM step and a whole trust-region loop under any of them.  Imports neither the product nor the oracle's solver.

A loss is a tuple (type, a, b, scale): type one of TRIVIAL .. TOLERANT below, ``a`` its parameter, ``b`` TolerantLoss' second
(ignored elsewhere), ``scale`` the factor of ScaledLoss (1: none).  ``rho(loss, s)`` evaluates the closed forms of the header in the
dtype asked for — np.float64: the definition, operation for operation; np.longdouble: the expected values of the device checks.

``lm_step`` is lm_step_reference.lm_step with that loss in place of Huber's: ``corrected`` and ``prior_blocks`` there apply the
whole corrector (Triggs) to whatever ``huber_rho`` returns, so the module attribute is substituted for the duration of the call,
with ``prob.huber_a`` positive so that the corrector is not skipped."""
from __future__ import annotations

import contextlib

import numpy as np

import lm_step_reference as R

TRIVIAL, HUBER, SOFT_L_ONE, CAUCHY, ARCTAN, TOLERANT = range(6)
NAMES = {TRIVIAL: "TRIVIAL", HUBER: "HUBER", SOFT_L_ONE: "SOFT_L_ONE", CAUCHY: "CAUCHY", ARCTAN: "ARCTAN", TOLERANT: "TOLERANT"}
TOLERANT_X = 36.7            # beyond it 1 + e^x is e^x in fp64
LD = np.longdouble


def loss(type, a=0.0, b=0.0, scale=1.0):
    return (int(type), float(a), float(b), float(scale))


def rho(loss_, s, dtype=np.float64):
    """(rho0, rho1, rho2) at s (array), in ``dtype``."""
    kind, a, b, scale = loss_
    T = dtype
    s = np.asarray(s, dtype=T)
    tiny = T(np.finfo(np.float64).tiny)
    one, two = T(1), T(2)
    a, b, scale = T(a), T(b), T(scale)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if kind == TRIVIAL:
            out = (s.copy(), np.ones_like(s), np.zeros_like(s))
        elif kind == HUBER:
            bb = a * a
            far = s > bb
            r = np.sqrt(np.where(far, s, one))
            r1 = np.where(far, np.fmax(tiny, a / r), one)
            out = (np.where(far, two * a * r - bb, s), r1, np.where(far, -r1 / (two * np.where(far, s, one)), T(0)))
        elif kind == SOFT_L_ONE:
            bb = a * a
            c = one / bb
            sm = one + s * c
            t = np.sqrt(sm)
            r1 = np.fmax(tiny, one / t)
            out = (two * bb * (t - one), r1, -(c * r1) / (two * sm))
        elif kind == CAUCHY:
            bb = a * a
            c = one / bb
            sm = one + s * c
            inv = one / sm
            out = (bb * np.log(sm), np.fmax(tiny, inv), -c * (inv * inv))
        elif kind == ARCTAN:
            bb = one / (a * a)
            sm = one + s * s * bb
            inv = one / sm
            out = (a * np.arctan2(s, a), np.fmax(tiny, inv), -two * s * bb * (inv * inv))
        elif kind == TOLERANT:
            c = b * np.log(one + np.exp(-a / b))
            x = (s - a) / b
            far = x > T(TOLERANT_X)
            xs = np.where(far, T(0), x)
            e = np.exp(xs)
            out = (np.where(far, s - a - c, b * np.log(one + e) - c), np.where(far, one, np.fmax(tiny, e / (one + e))),
                   np.where(far, T(0), T(0.5) / (b * (one + np.cosh(xs)))))
        else:
            raise ValueError(kind)
    return tuple(scale * v for v in out)


def knee(loss_):
    """The s around which the loss changes regime, and the constant K its rho0 subtracts or scales by (the forms cancel below it)."""
    kind, a, b, _ = loss_
    if kind in (HUBER, SOFT_L_ONE, CAUCHY):
        return a * a, (2.0 if kind == SOFT_L_ONE else 1.0) * a * a
    if kind == ARCTAN:
        return a, a
    if kind == TOLERANT:
        return a, b + b * float(np.log1p(np.exp(-a / b)))
    return 1.0, 0.0


@contextlib.contextmanager
def substituted(loss_):
    """lm_step_reference with ``loss_`` where it calls huber_rho (the parameter a it passes is ignored)."""
    saved = R.huber_rho
    R.huber_rho = lambda a, s: rho(loss_, s)
    try:
        yield
    finally:
        R.huber_rho = saved


def _with_loss(prob):
    q = prob.copy()
    q.huber_a = 1.0          # (any positive number: corrected() skips the corrector at 0)
    return q


def lm_step(prob, r, J, loss_, **kw):
    with substituted(loss_):
        return R.lm_step(_with_loss(prob), r, J, **kw)


def cost_and_gradient(prob, r, J, loss_):
    """(sum rho0 / 2, sum rho1 J^T r over the global columns of lm_step_reference.columns) in np.longdouble, over the observations'
    raw blocks and the prior blocks that take the loss; fixed columns included (rsba_evaluate's gradient has them)."""
    gcol, ncam, nparam, _ = R.columns(prob)
    blocks = [(np.asarray(r, dtype=np.float64).astype(LD), np.asarray(J, dtype=np.float64).astype(LD), gcol, True)]
    blocks += [(rp, Jp, g, takes) for rp, Jp, g, takes in R.prior_blocks(prob)]
    cost, grad = LD(0), np.zeros(nparam + 1, dtype=LD)
    for rb, Jb, g, takes in blocks:
        rb = rb.reshape(Jb.shape[0], Jb.shape[1])
        s = np.sum(rb * rb, axis=1)
        r0, r1, _ = rho(loss_ if takes else loss(TRIVIAL), s, LD)
        cost += np.sum(r0) / 2
        jtr = r1[:, None] * np.einsum("nd,ndk->nk", rb, Jb)
        np.add.at(grad, np.where(g >= 0, g, nparam), jtr)
    return cost, grad[:nparam]


def total_cost(prob, r, loss_):
    s = np.sum(np.asarray(r, dtype=np.float64).astype(LD) ** 2, axis=1)
    c = np.sum(rho(loss_, s, LD)[0]) / 2
    for rp, _, _, takes in R.prior_blocks(prob):
        sp_ = np.sum(rp.reshape(rp.shape[0], -1) ** 2, axis=1)
        c += np.sum(rho(loss_ if takes else loss(TRIVIAL), sp_, LD)[0]) / 2
    return float(c)


def lm_loop(oracle, prob, loss_, *, max_num_iterations=15, initial_trust_region_radius=1e4, max_trust_region_radius=1e16,
            min_trust_region_radius=1e-32, min_relative_decrease=1e-3, function_tolerance=1e-6, gradient_tolerance=1e-10,
            parameter_tolerance=1e-8, min_lm_diagonal=1e-6, max_lm_diagonal=1e32):
    """The trust-region loop of rsba_solve (Ceres 1.9 TrustRegionMinimizer) around lm_step: the radius update
    (radius / max(1/3, 1 - (2 rho - 1)^3) on success, radius / decrease with decrease doubling on failure), min_relative_decrease,
    the Jacobi scales of the FIRST linearisation, the three tolerances.  Residuals and Jacobians from oracle.evaluate_blocks at every
    iterate.  -> list of dict(iteration, cost, cost_change, relative_decrease, step_is_successful, trust_region_radius), the problem
    at the end."""
    q = prob.copy()
    r, J, ok = oracle.evaluate_blocks(q)
    assert ok.all()
    cost = total_cost(q, r, loss_)
    trace = [dict(iteration=0, cost=cost, cost_change=0.0, relative_decrease=0.0, step_is_successful=0, trust_region_radius=initial_trust_region_radius)]   # (iteration 0 is the initial evaluation: no step)
    radius, decrease, scale0 = initial_trust_region_radius, 2.0, None
    for it in range(1, max_num_iterations + 1):
        with substituted(loss_):
            step = _scaled_step(_with_loss(q), r, J, radius, scale0, min_lm_diagonal, max_lm_diagonal)
        if scale0 is None:
            scale0 = dict(zip(step.free.tolist(), step.scale.tolist()))
        if step.gradient_max_norm <= gradient_tolerance:
            break
        new = step.apply(q)
        cand = q.copy()
        cand.poses, cand.points, cand.intrinsics = new["poses"], new["points"], new["intrinsics"]
        if step.ratio[0] != 0.0:
            cand.inter_frame_ratio = float(new["ratio"][0])
        if cand.pose_prior_values is not None:
            cand.pose_prior_values = new["pose_priors"]
        rc, Jc, okc = oracle.evaluate_blocks(cand)
        new_cost = total_cost(cand, rc, loss_) if okc.all() else float(np.finfo(np.float64).max)
        rec = dict(iteration=it, cost=cost, cost_change=0.0, relative_decrease=0.0, step_is_successful=0, trust_region_radius=radius,
                   model_cost_change=step.model_cost_change, step_norm=step.step_norm)
        trace.append(rec)
        x_norm = float(np.sqrt(np.sum(_x_global(q)[step.free] ** 2)))          # over the parameters of the reduced program
        if step.step_norm <= parameter_tolerance * (x_norm + parameter_tolerance):
            break
        change = rec["cost_change"] = cost - new_cost
        if abs(change) < function_tolerance * cost:                               # (before the decision, as Ceres 1.9 has it: x stays)
            break
        rel = rec["relative_decrease"] = change / step.model_cost_change
        if rel > min_relative_decrease:
            q, r, J, cost = cand, rc, Jc, new_cost
            radius = min(max_trust_region_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
            decrease = 2.0
            rec.update(step_is_successful=1, cost=cost, trust_region_radius=radius)
        else:
            radius, decrease = radius / decrease, 2.0 * decrease
            rec.update(trust_region_radius=radius)
            if radius < min_trust_region_radius:
                break
    return trace, q


def _x_global(prob):
    """The parameters in the global numbering of lm_step_reference.layout."""
    Lo = R.layout(prob)
    x = np.zeros(Lo["nparam"])
    n = prob.poses.size
    x[:n] = prob.poses.reshape(-1)
    if not prob.calibrated:
        x[Lo["intr"]: Lo["intr"] + prob.intrinsics.size] = prob.intrinsics.reshape(-1)
    if Lo["iratio"] >= 0:
        x[Lo["iratio"]] = prob.inter_frame_ratio
    if Lo["ipp"] >= 0:
        x[Lo["ipp"]: Lo["ncam"]] = np.asarray(prob.pose_prior_values).reshape(-1)
    x[Lo["ncam"]:] = prob.points.reshape(-1)
    return x


def _scaled_step(prob, r, J, radius, scale0, lo, hi):
    """The LM step at ``radius`` as lm_step_reference.lm_step forms it (the whole damped system, solved in fp64 and refined in
    np.longdouble), with the Jacobi scales ``scale0`` (unknown's global column -> scale) of the first linearisation where given, as
    Ceres keeps them for the whole solve."""
    import scipy.linalg
    import scipy.sparse as sp
    Jld, rld, free, pos, ncam, nparam = R.assemble(prob, r, J)
    if scale0 is None:
        colsq = np.asarray(Jld.multiply(Jld).sum(axis=0)).reshape(-1)
        s = 1.0 / (1.0 + np.sqrt(colsq.astype(np.float64)))
    else:
        s = np.array([scale0[int(c)] for c in free])
    Js = (Jld @ sp.diags(s.astype(LD))).tocsr()
    JtJ = (Js.T @ Js).tocsr()
    diag = np.clip(JtJ.diagonal().astype(np.float64), lo, hi)
    H = (JtJ + sp.diags((diag / radius).astype(LD))).tocsr()
    b = Js.T @ rld
    cf = scipy.linalg.cho_factor(H.astype(np.float64).toarray(), lower=True)
    y = scipy.linalg.cho_solve(cf, b.astype(np.float64)).astype(LD)
    for _ in range(3):
        y = y + scipy.linalg.cho_solve(cf, (b - H @ y).astype(np.float64)).astype(LD)
    delta_free = -s.astype(LD) * y
    m = Jld @ delta_free
    g = (Jld.T @ rld).astype(np.float64)
    d = np.zeros(nparam)
    d[free] = delta_free.astype(np.float64)
    L = R.layout(prob)
    lb = R.ratio_lower_bound(prob)
    F, P, M, NI = prob.num_frames, prob.poses_per_frame, prob.num_points, prob.num_intrinsics
    NG = 0 if L["ipp"] < 0 else len(prob.pose_prior_block)
    moved = delta_free.copy()
    if L["iratio"] >= 0 and pos[L["iratio"]] >= 0:
        k = pos[L["iratio"]]
        x = LD(prob.inter_frame_ratio)
        moved[k] = max(LD(lb), x + delta_free[k]) - x
        g[k] = float(x) - max(lb, float(x) - g[k])
    return R.LMStep(poses=d[: F * 6 * P].reshape(F, P, 6), points=d[ncam:].reshape(M, 3),
                    intrinsics=np.zeros((NI, 9)) if prob.calibrated else d[L["intr"]: L["intr"] + 9 * NI].reshape(NI, 9),
                    ratio=np.array([d[L["iratio"]] if L["iratio"] >= 0 else 0.0]),
                    pose_priors=d[L["ipp"]: L["ipp"] + 6 * NG].reshape(NG, 6) if NG else np.zeros((0, 6)), ratio_lb=lb,
                    model_cost_change=-float(np.sum(m * (rld + m / 2))), gradient_max_norm=float(np.max(np.abs(g))) if len(g) else 0.0,
                    step_norm=float(np.sqrt(np.sum(moved * moved))), kappa=float("nan"), free=free, ncam=ncam, scale=s, H=H, b=b, y=y, refinement=[])
