"""Host reference for ONE Levenberg-Marquardt step of ceres::Solve, computed the textbook way (numpy / scipy only).

Semantics of Ceres 1.9's first LM iteration, as oracle/rsba_oracle.cpp (orc_solve) restates them:
  * the Huber corrector (Triggs) applied to each observation's residual and Jacobian (residual_block.cc, corrector.cc);
  * fixed pose coordinates (SubsetParameterization), constant point and intrinsics blocks, and parameter blocks no residual
    touches are not unknowns;
  * Jacobi scaling s = 1 / (1 + sqrt(colsq)), LM diagonal diag(Js^T Js) clamped to [min_lm_diagonal, max_lm_diagonal]
    and divided by the trust-region radius;
  * (Js^T Js + D) y = Js^T r, step delta = -s .* y.

The damped system is solved WITHOUT a Schur complement: a dense Cholesky of the whole system (a sparse LU above
``dense_limit`` unknowns), then rounds of iterative refinement whose residual is accumulated in np.longdouble against the
system formed in np.longdouble, so that the result is accurate well below the fp64 kappa * eps that a device solve can reach.

Inputs are per-observation residuals [N, 2] and RAW Jacobian blocks [N, 2, K] (columns [intrinsics 9]? [pose 6 P] [point 3],
the layout of oracle.evaluate_blocks and rsba_evaluate); nothing here imports the product or the oracle.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spl

EPS = 2.0 ** -53
LD = np.longdouble


def huber_rho(a: float, s: np.ndarray):
    """rho(s) of ceres::HuberLoss(a) and its two derivatives (loss_function.cc)."""
    s = np.asarray(s, dtype=np.float64)
    b = a * a
    out = s > b
    r = np.sqrt(np.where(out, s, 1.0))
    rho0 = np.where(out, 2.0 * a * r - b, s)
    rho1 = np.where(out, np.fmax(np.finfo(np.float64).tiny, a / r), 1.0)
    rho2 = np.where(out, -rho1 / (2.0 * np.where(out, s, 1.0)), 0.0)
    return rho0, rho1, rho2


def corrected(huber_a: float, r: np.ndarray, J: np.ndarray):
    """Residuals and Jacobians after ceres::Corrector (Triggs): J <- sqrt(rho1) (I - alpha r r^T / |r|^2) J, r <- sqrt(rho1) / (1 - alpha) r."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
    J = np.asarray(J, dtype=np.float64)
    if huber_a <= 0.0:
        return r.copy(), J.copy()
    s = np.sum(r * r, axis=1)
    _, rho1, rho2 = huber_rho(huber_a, s)
    sr1 = np.sqrt(rho1)
    plain = (s == 0.0) | (rho2 <= 0.0)
    ss = np.where(plain, 1.0, s)
    alpha = np.where(plain, 0.0, 1.0 - np.sqrt(np.where(plain, 1.0, 1.0 + 2.0 * ss * rho2 / rho1)))
    rscale = np.where(plain, sr1, sr1 / (1.0 - alpha))
    alpha_sq = np.where(plain, 0.0, alpha / ss)
    rtj = np.einsum("nd,ndk->nk", r, J)
    Jc = sr1[:, None, None] * (J - alpha_sq[:, None, None] * r[:, :, None] * rtj[:, None, :])
    return r * rscale[:, None], Jc


def columns(prob):
    """(global column of every Jacobian entry [N, K], number of camera-side columns, number of all columns, fixed mask per column).
    Global numbering: poses f * CD + 6 q + k, then intrinsics (uncalibrated only) F * CD + 9 c + k, then points ncam + 3 j + k."""
    F, P, M, NI = prob.num_frames, prob.poses_per_frame, prob.num_points, prob.num_intrinsics
    CD = 6 * P
    cal = bool(prob.calibrated)
    ncam = F * CD + (0 if cal else 9 * NI)
    nparam = ncam + 3 * M
    f = prob.obs_frame.astype(np.int64)
    j = prob.obs_point.astype(np.int64)
    cols = [f[:, None] * CD + np.arange(CD)[None, :]]
    if not cal:
        fi = np.zeros(F, dtype=np.int64) if prob.frame_intrinsics is None else prob.frame_intrinsics.astype(np.int64)
        cols.insert(0, F * CD + 9 * fi[f][:, None] + np.arange(9)[None, :])
    cols.append(ncam + 3 * j[:, None] + np.arange(3)[None, :])
    gcol = np.concatenate(cols, axis=1)
    fixed = np.zeros(nparam, dtype=bool)
    if prob.pose_fixed_mask is not None:
        bits = (prob.pose_fixed_mask.reshape(F, P)[:, :, None] >> np.arange(6)[None, None, :]) & 1
        fixed[: F * CD] = bits.reshape(-1).astype(bool)
    if not cal and prob.intrinsics_constant is not None:
        fixed[F * CD: ncam] = np.repeat(prob.intrinsics_constant.astype(bool), 9)
    if prob.point_constant is not None:
        fixed[ncam:] = np.repeat(prob.point_constant.astype(bool), 3)
    return gcol, ncam, nparam, fixed


@dataclasses.dataclass
class LMStep:
    poses: np.ndarray           # [F, P, 6] delta, 0 on fixed coordinates
    points: np.ndarray          # [M, 3]
    intrinsics: np.ndarray      # [NI, 9]
    model_cost_change: float    # -(g^T delta + 1/2 delta^T J^T J delta)
    gradient_max_norm: float    # |J^T r|_inf at x0
    step_norm: float            # |delta|_2
    kappa: float                # 2-norm condition number of the scaled, damped matrix
    free: np.ndarray            # global column of each unknown
    ncam: int                   # camera-side columns (poses + intrinsics) in the global numbering
    scale: np.ndarray           # Jacobi scale of each unknown
    H: sp.csr_matrix            # scaled, damped matrix over the unknowns (np.longdouble)
    b: np.ndarray               # Js^T r (np.longdouble)
    y: np.ndarray               # solution of H y = b (np.longdouble): delta = -scale .* y
    refinement: list            # |b - H y|_inf / |b|_inf after the first solve and after each round of refinement

    def delta(self) -> np.ndarray:
        """delta in the global column numbering of columns()."""
        d = np.zeros(self.ncam + 3 * self.points.shape[0])
        d[self.free] = (-self.scale * self.y).astype(np.float64)
        return d

    def apply(self, prob):
        """(poses, points, intrinsics) after x + delta in fp64, as the solver applies the step."""
        return prob.poses + self.poses, prob.points + self.points, prob.intrinsics + self.intrinsics


def lm_step(prob, r, J, *, initial_trust_region_radius: float = 1e4, min_lm_diagonal: float = 1e-6, max_lm_diagonal: float = 1e32,
            jacobi_scaling: bool = True, refinements: int = 3, dense_limit: int = 6000, solver: str = "lu", want_kappa: bool = True) -> LMStep:
    """The first LM step of ``prob`` linearised at its parameters; ``r`` [N, 2] and ``J`` [N, 2, K] are the raw blocks there.
    Above ``dense_limit`` unknowns the fp64 solves inside the refinement use a sparse LU of the whole system (``solver="lu"``) or,
    where its fill does not fit, a dense Cholesky of the camera system that eliminates the points (``"reduced"``); either way the
    refinement residual is that of the whole system in np.longdouble, so the answer does not rest on the elimination."""
    assert prob.prior_kind == 0 or prob.prior_frames is None or len(prob.prior_frames) == 0, "motion priors are not restated here"
    assert prob.pose_prior_block is None and prob.spherical_pose_block < 0 and prob.frame_global is None
    rc, Jc = corrected(float(prob.huber_a), r, J)
    N, _, K = Jc.shape
    gcol, ncam, nparam, fixed = columns(prob)
    touched = np.zeros(nparam, dtype=bool)
    touched[gcol.reshape(-1)] = True
    free = np.flatnonzero(touched & ~fixed)
    pos = np.full(nparam, -1, dtype=np.int64)
    pos[free] = np.arange(len(free))
    n = len(free)
    # sparse J over the unknowns, rows 2 i + d
    rows = np.repeat(np.arange(2 * N).reshape(N, 2, 1), K, axis=2)
    cols = np.broadcast_to(pos[gcol][:, None, :], (N, 2, K))
    keep = cols >= 0
    Jld = sp.csr_matrix((Jc[keep].astype(LD), (rows[keep], cols[keep])), shape=(2 * N, n))
    rld = rc.reshape(-1).astype(LD)
    colsq = np.asarray(Jld.multiply(Jld).sum(axis=0)).reshape(-1)
    scale = (1.0 / (1.0 + np.sqrt(colsq.astype(np.float64)))) if jacobi_scaling else np.ones(n)
    Js = (Jld @ sp.diags(scale.astype(LD))).tocsr()
    JtJ = (Js.T @ Js).tocsr()
    diag = np.clip(JtJ.diagonal().astype(np.float64), min_lm_diagonal, max_lm_diagonal)
    H = (JtJ + sp.diags((diag / initial_trust_region_radius).astype(LD))).tocsr()
    b = Js.T @ rld
    H64 = H.astype(np.float64)
    if n <= dense_limit:
        cf = scipy.linalg.cho_factor(H64.toarray(), lower=True)
        solve = lambda v: scipy.linalg.cho_solve(cf, v)  # noqa: E731
    elif solver == "lu":
        lu = spl.splu(H64.tocsc())
        solve = lu.solve
    else:
        solve = _reduced_solver(H64, free < ncam)
    y = solve(b.astype(np.float64)).astype(LD)
    bnorm = float(np.max(np.abs(b))) if n else 1.0
    hist = []
    for _ in range(refinements):
        res = b - H @ y
        hist.append(float(np.max(np.abs(res))) / bnorm)
        y = y + solve(res.astype(np.float64)).astype(LD)
    hist.append(float(np.max(np.abs(b - H @ y))) / bnorm)
    delta_free = -scale.astype(LD) * y
    # model cost change with the undamped, unscaled model: m = J delta; -(sum m (r + m / 2))
    m = Jld @ delta_free
    mcc = -float(np.sum(m * (rld + m / 2)))
    g = Jld.T @ rld
    gmax = float(np.max(np.abs(g))) if n else 0.0
    kappa = float("nan")
    if want_kappa and n:
        if n <= dense_limit:
            ev = scipy.linalg.eigvalsh(H64.toarray())
            kappa = float(ev[-1] / ev[0])
        else:
            lmax = spl.eigsh(H64, k=1, which="LA", return_eigenvectors=False, tol=1e-4)[0]
            inv = spl.LinearOperator(H64.shape, matvec=lambda v: solve(np.asarray(v).reshape(-1)), dtype=np.float64)
            lmin_inv = spl.eigsh(inv, k=1, which="LA", return_eigenvectors=False, tol=1e-4)[0]
            kappa = float(lmax * lmin_inv)
    d = np.zeros(nparam)
    d[free] = delta_free.astype(np.float64)
    F, P, M, NI = prob.num_frames, prob.poses_per_frame, prob.num_points, prob.num_intrinsics
    dpose = d[: F * 6 * P].reshape(F, P, 6)
    dintr = np.zeros((NI, 9)) if prob.calibrated else d[F * 6 * P: ncam].reshape(NI, 9)
    dpt = d[ncam:].reshape(M, 3)
    return LMStep(poses=dpose, points=dpt, intrinsics=dintr, model_cost_change=mcc, gradient_max_norm=gmax,
                  step_norm=float(np.sqrt(np.sum(delta_free * delta_free))), kappa=kappa, free=free, ncam=ncam, scale=scale, H=H, b=b, y=y,
                  refinement=hist)


def _reduced_solver(H64, cam):
    """fp64 solver of H v = w through the camera system S = Hcc - Hcp Hpp^-1 Hpc (Hpp: 3 x 3 point blocks), S dense."""
    c, q = np.flatnonzero(cam), np.flatnonzero(~cam)
    assert np.all(np.diff(q) == 1) and len(q) % 3 == 0      # the point unknowns: consecutive 3-vectors after the camera unknowns
    Hpp = H64[q][:, q].tocsr()
    blocks = np.zeros((len(q) // 3, 3, 3))
    for a in range(3):
        for b in range(3):
            blocks[:, a, b] = Hpp[np.arange(a, len(q), 3), np.arange(b, len(q), 3)].A1
    Vinv = sp.block_diag(list(np.linalg.inv(blocks)), format="csr")
    W = H64[c][:, q].tocsr()
    WV = (W @ Vinv).tocsr()
    cf = scipy.linalg.cho_factor((H64[c][:, c] - WV @ W.T).toarray(), lower=True)

    def solve(w):
        v = np.empty_like(w)
        v[c] = scipy.linalg.cho_solve(cf, w[c] - WV @ w[q])
        v[q] = Vinv @ (w[q] - W.T @ v[c])
        return v
    return solve


def block_errors(prob, ref: LMStep, poses1, points1, intrinsics1):
    """Worst |delta_got - delta_ref|_inf of every parameter block, against fl(x0 + delta_ref): per frame [F], per point [M],
    per intrinsics block [NI]; and the rounding allowance of x0 + delta in fp64 (two ulps of the result) of each block."""
    ep, ept, ei = ref.apply(prob)
    out = {}
    for name, got, want, x0 in (("poses", poses1, ep, prob.poses), ("points", points1, ept, prob.points), ("intrinsics", intrinsics1, ei, prob.intrinsics)):
        err = np.abs((np.asarray(got) - x0) - (want - x0)).reshape(len(x0), -1)
        ulp = 2.0 * np.spacing(np.maximum(np.abs(got), np.abs(want))).reshape(len(x0), -1)
        out[name] = (err.max(axis=1) if err.size else err, ulp.max(axis=1) if ulp.size else ulp)
    return out


def delta_inf(ref: LMStep) -> float:
    return max(float(np.max(np.abs(a))) if a.size else 0.0 for a in (ref.poses, ref.points, ref.intrinsics))


def step_ratio(prob, ref: LMStep, poses1, points1, intrinsics1):
    """Worst per-block error of a solved step, in units of kappa * eps * |delta_ref|_inf (beyond the two-ulp rounding allowance of
    x0 + delta), and the block it sits in: ("poses" | "points" | "intrinsics", index)."""
    unit = ref.kappa * EPS * delta_inf(ref)
    worst, where = 0.0, None
    for name, (err, ulp) in block_errors(prob, ref, poses1, points1, intrinsics1).items():
        if err.size:
            over = np.maximum(err - ulp, 0.0) / unit
            k = int(np.argmax(over))
            if over[k] > worst or where is None:
                worst, where = max(worst, float(over[k])), (name, k)
    return worst, where


def step_norm_bound(prob, ref: LMStep, c: float):
    """(|fl(x0 + delta) - x0|_2, allowed distance of a solver's step_norm from it: c kappa eps of the norm plus two ulps of x per coordinate)."""
    moved, ulp = [], []
    for got, x0 in zip(ref.apply(prob), (prob.poses, prob.points, prob.intrinsics)):
        moved.append((got - x0).ravel())
        ulp.append(2.0 * np.spacing(np.abs(got)).ravel())
    moved, ulp = np.concatenate(moved), np.concatenate(ulp)
    nrm = float(np.sqrt(np.sum(moved * moved)))
    return nrm, c * ref.kappa * EPS * nrm + float(np.sqrt(np.sum(ulp[moved != 0] ** 2)))
