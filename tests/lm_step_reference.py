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

The prior blocks of CeresHandler::Add are restated here from their meaning, in closed form and in np.longdouble (they are
linear in the poses and rational in the ratio), and appended to J:
  * motion priors (RsConstVeloPrior / RsConstAccelerationPrior, video_bundler_rs_inter.h:55-173; CeresHandler.h:147-185): 12
    residuals over [f.poses[0] | f.poses[1] | f-1.poses[0] | f-1.poses[1] | interFrameRatio], rotation rows times 0.01, the
    Huber corrector applied to the 12-vector as one block; the velocity prior's second half extrapolates with the previous
    velocity when ratio <= DBL_EPSILON.  Only two-pose frames carry them (no frame of ``frame_global`` may);
  * GoodPosePrior (CeresHandler.h:52-73,188-204): W (prior - pose) over [priorPoses block | pose block], no loss;
  * SphericalPrior (CeresHandler.h:36-50,127-130): |rot|^2 and 1e20 (1 - |cx| - |cy| - |cz|), no loss.
Extra unknowns, behind the intrinsics in the global numbering: the interFrameRatio when ``ratio_free`` (one column, Jacobi
scaled and damped like any other), then 6 per priorPoses block.  A block whose every column is constant only adds to the fixed
cost.  The second pose slot of a ``frame_global`` frame is data: neither touched nor an unknown.

Step application, as orc_solve restates Ceres 1.9 (rsba_oracle.cpp:790,855): x + delta, the ratio then projected onto its lower
bound (0 velocity, DBL_EPSILON acceleration; SetParameterLowerBound, ParameterBlock::Plus).  ``model_cost_change`` is that of the
MODEL step delta (before the projection); ``step_norm`` is |x_new - x0|_2 of the PROJECTED step; ``gradient_max_norm`` uses the
projected gradient x - max(lb, x - g) on the ratio.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spl

EPS = 2.0 ** -53
DBL_EPSILON = 2.0 ** -52      # _EPS of the reference (mat/core.h): the bounds and the branch of the motion priors
LD = np.longdouble
ROT_DOWNSCALE = 0.01          # rotation rows of the motion priors
SPHERICAL_WEIGHT = 1e20


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
    """Residuals [N, d] and Jacobians [N, d, K] of N blocks of d residuals after ceres::Corrector (Triggs), the loss acting on each
    d-vector as a whole: J <- sqrt(rho1) (I - alpha r r^T / |r|^2) J, r <- sqrt(rho1) / (1 - alpha) r."""
    J = np.asarray(J, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64).reshape(J.shape[0], J.shape[1])
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


# ---- prior blocks, closed forms ---------------------------------------------------------------------------------------------

def motion_prior(kind: int, scale: float, ratio, a, b, c, d):
    """RsConstVeloPrior (kind 1) / RsConstAccelerationPrior (kind 2) of frame f in np.longdouble.  a, b = f.poses[0], f.poses[1];
    c, d = (f-1).poses[0], (f-1).poses[1]; [..., 6] each.  Both residual halves are linear in the poses:
      velocity      r1 = a - (d + t (d - c))                      r2 = b - (a + (a - d) / t)     (t > eps)
                                                                 r2 = b - (a + (d - c))         (t <= eps)
      acceleration  r1 = a - (d + t (d - c) + ((a - d) - t (d - c)) / 2)
                    r2 = b - (a + (a - d) / t + ((b - a) - (a - d) / t) / 2)
    times scale, the rotation rows times 0.01.  Returns (r [..., 12], coefficients [2, 4] of (a, b, c, d) in each half,
    d r / d t [..., 12]); J over the 24 pose columns is kron(coefficients, I6) times the row weights."""
    t = LD(ratio)
    a, b, c, d = (np.asarray(v, dtype=np.float64).astype(LD) for v in (a, b, c, d))
    one, half = LD(1), LD(0.5)
    if kind == 1:
        C1 = (one, LD(0), t, -(one + t))
        dr1 = c - d
        if t > LD(DBL_EPSILON):
            C2 = (-(one + one / t), one, LD(0), one / t)
            dr2 = (a - d) / (t * t)
        else:
            C2 = (-one, one, one, -one)
            dr2 = np.zeros_like(a)
    elif kind == 2:
        C1 = (half, LD(0), half * t, -half * (one + t))
        dr1 = half * (c - d)
        C2 = (-half * (one + one / t), half, LD(0), half / t)
        dr2 = half * (a - d) / (t * t)
    else:
        raise ValueError(kind)
    w = LD(scale) * np.array([ROT_DOWNSCALE] * 3 + [1.0] * 3, dtype=np.float64).astype(LD)
    r1 = C1[0] * a + C1[1] * b + C1[2] * c + C1[3] * d
    r2 = C2[0] * a + C2[1] * b + C2[2] * c + C2[3] * d
    r = np.concatenate([w * r1, w * r2], axis=-1)
    return r, np.array([C1, C2], dtype=LD), np.concatenate([w * dr1, w * dr2], axis=-1)


def motion_prior_jacobian(kind: int, scale: float, ratio, a, b, c, d):
    """(r [n, 12], J [n, 12, 25]) over [a | b | c | d | t] in np.longdouble."""
    r, C, dt = motion_prior(kind, scale, ratio, a, b, c, d)
    w = LD(scale) * np.array([ROT_DOWNSCALE] * 3 + [1.0] * 3, dtype=np.float64).astype(LD)
    Jp = np.zeros((12, 24), dtype=LD)
    for h in range(2):
        for k in range(4):
            Jp[6 * h: 6 * h + 6, 6 * k: 6 * k + 6] = np.diag(C[h, k] * w)
    n = r.reshape(-1, 12).shape[0]
    J = np.concatenate([np.broadcast_to(Jp, (n, 12, 24)), dt.reshape(n, 12, 1)], axis=2)
    return r.reshape(n, 12), J


def good_pose_prior(rotation: float, position: float, prior, pose):
    """GoodPosePrior: W (prior - pose), W = diag(rotation x 3, position x 3); J over [prior | pose] = [W | -W]."""
    W = np.array([rotation] * 3 + [position] * 3, dtype=np.float64).astype(LD)
    prior, pose = (np.asarray(v, dtype=np.float64).reshape(-1, 6).astype(LD) for v in (prior, pose))
    r = W * (prior - pose)
    J = np.concatenate([np.diag(W), -np.diag(W)], axis=1)
    return r, np.broadcast_to(J, (len(r), 6, 12)).copy()


def spherical_prior(pose):
    """SphericalPrior: (|rot|^2, 1e20 (1 - |cx| - |cy| - |cz|)); J over the pose block, the sign of c at 0 that of ceres::abs(Jet): +."""
    x = np.asarray(pose, dtype=np.float64).reshape(6).astype(LD)
    sgn = np.where(x[3:] < 0, LD(-1), LD(1))
    r = np.array([np.sum(x[:3] * x[:3]), LD(SPHERICAL_WEIGHT) * (LD(1) - np.sum(np.abs(x[3:])))], dtype=LD)
    J = np.zeros((2, 6), dtype=LD)
    J[0, :3] = 2 * x[:3]
    J[1, 3:] = -LD(SPHERICAL_WEIGHT) * sgn
    return r[None, :], J[None, :, :]


def ratio_lower_bound(prob) -> float:
    return DBL_EPSILON if prob.prior_kind == 2 else 0.0


def has_motion_priors(prob) -> bool:
    return bool(prob.prior_kind) and prob.prior_frames is not None and len(prob.prior_frames) > 0


def layout(prob):
    """Global numbering: poses f * CD + 6 q + k, then intrinsics (uncalibrated only) F * CD + 9 c + k, then the interFrameRatio
    (free ratio with motion priors only), then the priorPoses blocks 6 g + k, then points ncam + 3 j + k.
    -> dict(CD, intr, iratio (-1: none), ipp (-1: none), ncam, nparam)."""
    F, P, M, NI = prob.num_frames, prob.poses_per_frame, prob.num_points, prob.num_intrinsics
    CD = 6 * P
    n = F * CD + (0 if prob.calibrated else 9 * NI)
    iratio = -1
    if has_motion_priors(prob) and prob.ratio_free:
        iratio, n = n, n + 1
    ipp = -1
    if prob.pose_prior_block is not None and len(prob.pose_prior_block):
        ipp, n = n, n + 6 * len(prob.pose_prior_block)
    return dict(CD=CD, intr=F * CD, iratio=iratio, ipp=ipp, ncam=n, nparam=n + 3 * M)


def columns(prob):
    """(global column of every Jacobian entry [N, K] (-1: not a parameter), number of camera-side columns, number of all columns,
    fixed mask per column), in the numbering of layout().  The second slot of a frame_global frame is not a parameter: its
    entries are -1 and its columns fixed."""
    F, P = prob.num_frames, prob.poses_per_frame
    L = layout(prob)
    CD, ncam, nparam = L["CD"], L["ncam"], L["nparam"]
    cal = bool(prob.calibrated)
    f = prob.obs_frame.astype(np.int64)
    j = prob.obs_point.astype(np.int64)
    pose_cols = f[:, None] * CD + np.arange(CD)[None, :]
    fixed = np.zeros(nparam, dtype=bool)
    if prob.frame_global is not None:
        assert P == 2
        glob = prob.frame_global.astype(bool)
        pose_cols[glob[f], 6:] = -1
        fixed[(np.flatnonzero(glob)[:, None] * CD + 6 + np.arange(6)[None, :]).reshape(-1)] = True
    cols = [pose_cols]
    if not cal:
        fi = np.zeros(F, dtype=np.int64) if prob.frame_intrinsics is None else prob.frame_intrinsics.astype(np.int64)
        cols.insert(0, L["intr"] + 9 * fi[f][:, None] + np.arange(9)[None, :])
    cols.append(ncam + 3 * j[:, None] + np.arange(3)[None, :])
    gcol = np.concatenate(cols, axis=1)
    if prob.pose_fixed_mask is not None:
        bits = (prob.pose_fixed_mask.reshape(F, P)[:, :, None] >> np.arange(6)[None, None, :]) & 1
        fixed[: F * CD] |= bits.reshape(-1).astype(bool)
    if not cal and prob.intrinsics_constant is not None:
        fixed[L["intr"]: L["intr"] + 9 * prob.num_intrinsics] = np.repeat(prob.intrinsics_constant.astype(bool), 9)
    if prob.point_constant is not None:
        fixed[ncam:] = np.repeat(prob.point_constant.astype(bool), 3)
    return gcol, ncam, nparam, fixed


def prior_blocks(prob):
    """The prior residual blocks of prob at its parameters: a list of (r [n, d], J [n, d, k], global columns [n, k], loss applies).
    r and J in np.longdouble, uncorrected; the ratio column of a constant ratio is -1 (not a parameter)."""
    L = layout(prob)
    CD = L["CD"]
    out = []
    if has_motion_priors(prob):
        assert prob.poses_per_frame == 2, "motion priors need two poses per frame (CeresHandler.h:151)"
        fr = prob.prior_frames.astype(np.int64)
        if prob.frame_global is not None:
            assert not np.any(prob.frame_global[fr]) and not np.any(prob.frame_global[fr - 1]), "no motion prior next to a one-pose frame"
        P = prob.poses
        r, J = motion_prior_jacobian(prob.prior_kind, prob.prior_scale, prob.inter_frame_ratio, P[fr, 0], P[fr, 1], P[fr - 1, 0], P[fr - 1, 1])
        g = np.concatenate([fr[:, None] * CD + np.arange(12)[None, :], (fr - 1)[:, None] * CD + np.arange(12)[None, :],
                            np.full((len(fr), 1), L["iratio"])], axis=1)
        out.append((r, J, g, True))
    if L["ipp"] >= 0:
        blk = prob.pose_prior_block.astype(np.int64)
        r, J = good_pose_prior(prob.pose_prior_rotation, prob.pose_prior_position, prob.pose_prior_values, prob.poses.reshape(-1, 6)[blk])
        g = np.concatenate([L["ipp"] + 6 * np.arange(len(blk))[:, None] + np.arange(6)[None, :], 6 * blk[:, None] + np.arange(6)[None, :]], axis=1)
        out.append((r, J, g, False))
    if prob.spherical_pose_block >= 0:
        r, J = spherical_prior(prob.poses.reshape(-1, 6)[prob.spherical_pose_block])
        out.append((r, J, (6 * int(prob.spherical_pose_block) + np.arange(6))[None, :], False))
    return out


@dataclasses.dataclass
class LMStep:
    poses: np.ndarray           # [F, P, 6] delta, 0 on fixed coordinates
    points: np.ndarray          # [M, 3]
    intrinsics: np.ndarray      # [NI, 9]
    ratio: np.ndarray           # [1] model delta of the interFrameRatio ([0] when it is not a parameter)
    pose_priors: np.ndarray     # [NG, 6] delta of the priorPoses blocks
    ratio_lb: float             # lower bound of the ratio
    model_cost_change: float    # -(g^T delta + 1/2 delta^T J^T J delta) of the model step
    gradient_max_norm: float    # |J^T r|_inf at x0 (projected on the ratio)
    step_norm: float            # |x_new - x0|_2, the ratio projected onto its bound
    kappa: float                # 2-norm condition number of the scaled, damped matrix
    free: np.ndarray            # global column of each unknown
    ncam: int                   # camera-side columns (poses, intrinsics, ratio, priorPoses) in the global numbering
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
        """Every parameter block after the step, as the solver applies it in fp64: {"poses", "points", "intrinsics", "ratio" [1],
        "pose_priors" [NG, 6]}; the ratio x + delta projected onto its lower bound."""
        ratio = np.array([prob.inter_frame_ratio], dtype=np.float64)
        if self.ratio[0] != 0.0:
            ratio = np.maximum(self.ratio_lb, ratio + self.ratio)
        pp = np.zeros((0, 6)) if prob.pose_prior_values is None else prob.pose_prior_values + self.pose_priors
        return dict(poses=prob.poses + self.poses, points=prob.points + self.points, intrinsics=prob.intrinsics + self.intrinsics,
                    ratio=ratio, pose_priors=pp)


def initial_blocks(prob):
    """The parameter blocks of prob as LMStep.apply names them."""
    return dict(poses=prob.poses, points=prob.points, intrinsics=prob.intrinsics, ratio=np.array([prob.inter_frame_ratio], dtype=np.float64),
                pose_priors=np.zeros((0, 6)) if prob.pose_prior_values is None else prob.pose_prior_values)


def assemble(prob, r, J, *, constant=None):
    """The whole Jacobian of ``prob`` over its unknowns, in np.longdouble: the observations' blocks after the Huber corrector (rows
    2 i + d), then the prior blocks'.  ``constant``: global columns held constant on top of the problem's own (the sensitivity tests'
    hook).  -> (J csr [rows, n], residuals [rows], free: global column of each unknown, pos: unknown of each global column (-1: none;
    pos[-1] serves the entries that are not a parameter), ncam, nparam)."""
    rc, Jc = corrected(float(prob.huber_a), r, J)
    gcol, ncam, nparam, fixed = columns(prob)
    if constant is not None:
        fixed = fixed.copy()
        fixed[np.asarray(constant, dtype=np.int64)] = True
    blocks = [(rc, Jc, gcol)]
    for rp, Jp, gp, loss in prior_blocks(prob):
        if loss:
            rp64, Jp64 = corrected(float(prob.huber_a), rp.astype(np.float64), Jp.astype(np.float64))
            blocks.append((rp64, Jp64, gp))
        else:
            blocks.append((rp, Jp, gp))
    touched = np.zeros(nparam, dtype=bool)
    for _, _, g in blocks:
        touched[g[g >= 0]] = True
    free = np.flatnonzero(touched & ~fixed)
    pos = np.full(nparam + 1, -1, dtype=np.int64)          # pos[-1]: the entries that are not a parameter
    pos[free] = np.arange(len(free))
    n = len(free)
    # sparse J over the unknowns, the observations' rows 2 i + d first, then the prior blocks'
    vals, rows_, cols_, rl = [], [], [], []
    row0 = 0
    for rb, Jb, g in blocks:
        nb, d, k = Jb.shape
        rows = np.repeat((row0 + np.arange(nb * d)).reshape(nb, d, 1), k, axis=2)
        cols = np.broadcast_to(pos[np.where(g >= 0, g, nparam)][:, None, :], (nb, d, k))
        keep = cols >= 0
        vals.append(np.asarray(Jb)[keep].astype(LD)); rows_.append(rows[keep]); cols_.append(cols[keep])
        rl.append(np.asarray(rb).reshape(-1).astype(LD))
        row0 += nb * d
    Jld = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows_), np.concatenate(cols_))), shape=(row0, n))
    rld = np.concatenate(rl)
    return Jld, rld, free, pos, ncam, nparam


def lm_step(prob, r, J, *, initial_trust_region_radius: float = 1e4, min_lm_diagonal: float = 1e-6, max_lm_diagonal: float = 1e32,
            jacobi_scaling: bool = True, refinements: int = 3, dense_limit: int = 6000, solver: str = "lu", want_kappa: bool = True,
            edit=None) -> LMStep:
    """The first LM step of ``prob`` linearised at its parameters; ``r`` [N, 2] and ``J`` [N, 2, K] are the raw blocks of the
    observations there (the prior blocks are evaluated here).  Above ``dense_limit`` unknowns the fp64 solves inside the refinement
    use a sparse LU of the whole system (``solver="lu"``) or, where its fill does not fit, a dense Cholesky of the camera system that
    eliminates the points (``"reduced"``); either way the refinement residual is that of the whole system in np.longdouble, so the
    answer does not rest on the elimination.  ``edit(H, free, scale)``, if given, returns a changed scaled, damped matrix (np.longdouble
    csr) to solve with instead: the sensitivity tests' hook."""
    Jld, rld, free, pos, ncam, nparam = assemble(prob, r, J)
    n = len(free)
    colsq = np.asarray(Jld.multiply(Jld).sum(axis=0)).reshape(-1)
    scale = (1.0 / (1.0 + np.sqrt(colsq.astype(np.float64)))) if jacobi_scaling else np.ones(n)
    Js = (Jld @ sp.diags(scale.astype(LD))).tocsr()
    JtJ = (Js.T @ Js).tocsr()
    diag = np.clip(JtJ.diagonal().astype(np.float64), min_lm_diagonal, max_lm_diagonal)
    H = (JtJ + sp.diags((diag / initial_trust_region_radius).astype(LD))).tocsr()
    if edit is not None:
        H = sp.csr_matrix(edit(H, free, scale))
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
    L = layout(prob)
    lb = ratio_lower_bound(prob)
    gproj = g.astype(np.float64)
    if L["iratio"] >= 0 and pos[L["iratio"]] >= 0:
        x = float(prob.inter_frame_ratio)
        k = pos[L["iratio"]]
        gproj[k] = x - max(lb, x - gproj[k])
    gmax = float(np.max(np.abs(gproj))) if n else 0.0
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
    dintr = np.zeros((NI, 9)) if prob.calibrated else d[L["intr"]: L["intr"] + 9 * NI].reshape(NI, 9)
    dratio = np.array([d[L["iratio"]] if L["iratio"] >= 0 else 0.0])
    NG = 0 if L["ipp"] < 0 else len(prob.pose_prior_block)
    dpp = d[L["ipp"]: L["ipp"] + 6 * NG].reshape(NG, 6) if NG else np.zeros((0, 6))
    dpt = d[ncam:].reshape(M, 3)
    # |x_new - x0|_2 with the ratio projected onto its bound (in exact arithmetic: delta elsewhere)
    moved = delta_free.copy()
    if L["iratio"] >= 0 and pos[L["iratio"]] >= 0:
        k = pos[L["iratio"]]
        x = LD(prob.inter_frame_ratio)
        moved[k] = max(LD(lb), x + delta_free[k]) - x
    return LMStep(poses=dpose, points=dpt, intrinsics=dintr, ratio=dratio, pose_priors=dpp, ratio_lb=lb, model_cost_change=mcc,
                  gradient_max_norm=gmax, step_norm=float(np.sqrt(np.sum(moved * moved))), kappa=kappa, free=free, ncam=ncam, scale=scale,
                  H=H, b=b, y=y, refinement=hist)


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


BLOCKS = ("poses", "points", "intrinsics", "ratio", "pose_priors")


def _solved(prob, poses1, points1, intrinsics1, ratio1, pose_priors1):
    got = dict(poses=poses1, points=points1, intrinsics=intrinsics1,
               ratio=np.array([prob.inter_frame_ratio if ratio1 is None else ratio1], dtype=np.float64).reshape(1),
               pose_priors=np.zeros((0, 6)) if pose_priors1 is None else pose_priors1)
    L = layout(prob)
    assert L["iratio"] < 0 or ratio1 is not None, "a free ratio is a parameter block: pass its solved value"
    assert L["ipp"] < 0 or pose_priors1 is not None, "the priorPoses blocks are parameter blocks: pass their solved values"
    return got


def block_errors(prob, ref: LMStep, poses1, points1, intrinsics1, ratio1=None, pose_priors1=None):
    """Worst |delta_got - delta_ref|_inf of every parameter block, against fl(x0 + delta_ref) (the ratio projected onto its bound):
    per frame [F], per point [M], per intrinsics block [NI], the ratio [1], per priorPoses block [NG]; and the rounding allowance of
    x0 + delta in fp64 (two ulps of the result) of each block.  ``ratio1`` and ``pose_priors1`` are the solved ratio and priorPoses
    values; both are required when the problem has those blocks."""
    got_all = _solved(prob, poses1, points1, intrinsics1, ratio1, pose_priors1)
    want_all, x0_all = ref.apply(prob), initial_blocks(prob)
    out = {}
    for name in BLOCKS:
        got, want, x0 = np.asarray(got_all[name]), want_all[name], x0_all[name]
        if not x0.size:
            out[name] = (np.zeros(0), np.zeros(0))
            continue
        err = np.abs((got - x0) - (want - x0)).reshape(len(x0), -1)
        ulp = 2.0 * np.spacing(np.maximum(np.abs(got), np.abs(want))).reshape(len(x0), -1)
        out[name] = (err.max(axis=1), ulp.max(axis=1))
    return out


def delta_inf(ref: LMStep) -> float:
    return max(float(np.max(np.abs(a))) if a.size else 0.0 for a in (ref.poses, ref.points, ref.intrinsics, ref.ratio, ref.pose_priors))


def step_ratio(prob, ref: LMStep, poses1, points1, intrinsics1, ratio1=None, pose_priors1=None):
    """Worst per-block error of a solved step, in units of kappa * eps * |delta_ref|_inf (beyond the two-ulp rounding allowance of
    x0 + delta), and the block it sits in: ("poses" | "points" | "intrinsics" | "ratio" | "pose_priors", index)."""
    unit = ref.kappa * EPS * delta_inf(ref)
    worst, where = 0.0, None
    for name, (err, ulp) in block_errors(prob, ref, poses1, points1, intrinsics1, ratio1, pose_priors1).items():
        if err.size:
            over = np.maximum(err - ulp, 0.0) / unit
            k = int(np.argmax(over))
            if over[k] > worst or where is None:
                worst, where = max(worst, float(over[k])), (name, k)
    return worst, where


def step_norm_bound(prob, ref: LMStep, c: float):
    """(|fl(x0 + delta) - x0|_2 with the ratio projected, allowed distance of a solver's step_norm from it: c kappa eps of the norm
    plus two ulps of x per coordinate)."""
    moved, ulp = [], []
    new, old = ref.apply(prob), initial_blocks(prob)
    for name in BLOCKS:
        moved.append((new[name] - old[name]).ravel())
        ulp.append(2.0 * np.spacing(np.abs(new[name])).ravel())
    moved, ulp = np.concatenate(moved), np.concatenate(ulp)
    nrm = float(np.sqrt(np.sum(moved * moved)))
    return nrm, c * ref.kappa * EPS * nrm + float(np.sqrt(np.sum(ulp[moved != 0] ** 2)))


def solved_blocks(q):
    """(poses, points, intrinsics, ratio, pose_priors) of a solved problem, the arguments of step_ratio / block_errors."""
    return q.poses, q.points, q.intrinsics, float(q.inter_frame_ratio), q.pose_prior_values


# ---- pose covariance: blocks of (J^T J)^-1 -----------------------------------------------------------------------------------

@dataclasses.dataclass
class Covariance:
    blocks: dict                # {frame: [CD, CD] np.longdouble}: zero rows and columns where a coordinate is not an unknown
    free: dict                  # {frame: bool [CD]}: the coordinates of the block that are unknowns
    kappa: float                # 2-norm condition number of the symmetrically scaled J^T J (nan when ok is False)
    refinement: list            # max |E - H^ Y| over all columns after the first solve and after each round of refinement
    ok: bool                    # False: J^T J is rank deficient (the fp64 factorisation of its scaled form fails, or kappa n eps >= 1)
    error: float = 0.0          # estimate of the reference's own error, in the unit of covariance_ratio (asserted <= 2^-6)


def _ld_matmul(A, Y, threads: int = 8):
    """A @ Y in np.longdouble, the columns of Y shared out among a few threads (the sparse product runs without the interpreter
    lock, and x87 arithmetic is all it does)."""
    from concurrent.futures import ThreadPoolExecutor
    k = Y.shape[1]
    if k < 2 * threads:
        return A @ Y
    parts = np.array_split(np.arange(k), threads)
    with ThreadPoolExecutor(threads) as ex:
        outs = list(ex.map(lambda c: A @ np.ascontiguousarray(Y[:, c]), parts))
    return np.concatenate(outs, axis=1)


def covariance_blocks(prob, r, J, frames, *, dense_limit: int = 6000, max_refinements: int = 8, constant=None, edit=None) -> Covariance:
    """What ceres::Covariance returns for the pose block(s) of each of ``frames``: the (frame, frame) block of (J^T J)^-1, J the
    Jacobian of assemble() — no Jacobi scaling, no damping, every unknown of the problem in it (points, intrinsics, the free ratio,
    the priorPoses blocks): nothing is eliminated.  H = J^T J is scaled symmetrically, H^ = H / (d d^T) with d = sqrt(diag H), and
    factored ONCE in fp64 (dense Cholesky up to ``dense_limit`` unknowns, a sparse LU above); every column H^ y = e_k of every asked
    frame goes through that factorisation together and is refined against H^ in np.longdouble until the residual stops falling, then
    unscaled by 1 / (d_a d_k).  ``constant``: see assemble(); ``edit(H, free)`` returns a changed unscaled H (np.longdouble csr)."""
    Jld, _, free, pos, ncam, nparam = assemble(prob, r, J, constant=constant)
    n = len(free)
    CD = layout(prob)["CD"]
    frames = [int(f) for f in frames]
    bad = Covariance(blocks={}, free={}, kappa=float("nan"), refinement=[], ok=False)
    H = (Jld.T @ Jld).tocsr()
    if edit is not None:
        H = sp.csr_matrix(edit(H, free))
    d = np.sqrt(H.diagonal())
    if n == 0 or not np.all(d > 0):
        return bad
    Dinv = sp.diags(LD(1) / d)
    Hs = (Dinv @ H @ Dinv).tocsr()
    H64 = Hs.astype(np.float64)
    try:
        if n <= dense_limit:
            A = H64.toarray()
            cf = scipy.linalg.cho_factor(A, lower=True)
            solve = lambda v: scipy.linalg.cho_solve(cf, v)  # noqa: E731
            ev = scipy.linalg.eigvalsh(A)
            lmin, lmax = float(ev[0]), float(ev[-1])
        else:
            lu = spl.splu(H64.tocsc())
            solve = lu.solve
            lmax = float(spl.eigsh(H64, k=1, which="LA", return_eigenvectors=False, tol=1e-4)[0])
            inv = spl.LinearOperator(H64.shape, matvec=lambda v: solve(np.asarray(v, dtype=np.float64).reshape(-1)), dtype=np.float64)
            lmin = 1.0 / float(spl.eigsh(inv, k=1, which="LA", return_eigenvectors=False, tol=1e-4)[0])
    except (np.linalg.LinAlgError, RuntimeError):        # not positive definite / exactly singular
        return bad
    if not (lmin > n * DBL_EPSILON * lmax):               # numerically rank deficient: no fp64 inverse means anything
        return bad
    kappa = lmax / lmin
    ks = [(f, a, int(pos[f * CD + a])) for f in frames for a in range(CD) if pos[f * CD + a] >= 0]
    blocks = {f: np.zeros((CD, CD), dtype=LD) for f in frames}
    isfree = {f: pos[f * CD + np.arange(CD)] >= 0 for f in frames}
    hist, error = [], 0.0
    if ks:
        E = np.zeros((n, len(ks)), dtype=LD)
        E[[k for _, _, k in ks], np.arange(len(ks))] = 1
        Y = solve(E.astype(np.float64)).astype(LD)
        res = E - _ld_matmul(Hs, Y)
        hist.append(float(np.max(np.abs(res))))
        for _ in range(max_refinements):
            dY = solve(res.astype(np.float64))
            Y2 = Y + dY.astype(LD)
            res2 = E - _ld_matmul(Hs, Y2)
            e2 = float(np.max(np.abs(res2)))
            if not e2 < hist[-1]:
                break
            fell = hist[-1] / max(e2, 1e-300)
            Y, res = Y2, res2
            hist.append(e2)
            if fell < 2.0:                               # (a round that gains less than a bit: the residual has stopped falling)
                break
        # what is left of the error, from one more fp64 solve of the last residual, in the unit of the comparison (covariance_ratio).
        # (The residual itself cannot fall below its own rounding, 2^-64 |H^| |y|: 2e-12 for a weakly determined frame at kappa^ 3e9.)
        dY = solve(res.astype(np.float64))
        diag = np.array([float(Y[k, c]) for c, (_, _, k) in enumerate(ks)])
        assert np.all(diag >= 1.0 - 1e-9), diag.min()      # H^ has a unit diagonal: that of its inverse is >= 1
        left = 0.0
        for c, (f, a, k) in enumerate(ks):
            rows = pos[f * CD + np.arange(CD)]
            m = rows >= 0
            blocks[f][m, a] = Y[rows[m], c] / (d[rows[m]] * d[k])
            own = np.array([diag[c2] for c2, (f2, _, _) in enumerate(ks) if f2 == f])
            left = max(left, float(np.max(np.abs(dY[rows[m], c]) / (kappa * EPS * np.sqrt(own * diag[c])))))
        assert left <= 2.0 ** -6, (left, hist)
        error = left
    return Covariance(blocks=blocks, free=isfree, kappa=kappa, refinement=hist, ok=True, error=error)


def covariance_ratio(ref: Covariance, frame: int, got) -> float:
    """Worst |got_ab - C_ab| / u_ab over the free coordinates of one block, u_ab = kappa * 2^-53 * sqrt(C_aa C_bb); inf when a
    fixed row or column of ``got`` is not exactly zero.  The same unit bounds |got - got^T| (covariance_asymmetry)."""
    C, m = ref.blocks[frame], ref.free[frame]
    got = np.asarray(got, dtype=np.float64)
    if np.any(got[~m, :] != 0) or np.any(got[:, ~m] != 0):
        return float("inf")
    if not m.any():
        return 0.0
    s = np.sqrt(np.diag(C)[m])
    u = LD(ref.kappa) * LD(EPS) * s[:, None] * s[None, :]
    return float(np.max(np.abs(got[np.ix_(m, m)] - C[np.ix_(m, m)]) / u))


def covariance_asymmetry(ref: Covariance, frame: int, got) -> float:
    """Worst |got_ab - got_ba| / u_ab over the free coordinates of one block."""
    C, m = ref.blocks[frame], ref.free[frame]
    if not m.any():
        return 0.0
    got = np.asarray(got, dtype=np.float64)[np.ix_(m, m)]
    s = np.sqrt(np.diag(C)[m])
    return float(np.max(np.abs(got - got.T) / (LD(ref.kappa) * LD(EPS) * s[:, None] * s[None, :])))
