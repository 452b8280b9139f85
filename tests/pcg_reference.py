"""Host reference for the iterative reduced solve of rsba_solve (rsba_set_linear_solver type 1): block-Jacobi preconditioned
conjugate gradients on the reduced camera system, restated in numpy from the rule in include/rsba_amd.h.

From an ``lm_step_reference.LMStep`` (its H, b, free, ncam, scale: the scaled, damped normal equations over the unknowns) the
points and the priorPoses blocks are eliminated block by block — S = Hcc - Hce Hee^-1 Hec, rhs = b_c - Hce Hee^-1 b_e — as the
device eliminates them, M is the block diagonal of S in the PROBLEM's partition (one block per frame: its free pose coordinates;
one per intrinsics block), and the textbook recurrence runs from y_0 = 0 with the library's stopping rule.  Everything is done
in one number format, np.longdouble (the reference) or np.float64 (the restatement whose distance from the reference calibrates
the bounds of tests/test_gpu_pcg.py).  Fixed coordinates and padding are not unknowns here; on the device they are decoupled
rows with a zero right-hand side, which changes nothing.

Nothing here imports the product or the oracle's solver.  The seeded errors of tests/test_pcg_reference.py are switches of
``pcg``: a frame's block of M replaced by the identity, the transposed use of one off-diagonal 48 x 48 tile left out of S p, a
stopping test that looks one iteration late."""
from __future__ import annotations

import dataclasses

import numpy as np
import scipy.sparse as sp

import lm_step_reference as R

LD = np.longdouble
TILE = 48


def chol(A):
    """Lower Cholesky factor of a small dense matrix in its own dtype (numpy.linalg has no long double)."""
    A = np.array(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError("block not positive definite")
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def chol_solve(L, b):
    n = L.shape[0]
    w = np.zeros_like(b)
    for i in range(n):
        w[i] = (b[i] - np.dot(L[i, :i], w[:i])) / L[i, i]
    z = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        z[i] = (w[i] - np.dot(L[i + 1:, i], z[i + 1:])) / L[i, i]
    return z


def _batched_inverse(blocks):
    """Inverses of [g, k, k] symmetric positive definite blocks, by Cholesky, in the blocks' dtype."""
    g, k, _ = blocks.shape
    L = np.zeros_like(blocks)
    for j in range(k):
        d = blocks[:, j, j] - np.sum(L[:, j, :j] * L[:, j, :j], axis=1)
        assert np.all(d > 0)
        L[:, j, j] = np.sqrt(d)
        for i in range(j + 1, k):
            L[:, i, j] = (blocks[:, i, j] - np.sum(L[:, i, :j] * L[:, j, :j], axis=1)) / L[:, j, j]
    Li = np.zeros_like(blocks)                    # L^-1, column by column
    for c in range(k):
        for i in range(c, k):
            e = 1 if i == c else 0
            Li[:, i, c] = (e - np.sum(L[:, i, c:i] * Li[:, c:i, c], axis=1)) / L[:, i, i]
    return np.einsum("gki,gkj->gij", Li, Li)      # L^-T L^-1


@dataclasses.dataclass
class Reduced:
    S: np.ndarray            # [nc, nc] reduced camera system over the camera-side unknowns that stay
    rhs: np.ndarray          # [nc]
    cam: np.ndarray          # [nc] their positions among the unknowns of the LMStep
    elim: np.ndarray         # [ne] positions of the eliminated unknowns (points, priorPoses)
    Einv: sp.csr_matrix      # Hee^-1
    Hec: sp.csr_matrix
    be: np.ndarray
    blocks: list             # index arrays into cam: the partition of M
    block_frame: list        # frame of each block (-1 - c for intrinsics block c)
    row: np.ndarray          # [nc] row of each unknown in the device's numbering of S (tiles of 48)
    dtype: type


def reduce_system(prob, ref: R.LMStep, dtype=LD) -> Reduced:
    L = R.layout(prob)
    assert L["iratio"] < 0, "a free interFrameRatio is outside the iterative solver"
    F, CD = prob.num_frames, L["CD"]
    free = np.asarray(ref.free)
    ncamcols = F * CD + (0 if prob.calibrated else 9 * prob.num_intrinsics)
    is_cam = free < ncamcols
    cam, elim = np.flatnonzero(is_cam), np.flatnonzero(~is_cam)
    H = sp.csr_matrix(ref.H).astype(dtype)
    b = np.asarray(ref.b).astype(dtype)
    # the eliminated blocks: 3 per point, 6 per priorPoses block — Hee is block diagonal over them
    ge = free[elim]
    key = np.where(ge >= ref.ncam, (ge - ref.ncam) // 3 + 10 ** 7, (ge - max(L["ipp"], 0)) // 6)
    order = np.argsort(key, kind="stable")
    assert np.array_equal(order, np.arange(len(order)))          # the unknowns are numbered block after block
    Hee = H[elim][:, elim].tocsr()
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    sizes = np.diff(np.r_[starts, len(key)])
    rows_, cols_, vals_ = [], [], []
    for k in np.unique(sizes):
        st = starts[sizes == k]
        idx = st[:, None] + np.arange(k)[None, :]
        blk = np.zeros((len(st), k, k), dtype=dtype)
        for a in range(k):
            for c in range(k):
                blk[:, a, c] = np.asarray(Hee[idx[:, a], idx[:, c]]).reshape(-1)
        inv = _batched_inverse(blk)
        rows_.append(np.repeat(idx[:, :, None], k, axis=2).ravel()); cols_.append(np.repeat(idx[:, None, :], k, axis=1).ravel()); vals_.append(inv.ravel())
    ne = len(elim)
    Einv = sp.csr_matrix((np.concatenate(vals_), (np.concatenate(rows_), np.concatenate(cols_))), shape=(ne, ne)) if ne else sp.csr_matrix((0, 0), dtype=dtype)
    if ne:                                        # nothing of Hee lies outside the blocks
        inside = sp.csr_matrix((np.ones(sum(len(v) for v in vals_)), (np.concatenate(rows_), np.concatenate(cols_))), shape=(ne, ne))
        outside = (Hee - Hee.multiply(inside)).tocsr()
        assert outside.nnz == 0 or np.max(np.abs(outside.data)) == 0
    Hcc, Hce = H[cam][:, cam].tocsr(), H[cam][:, elim].tocsr()
    Hec = Hce.T.tocsr()
    W = (Hce @ Einv).tocsr()
    S = np.asarray((Hcc - W @ Hec).toarray(), dtype=dtype)
    rhs = b[cam] - W @ b[elim]
    gcol = free[cam]
    frame = np.where(gcol < F * CD, gcol // CD, -1 - (gcol - F * CD) // 9)
    blocks, block_frame = [], []
    for f in dict.fromkeys(frame.tolist()):
        blocks.append(np.flatnonzero(frame == f)); block_frame.append(int(f))
    NPF = -(-9 // CD)
    c = (gcol - F * CD) // 9
    row = np.where(gcol < F * CD, gcol, F * CD + c * NPF * CD + (gcol - F * CD) % 9)
    return Reduced(S=S, rhs=np.asarray(rhs, dtype=dtype), cam=cam, elim=elim, Einv=Einv, Hec=Hec, be=b[elim], blocks=blocks, block_frame=block_frame,
                   row=row.astype(np.int64), dtype=dtype)


@dataclasses.dataclass
class PcgRun:
    y: list                  # iterates y_0 .. y_n (camera-side unknowns of Reduced.cam)
    iterations: int          # n: the iteration the rule stopped at
    Q: list                  # Q_0 .. Q_n
    zeta: list               # zeta_1 .. zeta_n at index k (index 0: nan)
    rel: list                # |r_k| / |rhs|
    reason: str              # "test" | "cap" | "exact"
    z: list                  # preconditioned residuals z_0 .. z_n (the M-orthogonality check)
    r: list


def prior_cross_entries(prob, ref: R.LMStep, red: Reduced) -> np.ndarray:
    """[nc, nc]: the entries of the motion priors' (f, f - 1) blocks of S — both orientations — that couple DIFFERENT pose coordinates
    (k of one pose with k' != k of another).  Without a loss, and under one with rho'' <= 0, a prior's Jacobian is kron(C, I6) times row
    weights and these entries are zero; the corrector's rank-one term (rho'' > 0: TolerantLoss) fills them.  The points and the
    priorPoses blocks couple no two frames through H's camera block, so what H holds there is the priors' and is S's entry too up to
    the points' fill, which stays."""
    F, CD = prob.num_frames, R.layout(prob)["CD"]
    g = np.asarray(ref.free)[red.cam]
    H = sp.csr_matrix(ref.H)[red.cam][:, red.cam].toarray().astype(red.dtype)
    pose = g < F * CD
    fr = np.where(pose, g // CD, -1)
    pf = np.zeros(F + 1, dtype=bool)
    pf[np.asarray(prob.prior_frames, dtype=np.int64)] = True
    upper = pose[:, None] & pose[None, :] & (fr[:, None] == fr[None, :] + 1) & pf[fr][:, None]   # rows in f, columns in f - 1
    other = (g % 6)[:, None] != (g % 6)[None, :]
    m = upper & other
    return np.where(m | m.T, H, 0)


def pcg(red: Reduced, *, min_iterations=1, max_iterations=500, eta=0.1, r_tolerance=-1.0, drop_block=None, drop_transposed=None, stop_late=0,
        drop_entries=None) -> PcgRun:
    """The recurrence and the stopping rule of include/rsba_amd.h in red.dtype.  Seeded errors: ``drop_block`` = index of a block of M
    replaced by the identity; ``drop_transposed`` = (I, J), I > J: tile (I, J) of S is not used for the rows of tile J;
    ``stop_late`` = 1: the stopping tests look at iteration k - 1's numbers; ``drop_entries`` = [nc, nc] (prior_cross_entries): these
    entries are missing from S in S p — the prior's (f, f - 1) block left as sparse as it is without a loss."""
    dt = red.dtype
    S, rhs = red.S, red.rhs
    if drop_entries is not None:
        S = S - np.asarray(drop_entries, dtype=dt)
    if drop_transposed is not None:
        I, J = drop_transposed
        S = S.copy()
        S[np.ix_(red.row // TILE == J, red.row // TILE == I)] = 0
    fac = [None if k == drop_block else chol(S0) for k, S0 in enumerate(red.S[np.ix_(ix, ix)] for ix in red.blocks)]

    def minv(v):
        z = v.copy()
        for ix, L in zip(red.blocks, fac):
            if L is not None:
                z[ix] = chol_solve(L, v[ix])
        return z

    n = len(rhs)
    y, r = np.zeros(n, dtype=dt), rhs.copy()
    z = minv(r)
    p = z.copy()
    rz = np.dot(r, z)
    b2 = np.dot(rhs, rhs)
    out = PcgRun(y=[y.copy()], iterations=0, Q=[dt(0)], zeta=[dt(np.nan)], rel=[dt(1)], reason="cap", z=[z.copy()], r=[r.copy()])
    if b2 == 0:
        out.reason = "exact"
        return out
    for k in range(1, max_iterations + 1):
        q = S @ p
        pq = np.dot(p, q)
        if not (pq > 0 and np.isfinite(pq)):
            raise np.linalg.LinAlgError("p.q not positive")
        alpha = rz / pq
        y = y + alpha * p
        r = r - alpha * q
        z = minv(r)
        rzn = np.dot(r, z)
        rr = np.dot(r, r)
        Q = dt(-0.5) * np.dot(y, rhs + r)
        zeta = k * (Q - out.Q[-1]) / Q
        out.y.append(y.copy()); out.Q.append(Q); out.zeta.append(zeta); out.rel.append(np.sqrt(rr / b2)); out.z.append(z.copy()); out.r.append(r.copy())
        out.iterations = k
        kk = k - stop_late
        stop = None
        if rr == 0:
            stop = "exact"
        if kk >= max(min_iterations, 1) and kk >= 1:
            if r_tolerance >= 0 and out.rel[kk] <= dt(r_tolerance):
                stop = "test"
            if eta > 0 and out.zeta[kk] < dt(eta):
                stop = "test"
        if stop:
            out.reason = stop
            return out
        p = z + (rzn / rz) * p
        rz = rzn
    return out


def full_solution(red: Reduced, ref: R.LMStep, yc):
    """The solution over all unknowns that follows from the camera-side y: the eliminated blocks back-substituted."""
    y = np.zeros(len(ref.free), dtype=red.dtype)
    y[red.cam] = yc
    if len(red.elim):
        y[red.elim] = red.Einv @ (red.be - red.Hec @ np.asarray(yc, dtype=red.dtype))
    return y


class StepMaker:
    """LMStep objects for other solutions y of one linearisation: the Jacobian is assembled once."""

    def __init__(self, prob, r, J, ref: R.LMStep):
        self.prob, self.ref = prob, ref
        self.Jld, self.rld, free, self.pos, self.ncam, self.nparam = R.assemble(prob, r, J)
        assert np.array_equal(free, ref.free)

    def step(self, y) -> R.LMStep:
        prob, ref = self.prob, self.ref
        delta_free = -ref.scale.astype(LD) * np.asarray(y).astype(LD)
        m = self.Jld @ delta_free
        mcc = -float(np.sum(m * (self.rld + m / 2)))
        d = np.zeros(self.nparam)
        d[ref.free] = delta_free.astype(np.float64)
        L = R.layout(prob)
        F, P, M, NI = prob.num_frames, prob.poses_per_frame, prob.num_points, prob.num_intrinsics
        NG = 0 if L["ipp"] < 0 else len(prob.pose_prior_block)
        return dataclasses.replace(
            ref, poses=d[: F * 6 * P].reshape(F, P, 6), points=d[self.ncam:].reshape(M, 3),
            intrinsics=np.zeros((NI, 9)) if prob.calibrated else d[L["intr"]: L["intr"] + 9 * NI].reshape(NI, 9),
            pose_priors=d[L["ipp"]: L["ipp"] + 6 * NG].reshape(NG, 6) if NG else np.zeros((0, 6)), ratio=np.zeros(1),
            model_cost_change=mcc, step_norm=float(np.sqrt(np.sum(delta_free * delta_free))), y=np.asarray(y).astype(LD))


def applied(prob, step: R.LMStep):
    """The parameter blocks after ``step`` in the argument order of R.step_ratio (what a solver that took exactly this step leaves)."""
    a = step.apply(prob)
    return a["poses"], a["points"], a["intrinsics"], float(a["ratio"][0]), (a["pose_priors"] if len(a["pose_priors"]) else None)
