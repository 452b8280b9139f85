"""Extended-precision covariance blocks of frames, pairs of frames, points and intrinsics blocks: the method of lm_step_reference.covariance_blocks
— the whole undamped J^T J with NOTHING eliminated, scaled symmetrically to a unit diagonal, factored once in fp64, every column refined
against the np.longdouble system, its own error estimated from one more solve of the last residual and asserted <= 2^-6 unit — run for
the unit vectors of every asked frame, point and intrinsics block, so that cross blocks come out of the same columns.

Unit of an entry: u_ab = kappa^ * 2^-53 * sqrt(C_aa C_bb), kappa^ the condition number of the scaled J^T J (as covariance_ratio).

selinv_fp64 is the device algorithm of rsba_covariance_compute and its getters restated in numpy fp64 (see there): what the bound of the
device tests is derived from (tests/test_cov_reference.py)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import lm_step_reference as R

LD = np.longdouble


@dataclass
class FullCovariance:
    frame_blocks: dict          # {(a, b): [CD, CD] longdouble}, zero rows / columns at coordinates that are not unknowns
    intr_blocks: dict           # {c: [9, 9]}
    point_blocks: dict          # {j: [3, 3]}
    free: dict                  # {("f", frame) | ("i", block) | ("p", point): bool [dim]}
    diag: dict                  # ... : C_aa of every coordinate (0 where it is not an unknown)
    kappa: float
    ok: bool
    error: float = 0.0          # the reference's own error in the unit above (asserted <= 2^-6)


def full_covariance(prob, r, J, frame_pairs, points=(), intrinsics=(), *, dense_limit: int = 6000, max_refinements: int = 8) -> FullCovariance:
    Jld, _, free, pos, ncam, _ = R.assemble(prob, r, J)
    n = len(free)
    L = R.layout(prob)
    CD = L["CD"]
    frame_pairs = [(int(a), int(b)) for a, b in frame_pairs]
    groups = {("f", f): f * CD + np.arange(CD) for f in sorted({f for ab in frame_pairs for f in ab})}
    groups.update({("i", int(c)): L["intr"] + 9 * int(c) + np.arange(9) for c in intrinsics})
    groups.update({("p", int(j)): ncam + 3 * int(j) + np.arange(3) for j in points})
    bad = FullCovariance({}, {}, {}, {}, {}, float("nan"), False)
    H = (Jld.T @ Jld).tocsr()
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
    except (np.linalg.LinAlgError, RuntimeError):
        return bad
    if not (lmin > n * R.DBL_EPSILON * lmax):
        return bad
    kappa = lmax / lmin
    # one column per unknown of the asked groups
    unk = np.array(sorted({int(pos[g]) for cols in groups.values() for g in cols if pos[g] >= 0}), dtype=np.int64)
    col_of = {int(k): c for c, k in enumerate(unk)}
    E = np.zeros((n, len(unk)), dtype=LD)
    E[unk, np.arange(len(unk))] = 1
    Y = solve(E.astype(np.float64)).astype(LD)
    res = E - R._ld_matmul(Hs, Y)
    last = float(np.max(np.abs(res))) if len(unk) else 0.0
    for _ in range(max_refinements):
        Y2 = Y + solve(res.astype(np.float64)).astype(LD)
        res2 = E - R._ld_matmul(Hs, Y2)
        e2 = float(np.max(np.abs(res2)))
        if not e2 < last:
            break
        fell = last / max(e2, 1e-300)
        Y, res, last = Y2, res2, e2
        if fell < 2.0:
            break
    dY = solve(res.astype(np.float64))
    sdiag = np.array([float(Y[k, c]) for c, k in enumerate(unk)])        # diagonal of the scaled inverse: >= 1
    assert np.all(sdiag >= 1.0 - 1e-9), sdiag.min()
    error = float(np.max(np.abs(dY[unk, :]) / (kappa * R.EPS * np.sqrt(np.outer(sdiag, sdiag))))) if len(unk) else 0.0
    assert error <= 2.0 ** -6, error

    def block(ga, gb):
        ka, kb = pos[groups[ga]], pos[groups[gb]]
        out = np.zeros((len(ka), len(kb)), dtype=LD)
        ma, mb = ka >= 0, kb >= 0
        cols = [col_of[int(k)] for k in kb[mb]]
        out[np.ix_(ma, mb)] = Y[np.ix_(ka[ma], cols)] / np.outer(d[ka[ma]], d[kb[mb]])
        return out

    isfree = {g: pos[cols] >= 0 for g, cols in groups.items()}
    diag = {g: np.diag(block(g, g)).copy() for g in groups}
    return FullCovariance({(a, b): block(("f", a), ("f", b)) for a, b in frame_pairs}, {int(c): block(("i", int(c)), ("i", int(c))) for c in intrinsics},
                          {int(j): block(("p", int(j)), ("p", int(j))) for j in points}, isfree, diag, kappa, True, error)


def block_ratio(ref: FullCovariance, ga, gb, C, got) -> float:
    """Worst |got_ab - C_ab| / u_ab over the unknowns of a block; inf when a row or column that is no unknown is not exactly zero."""
    ma, mb = ref.free[ga], ref.free[gb]
    got = np.asarray(got, dtype=np.float64)
    if np.any(got[~ma, :] != 0) or np.any(got[:, ~mb] != 0):
        return float("inf")
    if not ma.any() or not mb.any():
        return 0.0
    u = LD(ref.kappa) * LD(R.EPS) * np.sqrt(np.outer(ref.diag[ga][ma], ref.diag[gb][mb]))
    return float(np.max(np.abs(got[np.ix_(ma, mb)] - C[np.ix_(ma, mb)]) / u))


def frame_ratio(ref, a, b, got) -> float:
    return block_ratio(ref, ("f", a), ("f", b), ref.frame_blocks[(a, b)], got)


def intr_ratio(ref, c, got) -> float:
    return block_ratio(ref, ("i", c), ("i", c), ref.intr_blocks[c], got)


def point_ratio(ref, j, got) -> float:
    return block_ratio(ref, ("p", j), ("p", j), ref.point_blocks[j], got)


def asymmetry(ref: FullCovariance, g, got) -> float:
    """Worst |got_ab - got_ba| / u_ab of a diagonal block."""
    m = ref.free[g]
    if not m.any():
        return 0.0
    got = np.asarray(got, dtype=np.float64)[np.ix_(m, m)]
    return float(np.max(np.abs(got - got.T) / (LD(ref.kappa) * LD(R.EPS) * np.sqrt(np.outer(ref.diag[g][m], ref.diag[g][m])))))


# ---- the device algorithm, restated in numpy fp64 ----

TILE = 48


@dataclass
class SelectedInverse:
    frame_blocks: dict          # {(a, b): [CD, CD] float64}
    intr_blocks: dict           # {c: [9, 9]}
    point_blocks: dict          # {j: [3, 3]}
    nt: int
    nslots: int
    nlev: int


def selinv_fp64(prob, r, J, plan_of, frame_pairs, points=(), intrinsics=(), *, fault=None, fault_frame=None) -> SelectedInverse:
    """rsba_covariance_compute and its getters step by step, every product in fp64:
      1. Schur elimination of the points and the priorPoses blocks from J^T J (block diagonal: one sparse solve) -> the reduced camera
         system S, bordered by the column of a free interFrameRatio;
      2. S in the device's camera-side numbering — frame f at f CD, intrinsics block c at the front of its NPF = ceil(9 / CD) pseudo
         frames behind the real frames, padded to whole 48 x 48 tiles; a coordinate that is no unknown sits there as a decoupled diagonal;
      3. the tile Cholesky factor in the order and on the pattern plan_of(nt, edges) gives (tests/test_selinv_plan.py: plan — the lists
         of rsba_debug_selinv_plan), W_j = L_jj^-1 with rows and columns zeroed where the coordinate is no unknown;
      4. the Takahashi recurrence over the plan's G / OFF / DIAG lists, level by level;
      5. frame and intrinsics blocks read off the tiles (an entry off the pattern is NaN here: reading one shows), plus v_a v_b^T / s of
         the border, S v = b by substitution through the factor, s = h - b.v;
      6. point blocks V^-1 + V^-1 (W^T Sigma W) V^-1 + q q^T / s, q = V^-1 W^T v, W the point's cross block (nonzero in its frames only).
    fault (the negative controls of tests/test_cov_reference.py): "tile" — one diagonal tile of Sigma, the one of frame_pairs[-1][0], is
    off by 1e-9 relative; "transpose" — an OFF item takes Sigma_ki where it needs Sigma_ik = Sigma_ki^T; "border" — the border's term is
    left out; "record" (tests/test_loss_paths_reference.py: under a general loss, lm_step_reference.huber_rho substituted) — the point
    rows of frame ``fault_frame`` come from the record of the no-loss / Huber-at-scale-1 instantiation: in step 6 the observations of
    that frame enter W with the raw Jacobian (the problem here carries no Huber threshold of its own: rho' = 1, no corrector), V^-1 and
    Sigma, which the solver's passes left, stay."""
    assert fault in (None, "tile", "transpose", "border", "record")
    Jld, _, free, pos, ncam, nparam = R.assemble(prob, r, J)
    Hrec = None
    if fault == "record":
        raw = prob.copy()
        raw.huber_a = 0.0                                           # corrected() returns the blocks as they are
        Jraw, _, free_raw, _, _, _ = R.assemble(raw, r, J)
        assert np.array_equal(free, free_raw)
        obs = np.flatnonzero(prob.obs_frame == int(fault_frame))
        assert len(obs), "the frame of the fault has no observation"
        rows = (2 * obs[:, None] + np.arange(2)[None, :]).reshape(-1)   # assemble(): the observations' rows 2 i + d come first
        Jmix = Jld.astype(np.float64).tolil()
        Jmix[rows] = Jraw.astype(np.float64).tocsr()[rows]
        Jmix = Jmix.tocsr()
        Hrec = (Jmix.T @ Jmix).tocsc()
    L = R.layout(prob)
    CD, F = L["CD"], prob.num_frames
    NIB = 0 if prob.calibrated else prob.num_intrinsics
    NPF = -(-9 // CD) if NIB else 0
    npad = -(-((F + NIB * NPF) * CD) // TILE) * TILE
    nt = npad // TILE
    J64 = Jld.astype(np.float64).tocsr()
    H = (J64.T @ J64).tocsr()
    n = H.shape[0]
    # unknown -> device coordinate (camera side), -1 the ratio, -2 what the elimination takes out (points, priorPoses blocks)
    dev = np.full(n, -2, dtype=np.int64)
    g = free
    pose = g < F * CD
    dev[pose] = g[pose]
    if NIB:
        ii = (g >= L["intr"]) & (g < L["intr"] + 9 * NIB)
        c, k = (g[ii] - L["intr"]) // 9, (g[ii] - L["intr"]) % 9
        dev[ii] = (F + c * NPF) * CD + k
    if L["iratio"] >= 0:
        dev[g == L["iratio"]] = -1
    keep, elim = np.flatnonzero(dev >= -1), np.flatnonzero(dev == -2)
    Hkk = H[keep][:, keep].toarray()
    if len(elim):
        Hee = H[elim][:, elim].tocsc()
        Hek = H[elim][:, keep].toarray()
        Hkk = Hkk - Hek.T @ spl.splu(Hee).solve(Hek)
    kd = dev[keep]
    cam = kd >= 0
    S = np.eye(npad)
    live = np.zeros(npad, dtype=bool)
    live[kd[cam]] = True
    S[np.ix_(kd[cam], kd[cam])] = Hkk[np.ix_(cam, cam)]
    border = None
    if (~cam).any():
        assert (~cam).sum() == 1
        b = np.zeros(npad)
        b[kd[cam]] = Hkk[np.ix_(cam, ~cam)][:, 0]
        border = (b, float(Hkk[np.ix_(~cam, ~cam)][0, 0]))
    tile = lambda M, a, b: M[a * TILE:(a + 1) * TILE, b * TILE:(b + 1) * TILE]  # noqa: E731
    edges = [(a, b) for a in range(nt) for b in range(a) if tile(S, a, b).any()]
    p = plan_of(nt, edges)
    st = p["slot_tiles"]
    idx = (np.asarray(p["perm"], dtype=np.int64)[:, None] * TILE + np.arange(TILE)[None, :]).reshape(-1)
    Lc = np.linalg.cholesky(S[np.ix_(idx, idx)])
    Lfull = np.zeros((npad, npad))
    Lfull[np.ix_(idx, idx)] = Lc
    mask = np.zeros((nt, nt), dtype=bool)
    mask[st[:, 0], st[:, 1]] = True
    assert all(mask[a, b] or not tile(Lfull, a, b).any() for a in range(nt) for b in range(nt)), "the factor leaves the plan's pattern"
    W = {}
    for t in range(nt):
        w = np.linalg.inv(tile(Lfull, t, t))
        m = live[t * TILE:(t + 1) * TILE]
        W[t] = np.where(np.outer(m, m), w, 0.0)
    Lf = {s: tile(Lfull, st[s, 0], st[s, 1]) for s in range(p["nslots"])}
    G, Sg = {}, {}
    dropped = fault != "transpose"
    for lev in range(p["nlev"]):
        for q in range(p["lev_g_ptr"][lev], p["lev_g_ptr"][lev + 1]):
            slot, t = p["g_info"][q]
            G[int(slot)] = Lf[int(slot)] @ W[int(t)]
        for t in range(p["lev_off_ptr"][lev], p["lev_off_ptr"][lev + 1]):
            acc = np.zeros((TILE, TILE))
            for ss, trans, gs in p["off_list"][p["off_ptr"][t]:p["off_ptr"][t + 1]]:
                if trans and not dropped:
                    dropped = True                                  # (the fault: once)
                    acc -= Sg[int(ss)] @ G[int(gs)]
                else:
                    acc -= (Sg[int(ss)].T if trans else Sg[int(ss)]) @ G[int(gs)]
            Sg[int(p["off_info"][t, 0])] = acc
        for d in range(p["lev_diag_ptr"][lev], p["lev_diag_ptr"][lev + 1]):
            out, t = p["diag_info"][d]
            X = W[int(t)].T @ W[int(t)]
            for s in p["diag_list"][p["diag_ptr"][d]:p["diag_ptr"][d + 1]]:
                X -= Sg[int(s)].T @ G[int(s)]
            Sg[int(out)] = 0.5 * (X + X.T)
    assert fault != "transpose" or dropped, "the plan has no transposed operand: the control shows nothing"
    Sigma = np.full((npad, npad), np.nan)
    for s in range(p["nslots"]):
        a, b = int(st[s, 0]), int(st[s, 1])
        tile(Sigma, a, b)[:] = Sg[s]
        if a != b:
            tile(Sigma, b, a)[:] = Sg[s].T
    if fault == "tile":
        t = (int(frame_pairs[-1][0]) * CD) // TILE
        tile(Sigma, t, t)[:] *= 1.0 + 1e-9
    v, bs = np.zeros(npad), 0.0
    if border is not None and fault != "border":
        b, hh = border
        y = scipy.linalg.solve_triangular(Lc, b[idx], lower=True)
        v[idx] = scipy.linalg.solve_triangular(Lc.T, y, lower=False)
        v[~live] = 0.0
        bs = 1.0 / (hh - float(b @ v))

    def cam_block(r0, c0, dim):
        ra, ca = r0 + np.arange(dim), c0 + np.arange(dim)
        blk = Sigma[np.ix_(ra, ca)]
        assert np.isfinite(blk).all(), "a block off the factor's pattern"
        ok = np.outer(live[ra], live[ca])
        return np.where(ok, blk + np.outer(v[ra], v[ca]) * bs, 0.0)

    fb = {(int(a), int(b)): cam_block(int(a) * CD, int(b) * CD, CD) for a, b in frame_pairs}
    ib = {int(c): cam_block((F + int(c) * NPF) * CD, (F + int(c) * NPF) * CD, 9) for c in intrinsics}
    pb = {}
    Hc = H.tocsc()
    camk = keep[cam]                                                # unknowns of the camera side, their device coordinates kd[cam]
    for j in points:
        pj = pos[ncam + 3 * int(j) + np.arange(3)]
        if np.any(pj < 0):
            pb[int(j)] = np.zeros((3, 3))
            continue
        Wj = (Hc if Hrec is None else Hrec)[:, pj][camk].toarray()   # [camera-side unknowns, 3]
        nz = np.flatnonzero(np.any(Wj != 0, axis=1))
        rows = kd[cam][nz]
        Vinv = np.linalg.inv(Hc[:, pj][pj].toarray())
        Sg_j = Sigma[np.ix_(rows, rows)]
        assert np.isfinite(Sg_j).all(), "two frames of a point without a tile of the factor"
        q = Vinv @ (Wj[nz].T @ v[rows])
        C = Vinv + Vinv @ (Wj[nz].T @ Sg_j @ Wj[nz]) @ Vinv + np.outer(q, q) * bs
        pb[int(j)] = 0.5 * (C + C.T)
    return SelectedInverse(fb, ib, pb, nt, int(p["nslots"]), int(p["nlev"]))
