"""The device algorithm of rsba_covariance_compute, restated in numpy fp64 (tests/cov_reference.py: selinv_fp64 — Schur elimination,
tile factor on the plan's pattern, the Takahashi recurrence over the lists of rsba_debug_selinv_plan, the point formula, the border of
a free interFrameRatio), against the extended-precision inverse of the whole J^T J with nothing eliminated (full_covariance).  No GPU.

Per case: every (f, f) block, both blocks of adjacent frames, one co-visible pair, every intrinsics block, and the (point, point) block
of every point — rs_nt25 (about 8 600 unknowns): a seeded sample of 64 points plus EVERY point seen across the top separator of the
dissection (separator_points: the tiles of one point's frames are a clique of the tile graph, so no point has frames in BOTH sides of
a separator; some 900 of the 2 475 points have frames in the separator and in a side: 951 points are checked with the sample).  The reference solves three columns in extended
precision for each point asked, a minute and a half for these: the device tests, which share the cases, take a seeded sample of 64 of
them instead (case_of(..., sample_across=64)).  Unit of an entry: u_ab = kappa^ * 2^-53 * sqrt(C_aa C_bb); a block's ratio is max |got_ab - C_ab| / u_ab over its
unknowns.  Rows and columns that are no unknowns must be exactly zero (block_ratio returns inf otherwise).

C_COVP, the bound of the device tests (tests/test_gpu_cov_blocks.py), is the smallest power of two >= 4 x the worst ratio this
restatement reaches on these cases, never below C_COV = 8 (tests/test_lm_step_reference.py).  Measured here (worst ratio per family):

    case               (f, f)   (f, g)   intrinsics   points   kappa^
    rs_Fp1              0.053    0.053            -    0.054   1.55e+07   (225 of 225 points)
    gs_F2p1             0.471    0.344            -    0.106   6.67e+03   (765 of 765 points)
    rs_far_pair         0.114    0.112            -    0.125   1.26e+06   (765 of 765 points)
    rs_intr_shared      0.209    0.208        0.232    0.238   4.00e+07   (405 of 405 points)
    gs_intr_perframe    0.113    0.106        0.116    0.114   2.90e+09   (64 of 765 points)
    rs_acc_free         0.123    0.123            -    0.172   1.26e+05   (405 of 405 points)
    rs_pp_some          0.350    0.350            -    0.342   3.11e+06   (405 of 405 points)
    rs_scanline         0.108    0.091            -    0.038   8.33e+04   (450 of 450 points)
    rs_const_points     1.768    0.434            -    0.056   2.14e+03   (405 of 405 points)
    rs_const_frame      0.793    0.459            -    0.060   3.53e+03   (495 of 495 points)
    rs_nt25 (leaf 2)    0.133    0.133            -    0.131   1.90e+07   (951 of 2475 points)

The worst is 1.768 ((f, f) of rs_const_points, kappa^ 2.1e3: the unit is small where the problem is well conditioned); 4 x 1.768 = 7.07,
so C_COVP = 8 = C_COV.  Asymmetry is exactly zero everywhere (diagonal tiles and point blocks are symmetrised).

The controls, same units: a 1e-9 relative error in the diagonal tile of Sigma under the co-visible frame of rs_Fp1 gives 38.3 on the
points (V^-1 W^T Sigma W V^-1 nearly cancels against V^-1's share, which amplifies it) and 0.58 on the frame blocks themselves — at
kappa^ 1.55e7 the unit of a frame entry is 1.7e-9 of the entry, so no bound of this kind can see 1e-9 there, and the test asserts it on
the family that does; one dropped transpose on rs_nt25 1.6e9; the missing border term on rs_acc_free 4.2e10.

The negative controls show that the bound sees what it is there for: a 1e-9 relative error in one tile of Sigma, one dropped transpose
in the recurrence and a missing border term each push a ratio above C_COVP."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cov_reference as CR                                      # noqa: E402
import lm_step_cases as LC                                      # noqa: E402
from helpers import HOOKS_LIB                                   # noqa: E402
from test_lm_step_reference import C_COV                        # noqa: E402
from test_selinv_plan import plan as selinv_plan                # noqa: E402

C_COVP = 8
CASES = ["rs_Fp1", "gs_F2p1", "rs_far_pair", "rs_intr_shared", "gs_intr_perframe", "rs_acc_free", "rs_pp_some", "rs_scanline",
         "rs_const_points", "rs_const_frame", "rs_nt25"]
LEAF = {"rs_nt25": "2"}                                         # RSBA_CHOL_LEAF of a case: a dissection with fill and separators
ALL_POINTS_LIMIT = 2500                                         # unknowns up to which every point is checked


@pytest.fixture(scope="module")
def hooks():
    import __graft_entry__ as G
    G.build()
    return C.CDLL(HOOKS_LIB)


def covisible_pair(p):
    """Two frames >= 1 (frame 0 is constant in every case) that see a common point, as far apart as the scene has them."""
    keep = p.obs_frame >= 1
    order = np.argsort(p.obs_point[keep], kind="stable")
    f, j = p.obs_frame[keep][order], p.obs_point[keep][order]
    start = np.flatnonzero(np.r_[True, j[1:] != j[:-1], True])
    lo = np.minimum.reduceat(f, start[:-1]); hi = np.maximum.reduceat(f, start[:-1])
    k = int(np.argmax(hi - lo))
    return int(lo[k]), int(hi[k])


def pairs_of(p):
    """Every (f, f), both blocks of every pair of adjacent frames, one co-visible pair.  A video of more than 40 frames (rs_nt25: 99):
    frames f = 0, 5, 10, ... and their successors instead of all — the reference solves a column per coordinate of every frame named."""
    F = p.num_frames
    a, b = covisible_pair(p)
    first = range(F - 1) if F <= 40 else range(0, F - 1, 5)
    diag = range(F) if F <= 40 else sorted({g for f in first for g in (f, f + 1)} | {F - 1})
    out = [(f, f) for f in diag] + [(f, f + 1) for f in first] + [(f + 1, f) for f in first]
    return out + [q for q in ((a, a), (b, b), (a, b), (b, a)) if q not in out]


def separator_points(p, pl):
    """Points seen across the top separator of the plan's dissection, from either side.  The top separator: the tiles of the last
    elimination levels, one tile a level (the chain at the root of the elimination tree), down to where the factor's tile graph without
    them falls into two components: its sides.  The tiles of one point's frames are a clique of that graph, so no point has frames in
    both sides; the points whose blocks read tiles of the separator's columns AND of a part's — Sigma tiles of different levels of the
    recurrence, the (i, k) lookups of both orientations — are those with a frame in a separator tile and a frame in a side.  Both
    sides must have some."""
    nt, nlev = pl["nt"], pl["nlev"]
    iperm = np.empty(nt, dtype=np.int64)
    iperm[pl["perm"]] = np.arange(nt)
    level = pl["level"][iperm]                                  # by old tile index

    def components(sep):
        comp = np.full(nt, -1)
        adj = [[] for _ in range(nt)]
        for a, b in pl["slot_tiles"]:
            if a != b and a not in sep and b not in sep:
                adj[a].append(int(b)); adj[b].append(int(a))
        nc = 0
        for t in range(nt):
            if t in sep or comp[t] >= 0:
                continue
            stack, comp[t] = [t], nc
            while stack:
                for u in adj[stack.pop()]:
                    if comp[u] < 0:
                        comp[u] = nc; stack.append(u)
            nc += 1
        return comp, nc

    sep, comp, nc = set(), None, 0
    for lev in range(nlev - 1, -1, -1):
        at = np.flatnonzero(level == lev)
        if len(at) != 1:
            break
        sep.add(int(at[0]))
        comp, nc = components(sep)
        if nc >= 2:
            break
    if nc < 2:
        return set(), []
    FT = CR.TILE // (6 * p.poses_per_frame)
    side = comp[p.obs_frame // FT]
    out = []
    order = np.argsort(p.obs_point, kind="stable")
    j, sd = p.obs_point[order], side[order]
    start = np.flatnonzero(np.r_[True, j[1:] != j[:-1], True])
    sides = set()
    for a, b in zip(start[:-1], start[1:]):
        seen = {int(x) for x in sd[a:b]}
        if -1 in seen and len(seen) >= 2:
            out.append(int(j[a])); sides |= seen - {-1}
    return (sep, out) if len(sides) >= 2 else (sep, [])


_cache = {}


def case_of(name, oracle, hooks, sample_across=None):
    """(problem, r, J, pairs, points, intrinsics blocks, reference, plan_of): one extended-precision inverse per case and session.
    sample_across: a case with a dissection takes that many of its points across the top separator (seeded) instead of all."""
    def plan_of(nt, edges):
        old = os.environ.get("RSBA_CHOL_LEAF")
        try:
            if name in LEAF:
                os.environ["RSBA_CHOL_LEAF"] = LEAF[name]
            else:
                os.environ.pop("RSBA_CHOL_LEAF", None)
            return selinv_plan(hooks, nt, edges)
        finally:
            os.environ.pop("RSBA_CHOL_LEAF", None)
            if old is not None:
                os.environ["RSBA_CHOL_LEAF"] = old
    key = (name, sample_across if name in LEAF else None)
    if key not in _cache:
        p = LC.cov_case(name)
        r, J, ok = oracle.evaluate_blocks(p)
        assert ok.all()
        intr = [] if p.calibrated else list(range(p.num_intrinsics))
        pairs = pairs_of(p)
        nunk = R_unknowns(p)
        if nunk <= ALL_POINTS_LIMIT:
            points = list(range(p.num_points))
        elif name not in LEAF:
            points = sorted(int(j) for j in np.random.default_rng(25).choice(p.num_points, size=64, replace=False))
        else:
            got = {}

            def keep_plan(nt, edges):
                got["plan"] = plan_of(nt, edges)
                return got["plan"]
            CR.selinv_fp64(p, r, J, keep_plan, pairs[:1])
            sep, both = separator_points(p, got["plan"])
            assert sep and both, "no separator, or no point across it: the case does not exercise what it is there for"
            rng = np.random.default_rng(25)
            across = both if sample_across is None else rng.choice(np.asarray(both), size=min(sample_across, len(both)), replace=False)
            points = sorted({int(j) for j in across} | {int(j) for j in rng.choice(p.num_points, size=64, replace=False)})
        _cache[key] = (p, r, J, pairs, points, intr, CR.full_covariance(p, r, J, pairs, points, intr))
    return _cache[key] + (plan_of,)


def R_unknowns(p):
    L = CR.R.layout(p)
    return int(L["nparam"])


def worst_ratios(ref, fb, ib, pb):
    w = dict(diag=0.0, cross=0.0, intr=0.0, point=0.0, asym=0.0)
    for (a, b), blk in fb.items():
        kind = "diag" if a == b else "cross"
        w[kind] = max(w[kind], CR.frame_ratio(ref, a, b, blk))
        if a == b:
            w["asym"] = max(w["asym"], CR.asymmetry(ref, ("f", a), blk))
    for c, blk in ib.items():
        w["intr"] = max(w["intr"], CR.intr_ratio(ref, c, blk))
        w["asym"] = max(w["asym"], CR.asymmetry(ref, ("i", c), blk))
    for j, blk in pb.items():
        w["point"] = max(w["point"], CR.point_ratio(ref, j, blk))
        w["asym"] = max(w["asym"], CR.asymmetry(ref, ("p", j), blk))
    return w


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_matches_the_reference(oracle, hooks, name):
    p, r, J, pairs, points, intr, ref, plan_of = case_of(name, oracle, hooks)
    assert ref.ok
    got = CR.selinv_fp64(p, r, J, plan_of, pairs, points, intr)
    w = worst_ratios(ref, got.frame_blocks, got.intr_blocks, got.point_blocks)
    print(f"{name}: selinv_fp64, worst ratio (f, f) {w['diag']:.3f}, (f, g) {w['cross']:.3f}, intrinsics {w['intr']:.3f}, points {w['point']:.3f} "
          f"({len(points)} of {p.num_points}), asymmetry {w['asym']:.3f}, kappa^ {ref.kappa:.2e}, reference error {ref.error:.1e}, "
          f"{got.nt} tiles, {got.nslots} slots, {got.nlev} levels")
    assert 4 * max(w.values()) <= C_COVP, (name, w)
    if name == "rs_nt25":
        assert got.nlev < got.nt and got.nslots > 2 * got.nt - 1, "no dissection, or no fill"
    if name in ("rs_const_points",):
        const = np.flatnonzero(p.point_constant)
        assert len(const) and all(not got.point_blocks[int(j)].any() for j in const)
    assert any(blk.any() for blk in got.point_blocks.values())


def test_the_bound_is_derived_as_stated():
    assert C_COVP >= C_COV and C_COVP <= 64 and C_COVP & (C_COVP - 1) == 0


@pytest.mark.parametrize("fault, name", [("tile", "rs_Fp1"), ("transpose", "rs_nt25"), ("border", "rs_acc_free")])
def test_the_bound_sees_a_seeded_fault(oracle, hooks, fault, name):
    p, r, J, pairs, points, intr, ref, plan_of = case_of(name, oracle, hooks)
    got = CR.selinv_fp64(p, r, J, plan_of, pairs, points, intr, fault=fault)
    w = worst_ratios(ref, got.frame_blocks, got.intr_blocks, got.point_blocks)
    print(f"{name} with fault '{fault}' ({len(points)} points, kappa^ {ref.kappa:.2e}): worst ratio (f, f) {w['diag']:.3g}, (f, g) {w['cross']:.3g}, intrinsics {w['intr']:.3g}, points {w['point']:.3g}")
    assert max(w.values()) > C_COVP, (fault, w)
    if fault != "tile":                                         # (see the module's docstring: what a frame block sees of 1e-9 depends on kappa^)
        assert max(w["diag"], w["cross"]) > C_COVP, (fault, w)
