"""W = chol(D)^-1 of one 48 x 48 tile in extended precision, the yardsticks that hold a fp64 W against it, and the tiles on which
rsba_amd/csrc/tile_factor.hpp is checked (tests/test_tile_factor_reference.py on the host, tests/test_gpu_tile_factor.py on the device
through `tools/tile_factor_bench --check`).  No GPU, no rsba_amd import.

The unit of both yardsticks is eps * kappa_scaled(D), eps = 2^-53: the condition of the tile after the symmetric scaling that puts ones on
its diagonal is what the accuracy of a Cholesky factorisation depends on, so grading (S D S) and scale (2^k D) leave the unit alone.
  res(W, D) = max |W D W^T - I| / unit
  fwd(W, D) = max_i ( max_j |W - W_ref|_ij / max_j |W_ref|_ij ) / unit      row-wise: row i of W carries the scale d_i^-1/2

C_RES / C_FWD are the per-family bounds: 4 x the worst ratio the two host fp64 forms below reach on the family (measured by
tests/test_tile_factor_reference.py, which prints them and holds the host forms to the constants), rounded up to a power of two.  The
factor 4 is for what legitimately differs on the device: FMA contraction and the matrix instruction's order of summation (four products per
instruction, 16-blocks); the two hand refinements of the hardware estimates truncate at about e^3 = 2^-69 and add nothing visible."""
import functools
from collections import namedtuple

import numpy as np

T = 48
EPS = 2.0 ** -53
LD = np.longdouble
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)   # the empty pattern of rsba_amd/csrc/chol_cells.hpp, as the bits of a double

# families of the passing tiles ("kappa1" is the kappa = 1 member of the spectrum family: its unit is eps itself, where a host form reaches
# ratios of 1 - 3, against a few hundredths at kappa >= 1e2 — one constant over both would leave the large kappas a hundredfold slack)
FAMILIES = ("kappa1", "spectrum", "graded", "scale", "identity_rows", "block_diagonal", "bench", "pivot_edges")
# 4 x the worst host ratio, rounded up to a power of two (measured: the docstring of tests/test_tile_factor_reference.py)
C_RES = {"kappa1": 16.0, "spectrum": 4.0, "graded": 0.25, "scale": 8.0, "identity_rows": 4.0, "block_diagonal": 16.0, "bench": 1.0, "pivot_edges": 16.0}
C_FWD = {"kappa1": 8.0, "spectrum": 2.0, "graded": 2.0, "scale": 4.0, "identity_rows": 2.0, "block_diagonal": 8.0, "bench": 0.5, "pivot_edges": 8.0}

Tile = namedtuple("Tile", "family name D")


def _sym_lower(D, dtype):
    """The symmetric matrix whose lower triangle is D's (what the kernel reads)."""
    A = np.tril(np.asarray(D)).astype(dtype)
    return A + np.tril(A, -1).T


def reference_W(D):
    """chol(D)^-1 in long double: a column Cholesky, then the inverse of the factor by forward substitution (row i of W from the rows above)."""
    A = _sym_lower(D, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    W = np.zeros((n, n), LD)
    for i in range(n):
        rhs = -(L[i, :i] @ W[:i])
        rhs[i] += 1
        W[i] = rhs / L[i, i]
    return W


def kappa_scaled(D):
    """2-norm condition of diag(D)^-1/2 D diag(D)^-1/2."""
    A = _sym_lower(D, LD)
    s = 1 / np.sqrt(np.diag(A))
    ev = np.linalg.eigvalsh((A * s[:, None] * s[None, :]).astype(np.float64))
    return float(ev[-1] / ev[0])


def res(W, D, kappa=None):
    A, Wl = _sym_lower(D, LD), np.asarray(W).astype(LD)
    return float(np.max(np.abs(Wl @ A @ Wl.T - np.eye(A.shape[0], dtype=LD))) / (EPS * (kappa or kappa_scaled(D))))


def fwd(W, D, W_ref=None, kappa=None):
    W_ref = reference_W(D) if W_ref is None else W_ref
    rows = np.max(np.abs(np.asarray(W).astype(LD) - W_ref), axis=1) / np.max(np.abs(W_ref), axis=1)
    return float(np.max(rows) / (EPS * (kappa or kappa_scaled(D))))


# ---- two host fp64 forms of the same operation -------------------------------------------------------------------------------
def scipy_W(D):
    from scipy.linalg import cholesky, solve_triangular
    A = _sym_lower(D, np.float64)
    return solve_triangular(cholesky(A, lower=True), np.eye(A.shape[0]), lower=True)


DEFECTS = ("rcp_without_e2", "rsq_without_e2", "one_multiplier", "neighbour_pivot")
_EST = 1.0 - 2.0 ** -23   # a hardware estimate "good to 2^-23" (tile_factor.hpp), taken at the edge of that


def ldl_W(D, defect=None):
    """The device's algorithm in plain numpy: LDL^T without pivoting, the multipliers applied to an identity, W = d^-1/2 E.
    defect: one of DEFECTS — what a subtly wrong kernel could compute (tests/test_tile_factor_reference.py: the bounds see each)
      rcp_without_e2   the reciprocal of a pivot as y0 (1 + e), without e^2: good to 2^-46
      rsq_without_e2   the reciprocal square root as y0 (1 + e / 2), without 3 e^2 / 8
      one_multiplier   the multiplier of row 30 at pivot 20 off by 1e-13 relative
      neighbour_pivot  row 20 of W scaled with pivot 21"""
    assert defect is None or defect in DEFECTS
    A = _sym_lower(D, np.float64)
    n = A.shape[0]
    E = np.eye(n)
    d = np.zeros(n)
    for j in range(n):
        piv = d[j] = A[j, j]
        r = 1.0 / piv
        if defect == "rcp_without_e2":
            y0 = r * _EST
            r = y0 + y0 * (1.0 - piv * y0)
        m = A[j + 1:, j] * r
        if defect == "one_multiplier" and j == 20:
            m[30 - 21] *= 1.0 + 1e-13
        A[j + 1:, j + 1:] -= np.outer(m, A[j, j + 1:])
        E[j + 1:] -= np.outer(m, E[j])
    rs = 1.0 / np.sqrt(d)
    if defect == "rsq_without_e2":
        y0 = rs * _EST
        rs = y0 + y0 * 0.5 * (1.0 - d * y0 * y0)
    if defect == "neighbour_pivot":
        rs[20] = rs[21]
    return rs[:, None] * E


HOST_FORMS = (("scipy", scipy_W), ("ldl", ldl_W))


# ---- the tiles ------------------------------------------------------------------------------------------------------------------
# What the LM loop can put on a tile's diagonal: clamp(diag J^T J, min_lm_diagonal, max_lm_diagonal) / radius with the radius between
# min_trust_region_radius and max_trust_region_radius (rsba_amd/csrc/solver.hip: launch_clamp_diagonal, the radius rules of the loop;
# defaults in rsba_default_options, rsba_amd/csrc/capi.hip).  The scale family multiplies one tile by 2^k from below the one end to the other.
MIN_LM_DIAGONAL, MAX_LM_DIAGONAL = 1e-6, 1e32
MIN_RADIUS, MAX_RADIUS = 1e-32, 1e16
K_LO = int(np.floor(np.log2(MIN_LM_DIAGONAL / MAX_RADIUS)))   # -74
K_HI = int(np.ceil(np.log2(MAX_LM_DIAGONAL / MIN_RADIUS)))    # 213
SCALE_EXPONENTS = (-80, K_LO, -37, 1, 105, K_HI)
IDENTITY_ROW_SETS = {"edges": (0, 15, 16, 17, 31, 32, 47), "row15": (15,), "row16": (16,), "row32": (32,), "last1": (47,), "last6": tuple(range(42, 48)),
                     "last47": tuple(range(1, 48))}
FAIL_POSITIONS = (0, 15, 16, 31, 32, 47)
ULP1 = 2.0 ** -52


def _sym(D):
    return (D + D.T) / 2


# (The tiles are built from elementwise operations and numpy's own sums only — no BLAS or LAPACK call, whose order of summation depends on
# the processor — so that every machine meets the same bits and the measured ratios below mean the same thing everywhere.)
def _gram(B):
    return (B[:, None, :] * B[None, :, :]).sum(axis=2)   # B B^T


def spectrum_tile(rng, kappa, one_small=False):
    """Q diag(lambda) Q^T, Q a product of four random reflections: lambda geometric between 1 and 1 / kappa, or all one but the smallest."""
    lam = np.ones(T) if one_small else kappa ** (-np.arange(T) / (T - 1.0))
    lam[-1] = 1.0 / kappa
    A = np.diag(lam)
    for _ in range(4):   # A <- H A H, H = I - 2 v v^T
        v = rng.standard_normal(T)
        v /= np.sqrt((v * v).sum())
        Av = (A * v).sum(axis=1)
        A = A - 2.0 * np.outer(v, Av) - 2.0 * np.outer(Av, v) + 4.0 * (v * Av).sum() * np.outer(v, v)
        A = _sym(A)
    return A


def wellcond_tile(rng):
    return _sym(_gram(rng.uniform(-0.5, 0.5, (T, T))) + 2.0 * np.eye(T))   # kappa about 10, every entry coupled


def bench_tile():
    """The tile of tools/tile_factor_bench.hip: B B^T + 0.1 I, B from its 64-bit LCG."""
    st, B = 12345, np.empty(T * T)
    for i in range(T * T):
        st = (st * 6364136223846793005 + 1442695040888963407) % 2 ** 64
        B[i] = (st >> 11) * (1.0 / 9007199254740992.0) - 0.5
    return _sym(_gram(B.reshape(T, T)) + 0.1 * np.eye(T))


def with_identity_rows(D, rows):
    D = D.copy()
    rows = list(rows)
    D[rows, :] = 0.0
    D[:, rows] = 0.0
    D[rows, rows] = 1.0
    return D


def pose_block_tile(rng):
    D = np.zeros((T, T))
    for b in range(T // 6):
        J = rng.standard_normal((12, 6)) * 10.0 ** rng.uniform(-2, 2, 6)   # columns of a pose Jacobian differ in scale
        D[6 * b:6 * b + 6, 6 * b:6 * b + 6] = _gram(J.T.copy()) + 1e-6 * np.eye(6)
    return _sym(D)


ZERO_BLOCKS = ((1, 0), (2, 1))   # of the second block_diagonal tile; W has exact zeros in the same blocks (L_10 = 0, hence L_21 = (D_21 - L_20 L_10^T) L_11^-T = 0)


def zero_blocks_tile(rng):
    G = _sym(rng.uniform(-0.5, 0.5, (T, T)))
    for bi, bj in ZERO_BLOCKS:
        G[16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16] = 0.0
        G[16 * bj:16 * bj + 16, 16 * bi:16 * bi + 16] = 0.0
    return G + 5.0 * np.eye(T)   # (the spectrum of G lies within about +-4)


def pivot_edge_tile(rng, pivots):
    """diag(pivots) plus a coupling of 2^-30: the Schur updates (2^-60) are below half an ulp of every pivot, so the factorisation meets
    exactly these pivots — where the hardware estimates of 1 / x and x^-1/2 and their hand refinement are at their worst."""
    D = _sym(rng.uniform(-1.0, 1.0, (T, T))) * 2.0 ** -30 * np.sqrt(np.outer(pivots, pivots))
    D[np.arange(T), np.arange(T)] = pivots
    return D


@functools.lru_cache(maxsize=None)
def passing_tiles():
    """About 40 seeded tiles, in the order of the batch.  The bench tile stands at several places of it (first, either side of the tile of
    the largest scale, last): tests/test_gpu_tile_factor.py asks for the same bits at each."""
    rng = np.random.default_rng(4848)
    out = [Tile("bench", "bench", bench_tile())]
    out.append(Tile("kappa1", "kappa1", spectrum_tile(rng, 1.0)))
    for e in (2, 4, 6, 8, 10, 12):
        out.append(Tile("spectrum", f"geometric_1e{e}", spectrum_tile(rng, 10.0 ** e)))
    for e in (4, 8, 12):
        out.append(Tile("spectrum", f"one_small_1e{e}", spectrum_tile(rng, 10.0 ** e, one_small=True)))
    base = spectrum_tile(rng, 1e3)
    for name, ex in (("random", rng.integers(-40, 21, T)), ("descending", -np.arange(T)), ("ascending", np.arange(T) - (T - 1))):
        s = 2.0 ** ex.astype(np.float64)
        out.append(Tile("graded", name, base * np.outer(s, s)))
    base = wellcond_tile(rng)
    for k in SCALE_EXPONENTS:
        if k == K_HI:
            out.append(Tile("bench", "bench", out[0].D))
        out.append(Tile("scale", f"2^{k}", base * 2.0 ** k))
        if k == K_HI:
            out.append(Tile("bench", "bench", out[0].D))
    base = spectrum_tile(rng, 1e2)
    for name, rows in IDENTITY_ROW_SETS.items():
        out.append(Tile("identity_rows", name, with_identity_rows(base, rows)))
    out.append(Tile("identity_rows", "identity", np.eye(T)))
    out.append(Tile("block_diagonal", "pose_blocks", pose_block_tile(rng)))
    out.append(Tile("block_diagonal", "zero_blocks", zero_blocks_tile(rng)))
    for name, piv in (("powers_of_two", 2.0 ** ((np.arange(T) * 7) % 13 - 6.0)), ("one_plus_ulp", np.full(T, 1.0 + ULP1)), ("one_minus_ulp", np.full(T, 1.0 - ULP1 / 2)),
                      ("two_minus_ulp", np.full(T, 2.0 - ULP1)), ("three", np.full(T, 3.0))):
        out.append(Tile("pivot_edges", name, pivot_edge_tile(rng, piv)))
    out.append(Tile("bench", "bench", out[0].D))
    return tuple(out)


def pivots(D):
    """The pivots of the LDL^T without pivoting, in long double."""
    A = _sym_lower(D, LD)
    d = np.zeros(A.shape[0], LD)
    for j in range(A.shape[0]):
        d[j] = A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j] / d[j], A[j, j + 1:])
    return d


@functools.lru_cache(maxsize=None)
def failing_tiles():
    """Tiles that are not positive definite; every entry finite or +inf, never a NaN (the follower wave waits on the all-ones pattern by
    design: a payload that equals it would hang, and the elimination posts all sixteen messages of a block whatever ok becomes)."""
    out = []
    base = bench_tile()
    piv = pivots(base)
    for p in FAIL_POSITIONS:   # symmetric indefinite: pivot p becomes minus what it was, the pivots before it stay
        D = base.copy()
        D[p, p] -= 2.0 * float(piv[p])
        out.append(Tile("indefinite", f"negative_pivot_{p}", D))
    for p in FAIL_POSITIONS:   # an exactly zero pivot: 1 - 2 * (2 / 4) behind a pivot of 4 (at 16 and 32 the update comes from the block product), or a zero diagonal entry
        D = 4.0 * np.eye(T)
        if p == 0:
            D[0, 0] = 0.0
        else:
            D[p, p], D[p, p - 1], D[p - 1, p] = 1.0, 2.0, 2.0
        out.append(Tile("zero_pivot", f"zero_pivot_{p}", D))
    D = base.copy()
    D[20, 20] = np.inf
    out.append(Tile("inf", "inf_diagonal_20", D))
    for t in out:
        assert not np.isnan(t.D).any() and not np.isneginf(t.D).any()
    return tuple(out)


# ---- the files of `tile_factor_bench --check IN OUT` ---------------------------------------------------------------------------
CHECK_RECORD = np.dtype([("ok", "<i4", (2,)), ("W", "<f8", (2, T, T)), ("published", "<f8", (T, T))])   # per tile; index 0 = plain form, 1 = the DAG form


def write_tiles(path, tiles):
    with open(path, "wb") as f:
        f.write(np.int32(len(tiles)).tobytes())
        for t in tiles:
            f.write(np.ascontiguousarray(t.D, dtype="<f8").tobytes())


def read_check(path, n):
    raw = open(path, "rb").read()
    assert len(raw) == 4 + n * CHECK_RECORD.itemsize and int(np.frombuffer(raw, "<i4", 1)[0]) == n, (len(raw), n)
    return np.frombuffer(raw, CHECK_RECORD, n, 4).copy()
