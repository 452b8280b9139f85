"""The extended-precision reference of the 48 x 48 tile factor (tests/tile_factor_reference.py) against mpmath, the calibration of the
bounds that tests/test_gpu_tile_factor.py puts on the device's W = chol(D)^-1, and proof that those bounds see a subtly wrong kernel.

reference_W (long double) against a 60-digit mpmath Cholesky and triangular inverse, row-wise as fwd, in units of 2^-64 kappa_scaled:
kappa = 1: below 1e-3 (the tile is the identity up to rounding), kappa = 1e12: 0.054, graded: 0.19, identity rows: 0.094 — bound 8, a small
multiple, as for any backward-stable factorisation in its own precision (the fp64 forms below reach 1.5 in theirs).

The two host fp64 forms (scipy's cholesky + solve_triangular; the device's algorithm in numpy, ldl_W), worst ratio per family in units of
2^-53 kappa_scaled, and the constants C = 4 x worst rounded up to a power of two (tile_factor_reference.C_RES / C_FWD):

  family           res: scipy   ldl     C_RES    fwd: scipy   ldl     C_FWD
  kappa1                3.00    3.00    16            1.50    1.50    8
  spectrum              0.45    0.58    4             0.23    0.29    2
  graded                0.029   0.049   0.25          0.23    0.30    2
  scale                 0.39    1.19    8             0.22    0.60    4
  identity_rows         0.96    0.96    4             0.48    0.48    2
  block_diagonal        1.52    2.32    16            0.76    1.16    8
  bench                 0.079   0.15    1             0.071   0.098   0.5
  pivot_edges           3.00    3.00    16            1.50    1.50    8

(kappa1, pivot_edges and the all-but-one-row identity tile of identity_rows have kappa = 1: their unit is eps itself, and what both forms
reach there is the rounding of 1 / sqrt(d) — correctly rounded in both, hence equal.)

Seeded defects of ldl_W, as a multiple of the named family's constant (above 1 fails the bound):
  the reciprocal without e^2 (good to 2^-46)             bench res 10.9, fwd 17; graded res 9.2
  the reciprocal square root without 3 e^2 / 8          kappa1 24, pivot_edges 24, scale 6.0 (res and fwd alike)
  one multiplier off by 1e-13                           bench fwd 3.0
  one row of W scaled with the neighbouring pivot       bench, spectrum, graded: above 1e3"""
import math

import numpy as np
import pytest

import mpmath

import tile_factor_reference as R

C_MPMATH = 8.0


def by_name(name):
    return next(t for t in R.passing_tiles() if t.name == name)


def mpmath_W(D):
    """chol(D)^-1 with 60 digits: mpmath's Cholesky, then the rows of the inverse by forward substitution."""
    n = D.shape[0]
    with mpmath.workdps(60):
        A = mpmath.matrix(n, n)
        for i in range(n):
            for j in range(n):
                A[i, j] = mpmath.mpf(float(D[max(i, j), min(i, j)]))
        L = mpmath.cholesky(A)
        W = [[mpmath.mpf(0)] * n for _ in range(n)]
        for i in range(n):
            for c in range(i + 1):
                s = mpmath.mpf(1 if i == c else 0)
                for k in range(c, i):
                    s -= L[i, k] * W[k][c]
                W[i][c] = s / L[i, i]
        # as long doubles: head + tail of each entry (a long double holds 64 bits, two doubles give 106)
        out = np.zeros((n, n), R.LD)
        for i in range(n):
            for c in range(i + 1):
                hi = float(W[i][c])
                out[i, c] = R.LD(hi) + R.LD(float(W[i][c] - mpmath.mpf(hi)))
    return out


@pytest.mark.parametrize("name", ["kappa1", "geometric_1e12", "random", "edges"])
def test_reference_W_matches_mpmath(name):
    D = by_name(name).D
    W_ref, W_mp, kappa = R.reference_W(D), mpmath_W(D), R.kappa_scaled(D)
    rows = np.max(np.abs(W_ref - W_mp), axis=1) / np.max(np.abs(W_mp), axis=1)
    ratio = float(np.max(rows)) / (2.0 ** -64 * kappa)
    print(f"{name}: reference_W against mpmath {ratio:.3g} x 2^-64 kappa, kappa {kappa:.3g}")
    assert ratio <= C_MPMATH, (ratio, kappa)
    assert np.all(np.triu(W_ref, 1) == 0)


def test_yardsticks_on_a_tile_with_a_known_inverse():
    D = np.diag(4.0 ** np.arange(R.T))   # W = diag(2^-i) exactly, at any grading
    W = np.diag(2.0 ** -np.arange(R.T))
    assert R.kappa_scaled(D) == 1.0 and np.array_equal(R.reference_W(D).astype(np.float64), W)
    assert R.res(W, D) == 0.0 and R.fwd(W, D) == 0.0
    W[7, 7] *= 1 + 2.0 ** -50   # 8 eps relative on one entry: 8 in fwd, 16 in res
    assert R.fwd(W, D) == pytest.approx(8.0) and R.res(W, D) == pytest.approx(16.0, rel=1e-6)


@pytest.fixture(scope="module")
def measured():
    """Per tile (duplicates of the batch left out): kappa, W_ref, and (res, fwd) of each host form."""
    out = {}
    for t in R.passing_tiles():
        if t.name in out:
            continue
        kappa, W_ref = R.kappa_scaled(t.D), R.reference_W(t.D)
        out[t.name] = (t, kappa, W_ref, {form: (R.res(f(t.D), t.D, kappa), R.fwd(f(t.D), t.D, W_ref, kappa)) for form, f in R.HOST_FORMS})
    return out


def test_the_tiles_are_what_they_claim(measured):
    fams = [t.family for t in R.passing_tiles()]
    assert set(fams) == set(R.FAMILIES) == set(R.C_RES) == set(R.C_FWD) and 30 <= len(fams) <= 48
    for t, kappa, W_ref, _ in measured.values():
        assert t.D.shape == (R.T, R.T) and np.array_equal(t.D, t.D.T) and np.isfinite(W_ref).all(), t.name
    kap = {n: m[1] for n, m in measured.items()}
    assert kap["kappa1"] < 1 + 1e-12 and kap["identity"] == 1.0
    for e in (2, 4, 6, 8, 10, 12):
        assert 0.1 * 10.0 ** e <= kap[f"geometric_1e{e}"] <= 10.0 ** (e + 0.5)
    assert kap["random"] == pytest.approx(kap["ascending"], rel=1e-9) and 1e2 <= kap["random"] <= 1e4      # grading leaves the unit alone
    assert len({round(kap[f"2^{k}"], 9) for k in R.SCALE_EXPONENTS}) == 1 and (R.K_LO, R.K_HI) == (-74, 213)   # and so does scale
    for name, piv in (("one_plus_ulp", 1 + 2.0 ** -52), ("one_minus_ulp", 1 - 2.0 ** -53), ("two_minus_ulp", 2 - 2.0 ** -52), ("three", 3.0)):
        assert np.all(R.pivots(by_name(name).D).astype(np.float64) == piv), name   # the pivots the factorisation meets are exactly these
    p2 = R.pivots(by_name("powers_of_two").D).astype(np.float64)
    assert np.all(np.frexp(p2)[0] == 0.5)
    for t in R.failing_tiles():
        assert not np.isnan(t.D).any() and np.array_equal(t.D, t.D.T)
        with np.errstate(all="ignore"):
            piv = R.pivots(t.D).astype(np.float64)
        p = int(t.name.rsplit("_", 1)[1])
        assert np.all(piv[:p] > 0) and np.all(np.isfinite(piv[:p])) and not (piv[p] > 0 and np.isfinite(piv[p])), t.name
        if t.family == "zero_pivot":
            assert piv[p] == 0.0


def test_calibration_of_the_bounds(measured):
    worst = {f: {form: [0.0, 0.0] for form, _ in R.HOST_FORMS} for f in R.FAMILIES}
    for t, kappa, W_ref, forms in measured.values():
        for form, (r, f) in forms.items():
            w = worst[t.family][form]
            w[0], w[1] = max(w[0], r), max(w[1], f)
    for fam in R.FAMILIES:
        w = worst[fam]
        print(f"{fam:15s} res: scipy {w['scipy'][0]:.3g} ldl {w['ldl'][0]:.3g}  C_RES {R.C_RES[fam]:g}   fwd: scipy {w['scipy'][1]:.3g} ldl {w['ldl'][1]:.3g}  C_FWD {R.C_FWD[fam]:g}")
    for fam in R.FAMILIES:
        for q, C in ((0, R.C_RES[fam]), (1, R.C_FWD[fam])):
            top = max(worst[fam][form][q] for form, _ in R.HOST_FORMS)
            assert C == 2.0 ** round(math.log2(C)), (fam, C)
            assert 4.0 * top <= C, (fam, q, top, C)          # the host forms hold the bounds, with the factor 4 to spare
            assert C < 16.0 * top, (fam, q, top, C)          # and the constant is no looser than the rule makes it (4 x, then at most 2 x of rounding up), give or take what another BLAS moves


# defect -> the families that must see it, and by which yardstick (0 = res, 1 = fwd)
SEEN_BY = {"rcp_without_e2": (("bench", 0), ("bench", 1), ("graded", 0)),
           "rsq_without_e2": (("kappa1", 1), ("pivot_edges", 1), ("scale", 0), ("scale", 1)),
           "one_multiplier": (("bench", 1),),
           "neighbour_pivot": (("bench", 1), ("spectrum", 0), ("graded", 1))}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_the_bounds_see_a_seeded_defect(measured, defect):
    worst = {}
    for t, kappa, W_ref, _ in measured.values():
        W = R.ldl_W(t.D, defect)
        w = worst.setdefault(t.family, [0.0, 0.0])
        w[0], w[1] = max(w[0], R.res(W, t.D, kappa) / R.C_RES[t.family]), max(w[1], R.fwd(W, t.D, W_ref, kappa) / R.C_FWD[t.family])
    print(defect, {f: (round(a, 2), round(b, 2)) for f, (a, b) in worst.items()})
    for fam, q in SEEN_BY[defect]:
        assert worst[fam][q] > 2.0, (defect, fam, q, worst[fam])   # not by a hair: twice the bound at least


def test_check_file_roundtrip(tmp_path):
    tiles = R.passing_tiles()[:3]
    R.write_tiles(tmp_path / "in.bin", tiles)
    raw = (tmp_path / "in.bin").read_bytes()
    assert len(raw) == 4 + 3 * R.T * R.T * 8 and np.array_equal(np.frombuffer(raw, "<f8", R.T * R.T, 4).reshape(R.T, R.T), tiles[0].D)
    rec = np.zeros(3, R.CHECK_RECORD)
    rec["ok"][1] = (1, 0)
    rec["published"][2].view(np.uint64)[:] = R.EMPTY
    (tmp_path / "out.bin").write_bytes(np.int32(3).tobytes() + rec.tobytes())
    back = R.read_check(tmp_path / "out.bin", 3)
    assert R.CHECK_RECORD.itemsize == 8 + 3 * R.T * R.T * 8 and back["ok"][1].tolist() == [1, 0] and np.all(back["published"][2].view(np.uint64) == R.EMPTY)
