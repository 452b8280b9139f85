"""The serial core of the tile Cholesky on its own (tools/tile_factor_bench.hip includes rsba_amd/csrc/tile_factor.hpp, the library's tile
factorisation, and tools/tile_factor_baselines.hpp, its earlier forms): W = chol(D)^-1 of one 48 x 48 tile by one workgroup — the MFMA-pivot
LDL^T on two waves that the DIAG tasks run (plain, with phase stamps, and publishing W by row blocks as the persistent driver does), round 2's
MFMA second wave and the round-1 lane-per-row form — each against a host factorisation of the same tile.

`tile_factor_bench --check`: every tile of tests/tile_factor_reference.py through one launch of the tool's check mode (one workgroup per tile,
a few dozen workgroups, each arming its own pivot messages): factor_invert_tile plain (form 0) and publishing W by row blocks as
diag_factor runs it (form 1).  res and fwd in units of 2^-53 kappa_scaled, worst per family; host = the worse of the two host fp64 forms
(tests/test_tile_factor_reference.py), device = an MI355X, both forms (they are bit-equal).  The three calls of the tool (38 tiles, the same again, 13 failing
tiles) take 0.3 s each.

  family           res: host   device   C_RES    fwd: host   device   C_FWD
  kappa1                3.00   3.00      16            1.50   1.50      8
  spectrum              0.58   0.33      4             0.29   0.17      2
  graded                0.049  0.050     0.25          0.30   0.22      2
  scale                 1.19   1.20      8             0.60   0.60      4
  identity_rows         0.96   0.96      4             0.48   0.48      2
  block_diagonal        2.32   2.32      16            1.16   1.16      8
  bench                 0.15   0.22      1             0.098  0.17      0.5
  pivot_edges           3.00   3.00      16            1.50   1.50      8"""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import tile_factor_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "tile_factor_bench")
# the tool's five rows: lane-per-row baseline, the library's form (rows follower), the same with stamps, the MFMA follower baseline, W published by row blocks
VARIANTS = ["lane-per-row potrf + blocked inverse", "MFMA-pivot LDL^T, W by rows (round 3)", "the same with phase stamps",
            "MFMA-pivot LDL^T, W by MFMAs (round 2)", "round 3 + W published by row blocks"]


@pytest.mark.gpu
def test_tile_factor_and_inverse_match_a_host_factorisation():
    if not os.path.exists(TOOL):
        pytest.skip("tools/tile_factor_bench is not built (python __graft_entry__.py builds it)")
    out = subprocess.run([TOOL], capture_output=True, text=True, timeout=120).stdout
    rows = re.findall(r"^(.*?): *([0-9.]+) us per tile .*?\|W A W\^T - I\| = ([0-9.e+-]+), \|W - W_host\| = ([0-9.e+-]+) \(\|W\| = ([0-9.e+-]+)\), (.*)$", out, re.M)
    assert [r[0].strip() for r in rows] == VARIANTS, out   # every variant, by name: a baseline must not fall out of the tool unnoticed
    for name, us, err_id, err_ref, wmax, status in rows:
        assert status.strip() == "no error", (name, status)
        assert float(err_id) <= 1e-13, (name, err_id)                 # W D W^T = I: backward stable on a tile of condition ~1e2
        assert float(err_ref) <= 1e-13 * max(1.0, float(wmax)), (name, err_ref)


# ---- `tile_factor_bench --check`: the library's two forms against the extended-precision reference ------------------------------------
FORMS = ("plain", "published")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    """The tool's three calls, once per module: the passing tiles, the same file again, the failing tiles.  A call that fails stops the rest."""
    if not os.path.exists(TOOL):
        pytest.skip("tools/tile_factor_bench is not built (python __graft_entry__.py builds it)")
    d = tmp_path_factory.mktemp("tile_check")
    out = {}
    for key, tiles in (("pass", R.passing_tiles()), ("again", R.passing_tiles()), ("fail", R.failing_tiles())):
        src, dst = str(d / (key + "_in.bin")), str(d / (key + "_out.bin"))
        R.write_tiles(src, tiles)
        t0 = time.perf_counter()
        run = subprocess.run([TOOL, "--check", src, dst], capture_output=True, text=True, timeout=60)
        print(f"tile_factor_bench --check, {key}: {len(tiles)} tiles, {time.perf_counter() - t0:.2f} s")
        assert run.returncode == 0, (key, run.returncode, run.stderr)
        out[key] = R.read_check(dst, len(tiles))
    return out


@pytest.fixture(scope="module")
def refs():
    """kappa_scaled and the long-double W of every passing tile, once."""
    out = {}
    for t in R.passing_tiles():
        if t.name not in out:
            out[t.name] = (R.kappa_scaled(t.D), R.reference_W(t.D))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("form", (0, 1), ids=FORMS)
def test_tile_factor_against_the_extended_precision_reference(checked, refs, form, family):
    worst = [0.0, 0.0]
    for i, t in enumerate(R.passing_tiles()):
        if t.family != family:
            continue
        W, (kappa, W_ref) = checked["pass"]["W"][i, form], refs[t.name]
        assert checked["pass"]["ok"][i, form] == 1, t.name
        assert np.isfinite(W).all(), t.name
        r, f = R.res(W, t.D, kappa), R.fwd(W, t.D, W_ref, kappa)
        print(f"{FORMS[form]} {family} {t.name}: res {r:.3g} (C {R.C_RES[family]:g})  fwd {f:.3g} (C {R.C_FWD[family]:g})  kappa {kappa:.3g}")
        worst = [max(worst[0], r), max(worst[1], f)]
        assert np.all(np.triu(W, 1) == 0.0), t.name   # exact zeros above the diagonal
        if t.name in R.IDENTITY_ROW_SETS or t.name == "identity":
            rows = list(R.IDENTITY_ROW_SETS.get(t.name, range(R.T)))
            assert np.array_equal(W[rows, :], np.eye(R.T)[rows, :]) and np.array_equal(W[:, rows], np.eye(R.T)[:, rows]), t.name
        if t.name == "pose_blocks":
            assert np.all(W[np.kron(np.eye(R.T // 6), np.ones((6, 6))) == 0] == 0.0)
        if t.name == "zero_blocks":
            for bi, bj in R.ZERO_BLOCKS:
                assert np.all(W[16 * bi:16 * bi + 16, 16 * bj:16 * bj + 16] == 0.0), (bi, bj)
    print(f"{FORMS[form]} {family}: worst res {worst[0]:.3g}  fwd {worst[1]:.3g}")
    assert worst[0] <= R.C_RES[family] and worst[1] <= R.C_FWD[family], (family, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ("pass", "fail"))
def test_published_copy_is_complete_and_equals_W(checked, key):
    rec = checked[key]
    assert not np.any(bits(rec["published"]) == R.EMPTY)   # no cell still holds the empty pattern, whatever became of the factorisation
    assert not np.any(bits(rec["W"]) == R.EMPTY)           # and none of the 16-blocks on or below the diagonal of W in LDS was left unwritten
    for b in range(2):   # exact zeros right of each row block's diagonal block
        assert np.all(bits(rec["published"][:, 16 * b:16 * b + 16, 16 * (b + 1):]) == 0)
    if key == "pass":
        assert np.array_equal(bits(rec["published"]), bits(rec["W"][:, 1]))


@pytest.mark.gpu
def test_forms_positions_and_repeats_give_the_same_bits(checked):
    rec = checked["pass"]
    assert np.array_equal(bits(rec["W"][:, 0]), bits(rec["W"][:, 1]))          # plain and publishing form
    where = [i for i, t in enumerate(R.passing_tiles()) if t.name == "bench"]
    names = [t.name for t in R.passing_tiles()]
    assert where[0] == 0 and where[-1] == len(names) - 1 and len(where) == 4 and names[where[1] + 1] == f"2^{R.K_HI}" == names[where[2] - 1]
    for i in where[1:]:   # the same tile first, last and either side of the tile of the largest scale
        assert np.array_equal(bits(rec["W"][i]), bits(rec["W"][0])) and np.array_equal(bits(rec["published"][i]), bits(rec["published"][0])), i
    assert checked["again"].tobytes() == rec.tobytes()                           # a second call on the same file


@pytest.mark.gpu
@pytest.mark.parametrize("name", [t.name for t in R.failing_tiles()])
def test_a_tile_that_is_not_positive_definite_is_reported(checked, name):
    # (that the call came back within its time limit and exited 0 is the fixture's assertion; nothing is asked of W)
    i = [t.name for t in R.failing_tiles()].index(name)
    assert checked["fail"]["ok"][i].tolist() == [0, 0], name
