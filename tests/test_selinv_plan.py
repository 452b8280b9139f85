"""The selected-inverse plan (rsba_amd/csrc/chol_plan.hpp: selinv_plan), checked on the host from its lists alone:
rsba_debug_selinv_plan — instrumented library only — orders a tile graph and plans its Cholesky as the solver does (one rank), then
lists the G / OFF / DIAG items of the Takahashi recurrence level by level, descending.  No GPU.

The device runs one launch per (level, kind) and nobody waits inside a launch (kernels_selinv.hip): an item that names a tile of a
later launch reads garbage there.  So, for the tile graphs of tests/test_chol_plan.py and every leaf size:
  * every packed slot of Sigma has exactly one producer;
  * every Sigma operand of an OFF item is produced at an earlier position (a higher level), every Sigma operand of a DIAG item by an
    OFF item of its own column, every G operand by the G item of that tile;
  * every operand is the tile the recurrence means: (i, k) or, transposed, (k, i), and (k, j);
  * replaying the lists in numpy on a random symmetric positive definite matrix with that tile pattern gives the dense inverse on the
    pattern to 1e-10 of its largest entry.  The matrix is diagonally dominant — diagonal = absolute row sum + 1, entries in [-1, 1] —,
    so its eigenvalues lie in [1, 2 * row sum + 1] (Gershgorin): a condition number of a few hundred at most, 1e-10 is four orders
    above what fp64 leaves.  Tiles are 3 x 3 here: the lists know nothing of the tile size."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import HOOKS_LIB  # noqa: E402
from test_chol_plan import EMIT, GRAPHS, LEAVES  # noqa: E402

B = 3   # tile size of the numeric replay


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    return C.CDLL(HOOKS_LIB)


def plan(lib, nt, edges):
    out = {}

    def take(_ctx, name, data, count):
        out[name.decode()] = np.ctypeslib.as_array(data, shape=(count,)).copy() if count else np.zeros(0, dtype=np.int32)

    e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    rc = lib.rsba_debug_selinv_plan(C.c_int32(nt), C.c_int32(len(e)), e.ctypes.data_as(C.c_void_p), EMIT(take), None)
    assert rc == 0, "the plan found an (i, k) pair of a column's rows without a slot"
    for k in ("g_info", "off_info", "diag_info", "slot_tiles"):
        out[k] = out[k].reshape(-1, 2)
    out["off_list"] = out["off_list"].reshape(-1, 3)
    out["nlev"], out["nslots"], out["nt"] = (int(v) for v in out["meta"])
    return out


def check_lists(p, nt):
    nlev, nslots = p["nlev"], p["nslots"]
    assert p["nt"] == nt and len(p["diag_info"]) == nt
    iperm = np.empty(nt, dtype=np.int64)
    iperm[p["perm"]] = np.arange(nt)
    st = p["slot_tiles"]
    assert np.all(iperm[st[:, 0]] >= iperm[st[:, 1]])                      # a packed tile is (row, column) with row >= column in the new order
    for name, n in (("g", len(p["g_info"])), ("off", len(p["off_info"])), ("diag", nt)):
        ptr = p[f"lev_{name}_ptr"]
        assert len(ptr) == nlev + 1 and ptr[0] == 0 and ptr[-1] == n and np.all(np.diff(ptr) >= 0)
    pos_g = np.repeat(np.arange(nlev), np.diff(p["lev_g_ptr"]))
    pos_o = np.repeat(np.arange(nlev), np.diff(p["lev_off_ptr"]))
    pos_d = np.repeat(np.arange(nlev), np.diff(p["lev_diag_ptr"]))
    # position p is elimination level nlev - 1 - p: descending
    assert np.array_equal(p["level"][iperm[p["diag_info"][:, 1]]], nlev - 1 - pos_d)
    # one producer per Sigma slot; one G item per sub-diagonal slot
    producers = np.concatenate([p["off_info"][:, 0], p["diag_info"][:, 0]])
    assert sorted(producers) == list(range(nslots)), "a packed slot of Sigma without exactly one producer"
    assert sorted(p["g_info"][:, 0]) == sorted(p["off_info"][:, 0])
    sigma_pos = np.empty(nslots, dtype=np.int64); sigma_is_off = np.zeros(nslots, dtype=bool)
    sigma_pos[p["off_info"][:, 0]] = pos_o; sigma_is_off[p["off_info"][:, 0]] = True
    sigma_pos[p["diag_info"][:, 0]] = pos_d
    g_pos = np.full(nslots, -1, dtype=np.int64)
    g_pos[p["g_info"][:, 0]] = pos_g
    for g, (slot, tile) in enumerate(p["g_info"]):
        assert st[slot, 1] == tile and st[slot, 0] != tile
    assert len(p["off_ptr"]) == len(p["off_info"]) + 1 and p["off_ptr"][0] == 0 and p["off_ptr"][-1] == len(p["off_list"])
    for t, (out, tile_j) in enumerate(p["off_info"]):
        i, j = st[out]
        assert j == tile_j and i != j
        terms = p["off_list"][p["off_ptr"][t]:p["off_ptr"][t + 1]]
        ks = []
        for ss, trans, gs in terms:
            k = st[gs, 0]
            ks.append(int(k))
            assert st[gs, 1] == j and g_pos[gs] == pos_o[t], "G operand of another column or another launch"
            assert tuple(st[ss]) == ((k, i) if trans else (i, k)), "Sigma operand is not tile (i, k)"
            assert not (trans and i == k)
            assert sigma_pos[ss] < pos_o[t], "an OFF item reads a Sigma tile that is not finished before its launch"
        # the sum runs over every row tile of the column, once, in the order of the column's slots
        col_rows = [int(st[s, 0]) for s in range(nslots) if st[s, 1] == j and st[s, 0] != j]
        assert ks == col_rows
    assert len(p["diag_ptr"]) == nt + 1 and p["diag_ptr"][0] == 0 and p["diag_ptr"][-1] == len(p["diag_list"])
    for d, (out, tile_j) in enumerate(p["diag_info"]):
        assert tuple(st[out]) == (tile_j, tile_j)
        slots = p["diag_list"][p["diag_ptr"][d]:p["diag_ptr"][d + 1]]
        assert list(slots) == [s for s in range(nslots) if st[s, 1] == tile_j and st[s, 0] != tile_j]
        for s in slots:
            assert sigma_is_off[s] and sigma_pos[s] == pos_d[d] and g_pos[s] == pos_d[d], "a DIAG item reads what its own level's OFF launch does not produce"


def replay(p, nt, edges, seed):
    """max |Sigma (lists replayed) - A^-1| over the pattern / max |A^-1|, A random, diagonally dominant, with the graph's tile pattern."""
    rng = np.random.default_rng(seed)
    n = nt * B
    A = np.zeros((n, n))
    for a, b in edges:
        blk = rng.uniform(-1.0, 1.0, (B, B))
        A[a * B:(a + 1) * B, b * B:(b + 1) * B] = blk
        A[b * B:(b + 1) * B, a * B:(a + 1) * B] = blk.T
    for t in range(nt):
        blk = rng.uniform(-1.0, 1.0, (B, B))
        A[t * B:(t + 1) * B, t * B:(t + 1) * B] = np.tril(blk, -1) + np.tril(blk, -1).T
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(axis=1) + 1.0
    # the factor in the plan's order, cut into its tiles (old tile numbers, as slot_tiles names them)
    idx = (np.asarray(p["perm"], dtype=np.int64)[:, None] * B + np.arange(B)[None, :]).reshape(-1)
    L = np.linalg.cholesky(A[np.ix_(idx, idx)])
    Lfull = np.zeros((n, n))
    Lfull[np.ix_(idx, idx)] = L                               # entry (old row, old column) of the permuted factor
    tile = lambda M, r, c: M[r * B:(r + 1) * B, c * B:(c + 1) * B]  # noqa: E731
    st = p["slot_tiles"]
    # the factor has nothing outside the packed slots (the symbolic factorisation covers the fill)
    mask = np.zeros((nt, nt), dtype=bool)
    mask[st[:, 0], st[:, 1]] = True
    assert all(mask[r, c] or not tile(Lfull, r, c).any() for r in range(nt) for c in range(nt))
    W = {int(t): np.linalg.inv(tile(Lfull, t, t)) for t in range(nt)}
    Lf = {s: tile(Lfull, st[s, 0], st[s, 1]) for s in range(p["nslots"])}
    G, Sg = {}, {}
    for pos in range(p["nlev"]):
        for g in range(p["lev_g_ptr"][pos], p["lev_g_ptr"][pos + 1]):
            slot, t = p["g_info"][g]
            G[int(slot)] = Lf[int(slot)] @ W[int(t)]
        for t in range(p["lev_off_ptr"][pos], p["lev_off_ptr"][pos + 1]):
            acc = np.zeros((B, B))
            for ss, trans, gs in p["off_list"][p["off_ptr"][t]:p["off_ptr"][t + 1]]:
                acc -= (Sg[int(ss)].T if trans else Sg[int(ss)]) @ G[int(gs)]
            Sg[int(p["off_info"][t, 0])] = acc
        for d in range(p["lev_diag_ptr"][pos], p["lev_diag_ptr"][pos + 1]):
            out, t = p["diag_info"][d]
            X = W[int(t)].T @ W[int(t)]
            for s in p["diag_list"][p["diag_ptr"][d]:p["diag_ptr"][d + 1]]:
                X -= Sg[int(s)].T @ G[int(s)]
            Sg[int(out)] = 0.5 * (X + X.T)
    inv = np.linalg.inv(A)
    worst = max(float(np.abs(Sg[s] - tile(inv, st[s, 0], st[s, 1])).max()) for s in range(p["nslots"]))
    return worst / float(np.abs(inv).max())


@pytest.mark.parametrize("name", list(GRAPHS))
def test_selected_inverse_plan_of_a_graph(lib, monkeypatch, name):
    nt, edges = GRAPHS[name]
    for leaf in LEAVES:
        if leaf is None:
            monkeypatch.delenv("RSBA_CHOL_LEAF", raising=False)
        else:
            monkeypatch.setenv("RSBA_CHOL_LEAF", leaf)
        try:
            p = plan(lib, nt, edges)
            check_lists(p, nt)
            err = replay(p, nt, edges, seed=7)
            assert err <= 1e-10, f"replayed lists miss the dense inverse on the pattern: {err:.2e}"
        except AssertionError as e:
            raise AssertionError(f"leaf {leaf}: {e}") from e


def test_the_release_library_has_no_debug_entry(lib):
    from rsba_amd import capi
    assert hasattr(lib, "rsba_debug_selinv_plan") and not hasattr(C.CDLL(capi.LIB_PATH), "rsba_debug_selinv_plan")
