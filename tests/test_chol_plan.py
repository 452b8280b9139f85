"""The task graph of the tile Cholesky (rsba_amd/csrc/chol_plan.hpp), checked on the host from its lists alone: rsba_debug_chol_plan
— instrumented library only — orders a tile graph and plans it as the solver does, for one rank of a world.  No GPU.

The device runs the items under a persistent kernel whose tasks wait on write-once cells: a list that names a cell nobody writes, or
a ticket order that is not topological, is a hang there.  Here the ticket orders are replayed with one "written" flag per cell —
what every task kind reads and writes is restated below from the task bodies of chol_tasks.hpp, by cell, without any arithmetic."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import HOOKS_LIB, observation_tiles  # noqa: E402

UPDATE, DIAG, SUB, BACK, FWD2, ETA, FWD2P = range(7)
EMIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.POINTER(C.c_int32), C.c_int64)
# chunk, tail, fuse_last: the defaults and the sets KNOBS of test_gpu_lm_step.py runs (RSBA_CHOL_CHUNK=1 + RSBA_CHOL_TAIL=1, RSBA_CHOL_FUSE=0)
OPTIONS = [(12, 2, 1), (1, 1, 1), (12, 2, 0)]
LEAVES = [None, "1", "2"]          # RSBA_CHOL_LEAF (read inside plan_leaf_size)
WORLDS = [1, 2, 4]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    return C.CDLL(HOOKS_LIB)


def plan(lib, nt, edges, world, rank, two_rhs, opt):
    out = {}

    def take(_ctx, name, data, count):
        out[name.decode()] = np.ctypeslib.as_array(data, shape=(count,)).copy() if count else np.zeros(0, dtype=np.int32)

    e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    rc = lib.rsba_debug_chol_plan(C.c_int32(nt), C.c_int32(len(e)), e.ctypes.data_as(C.c_void_p), C.c_int32(world), C.c_int32(rank), C.c_int32(two_rhs),
                                  C.c_int32(opt[0]), C.c_int32(opt[1]), C.c_int32(opt[2]), EMIT(take), None)
    assert rc == 0
    for k in ("upd", "diag_info", "sub_info", "diag_info_sh", "sub_info_sh"):
        out[k] = out[k].reshape(-1, 4)
    for k in ("diag_list", "sub_list", "back_info", "back_list", "tasks", "tasks_a", "tasks_b", "fwd_full", "fwd_a", "fwd_b", "top_info", "slot_tiles"):
        out[k] = out[k].reshape(-1, 2)
    out["sharded"], out["nlev"], out["nparts"], out["nslots"] = (int(v) for v in out["meta"])
    return out


# ---- what the lists say, item by item ----

def check_items(p, nt):
    """Every packed slot is the output of exactly one DIAG or SUB item; every contributor an item names is the output of an item of an
    earlier level; the chunking is a partition of every contributor list; the look-ahead pairs (diag_fuse, sub_pub) name each other."""
    nd, ns, nu = len(p["diag_info"]), len(p["sub_info"]), len(p["upd"])
    assert nd == nt and sorted(p["diag_info"][:, 1]) == list(range(nt))
    outs = np.concatenate([p["diag_info"][:, 0], p["sub_info"][:, 0]])
    assert sorted(outs) == list(range(p["nslots"])), "a packed slot without exactly one producer"
    for name, n in (("diag", nd), ("sub", ns), ("upd", nu)):
        ptr = p[f"lev_{name}_ptr"]
        assert len(ptr) == p["nlev"] + 1 and ptr[0] == 0 and ptr[-1] == n and np.all(np.diff(ptr) >= 0)
    lev_d = np.repeat(np.arange(p["nlev"]), np.diff(p["lev_diag_ptr"]))
    lev_s = np.repeat(np.arange(p["nlev"]), np.diff(p["lev_sub_ptr"]))
    sub_of_slot = {int(s): t for t, s in enumerate(p["sub_info"][:, 0])}
    diag_of_tile = {int(t): d for d, t in enumerate(p["diag_info"][:, 1])}
    for t in range(ns):   # a SUB item sits in the level of its column's DIAG item, whose slot it names
        d = diag_of_tile[int(p["sub_col"][t])]
        assert lev_s[t] == lev_d[d] and p["sub_info"][t, 1] == p["diag_info"][d, 0]
    for d in range(nd):
        for q in range(p["diag_ptr"][d], p["diag_ptr"][d + 1]):
            slot, tile = (int(v) for v in p["diag_list"][q])
            t = sub_of_slot[slot]
            assert lev_s[t] < lev_d[d] and p["sub_col"][t] == tile and p["slot_tiles"][slot, 0] == p["diag_info"][d, 1]
    for t in range(ns):
        for q in range(p["sub_ptr"][t], p["sub_ptr"][t + 1]):
            a, b = (sub_of_slot[int(v)] for v in p["sub_list"][q])
            assert lev_s[a] < lev_s[t] and lev_s[b] < lev_s[t] and p["sub_col"][a] == p["sub_col"][b]
            assert p["slot_tiles"][p["sub_info"][a, 0], 0] == p["slot_tiles"][p["sub_info"][t, 0], 0]      # L_ik: the item's row
            assert p["slot_tiles"][p["sub_info"][b, 0], 0] == p["sub_col"][t]                              # L_jk: the item's column
    for d in range(nd):   # the backward solve: every tile of the column, once
        rows = [int(p["slot_tiles"][s, 0]) for s, _ in p["back_list"][p["back_ptr"][d]:p["back_ptr"][d + 1]]]
        assert all(p["slot_tiles"][s, 1] == p["back_info"][d, 1] and p["slot_tiles"][s, 0] == i for s, i in p["back_list"][p["back_ptr"][d]:p["back_ptr"][d + 1]])
        assert sorted(rows) == sorted(int(p["slot_tiles"][p["sub_info"][t, 0], 0]) for t in range(ns) if p["sub_col"][t] == p["back_info"][d, 1])
        assert p["back_info"][d, 0] == p["diag_info"][d, 0] and p["back_info"][d, 1] == p["diag_info"][d, 1]
    # chunking: each item's contributor range = its UPDATE items' ranges, in order, then its own share
    assert sorted(p["upd"][:, 3]) == list(range(p["nparts"])) and nu == p["nparts"]
    upd_of_part = {int(u[3]): i for i, u in enumerate(p["upd"])}
    seen = 0
    for kind, info, ptr, own in ((0, p["diag_info"], p["diag_ptr"], p["diag_own"]), (1, p["sub_info"], p["sub_ptr"], p["sub_own"])):
        for b in range(len(info)):
            at = int(ptr[b])
            for part in range(info[b, 2], info[b, 2] + info[b, 3]):
                u = p["upd"][upd_of_part[part]]
                assert u[0] == kind and u[1] == at and u[2] > u[1], "UPDATE items do not tile the contributor list"
                at = int(u[2]); seen += 1
            assert at == own[b] <= ptr[b + 1]
    assert seen == nu, "an UPDATE item that belongs to no item"
    for d in range(nd):
        fs = int(p["diag_fuse"][d])
        if fs >= 0:   # the fused contributor is the last one, it is in the owner's share, and its SUB item publishes for this DIAG item
            last = p["diag_ptr"][d + 1] - 1
            assert p["sub_pub"][fs] == d and p["diag_list"][last, 0] == p["sub_info"][fs, 0] and p["diag_own"][d] <= last
    for t in range(ns):
        if p["sub_pub"][t] >= 0:
            assert p["diag_fuse"][p["sub_pub"][t]] == t


# ---- the ticket orders, replayed ----

class Cells:
    def __init__(self):
        self.written = set()

    def read(self, *cell):
        assert cell in self.written, f"reads {cell} before anybody wrote it"

    def write(self, *cell):
        assert cell not in self.written, f"{cell} written twice"
        self.written.add(cell)


def replay(p, cells, tasks, launch, two_rhs):
    """launch: "all" (the replicated plan), "a" / "b" (the two launches of a sharded plan: plan_a / plan_b of solver.hpp, filled by solver_plan.hip)."""
    diag_info = p["diag_info_sh"] if launch == "b" else p["diag_info"]
    sub_info = p["sub_info_sh"] if launch == "b" else p["sub_info"]
    fwd = {"all": p["fwd_full"], "a": p["fwd_a"], "b": p["fwd_b"]}[launch]
    eta_tiles = {"all": None, "a": p["row_check"], "b": p["row_sep"]}[launch]
    ran = set()
    for kind, item in tasks:
        kind, item = int(kind), int(item)
        assert (kind, item) not in ran, f"task {(kind, item)} twice"
        ran.add((kind, item))
        if kind == UPDATE:
            k, c0, c1, part = (int(v) for v in p["upd"][item])
            for q in range(c0, c1):
                if k == 0:
                    cells.read("L", int(p["diag_list"][q, 0])); cells.read("z", int(p["diag_list"][q, 1]))
                else:
                    cells.read("L", int(p["sub_list"][q, 0])); cells.read("L", int(p["sub_list"][q, 1]))
            cells.write("P", part)
        elif kind == DIAG:
            slot, tile, part0, n = (int(v) for v in diag_info[item])
            fs = int(p["diag_fuse"][item])
            for part in range(part0, part0 + n):
                cells.read("P", part)
            for q in range(p["diag_own"][item], p["diag_ptr"][item + 1] - (fs >= 0)):
                cells.read("L", int(p["diag_list"][q, 0])); cells.read("z", int(p["diag_list"][q, 1]))
            if fs >= 0:
                cells.read("X", item); cells.read("W", int(p["sub_col"][fs])); cells.read("z", int(p["sub_col"][fs]))
            cells.write("L", slot); cells.write("W", tile); cells.write("z", tile)
        elif kind == SUB:
            slot, _, part0, n = (int(v) for v in sub_info[item])
            for part in range(part0, part0 + n):
                cells.read("P", part)
            for q in range(p["sub_own"][item], p["sub_ptr"][item + 1]):
                cells.read("L", int(p["sub_list"][q, 0])); cells.read("L", int(p["sub_list"][q, 1]))
            if p["sub_pub"][item] >= 0:
                cells.write("X", int(p["sub_pub"][item]))   # (before the task waits for W)
            cells.read("W", int(p["sub_col"][item]))
            cells.write("L", slot)
        elif kind == BACK:
            tile = int(p["back_info"][item, 1])
            for q in range(p["back_ptr"][item], p["back_ptr"][item + 1]):
                cells.read("L", int(p["back_list"][q, 0])); cells.read("y", int(p["back_list"][q, 1]))
            cells.read("W", tile); cells.read("z", tile)
            if two_rhs:
                cells.read("eta"); cells.read("z2", tile)
            cells.write("y", tile)
        elif kind in (FWD2, FWD2P):
            assert two_rhs
            tile = int(p["diag_info"][item, 1])
            for q in range(fwd[item, 0], fwd[item, 1]):
                assert p["diag_ptr"][item] <= q < p["diag_ptr"][item + 1]
                cells.read("L", int(p["diag_list"][q, 0])); cells.read("z2", int(p["diag_list"][q, 1]))
            if kind == FWD2P:
                assert launch == "a" and p["diag_toprow"][item] >= 0
                cells.write("z2 share", int(p["diag_toprow"][item]))
            else:
                cells.read("W", tile); cells.write("z2", tile)
        else:
            assert kind == ETA and two_rhs
            for t in range(len(p["row_mine"])):
                if eta_tiles is None or eta_tiles[t]:
                    cells.read("z", t); cells.read("z2", t)
            cells.write("dots share" if launch == "a" else "eta")
    return ran


def check_replicated(p, nt, two_rhs):
    cells = Cells()
    ran = replay(p, cells, p["tasks"], "all", two_rhs)
    want = {(UPDATE, u) for u in range(len(p["upd"]))} | {(k, d) for d in range(nt) for k in ((DIAG, BACK, FWD2) if two_rhs else (DIAG, BACK))} | \
           {(SUB, t) for t in range(len(p["sub_info"]))} | ({(ETA, 0)} if two_rhs else set())
    assert ran == want
    assert [int(k) for k, _ in p["tasks"][-nt:]] == [BACK] * nt   # (launch_chol_solve takes the BACK tasks from the end of the list)
    assert all(("y", t) in cells.written for t in range(nt))


def check_sharded(plans, nt, world, two_rhs):
    p0 = plans[0]
    sep = p0["row_sep"].astype(bool)
    top_order = [int(t) for t in p0["top_tiles"]]
    assert sorted(top_order) == sorted(np.flatnonzero(sep)) and np.array_equal(sep[p0["perm"]], p0["cpart"] < 0)
    owner = p0["upd_owner"]
    item_is_sep = {(DIAG, d): bool(sep[p0["diag_info"][d, 1]]) for d in range(nt)}
    item_is_sep.update({(SUB, t): bool(sep[p0["sub_col"][t]]) for t in range(len(p0["sub_info"]))})
    mine_total = np.zeros(nt, dtype=int)
    in_a = [set(map(tuple, p["tasks_a"].tolist())) for p in plans]
    in_b = [set(map(tuple, p["tasks_b"].tolist())) for p in plans]
    for r, p in enumerate(plans):
        for k in ("upd", "upd_owner", "diag_info", "diag_list", "sub_info", "sub_list", "diag_info_sh", "sub_info_sh", "tasks", "top_slots", "top_info", "row_sep", "diag_toprow"):
            assert np.array_equal(p[k], p0[k]), f"rank {r} plans another {k}"
        mine_total += p["row_mine"]
        part = p["perm"][p["cpart"] == r]
        assert np.array_equal(np.flatnonzero(p["row_check"]), np.sort(part))
        assert np.array_equal(p["row_mine"].astype(bool), p["row_check"].astype(bool) | (sep if r == 0 else False))
        # launch A, the exchange, launch B
        cells = Cells()
        replay(p, cells, p["tasks_a"], "a", two_rhs)
        for part_tile in p["asm_list"]:
            cells.read("P", int(part_tile))
        if two_rhs:
            for row in range(len(top_order)):
                cells.read("z2 share", row)
            cells.read("dots share")
        replay(p, cells, p["tasks_b"], "b", two_rhs)
        assert all(("y", int(t)) in cells.written for t in np.flatnonzero(p["row_mine"]))
        # asm_ptr / asm_list: this rank's partial tiles of the separators' items, tile by tile
        info_of_slot = {int(i[0]): i for i in np.concatenate([p["diag_info"], p["sub_info"]])}
        upd_of_part = {int(u[3]): i for i, u in enumerate(p["upd"])}
        assert len(p["asm_ptr"]) == len(p["top_slots"]) + 1 and p["asm_ptr"][0] == 0 and p["asm_ptr"][-1] == len(p["asm_list"])
        for x, slot in enumerate(p["top_slots"]):
            i = info_of_slot[int(slot)]
            want = [part for part in range(i[2], i[2] + i[3]) if owner[upd_of_part[part]] == r]
            assert list(p["asm_list"][p["asm_ptr"][x]:p["asm_ptr"][x + 1]]) == want
            assert sep[p["slot_tiles"][slot, 0]] and sep[p["slot_tiles"][slot, 1]]
        assert sorted(p["top_slots"]) == sorted(s for s in range(p["nslots"]) if sep[p["slot_tiles"][s, 1]])
        assert list(p["top_fill"]) == [int(s) for s, i in zip(p["top_slots"], p["top_info"]) if not i[0]]
        for x, slot in enumerate(p["top_slots"]):   # the diagonal tile of a separator column carries its row of the right-hand side
            r0, c0 = p["slot_tiles"][slot]
            assert p["top_info"][x, 1] == (top_order.index(int(r0)) if r0 == c0 else -1)
        # what is left to subtract in launch B: the tail of every item's partial tiles, the ones every rank forms
        for info, sh in ((p["diag_info"], p["diag_info_sh"]), (p["sub_info"], p["sub_info_sh"])):
            for i, s in zip(info, sh):
                assert i[0] == s[0] and i[1] == s[1]
                parts_all = list(range(i[2], i[2] + i[3]))
                assert list(range(s[2], s[2] + s[3])) == [q for q in parts_all if owner[upd_of_part[q]] < 0] or not sep[p["slot_tiles"][i[0], 1]]
    assert np.all(mine_total == 1), "a tile's rows of the step come from no rank, or from two"
    for u in range(len(owner)):
        where_a = [r for r in range(world) if (UPDATE, u) in in_a[r]]
        where_b = [r for r in range(world) if (UPDATE, u) in in_b[r]]
        assert (where_a, where_b) == (([int(owner[u])], []) if owner[u] >= 0 else ([], list(range(world))))
    for item, is_sep in item_is_sep.items():
        where_a = [r for r in range(world) if item in in_a[r]]
        where_b = [r for r in range(world) if item in in_b[r]]
        if is_sep:
            assert where_a == [] and where_b == list(range(world))
        else:
            assert len(where_a) == 1 and where_b == []


def check_graph(lib, monkeypatch, nt, edges):
    for leaf in LEAVES:
        if leaf is None:
            monkeypatch.delenv("RSBA_CHOL_LEAF", raising=False)
        else:
            monkeypatch.setenv("RSBA_CHOL_LEAF", leaf)
        for world in WORLDS:
            for two_rhs in (0, 1):
                for opt in (OPTIONS if leaf is None else OPTIONS[:1]):
                    plans = [plan(lib, nt, edges, world, r, two_rhs, opt) for r in range(world)]
                    try:
                        check_items(plans[0], nt)
                        check_replicated(plans[0], nt, two_rhs)
                        if plans[0]["sharded"]:
                            check_sharded(plans, nt, world, two_rhs)
                        else:   # (world == 1, or the dissection could not cut the graph into that many parts: a replicated plan)
                            assert all(len(p["tasks_a"]) == 0 and len(p["tasks_b"]) == 0 and np.array_equal(p["tasks"], plans[0]["tasks"]) for p in plans)
                    except AssertionError as e:
                        raise AssertionError(f"leaf {leaf}, world {world}, two_rhs {two_rhs}, chunk/tail/fuse {opt}: {e}") from e
    return plans


# ---- the graphs ----

def chain(n):
    return n, [(i, i + 1) for i in range(n - 1)]


def grid(a, b):
    return a * b, [(i * b + j, i * b + j + 1) for i in range(a) for j in range(b - 1)] + [(i * b + j, (i + 1) * b + j) for i in range(a - 1) for j in range(b)]


def star(n, band=2):
    """A band with one row that is adjacent to everything: the dense border of a shared intrinsics block."""
    return n, [(i, j) for i in range(n - 1) for j in range(i + 1, min(i + 1 + band, n - 1))] + [(i, n - 1) for i in range(n - 1)]


def random_sparse(seed):
    """nt from 1 to ~200: a band of random width (a video's co-visibility) with a few random far pairs (loop closures); some seeds in several pieces."""
    rng = np.random.default_rng(1000 + seed)
    nt = int(rng.integers(1, 201)) if seed >= 4 else seed + 1
    band = int(rng.integers(1, 5))
    edges = [(i, j) for i in range(nt) for j in range(i + 1, min(i + 1 + band, nt)) if rng.random() < 0.8]
    edges += [tuple(sorted(rng.choice(nt, size=2, replace=False))) for _ in range(int(rng.integers(0, 4))) if nt > 2]
    if seed % 5 == 0 and nt > 10:   # cut the band in two
        c = nt // 2
        edges = [(a, b) for a, b in edges if not (a < c <= b)]
    return nt, [(int(a), int(b)) for a, b in edges]


def scene_graph(prob):
    """The tile graph of a problem: two tiles are adjacent when a point is seen in both (pseudo frames' tiles included)."""
    real, pseudo, nt = observation_tiles(prob)
    tiles = np.concatenate([real[:, None], pseudo], axis=1)
    pairs = set()
    order = np.argsort(prob.obs_point, kind="stable")
    pts, start = np.unique(prob.obs_point[order], return_index=True)
    for a, b in zip(start, list(start[1:]) + [len(order)]):
        ts = np.unique(tiles[order[a:b]])
        pairs.update((int(x), int(y)) for i, x in enumerate(ts) for y in ts[i + 1:])
    return nt, sorted(pairs)


def scene(name):
    import lm_step_cases as LC
    from dist_worker import nd_problem
    if name.startswith("nd:"):
        cfg, *flags = name[3:].split(":")
        return nd_problem(cfg, flags)
    return LC.case(name)[0]


GRAPHS = {f"chain{n}": chain(n) for n in (1, 2, 3, 9, 40, 150)}
GRAPHS.update({f"grid{a}x{b}": grid(a, b) for a, b in ((3, 3), (6, 7), (10, 14))})
GRAPHS.update({f"star{n}": star(n) for n in (9, 30, 120)})
GRAPHS.update({f"random{s}": random_sparse(s) for s in range(36)})
SCENES = ["rs_far_pair", "gs_intr_run3", "rs_nt25", "rs_free_huber", "rs_spherical_pp", "rs_F2p1", "nd:S100", "nd:S40:perframe", "nd:S60:intr", "nd:C2"]


@pytest.mark.parametrize("name", list(GRAPHS))
def test_task_graph_of_a_graph(lib, monkeypatch, name):
    check_graph(lib, monkeypatch, *GRAPHS[name])


@pytest.mark.parametrize("name", SCENES)
def test_task_graph_of_a_scene(lib, monkeypatch, name):
    check_graph(lib, monkeypatch, *scene_graph(scene(name)))


def test_the_cut_graphs_are_sharded_and_the_short_ones_are_not(lib, monkeypatch):
    """The cases above cover both forms: a long chain is cut for 2 and 4 ranks, a graph too short to cut falls back on the replicated plan."""
    monkeypatch.delenv("RSBA_CHOL_LEAF", raising=False)
    for world in (2, 4):
        assert plan(lib, *chain(150), world, 0, 1, OPTIONS[0])["sharded"] == 1
        assert plan(lib, *grid(10, 14), world, 0, 1, OPTIONS[0])["sharded"] == 1
        assert plan(lib, *chain(2), world, 0, 1, OPTIONS[0])["sharded"] == 0
