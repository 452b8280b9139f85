"""Descriptor matching on the device (rsba_match_descriptors, include/rsba/match_frames.hpp) against the Python restatement of
VideoSfMClient::Match (tests/match_reference.py).

Integer-valued descriptors in [0, 255] — what OpenCV's SIFT emits: indices, counts and distances BIT-EQUAL to the integer
restatement (int64 sums, np.sqrt(np.float32(d2)), ties to the lower index); no exclusions, no tolerance.

General finite float descriptors, u = 2^-24 (the contract of the issue, on 257 x 288 uniform [0, 1) descriptors):
  1. every returned (i, j): |d_dev - d64| <= 130 u d64                  (a direct-form fmaf chain of 128 positive terms, then the root)
  2. every query: the r-th returned squared distance <= the true r-th smallest + 2 max_j B(i, j),
     B(i, j) = 130 u (|q_i|^2 + |t_j|^2 + 2 sum_c |q_ic| |t_jc|)        (the GEMM-form search may confuse near-ties, no more)
  3. a query whose true k + 1 nearest are separated by more than the sum of their B is "decided": its indices equal the fp64
     ranking; at most 10 % of the queries may be undecided (printed; 1.6 % for k = 2 and 5.4 % for k = 5 on these inputs —
     q = default_rng(5).random((257, 128), dtype=float32), t the next (288, 128) — by numpy on the host).
Then whole sessions through examples/match_frames and on into examples/create_tracks."""
import json
import os
import subprocess

import numpy as np
import pytest

import create_tracks_reference as R
import match_reference as M
import thrift_encode as T
from rsba_amd.scene import make_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "match_frames")
TRACKS_EXE = os.path.join(ROOT, "examples", "create_tracks")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    return capi


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as G
    if not (os.path.exists(EXE) and os.path.exists(TRACKS_EXE)):
        G.build()
    return EXE


def int_desc(rng, n, lo=0, hi=256):
    return rng.integers(lo, hi, (n, 128)).astype(np.float32)


def assert_bit_equal(got, want, what=""):
    gi, gd, gc = got
    wi, wd, wc = want
    assert np.array_equal(gc, wc), what
    bad = np.argwhere(gi != wi)
    assert len(bad) == 0, (what, bad[:5], gi[bad[0][0]], wi[bad[0][0]], gd[bad[0][0]], wd[bad[0][0]])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


# ---- the neighbour search against the integer restatement ----

@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("shape", [(1, 2), (2, 1), (5, 3), (31, 33), (33, 31), (64, 64), (129, 257), (257, 129), (1100, 900)])
def test_knn_is_bit_equal_to_the_integer_restatement(capi, shape, k):
    nq, nt = shape
    rng = np.random.default_rng(1000 * nq + nt)
    # asymmetric data: queries and train rows from different ranges, and some queries near a train row so that the nearest
    # neighbours are not all alike
    q = int_desc(rng, nq, 0, 200); t = int_desc(rng, nt, 40, 256)
    for i in range(0, nq, 3):
        q[i] = np.clip(t[rng.integers(0, nt)] + rng.integers(-3, 4, 128), 0, 255)
    got = capi.match_descriptors([q, t], [(0, 1)], k=k)[0]
    assert got[0].shape == (nq, k)
    assert_bit_equal(got, M.knn_int(q, t, k), shape)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_every_k(capi, k):
    rng = np.random.default_rng(k)
    q = int_desc(rng, 70); t = int_desc(rng, 150)
    assert_bit_equal(capi.match_descriptors([q, t], [(0, 1)], k=k)[0], M.knn_int(q, t, k) if k > 1 else knn1(q, t))


def knn1(q, t):
    i, d, c = M.knn_int(q, t, 2)
    return i[:, :1], d[:, :1], np.minimum(c, 1)


@pytest.mark.parametrize("k", [2, 5])
def test_edge_data(capi, k):
    rng = np.random.default_rng(11)
    # ties: 50 train rows duplicated (at higher indices, in other tiles and other lane halves), queries next to them
    t = int_desc(rng, 333)
    dup = rng.choice(283, 50, replace=False)
    t[283:] = t[dup]
    q = np.concatenate([t[dup[:20]], np.clip(t[dup[20:40]] + rng.integers(-1, 2, (20, 128)), 0, 255), int_desc(rng, 30)]).astype(np.float32)
    assert_bit_equal(capi.match_descriptors([q, t], [(0, 1)], k=k)[0], M.knn_int(q, t, k), "ties")
    # all-zero and near-zero queries, n_train no multiple of any tile: a zero row that pads the last tile would win
    t = int_desc(rng, 131, 1, 256)
    q = np.zeros((37, 128), dtype=np.float32); q[1::2] = rng.integers(0, 2, (18, 128))
    got = capi.match_descriptors([q, t], [(0, 1)], k=k)[0]
    assert got[0].max() < 131 and got[0].min() >= 0
    assert_bit_equal(got, M.knn_int(q, t, k), "zero queries")
    # the top of the exact range: d2 = 128 * 255^2 = 8 323 200
    q = np.full((3, 128), 255, dtype=np.float32); t = np.zeros((7, 128), dtype=np.float32)
    got = capi.match_descriptors([q, t], [(0, 1)], k=k)[0]
    assert got[1][0, 0] == np.sqrt(np.float32(8323200)) and got[0][0].tolist() == list(range(k))
    assert_bit_equal(got, M.knn_int(q, t, k), "255 against 0")
    assert_bit_equal(capi.match_descriptors([t, q], [(0, 1)], k=k)[0], M.knn_int(t, q, k), "0 against 255")
    # two squared distances one apart that share a rounded root, the larger at the lower index and in the other lane half:
    # the order is by the root, then the index
    q, two = M.shared_root_rows()
    t = np.full((5, 128), 255, dtype=np.float32); t[0] = two[0]; t[4] = two[1]
    got = capi.match_descriptors([q, t], [(0, 1)], k=k)[0]
    assert got[0][0].tolist() == [0, 4, 1, 2, 3][:k]
    assert_bit_equal(got, M.knn_int(q, t, k), "shared root")


# ---- several train tiles per workgroup ----
# The host splits a pair's 128-row train tiles over min(16, ceil(1024 / query blocks)) workgroups.  With a handful of query
# blocks and fewer than 17 tiles every workgroup gets ONE tile; the shapes below give each workgroup 2 .. 6 consecutive tiles, so
# that the tile loop, the barrier that guards the LDS tile against the next fill and the top-K carried from tile to tile are run.

def tiles_per_workgroup(pair_shapes):
    """the host's split rule (match_capi.hip), restated: -> tiles per workgroup of each pair"""
    blocks = sum((nq + 127) // 128 for nq, nt in pair_shapes if nt >= 2)
    split = min(16, max(1, -(-1024 // blocks)))
    return [-(-((nt + 127) // 128) // split) for nq, nt in pair_shapes]


@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("shape", [(300, 2500), (129, 4200), (40, 12000)])
def test_knn_over_several_train_tiles_per_workgroup(capi, shape, k):
    nq, nt = shape
    assert tiles_per_workgroup([shape])[0] == {2500: 2, 4200: 3, 12000: 6}[nt]
    rng = np.random.default_rng(7 * nq + nt)
    q = int_desc(rng, nq, 0, 200); t = int_desc(rng, nt, 40, 256)
    for i in range(0, nq, 2):                                          # a near neighbour somewhere in the train set ...
        q[i] = np.clip(t[rng.integers(0, nt)] + rng.integers(-3, 4, 128), 0, 255)
    # ... and ties that span tiles of ONE workgroup: a row repeated 128 (the next tile, same lane) and 133 rows (the next
    # tile, other lane half) further on, the queries next to those rows
    per = tiles_per_workgroup([shape])[0]
    for n, i in enumerate(range(1, nq, 4)):
        j = 128 * per * (n % 3) + (5 * n) % 100                        # in the first tile of a workgroup
        t[j + 128] = t[j]; t[j + 133] = t[j]
        q[i] = np.clip(t[j] + (n % 2) * rng.integers(-1, 2, 128), 0, 255)
    want = M.knn_int(q, t, k)
    assert np.mean(want[1][:, 0] == want[1][:, 1]) > 0.15               # the ties are there
    assert_bit_equal(capi.match_descriptors([q, t], [(0, 1)], k=k)[0], want, shape)


@pytest.mark.parametrize("k", [2, 5])
def test_many_query_blocks_so_that_the_split_falls_below_the_tile_count(capi, k):
    rng = np.random.default_rng(31)
    sizes = (1400, 2100, 1300, 2200)
    frames = [int_desc(rng, n, 0, 200) if f % 2 == 0 else int_desc(rng, n, 40, 256) for f, n in enumerate(sizes)]
    for f in (0, 2):
        for i in range(0, sizes[f], 3):
            g = 1 + 2 * rng.integers(0, 2)
            frames[f][i] = np.clip(frames[g][rng.integers(0, sizes[g])] + rng.integers(-3, 4, 128), 0, 255)
    frames[1][700:900] = frames[1][500:700]                             # ties across tiles
    pairs = [(0, 1), (0, 3), (2, 1), (2, 3), (1, 3), (3, 1), (0, 2), (1, 0)]
    per = tiles_per_workgroup([(sizes[a], sizes[b]) for a, b in pairs])
    assert min(per) >= 2, per                                           # every workgroup of every pair loops over tiles
    got = capi.match_descriptors(frames, pairs, k=k)
    for (fq, ft), g in zip(pairs, got):
        assert_bit_equal(g, M.knn_int(frames[fq], frames[ft], k), (fq, ft))


@pytest.mark.parametrize("k", [2, 5])
def test_several_pairs_in_one_call_equal_one_call_each(capi, k):
    rng = np.random.default_rng(21)
    frames = [int_desc(rng, n) for n in (140, 0, 260, 1, 35, 2)]
    pairs = [(0, 2), (2, 0), (2, 4), (4, 2), (0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (2, 2), (4, 0)]   # frame 2: query and train, and against itself
    got = capi.match_descriptors(frames, pairs, k=k)
    assert len(got) == len(pairs)
    for (fq, ft), g in zip(pairs, got):
        one = capi.match_descriptors([frames[fq], frames[ft]], [(0, 1)], k=k)[0]
        assert_bit_equal(g, one, (fq, ft))
        assert_bit_equal(g, M.knn_int(frames[fq], frames[ft], k), (fq, ft))
        assert g[0].shape == (len(frames[fq]), k)
    assert got[6][2].tolist() == [0] * 260 and np.all(got[6][0] == -1) and np.all(np.isinf(got[6][1]))   # one train row: nothing


def test_bad_arguments_are_refused_with_a_message(capi):
    d = np.zeros((4, 64), dtype=np.float32)
    with pytest.raises(capi.RsbaError, match="128"):
        capi.match_descriptors([d, d], [(0, 1)], k=2)
    d = np.zeros((4, 128), dtype=np.float32)
    for k in (0, 6, -1):
        with pytest.raises(capi.RsbaError, match=r"\[1, 5\]"):
            capi.match_descriptors([d, d], [(0, 1)], k=k)
    with pytest.raises(capi.RsbaError, match="frame"):
        capi.match_descriptors([d, d], [(0, 2)], k=2)


# ---- general float descriptors ----

@pytest.fixture(scope="module")
def float_case():
    rng = np.random.default_rng(5)
    q = rng.random((257, 128), dtype=np.float32); t = rng.random((288, 128), dtype=np.float32)
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    d2 = M.d2_f64(q, t)
    B = 130 * U * ((q64 ** 2).sum(1)[:, None] + (t64 ** 2).sum(1)[None, :] + 2 * np.abs(q64) @ np.abs(t64).T)
    return q, t, d2, B


@pytest.mark.parametrize("k", [2, 5])
def test_general_float_descriptors_within_the_contract(capi, float_case, k):
    q, t, d2, B = float_case
    idx, dist, cnt = capi.match_descriptors([q, t], [(0, 1)], k=k)[0]
    assert np.all(cnt == k) and idx.min() >= 0 and idx.max() < len(t)
    assert all(len(set(r)) == k for r in idx.tolist())
    # 1. the reported distances: every query
    true_d = np.sqrt(np.take_along_axis(d2, idx.astype(np.int64), 1))
    err = np.abs(dist.astype(np.float64) - true_d) / true_d
    print(f"k={k}: max relative distance error {err.max() / U:.2f} u (bound 130 u)")
    assert np.all(err <= 130 * U)
    assert np.all(np.diff(dist, axis=1) >= 0)
    # 2. never a clearly worse neighbour: every query
    order = np.argsort(d2, axis=1, kind="stable")
    srt = np.take_along_axis(d2, order, 1)
    slack = 2 * B.max(1)
    got_d2 = np.sort(np.take_along_axis(d2, idx.astype(np.int64), 1), axis=1)
    excess = (got_d2 - srt[:, :k]) / slack[:, None]
    print(f"k={k}: largest excess of a returned squared distance over the true r-th smallest: {excess.max():.3g} of the allowed 2 max B")
    assert np.all(got_d2 <= srt[:, :k] + slack[:, None])
    # 3. decided queries: the fp64 ranking
    Bs = np.take_along_axis(B, order[:, :k + 1], 1)
    decided = np.all(np.diff(srt[:, :k + 1], axis=1) > Bs[:, :-1] + Bs[:, 1:], axis=1)
    share = 1.0 - decided.mean()
    print(f"k={k}: undecided share {100 * share:.1f} % ({int((~decided).sum())} of {len(q)} queries)")
    assert share <= 0.10
    assert np.array_equal(idx[decided], order[decided, :k])


# ---- whole sessions ----

def descriptor_session(seed=3, F=6, P=300):
    """6 frames x ~300 observations: positions are make_scene's projections rounded to float, a descriptor is its 3-D point's
    random integer vector plus per-observation integer noise; ~15 % of the observations carry an unrelated descriptor and a
    tenth of the points share their vector with another point (ambiguous: the ratio test has something to reject)."""
    sc = make_scene(F, P, rolling=True, seed=seed, noise_px=0.3)
    p = sc.problem
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (P, 128))
    twins = rng.choice(P, P // 10, replace=False)
    base[twins] = base[(twins + 1) % P]
    frames = [R.Frame(obs=[], poses=[list(q) for q in p.poses[f]]) for f in range(F)]
    descs = [[] for _ in range(F)]
    for i in np.argsort(p.obs_frame, kind="stable"):
        f, j = int(p.obs_frame[i]), int(p.obs_point[i])
        d = rng.integers(0, 256, 128) if rng.random() < 0.15 else np.clip(base[j] + rng.integers(-6, 7, 128), 0, 255)
        frames[f].obs.append(R.Obs(float(np.float32(p.obs_xy[i, 0])), float(np.float32(p.obs_xy[i, 1]))))
        descs[f].append(d.astype(np.float32))
    descs = [np.stack(d) for d in descs]
    sess = R.Session(cam=list(p.intrinsics[0]), frames=frames, tracks=[], rs=int(p.shutter), scanlines=list(p.scanlines))
    return sess, descs


def cache_with_descriptors(sess, descs):
    frames = [T.frame([T.observation(o.x, o.y, descriptor=d.astype("<f4").tobytes()) for o, d in zip(fr.obs, ds)], poses=fr.poses)
              for fr, ds in zip(sess.frames, descs)]
    return T.file_events(T.session(sess.cam, frames, [], sess.rs, list(sess.scanlines), 1280, 720), np.random.default_rng(1), max_event=4096)


@pytest.fixture(scope="module")
def session_case():
    sess, descs = descriptor_session()
    xys = [[[o.x, o.y] for o in fr.obs] for fr in sess.frames]
    want = {m: M.match_session(descs, xys, 5, m) for m in (False, True)}
    return sess, descs, want


def run_match(exe, tmp_path, sess, descs, *flags, out=None):
    (tmp_path / "s.cache").write_bytes(cache_with_descriptors(sess, descs))
    r = subprocess.run([exe, "match", str(tmp_path / "s.cache"), *flags, *([str(out)] if out else [])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)["frames"]


@pytest.mark.parametrize("multiple", [False, True])
def test_match_frames_equals_the_restatement(exe, tmp_path, session_case, multiple):
    sess, descs, want = session_case
    assert all(250 <= len(d) <= 300 for d in descs)
    n = sum(len(m) for fr in want[multiple] for m in fr)
    unmatched = sum(not m for fr in want[multiple][1:] for m in fr)
    assert n > 2000 and (multiple or unmatched > 30)                                    # most observations find their point, the outliers nothing
    flags = ["--multiple"] if multiple else []
    batch = run_match(exe, tmp_path, sess, descs, *flags)
    assert batch == want[multiple]
    assert run_match(exe, tmp_path, sess, descs, *flags, "--per-frame") == batch


def test_a_missing_descriptor_throws(exe, tmp_path, session_case):
    sess, descs, _ = session_case
    frames = [T.frame([T.observation(o.x, o.y, descriptor=d.astype("<f4").tobytes() if (f, i) != (1, 7) else None)
                       for i, (o, d) in enumerate(zip(fr.obs, ds))], poses=fr.poses) for f, (fr, ds) in enumerate(zip(sess.frames, descs))]
    (tmp_path / "m.cache").write_bytes(T.file_events(T.session(sess.cam, frames, [], sess.rs, list(sess.scanlines), 1280, 720)))
    r = subprocess.run([exe, "match", str(tmp_path / "m.cache")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "observation 7 of frame 1" in r.stderr


def test_matched_session_goes_through_create_tracks(exe, oracle, tmp_path, session_case):
    sess, descs, want = session_case
    run_match(exe, tmp_path, sess, descs, out=tmp_path / "matched.cache")
    r = subprocess.run([TRACKS_EXE, "batch", str(tmp_path / "matched.cache"), str(tmp_path / "o.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _, frames, tracks = R.read_state(tmp_path / "o.bin")
    ref = R.clone(sess)
    for fr, ms in zip(ref.frames, want[False]):
        for o, m in zip(fr.obs, ms):
            o.matches = [[a, b, False] for a, b in m] if m else None
    opt = R.Options()
    g = R.OracleGeometry(oracle, opt)
    for f in range(len(ref.frames)):
        R.create_tracks(ref, f, opt, g)
    wf, wt = R.state_of(ref)
    assert len(wt) > 100
    assert frames == wf and len(tracks) == len(wt)
    for (pg, vg, og), (pw, vw, ow) in zip(tracks, wt):
        assert og == ow and vg == vw
        assert np.abs(np.array(pg) - np.array(pw)).max() <= 1e-9 * (1 + np.abs(pw).max()), (pg, pw)
