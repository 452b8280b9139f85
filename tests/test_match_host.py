"""Descriptor matching, the parts that need no GPU: hand-computed known answers for the Python restatement of
VideoSfMClient::Match (tests/match_reference.py), the host filter of include/rsba/match_frames.hpp (examples/match_frames filter)
against that restatement, the C ABI's refusal without a device, and the cache loader's opt-in descriptor field."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import match_reference as M
import thrift_encode as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "match_frames")
TOOL = os.path.join(ROOT, "examples", "session_cache_tool")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as G
    if not (os.path.exists(EXE) and os.path.exists(TOOL)):
        G.build()
    return EXE


def one_hot(values):
    """descriptors whose first component is the given value, the rest 0: distances are |differences|"""
    d = np.zeros((len(values), 128), dtype=np.float32)
    d[:, 0] = values
    return d


# ---- known answers for the restatement ----

def test_ratio_test_rejects_4_against_5_in_float():
    assert np.float32(0.8) * np.float32(5.0) == np.float32(4.0)          # the float product rounds to 4: 4 < 4 is false
    assert 0.8 * 5.0 == 4.0 and float(np.float32(0.8)) * 5.0 > 4.0       # (the float constant widened to double would accept)
    q = one_hot([0]); xy_q = [[10.0, 10.0]]; xy_t = [[11.0, 10.0], [50.0, 50.0]]
    idx, dist, cnt = M.knn_int(q, one_hot([4, 5]), 2)
    assert idx.tolist() == [[0, 1]] and dist.tolist() == [[4.0, 5.0]] and cnt.tolist() == [2]
    assert M.match(q, one_hot([4, 5]), xy_q, xy_t) == []
    assert M.match(q, one_hot([4, 6]), xy_q, xy_t) == [(0, 0)]           # 4 < 0.8f * 6
    assert M.match(q, one_hot([5, 4]), xy_q, [[50.0, 50.0], [11.0, 10.0]]) == []   # the same pair the other way round in the train frame


def test_ties_go_to_the_lower_train_index():
    t = one_hot([7, 3, 7, 3, 9])
    idx, dist, cnt = M.knn_int(one_hot([5]), t, 5)
    assert idx.tolist() == [[0, 1, 2, 3, 4]] and dist.tolist() == [[2.0, 2.0, 2.0, 2.0, 4.0]] and cnt.tolist() == [5]
    idx, dist, _ = M.knn_int(one_hot([4]), t, 2)
    assert idx.tolist() == [[1, 3]] and dist.tolist() == [[1.0, 1.0]]
    # two squared distances that share a rounded root: the order is by the ROOT, so the lower index comes first
    q, t2 = M.shared_root_rows()
    d2 = [int((t2[j].astype(np.int64) ** 2).sum()) for j in range(2)]
    assert d2[0] == d2[1] + 1 and d2[0] < 2 ** 24
    idx, dist, _ = M.knn_int(q, t2, 2)
    assert idx.tolist() == [[0, 1]] and dist[0, 0] == dist[0, 1]


def test_the_multiple_quirk_on_a_2_by_5_case():
    q = one_hot([0, 100]); t = one_hot([1, 2, 3, 4, 5])
    xy_q = [[0.0, 0.0], [0.0, 0.0]]
    xy_t = [[1.0, 0.0], [9.0, 0.0], [9.0, 0.0], [2.0, 0.0], [3.0, 0.0]]
    idx, dist, cnt = M.knn_int(q, t, 5)
    assert idx.tolist() == [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]] and dist[1].tolist() == [95.0, 96.0, 97.0, 98.0, 99.0]
    # 2-D: best neighbours at 1 and 3 -> mean 2, threshold 4.
    # query 0: distances 1, 2: 1 > 0.8 * 2 is false -> ms[0] alone (its 2-D distance 1 < 4)
    # query 1: 95 > 0.8 * 96 -> AMBIGUOUS, and that is when the reference keeps the further neighbours: 3 (2-D 2) and 0 (2-D 1),
    #          not 2 and 1 (2-D 9); ms[0] = 4 is kept on its 2-D distance alone, with no ratio test
    assert M.match(q, t, xy_q, xy_t, multiple=True) == [(0, 0), (1, 4), (1, 3), (1, 0)]
    assert M.match(q, t, xy_q, xy_t, multiple=False) == [(0, 0)]


@pytest.mark.parametrize("multiple", [False, True])
def test_fewer_than_two_train_rows_or_no_query_gives_nothing(multiple):
    q = one_hot([0, 3])
    for nt in (0, 1):
        idx, dist, cnt = M.knn_int(q, one_hot([1][:nt]), 5 if multiple else 2)
        assert cnt.tolist() == [0, 0] and np.all(idx == -1) and np.all(np.isinf(dist))
        assert M.match(q, one_hot([1][:nt]), [[0.0, 0.0]] * 2, [[1.0, 1.0]] * nt, multiple) == []
    assert M.match(one_hot([]), one_hot([1, 2, 3]), [], [[1.0, 1.0]] * 3, multiple) == []
    assert M.match_session([one_hot([1, 2]), one_hot([5]), one_hot([1, 9])], [[[0.0, 0.0]] * 2, [[0.0, 0.0]], [[1.0, 0.0]] * 2])[1] == [[]]


def test_calc2ddist_subtracts_in_float():
    """Three queries with clear best neighbours at 2-D distances a = b = 1 and c; the threshold is 2 (a + b + c) / 3, so the third
    is kept iff c < 4 (up to rounding).  x_q = 4 - 1e-9 is 4.0f as a float: c = 4 exactly, the threshold 4, rejected.  In double
    the difference 3.999999999 lies below the threshold 3.9999999993 and the match would be kept."""
    q = one_hot([0, 50, 100]); t = one_hot([1, 51, 101, 200])
    xq = 4.0 - 1e-9
    xy_q = [[1.0, 0.0], [1.0, 0.0], [xq, 0.0]]
    xy_t = [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]
    assert np.float32(xq) == np.float32(4.0) and M.dist2d(xy_q[2], xy_t[2]) == 4.0
    c = xq - 0.0
    thr = (1.0 + 1.0 + c) / 3
    assert c < thr + thr                                                   # double arithmetic keeps it
    assert M.match(q, t, xy_q, xy_t) == [(0, 0), (1, 1)]                   # float subtraction: rejected
    xy_q[2][0] = 3.99
    assert M.match(q, t, xy_q, xy_t) == [(0, 0), (1, 1), (2, 2)]


# ---- the host filter of match_frames.hpp against the restatement ----

def random_knn(rng, nq, nt, k):
    idx = np.stack([rng.choice(nt, k, replace=False) for _ in range(nq)]).astype(np.int32)
    # distances: roots of small integers (so that 0.8f * d1 == d0 and near-ties happen), ascending
    d2 = np.sort(rng.integers(1, 60, (nq, k)), axis=1)
    d2[::7, 0] = 16; d2[::7, 1] = 25                                       # the 4-against-5 case
    dist = np.sqrt(d2.astype(np.float32))
    xy_q = rng.uniform(0, 1000, (nq, 2)); xy_t = rng.uniform(0, 1000, (nt, 2))
    near = rng.random(nq) < 0.7                                            # most best neighbours lie near their query
    xy_t[idx[near, 0]] = xy_q[near] + rng.normal(0, 30, (int(near.sum()), 2))
    return idx, dist, np.full(nq, k, dtype=np.int32), xy_q, xy_t


def run_filter(exe, tmp_path, idx, dist, cnt, xy_q, xy_t, multiple):
    nq, k = idx.shape
    blob = struct.pack("<4q", nq, len(xy_t), k, int(multiple)) + np.asarray(xy_q, dtype="<f8").tobytes() + np.asarray(xy_t, dtype="<f8").tobytes()
    blob += idx.astype("<i4").tobytes() + dist.astype("<f4").tobytes() + cnt.astype("<i4").tobytes()
    (tmp_path / "knn.bin").write_bytes(blob)
    r = subprocess.run([exe, "filter", str(tmp_path / "knn.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return [tuple(m) for m in json.loads(r.stdout)]


@pytest.mark.parametrize("multiple", [False, True])
@pytest.mark.parametrize("nq", [1, 2, 300])
def test_filter_matches_equals_the_restatement(exe, tmp_path, nq, multiple):
    rng = np.random.default_rng(100 + nq + multiple)
    k = 5 if multiple else 2
    idx, dist, cnt, xy_q, xy_t = random_knn(rng, nq, 40 + nq, k)
    want = M.filter_matches(idx, dist, cnt, xy_q, xy_t, multiple)
    got = run_filter(exe, tmp_path, idx, dist, cnt, xy_q, xy_t, multiple)
    assert got == want
    if nq == 300:
        assert 20 < len(want) < (4 * nq if multiple else nq)              # the filter both keeps and rejects
    # the known answers through the C++ filter as well
    i2, d2, c2 = M.knn_int(one_hot([0]), one_hot([4, 5]), 2)
    assert run_filter(exe, tmp_path, i2, d2, c2, [[10.0, 10.0]], [[11.0, 10.0], [50.0, 50.0]], False) == []
    q = one_hot([0, 50, 100]); t = one_hot([1, 51, 101, 200])
    i3, d3, c3 = M.knn_int(q, t, 2)
    assert run_filter(exe, tmp_path, i3, d3, c3, [[1.0, 0.0], [1.0, 0.0], [4.0 - 1e-9, 0.0]], [[0.0, 0.0]] * 4, False) == [(0, 0), (1, 1)]


def test_match_descriptors_without_a_device_is_an_error():
    import torch
    from rsba_amd import capi
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.RsbaError):
        capi.match_descriptors([np.zeros((3, 128), dtype=np.float32), np.ones((4, 128), dtype=np.float32)], [(0, 1)], k=2)


# ---- the cache loader ----

def descriptor_session(rng, with_descriptors):
    frames, want = [], []
    for f in range(3):
        obs, row = [], []
        for i in range(4 + f):
            d = rng.integers(0, 256, 128).astype("<f4").tobytes()
            row.append(d.hex())
            obs.append(T.observation(float(i), float(f), track=None, matches=[(0, 0, False)] if f else None,
                                     descriptor=d if with_descriptors else None, color=b"\x01\x02\x03" if with_descriptors else None))
        frames.append(T.frame(obs, poses=[[0.0] * 6]))
        want.append(row)
    return T.session([800, 800, 0, 0, 0, 0, 0, 640, 360], frames, [], 1, [0, 720], 1280, 720), want


def test_descriptors_survive_a_write_and_a_read_only_when_asked_for(exe, tmp_path):
    with_d, want = descriptor_session(np.random.default_rng(2), True)
    without_d, _ = descriptor_session(np.random.default_rng(2), False)
    (tmp_path / "d.cache").write_bytes(T.file_events(with_d, np.random.default_rng(3), max_event=700))
    (tmp_path / "n.cache").write_bytes(T.file_events(without_d))

    def descriptors(path):
        r = subprocess.run([exe, "descriptors", str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    assert descriptors(tmp_path / "d.cache") == want
    assert subprocess.run([exe, "copy", str(tmp_path / "d.cache"), str(tmp_path / "d2.cache")], capture_output=True).returncode == 0
    assert descriptors(tmp_path / "d2.cache") == want                     # bit for bit through writer and reader
    # the defaults: the tool that loads and saves without the flag drops them, and prints what it prints for a file without
    assert subprocess.run([TOOL, "copy", "session", str(tmp_path / "d.cache"), str(tmp_path / "d3.cache")], capture_output=True).returncode == 0
    assert descriptors(tmp_path / "d3.cache") == [[""] * len(r) for r in want]
    dumps = [subprocess.run([TOOL, "dump", "session", str(tmp_path / n)], capture_output=True) for n in ("d.cache", "n.cache", "d2.cache", "d3.cache")]
    assert all(d.returncode == 0 for d in dumps)
    assert dumps[0].stdout == dumps[1].stdout == dumps[2].stdout == dumps[3].stdout and b"descriptor" not in dumps[0].stdout
