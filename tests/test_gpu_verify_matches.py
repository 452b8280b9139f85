"""verifyMatches on the device through examples/verify_matches: a session of 5 frames whose observations are matched into the two frames
before them, with seeded wrong refs (verify_pairs_common.SmallSession), written as a session cache by tests/thrift_encode.py.  The refs that
remain are exactly those the masks of findEssentialRansac keep, pair by pair (the existing single-pair path, run by the same example on the
pairs assembled here); the pair under 8 correspondences is untouched, or gone with dropUnverified; pickBootstrapPair names the ok pair with
the most inliers in front; and createTracks runs on the session the example wrote back."""
import os
import struct
import subprocess

import numpy as np
import pytest

import thrift_encode as T
import verify_pairs_common as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exes():
    import __graft_entry__ as G
    paths = [os.path.join(ROOT, "examples", name) for name in ("verify_matches", "create_tracks")]
    if not all(os.path.exists(p) for p in paths):
        G.build()
    return paths


@pytest.fixture(scope="module")
def session():
    return V.SmallSession()


def cache_bytes(s):
    p = s.sc.problem
    frames = [T.frame([T.observation(o["x"], o["y"], track=None, matches=[(fa, oa, True) for fa, oa in o["matches"]] or None) for o in fr], poses=s.true_poses[k], prior_poses=None)
              for k, fr in enumerate(s.frames)]
    return T.file_events(T.session(s.cam, frames, [], int(p.shutter), list(p.scanlines), 1280, 720), np.random.default_rng(1), max_event=4096)


def run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def count_tracks(buf):
    """the layout examples/create_tracks.cpp writes -> (tracks, valid tracks)"""
    pos = 0

    def q():
        nonlocal pos
        v = struct.unpack_from("<q", buf, pos)[0]; pos += 8; return v
    def skip(count, size):
        nonlocal pos
        pos += count * size
    for _ in range(q()):
        skip(q(), 48)
        for _ in range(q()):
            q(); q(); skip(q(), 8)
    total = q(); valid = 0
    for _ in range(total):
        skip(1, 24); valid += q(); skip(q(), 24)
    assert pos == len(buf)
    return total, valid


@pytest.mark.parametrize("solver", ["eight_point", "five_point"])
def test_the_refs_left_are_those_the_single_pair_masks_keep(exes, session, tmp_path, solver):
    verify, create = exes
    o = V.OPTIONS
    (tmp_path / "s.cache").write_bytes(cache_bytes(session))
    found = session.pairs()
    V.write_pairs_file(tmp_path / "pairs.bin", [session.pair_arrays(fa, fb, refs) for (fa, fb), refs in found.items()])
    per_pair = V.parse_results(run(verify, "pairs", tmp_path / "pairs.bin", "sequential", o["iterations"], o["threshold_px"], o["refits"], o["min_inliers"], o["rng_state"], 0, solver), len(found))
    kv = (f"iterations={o['iterations']}", f"threshold={o['threshold_px']}", f"refits={o['refits']}", f"minInliers={o['min_inliers']}", f"seed={o['rng_state']}", f"solver={solver}", "dump=1")
    for drop in (0, 1):
        reports, bootstrap, left, _ = V.parse_session_output(run(verify, tmp_path / "s.cache", tmp_path / f"out{drop}.cache", *kv, f"dropUnverified={drop}"))
        want_left, want_removed = session.expected(per_pair, o["min_inliers"], bool(drop))
        assert [(r["frameA"], r["frameB"]) for r in reports] == list(found) and [r["correspondences"] for r in reports] == [len(v) for v in found.values()]
        assert [r["ok"] for r in reports] == [p["ok"] for p in per_pair]
        assert [r["num_inliers"] for r in reports] == [p["num_inliers"] for p in per_pair] and [r["num_front"] for r in reports] == [p["num_front"] for p in per_pair]
        assert all(np.array_equal(r["E"], p["E"]) and np.array_equal(r["pose"], p["pose"]) for r, p in zip(reports, per_pair))
        assert [r["removed"] for r in reports] == want_removed
        assert left == want_left
        few = reports[3]
        assert (few["frameA"], few["frameB"], few["correspondences"]) == (0, 3, 5) and not few["ok"] and few["removed"] == (5 if drop else 0)
        assert sum(1 for (fb, oi), ms in left.items() if fb == 3 for m in ms if m[0] == 0) == (0 if drop else 5)
        assert all(r["ok"] for k, r in enumerate(reports) if k != 3)
        best = max((k for k, r in enumerate(reports) if r["ok"]), key=lambda k: (reports[k]["num_front"], -reports[k]["frameB"], -reports[k]["frameA"]))
        assert bootstrap == best
        wrong = {(fb, oi, session.frames[fb][oi]["matches"][s]) for fb in range(5) for oi, ob in enumerate(session.frames[fb]) for s in ob["wrong"]}
        left_set = {(fb, oi, m) for (fb, oi), ms in left.items() for m in ms}
        print(f"{solver} drop={drop}: {len(wrong)} seeded wrong refs, {len(wrong & left_set)} left; removed per pair {[r['removed'] for r in reports]}; bootstrap pair {bootstrap}")
        assert len(wrong & left_set) <= 0.25 * len(wrong)      # (test_verify_pairs_host.py on why "most")
    # createTracks on the verified session, from the cache the example wrote back (every frame has its true pose)
    run(create, "batch", tmp_path / "out0.cache", tmp_path / "tracks.bin", "first=1", "last=4")
    total, valid = count_tracks((tmp_path / "tracks.bin").read_bytes())
    print(f"{solver}: createTracks on the verified session: {total} tracks, {valid} valid")
    assert total > 0
