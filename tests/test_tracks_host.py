"""Track creation on the host (include/rsba/create_tracks.hpp), without a GPU: the C++ decision replay (replayCreateTracks,
through examples/create_tracks replay) against the Python restatement (tests/create_tracks_reference.py) on random sessions and
random flag tables, one hand-built session per quirk, the oracle-geometry restatement on the geometric quirks, and the new
entry's failure without a device."""
import os
import subprocess

import numpy as np
import pytest

import create_tracks_reference as R
import thrift_encode as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "create_tracks")
CAM = [500.0, 500.0, 0.0, 0.0, 0.0, 0.0, 0.0, 320.0, 240.0]


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as G
    if not os.path.exists(EXE):
        G.build()
    return EXE


def run_replay(exe, tmp_path, sess, tables, opt, first, last):
    (tmp_path / "s.cache").write_bytes(R.to_cache(sess, T))
    R.write_flags(tmp_path / "f.bin", sess, tables, first, last)
    args = [exe, "replay", str(tmp_path / "s.cache"), str(tmp_path / "o.bin"), f"flags={tmp_path / 'f.bin'}", f"first={first}", f"last={last}",
            f"minReprojections={opt.min_reprojections}", f"maxReprojections={opt.max_reprojections}", f"const3d={int(opt.const3d)}"]
    r = subprocess.run(args, capture_output=True, text=True)
    if r.returncode == 3:
        return "threw"
    assert r.returncode == 0, r.stderr
    _, frames, tracks = R.read_state(tmp_path / "o.bin")
    return frames, tracks


def py_replay(sess, tables, opt, first, last):
    s = R.clone(sess)
    g = R.TableGeometry(s, tables)
    try:
        for f in range(first, last + 1):
            R.create_tracks(s, f, opt, g)
    except R.CreateTracksError:
        return "threw", s
    return R.state_of(s), s


def random_session(rng):
    F = int(rng.integers(2, 6))
    frames = []
    for f in range(F):
        poses = None if rng.random() < 0.1 else [list(rng.normal(size=6)) for _ in range(int(rng.integers(1, 4)))]
        frames.append(R.Frame(obs=[R.Obs(float(rng.uniform(0, 640)), float(rng.uniform(0, 480))) for _ in range(int(rng.integers(0, 6)))], poses=poses))
    all_obs = [(f, k) for f in range(F) for k in range(len(frames[f].obs))]
    # existing tracks: each tracked observation is listed in its track, at most one observation per frame
    tracks = []
    free = list(all_obs)
    rng.shuffle(free)
    while free and rng.random() < 0.7:
        members, used = [], set()
        for fk in list(free):
            if fk[0] not in used and len(members) < int(rng.integers(1, 5)):
                members.append(fk); used.add(fk[0]); free.remove(fk)
        tid = len(tracks)
        tracks.append(R.Track(obs=[[f, k, bool(rng.random() < 0.5)] for f, k in members], pt=list(rng.normal(size=3)), valid=bool(rng.random() < 0.5)))
        for f, k in members:
            frames[f].obs[k].track, frames[f].obs[k].has_track = tid, True
    for f in range(F):
        for o in frames[f].obs:
            if rng.random() < 0.8:
                others = [fk for fk in all_obs if fk[0] != f or rng.random() < 0.03]   # now and then a match inside the frame
                n = int(rng.integers(0, 4))
                o.matches = [[int(a), int(b), bool(rng.random() < 0.2)] for a, b in (others[i] for i in rng.integers(0, len(others), n))] if others else []
    return R.Session(cam=CAM, frames=frames, tracks=tracks, rs=int(rng.integers(0, 3)), scanlines=[0, 480])


def random_tables(rng, sess):
    tables = {}
    for f, fr in enumerate(sess.frames):
        n = R.ref_offsets(fr)[-1]
        tables[f] = (rng.integers(0, 2, n), rng.integers(0, 2, n), rng.normal(size=(n, 3)))
    return tables


def test_cpp_replay_equals_python_replay_on_random_sessions(exe, tmp_path):
    rng = np.random.default_rng(20261016)
    outcomes = {"threw": 0, "created": 0, "joined": 0}
    for case in range(2000):
        sess = random_session(rng)
        tables = random_tables(rng, sess)
        opt = R.Options(min_reprojections=int(rng.integers(1, 4)), max_reprojections=int(rng.choice([0, 2, 3, 10])), const3d=bool(rng.random() < 0.15))
        F = len(sess.frames)
        first = int(rng.integers(0, F)); last = int(rng.integers(first, F))
        want, s = py_replay(sess, tables, opt, first, last)
        got = run_replay(exe, tmp_path, sess, tables, opt, first, last)
        assert got == want, (case, first, last, opt)
        if want == "threw":
            outcomes["threw"] += 1
        else:
            outcomes["created"] += len(s.tracks) > len(sess.tracks)
            outcomes["joined"] += sum(len(t.obs) for t in s.tracks[:len(sess.tracks)]) > sum(len(t.obs) for t in sess.tracks)
    assert min(outcomes.values()) > 50, outcomes


# ---- one hand-built session per quirk (flag tables: tri, reproj, pt per match of each observation) ----

def two_frame_session():
    """frame 0: o0 with matches; frames 1, 2: candidate partners"""
    frames = [R.Frame(obs=[R.Obs(10, 10)], poses=[[0.0] * 6]), R.Frame(obs=[R.Obs(11, 11), R.Obs(12, 12)], poses=[[0, 0, 0, 1, 0, 0]]),
              R.Frame(obs=[R.Obs(13, 13)], poses=[[0, 0, 0, 2, 0, 0]])]
    return R.Session(cam=CAM, frames=frames, tracks=[], rs=0, scanlines=[0, 480])


def both(exe, tmp_path, sess, tables, opt, first=0, last=0):
    want, s = py_replay(sess, tables, opt, first, last)
    got = run_replay(exe, tmp_path, sess, tables, opt, first, last)
    assert got == want
    return s


def test_the_match_loop_goes_on_after_it_creates_a_track(exe, tmp_path):
    sess = two_frame_session()
    sess.frames[0].obs[0].matches = [[1, 0, False], [2, 0, False]]
    tables = {0: ([1, 1], [0, 0], [[1, 2, 3], [4, 5, 6]])}
    s = both(exe, tmp_path, sess, tables, R.Options())
    assert len(s.tracks) == 2 and s.frames[0].obs[0].track == 1                       # o names the newest track
    assert s.frames[1].obs[0].track == 0 and s.frames[2].obs[0].track == 1
    assert s.tracks[0].obs == [[1, 0, True], [0, 0, True]] and s.tracks[1].obs == [[2, 0, True], [0, 0, True]]
    assert s.tracks[0].pt == [1, 2, 3] and not s.tracks[0].valid                       # 2 < minReprojections
    assert all(m[2] for m in s.frames[0].obs[0].matches)


def test_reprojection_moves_an_observation_that_already_has_a_track(exe, tmp_path):
    sess = two_frame_session()
    sess.tracks = [R.Track(obs=[[0, 0, True], [2, 0, True]], pt=[0, 0, 5], valid=True), R.Track(obs=[[1, 0, True], [2, 0, True]], pt=[0, 0, 6])]
    sess.frames[2].obs[0].track = 0; sess.frames[2].obs[0].has_track = True
    sess.frames[0].obs[0].track, sess.frames[0].obs[0].has_track = 0, True
    sess.frames[1].obs[0].track, sess.frames[1].obs[0].has_track = 1, True
    sess.frames[0].obs[0].matches = [[1, 0, False]]
    s = both(exe, tmp_path, sess, {0: ([0], [1], [[0, 0, 0]])}, R.Options(min_reprojections=3))
    assert s.frames[0].obs[0].track == 1 and s.tracks[1].obs[-1] == [0, 0, True] and s.tracks[1].valid
    assert s.tracks[0].obs == [[0, 0, True], [2, 0, True]]                             # the old track still lists it


def test_max_reprojections(exe, tmp_path):
    sess = two_frame_session()
    sess.tracks = [R.Track(obs=[[1, 0, True], [2, 0, True]], pt=[0, 0, 6])]
    for f in (1, 2):
        sess.frames[f].obs[0].track, sess.frames[f].obs[0].has_track = 0, True
    sess.frames[0].obs[0].matches = [[1, 0, False]]
    tables = {0: ([1], [1], [[0, 0, 0]])}
    s = both(exe, tmp_path, sess, tables, R.Options(max_reprojections=2))
    assert not s.frames[0].obs[0].has_track and len(s.tracks[0].obs) == 2            # full: skipped, o2 tracked: no creation
    s = both(exe, tmp_path, sess, tables, R.Options(max_reprojections=0))
    assert s.frames[0].obs[0].track == 0 and len(s.tracks[0].obs) == 3                # 0: no limit


def test_const3d_joins_but_neither_creates_nor_validates(exe, tmp_path):
    sess = two_frame_session()
    sess.tracks = [R.Track(obs=[[1, 0, True], [2, 0, True]], pt=[0, 0, 6])]
    for f in (1, 2):
        sess.frames[f].obs[0].track, sess.frames[f].obs[0].has_track = 0, True
    sess.frames[0].obs.append(R.Obs(20, 20, matches=[[1, 1, False]]))
    sess.frames[0].obs[0].matches = [[1, 0, False]]
    tables = {0: ([0, 1], [1, 0], [[0, 0, 0], [7, 8, 9]])}
    s = both(exe, tmp_path, sess, tables, R.Options(const3d=True, min_reprojections=3))
    assert s.frames[0].obs[0].track == 0 and not s.tracks[0].valid and len(s.tracks) == 1
    s = both(exe, tmp_path, sess, tables, R.Options(const3d=False, min_reprojections=3))
    assert s.tracks[0].valid and len(s.tracks) == 2


def test_matches_inside_the_frame_or_into_a_frame_without_poses_throw_in_the_creation_branch(exe, tmp_path):
    sess = two_frame_session()
    sess.frames[1].obs[1].matches = [[1, 0, False]]
    assert py_replay(sess, {1: ([0], [0], [[0, 0, 0]])}, R.Options(), 1, 1)[0] == "threw"
    assert run_replay(exe, tmp_path, sess, {1: ([0], [0], [[0, 0, 0]])}, R.Options(), 1, 1) == "threw"
    sess = two_frame_session()
    sess.frames[2].poses = None
    sess.frames[0].obs[0].matches = [[2, 0, False]]
    assert py_replay(sess, {0: ([1], [0], [[0, 0, 0]])}, R.Options(), 0, 0)[0] == "threw"
    assert run_replay(exe, tmp_path, sess, {0: ([1], [0], [[0, 0, 0]])}, R.Options(), 0, 0) == "threw"
    # the reprojection branch takes a match inside the frame: o joins the track of another observation of its frame
    sess = two_frame_session()
    sess.tracks = [R.Track(obs=[[2, 0, True]], pt=[0, 0, 6])]
    sess.frames[1].obs[1].track, sess.frames[1].obs[1].has_track = 0, True          # listed nowhere: the session is not consistent
    sess.frames[1].obs[0].matches = [[1, 1, False]]
    s = both(exe, tmp_path, sess, {1: ([0], [1], [[0, 0, 0]])}, R.Options(), 1, 1)
    assert s.frames[1].obs[0].track == 0 and s.tracks[0].obs[-1] == [1, 0, True]


def test_a_flag_the_replay_needs_but_was_not_given_is_an_error(exe, tmp_path):
    sess = two_frame_session()
    sess.frames[0].obs[0].matches = [[1, 0, False]]
    tables = {0: ([2], [0], [[0, 0, 0]])}                                          # 2: not computed
    with pytest.raises(LookupError):
        py_replay(sess, tables, R.Options(), 0, 0)
    assert run_replay(exe, tmp_path, sess, tables, R.Options(), 0, 0) == "threw"


def test_a_frame_without_poses_throws_only_where_get_pose_is_reached(exe, tmp_path):
    """getPose throws "empty frame" lazily (struct/VideoSfM.cc:105): a pose-less frame whose matches are all skipped before any
    pose is needed goes through; one whose creation or reprojection branch needs the pose throws.  No device call is reached."""
    def run(sess, mode):
        (tmp_path / "s.cache").write_bytes(R.to_cache(sess, T))
        return subprocess.run([exe, mode, str(tmp_path / "s.cache"), str(tmp_path / "o.bin"), "first=0", "last=0"], capture_output=True, text=True)

    # o tracked, its only match in the same track (inTrack): nothing needs a pose
    sess = two_frame_session()
    sess.frames[0].poses = None
    sess.tracks = [R.Track(obs=[[0, 0, True], [1, 0, True]], pt=[0, 0, 5], valid=True)]
    for f in (0, 1):
        sess.frames[f].obs[0].track, sess.frames[f].obs[0].has_track = 0, True
    sess.frames[0].obs[0].matches = [[1, 0, False]]
    want = R.clone(sess)
    R.create_tracks(want, 0, R.Options(), R.TableGeometry(want, {0: ([2], [2], [[0, 0, 0]])}))   # (2: a flag it reads would raise)
    for mode in ("frame", "batch"):
        r = run(sess, mode)
        assert r.returncode == 0, r.stderr
        assert R.read_state(tmp_path / "o.bin")[1:] == R.state_of(want)
    # creation branch: o and o2 untracked -> getPose(o)
    sess = two_frame_session()
    sess.frames[0].poses = None
    sess.frames[0].obs[0].matches = [[1, 0, False]]
    # reprojection branch: o2 in a track without frame 0 -> getPose(o) before validate
    sess2 = two_frame_session()
    sess2.frames[0].poses = None
    sess2.tracks = [R.Track(obs=[[1, 0, True]], pt=[0, 0, 5])]
    sess2.frames[1].obs[0].track, sess2.frames[1].obs[0].has_track = 0, True
    sess2.frames[0].obs[0].matches = [[1, 0, False]]
    for s_ in (sess, sess2):
        with pytest.raises(R.CreateTracksError, match="empty frame"):
            R.create_tracks(R.clone(s_), 0, R.Options(), R.TableGeometry(s_, {0: ([3], [3], [[0, 0, 0]])}))
        for mode in ("frame", "batch"):
            r = run(s_, mode)
            assert r.returncode == 3 and "empty frame" in r.stderr, (r.returncode, r.stderr)


# ---- self-checks of the restatement's oracle geometry (no product code: the device side of both quirks is checked in
# ---- tests/test_gpu_tracks.py, test_a_thousands_of_candidates_call_and_equal_poses and test_synthetic_runs_eval_tracks)

def test_restatement_skips_equal_poses_bitwise(oracle):
    sess = two_frame_session()
    sess.frames[1].poses = [[0.0] * 6]
    sess.frames[0].obs[0] = R.Obs(330, 245, matches=[[1, 0, False]])   # (not the principal point: its undistortion never converges)
    sess.frames[1].obs[0] = R.Obs(340, 250)
    opt = R.Options()
    g = R.OracleGeometry(oracle, opt)
    assert g.tri(sess, 0, 0, 0) == (False, None)                                     # equal: no triangulation at all
    sess.frames[1].poses = [[0.0, 0.0, -0.0, 0.0, 0.0, 0.0]]                        # -0.0 != +0.0 for memcmp: the solve runs
    good, pt = g.tri(sess, 0, 0, 0)
    assert not good and pt is not None and np.abs(pt).max() < 1e-12                 # (it meets at the common centre, behind w2i's 1e-8)
    s = R.clone(sess)
    R.create_tracks(s, 0, opt, g)
    assert len(s.tracks) == 0


def test_restatement_synthetic_drops_the_observations_validate_accepts(oracle):
    cam = CAM
    sess = R.Session(cam=cam, frames=[R.Frame(obs=[R.Obs(320, 240), R.Obs(100, 100)], poses=[[0.0] * 6]),
                                      R.Frame(obs=[R.Obs(320, 240)], poses=[[0, 0, 0, 1, 0, 0]])],
                     tracks=[R.Track(obs=[[0, 0, True], [0, 1, True], [1, 0, True]], pt=[0, 0, 5], valid=True)], rs=0, scanlines=[0, 480])
    for k in (0, 1):
        sess.frames[0].obs[k].track, sess.frames[0].obs[k].has_track = 0, True
    opt = R.Options(synthetic=True, min_reprojections=3)
    s = R.clone(sess)
    R.create_tracks(s, 0, opt, R.OracleGeometry(oracle, opt))
    # (320, 240) sees [0, 0, 5] exactly: validate accepts, so it is DROPPED; (100, 100) is 312 px off and stays
    assert not s.frames[0].obs[0].has_track and s.frames[0].obs[1].has_track
    assert s.tracks[0].obs == [[0, 1, True], [1, 0, True]] and not s.tracks[0].valid


def test_the_new_entry_fails_loudly_without_a_device(exe, tmp_path):
    import torch
    from rsba_amd import capi
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.RsbaError):
        capi.track_candidates(np.array(CAM), None, [np.zeros((1, 6)), np.array([[0, 0, 0, 1, 0, 0.0]])], 0, [0, 480], [0, 1],
                              [[320, 240], [330, 240]], [0], [1], [capi.TRACK_TRIANGULATE])
    sess = two_frame_session()
    sess.frames[0].obs[0].matches = [[1, 0, False]]
    (tmp_path / "s.cache").write_bytes(R.to_cache(sess, T))
    for mode in ("frame", "batch"):
        r = subprocess.run([exe, mode, str(tmp_path / "s.cache"), str(tmp_path / "o.bin")], capture_output=True, text=True)
        assert r.returncode == 3 and "rsba_amd" in r.stderr, (r.returncode, r.stderr)
