"""The incremental step over a session (include/rsba/new_frame.hpp: processFrame -> newFrame -> solve -> solveRsPnP / createTracks /
windowedBA) through examples/new_frame, on a 12-frame, 300-point rolling-shutter scene with matches and tracks: the true poses and
points of rsba_amd.scene.make_scene, 0.3 px of observation noise, every observation matched to its point's two previous observations,
tracks for half of the points."""
import os
import struct
import subprocess

import numpy as np
import pytest

import thrift_encode as T
from rsba_amd.problem import GLOBAL
from rsba_amd.scene import make_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, M = 12, 300


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as G
    path = os.path.join(ROOT, "examples", "new_frame")
    if not os.path.exists(path):
        G.build()
    return path


class Sess:
    """frames: [dict(obs=[dict(x, y, matches, track)], poses, prior)], tracks: [dict(obs, pt)]"""
    def __init__(self, rolling=True, seed=5):
        self.sc = sc = make_scene(F, M, rolling=rolling, seed=seed, noise_px=0.3, rot_noise=0.0, pos_noise=0.0, pt_noise=0.0)
        p = sc.problem
        self.cam, self.rs, self.scan = p.intrinsics[0], int(p.shutter), list(p.scanlines)
        self.frames = [dict(obs=[], poses=[list(q) for q in sc.true_poses[f]], prior=None) for f in range(F)]
        seen = {}
        for i in np.argsort(p.obs_frame, kind="stable"):
            f, j = int(p.obs_frame[i]), int(p.obs_point[i])
            k = len(self.frames[f]["obs"])
            self.frames[f]["obs"].append(dict(x=float(p.obs_xy[i, 0]), y=float(p.obs_xy[i, 1]), matches=[(pf, pk, False) for pf, pk in seen.get(j, [])[-2:]], track=None))
            seen.setdefault(j, []).append((f, k))
        keep = [j for j in sorted(seen) if j % 2 == 0]
        self.tracks = [dict(obs=[(f, k, True) for f, k in seen[j]], pt=list(sc.true_points[j])) for j in keep]
        for t, j in enumerate(keep):
            for f, k in seen[j]:
                self.frames[f]["obs"][k]["track"] = t

    def cache(self):
        frames = [T.frame([T.observation(o["x"], o["y"], track=o["track"], matches=o["matches"] or None) for o in fr["obs"]], poses=fr["poses"], prior_poses=fr["prior"])
                  for fr in self.frames]
        tracks = [T.track(t["obs"], pt=t["pt"], valid=True) for t in self.tracks]
        return T.file_events(T.session(self.cam, frames, tracks, self.rs, self.scan, 1280, 720), np.random.default_rng(1), max_event=4096)


@pytest.fixture(scope="module")
def base():
    return Sess()


def run(exe, tmp_path, sess, *kv, name="o"):
    (tmp_path / "s.cache").write_bytes(sess.cache())
    out = tmp_path / (name + ".bin")
    r = subprocess.run([exe, str(tmp_path / "s.cache"), str(out), *kv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    buf = out.read_bytes()
    pos = 0

    def q():
        nonlocal pos
        v = struct.unpack_from("<q", buf, pos)[0]; pos += 8; return v

    def d(n):
        nonlocal pos
        v = struct.unpack_from(f"<{n}d", buf, pos); pos += 8 * n; return list(v)
    report = [dict(key=q(), ok=q(), localised=q(), before=q(), after=q()) for _ in range(q())]
    poses, frames, tracks = [], [], []
    for _ in range(q()):
        poses.append([d(6) for _ in range(q())])
        frames.append([(q(), bool(q()), [bool(q()) for _ in range(q())]) for _ in range(q())])
    for _ in range(q()):
        pt = d(3); valid = bool(q())
        tracks.append((pt, valid, [[q(), q(), bool(q())] for _ in range(q())]))
    assert pos == len(buf)
    return dict(report=report, poses=poses, frames=frames, tracks=tracks, bytes=buf)


def pose_error(got, sess, f):
    return float(np.max(np.abs(np.array(got["poses"][f]) - sess.sc.true_poses[f][:len(got["poses"][f])])))


def test_last_frame_without_poses_is_localised_and_tracked(exe, tmp_path, base):
    got = run(exe, tmp_path, base)
    rep = got["report"][0]
    assert rep["key"] == F - 1 and rep["ok"] == 1 and rep["localised"] == 1
    assert len(got["poses"][F - 1]) == 2 and pose_error(got, base, F - 1) <= 0.05      # the tolerance of the PnP tests on scenes with this noise
    assert rep["after"] > rep["before"] == len(base.tracks)                             # new tracks (the points without one, seen three times)
    with_track = [o for o in got["frames"][F - 1] if o[1]]
    assert len(with_track) >= 0.5 * len(got["frames"][F - 1])
    assert any(o[0] >= rep["before"] for o in with_track) and any(o[0] < rep["before"] for o in with_track)
    # baIterationsOnNewFrame = 0: the earlier frames' poses and all points are bitwise what they were
    for f in range(F - 1):
        assert np.array_equal(np.array(got["poses"][f]), np.array(base.frames[f]["poses"]))
    for t, tr in enumerate(base.tracks):
        assert got["tracks"][t][0] == [float(v) for v in tr["pt"]]
    again = run(exe, tmp_path, base, name="again")
    assert again["bytes"] == got["bytes"]                                               # two runs, the same bytes


def average_reprojection_error(oracle, sess, got):
    """root mean square reprojection error over every observation whose track has a point, at the state the example wrote"""
    sq, cnt = 0.0, 0
    for f, obs in enumerate(got["frames"]):
        for k, (track, has, _) in enumerate(obs):
            if not has or not got["tracks"][track][1]:
                continue
            ok, p = oracle.reproject(sess.cam, np.array(got["poses"][f]), sess.rs, sess.scan, np.array(got["tracks"][track][0]), 1e12)
            o = sess.frames[f]["obs"][k]
            if ok:
                sq += (p[0] - o["x"]) ** 2 + (p[1] - o["y"]) ** 2; cnt += 1
    return np.sqrt(sq / cnt), cnt


def test_three_frames_re_added_with_a_windowed_ba(exe, oracle, tmp_path, base):
    """every frame is localised, and the final average reprojection error is not above that of the same run started from the true poses
    (keepPoses=1: nothing to localise, the same windowed BA after every frame) by more than a margin.

    The margin: both runs end in the same windowed bundle adjustments (five iterations each, Ceres' function tolerance 1e-6) over the same
    observations, so once the re-localised frames are in the basin of the true ones the two final errors differ by what five capped
    iterations leave between two starts — a small fraction of the error itself, which is set by the 0.3 px observation noise — while one
    mislocalised frame adds tens of pixels over its ~150 observations.  The margin is 2 % of the reference run's error: between the two.
    Measured on an MI355X: from the true poses 0.770287 px over 2229 observations, re-localised 0.769754 px over 2229 (0.07 % below)."""
    kv = ("k=3", "baIterationsOnNewFrame=5", "baWindowOnNewFrame=4", "fixFirstN=1")
    got = run(exe, tmp_path, base, *kv)
    assert [r["key"] for r in got["report"]] == [F - 3, F - 2, F - 1]
    assert all(r["ok"] == 1 and r["localised"] == 1 and r["after"] >= r["before"] for r in got["report"])
    assert max(pose_error(got, base, f) for f in range(F - 3, F)) <= 0.05
    ref = run(exe, tmp_path, base, *kv, "keepPoses=1", name="ref")
    e_got, n_got = average_reprojection_error(oracle, base, got)
    e_ref, n_ref = average_reprojection_error(oracle, base, ref)
    print(f"average reprojection error: re-localised {e_got:.6f} px over {n_got} observations, from the true poses {e_ref:.6f} px over {n_ref}")
    assert n_got >= 0.98 * n_ref
    assert e_got <= 1.02 * e_ref


def test_prior_poses_are_the_start(exe, tmp_path):
    """with both solvers off the success rule of VideoSfMHandler.cc:748 writes the start back: the priors when the frame has them, the last
    pose of the previous frame otherwise (reuseLastPose); with the solver on, the frame is localised from them"""
    s = Sess()
    rng = np.random.default_rng(3)
    prior = [list(np.array(q) + np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.08, 3)])) for q in s.sc.true_poses[F - 1]]
    s.frames[F - 1]["prior"] = prior
    start = run(exe, tmp_path, s, "solveRsPnP=0", "reuseLastPose=0")
    assert start["report"][0]["localised"] == 1 and np.max(np.abs(np.array(start["poses"][F - 1]) - np.array(prior))) <= 1e-12
    last = run(exe, tmp_path, s, "solveRsPnP=0", "keepPriors=0")
    assert np.max(np.abs(np.array(last["poses"][F - 1]) - np.array(s.frames[F - 2]["poses"][1])[None, :])) <= 1e-12
    got = run(exe, tmp_path, s, "reuseLastPose=0")
    assert got["report"][0]["localised"] == 1 and pose_error(got, s, F - 1) <= 0.05


def test_the_dlt_path_alone_localises_the_frame(exe, tmp_path, base):
    got = run(exe, tmp_path, base, "reuseLastPose=0", "solveGsPnP=1")
    assert got["report"][0]["localised"] == 1 and pose_error(got, base, F - 1) <= 0.05


def test_global_shutter_session(exe, tmp_path):
    s = Sess(rolling=False)
    assert s.rs == GLOBAL
    got = run(exe, tmp_path, s, "solveGsPnP=1", "reuseLastPose=0")
    assert got["report"][0]["localised"] == 1 and len(got["poses"][F - 1]) == 1 and pose_error(got, s, F - 1) <= 0.05
    assert got["report"][0]["after"] > got["report"][0]["before"]
    guess = run(exe, tmp_path, s, "solveGsPnP=1")                # from the last pose: the extrinsic-guess attempt
    assert guess["report"][0]["localised"] == 1 and pose_error(guess, s, F - 1) <= 0.05


def test_too_few_correspondences(exe, tmp_path):
    """at most 4 correspondences: false, the frame is left without poses, the session untouched (minReprojections above the frame's key
    keeps the direct PnP, which would extrapolate a pose, out of it)"""
    s = Sess()
    linked = 0
    for o in s.frames[F - 1]["obs"]:
        if o["matches"] and any(s.frames[pf]["obs"][pk]["track"] is not None for pf, pk, _ in o["matches"]):
            linked += 1
            if linked > 4:
                o["matches"] = []
    got = run(exe, tmp_path, s, "minReprojections=100")
    rep = got["report"][0]
    assert rep["ok"] == 0 and rep["localised"] == 0 and got["poses"][F - 1] == [] and rep["after"] == rep["before"]
    assert not any(o[1] for o in got["frames"][F - 1])
    for f in range(F - 1):
        assert np.array_equal(np.array(got["poses"][f]), np.array(s.frames[f]["poses"]))
    for t, tr in enumerate(s.tracks):
        assert got["tracks"][t][0] == [float(v) for v in tr["pt"]] and got["tracks"][t][2] == [[f, k, True] for f, k, _ in tr["obs"] if f < F - 1]


def frame_cost(oracle, sess, poses, f):
    """sum of squared reprojection errors of frame f's observations that reach a point through their matches, at `poses`"""
    sq = 0.0
    for o in sess.frames[f]["obs"]:
        for pf, pk, _ in o["matches"]:
            t = sess.frames[pf]["obs"][pk]["track"]
            if t is not None:
                ok, p = oracle.reproject(sess.cam, np.array(poses), sess.rs, sess.scan, np.array(sess.tracks[t]["pt"]), 1e12)
                assert ok
                sq += (p[0] - o["x"]) ** 2 + (p[1] - o["y"]) ** 2
                break
    return sq


def test_pnp_new_frame_runs_the_direct_pnp_with_constant_points(exe, oracle, tmp_path):
    s = Sess()
    rng = np.random.default_rng(7)
    start = [list(np.array(q) + np.concatenate([rng.normal(0, 0.004, 3), rng.normal(0, 0.03, 3)])) for q in s.sc.true_poses[F - 1]]
    s.frames[F - 1]["poses"] = start
    still = run(exe, tmp_path, s, "keepPoses=1")
    assert np.array_equal(np.array(still["poses"][F - 1]), np.array(start))                       # without pnpNewFrame the poses stay
    # baWindowOnNewFrame=1: the windowed BA that follows covers this frame alone, and freezes every track an earlier frame sees
    got = run(exe, tmp_path, s, "keepPoses=1", "pnpNewFrame=1", "baIterationsOnNewFrame=8", "baWindowOnNewFrame=1", name="pnp")
    assert got["report"][0]["localised"] == 1
    for t, tr in enumerate(s.tracks):
        assert got["tracks"][t][0] == [float(v) for v in tr["pt"]]                                # const3d, and the frozen old tracks of the window
    before, after = frame_cost(oracle, s, start, F - 1), frame_cost(oracle, s, got["poses"][F - 1], F - 1)
    print(f"frame cost before {before:.4f} after {after:.4f}")
    assert after <= before and not np.array_equal(np.array(got["poses"][F - 1]), np.array(start))


def test_refine_pnp_runs(exe, tmp_path, base):
    got = run(exe, tmp_path, base, "refinePnP=1")
    assert got["report"][0]["localised"] == 1 and pose_error(got, base, F - 1) <= 0.05 and got["report"][0]["after"] > got["report"][0]["before"]
