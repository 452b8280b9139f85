"""What the tests of the geometric verification share (test_verify_pairs_host.py, test_gpu_verify_pairs.py, test_gpu_verify_matches.py): the
frame pairs, assembled from the scenes the two-view tests already use, the files the C++ programs read, and the small session with seeded
wrong refs.  Nothing here calls the library."""
import struct

import numpy as np

import five_point_reference as F5
import two_view_reference as R
from p3p_reference import CAM_DIST, CAM_PLAIN, project

OPTIONS = dict(iterations=100, threshold_px=4.0, refits=3, min_inliers=16, rng_state=R.RANSAC["rng_state"])


def pair(cam_a, cam_b, xy_a, xy_b, name):
    return dict(cam_a=np.asarray(cam_a, dtype=np.float64), cam_b=np.asarray(cam_b, dtype=np.float64), xy_a=np.ascontiguousarray(xy_a, dtype=np.float32),
                xy_b=np.ascontiguousarray(xy_b, dtype=np.float32), name=name)


def small_pairs():
    """the case list of two_view_reference (n = 8 .. 48; the degenerate case cut into its pure-rotation and coincident-point parts, n = 8
    each, every hypothesis declined), the planar scene, a pair with two different cameras (distorted / pinhole), a pair with n = 7"""
    out = []
    for name, c in R.cases().items():
        if name == "degenerate":
            out.append(pair(c["cam_a"], c["cam_b"], c["xy_a"][32:40], c["xy_b"][32:40], "pure_rotation"))
            out.append(pair(c["cam_a"], c["cam_b"], c["xy_a"][40:48], c["xy_b"][40:48], "coincident"))
        out.append(pair(c["cam_a"], c["cam_b"], c["xy_a"], c["xy_b"], name))
    s = F5.planar_scene(0)
    out.append(pair(s["cam"], s["cam"], s["xy_a"], s["xy_b"], "planar"))
    rng = np.random.default_rng(41)
    X = R._cloud(rng, 37)
    pose = R._unit_centre(R.POSE_B)
    out.append(pair(CAM_DIST, CAM_PLAIN, project(CAM_DIST, np.zeros(6), X), project(CAM_PLAIN, pose, X), "two_cameras"))
    out.append(pair(CAM_PLAIN, CAM_DIST, project(CAM_PLAIN, np.zeros(6), X), project(CAM_DIST, pose, X), "two_cameras_swapped"))
    return out


def short_pair():
    c = R.cases()["main_distorted"]
    return pair(c["cam_a"], c["cam_b"], c["xy_a"][:7], c["xy_b"][:7], "seven")


SPARSE_SEED = 6   # of seeds 0 .. 11, the one whose m = 5 winner keeps exactly the six (the others: seven or eight inliers)


def sparse_pair(seed=SPARSE_SEED):
    """n = 10, mostly gross outliers: six noise-free correspondences of a cloud and four pairs of unrelated pixels, shuffled.  A five-point
    hypothesis from five of the six collects the six (and, by chance, perhaps a seventh) and nothing more, so the winner of m = 5 has fewer
    inliers than a refit takes: the loop ends at the compaction of the first round with a non-zero count.  test_verify_pairs_host.py checks on
    the host that this seed does so."""
    rng = np.random.default_rng(seed)
    X = R._cloud(rng, 6)
    pose = R._unit_centre(R.POSE_B)
    xy_a = np.concatenate([project(CAM_PLAIN, np.zeros(6), X), rng.uniform([40.0, 40.0], [1240.0, 680.0], (4, 2))])
    xy_b = np.concatenate([project(CAM_PLAIN, pose, X), rng.uniform([40.0, 40.0], [1240.0, 680.0], (4, 2))])
    order = rng.permutation(10)
    return pair(CAM_PLAIN, CAM_PLAIN, xy_a[order], xy_b[order], "sparse")


def outlier_pairs():
    out = []
    for fb, rolling in R.OUTLIER_SCENES:
        s = R.outlier_scene(fb, rolling)
        out.append(pair(s["cam"], s["cam"], s["xy_a"], s["xy_b"], R.scene_name(fb, rolling)))
    return out


def write_pairs_file(path, pairs):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(pairs)))
        for p in pairs:
            f.write(struct.pack("<i", len(p["xy_a"])))
            f.write(p["cam_a"].astype("<f8").tobytes()); f.write(p["cam_b"].astype("<f8").tobytes())
            f.write(p["xy_a"].astype("<f4").tobytes()); f.write(p["xy_b"].astype("<f4").tobytes())


def parse_results(text, count):
    """the four lines per pair that the programs print -> list of dict(ok, winner_task, num_inliers, num_front, refits_adopted, E, pose, mask)"""
    lines = text.split("\n")
    assert len(lines) >= 4 * count
    out = []
    for p in range(count):
        head = [int(v) for v in lines[4 * p].split()]
        out.append(dict(ok=bool(head[0]), winner_task=head[1], num_inliers=head[2], num_front=head[3], refits_adopted=head[4],
                        E=np.array([float(v) for v in lines[4 * p + 1].split()]), pose=np.array([float(v) for v in lines[4 * p + 2].split()]),
                        mask=np.array([int(v) for v in lines[4 * p + 3].split()], dtype=bool)))
    return out


def option_args(o, solver):
    return [str(o["iterations"]), str(o["threshold_px"]), str(o["refits"]), str(o["min_inliers"]), str(o["rng_state"]), str(solver)]


# ---------------------------------------------------------------- the session ----------------------------------------------------------------
class SmallSession:
    """5 frames of the global-shutter 12-frame scene (frames 0, 1, 2, 4, 5 of it), 120 of its points; an observation is matched to its
    point's observation in each of the (up to) two frames before it.  Seeded wrong refs: every seventh match points at another point's
    observation of that frame — a gross outlier of the pair's geometry — and a fifth of the observations carry BOTH the right ref and a wrong
    one into the same frame, so an observation's list holds refs of several pairs and several refs of one.  Frame 4 also has 5 refs into
    frame 0: a pair under 8 correspondences."""
    SOURCE = (0, 1, 2, 4, 5)

    def __init__(self):
        from rsba_amd.scene import make_scene
        self.sc = sc = make_scene(12, 600, rolling=False, seed=5, noise_px=0.3, rot_noise=0.0, pos_noise=0.0, pt_noise=0.0)
        p = sc.problem
        self.cam = np.asarray(p.intrinsics[0], dtype=np.float64)
        self.true_poses = [sc.true_poses[f, :1].tolist() for f in self.SOURCE]
        index = {f: i for i, f in enumerate(self.SOURCE)}
        self.frames = [[] for _ in self.SOURCE]               # per frame: dict(x, y, point, matches [(frame, obs)], wrong: set of slots)
        where = [dict() for _ in self.SOURCE]                  # per frame: point -> observation
        for i in np.argsort(p.obs_frame, kind="stable"):
            f, j = int(p.obs_frame[i]), int(p.obs_point[i])
            if f in index and j < 120:
                where[index[f]][j] = len(self.frames[index[f]])
                self.frames[index[f]].append(dict(x=float(p.obs_xy[i, 0]), y=float(p.obs_xy[i, 1]), point=j, matches=[], wrong=set()))
        count = 0
        for fi in range(1, len(self.frames)):
            for o in self.frames[fi]:
                for fa in range(max(0, fi - 2), fi):
                    if o["point"] not in where[fa]:
                        continue
                    right = where[fa][o["point"]]
                    other = (right + 11) % len(self.frames[fa])
                    count += 1
                    if count % 7 == 0:
                        o["wrong"].add(len(o["matches"])); o["matches"].append((fa, other))
                    else:
                        o["matches"].append((fa, right))
                        if count % 5 == 0:
                            o["wrong"].add(len(o["matches"])); o["matches"].append((fa, other))
        few = 0
        for o in self.frames[3]:
            if o["point"] in where[0] and few < 5:
                o["matches"].append((0, where[0][o["point"]])); few += 1

    def pairs(self):
        """(frameA, frameB) -> list of (observation of B, slot), in observation order, then list order — as verifyMatches states it"""
        out = {}
        for fb, frame in enumerate(self.frames):
            for oi, o in enumerate(frame):
                for slot, (fa, _) in enumerate(o["matches"]):
                    if fa < fb:
                        out.setdefault((fb, fa), []).append((oi, slot))
        return {(fa, fb): out[(fb, fa)] for fb, fa in sorted(out)}

    def pair_arrays(self, fa, fb, refs):
        xy_a = [[self.frames[fa][self.frames[fb][oi]["matches"][slot][1]][k] for k in ("x", "y")] for oi, slot in refs]
        xy_b = [[self.frames[fb][oi][k] for k in ("x", "y")] for oi, _ in refs]
        return pair(self.cam, self.cam, np.array(xy_a).reshape(-1, 2), np.array(xy_b).reshape(-1, 2), f"{fa}_{fb}")

    def expected(self, results, min_inliers, drop_unverified):
        """results: the per-pair RANSAC of every pair in the order of pairs() -> (the refs that remain per (frame, obs), removed per pair)"""
        kill, removed = set(), []
        for ((fa, fb), refs), r in zip(self.pairs().items(), results):
            ok = len(refs) >= 8 and r["ok"]
            gone = [i for i in range(len(refs)) if (ok and not r["mask"][i]) or (not ok and drop_unverified)]
            removed.append(len(gone))
            kill |= {(fb, refs[i][0], refs[i][1]) for i in gone}
        left = {}
        for fb, frame in enumerate(self.frames):
            for oi, o in enumerate(frame):
                keep = [m for slot, m in enumerate(o["matches"]) if (fb, oi, slot) not in kill]
                if keep:
                    left[(fb, oi)] = keep
        return left, removed

    def write_plain(self, path):
        """the file tests/verify_pairs_host.cpp reads"""
        with open(path, "wb") as f:
            f.write(struct.pack("<i", len(self.frames))); f.write(self.cam.astype("<f8").tobytes())
            for frame in self.frames:
                f.write(struct.pack("<ii", 0, len(frame)))
                for o in frame:
                    f.write(struct.pack("<ddi", o["x"], o["y"], len(o["matches"])))
                    for fa, oa in o["matches"]:
                        f.write(struct.pack("<ii", fa, oa))


def parse_session_output(text):
    """what verify_pairs_host session and examples/verify_matches dump=1 print -> (reports, bootstrap, refs left per (frame, obs), untouched or None)"""
    lines = text.strip().split("\n")
    count = int(lines[0].split()[1])
    reports = []
    for line in lines[1:1 + count]:
        v = line.split()
        reports.append(dict(frameA=int(v[0]), frameB=int(v[1]), correspondences=int(v[2]), ok=bool(int(v[3])), num_inliers=int(v[4]), num_front=int(v[5]), removed=int(v[6]),
                            E=np.array([float(x) for x in v[7:16]]), pose=np.array([float(x) for x in v[16:22]])))
    bootstrap = int(lines[1 + count].split()[1])
    left, untouched = {}, None
    for line in lines[2 + count:]:
        v = line.split()
        if v[0] == "refs":
            left[(int(v[1]), int(v[2]))] = [(int(v[k]), int(v[k + 1])) for k in range(3, len(v), 2)]
        elif v[0] == "untouched":
            untouched = bool(int(v[1]))
    return reports, bootstrap, left, untouched
