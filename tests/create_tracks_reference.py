"""A Python restatement of rsba's track creation, for the tests: VideoSfMHandler::reprojectMatches, createTracks and evalTracks
(VideoSfMHandler.cc:231-410) and inTrack (struct/VideoSfM.h:155-160), written from their meaning, decision by decision in the
reference's order.  The geometry is injectable: `OracleGeometry` composes the CPU oracle's scalar restatements (getPose,
direction, triangulate, validate), `TableGeometry` answers from given flag tables (the layout of TrackFlags in
include/rsba/create_tracks.hpp and of the flag file of examples/create_tracks.cpp).

Sessions are plain objects: Session(cam, frames, tracks, rs, scanlines), Frame(obs, poses, cam), Obs(x, y, matches, track,
has_track), Track(obs, pt, valid); a match / track entry is a list [frame, obs, valid]."""
from __future__ import annotations

import copy
import struct
from dataclasses import dataclass, field

import numpy as np


@dataclass
class Obs:
    x: float
    y: float
    matches: list | None = None      # None: __isset.matches false
    track: int = 0
    has_track: bool = False


@dataclass
class Frame:
    obs: list
    poses: list | None = None        # None: __isset.poses false
    cam: list | None = None


@dataclass
class Track:
    obs: list
    pt: list | None
    valid: bool = False


@dataclass
class Session:
    cam: list
    frames: list
    tracks: list
    rs: int = 0
    scanlines: list = field(default_factory=lambda: [0, 1])


@dataclass
class Options:
    sqrd_threshold: float = 16.0
    min_reprojections: int = 3
    max_reprojections: int = 10
    min_distance: float = 0.0
    const3d: bool = False
    synthetic: bool = False
    interpolate_rotation: bool = True


class CreateTracksError(RuntimeError):
    pass


def in_track(t, frame_key):
    """struct/VideoSfM.h:155-160"""
    return any(r[0] == frame_key for r in t.obs)


def ref_offsets(frame):
    off = [0]
    for o in frame.obs:
        off.append(off[-1] + (len(o.matches) if o.matches is not None else 0))
    return off


def reproject_matches(sess, fk, ok, opt, geom):
    """VideoSfMHandler.cc:231-280.  The distance gate (:253-256, at getPose(o) — see the header of create_tracks.hpp) and the
    validation (:262) are one predicate of the geometry; both only skip the match, so asking after inTrack is the same decision."""
    o = sess.frames[fk].obs[ok]
    if o.matches is None:
        return False
    for j, ref in enumerate(o.matches):
        o2 = sess.frames[ref[0]].obs[ref[1]]
        if not o2.has_track:
            continue
        t = sess.tracks[o2.track]
        if opt.max_reprojections > 0 and len(t.obs) >= opt.max_reprojections:
            continue
        if in_track(t, fk):
            continue
        if geom.reproj(sess, fk, ok, j, t.pt):
            o.track = o2.track
            o.has_track = True
            t.obs.append([fk, ok, True])
            if not opt.const3d and len(t.obs) >= opt.min_reprojections:
                t.valid = True
            return True
    return False


def create_tracks(sess, fk, opt, geom):
    """VideoSfMHandler.cc:283-372"""
    if opt.synthetic:
        return eval_tracks(sess, fk, opt, geom)
    f = sess.frames[fk]
    for ok, o in enumerate(f.obs):
        if o.matches is None:
            continue
        reproject_matches(sess, fk, ok, opt, geom)
        if opt.const3d or o.has_track:
            continue
        for j, ref in enumerate(o.matches):            # does not stop after a track is created
            if ref[0] == fk:
                raise CreateTracksError("a match inside its own frame")          # CHECK, :308
            f2 = sess.frames[ref[0]]
            if f2.poses is None:
                raise CreateTracksError("a match into a frame without poses")    # CHECK, :310
            o2 = f2.obs[ref[1]]
            if o2.has_track:
                continue
            good, pt = geom.tri(sess, fk, ok, j)
            if not good:
                continue
            o.track = len(sess.tracks)
            sess.tracks.append(Track(obs=[], pt=[float(v) for v in pt], valid=False))
            t = sess.tracks[-1]
            o2.track = o.track
            ref[2] = True
            t.obs.append(list(ref))
            t.obs.append([fk, ok, True])
            t.valid = len(t.obs) >= opt.min_reprojections
            o.has_track = o2.has_track = True
            reproject_matches(sess, fk, ok, opt, geom)


def eval_tracks(sess, fk, opt, geom):
    """VideoSfMHandler.cc:377-410, as written: an observation whose track point validate ACCEPTS (:389) leaves its track."""
    f = sess.frames[fk]
    for oi, o in enumerate(f.obs):
        if not o.has_track:
            continue
        t = sess.tracks[o.track]
        if geom.validate(sess, fk, oi, t.pt):
            o.has_track = False
            for i, r in enumerate(t.obs):
                if r[0] == fk and r[1] == oi:
                    del t.obs[i]
                    if t.valid and len(t.obs) < opt.min_reprojections:
                        t.valid = False
                    break


# ---- geometry -------------------------------------------------------------------------------------------------------------

def frame_cam(sess, f):
    fr = sess.frames[f]
    return np.asarray(fr.cam if fr.cam is not None else sess.cam, dtype=np.float64)


def get_pose(O, sess, f, xy, opt):
    """struct/VideoSfM.cc:103-133, through the oracle: one pose, interpolate_rs for two, the scan line's pose for more"""
    if not sess.frames[f].poses:
        raise CreateTracksError("empty frame")
    ps = np.asarray(sess.frames[f].poses, dtype=np.float64).reshape(-1, 6)
    if len(ps) == 1:
        return ps[0].copy()
    if len(ps) == 2:
        return O.interpolate_rs(ps[0], ps[1], sess.rs, sess.scanlines, np.asarray(xy, dtype=np.float64), opt.interpolate_rotation)
    return ps[O.scanline_pose_index(len(ps), sess.rs, np.asarray(xy, dtype=np.float64))].copy()


class OracleGeometry:
    """The predicates composed from the CPU oracle's scalar restatements (oracle/rsba_oracle_math.hpp)."""

    def __init__(self, O, opt):
        self.O, self.opt = O, opt
        self.calls = 0

    def _obs(self, sess, f, k):
        o = sess.frames[f].obs[k]
        xy = np.array([o.x, o.y])
        return xy, frame_cam(sess, f), get_pose(self.O, sess, f, xy, self.opt)

    def reproj(self, sess, fk, ok, j, pt):
        self.calls += 1
        xy, cam, pose = self._obs(sess, fk, ok)
        X = np.asarray(pt, dtype=np.float64)
        return self.O.norm3(pose[3:] - X) >= self.opt.min_distance and self.O.validate(cam, pose, xy, X, self.opt.sqrd_threshold)

    def validate(self, sess, fk, ok, pt):
        return self.reproj(sess, fk, ok, None, pt)

    def tri(self, sess, fk, ok, j):
        O, opt = self.O, self.opt
        ref = sess.frames[fk].obs[ok].matches[j]
        xy, cam, pose = self._obs(sess, fk, ok)
        xy2, cam2, pose2 = self._obs(sess, ref[0], ref[1])
        if pose.tobytes() == pose2.tobytes():                      # memcmp (:321)
            return False, None
        ok1, d1 = O.direction_pixel(cam, pose, xy)
        ok2, d2 = O.direction_pixel(cam2, pose2, xy2)
        if not (ok1 and ok2):
            return False, None
        good, pt = O.triangulate(pose[3:], d1, pose2[3:], d2)
        if not good:
            return False, None
        if O.norm3(pose[3:] - pt) < opt.min_distance or O.norm3(pose2[3:] - pt) < opt.min_distance:
            return False, pt
        return (O.validate(cam, pose, xy, pt, opt.sqrd_threshold) and O.validate(cam2, pose2, xy2, pt, opt.sqrd_threshold)), pt


class TableGeometry:
    """Given flags: tables[frame] = (tri [n], reproj [n], pt [n, 3]) in TrackFlags order; 2 = not computed (raises LookupError),
    3 = the predicate needs the pose of a frame without poses (raises "empty frame", as getPose does)."""

    def __init__(self, sess, tables, validate=None):
        self.tables = tables
        self.off = {f: ref_offsets(sess.frames[f]) for f in tables}
        self.valid_table = validate

    def _flag(self, v, what):
        if v == 3:
            raise CreateTracksError("empty frame")
        if v > 1:
            raise LookupError(f"the {what} flag of a candidate the replay reached was not computed")
        return bool(v)

    def reproj(self, sess, fk, ok, j, pt):
        return self._flag(self.tables[fk][1][self.off[fk][ok] + j], "reprojection")

    def tri(self, sess, fk, ok, j):
        e = self.off[fk][ok] + j
        return self._flag(self.tables[fk][0][e], "triangulation"), self.tables[fk][2][e]

    def validate(self, sess, fk, ok, pt):
        return bool(self.valid_table[fk][ok])


# ---- files shared with examples/create_tracks.cpp -------------------------------------------------------------------------

def to_cache(sess, T):
    """Thrift cache bytes of a Session (T = tests/thrift_encode)"""
    frames = []
    for fr in sess.frames:
        obs = [T.observation(o.x, o.y, track=o.track if o.has_track else None,
                             matches=[tuple(m) for m in o.matches] if o.matches is not None else None) for o in fr.obs]
        frames.append(T.frame(obs, poses=fr.poses, cam=fr.cam))
    tracks = [T.track([tuple(r) for r in t.obs], pt=t.pt, valid=t.valid) for t in sess.tracks]
    return T.file_events(T.session(sess.cam, frames, tracks, sess.rs, list(sess.scanlines), 1280, 720), np.random.default_rng(1), max_event=4096)


def write_flags(path, sess, tables, first, last):
    with open(path, "wb") as g:
        for f in range(first, last + 1):
            tri, rep, pt = tables[f]
            g.write(struct.pack("<q", len(tri)))
            for e in range(len(tri)):
                g.write(struct.pack("<qq3d", int(tri[e]), int(rep[e]), *[float(v) for v in pt[e]]))


def read_state(path):
    """The state examples/create_tracks.cpp writes -> (poses per frame, per-frame [(track, has_track, [ref valid])], tracks)"""
    buf = open(path, "rb").read()
    pos = 0

    def q():
        nonlocal pos
        v = struct.unpack_from("<q", buf, pos)[0]; pos += 8; return v

    def d(n):
        nonlocal pos
        v = struct.unpack_from(f"<{n}d", buf, pos); pos += 8 * n; return list(v)
    poses, frames, tracks = [], [], []
    for _ in range(q()):
        np_ = q()
        poses.append([d(6) for _ in range(np_)])
        obs = []
        for _ in range(q()):
            tr, has = q(), q()
            obs.append((tr, bool(has), [bool(q()) for _ in range(q())]))
        frames.append(obs)
    for _ in range(q()):
        pt = d(3); valid = bool(q())
        tracks.append((pt, valid, [[q(), q(), bool(q())] for _ in range(q())]))
    assert pos == len(buf)
    return poses, frames, tracks


def state_of(sess):
    """The same tuple for a Python Session (points as floats; missing points as zeros)"""
    frames = [[(o.track, o.has_track, [bool(m[2]) for m in (o.matches or [])]) for o in fr.obs] for fr in sess.frames]
    tracks = [([float(v) for v in t.pt] if t.pt is not None else [0.0, 0.0, 0.0], bool(t.valid), [[int(r[0]), int(r[1]), bool(r[2])] for r in t.obs])
              for t in sess.tracks]
    return frames, tracks


def clone(sess):
    return copy.deepcopy(sess)
