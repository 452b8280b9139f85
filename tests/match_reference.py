"""A Python restatement of rsba's descriptor matching, for the tests: VideoSfMClient::Match (VideoSfMClient.cc:73-129, with
calc2Ddist :57-69) and the matching loop of parseFrame (:196-201, convertCV struct/VideoSfM.cc:48-54), written from their
meaning.  The neighbour search is cv::BFMatcher().knnMatch with NORM_L2 as include/rsba_amd.h defines it:
distance = sqrtf(float(sum (q - t)^2)), ascending, ties to the lower train index, k' = min(k, n_train); a pair with n_train < 2
or n_query == 0 yields nothing.

knn_int   integer descriptors: the sums in int64, np.sqrt(np.float32(d2))                     (the bit-exact contract)
d2_f64    any finite descriptors: squared distances in float64 (for the tolerance checks)
"""
from __future__ import annotations

import numpy as np

RATIO = np.float32(0.80)


def knn_int(q, t, k):
    """-> index [nq, k] int32 (-1 unused), distance [nq, k] float32 (+inf unused), count [nq] int32"""
    q = np.asarray(q); t = np.asarray(t)
    qi = q.astype(np.int64); ti = t.astype(np.int64)
    assert np.array_equal(qi, q) and np.array_equal(ti, t), "knn_int is for integer-valued descriptors"
    nq, nt = len(qi), len(ti)
    idx = np.full((nq, k), -1, dtype=np.int32); dist = np.full((nq, k), np.inf, dtype=np.float32); cnt = np.zeros(nq, dtype=np.int32)
    if nq == 0 or nt < 2:
        return idx, dist, cnt
    kk = min(k, nt)
    d2 = (qi * qi).sum(1)[:, None] + (ti * ti).sum(1)[None, :] - 2 * (qi @ ti.T)       # exact in int64
    d = np.sqrt(d2.astype(np.float32))                                                  # float32 sqrt: correctly rounded
    order = np.lexsort((np.broadcast_to(np.arange(nt), d.shape), d), axis=1)[:, :kk]   # by (distance, index)
    idx[:, :kk] = order
    dist[:, :kk] = np.take_along_axis(d, order, 1)
    cnt[:] = kk
    return idx, dist, cnt


def d2_f64(q, t):
    q = np.asarray(q, dtype=np.float64); t = np.asarray(t, dtype=np.float64)
    return ((q[:, None, :] - t[None, :, :]) ** 2).sum(2)


def dist2d(pq, pt):
    """calc2Ddist: the subtraction in float (cv::Point2f), the rest in double"""
    fx = np.float32(pq[0]) - np.float32(pt[0]); fy = np.float32(pq[1]) - np.float32(pt[1])
    dx = float(fx); dy = float(fy)
    return float(np.sqrt(np.float64(dx * dx + dy * dy)))


def filter_matches(idx, dist, cnt, xy_q, xy_t, multiple=False):
    """The filter of Match (:85-128) -> [(queryIdx, trainIdx)] in query order, then neighbour order"""
    nq = len(idx)
    if nq == 0 or np.any(np.asarray(cnt) < 2):
        return []
    l2 = [dist2d(xy_q[i], xy_t[idx[i][0]]) for i in range(nq)]
    s = 0.0
    for v in l2:                       # std::accumulate: sequential, in double
        s += v
    mean = s / nq
    thr = mean + mean
    good = []
    for i in range(nq):
        d0, d1 = np.float32(dist[i][0]), np.float32(dist[i][1])
        bound = RATIO * d1             # float product
        if multiple:
            if l2[i] < thr:
                good.append((i, int(idx[i][0])))
            for n in range(1, int(cnt[i])):
                if d0 > bound and dist2d(xy_q[i], xy_t[idx[i][n]]) < thr:
                    good.append((i, int(idx[i][n])))
        else:
            if d0 < bound and l2[i] < thr:
                good.append((i, int(idx[i][0])))
    return good


def match(desc_q, desc_t, xy_q, xy_t, multiple=False, knn=knn_int):
    idx, dist, cnt = knn(desc_q, desc_t, 5 if multiple else 2)
    return filter_matches(idx, dist, cnt, xy_q, xy_t, multiple)


def frame_pairs(frame_key, max_frames_to_match=5):
    return [(frame_key, frame_key - i) for i in range(1, min(frame_key, max_frames_to_match) + 1)]


def match_session(descs, xys, max_frames_to_match=5, multiple=False, knn=knn_int):
    """parseFrame's loop for frameKey = 1 .. F - 1 -> per frame, per observation, the list of [frame, obs] in the order appended"""
    out = [[[] for _ in range(len(d))] for d in descs]
    for fk in range(1, len(descs)):
        for q, t in frame_pairs(fk, max_frames_to_match):
            for qi, ti in match(descs[q], descs[t], xys[q], xys[t], multiple, knn):
                out[fk][qi].append([t, ti])
    return out


def shared_root_rows():
    """Two train rows whose integer squared distances to the zero query differ by one yet share a rounded float32 root, the
    LARGER one at the lower index: the order is by the root, so that one comes first.  -> (q [1, 128], t [2, 128])"""
    two = (np.arange(256)[:, None] ** 2 + np.arange(256)[None, :] ** 2)
    base = 124 * 255 * 255
    for n in range(base + 100000, base + 101000):
        if np.sqrt(np.float32(n)) != np.sqrt(np.float32(n + 1)):
            continue
        rows = []
        for m in (n + 1 - base, n - base):
            hit = np.argwhere(np.isin(m - two, two))
            if not len(hit):
                break
            x1, x2 = hit[0]
            x3, x4 = np.argwhere(two == m - two[x1, x2])[0]
            r = np.full(128, 255.0, dtype=np.float32); r[:4] = [x1, x2, x3, x4]
            rows.append(r)
        if len(rows) == 2:
            return np.zeros((1, 128), dtype=np.float32), np.stack(rows)
    raise AssertionError("no such pair found")
