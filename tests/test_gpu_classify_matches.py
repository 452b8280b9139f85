"""classifyMatches on the device through examples/classify_pairs: a session of 5 frames over one cloud (homography_reference.classify_session),
every later frame matched into frame 0 with seeded wrong refs, written as a session cache by tests/thrift_encode.py.  Frames 0-1 differ by
a baseline of a per cent of the depth, frames 0-4 by 0.3 of it: the plain pick takes the pair without a baseline, the pick with the
geometry the wide one; the classification leaves the session's matches as they are."""
import os
import subprocess

import pytest

import homography_reference as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example():
    import __graft_entry__ as G
    path = os.path.join(ROOT, "examples", "classify_pairs")
    if not os.path.exists(path):
        G.build()
    return path


def check(rows, pick, untouched):
    assert [(r["frameA"], r["frameB"]) for r in rows] == [(0, 1), (0, 2), (0, 3), (0, 4)]
    assert all(r["ok"] for r in rows)
    for r in rows:
        print(r)
    assert [r["kind"] for r in rows] == ["LowParallax", "LowParallax", "LowParallax", "General"]
    assert rows[0]["num_h_inliers"] > 0.8 * rows[0]["num_inliers"] and rows[3]["num_h_inliers"] < 0.8 * rows[3]["num_inliers"]
    assert rows[3]["num_parallax"] > 0.9 * rows[3]["num_front"] and all(2 * r["num_parallax"] < r["num_front"] for r in rows[:3])
    # after the erasure every remaining ref is an inlier of the pair's E: the call forms that mask itself and finds the same inliers
    assert all(r["num_front"] == r["essential_front"] for r in rows)
    assert rows[0]["essential_front"] > max(r["essential_front"] for r in rows[1:])
    assert pick == [0, 3]
    assert untouched


def run_session(example, tmp_path, *extra):
    s = H.classify_session()
    (tmp_path / "s.cache").write_bytes(H.session_cache_bytes(s))
    o = H.CLASSIFY
    r = subprocess.run([example, str(tmp_path / "s.cache"), f"iterations={o['iterations']}", f"threshold={o['threshold_px']}", f"refits={o['refits']}", f"minInliers={o['min_inliers']}",
                        f"seed={o['rng_state']}", f"minParallaxDeg={o['min_parallax_deg']}", *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return H.parse_classify_output(r.stdout)


def test_kinds_and_both_picks(example, tmp_path):
    check(*run_session(example, tmp_path))


def test_a_few_pairs_per_launch_print_the_same(example, tmp_path):
    assert run_session(example, tmp_path, "maxTasks=450") == run_session(example, tmp_path)


def test_allow_planar_and_the_default_angle(example, tmp_path):
    """at the default 16 degrees no pair of this session has parallax: no pick with the geometry"""
    rows, pick, untouched = run_session(example, tmp_path, "minParallaxDeg=16")
    assert [r["kind"] for r in rows[:3]] == ["LowParallax"] * 3 and pick[0] == 0 and untouched
    print(rows[3], pick)
    assert pick[1] in (-1, 3) and (pick[1] == 3) == (rows[3]["kind"] == "General")
