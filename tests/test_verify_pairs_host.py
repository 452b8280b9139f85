"""The host side of the geometric verification (include/rsba/two_view.hpp: findEssentialRansacPairs with hypotheses_on_device = false,
verifyMatches, pickBootstrapPair) through tests/verify_pairs_host.cpp: host definitions only, no device, nothing of the library linked —
the program defines the batched entry point itself and ends if the host path ever reaches it."""
import subprocess

import pytest

import verify_pairs_common as V
from helpers import build_host_program


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("verify_pairs_host")
    return build_host_program("verify_pairs_host", d), d


def run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def pairs():
    small = V.small_pairs()
    return small[:6] + [V.short_pair()] + small[6:] + V.outlier_pairs()[:1]


@pytest.mark.parametrize("solver", [8, 5])
def test_pairs_from_the_host_definitions_equal_host_ransac_per_pair(host, pairs, solver):
    """every line the two print is the same text (%.17g: the same doubles); the list has a pair of 7 in the middle, the two pairs no
    hypothesis accepts, and one outlier scene that takes refits"""
    exe, d = host
    path = d / "pairs.bin"
    V.write_pairs_file(path, pairs)
    batched = run(exe, "pairs", path, "pairs", *V.option_args(V.OPTIONS, solver))
    single = run(exe, "pairs", path, "single", *V.option_args(V.OPTIONS, solver))
    assert batched == single
    res = V.parse_results(batched, len(pairs))
    by_name = {p["name"]: r for p, r in zip(pairs, res)}
    assert by_name["seven"]["winner_task"] == -1 and not by_name["seven"]["mask"].any() and len(by_name["seven"]["mask"]) == 7
    assert by_name["pure_rotation"]["winner_task"] == -1 and by_name["coincident"]["winner_task"] == -1
    assert by_name["main_pinhole"]["ok"] and by_name["two_cameras"]["ok"] and by_name["frames_0_1_global"]["ok"]
    assert len({r["winner_task"] for r in res}) > 3


def test_the_sparse_pair_keeps_a_winner_below_the_refit_size(host):
    """the pair the device tests use for the compaction of a pair under the refit size with a non-zero count: with five-point subsets the
    host loop's winner keeps 5, 6 or 7 inliers, so no refit is tried (seed V.SPARSE_SEED; checked here, not assumed)"""
    exe, d = host
    path = d / "sparse.bin"
    sparse = V.sparse_pair()
    assert 8 <= len(sparse["xy_a"]) <= 12
    V.write_pairs_file(path, [sparse])
    r = V.parse_results(run(exe, "pairs", path, "single", *V.option_args(V.OPTIONS, 5)), 1)[0]
    print(f"sparse pair, m = 5: winner {r['winner_task']}, {r['num_inliers']} inliers, {r['refits_adopted']} refits adopted")
    assert r["winner_task"] >= 0 and 5 <= r["num_inliers"] <= 7 and r["refits_adopted"] == 0
    assert int(r["mask"].sum()) == r["num_inliers"]


@pytest.fixture(scope="module")
def session():
    return V.SmallSession()


@pytest.mark.parametrize("drop", [0, 1])
def test_verify_matches_erases_what_the_pair_masks_flag(host, session, drop):
    """the refs left are exactly those the per-pair host_ransac masks keep (pairs assembled here, in the order the header states); `removed`
    per pair; the pair under 8 correspondences untouched, or gone with drop_unverified; nothing but the match lists changes"""
    exe, d = host
    spath, ppath = d / "session.bin", d / "session_pairs.bin"
    session.write_plain(spath)
    found = session.pairs()
    assert list(found) == [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3), (2, 4), (3, 4)] and len(found[(0, 3)]) == 5
    V.write_pairs_file(ppath, [session.pair_arrays(fa, fb, refs) for (fa, fb), refs in found.items()])
    per_pair = V.parse_results(run(exe, "pairs", ppath, "single", *V.option_args(V.OPTIONS, 8)), len(found))
    reports, bootstrap, left, untouched = V.parse_session_output(run(exe, "session", spath, drop, *V.option_args(V.OPTIONS, 8)))
    want_left, want_removed = session.expected(per_pair, V.OPTIONS["min_inliers"], bool(drop))
    assert untouched is True
    assert [(r["frameA"], r["frameB"]) for r in reports] == list(found)
    assert [r["correspondences"] for r in reports] == [len(v) for v in found.values()]
    assert [r["ok"] for r in reports] == [p["ok"] for p in per_pair] and [r["num_front"] for r in reports] == [p["num_front"] for p in per_pair]
    assert all((r["E"] == p["E"]).all() and (r["pose"] == p["pose"]).all() for r, p in zip(reports, per_pair))
    assert [r["removed"] for r in reports] == want_removed
    assert left == want_left
    # the seeded wrong refs are what goes, and the right ones stay: every pair of 8 or more is ok on this scene
    few = reports[3]
    assert few["correspondences"] == 5 and not few["ok"] and few["removed"] == (5 if drop else 0)
    assert all(r["ok"] for k, r in enumerate(reports) if k != 3)
    wrong = {(fb, oi, session.frames[fb][oi]["matches"][s]) for fb in range(5) for oi, o in enumerate(session.frames[fb]) for s in o["wrong"]}
    left_set = {(fb, oi, m) for (fb, oi), ms in left.items() for m in ms}
    # (an epipolar test cannot flag a wrong ref whose point happens to lie within the threshold of the epipolar line, so "most", not "all":
    # this only says that the seeded refs are the kind the step exists for; the exact statement is `left == want_left` above)
    total = sum(len(o["matches"]) for fr in session.frames for o in fr)
    print(f"drop={drop}: {len(wrong)} seeded wrong refs, {len(wrong & left_set)} of them left; {total - len(left_set)} of {total} refs erased")
    assert len(wrong) >= 40 and len(wrong & left_set) <= 0.25 * len(wrong)
    assert len(left_set) >= 0.9 * (total - len(wrong) - 5)
    best = max((k for k, r in enumerate(reports) if r["ok"]), key=lambda k: (reports[k]["num_front"], -reports[k]["frameB"], -reports[k]["frameA"]))
    assert bootstrap == best


def test_pick_bootstrap_pair_tie_rules(host):
    exe, _ = host
    pick = lambda *rows: int(run(exe, "pick", *[v for row in rows for v in row]))
    assert pick() == -1
    assert pick((0, 1, 0, 500), (1, 2, 0, 700)) == -1                                  # none ok
    assert pick((0, 1, 1, 100), (0, 2, 0, 900), (1, 2, 1, 300)) == 2                   # the most in front among the ok ones
    assert pick((2, 3, 1, 300), (1, 2, 1, 300), (0, 3, 1, 300)) == 1                   # a tie: the lowest frameB
    assert pick((2, 3, 1, 300), (1, 3, 1, 300), (0, 4, 1, 300)) == 1                   # then the lowest frameA
    assert pick((1, 3, 1, 300), (1, 3, 1, 300)) == 0                                   # the first of two equal reports
