"""classifyMatches and pickBootstrapPair with a geometry on the host path (examples/classify_pairs hostHypotheses=1: both RANSACs and the
parallax counts from the host definitions, no device): the session and the expectations of test_gpu_classify_matches.py."""
import os

import pytest

import test_gpu_classify_matches as G


@pytest.fixture(scope="module")
def example():
    import __graft_entry__ as E
    path = os.path.join(G.ROOT, "examples", "classify_pairs")
    if not os.path.exists(path):
        E.build()
    return path


def test_kinds_and_both_picks_on_the_host_path(example, tmp_path):
    G.check(*G.run_session(example, tmp_path, "hostHypotheses=1"))
