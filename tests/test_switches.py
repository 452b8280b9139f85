"""The RSBA_* environment switches (rsba_amd/csrc/switches.hpp): what every parse rule makes of a value, checked on
tests/switches_host.cpp — a host program that prints every field of PlanSwitches / SolveSwitches and chol_leaf_override() for the
environment it is started in, compiled here without and with -DRSBA_TEST_HOOKS — and that the header, the hook call sites and README.md's
table name the same variables.  No GPU, nothing of the library is loaded.

The rules (README.md, "Environment switches"): an on-by-default feature goes off on a leading '0' only; an off-by-default one goes on on a
leading '1' only; RSBA_NO_FUSED_SWEEP, RSBA_NO_SIDE_SWEEP, RSBA_PLAN_LISTED_KEYS, RSBA_DEBUG_PLAN and the trace paths count as set whatever
their value; numbers are clamped per switch."""
import json
import os
import re
import subprocess

import pytest

from helpers import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rsba_amd", "csrc")
RING = 4   # what the program is told the LM control ring holds (the library passes Solver::kCtlRing): RSBA_LM_AHEAD is capped at RING - 2
HOOKS = {"RSBA_TEST_FAIL_PLAN": "1", "RSBA_TEST_FAIL_DEVICE_PLAN": "1", "RSBA_CHOL_TEST_CORRUPT": "1", "RSBA_DEVICE_LM_OFF_ON_THIS_RANK": "1"}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return {False: build_host_program("switches_host", tmp_path_factory.mktemp("switches")),
            True: build_host_program("switches_host", tmp_path_factory.mktemp("switches_hooks"), extra_flags=("-DRSBA_TEST_HOOKS",))}


@pytest.fixture(scope="module")
def read(programs):
    def run(env=None, hooks=False, ring=RING):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("RSBA_")}
        clean.update(env or {})
        return json.loads(subprocess.run([programs[hooks], str(ring)], env=clean, check=True, capture_output=True, text=True).stdout)
    return run


def test_defaults_with_everything_unset(read):
    r = read()
    assert r["test_hooks"] is False
    assert r["plan"] == {
        "plan_threads": None, "keep_records": False, "records_alt": True, "factored": True, "plan_device": True, "listed_keys": False,
        "schur_block": r["schur_block_unset"], "schur_linear": False, "schur_variant": 0, "schur_trace": None, "sharded": True,
        "chol_fuse": r["chol_plan_options"]["fuse_last"], "chol_tail": r["chol_plan_options"]["tail"], "chol_chunk": r["chol_plan_options"]["chunk"],
        "chol_wgs": None, "chol_verify": True, "chol_levels_before_solve": False, "chol_trace": None, "no_fused_sweep": False, "debug_plan": False,
        "test_fail_plan": False, "test_fail_device_plan": False, "test_chol_corrupt": False}
    assert r["chol_plan_options"] == {"chunk": 12, "tail": 2, "fuse_last": True}   # (what the plan has used so far)
    assert r["schur_block_unset"] < 0 and r["schur_pair_major"] == 0                # three states: unset / pair-major / >= 16 points
    assert r["solve"] == {"device_lm": True, "lm_ahead": 0, "speculate": True, "chol_levels": False, "no_side_sweep": False, "test_device_lm_off_on_this_rank": False}
    assert r["chol_leaf_override"] is None and r["debug_plan"] is False
    assert r["process"] == {"sweep_points_override": 0, "project_chunks_override": 0, "cov_times": False, "device_cache_mb": 2048, "rccl_lib": None}


# one list per parse rule: (variable, where the program prints its field)
ON_UNLESS_0 = [("RSBA_FACTORED", ("plan", "factored")), ("RSBA_PLAN_DEVICE", ("plan", "plan_device")), ("RSBA_SHARDED", ("plan", "sharded")),
               ("RSBA_CHOL_FUSE", ("plan", "chol_fuse")), ("RSBA_CHOL_VERIFY", ("plan", "chol_verify")), ("RSBA_RECORDS_ALT", ("plan", "records_alt")),
               ("RSBA_SPECULATE", ("solve", "speculate")), ("RSBA_DEVICE_LM", ("solve", "device_lm"))]
OFF_UNLESS_1 = [("RSBA_CHOL_LEVELS", ("plan", "chol_levels_before_solve")), ("RSBA_CHOL_LEVELS", ("solve", "chol_levels")), ("RSBA_SCHUR_LINEAR", ("plan", "schur_linear")),
                ("RSBA_COV_TIMES", ("process", "cov_times")), ("RSBA_RECORDS", ("plan", "keep_records"))]
PRESENCE = [("RSBA_NO_FUSED_SWEEP", ("plan", "no_fused_sweep")), ("RSBA_PLAN_LISTED_KEYS", ("plan", "listed_keys")), ("RSBA_DEBUG_PLAN", ("plan", "debug_plan")),
            ("RSBA_NO_SIDE_SWEEP", ("solve", "no_side_sweep"))]


@pytest.mark.parametrize("rule, table, expect", [("on unless 0", ON_UNLESS_0, {"0": False, "1": True, "": True, "00": False, "no": True}),
                                                  ("off unless 1", OFF_UNLESS_1, {"0": False, "1": True, "": False, "10": True, "yes": False}),
                                                  ("presence", PRESENCE, {"0": True, "1": True, "": True})], ids=["on-unless-0", "off-unless-1", "presence"])
def test_the_flag_rules(read, rule, table, expect):
    for name, (group, field) in table:
        for value, want in expect.items():
            assert read({name: value})[group][field] is want, (rule, name, value)


def test_records_0_against_1(read):
    assert read({"RSBA_RECORDS": "0"})["plan"]["keep_records"] is False   # ("0" keeps the recomputation, like unset)
    assert read({"RSBA_RECORDS": "1"})["plan"]["keep_records"] is True


def test_debug_plan_outside_a_solver_is_the_same_switch(read):
    assert read({"RSBA_DEBUG_PLAN": "0"})["debug_plan"] is True


def test_the_numbers_and_their_clamps(read):
    pm = read()["schur_pair_major"]
    for value, want in (("0", pm), ("-3", pm), ("x", pm), ("5", 16), ("16", 16), ("4096", 4096)):
        assert read({"RSBA_SCHUR_BLOCK": value})["plan"]["schur_block"] == want, value
    for value, want in (("0", 1), ("999", 64), ("7", 7)):
        assert read({"RSBA_PLAN_THREADS": value})["plan"]["plan_threads"] == want, value
    r = read({"RSBA_CHOL_TAIL": "3", "RSBA_CHOL_CHUNK": "1"})["plan"]
    assert (r["chol_tail"], r["chol_chunk"]) == (3, 3)
    r = read({"RSBA_CHOL_TAIL": "0", "RSBA_CHOL_CHUNK": "20"})["plan"]
    assert (r["chol_tail"], r["chol_chunk"]) == (1, 20)
    r = read({"RSBA_CHOL_TAIL": "20"})["plan"]                 # (the chunk's default is not raised to the tail: as the plan has parsed it so far)
    assert (r["chol_tail"], r["chol_chunk"]) == (20, 12)
    assert read({"RSBA_CHOL_CHUNK": "1"})["plan"]["chol_chunk"] == 2
    for value, want in (("-1", 0), ("99", RING - 2), ("1", 1)):
        assert read({"RSBA_LM_AHEAD": value})["solve"]["lm_ahead"] == want, value
    assert read({"RSBA_LM_AHEAD": "99"}, ring=8)["solve"]["lm_ahead"] == 6
    for value, want in (("1", 2), ("2", 2), ("24", 24)):
        assert read({"RSBA_CHOL_LEAF": value})["chol_leaf_override"] == want, value
    assert read({"RSBA_CHOL_WGS": "-5"})["plan"]["chol_wgs"] == -5   # (the plan clamps it: to its tasks and two per CU)
    assert read({"RSBA_SCHUR_VARIANT": "2"})["plan"]["schur_variant"] == 2
    for value, want in (("0", 0), ("4", 4), ("16", 16), ("17", 0)):
        assert read({"RSBA_SWEEP_POINTS": value})["process"]["sweep_points_override"] == want, value
    for value, want in (("0", 0), ("64", 64), ("65", 0)):
        assert read({"RSBA_PROJECT_CHUNKS": value})["process"]["project_chunks_override"] == want, value
    assert read({"RSBA_DEVICE_CACHE_MB": "0"})["process"]["device_cache_mb"] == 0
    assert read({"RSBA_DEVICE_CACHE_MB": "512"})["process"]["device_cache_mb"] == 512


def test_the_paths(read):
    r = read({"RSBA_SCHUR_TRACE": "/tmp/s.bin", "RSBA_CHOL_TRACE": "", "RSBA_RCCL_LIB": "libmock.so"})
    assert r["plan"]["schur_trace"] == "/tmp/s.bin" and r["plan"]["chol_trace"] == "" and r["process"]["rccl_lib"] == "libmock.so"   # (an empty path still switches the trace on)


def test_the_release_build_reads_no_hook(read):
    """Without RSBA_TEST_HOOKS the four fault-injection variables and the Schur ablations change nothing; with it they are read."""
    env = dict(HOOKS, RSBA_SCHUR_VARIANT="5")
    assert read(env) == read()
    r = read(env, hooks=True)
    assert r["test_hooks"] is True
    assert r["plan"]["test_fail_plan"] and r["plan"]["test_fail_device_plan"] and r["plan"]["test_chol_corrupt"] and r["solve"]["test_device_lm_off_on_this_rank"]
    assert r["plan"]["schur_variant"] == 5
    assert read({"RSBA_CHOL_TEST_CORRUPT": "0"}, hooks=True)["plan"]["test_chol_corrupt"] is False
    base = read(hooks=True)
    assert not any(base["plan"][k] for k in ("test_fail_plan", "test_fail_device_plan", "test_chol_corrupt")) and not base["solve"]["test_device_lm_off_on_this_rank"]


def _literals(text):
    return set(re.findall(r'"(RSBA_[A-Z0-9_]+)"', text))


def test_code_and_readme_agree():
    """The names in switches.hpp and at the test_hook() call sites are the names of README.md's table; nothing else under
    rsba_amd/csrc reads the environment."""
    sources = {f: open(os.path.join(CSRC, f), encoding="utf-8").read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    in_code = _literals(sources["switches.hpp"])
    for text in sources.values():
        in_code |= set(re.findall(r'test_hook\(\s*"(RSBA_[A-Z0-9_]+)"', text))
    readme = open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()
    section = readme[readme.index("### Environment switches"):]
    in_table = set(re.findall(r"^\| `(RSBA_[A-Z0-9_]+)` \|", section, flags=re.M))
    assert in_code == in_table, (sorted(in_code - in_table), sorted(in_table - in_code))
    assert set(HOOKS) <= in_code
    assert [f for f, text in sources.items() if "getenv" in text] == ["switches.hpp", "test_hooks.hpp"]
