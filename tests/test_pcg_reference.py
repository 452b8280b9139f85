"""CPU side of the iterative linear solver's checks: the host reference of tests/pcg_reference.py is a conjugate-gradient solver
(it converges to lm_step's solution, its residuals are M^-1-orthogonal), the constants of tests/test_gpu_pcg.py are what the fp64
restatement's distance from the long-double reference gives, three seeded errors exceed those bounds, and the new entry points
are declared, exported, bound and mirrored with the C compiler's sizes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lm_step_reference as R
import pcg_reference as PR
from test_gpu_pcg import C_ITER, C_PCG, N_CASE, OFF, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD_EPS = 2.0 ** -64
NEW_NAMES = ["rsba_default_linear_solver_options", "rsba_set_linear_solver", "rsba_get_linear_solver_stats"]


@pytest.mark.parametrize("name", ["rs_Fp1", "gs_intr_run3", "rs_spherical_pp"])
def test_long_double_pcg_reaches_the_solution_of_lm_step(oracle, name):
    """Run until the residual is at the long-double floor: the camera-side unknowns of LMStep.y, to 64 kappa 2^-64 (the unit of C_TOL
    in the precision of this reference)."""
    p, opts, ref, red, sm, _ = reference(oracle, name)
    run = PR.pcg(red, eta=0.0, r_tolerance=1e-18, max_iterations=1500)
    assert run.reason == "test", (run.iterations, float(run.rel[-1]))
    yc = np.asarray(ref.y)[red.cam]
    err = float(np.max(np.abs(run.y[-1] - yc)) / np.max(np.abs(yc)))
    print(f"{name}: {run.iterations} iterations, error {err:.3g}, bound {64 * ref.kappa * LD_EPS:.3g}")
    assert err <= 64 * ref.kappa * LD_EPS


def test_residuals_are_orthogonal_in_the_preconditioner(oracle):
    """r_i^T M^-1 r_j = 0 for i != j, as conjugate gradients keep it: the first eight iterates of rs_Fp1 in long double."""
    p, opts, ref, red, sm, _ = reference(oracle, "rs_Fp1")
    run = PR.pcg(red, max_iterations=8, **OFF)
    G = np.array([[float(np.dot(run.r[i], run.z[j])) for j in range(9)] for i in range(9)])
    d = np.sqrt(np.diag(G))
    off = np.abs(G / d[:, None] / d[None, :] - np.eye(9))
    assert off.max() <= 1e-12, off.max()
    assert np.all(np.diff([float(q) for q in run.Q]) < 0)       # and the model value falls with every iteration


@pytest.mark.parametrize("name", ["rs_huber", "rs_intr_shared", "rs_far_pair", "gs_intr_run3"])
def test_the_constants_are_four_times_the_restatement(oracle, name):
    """The fp64 restatement against the long-double reference (early iterates) and against lm_step (N_CASE iterations): a quarter of
    C_ITER and of C_PCG at the most.  rs_huber sets C_ITER, rs_intr_shared is the worst converged case."""
    p, opts, ref, red, sm, run = reference(oracle, name)
    red64 = PR.reduce_system(p, ref, np.float64)
    r64 = PR.pcg(red64, eta=0.0, r_tolerance=0.0, max_iterations=N_CASE[name])
    for k in (1, 2, 3):
        want = sm.step(PR.full_solution(red, ref, run.y[k]))
        got = sm.step(PR.full_solution(red64, ref, r64.y[k]))
        ratio, where = R.step_ratio(p, want, *PR.applied(p, got))
        assert ratio <= C_ITER / 4 * (1 + 1e-9), (k, ratio, where)
    got = sm.step(PR.full_solution(red64, ref, r64.y[-1]))
    ratio, where = R.step_ratio(p, ref, *PR.applied(p, got))
    print(f"{name}: converged restatement {ratio:.3g}")
    assert ratio <= C_PCG / 4, (ratio, where)


def _early_ratio(p, ref, red, sm, good, bad, k):
    want = sm.step(PR.full_solution(red, ref, good.y[k]))
    got = sm.step(PR.full_solution(red, ref, bad.y[k]))
    return R.step_ratio(p, want, *PR.applied(p, got))[0]


@pytest.mark.parametrize("name", ["rs_far_pair", "rs_huber"])
def test_a_dropped_preconditioner_block_exceeds_the_bound(oracle, name):
    """Frame 2's block of M replaced by the identity: every early iterate leaves the bound of test_early_iterates."""
    p, opts, ref, red, sm, run = reference(oracle, name)
    bad = PR.pcg(red, max_iterations=3, drop_block=red.block_frame.index(2), **OFF)
    for k in (1, 2, 3):
        ratio = _early_ratio(p, ref, red, sm, run, bad, k)
        assert ratio > 100 * C_ITER, (k, ratio)


def test_a_missing_transposed_tile_exceeds_the_bounds(oracle):
    """rs_far_pair: tile (4, 0) serves the rows of tile 4 but not, transposed, the rows of tile 0."""
    name = "rs_far_pair"
    p, opts, ref, red, sm, run = reference(oracle, name)
    tiles = red.row // PR.TILE
    assert np.any(red.S[np.ix_(tiles == 0, tiles == 4)] != 0)
    bad = PR.pcg(red, max_iterations=3, drop_transposed=(4, 0), **OFF)
    assert max(_early_ratio(p, ref, red, sm, run, bad, k) for k in (1, 2, 3)) > 100 * C_ITER
    red64 = PR.reduce_system(p, ref, np.float64)
    try:
        conv = PR.pcg(red64, eta=0.0, r_tolerance=0.0, max_iterations=N_CASE[name], drop_transposed=(4, 0))
    except np.linalg.LinAlgError:                # the matrix is no longer symmetric: p.q <= 0 fails the solve, the step is invalid
        return
    got = sm.step(PR.full_solution(red64, ref, conv.y[-1]))
    ratio, where = R.step_ratio(p, ref, *PR.applied(p, got))
    assert ratio > 100 * C_PCG, (ratio, where)


@pytest.mark.parametrize("name", ["rs_far_pair", "rs_Fp1"])
def test_a_stopping_test_one_iteration_late_is_caught(oracle, name):
    """The count differs from the reference's by one although no criterion value is near eta, and the step it returns is not the
    reference's."""
    p, opts, ref, red, sm, _ = reference(oracle, name)
    good, late = PR.pcg(red), PR.pcg(red, stop_late=1)
    assert late.iterations == good.iterations + 1
    assert not any(abs(float(z) - 0.1) <= 1e-7 for z in good.zeta[1:])
    want = sm.step(PR.full_solution(red, ref, good.y[-1]))
    got = sm.step(PR.full_solution(red, ref, late.y[-1]))
    assert R.step_ratio(p, want, *PR.applied(p, got))[0] > 100 * C_ITER


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as G
    G.build()
    from rsba_amd import capi
    return ctypes.CDLL(capi.LIB_PATH)


def test_new_entry_points_are_declared_exported_and_bound(built_lib):
    from rsba_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsba_amd.h")).read(), flags=re.S)
    for n in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(built_lib, n), n
        assert n in capi.EXPORTS, n
    assert re.search(r"#define RSBA_AMD_ABI_VERSION 4\b", src)
    assert hasattr(capi.DeviceProblem, "set_linear_solver") and hasattr(capi.DeviceProblem, "linear_solver_stats")


def test_option_and_stats_mirrors_have_the_c_sizes_and_defaults(built_lib, tmp_path):
    from rsba_amd import capi
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsba_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(rsba_linear_solver_options), '
                    'sizeof(rsba_linear_solver_stats), offsetof(rsba_linear_solver_options, eta), offsetof(rsba_linear_solver_stats, last_relative_residual), '
                    'sizeof(rsba_solver_options), sizeof(rsba_phase_times), RSBA_AMD_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [ctypes.sizeof(capi.LinearSolverOptions), ctypes.sizeof(capi.LinearSolverStats), capi.LinearSolverOptions.eta.offset,
                   capi.LinearSolverStats.last_relative_residual.offset, ctypes.sizeof(capi.SolverOptions), ctypes.sizeof(capi.PhaseTimes), 4]
    o = capi.LinearSolverOptions()
    built_lib.rsba_default_linear_solver_options(ctypes.byref(o))
    assert (o.type, o.min_iterations, o.max_iterations, o.eta, o.r_tolerance) == (0, 1, 500, 0.1, -1.0)
    built_lib.rsba_abi_version.restype = ctypes.c_int32
    assert built_lib.rsba_abi_version() == 4
