"""CPU-side checks of the drop-in boundary: the library loads and exports every symbol that
include/rsba_amd.h declares; struct mirrors match; no compute is attempted without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as G
    G.build()
    from rsba_amd import capi
    return ctypes.CDLL(capi.LIB_PATH)


def declared_functions():
    src = open(os.path.join(ROOT, "include", "rsba_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rsba_[a-z_0-9]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(built_lib):
    names = declared_functions()
    assert len(names) >= 14
    for n in names:
        assert hasattr(built_lib, n), f"{n} declared in include/rsba_amd.h but not exported"


def test_the_instrumented_library_is_the_same_abi_plus_its_counters(built_lib):
    """rsba_amd/_lib/librsba_amd_hooks.so (-DRSBA_TEST_HOOKS: fault-injection switches, ablation branches, the Cholesky's coherent-read counters) is what
    the fault-injection tests load; the library the product ships has none of it — not even the debug entry point."""
    hooks = ctypes.CDLL(os.path.join(ROOT, "rsba_amd", "_lib", "librsba_amd_hooks.so"))
    for n in declared_functions():
        assert hasattr(hooks, n), n
    assert hasattr(hooks, "rsba_debug_chol_coherent") and not hasattr(built_lib, "rsba_debug_chol_coherent")
    assert hasattr(hooks, "rsba_debug_partition_tiles") and not hasattr(built_lib, "rsba_debug_partition_tiles")


def test_python_binding_lists_the_same_symbols():
    from rsba_amd import capi
    assert sorted(capi.EXPORTS) == declared_functions()


def test_struct_mirrors_have_the_c_sizes(built_lib, tmp_path):
    """ctypes mirrors vs sizeof() as the C compiler sees the header."""
    from rsba_amd import capi
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include "rsba_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(rsba_problem_desc), '
                    'sizeof(rsba_solver_options), sizeof(rsba_iteration), sizeof(rsba_solver_summary), sizeof(rsba_device_view));return 0;}\n')
    exe = tmp_path / "sz"
    import subprocess
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    sizes = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert sizes == [ctypes.sizeof(capi.ProblemDesc), ctypes.sizeof(capi.SolverOptions), ctypes.sizeof(capi.Iteration),
                     ctypes.sizeof(capi.SolverSummary), ctypes.sizeof(capi.DeviceView)]


def test_no_cpu_fallback_without_a_device(built_lib):
    """On a box without a GPU the product must fail loudly, not compute on the CPU."""
    import torch
    from rsba_amd import capi
    from rsba_amd.scene import make_scene
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.RsbaError):
        capi.device_count()
    with pytest.raises(capi.RsbaError):
        capi.DeviceProblem(make_scene(4, 50).problem)


def test_product_never_references_the_oracle():
    """The oracle is test infrastructure: nothing under rsba_amd/ or include/ may mention it."""
    bad = []
    for base in ("rsba_amd", "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            if "_lib" in dp or "__pycache__" in dp:
                continue
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp", "Makefile")):
                    txt = open(os.path.join(dp, f), errors="ignore").read()
                    if re.search(r"\boracle\b", txt) and not f == "__init__.py":
                        # comments saying "no oracle" are fine only in capi docs; be strict: flag imports/includes
                        if re.search(r"(import\s+oracle|from\s+oracle|#include\s+\".*oracle|liboracle)", txt):
                            bad.append(os.path.join(dp, f))
    assert not bad, bad
