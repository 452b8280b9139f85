"""The exact reduced solve against the iterative one (rsba_set_linear_solver type 1), same box, same run: wall time per LM
iteration, the device time of the "reduced solve" phase (RSBA_PHASE_CHOLESKY, HIP events of options.profile_phases) and the
conjugate-gradient iterations per LM step, at eta = 0.1 and at a tight residual tolerance.

usage: python tools/pcg_time.py [C2 C4 C5] [--iters 12] [--json out.json]

Every variant runs the LM loop in the form where the host decides (profile_phases does that for the exact solver too), so the
three rows differ in the linear solver alone; the exact solver's production loop (no host wait) is what bench.py measures.
ms/iteration is the wall time of the second of two solves from the same start over its LM iterations."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsba_amd import capi  # noqa: E402
from rsba_amd.scene import make_config  # noqa: E402

VARIANTS = [("exact", dict(type=0)), ("pcg eta=0.1", dict(type=1, eta=0.1)), ("pcg r_tol=1e-10", dict(type=1, eta=0.0, r_tolerance=1e-10, max_iterations=5000))]


def measure(name, iters):
    prob = make_config(name).problem
    p0, x0, c0 = prob.poses.copy(), prob.points.copy(), prob.intrinsics.copy()
    rows = []
    with capi.DeviceProblem(prob) as dp:
        plan = dp.plan_stats()
        for label, kw in VARIANTS:
            dp.set_linear_solver(**kw)
            for rep in range(2):
                prob.poses[...] = p0; prob.points[...] = x0; prob.intrinsics[...] = c0
                dp.upload_parameters()
                t = time.perf_counter()
                s, tr = dp.solve(capi.default_options(max_num_iterations=iters, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0, profile_phases=1))
                wall = time.perf_counter() - t
            ph, ls = dp.phase_times(), dp.linear_solver_stats()
            n = max(1, s.num_iterations - 1)
            chol_ms, chol_calls = ph["cholesky"] if "cholesky" in ph else next(v for k, v in ph.items() if "chol" in k.lower())
            rows.append(dict(config=name, solver=label, lm_iterations=n, final_cost=s.final_cost, ms_per_iteration=1e3 * wall / n,
                             reduced_solve_ms=chol_ms / max(1, chol_calls), linear_solves=int(ls["num_linear_solves"]),
                             cg_iterations_per_solve=ls["total_iterations"] / max(1, ls["num_linear_solves"]), cg_max=int(ls["max_iterations"]),
                             solves_at_cap=int(ls["num_solves_at_cap"]), failed_solves=int(ls["num_failed_solves"]),
                             tiles=plan["tiles"], factor_tiles=plan["factor_tiles"],
                             spmv_bytes_per_cg_iteration=plan["factor_tiles"] * 48 * 48 * 8))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C2", "C4", "C5"])
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = []
    for name in a.configs:
        rows = measure(name, a.iters)
        out += rows
        for r in rows:
            cg_ms = r["reduced_solve_ms"] / r["cg_iterations_per_solve"] if r["cg_iterations_per_solve"] else float("nan")
            print(f"{r['config']:3s} {r['solver']:16s} {r['ms_per_iteration']:8.3f} ms/LM iteration  reduced solve {r['reduced_solve_ms']:8.3f} ms  "
                  f"CG/step {r['cg_iterations_per_solve']:7.1f} (max {r['cg_max']}, at cap {r['solves_at_cap']}, failed {r['failed_solves']})  "
                  f"ms/CG iteration {cg_ms:6.4f}  final cost {r['final_cost']:.9e}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
