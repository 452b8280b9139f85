"""What the loss costs: for each loss on the SAME handle and scene, the marginal milliseconds of one LM iteration (a solve of twice as
many iterations against one of ``iters``, per extra iteration, as tools/lm_time.py) and the HIP-event time of the LM-mode evaluation
(eval_kernel<.., kLmJacobian> + cost reduction: RSBA_PHASE_EVAL_LM and, for the candidates, RSBA_PHASE_EVAL_TRIAL of a solve with
profile_phases = 1) per launch.  "none" and "huber(2)" run the instantiations of old, the others the general ones.
usage: python tools/loss_time.py [C4] [iters] [--json out.json]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsba_amd import capi
from rsba_amd.scene import make_config

args = [a for a in sys.argv[1:] if not a.startswith("--")]
name = args[0] if args else "C4"
iters = int(args[1]) if len(args) > 1 else 12
LOSSES = [("none", dict(type=capi.LOSS_TRIVIAL)), ("huber(2)", dict(type=capi.LOSS_HUBER, a=2.0)), ("huber(2) x 0.5", dict(type=capi.LOSS_HUBER, a=2.0, scale=0.5)),
          ("soft_l_one(10)", dict(type=capi.LOSS_SOFT_L_ONE, a=10.0)), ("cauchy(10)", dict(type=capi.LOSS_CAUCHY, a=10.0)), ("arctan(100)", dict(type=capi.LOSS_ARCTAN, a=100.0)),
          ("tolerant(150, 50)", dict(type=capi.LOSS_TOLERANT, a=150.0, b=50.0))]

prob = make_config(name).problem
prob.huber_a = 0.0
p0, x0, i0 = prob.poses.copy(), prob.points.copy(), prob.intrinsics.copy()
rows = []
with capi.DeviceProblem(prob) as dp:
    def solve(n, profile=0):
        prob.poses[...] = p0; prob.points[...] = x0; prob.intrinsics[...] = i0
        dp.upload_parameters()
        o = capi.default_options(max_num_iterations=n, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
        o.profile_phases = profile
        return dp.solve(o)[0]
    for label, kw in LOSSES:
        dp.set_loss(**kw)
        solve(iters)                                  # warm-up (the plan is built by the first solve of the handle)
        a, b = solve(iters), solve(2 * iters)
        extra = b.num_iterations - a.num_iterations
        marginal = (b.total_time_s - a.total_time_s) / extra * 1e3 if extra > 0 else float("nan")
        solve(iters, profile=1)
        ph = dp.phase_times()
        ms = ph["eval_lm"][0] + ph["eval_trial"][0]
        calls = ph["eval_lm"][1] + ph["eval_trial"][1]
        rows.append(dict(loss=label, marginal_ms_per_iteration=marginal, eval_ms_per_launch=ms / max(calls, 1), eval_launches=calls, final_cost=a.final_cost, lm_iterations=a.num_iterations - 1))
        print(f"{name} {label:18s}: marginal {marginal:.3f} ms per LM iteration; LM-mode evaluation {ms / max(calls, 1):.4f} ms per launch ({calls} launches); "
              f"{a.num_iterations - 1} iterations, final cost {a.final_cost:.6e}", flush=True)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(dict(config=name, iters=iters, rows=rows), f, indent=1)
