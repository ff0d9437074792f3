#!/usr/bin/env python3
"""Time of the pose graph on the device (cs_essential_graph_optimize, Optimizer::OptimizeEssentialGraph) on the ~300-vertex case of tests/essential_graph_patterns.py and on
its 2 000-vertex / ~12 000-edge map, and, where the reference tree and the g2o objects of oracle/_ref are present, the time of the reference's own function text on the same
maps on this host's CPU (built by the recipe of tests/test_essential_graph_restatement_pins.py into a temporary directory, one thread).  Prints one JSON line.

    python tools/essential_graph_bench.py [--graphs 300,2000] [--reps 7] [--warmup 2] [--cpu-only | --gpu-only] [--cpu-reps 3]

wall_ms is the host clock around one optimise on an existing handle: uploads, every launch of every LM trial, the per-trial read-back and the final download.  create_ms is the
symbolic analysis and its upload, once per graph.  The kernel times are device-event sums per optimise, taken in repetitions of their own: linearize_ms (eg_linearize),
assemble_ms (eg_assemble), factor_solve_ms (eg_factor + eg_back).  The reference's linear solver in this build is the dense shadow of linear_solver_eigen.h, not Eigen's sparse
Cholesky, so its time says what this build of the text costs, not what an ORB-SLAM2 binary costs."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="300,2000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    args = ap.parse_args()
    from tests import essential_graph_patterns as P
    from tests import essential_graph_restatement as R
    maps = {}
    for g in args.graphs.split(","):
        maps[g] = (P.case("kf300"), P.CASES["kf300"][1]) if g == "300" else P.graph_2000()
    out = {"what": "Optimizer::OptimizeEssentialGraph", "reps": args.reps, "warmup": args.warmup}
    if not args.cpu_only:
        import torch  # first: one copy of the HIP runtime in the process (see tests/conftest.py)
        torch.cuda.is_available()
        from cube_slam_amd import _lib
        from cube_slam_amd import optimizer as O
        ctx = _lib.Context(0)  # raises without a HIP device
        out["gpu"] = {}
        for name, (mp, fix) in maps.items():
            g = O.build_essential_graph(R.flatten(mp))
            t = time.perf_counter()
            eg = O.EssentialGraph(g, fix, ctx=ctx)
            create_ms = (time.perf_counter() - t) * 1e3
            run = lambda: eg.optimize(g["Scw"], g["Snc"], g["has_nc"])
            for _ in range(args.warmup):
                run()
            ts = []
            for _ in range(args.reps):
                t = time.perf_counter()
                st = run()[2]  # returns after the synchronise that ends the call
                ts.append((time.perf_counter() - t) * 1e3)
            ctx.timing(True)
            ctx.timing_reset()
            k_reps = max(2, args.reps // 3)
            for _ in range(k_reps):
                run()
            k = {n: ctx.timing_get(n) for n in ("eg_linearize", "eg_assemble", "eg_factor", "eg_back", "eg_error", "eg_update", "eg_reduce", "eg_measure")}
            ctx.timing(False)
            eg.close()
            sy = P.symbolic(len(g["Scw"]), g["edge_i"], g["edge_j"], g["fixed_vertex"])
            out["gpu"][name] = {"vertices": len(g["Scw"]), "edges": len(g["edge_i"]), "create_ms": round(create_ms, 3), "wall_ms": _stats(ts), "iterations": st["iterations"],
                                "trials": st["trials"], "launches_per_trial": st["launches_per_trial"], "levels": st["levels"], "widest_level": max(sy["widths"]),
                                "levels_of_one_column": sum(1 for w in sy["widths"] if w == 1), "l_blocks": st["l_blocks"], "h_blocks": st["h_blocks"],
                                "linearize_ms": round(k["eg_linearize"][0] / k_reps, 4), "assemble_ms": round(k["eg_assemble"][0] / k_reps, 4),
                                "factor_solve_ms": round((k["eg_factor"][0] + k["eg_back"][0]) / k_reps, 4),
                                "other_kernels_ms": round(sum(k[n][0] for n in ("eg_error", "eg_update", "eg_reduce", "eg_measure")) / k_reps, 4),
                                "chi2": [st["chi2_first"], st["chi2_last"]]}
        ctx.close()
    if not args.gpu_only:
        if R.reference_available():
            out["reference_cpu"] = {"threads": 1, "solver": "dense shadow of linear_solver_eigen.h"}
            with tempfile.TemporaryDirectory() as d:
                lib = R.build_reference(d)
                for name, (mp, fix) in maps.items():
                    if len(mp.all_kfs) > 500:
                        out["reference_cpu"][name] = "not measured: the dense shadow solver needs hours on 14 000 unknowns"
                        continue
                    ts = [R.run_reference(lib, mp, fix)["seconds"] * 1e3 for _ in range(args.cpu_reps)]
                    out["reference_cpu"][name] = {"ms": _stats(ts)}
        else:
            out["reference_cpu"] = "not measured: the reference tree or the g2o objects of oracle/_ref are not here"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
