#!/usr/bin/env python3
"""Rate of the batched Sim3 refinement (cs_sim3_optimization, Optimizer::OptimizeSim3) for batches of 1, 8, 64 and 512 problems of 200 correspondences, and, where the
reference tree and the g2o objects of oracle/_ref are present, the time of the reference's own function text for one such problem on this host's CPU (built by the recipe
of tests/test_sim3_opt_restatement_pins.py into a temporary directory).  Prints one JSON line.

    python tools/sim3_opt_bench.py [--corr 200] [--batches 1,8,64,512] [--reps 20] [--warmup 3] [--cpu-only | --gpu-only]

*_wall_ms is the host clock around one call: uploads, the one kernel, downloads and the synchronise that ends it.  kernel_ms is the device-event time of sim3_opt_kernel,
taken in repetitions of their own.  Every batch size is warmed up before it is timed."""
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
    ap.add_argument("--corr", type=int, default=200)
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    args = ap.parse_args()
    from tests import sim3_opt_restatement as R
    batches = [int(b) for b in args.batches.split(",")]
    problems = [R.make_case(seed=5000 + i, n=args.corr, n_outliers=args.corr // 8) for i in range(max(batches))]
    out = {"what": "Optimizer::OptimizeSim3, batched", "correspondences": args.corr, "reps": args.reps, "warmup": args.warmup}
    if not args.cpu_only:
        import torch  # first: one copy of the HIP runtime in the process (see tests/conftest.py)
        torch.cuda.is_available()
        from cube_slam_amd import _lib
        from cube_slam_amd.optimizer import OptimizeSim3
        ctx = _lib.Context(0)  # raises without a HIP device
        out["gpu"] = {}
        for b in batches:
            for _ in range(args.warmup):
                OptimizeSim3(problems[:b], ctx=ctx)
            ts = []
            for _ in range(args.reps):
                t = time.perf_counter()
                res = OptimizeSim3(problems[:b], ctx=ctx)  # returns after the synchronise that ends the call
                ts.append((time.perf_counter() - t) * 1e3)
            ctx.timing(True)
            ctx.timing_reset()
            k_reps = max(2, args.reps // 4)
            for _ in range(k_reps):
                OptimizeSim3(problems[:b], ctx=ctx)
            ms, n = ctx.timing_get("sim3_opt_kernel")
            ctx.timing(False)
            st = _stats(ts)
            out["gpu"][str(b)] = {"wall_ms": st, "problems_per_s": round(b / (st["median"] * 1e-3), 1), "kernel_ms": round(ms / max(n, 1), 4),
                                  "accepted": sum(1 for r in res if r[2] > 0)}
        ctx.close()
    if not args.gpu_only:
        if R.reference_available():
            with tempfile.TemporaryDirectory() as d:
                lib = R.build_reference(d)
                c = problems[0]
                for _ in range(args.warmup):
                    R.run_reference(lib, c)
                ts = []
                for _ in range(args.reps):
                    t = time.perf_counter()
                    R.run_reference(lib, c, repeats=5)
                    ts.append((time.perf_counter() - t) * 1e3 / 5)
                st = _stats(ts)
                out["reference_cpu"] = {"one_problem_ms": st, "problems_per_s": round(1e3 / st["median"], 1), "threads": 1}
        else:
            out["reference_cpu"] = "not measured: the reference tree or the g2o objects of oracle/_ref are not here"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
