#!/usr/bin/env python3
"""Time of Sim3Solver.evaluate_many on the device -- one cs_sim3_solver_hypotheses for 1, 4 and 16 loop candidates of 100 and 400 correspondences with 300 hypotheses each --
with the CPU path of the same header beside it: cubeslam::Sim3Solver::evaluate_many without a context (csrc/horn_math.h, g++ -O2 -ffp-contract=off, one thread of this host;
tools/sim3_solver_bench_host.cpp, compiled into a temporary directory).  The device's tables are compared with the library's host path (ctx=None) byte for byte.  Prints one JSON
line.  Independent of bench.py.

    python tools/sim3_solver_bench.py [--candidates 1 4 16] [--correspondences 100 400] [--hypotheses 300] [--reps 20] [--warmup 3] [--no-cpu]

wall_ms is the host clock around one call: packing, uploads, the kernel, downloads and the synchronise that ends it (median, min and max of the repetitions: the spread).
kernel_ms is the device-event time of s3s_hypotheses, taken in repetitions of their own.  Every size is warmed up before it is timed."""
import argparse
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--correspondences", type=int, nargs="+", default=[100, 400])
    ap.add_argument("--hypotheses", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch  # first: one copy of the HIP runtime in the process (see tests/conftest.py)
    torch.cuda.is_available()
    from cube_slam_amd import _lib
    from cube_slam_amd.sim3_solver import solver_hypotheses
    from tests import sim3_solver_patterns as P
    ctx = _lib.Context(0)  # raises without a HIP device
    out = {"what": "Sim3Solver.evaluate_many: every hypothesis of every loop candidate in one call", "hypotheses": args.hypotheses, "reps": args.reps, "warmup": args.warmup,
           "host": platform.node(), "cpu_model": next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "?"), "sizes": []}
    tmp = tempfile.mkdtemp(prefix="sim3_solver_bench_")
    exe = None
    if not args.no_cpu:
        exe = os.path.join(tmp, "sim3_solver_bench_host")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", ROOT, os.path.join(ROOT, "tools", "sim3_solver_bench_host.cpp"), "-o", exe, "-L",
                               os.path.join(ROOT, "cube_slam_amd"), "-lcubeslam_hip", "-Wl,-rpath," + os.path.join(ROOT, "cube_slam_amd")])
    H = args.hypotheses
    for N in args.correspondences:
        for n in args.candidates:
            cases = [P.raw_case(N, H, 500 + k) for k in range(n)]
            co = (np.arange(n + 1) * N).astype(np.int32); ho = (np.arange(n + 1) * H).astype(np.int32)
            cat = lambda k, w, dt: np.concatenate([np.asarray(c[k], dt).reshape(-1, w) for c in cases])
            a = (co, cat("X1", 3, np.float32), cat("X2", 3, np.float32), cat("e1", 1, np.float32), cat("e2", 1, np.float32), cat("K8", 8, np.float32), np.zeros(n, np.uint8), ho,
                 cat("triples", 3, np.int32))
            call = lambda c=ctx: solver_hypotheses(c, *a)
            for _ in range(args.warmup):
                call()
            ts = []
            for _ in range(args.reps):
                t = time.perf_counter(); got = call(); ts.append((time.perf_counter() - t) * 1e3)
            ctx.timing(True); ctx.timing_reset()
            for _ in range(max(3, args.reps // 3)):
                call()
            ms, cnt = ctx.timing_get("s3s_hypotheses")
            ctx.timing(False)
            r = {"candidates": n, "correspondences": N, "wall_ms": _stats(ts), "kernel_ms": round(ms / max(cnt, 1), 4)}
            if exe:
                t = time.perf_counter(); ref = call(None); r["library_host_path_ms"] = round((time.perf_counter() - t) * 1e3, 3)
                nan = np.isnan(ref[1])
                r["equal"] = bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and np.array_equal(np.isnan(got[1]), nan)
                                  and np.array_equal(got[1].view(np.uint32)[~nan], ref[1].view(np.uint32)[~nan]))
                path = os.path.join(tmp, "in_%d_%d.bin" % (N, n))
                with open(path, "wb") as f:
                    f.write(np.int32(n).tobytes())
                    for c in cases:
                        f.write(np.asarray([N, H, 0], np.int32).tobytes())
                        for k in ("X1", "X2", "e1", "e2", "K8"):
                            f.write(np.ascontiguousarray(c[k], np.float32).tobytes())
                        f.write(np.ascontiguousarray(c["triples"], np.int32).tobytes())
                cpu = json.loads(subprocess.check_output([exe, path, str(args.reps), str(args.warmup)]))
                r["gpp_O2_one_thread_ms"] = _stats(cpu["ms"])
                r["counts_sum_equal"] = bool(cpu["sum"] == int(got[0].sum()))
                r["cpu_over_device_wall"] = round(r["gpp_O2_one_thread_ms"]["median"] / r["wall_ms"]["median"], 2)
            out["sizes"].append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
