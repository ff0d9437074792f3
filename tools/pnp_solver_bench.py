#!/usr/bin/env python3
"""Time of one cs_pnp_solver_evaluate on the device -- the hypotheses and refinements of 1, 4 and 16 relocalisation candidates of 100 and 400 correspondences, with the table
sizes SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) gives (Tracking.cc:2921) -- with the CPU path of the same headers beside it: cubeslam::PnPsolver::evaluate_many without
a context (csrc/epnp_math.h, csrc/cv_svd_math.h; g++ -O2 -ffp-contract=off, one thread of this host; tools/pnp_solver_bench_host.cpp, compiled into a temporary directory).
The device's tables are compared with the g++ build's byte for byte (a NaN as a class).  Wall time of the call, copies included.  Prints one JSON line per size.

    python tools/pnp_solver_bench.py [--candidates 1 4 16] [--correspondences 100 400] [--reps 20] [--warmup 3] [--no-cpu]

Kernel times come from a run of their own:  rocprofv3 --kernel-trace --stats -- python tools/pnp_solver_bench.py --no-cpu"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--correspondences", type=int, nargs="+", default=[100, 400])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    from cube_slam_amd import _lib
    from tests import pnp_solver_patterns as P
    ctx = _lib.Context(0)
    tmp = tempfile.mkdtemp(prefix="pnp_solver_bench_")
    try:
        exe = os.path.join(tmp, "pnp_solver_bench_host")
        if not a.no_cpu:
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DCUBESLAM_HOST_ONLY", "-I", ROOT, os.path.join(ROOT, "tools", "pnp_solver_bench_host.cpp"), "-o", exe])
        for N in a.correspondences:
            for nc in a.candidates:
                cases = []
                for k in range(nc):
                    c = P.correspondences(N, 1000 + 17 * k + N, inlier=0.6, noise=0.3)
                    c["min_inliers"], c["max_its"], _ = P.parameters(P.RELOC, N)
                    c["max_err"] = c["sigma2"] * np.float32(P.RELOC[5])
                    c["quads"] = P.draw(N, c["max_its"], 2000 + k)
                    cases.append(c)
                ms = []
                for r in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    dev = P.evaluate(cases, ctx=ctx)
                    if r >= a.warmup:
                        ms.append((time.perf_counter() - t0) * 1e3)
                rec = {"candidates": nc, "correspondences": N, "hypotheses": int(sum(len(c["quads"]) for c in cases)), "records": int((dev["refined_n"] >= 0).sum()),
                       "device": stats(ms)}
                if not a.no_cpu:
                    with open(os.path.join(tmp, "in.bin"), "wb") as f:
                        f.write(np.int32(nc).tobytes())
                        for c in cases:
                            f.write(np.array([N, len(c["quads"])], np.int32).tobytes()); f.write(np.asarray(c["K"], np.float32).tobytes())
                            for k, dt in (("P3Dw", np.float32), ("P2D", np.float32), ("sigma2", np.float32), ("quads", np.int32)):
                                f.write(np.ascontiguousarray(c[k], dt).tobytes())
                    o = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), str(a.reps), str(a.warmup)], check=True, capture_output=True, text=True)
                    rec["cpu_gpp_O2_one_thread"] = stats([float(v) for v in o.stdout.split()])
                    raw = open(os.path.join(tmp, "out.bin"), "rb").read()
                    pos, h0, w0, equal = 0, 0, 0, True
                    for c in cases:
                        H, W = len(c["quads"]), (N + 31) // 32
                        for key, dt, per, base, width in (("n_inliers", np.int32, 1, h0, 1), ("refined_n", np.int32, 1, h0, 1), ("status", np.uint32, 1, h0, 1), ("Rt", np.float64, 12, h0, 12),
                                                          ("refined_Rt", np.float64, 12, h0, 12), ("mask", np.uint32, W, w0, 1), ("refined_mask", np.uint32, W, w0, 1)):
                            got = np.frombuffer(raw, dt, H * per, pos); pos += got.nbytes
                            want = dev[key].reshape(-1)[base * width:base * width + H * per] if key.endswith("mask") else dev[key].reshape(-1)[base * per:(base + H) * per]
                            if dt == np.float64:
                                na, nb = np.isnan(got), np.isnan(want)
                                equal &= bool(np.array_equal(na, nb) and got[~na].tobytes() == want[~nb].tobytes())
                            else:
                                equal &= got.tobytes() == want.tobytes()
                        h0 += H; w0 += H * W
                    rec["byte_equal"] = bool(equal and pos == len(raw))
                    rec["cpu_over_device"] = round(rec["cpu_gpp_O2_one_thread"]["median_ms"] / rec["device"]["median_ms"], 2)
                print(json.dumps(rec), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
