#!/usr/bin/env python3
"""Time of one cs_initializer_evaluate on the device -- 512 frame pairs of 300 matches, 200 RANSAC iterations each (2 x 200 hypotheses, then the CheckRT passes of the chosen
model's candidates), in one call -- with the CPU path of the same headers beside it: csrc/initializer_host.h without a context (g++ -O2 -ffp-contract=off, on one thread and on
16 of this host; tools/initializer_bench_host.cpp, compiled into a temporary directory).  The device's tables are compared with the g++ build's byte for byte (a NaN as a class).  Wall time of the
call, copies included.  Prints one JSON line.

    python tools/initializer_bench.py [--pairs 512] [--matches 300] [--iterations 200] [--reps 5] [--warmup 2] [--threads 1 16] [--no-cpu]

Kernel times come from a run of their own:  rocprofv3 --kernel-trace --stats -- python tools/initializer_bench.py --no-cpu"""
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
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3), "max_ms": round(float(ms.max()), 3)}


def same(raw, want):
    """The host program's output against the device's tables: equal as bit patterns, a NaN equal to any NaN (x86 and the device give NaNs of different sign; a degenerate
    set of eight has a NaN score on both)."""
    pos = 0
    for parts in want:
        for a in parts:
            b = np.frombuffer(raw, a.dtype, a.size, pos).reshape(a.shape); pos += a.nbytes
            if a.dtype.kind == "f":
                na, nb = np.isnan(a), np.isnan(b)
                if not (np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()):
                    return False
            elif a.tobytes() != b.tobytes():
                return False
    return pos == len(raw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch  # its copy of the HIP runtime first (see bench.py)
    torch.cuda.is_available()
    from cube_slam_amd import _lib
    from cube_slam_amd._ransac import draw
    from cube_slam_amd.initializer import problem_tables
    from tests import initializer_patterns as P
    ctx = _lib.Context(0)
    cases = []
    for k in range(a.pairs):  # general scenes and planes alternate, a fifth of the matches gross outliers
        c = P.scene("plane" if k % 2 else "general", a.matches, 5000 + k, outliers=0.2, **({"tilt": (1.0, 0.0)} if k % 2 else {}))
        rng = np.random.RandomState(9000 + k)
        first = np.nonzero(c["vMatches12"] >= 0)[0]
        c.update(K=P.K, sigma=np.float32(1.0), N=a.matches, sets=draw(a.matches, 8, a.iterations, lambda lo, hi: int(rng.randint(lo, hi + 1))),
                 matches=np.stack([first, c["vMatches12"][first]], 1).astype(np.int32))
        cases.append(c)
    ms = []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        dev, co, ho = P.evaluate(cases, ctx=ctx)
        if r >= a.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    rec = {"pairs": a.pairs, "matches": a.matches, "iterations": a.iterations, "hypotheses": int(2 * ho[-1]), "model_H": int((dev["model"] == 0).sum()),
           "model_F": int((dev["model"] == 1).sum()), "device": stats(ms)}
    if not a.no_cpu:
        tmp = tempfile.mkdtemp(prefix="initializer_bench_")
        try:
            exe = os.path.join(tmp, "initializer_bench_host")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-DCUBESLAM_HOST_ONLY", "-I", ROOT,
                                   os.path.join(ROOT, "tools", "initializer_bench_host.cpp"), "-o", exe])
            with open(os.path.join(tmp, "in.bin"), "wb") as f:
                f.write(np.int32(len(cases)).tobytes())
                for c in cases:
                    f.write(np.array([len(c["keys1"]), len(c["keys2"]), c["N"], len(c["sets"])], np.int32).tobytes())
                    f.write(np.float32(c["sigma"]).tobytes()); f.write(c["K"].astype(np.float32).tobytes())
                    f.write(c["keys1"].tobytes()); f.write(c["keys2"].tobytes()); f.write(c["matches"].tobytes()); f.write(c["sets"].astype(np.int32).tobytes())
            names = ("nGood", "S", "RH", "cand_Rt", "cos_parallax", "score", "matrix", "mask", "good_mask", "points")
            want = [[np.array([t["model"], t["best"][0], t["best"][1], t["n_inliers"], t["n_cand"]], np.int32)] + [np.ascontiguousarray(t[k]) for k in names]
                    for t in problem_tables(dev, co, ho)]
            for th in a.threads:
                o = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), str(th), "1" if th == 1 else "3"], check=True, capture_output=True, text=True)
                rec["cpu_gpp_O2_%d_thread%s" % (th, "" if th == 1 else "s")] = stats([float(v) for v in o.stdout.split()])
                rec["byte_equal"] = rec.get("byte_equal", True) and same(open(os.path.join(tmp, "out.bin"), "rb").read(), want)
                rec["cpu_%d_over_device" % th] = round(rec["cpu_gpp_O2_%d_thread%s" % (th, "" if th == 1 else "s")]["median_ms"] / rec["device"]["median_ms"], 2)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
