#!/usr/bin/env python3
"""Time of the local-mapping entry points on the device -- cs_create_new_map_points for one key frame of 1 000 key points with 20 neighbours of 1 000 key points (300 matched
pairs per neighbour), cs_mappoint_distinctive_descriptors and cs_mappoint_update_normal_and_depth for 100 000 points of 6 observations -- with the time of the restatement
(tests/local_mapping_restatement.py: numpy scalars for the triangulation loop, numpy arrays for the two MapPoint methods, one CPU thread of this host) beside it.  Prints one
JSON line.

    python tools/local_mapping_bench.py [--neighbours 20] [--keypoints 1000] [--pairs 300] [--points 100000] [--observations 6] [--reps 10] [--warmup 2] [--no-cpu]

*_wall_ms is the host clock around one call: uploads, kernels, downloads and the synchronise that ends it.  *_kernel_ms is the device-event time of the named kernel, taken in
repetitions of their own.  Every size is warmed up before it is timed."""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def _timed(ctx, fn, kernels, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    ctx.timing(True); ctx.timing_reset()
    for _ in range(max(2, reps // 3)):
        fn()
    r = {"wall_ms": _stats(ts)}
    for name in kernels:
        ms, n = ctx.timing_get(name)
        r[name + "_kernel_ms"] = round(ms / max(n, 1), 4)
    ctx.timing(False)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--observations", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch  # first: one copy of the HIP runtime in the process (see tests/conftest.py)
    torch.cuda.is_available()
    from cube_slam_amd import _lib
    from cube_slam_amd.local_mapping import ComputeDistinctiveDescriptors, KeyFrameView, UpdateNormalAndDepth, create_new_map_points
    from tests import local_mapping_patterns as P
    from tests import local_mapping_restatement as R
    ctx = _lib.Context(0)  # raises without a HIP device
    out = {"what": "CreateNewMapPoints' triangulation loop, ComputeDistinctiveDescriptors, UpdateNormalAndDepth", "neighbours": args.neighbours, "keypoints": args.keypoints,
           "pairs_per_neighbour": args.pairs, "points": args.points, "observations": args.observations, "reps": args.reps, "warmup": args.warmup, "host": platform.node(),
           "cpu_model": next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "?")}
    s = P.random_scene(9, args.keypoints, [args.pairs] * args.neighbours, "mixed", N2=args.keypoints)
    view = lambda f: KeyFrameView(f.keysUn, f.keys_xy, f.u_right, f.depth, f.Rcw, f.tcw, f.Ow, f.fx, f.fy, f.cx, f.cy, f.invfx, f.invfy, f.mbf, f.mb, f.scale_factors, f.level_sigma2,
                                  f.scale_factor)
    kf, nbs = view(s["kf"]), [view(f) for f in s["neighbours"]]
    search = R.table_search(s["best2"])
    m = np.stack([search(n, s["skip1"]) for n in range(args.neighbours)])
    res = create_new_map_points(ctx, kf, nbs, m)
    out["create_new_map_points"] = _timed(ctx, lambda: create_new_map_points(ctx, kf, nbs, m), ("lm_triangulate", "lm_claim"), args.reps, args.warmup)
    out["create_new_map_points"].update(pairs=int(res["pair_off"][-1]), new_points=res["nnew"])

    rng = np.random.default_rng(3)
    n, k = args.points, args.observations
    off = (np.arange(n + 1) * k).astype(np.int32)
    desc = rng.integers(0, 256, (n, 1, 32), dtype=np.uint8).repeat(k, axis=1)
    desc ^= (rng.random((n, k, 32)) < 0.1).astype(np.uint8) << rng.integers(0, 8, (n, k, 32), dtype=np.uint8)  # observations of one point: copies with a few bits flipped
    desc = np.ascontiguousarray(desc.reshape(-1, 32))
    out["distinctive_descriptors"] = _timed(ctx, lambda: ComputeDistinctiveDescriptors(ctx, off, desc), ("mp_distinctive",), args.reps, args.warmup)
    n_kf = 200
    kf_Ow = rng.uniform(-3, 3, (n_kf, 3)).astype(np.float32)
    pos = (rng.uniform(-1, 1, (n, 3)) * [4, 4, 1] + [0, 0, 9]).astype(np.float32)
    obs = rng.integers(0, n_kf, n * k).astype(np.int32)
    ref_kf = obs[::k].copy(); ref_oct = rng.integers(0, P.N_LEVELS, n).astype(np.int32)
    out["update_normal_and_depth"] = _timed(ctx, lambda: UpdateNormalAndDepth(ctx, pos, off, obs, kf_Ow, ref_kf, ref_oct, P.SF), ("mp_normal_depth",), args.reps, args.warmup)
    if not args.no_cpu:
        t = time.perf_counter()
        pts, _ = R.create_new_map_points(s["kf"], s["neighbours"], search, s["skip1"])
        cpu = {"create_new_map_points_ms": round((time.perf_counter() - t) * 1e3, 1), "new_points": len(pts)}
        t = time.perf_counter()
        best = R.distinctive_descriptors(off, desc)
        cpu["distinctive_descriptors_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        t = time.perf_counter()
        z = lambda *sh: np.zeros(sh, np.float32)
        ref = R.update_normal_and_depth_many(pos, off, obs, kf_Ow, ref_kf, ref_oct, P.SF, z(n, 3), z(n), z(n), np.zeros(n, np.uint8))
        cpu["update_normal_and_depth_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        got = UpdateNormalAndDepth(ctx, pos, off, obs, kf_Ow, ref_kf, ref_oct, P.SF)
        cpu["equal"] = bool(len(pts) == res["nnew"] and np.array_equal(best, ComputeDistinctiveDescriptors(ctx, off, desc)) and got[0].tobytes() == ref[0].tobytes()
                            and got[1].tobytes() == ref[1].tobytes() and got[2].tobytes() == ref[2].tobytes())
        out["restatement_cpu"] = cpu
    print(json.dumps(out))


if __name__ == "__main__":
    main()
