#!/usr/bin/env python3
"""Time of the dynamic-object KLT on the device: pyramids and derivatives of a batch of frames (cs_klt_set_frames) and the tracker over all pairs of the batch in one
call (cs_klt_track), against the C++ host mirror of the same statement on 1 and on --host-threads threads.  Prints one JSON line.

    python tools/klt_bench.py [--pairs 512] [--width 640 --height 480 --points 300] [--reps 5] [--warmup 1] [--host-threads 16] [--host-pairs 64]

All numbers after a warm-up of every call:
  set_frames_wall_ms   host clock around cs_klt_set_frames (the upload of pairs + 1 gray frames from pageable memory, 8 launches, the synchronise);
                       pyramid_kernel_ms = the device-event time of klt_level + klt_scharr over all levels, taken in repetitions of their own;
                       torch_h2d_same_array_ms = the same pageable array through torch's host-to-device copy, a cross-check of the upload's share
  track_wall_ms        cs_klt_track for all pairs: upload of the points, the kernel, the results back; track_kernel_ms = klt_track alone
  host_ms              cubeslam::ORBmatcher::calcOpticalFlowPyrLK without a context (tools/klt_bench_host.cpp, g++ -O2) over the first --host-pairs pairs; the mirror builds
                       both pyramids of every pair, where the device builds one per frame; host_ms_per_pair * pairs is the figure to put beside the device's two
Frame f is the texture cut at a column that moves by 3 pixels a frame (to and fro), so every pair has a real flow; the points are a seeded scatter over the frame."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def make_frames(n, W, H):
    from cube_slam_amd import synth
    base = synth._texture_base(3000, W, H)
    gray = np.zeros((n, H, W), np.uint8)
    for f in range(n):
        s = 100 + 3 * abs(f % 32 - 16)
        gray[f] = base[:, s:s + W]
    return gray


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--points", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-pairs", type=int, default=64)
    args = ap.parse_args()
    import torch  # first: one copy of the HIP runtime in the process (see tests/conftest.py)
    torch.cuda.is_available()
    from cube_slam_amd import _lib
    from cube_slam_amd.klt import KLTTracker

    P, W, H, n = args.pairs, args.width, args.height, args.points
    gray = make_frames(P + 1, W, H)
    rng = np.random.default_rng(7)
    pts = [rng.uniform([5, 5], [W - 5, H - 5], (n, 2)).astype(np.float32) for _ in range(P)]
    pairs = [(p, p + 1) for p in range(P)]
    ctx = _lib.Context(0)  # raises without a HIP device
    t = KLTTracker(P + 1, W, H, P * n, ctx=ctx)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    res = {}
    setf = lambda: t.set_frames(gray)  # noqa: E731

    def track():
        res["r"] = t.track(pairs, pts)

    for _ in range(args.warmup):
        timed(setf); timed(track)
    t_s, t_t = [], []
    for _ in range(args.reps):
        t_s.append(timed(setf)); t_t.append(timed(track))
    # a cross-check of the upload inside set_frames: the same pageable array through torch's copy, synchronised
    tg = torch.from_numpy(gray)
    t_h2d = []
    for _ in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        d = tg.to("cuda")
        torch.cuda.synchronize()
        t_h2d.append((time.perf_counter() - t0) * 1e3)
        del d
    t_h2d = t_h2d[args.warmup:]
    ctx.timing(True)
    ctx.timing_reset()
    k_reps = max(2, args.reps // 2)
    for _ in range(k_reps):
        timed(setf); timed(track)
    kern = {name: round(ctx.timing_get(name)[0] / k_reps, 4) for name in ("klt_level", "klt_scharr", "klt_track")}
    ctx.timing(False)
    tracked = [int(r[1].sum()) for r in res["r"]]
    flow = np.concatenate([r[0][r[1] > 0] - q[r[1] > 0] for r, q in zip(res["r"], pts)])
    hp = min(args.host_pairs, P)
    host = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe, inp = os.path.join(tmp, "klt_bench_host"), os.path.join(tmp, "in.bin")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-DCUBESLAM_HOST_ONLY", "-I", ROOT, os.path.join(ROOT, "tools", "klt_bench_host.cpp"), "-o", exe])
        with open(inp, "wb") as fh:
            fh.write(np.array([hp, W, H, n], np.int32).tobytes() + gray[:hp + 1].tobytes() + np.concatenate(pts[:hp]).tobytes())
        for threads in sorted({1, args.host_threads}):
            lines = subprocess.check_output([exe, inp, str(threads), str(max(1, args.reps // 2)), "1"], timeout=1500).decode().split()
            host[threads] = _stats([float(x) for x in lines[:-1]])
            assert int(lines[-1]) == sum(tracked[:hp]), (lines[-1], sum(tracked[:hp]))  # both sides tracked the same number of points
    ss, st = _stats(t_s), _stats(t_t)
    pyr = round(kern["klt_level"] + kern["klt_scharr"], 4)
    out = {
        "what": "dynamic-object KLT on the device: pyramids + derivatives, then all pairs in one call", "pairs": P, "width": W, "height": H, "points_per_pair": n,
        "levels": t.levels, "tracked_share": round(sum(tracked) / (P * n), 4), "median_flow_px": [round(float(v), 3) for v in np.median(flow, axis=0)],
        "set_frames_wall_ms": ss, "pyramid_kernel_ms": pyr, "pyramid_kernels": {k: kern[k] for k in ("klt_level", "klt_scharr")}, "track_wall_ms": st,
        "track_kernel_ms": kern["klt_track"], "track_kernel_us_per_point": round(kern["klt_track"] * 1e3 / (P * n), 4), "bytes_frames": int(gray.nbytes), "kernel_reps": k_reps,
        "torch_h2d_same_array_ms": _stats(t_h2d), "set_frames_minus_kernels_GBps": round(gray.nbytes / max(ss["median"] - pyr, 1e-9) / 1e6, 2),
        "torch_h2d_GBps": round(gray.nbytes / _stats(t_h2d)["median"] / 1e6, 2),
        "host_pairs": hp, "host_ms": {str(k): v for k, v in host.items()},
        "host_ms_per_pair": {str(k): round(v["median"] / hp, 4) for k, v in host.items()},
        "host_all_pairs_ms": {str(k): round(v["median"] / hp * P, 2) for k, v in host.items()},
        "host_threads_over_device_wall": round(host[max(host)]["median"] / hp * P / (ss["median"] + st["median"]), 2),
    }
    print(json.dumps(out))
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
