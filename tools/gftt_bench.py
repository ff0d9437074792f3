#!/usr/bin/env python3
"""Time of the new-dynamic-point path on the device: cv::goodFeaturesToTrack on the resident frames of a KLT handle (cs_klt_good_features, with the object masks as
masks) and the whole new-feature loop of Tracking::CreateNewKeyFrame (cs_track_new_harris_features: mask with discs, corners, unprojection), each for all frames in one
call, against the C++ host mirror of the same statements on 1 and on --host-threads threads.  Prints one JSON line.

    python tools/gftt_bench.py [--frames 512] [--width 640 --height 480 --exist 100] [--reps 5] [--warmup 1] [--host-threads 16] [--host-frames 64]

All numbers after a warm-up of every call:
  good_features_wall_ms   host clock around cs_klt_good_features: the upload of the masks from pageable memory, five launches, the corners back
  new_harris_wall_ms      the same around cs_track_new_harris_features (the optional mask read-back is off)
  kernels                 device-event time of every kernel per call, taken in repetitions of their own (the events serialise the launches)
  host_ms                 cubeslam::goodFeaturesToTrack / Tracking::CreateNewHarrisFeatures without a context (tools/gftt_bench_host.cpp, g++ -O2) over the first --host-frames
                          frames; host_all_frames_ms scales it to --frames
Frame f is the 1/f texture cut at a column that moves with f; the object masks are two rectangles that cover about a quarter of the frame and move with it; the
existing points are a seeded scatter over the objects."""
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

K4 = np.array([520.0, 520.0, 320.0, 240.0], np.float32)
TWC = np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 0.3]], np.float32)


def make_inputs(n, W, H, n_exist):
    from cube_slam_amd import synth
    base = synth._texture_base(3000, W, H)
    gray, masks = np.zeros((n, H, W), np.uint8), np.zeros((n, H, W), np.uint8)
    rng = np.random.default_rng(11)
    pts = []
    for f in range(n):
        s = 3 * abs(f % 32 - 16)
        gray[f] = base[:, 100 + s:100 + s + W]
        a = (W // 16 + s, H // 8, W // 16 + s + W * 3 // 10, H // 8 + H * 2 // 5)          # two objects of 0.3 W x 0.4 H: 24 % of the frame
        b = (W // 2 + s, H // 2, W // 2 + s + W * 3 // 10, H // 2 + H * 2 // 5)
        masks[f, a[1]:a[3], a[0]:a[2]] = 1
        masks[f, b[1]:b[3], b[0]:b[2]] = 2
        half = n_exist // 2
        pts.append(np.concatenate([rng.uniform(a[:2], a[2:], (half, 2)), rng.uniform(b[:2], b[2:], (n_exist - half, 2))]).astype(np.float32))
    return gray, masks, pts, [rng.integers(1, 6, n_exist).astype(np.int32) for _ in range(n)]


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--exist", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-frames", type=int, default=64)
    args = ap.parse_args()
    import torch  # first: one copy of the HIP runtime in the process (see tests/conftest.py)
    torch.cuda.is_available()
    from cube_slam_amd import _lib
    from cube_slam_amd.klt import KLTTracker

    F, W, H = args.frames, args.width, args.height
    gray, masks, pts, obs = make_inputs(F, W, H, args.exist)
    depth = [np.array([3.0, 5.0], np.float32)] * F
    Twc = np.stack([TWC] * F)
    ctx = _lib.Context(0)  # raises without a HIP device
    t = KLTTracker(F, W, H, 1, ctx=ctx)
    t.set_frames(gray)
    frames = np.arange(F)
    res = {}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    def good():
        res["g"] = t.good_features(frames, masks, 200, 0.1, 10.0)

    def harris():
        res["h"] = t.new_harris_features(frames, masks, pts, obs, K4, Twc, depth)

    for _ in range(args.warmup):
        timed(good); timed(harris)
    t_g, t_h = [], []
    for _ in range(args.reps):
        t_g.append(timed(good)); t_h.append(timed(harris))
    names = ("gftt_init", "gftt_eig", "gftt_candidates", "gftt_select", "gftt_mask", "gftt_new_points")
    k_reps = max(2, args.reps // 2)
    kern = {}
    for what, fn in (("good_features", good), ("new_harris", harris)):
        ctx.timing(True)
        ctx.timing_reset()
        for _ in range(k_reps):
            timed(fn)
        kern[what] = {k: round(ctx.timing_get(k)[0] / k_reps, 4) for k in names if ctx.timing_get(k)[1]}
        ctx.timing(False)
    hf = min(args.host_frames, F)
    host = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe, inp = os.path.join(tmp, "gftt_bench_host"), os.path.join(tmp, "in.bin")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-DCUBESLAM_HOST_ONLY", "-I", ROOT, os.path.join(ROOT, "tools", "gftt_bench_host.cpp"), "-o", exe])
        with open(inp, "wb") as fh:
            fh.write(np.array([hf, W, H, args.exist], np.int32).tobytes() + gray[:hf].tobytes() + masks[:hf].tobytes() + np.concatenate(pts[:hf]).tobytes() + np.concatenate(obs[:hf]).tobytes() +
                     K4.tobytes() + TWC.tobytes())
        for threads in sorted({1, args.host_threads}):
            lines = subprocess.check_output([exe, inp, str(threads), str(max(1, args.reps // 2)), "1"], timeout=1500).decode().split()
            vals = [float(x) for x in lines[:-2]]
            host[threads] = {"good_features": _stats(vals[0::2]), "new_harris": _stats(vals[1::2])}
            assert int(lines[-2]) == sum(len(r["corners"]) for r in res["g"][:hf]) and int(lines[-1]) == sum(len(r["pts"]) for r in res["h"][:hf]), lines[-2:]  # the same corners on both sides
    sg, sh = _stats(t_g), _stats(t_h)
    scale = lambda what: {str(k): round(v[what]["median"] / hf * F, 2) for k, v in host.items()}  # noqa: E731
    out = {"what": "goodFeaturesToTrack and the new-Harris-feature loop on resident frames, all frames in one call", "frames": F, "width": W, "height": H, "existing_points": args.exist,
           "mask_share": round(float((masks > 0).mean()), 4), "corners_per_frame": round(float(np.mean([len(r["corners"]) for r in res["g"]])), 2),
           "new_points_per_frame": round(float(np.mean([len(r["pts"]) for r in res["h"]])), 2), "candidates_per_frame": round(float(np.mean([r["n_candidates"] for r in res["g"]])), 1),
           "good_features_wall_ms": sg, "new_harris_wall_ms": sh, "kernels_ms": kern, "kernel_sum_ms": {k: round(sum(v.values()), 4) for k, v in kern.items()}, "kernel_reps": k_reps,
           "bytes_masks": int(masks.nbytes), "host_frames": hf, "host_ms": {str(k): v for k, v in host.items()},
           "host_all_frames_ms": {"good_features": scale("good_features"), "new_harris": scale("new_harris")},
           "host_threads_over_device_wall": {"good_features": round(scale("good_features")[str(max(host))] / sg["median"], 2), "new_harris": round(scale("new_harris")[str(max(host))] / sh["median"], 2)}}
    print(json.dumps(out))
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
