#!/usr/bin/env python3
"""Time of the RGB-D frame on the device: the upload of the raw depth images, the gather (cs_rgbd_from_orb, Frame::ComputeStereoFromRGBD) and the close-point pass
(cs_rgbd_close_points) against the C++ host mirror of the same rule on 16 threads.  Prints one JSON line.

    python tools/rgbd_bench.py [--frames 512] [--width 640 --height 480 --features 1000] [--reps 10] [--warmup 2] [--host-threads 16]

All numbers after a warm-up of every call, the calls alternating within a repetition:
  upload_wall_ms        host clock around cs_rgbd_upload_depth (pageable host memory, as a caller's cv::Mat) and the synchronise behind it
  gather_wall_ms        the same around cs_rgbd_from_orb; gather_kernel_ms = the device-event time of rgbd_gather, taken in repetitions of their own
  close_points_wall_ms  cs_rgbd_close_points through the Python mirror's raw form: upload of need_new and the poses, the kernel, the results back; close_points_kernel_ms = rgbd_close_points alone
  host_close_points_ms  cubeslam::ClosePoints without a context (tools/rgbd_bench_host.cpp, g++ -O2) over the same frames on --host-threads threads
The extraction that leaves the key points on the device runs once and is not timed."""
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

K4 = np.array([517.306408, 516.469215, 318.643040, 255.313989], np.float32)  # TUM1.yaml
DIST5 = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], np.float32)
BF, FACTOR = 40.0, float(np.float32(1.0) / np.float32(5000.0))
TH_DEPTH = float(np.float32(BF) * np.float32(40.0) / K4[0])


def make_frames(n, W, H, n_bases=8):
    """n gray frames (a band-limited texture cut at a moving column, noise) and n raw depth images: smooth surfaces 0.5 - 6 m in the sensor's units with 25 % holes."""
    from cube_slam_amd import synth
    bases = [synth._texture_base(2000 + i, W, H).astype(np.float32) for i in range(min(n_bases, n))]
    gray, depth = np.zeros((n, H, W), np.uint8), np.zeros((n, H, W), np.uint16)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for f in range(n):
        rng = np.random.default_rng(f)
        s = 100 + 3 * (f // len(bases))
        gray[f] = np.clip(np.rint(bases[f % len(bases)][:, s:s + W] + 2.0 * rng.standard_normal((H, W), dtype=np.float32)), 0, 255)
        a, b, c = rng.uniform(0.5, 3.0), rng.uniform(0, 3.0 / W), rng.uniform(0, 1.0 / H)
        z = (a + b * xx + c * yy) * 5000.0 + 40.0 * rng.standard_normal((H, W), dtype=np.float32)
        d = np.clip(z, 1, 65535).astype(np.uint16)
        d[rng.random((H, W)) < 0.25] = 0
        depth[f] = d
    return gray, depth


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-threads", type=int, default=16)
    args = ap.parse_args()
    import torch  # first: one copy of the HIP runtime in the process (see tests/conftest.py)
    torch.cuda.is_available()
    from cube_slam_amd import _lib
    from cube_slam_amd.orb import ORBextractor
    from cube_slam_amd.rgbd import RGBDAssociator

    F, W, H = args.frames, args.width, args.height
    gray, depth = make_frames(F, W, H)
    ctx = _lib.Context(0)  # raises without a HIP device
    orb = ORBextractor(args.features, 1.2, 8, 20, 7, W, H, max_frames=F, ctx=ctx)
    orb.upload(gray)
    orb.run()
    ctx.sync()
    del gray
    a = RGBDAssociator(W, H, orb.cap, F, ctx=ctx)
    Tcw = np.tile(np.eye(4, dtype=np.float32)[:3], (F, 1, 1))
    Tcw[:, :, 3] = np.random.default_rng(1).uniform(-1, 1, (F, 3))

    def timed(fn):
        t = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3

    upload = lambda: a.upload_depth(depth)
    gather = lambda: a.from_orb(orb, K4, DIST5, BF, FACTOR)
    upload(); gather(); ctx.sync()
    _, dep, first, n_with, n_out = a.read_packed()
    need = (np.random.default_rng(2).random(len(dep)) < 0.5).astype(np.uint8)
    result = {}

    def close():
        result["r"] = a.close_points(need, Tcw, K4, TH_DEPTH, raw=True)

    for _ in range(args.warmup):
        timed(upload); timed(gather); timed(close)
    t_up, t_g, t_c = [], [], []
    for _ in range(args.reps):  # alternating
        t_up.append(timed(upload)); t_g.append(timed(gather)); t_c.append(timed(close))
    ctx.timing(True)
    ctx.timing_reset()
    k_reps = max(2, args.reps // 3)
    for _ in range(k_reps):
        timed(gather); timed(close)
    kern = {name: round(ctx.timing_get(name)[0] / k_reps, 4) for name in ("rgbd_gather", "rgbd_close_points")}
    ctx.timing(False)
    created = int(result["r"][4][-1])  # new_first[n_frames]
    # the host mirror over the same frames
    host = None
    with tempfile.TemporaryDirectory() as tmp:
        exe, inp = os.path.join(tmp, "rgbd_bench_host"), os.path.join(tmp, "in.bin")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-DCUBESLAM_HOST_ONLY", "-I", ROOT, os.path.join(ROOT, "tools", "rgbd_bench_host.cpp"), "-o", exe])
        with open(inp, "wb") as fh:
            fh.write(np.int32(F).tobytes() + first.astype(np.int32).tobytes() + K4.tobytes() + np.float32(TH_DEPTH).tobytes() + Tcw.tobytes() + dep.tobytes()
                     + a.read_keys_un().tobytes() + need.tobytes())
        lines = subprocess.check_output([exe, inp, str(args.host_threads), str(args.reps), str(args.warmup)], timeout=600).decode().split()
        host = _stats([float(x) for x in lines[:-1]])
        assert int(lines[-1]) == created, (lines[-1], created)  # both sides created the same number of points
    su, sg, sc = _stats(t_up), _stats(t_g), _stats(t_c)
    n_kp = int(first[-1])
    out = {
        "what": "RGB-D frame on the device: raw depth upload, gather, close points", "frames": F, "width": W, "height": H, "depth_type": "u16", "features": args.features,
        "keypoints": n_kp, "with_depth_share": round(float(n_with.sum()) / max(n_kp, 1), 4), "outside": int(n_out.sum()), "created": created,
        "upload_wall_ms": su, "upload_GBps": round(depth.nbytes / su["median"] / 1e6, 2), "gather_wall_ms": sg, "gather_kernel_ms": kern["rgbd_gather"],
        "upload_over_gather_wall": round(su["median"] / sg["median"], 2), "bytes_image": int(depth.nbytes), "bytes_samples_read": 2 * n_kp,
        "close_points_wall_ms": sc, "close_points_kernel_ms": kern["rgbd_close_points"], "host_close_points_ms": host, "host_threads": args.host_threads,
        "host_over_device_wall": round(host["median"] / sc["median"], 2), "kernel_reps": k_reps,
    }
    print(json.dumps(out))
    a.close()
    orb.close()
    ctx.close()


if __name__ == "__main__":
    main()
