#!/usr/bin/env python3
"""The headline's runner (bench.py: ORB + cuboid on the caller's context, four line detectors on contexts of their own, 1 024 resident frames) with the
lsd_rg_seq launches of the timed region counted PER line context -- bench.py reports their sum.  Detectors that cycle at the same rate show the same count
(+- 1); a pair held up by a neighbour's wait shows about half the others'.  Prints one JSON line: the queue count the process saw, the counts, frames/s.
usage: tools/walk_counts.py [steps [warmup [frames]]]   (the environment decides GPU_MAX_HW_QUEUES, as for bench.py)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (sets GPU_MAX_HW_QUEUES only where the environment has not)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    frames = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    torch.cuda.set_device(0)
    from cube_slam_amd import _lib
    from cube_slam_amd.cuboid import CuboidBatch, detect_3d_cuboid
    from cube_slam_amd.frontend import Frontend
    from cube_slam_amd.lsd import line_lbd_detect
    from cube_slam_amd.orb import ORBextractor

    ctx = _lib.Context(0, priority=1)
    scenes = bench.make_frames(frames, 3, seed0=1000)
    gray = np.stack([s["gray"] for s in scenes])
    det = detect_3d_cuboid(ctx)
    det.set_calibration(scenes[0]["K"])
    det.yaw_step_deg = 0.5
    batch = CuboidBatch(ctx, gray, scenes[0]["K"], np.stack([s["Twc"] for s in scenes]), [s["boxes"] for s in scenes], [s["lines"] for s in scenes], det.opts())
    orb = ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, max_frames=frames, ctx=ctx)
    orb.upload(gray)
    lctx = [_lib.Context(0, priority=1) for _ in range(4)]
    lsds = [line_lbd_detect(640, 480, max_frames=frames, ctx=c) for c in lctx]
    for d in lsds:
        d.upload(gray)
    fe = Frontend(ctx, orb=orb, batch=batch, line_detectors=lsds)

    def barrier():
        fe.drain()
        for c in [ctx] + lctx:
            c.sync()
        torch.cuda.synchronize()

    fe.set_backlog(warmup)
    for _ in range(warmup):
        fe.step()
    barrier()
    for c in [ctx] + lctx:
        c.timing(True)
        c.timing_reset()
    t0 = time.perf_counter()
    fe.set_backlog(steps)
    for _ in range(steps):
        fe.step()
    barrier()
    elapsed = time.perf_counter() - t0
    walks = [c.timing_get("lsd_rg_seq") for c in lctx]
    scans = [c.timing_get("lsd_rg_cand_scan")[1] for c in lctx]
    enough, n_streams, n_queues = fe.queues()
    print(json.dumps({"hw_queues": n_queues, "streams": n_streams, "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": steps, "frames": frames,
                      "lsd_rg_seq_per_context": [n for _, n in walks], "lsd_rg_seq_avg_ms": [round(ms / max(n, 1), 2) for ms, n in walks],
                      "lsd_rg_cand_scan_per_context": scans, "frames_per_s": round(frames * steps / elapsed, 1), "ms_per_step": round(1e3 * elapsed / steps, 2)}))
    fe.close()


if __name__ == "__main__":
    main()
