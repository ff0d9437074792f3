"""The window form of the frame-to-frame search, monocular against stereo, on the window of bench.py's c3 (1241 x 376, 2 000 ORB features per frame, th = 15):
cs_match_by_projection_stream (the monocular code, unchanged) and cs_match_by_projection_stream_stereo with a seeded mvuRight on 70 % of the key points and one direction per third
of the pairs (forward, backward, neither).  Per form: the call's wall time (median, min, max over the repetitions after warm-up), the device time of match_project /
match_candidates / match_resolve per call, and the candidates the windows enumerated -- for the stereo form AFTER the mvuRight test.  One JSON line.

    python tools/stereo_search_bench.py [--frames 64] [--reps 30] [--warmup 5] [--motion thirds|neither]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--motion", choices=["thirds", "neither"], default="thirds", help="thirds: forward, backward and neither, a third of the pairs each; neither: no pair moves by a baseline "
                    "(the level windows are then the monocular ones and the mvuRight test is the only difference)")
    a = ap.parse_args()
    from cube_slam_amd import _lib, synth
    from cube_slam_amd.matcher import ORBmatcherStream
    from cube_slam_amd.orb import ORBextractor
    W, H, frames = 1241, 376, a.frames
    fx, fy, cx, cy = 721.5377, 721.5377, 609.5593, 172.854
    bf, mb = 387.5744, 387.5744 / 721.5377
    ctx = _lib.Context(0)
    orb = ORBextractor(2000, 1.2, 8, 20, 7, W, H, max_frames=frames, ctx=ctx)
    orb.upload(synth.texture_stream(77, W, H, frames, step=3))
    orb.run()
    kall, _, first = orb.read_packed()
    n_pairs = frames - 1
    pk = kall[:first[n_pairs]]
    z = np.full(len(pk), 10.0, np.float32)
    wp = np.stack([(pk["x"] - 3.0 - cx) / fx * z, (pk["y"] - cy) / fy * z, z], axis=1).astype(np.float32)
    ones = np.ones(len(pk), np.uint8)
    K4 = np.array([fx, fy, cx, cy], np.float32)
    bounds = (0.0, float(W), 0.0, float(H))
    sf = np.array([1.2 ** i for i in range(8)], np.float32)
    Tcw = np.broadcast_to(np.eye(4, dtype=np.float32)[:3], (n_pairs, 3, 4)).copy()
    Tlw = Tcw.copy()
    if a.motion == "thirds":
        Tlw[:, 2, 3] = np.array([1.0, -1.0, 0.0], np.float32)[np.arange(n_pairs) * 3 // n_pairs]  # tlc.z = +1, -1, 0 m against a baseline of 0.54 m: a third of the pairs each
    n_train = int(first[frames] - first[1])
    tk = kall[first[1]:first[frames]]
    rng = np.random.default_rng(11)
    # the right coordinate a point 10 m away has (x - bf / 10) and up to 12 px of disparity error around it; the radius at level 0 is 15 px
    u_right = np.where(rng.uniform(size=n_train) < 0.7, tk["x"] - np.float32(bf / 10.0) + rng.uniform(-12.0, 12.0, n_train).astype(np.float32), np.float32(-1.0)).astype(np.float32)
    ms = ORBmatcherStream(True, ctx=ctx)
    base = (orb, 0, n_pairs, K4, None, bounds, wp, ones, ones, Tcw, fx, fy, cx, cy, sf, 15.0, n_train)
    forms = {"mono": lambda: ms.search(*base), "stereo": lambda: ms.search(*base, bMono=False, Tlw=Tlw, u_right=u_right, bf=bf, mb=mb)}
    out = {"frames": frames, "motion": a.motion, "pairs": n_pairs, "queries": int(len(pk)), "train": n_train, "u_right_share": round(float((u_right > 0).mean()), 3)}
    kernels = ("match_project", "match_candidates", "match_resolve")
    for name, call in forms.items():
        for _ in range(a.warmup):
            call()
        ctx.sync()
        wall = []
        for _ in range(a.reps):  # (every call ends with its own wait for the results: the wall time is the call's)
            t0 = time.perf_counter()
            _, nm = call()
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.timing(True); ctx.timing_reset()  # the kernels' device times in repetitions of their own: the events are not in the wall times above
        for _ in range(5):
            call()
        dev = {}
        for k in kernels:
            t_ms, n = ctx.timing_get(k)
            dev[k + "_us"] = round(1e3 * t_ms / max(n, 1), 2)
        ctx.timing(False)
        out[name] = dict(_stats(wall), matches=int(nm.sum()), candidates=ms.last_counts()["candidates"], **dev)
        if name == "stereo":
            d = np.asarray(ms.last_direction)
            out[name]["directions"] = [int((d == v).sum()) for v in (0, 1, 2)]
    out["stereo_over_mono"] = round(out["stereo"]["median_ms"] / out["mono"]["median_ms"], 4)
    print(json.dumps(out))
    ms.close(); orb.close()


if __name__ == "__main__":
    main()
