#!/usr/bin/env python3
"""Time of the stereo association (cs_stereo_match_from_orb, Frame::ComputeStereoMatches) against the stage that feeds it: cs_orb_run over the same
2 x PAIRS frames.  Prints one JSON line.

    python tools/stereo_bench.py [--pairs 512] [--width 1241 --height 376 --features 2000] [--reps 10] [--warmup 2]

Two kinds of numbers, both after a warm-up of every shape and with the two calls alternating:
  *_wall_ms     host clock around the call and the synchronise that ends it (cs_orb_run waits for the device between its phases by itself)
  *_kernels_ms  the sum of the device-event times of the call's kernels (cs_timing_*), taken in repetitions of their own: per-kernel split
The bound the association is held to is `ratio < 1` (it must take less than the extraction that feeds it).  `pcie_bytes_per_pair_avoided` is computed from
the level sizes: the two pyramids a host implementation reads (mvImagePyramid of both extractors) and mvuRight going back up."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ORB_KERNELS = ("orb_resize", "orb_fast_score", "orb_cells", "orb_scan", "orb_quadtree", "orb_blur", "orb_angle", "orb_desc")
STEREO_KERNELS = ("stereo_prep", "stereo_match", "stereo_sad", "stereo_cut")


def make_pairs(n_pairs, W, H, n_bases=8):
    """n_pairs distinct rectified pairs: a band-limited texture cut at a column that moves from pair to pair, four horizontal bands of constant disparity
    in [2, 120) px (linear interpolation for the fraction), Gaussian noise (sigma 2) on both images."""
    from cube_slam_amd import synth
    bases = [synth._texture_base(1000 + i, W, H).astype(np.float32) for i in range(min(n_bases, n_pairs))]
    lefts, rights = np.zeros((n_pairs, H, W), np.uint8), np.zeros((n_pairs, H, W), np.uint8)
    band = H // 4
    for p in range(n_pairs):
        base = bases[p % len(bases)]
        rng = np.random.default_rng(p)
        s = 100 + 3 * (p // len(bases))
        left = base[:, s:s + W] + 2.0 * rng.standard_normal((H, W), dtype=np.float32)
        right = np.empty((H, W), np.float32)
        for k, d in enumerate(rng.uniform(2, 120, 4)):
            r0, r1 = k * band, (H if k == 3 else (k + 1) * band)
            i = int(np.floor(d))
            fr = np.float32(d - i)
            right[r0:r1] = (1 - fr) * base[r0:r1, s + i:s + i + W] + fr * base[r0:r1, s + i + 1:s + i + 1 + W]
        right += 2.0 * rng.standard_normal((H, W), dtype=np.float32)
        lefts[p] = np.clip(np.rint(left), 0, 255)
        rights[p] = np.clip(np.rint(right), 0, 255)
    return lefts, rights


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--width", type=int, default=1241)
    ap.add_argument("--height", type=int, default=376)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bf", type=float, default=386.1448)
    ap.add_argument("--fx", type=float, default=718.856)
    args = ap.parse_args()
    import torch  # first: one copy of the HIP runtime in the process (see tests/conftest.py)
    torch.cuda.is_available()
    from cube_slam_amd import _lib
    from cube_slam_amd.orb import ORBextractor
    from cube_slam_amd.stereo import StereoMatcher

    P, W, H = args.pairs, args.width, args.height
    lefts, rights = make_pairs(P, W, H)
    ctx = _lib.Context(0)  # raises without a HIP device
    orb = ORBextractor(args.features, 1.2, 8, 20, 7, W, H, max_frames=2 * P, ctx=ctx)  # both extractions in one run: left halves, then right halves
    orb.upload(np.concatenate([lefts, rights]))
    del lefts, rights
    st = StereoMatcher(orb.cap, P, ctx=ctx)
    b = args.bf / args.fx

    def run_orb():
        t = time.perf_counter()
        orb.run()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3

    def run_stereo():
        t = time.perf_counter()
        st.match(orb, orb, args.bf, b, left_first=0, right_first=P, n_pairs=P)
        ctx.sync()
        return (time.perf_counter() - t) * 1e3

    for _ in range(args.warmup):
        run_orb()
        run_stereo()
    t_orb, t_st = [], []
    for _ in range(args.reps):  # alternating
        t_orb.append(run_orb())
        t_st.append(run_stereo())
    # per-kernel device-event times, in repetitions of their own
    ctx.timing(True)
    ctx.timing_reset()
    k_reps = max(2, args.reps // 3)
    for _ in range(k_reps):
        run_orb()
        run_stereo()
    split = {}
    for name in ORB_KERNELS + STEREO_KERNELS:
        ms, n = ctx.timing_get(name)
        if n:
            split[name] = round(ms / k_reps, 4)
    ctx.timing(False)
    orb_k = sum(v for k, v in split.items() if k in ORB_KERNELS)
    st_k = sum(v for k, v in split.items() if k in STEREO_KERNELS)
    _, _, first, nm = st.read_packed()
    n_left = int(first[-1])
    level_bytes = sum(int(np.prod(orb.level(0, l).shape)) for l in range(orb.nlevels))
    so, ss = _stats(t_orb), _stats(t_st)
    out = {
        "what": "stereo association vs the extraction that feeds it", "pairs": P, "frames_extracted": 2 * P, "width": W, "height": H, "features": args.features,
        "left_keypoints": n_left, "matched": int(nm.sum()), "matched_share": round(float(nm.sum()) / max(n_left, 1), 4),
        "orb_run_wall_ms": so, "stereo_wall_ms": ss, "ratio_wall": round(ss["median"] / so["median"], 5),
        "orb_run_kernels_ms": round(orb_k, 4), "stereo_kernels_ms": round(st_k, 4), "ratio_kernels": round(st_k / orb_k, 5) if orb_k else None,
        "stereo_us_per_pair": round(1e3 * ss["median"] / P, 3), "kernel_ms": split, "kernel_reps": k_reps,
        "bound_met": bool(ss["median"] < so["median"] and ss["max"] < so["min"] and (not orb_k or st_k < orb_k)),
        "pcie_bytes_per_pair_avoided": {"pyramids_down": 2 * level_bytes, "u_right_up": 4 * (n_left // max(P, 1)), "total": 2 * level_bytes + 4 * (n_left // max(P, 1))},
    }
    print(json.dumps(out))
    st.close()
    orb.close()
    ctx.close()


if __name__ == "__main__":
    main()
