#!/usr/bin/env python3
"""Times of Tracking::SearchLocalPoints on the device at the shape of bench.py's c3.local_map block (10 000 local map points, th 3) and of cs_track_local_points at
80 x 2 000 entries.  Prints one JSON line.

    python tools/track_local_bench.py [--points 10000] [--th 3] [--reps 20] [--warmup 3]

Two paths over the same map points, poses and frame, alternating:
  frustum   cs_match_local_map_frustum: isInFrustum, the query records and the search in one call
  parent    the path before that entry: Frame::isInFrustum on the host (numpy, vectorised over the points -- its logf is numpy's, which is why this is a timing and no parity
            run) and cs_match_local_map, which builds its query records on the host
*_wall_ms is the host clock around the whole path, host side included; *_kernels_ms the sum of the device-event times of its kernels (cs_timing_*), taken in repetitions of
their own.  The key points of five frames stand in for the map points, as in bench.py."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

W, H = 1241, 376
FX, FY, CX, CY, BF = 721.5377, 721.5377, 609.5593, 172.854, 386.1448
SEARCH_KERNELS = ("match_project_map", "match_candidates", "match_resolve")
POINT_KERNELS = ("tracklocal_first", "tracklocal_count", "tracklocal_bases", "tracklocal_emit")


def host_frustum(wp, nr, mn, mx, R, t, Ow, log_sf, n_levels, limit=0.5):
    """Frame::isInFrustum over all points at once, in float32 where the reference is."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        pc = (wp.astype(np.float64) @ R.astype(np.float64).reshape(3, 3).T + t.astype(np.float64)).astype(f32)
        invz = (f32(1.0) / pc[:, 2]).astype(f32)
        u = (f32(FX) * pc[:, 0] * invz + f32(CX)).astype(f32)
        v = (f32(FY) * pc[:, 1] * invz + f32(CY)).astype(f32)
        ok = (pc[:, 2] >= 0) & np.isfinite(u) & np.isfinite(v) & (u >= 0) & (u <= W) & (v >= 0) & (v <= H)
        po = (wp - Ow).astype(f32)
        dist = np.sqrt((po.astype(np.float64) ** 2).sum(1)).astype(f32)
        ok &= (dist >= f32(0.8) * mn) & (dist <= f32(1.2) * mx)
        cos = ((po.astype(np.float64) * nr.astype(np.float64)).sum(1) / dist.astype(np.float64)).astype(f32)
        ok &= cos >= f32(limit)
        lvl = np.ceil(np.log((mx / dist).astype(f32)) / f32(log_sf))
        ok &= (lvl >= 0) & (lvl < n_levels)
    return np.stack([u, v], axis=1), cos, np.where(ok, lvl, 0).astype(np.int32), ok.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--th", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.is_available()  # (torch's HIP runtime first, as bench.py does)
    from cube_slam_amd import _lib, synth
    from cube_slam_amd.matcher import ORBmatcher
    from cube_slam_amd.orb import ORBextractor
    from cube_slam_amd.tracking import track_local_points
    ctx = _lib.Context(0)
    ext = ORBextractor(2000, 1.2, 8, 20, 7, W, H, ctx=ctx)
    per = [ext(synth.texture_image(77, W, H, shift=2 * i)) for i in range(6)]
    pk = np.concatenate([k for k, _ in per[:5]])[:a.points]; pd = np.concatenate([d for _, d in per[:5]])[:a.points]
    n = len(pk)
    rng = np.random.default_rng(5)
    sf = np.float32(1.2) ** np.arange(8, dtype=np.float32)
    log_sf = float(np.float32(np.log(1.2)))
    z = rng.uniform(4, 40, n)
    x = pk["x"] + rng.normal(0, 1.0, n); y = pk["y"] + rng.normal(0, 1.0, n)
    wp = np.stack([(x - CX) / FX * z, (y - CY) / FY * z, z], axis=1).astype(np.float32)
    R, t, Ow = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32), np.zeros(3, np.float32)
    nr = (wp / np.linalg.norm(wp, axis=1, keepdims=True) + rng.normal(0, 0.03, (n, 3))).astype(np.float32)
    mx = (np.linalg.norm(wp, axis=1) * sf[np.clip(pk["octave"], 0, 7)] * rng.uniform(0.85, 1.0, n)).astype(np.float32)
    mn = (mx / sf[7]).astype(np.float32)
    zeros, ones = np.zeros(n, np.uint8), np.ones(n, np.uint8)
    m = ORBmatcher(0.8, True, ctx=ctx, max_queries=max(16384, n))
    m.set_frame(per[5][0], per[5][1], (0.0, float(W), 0.0, float(H)))

    def frustum():
        return m.SearchLocalPoints(R, t, Ow, wp, nr, mn, mx, zeros, ones, pd, FX, FY, CX, CY, BF, log_sf, sf, a.th)

    def parent():
        proj, cos, lvl, iv = host_frustum(wp, nr, mn, mx, R, t, Ow, log_sf, len(sf))
        return m.SearchByProjectionLocalMap(proj, cos, lvl, iv, ones, pd, sf, a.th)

    n_kf, per_kf = 80, 2000
    kf_mp = rng.integers(-1, 60000, n_kf * per_kf).astype(np.int32)
    kf_off = (np.arange(n_kf + 1) * per_kf).astype(np.int32)
    skip = (rng.uniform(size=60000) < 0.05).astype(np.uint8)

    def points():
        return track_local_points(ctx, kf_off, kf_mp, skip)

    out = {"points": n, "th": a.th, "reps": a.reps}
    for _ in range(a.warmup):
        r = frustum(); pm = parent(); lp = points()
    out["matches_frustum"], out["matches_parent"], out["n_to_match"], out["local_points"] = r["nmatches"], pm[1], r["n_to_match"], int(len(lp))
    wall = {"frustum": [], "parent": [], "points": []}
    for _ in range(a.reps):
        for name, fn in (("frustum", frustum), ("parent", parent), ("points", points)):
            ctx.sync(); t0 = time.perf_counter(); fn(); ctx.sync()
            wall[name].append(1e3 * (time.perf_counter() - t0))
    for name, v in wall.items():
        out[name + "_wall_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    for name, fn, kernels in (("frustum", frustum, SEARCH_KERNELS), ("parent", parent, SEARCH_KERNELS), ("points", points, POINT_KERNELS)):
        ctx.sync(); ctx.timing(True); ctx.timing_reset()
        for _ in range(a.reps):
            fn()
        ctx.sync()
        ks = {}
        for k in kernels:
            ms, cnt = ctx.timing_get(k)
            if cnt:
                ks[k + "_us"] = 1e3 * ms / a.reps
        ctx.timing(False)
        out[name + "_kernels_ms"] = sum(ks.values()) / 1e3
        out[name + "_kernels"] = ks
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
