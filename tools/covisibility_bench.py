"""Times of cs_covisibility_update and cs_keyframe_culling on one MI355X, beside their host forms on one thread.
  case 1: 64 queries x 2 000 slots x 8 observations over 2 000 key frames -- the UpdateConnections calls of a LoopClosing::CorrectLoop
  case 2: 40 local key frames of 2 000 slots with 0, 1 and 4 erasing ones -- LocalMapping::KeyFrameCulling
Device and restatement must agree at these sizes before anything is timed.  Per case: the kernels' times (hipEvent pairs, a run of their own), the call's wall time (median of
10) and the host form's, and the number of culling rounds.  One JSON line per case.
  usage: python tools/covisibility_bench.py [--repeats 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("covis_vote_count", "covis_offsets", "covis_vote_emit", "covis_cull_init", "covis_cull_eval", "covis_cull_erase")


def loop_map(rng, n_kf=2000, n_query=64, n_slots=2000, n_obs=8):
    """Every queried key frame holds n_slots points of its own, each seen by it and n_obs - 1 key frames near it."""
    queries = np.sort(rng.choice(n_kf, n_query, replace=False)).astype(np.int32)
    obs_kf, kf_mp = [], []
    for q, kf in enumerate(queries):
        near = np.setdiff1d(np.clip(np.arange(kf - 40, kf + 41), 0, n_kf - 1), [kf])
        for s in range(n_slots):
            obs_kf.append(np.sort(np.concatenate([[kf], rng.choice(near, n_obs - 1, replace=False)])))
        kf_mp.append(np.arange(q * n_slots, (q + 1) * n_slots))
    n_points = n_query * n_slots
    t = dict(n_kf=n_kf, n_points=n_points, obs_off=(np.arange(n_points + 1) * n_obs).astype(np.int32), obs_kf=np.concatenate(obs_kf).astype(np.int32),
             obs_octave=np.zeros(n_points * n_obs, np.int32), obs_stereo=np.zeros(n_points * n_obs, np.uint8), mp_nobs=np.full(n_points, n_obs, np.int32),
             mp_flags=np.zeros(n_points, np.uint8))
    return t, queries, (np.arange(n_query + 1) * n_slots).astype(np.int32), np.concatenate(kf_mp).astype(np.int32)


def culling_map(n_erasing, n_local=40, n_slots=2000):
    """n_local key frames with n_slots points of their own each.  An erasing key frame's points are seen by it and four key frames outside the list; the others' by two."""
    erasing = set(np.linspace(3, n_local - 4, n_erasing).astype(int).tolist()) if n_erasing else set()
    outside = [n_local + k for k in range(4)]
    obs_kf, off = [], [0]
    for kf in range(n_local):
        seen = [kf] + (outside if kf in erasing else outside[:2])
        for s in range(n_slots):
            obs_kf += seen
            off.append(len(obs_kf))
    n_points = n_local * n_slots
    t = dict(n_kf=n_local + 4, n_points=n_points, obs_off=np.array(off, np.int32), obs_kf=np.array(obs_kf, np.int32), obs_octave=np.zeros(len(obs_kf), np.int32),
             obs_stereo=np.zeros(len(obs_kf), np.uint8), mp_nobs=np.diff(off).astype(np.int32), mp_flags=np.zeros(n_points, np.uint8))
    return dict(kind="cull", t=t, local_kf=np.arange(n_local, dtype=np.int32), kf_off=(np.arange(n_local + 1) * n_slots).astype(np.int32), kf_mp=np.arange(n_points, dtype=np.int32),
                slot_octave=np.zeros(n_points, np.int32), slot_depth=np.ones(n_points, np.float32), kf_th_depth=np.full(n_local, 40.0, np.float32), monocular=1,
                kf_flags=np.zeros(n_local, np.uint8), th_obs=3), len(erasing)


def median_ms(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        a = time.perf_counter()
        fn()
        times.append((time.perf_counter() - a) * 1e3)
    return float(np.median(times))


def kernel_ms(ctx, fn):
    ctx.timing(True); ctx.timing_reset()
    fn()
    out = {}
    for k in KERNELS:
        ms, n = ctx.timing_get(k)
        if n:
            out[k] = dict(ms=round(ms, 4), launches=n)
    ctx.timing(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    import torch
    torch.cuda.is_available()  # torch's HIP runtime first, as in bench.py
    from cube_slam_amd import _lib
    from cube_slam_amd.covisibility import KeyFrameCulling, covisibility_update
    from tests import covisibility_patterns as P
    from tests import covisibility_restatement as R
    ctx = _lib.Context(0)

    t, queries, kf_off, kf_mp = loop_map(np.random.default_rng(5))
    table = P.obs_table(t)
    got = covisibility_update(ctx, table, queries, kf_off, kf_mp)
    P.assert_equal(got, P.flat_vote(R.update_connections(t, queries, kf_off, kf_mp, 0, 15)), P.VOTE_KEYS, "case 1")
    cap = int(got["cnt_off"][-1])
    print(json.dumps(dict(case="update_connections", queries=len(queries), slots=2000, observations=8, key_frames=2000, counters=cap, ordered=int(got["ord_off"][-1]),
                          kernels=kernel_ms(ctx, lambda: covisibility_update(ctx, table, queries, kf_off, kf_mp, conn_cap=cap)),
                          call_ms=round(median_ms(lambda: covisibility_update(ctx, table, queries, kf_off, kf_mp, conn_cap=cap), a.repeats), 3),
                          host_ms=round(median_ms(lambda: covisibility_update(None, table, queries, kf_off, kf_mp, conn_cap=cap), a.repeats), 3))))

    for n_erasing in (0, 1, 4):
        c, n = culling_map(n_erasing)
        want = R.keyframe_culling(c["t"], c["local_kf"], c["kf_off"], c["kf_mp"], c["slot_octave"], c["slot_depth"], c["kf_th_depth"], 1, c["kf_flags"], 3)
        got = P.run_cull(ctx, c)
        P.assert_equal(got, want, P.CULL_KEYS, "case 2, %d erasing" % n_erasing)
        assert int((want["verdict"] == 1).sum()) == n
        print(json.dumps(dict(case="keyframe_culling", local_key_frames=40, slots=2000, erasing=n, rounds=got["n_rounds"], kernels=kernel_ms(ctx, lambda: P.run_cull(ctx, c)),
                              call_ms=round(median_ms(lambda: P.run_cull(ctx, c), a.repeats), 3), host_ms=round(median_ms(lambda: P.run_cull(None, c), a.repeats), 3))))
    ctx.close()


if __name__ == "__main__":
    main()
