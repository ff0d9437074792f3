#!/usr/bin/env python3
"""Time of place recognition on the device (cs_bow_transform, cs_bow_db_query) on a synthetic k = 10, L = 6 vocabulary (1 111 111 nodes, 10^6 words, 35.6 MB of
descriptors): the transform for 1, 64 and 1 024 frames of 2 000 features, and a query of 1 and 64 BowVectors against 2 000 and 20 000 key frames.  Where the reference tree is
present, --cpu also times the reference's own transform (the text tests/test_bow_restatement_pins.py compiles, built into a temporary directory) for one frame on one CPU thread
of this host.  Prints one JSON line.

    python tools/bow_bench.py [--frames 1,64,1024] [--features 2000] [--keyframes 2000,20000] [--queries 1,64] [--reps 10] [--warmup 2] [--cpu | --cpu-only]

*_wall_ms is the host clock around one call: uploads, kernels, downloads and the synchronise that ends it.  *_kernel_ms is the device-event time of the named kernel,
taken in repetitions of their own.  Every size is warmed up before it is timed."""
import argparse
import ctypes as C
import json
import os
import platform
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def synthetic_vocabulary(k, L, seed=7):
    """A full tree in breadth-first order: parent of node i is (i - 1) // k; the last level are the words."""
    rng = np.random.default_rng(seed)
    n = (k ** (L + 1) - 1) // (k - 1)
    parent = (np.arange(n, dtype=np.int64) - 1) // k
    parent[0] = 0
    first_leaf = (k ** L - 1) // (k - 1)
    is_leaf = (np.arange(n) >= first_leaf).astype(np.uint8)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    weight = np.where(is_leaf > 0, rng.random(n) * 9.0 + 0.25, 0.0)
    return k, L, parent.astype(np.int32), is_leaf, desc, weight


def synthetic_bow(rng, n_words, size):
    w = np.unique(rng.integers(0, n_words, size)).astype(np.int32)
    x = rng.random(len(w)) + 0.05
    return dict(zip(w.tolist(), (x / x.sum()).tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,64,1024")
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--keyframes", default="2000,20000")
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--words-per-keyframe", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu", action="store_true", help="also time the reference's transform on one CPU thread (needs the reference tree)")
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    k, L = 10, 6
    voc = synthetic_vocabulary(k, L)
    rng = np.random.default_rng(11)
    frames = [int(x) for x in args.frames.split(",")]
    out = {"what": "DBoW2 transform and key-frame database query", "k": k, "L": L, "features": args.features, "reps": args.reps, "warmup": args.warmup, "host": platform.node(),
           "cpu_model": next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "?")}
    one_frame = rng.integers(0, 256, (args.features, 32), dtype=np.uint8)
    if not args.cpu_only:
        import torch  # first: one copy of the HIP runtime in the process (see tests/conftest.py)
        torch.cuda.is_available()
        from cube_slam_amd import _lib
        from cube_slam_amd.bow import KeyFrameDatabase, ORBVocabulary
        ctx = _lib.Context(0)  # raises without a HIP device
        v = ORBVocabulary(*voc, levelsup=4, ctx=ctx)
        out["transform"] = {}
        for nf in frames:
            batch = [one_frame] + [rng.integers(0, 256, (args.features, 32), dtype=np.uint8) for _ in range(nf - 1)]
            for _ in range(args.warmup):
                v.transform_raw(batch)
            ts = []
            for _ in range(args.reps):
                t = time.perf_counter()
                v.transform_raw(batch)
                ts.append((time.perf_counter() - t) * 1e3)
            ctx.timing(True); ctx.timing_reset()
            k_reps = max(2, args.reps // 3)
            for _ in range(k_reps):
                v.transform_raw(batch)
            r = {"wall_ms": _stats(ts)}
            for name in ("bow_descend", "bow_accumulate"):
                ms, n = ctx.timing_get(name)
                r[name + "_kernel_ms"] = round(ms / max(n, 1), 4)
            ctx.timing(False)
            r["features_per_s_kernels"] = round(nf * args.features / ((r["bow_descend_kernel_ms"] + r["bow_accumulate_kernel_ms"]) * 1e-3))
            out["transform"][str(nf)] = r
        out["query"] = {}
        db = KeyFrameDatabase(ctx=ctx)
        n_have = 0
        queries = [synthetic_bow(rng, 10 ** L, args.words_per_keyframe) for _ in range(max(int(x) for x in args.queries.split(",")))]
        for nk in sorted(int(x) for x in args.keyframes.split(",")):
            while n_have < nk:
                db.add(n_have, synthetic_bow(rng, 10 ** L, args.words_per_keyframe))
                n_have += 1
            for nq in (int(x) for x in args.queries.split(",")):
                for _ in range(args.warmup):
                    db.query_raw(queries[:nq])
                ts = []
                for _ in range(args.reps):
                    t = time.perf_counter()
                    res = db.query_raw(queries[:nq])
                    ts.append((time.perf_counter() - t) * 1e3)
                ctx.timing(True); ctx.timing_reset()
                k_reps = max(2, args.reps // 3)
                for _ in range(k_reps):
                    db.query_raw(queries[:nq])
                ms, n = ctx.timing_get("bow_query")
                ctx.timing(False)
                out["query"]["%d x %d" % (nq, nk)] = {"wall_ms": _stats(ts), "bow_query_kernel_ms": round(ms / max(n, 1), 4), "pairs_sharing_a_word": len(res[0])}
        db.close(); v.close()
    if args.cpu or args.cpu_only:
        from tests import bow_restatement as R
        if not R.reference_available():
            out["reference_cpu"] = "the reference tree is not on this machine"
        else:
            with tempfile.TemporaryDirectory() as d:
                lib = R.build_reference(d)
                path = os.path.join(d, "voc.txt")
                kk, LL, parent, is_leaf, desc, weight = voc
                table = np.concatenate([parent[1:, None], is_leaf[1:, None], desc[1:]], axis=1).astype(np.int64)
                with open(path, "w") as f:
                    f.write("%d %d 0 0\n" % (kk, LL))
                    step = 100000
                    for a in range(0, len(table), step):
                        rows = [" ".join(map(str, r)) + " " + repr(float(w)) for r, w in zip(table[a:a + step].tolist(), weight[1 + a:1 + a + step].tolist())]
                        f.write("\n".join(rows) + ("\n" if a + step < len(table) else ""))
                t = time.perf_counter()
                h = C.c_void_p(lib.pin_voc_load(path.encode()))
                load_s = time.perf_counter() - t
                n = len(one_frame)
                bw, bv, fn, ff, nfv = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.float64), np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), C.c_int()
                p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
                ts = []
                for i in range(args.warmup + args.reps):
                    t = time.perf_counter()
                    lib.pin_transform(h, n, p(one_frame, C.c_uint8), 4, p(bw, C.c_int), p(bv, C.c_double), C.byref(nfv), p(fn, C.c_int), p(ff, C.c_int))
                    if i >= args.warmup:
                        ts.append((time.perf_counter() - t) * 1e3)
                out["reference_cpu"] = {"transform_one_frame_ms": _stats(ts), "threads": 1, "load_text_s": round(load_s, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
