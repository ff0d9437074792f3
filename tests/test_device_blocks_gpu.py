"""GPU: no entry point of csrc keeps a device block it should have released.

Ownership of device blocks lies with cs_owner / cs_scratch (csrc/common.h).  The parity tests cannot see a block that is never released, so this file
repeats every small handle's create / destroy and every one-shot call REPEATS times and compares the device's free memory (torch.cuda.mem_get_info)
with what it was after one warm-up pass.

The allowed drop, measured on an MI355X with the loops below run against the commit before cs_owner moved into common.h (every entry point exists there):
  largest drop of free memory over three runs of all parts, at 200, 1000 and 2560 repeats each ...... PARENT_DROP = 0 bytes (every part, every run)
  what mem_get_info moves by for 4-byte hipMallocs (the driver's granule) ........................... GRANULE = 2 097 152 bytes
  ALLOWED_DROP = PARENT_DROP + GRANULE = 2 097 152 bytes.
The granule: the runtime carves small blocks out of 2 MiB chunks, 4 KiB apiece.  One 4-byte hipMalloc alone moved free memory by 0 (three times out of three); held
one after the other, 4-byte blocks moved it by 2 097 152 bytes at the 257th and again at every 512th after it (twice the same), and by nothing in between.  So 2 MiB is
the only step there is, and a pass that merely tips into the next chunk is not a leak.
REPEATS: a block leaked once per call must cost at least four times ALLOWED_DROP.  200 held 4-byte blocks cost 0 bytes and 1000 cost 4 MiB, which is too few; 2560 cost
10 485 760 bytes = 5 x ALLOWED_DROP (measured in the same session), so every loop runs 2560 times.  A part takes 0.1 to 0.4 s at that count.

cs_cuboid_batch is the one handle that is re-planned while it lives: its parts (cuboid_batch_parts) take it through create / destroy, through every growth path of batch_reserve
and down its refusals.  The same loops against the commit before batch_reserve, 2560 repeats each, on an MI355X: drop of free memory 0 bytes in every part (so PARENT_DROP
stays 0); seconds per part: create_destroy 0.31, create_set_scene_destroy 0.97, alternate_set_scene 0.18, alternate_set_lines 0.13, refuse_create 0.05, refuse_set_scene 0.56.
refuse_offsets could not run there: that commit read boxes and lines by whatever offsets it was handed."""
import ctypes as C

import numpy as np
import pytest

from cube_slam_amd import synth
from cube_slam_amd._lib import CubeSlamError, lib
from cube_slam_amd.bow import KeyFrameDatabase, ORBVocabulary
from cube_slam_amd.cuboid import CuboidBatch, detect_3d_cuboid
from cube_slam_amd.matcher import ORBmatcher
from cube_slam_amd.optimizer import EssentialGraph, OptimizeSim3, correct_points, sim3_log
from cube_slam_amd.stereo import StereoMatcher

gpu = pytest.mark.gpu

PARENT_DROP = 0
GRANULE = 2 << 20
ALLOWED_DROP = PARENT_DROP + GRANULE
REPEATS = 2560
CS_ERR_BAD_ARG, CS_ERR_CAPACITY = -2, -4


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def drop_after(fn, repeats):
    """One warm-up pass of fn, then how far free memory fell over `repeats` more."""
    fn()
    base = free_bytes()
    for _ in range(repeats):
        fn()
    return base - free_bytes()


# ---- the smallest legal inputs ----------------------------------------------------------------------------------------------------------------------
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float64)  # tx ty tz qx qy qz qw s
CHAIN = {"Scw": np.tile(IDENTITY, (3, 1)), "edge_i": [1, 2], "edge_j": [0, 1], "edge_kind": [1, 1], "fixed_vertex": 0}  # three key frames, each linked to the one before
BOW_A, BOW_B = {0: 0.5, 1: 0.5}, {1: 1.0}
SIM3 = {"P1c": [[0, 0, 4], [1, 0, 5], [0, 1, 6]], "P2c": [[0, 0, 4], [1, 0, 5], [0, 1, 6]], "obs1": [[320, 240], [420, 240], [320, 323]], "obs2": [[320, 240], [420, 240], [320, 323]],
        "inv_sigma2_1": [1, 1, 1], "inv_sigma2_2": [1, 1, 1], "intrinsics": [500, 500, 320, 240] * 2, "sim3_in": IDENTITY, "th2": 10.0, "fix_scale": False}


def tiny_vocabulary(ctx):  # k = 2, L = 1: a root and two words
    desc = np.zeros((3, 32), np.uint8)
    desc[2] = 255
    return ORBVocabulary(2, 1, [0, 0, 0], [0, 1, 1], desc, [0.0, 1.0, 1.0], ctx=ctx)


def db_query_with_cap(ctx, db, bows, cap):
    """cs_bow_db_query with room for `cap` pairs -> (status, pairs that share a word)"""
    w = np.concatenate([np.fromiter(b.keys(), np.int32) for b in bows]); x = np.concatenate([np.fromiter(b.values(), np.float64) for b in bows])
    off = np.zeros(len(bows) + 1, np.int32)
    off[1:] = np.cumsum([len(b) for b in bows])
    n = max(cap, 1)
    oq, oc, om = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    oid, oord, osc = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
    found = C.c_long()
    r = lib().cs_bow_db_query(ctx.ptr, db._db, len(bows), _p(off, C.c_int), _p(w, C.c_int), _p(x, C.c_double), C.c_long(cap), C.byref(found), _p(oq, C.c_int), _p(oid, C.c_long),
                              _p(oord, C.c_long), _p(oc, C.c_int), _p(om, C.c_int), _p(osc, C.c_double))
    return r, found.value


# ---- one pass of every part -------------------------------------------------------------------------------------------------------------------------
def handle_parts(ctx):
    def vocab():
        tiny_vocabulary(ctx).close()

    words, values = np.arange(1 << 16, dtype=np.int32), np.ones(1 << 16)

    def db():
        d = KeyFrameDatabase(ctx)
        d.add(1, {0: 0.25, 1: 0.25, 2: 0.25, 3: 0.25})  # the first add allocates the pool (65 536 entries)
        # 65 536 more do not fit behind the first four: bow_db_reserve allocates a new pair, copies and frees the old one
        assert lib().cs_bow_db_add(ctx.ptr, d._db, C.c_long(2), len(words), _p(words, C.c_int), _p(values, C.c_double)) == 0 and d.size() == 2
        d.close()

    def stereo():
        StereoMatcher(1, 1, ctx=ctx).close()

    def graph():
        EssentialGraph(CHAIN, True, ctx=ctx).close()

    def matcher():
        ORBmatcher(ctx=ctx, max_keypoints=1, max_queries=1, max_candidates=1).close()

    return {"cs_bow_vocab": vocab, "cs_bow_db": db, "cs_stereo": stereo, "cs_essential_graph": graph, "cs_matcher": matcher}


def call_parts(ctx, voc, db):
    one = np.zeros((1, 32), np.uint8)
    return {"cs_bow_transform": lambda: voc.transform_raw([one]),
            "cs_bow_score": lambda: voc.score_pairs([BOW_A, BOW_B], [(0, 1)]),
            "cs_bow_db_query": lambda: db.query_raw([BOW_B]),
            "cs_sim3_optimization": lambda: OptimizeSim3(SIM3, ctx=ctx),
            "cs_sim3_correct_points": lambda: correct_points([[1.0, 2.0, 3.0]], [2], CHAIN["Scw"], CHAIN["Scw"], ctx=ctx),
            "cs_sim3_log": lambda: sim3_log(IDENTITY, ctx=ctx)}


def refusal_parts(ctx, voc, db):
    """Each one-shot call down an ordinary refusal.  cs_bow_db_query is the one call that refuses after its scratch was allocated (more sharing pairs than
    `cap`); the others check their arguments first, and are held to leaving nothing behind all the same."""
    def raises(fn):
        with pytest.raises(CubeSlamError):
            fn()

    def query():
        assert db_query_with_cap(ctx, db, [BOW_B, BOW_A], 1) == (CS_ERR_CAPACITY, 4)

    return {"cs_bow_transform": lambda: raises(lambda: voc.transform_raw([np.zeros((8193, 32), np.uint8)])),  # CS_ERR_CAPACITY: more than 8192 features in one frame
            "cs_bow_score": lambda: raises(lambda: voc.score_pairs([BOW_A, BOW_B], [(0, 2)])),  # a pair outside the vectors
            "cs_bow_db_query": query,
            "cs_sim3_optimization": lambda: _sim3_refusal(ctx),
            "cs_sim3_correct_points": lambda: raises(lambda: correct_points([[1.0, 2.0, 3.0]], [3], CHAIN["Scw"], CHAIN["Scw"], ctx=ctx)),  # a reference vertex outside the graph
            "cs_sim3_log": lambda: _expect(lib().cs_sim3_log(ctx.ptr, -1, None, None), CS_ERR_BAD_ARG)}


def _expect(status, want):
    assert status == want


def _sim3_refusal(ctx):  # correspondence offsets that decrease
    off = np.array([0, -1], np.int32)
    z = np.zeros(8)
    _expect(lib().cs_sim3_optimization(ctx.ptr, 1, _p(off, C.c_int), None, None, None, None, None, None, _p(z, C.c_double), _p(z, C.c_double), _p(np.zeros(1, np.float32), C.c_float),
                                       _p(np.zeros(1, np.uint8), C.c_uint8), _p(z, C.c_double), None, _p(np.zeros(1, np.int32), C.c_int)), CS_ERR_BAD_ARG)


# ---- cs_cuboid_batch: the handle whose arrays are re-planned while it lives -----------------------------------------------------------------------
# One 128 x 96 frame of zeros (content does not matter for ownership) and the box (30, 20, 60, 50): ew = 10, the ROI (20, 10) .. (100, 80) lies inside the image, nine top samples.
CB_GRAY = np.zeros((1, 96, 128), np.uint8)
CB_T = synth.camera_pose(height=1.1, pitch_deg=25.0, yaw_deg=0.0)[None]
CB_LINES = np.array([[22.0 + 3 * i, 12.0, 24.0 + 3 * i, 78.0] for i in range(24)])
CB_SMALL = ([np.array([[30.0, 20.0, 60.0, 50.0, 0.9]])], [CB_LINES[:4]])  # (boxes of every frame, lines of every frame)
CB_LARGE = ([np.array([[30.0, 20.0, 60.0, 50.0, 0.9], [10.0, 10.0, 40.0, 40.0, 0.9], [60.0, 30.0, 50.0, 50.0, 0.9]])], [CB_LINES])  # three units, six times the lines: every size class grows
CB_OUTSIDE = ([np.array([[200.0, 20.0, 60.0, 50.0, 0.9]])], [CB_LINES[:4]])  # roi_x = 190 lies right of the last column


def cb_create(ctx, scene):
    return CuboidBatch(ctx, CB_GRAY, synth.K_TUM, CB_T, scene[0], scene[1], detect_3d_cuboid(ctx).opts())


def cb_refused(fn):
    with pytest.raises(CubeSlamError, match="CS_ERR_BAD_ARG"):
        fn()


def cb_runs_and_reads(b):
    b.run()
    assert len(b.read()) == b.n_boxes


def cuboid_batch_parts(ctx, small, lines):
    """small: a batch created on CB_SMALL that the alternating set_scene part grows once; lines: another one for the alternating set_lines part"""
    def create_destroy():
        cb_create(ctx, CB_SMALL).close()

    def create_grow_destroy():
        b = cb_create(ctx, CB_SMALL)
        b.set_scene(CB_T, *CB_LARGE)
        b.close()

    def alternate_scenes():
        small.set_scene(CB_T, *CB_LARGE)
        small.set_scene(CB_T, *CB_SMALL)

    def alternate_lines():
        lines.set_lines(CB_LARGE[1])
        lines.set_lines(CB_SMALL[1])

    def refuse_create():
        cb_refused(lambda: cb_create(ctx, CB_OUTSIDE))

    def refuse_scene():
        cb_refused(lambda: small.set_scene(CB_T, *CB_OUTSIDE))
        cb_runs_and_reads(small)

    def refuse_offsets():  # what cs_frontend_stream_push_scene hands on: box offsets that decrease, line offsets that do not start at 0
        T, bo, boxes, lo, ln = CuboidBatch.pack_scene(CB_T, *CB_SMALL)
        cb_refused(lambda: small.set_scene(None, None, packed=(T, np.array([0, -1], np.int32), boxes, lo, ln)))
        cb_refused(lambda: small.set_scene(None, None, packed=(T, bo, boxes, np.array([1, 4], np.int32), ln)))
        cb_runs_and_reads(small)

    return {"create_destroy": create_destroy, "create_set_scene_destroy": create_grow_destroy, "alternate_set_scene": alternate_scenes, "alternate_set_lines": alternate_lines,
            "refuse_create": refuse_create, "refuse_set_scene": refuse_scene, "refuse_offsets": refuse_offsets}


@pytest.fixture(scope="module")
def resident(ctx):
    """a vocabulary and a database of two key frames for the one-shot calls"""
    voc, db = tiny_vocabulary(ctx), KeyFrameDatabase(ctx)
    db.add(1, BOW_A)
    db.add(2, BOW_B)
    yield voc, db
    db.close()
    voc.close()


def check_drop(name, drop):
    print("%s: free memory fell by %d bytes (allowed %d)" % (name, drop, ALLOWED_DROP))
    assert drop <= ALLOWED_DROP, name


@gpu
@pytest.mark.parametrize("name", ["cs_bow_vocab", "cs_bow_db", "cs_stereo", "cs_essential_graph", "cs_matcher"])
def test_create_destroy_returns_every_block(ctx, name):
    check_drop(name, drop_after(handle_parts(ctx)[name], REPEATS))


@gpu
@pytest.mark.parametrize("name", ["cs_bow_transform", "cs_bow_score", "cs_bow_db_query", "cs_sim3_optimization", "cs_sim3_correct_points", "cs_sim3_log"])
def test_one_shot_calls_return_their_scratch(ctx, resident, name):
    check_drop(name, drop_after(call_parts(ctx, *resident)[name], REPEATS))
    fn = refusal_parts(ctx, *resident)[name]
    base = free_bytes()
    fn()
    check_drop(name + " refused", base - free_bytes())


@gpu
@pytest.mark.parametrize("name", ["create_destroy", "create_set_scene_destroy", "alternate_set_scene", "alternate_set_lines", "refuse_create", "refuse_set_scene", "refuse_offsets"])
def test_cuboid_batch_returns_every_block(ctx, name):
    """cs_cuboid_batch through create, reserve (set_scene, set_lines) and destroy, and down each refusal; every part has batches of its own, so none hides another's leak"""
    small, lines = cb_create(ctx, CB_SMALL), cb_create(ctx, CB_SMALL)
    try:
        check_drop("cs_cuboid_batch " + name, drop_after(cuboid_batch_parts(ctx, small, lines)[name], REPEATS))
        cb_runs_and_reads(small)
        cb_runs_and_reads(lines)
    finally:
        small.close()
        lines.close()


@gpu
def test_unpooled_blocks_come_and_go_beside_the_pool(ctx, resident):
    """cs_cuboid_detect leaves its batch's blocks in the context's pool; a call that takes and returns unpooled blocks must neither disturb them nor be kept by it."""
    voc, _ = resident
    s = synth.cuboid_scene(synth.SEED, n_boxes=3)
    det = detect_3d_cuboid(ctx)
    det.set_calibration(s["K"])
    detect = lambda: det.detect_cuboid(s["gray"], s["Twc"], s["boxes"], s["lines"])
    detect()  # (warm-up: the pool is filled)
    voc.score_pairs([BOW_A, BOW_B], [(0, 1)])
    base = free_bytes()
    first = detect()
    score = voc.score_pairs([BOW_A, BOW_B], [(0, 1)])
    second = detect()
    check_drop("cs_cuboid_detect, cs_bow_score, cs_cuboid_detect", base - free_bytes())
    assert score[0] == voc.score(BOW_A, BOW_B)
    assert len(first) == len(second) == 3 and all(len(a) >= 1 and a.tobytes() == b.tobytes() for a, b in zip(first, second))
