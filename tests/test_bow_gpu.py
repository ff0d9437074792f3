"""Place recognition on the device against the restatement (tests/bow_restatement.py, pinned to the reference's text by tests/test_bow_restatement_pins.py): every pattern of
tests/bow_patterns.py through the C-ABI (cs_bow_*) and through cube_slam_amd.bow.  No tolerance anywhere: words, nodes and FeatureVectors equal entry for entry, BowVector
values and scores equal as 64-bit patterns, candidate lists equal in content and order."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import bow_patterns as P
from tests import bow_restatement as R

pytestmark = pytest.mark.gpu
VOCS = sorted(P.vocabularies())
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def expected(voc):
    """The restatement on every frame of the vocabulary's batch, computed once and shared."""
    v, up = P.vocabularies()[voc]
    return [R.transform(v, d, up) for d in P.batch(voc)]


@functools.lru_cache(maxsize=None)
def device_vocabulary(voc):
    from cube_slam_amd.bow import ORBVocabulary
    v, up = P.vocabularies()[voc]
    return ORBVocabulary(*v.arrays(), levelsup=up)


def _bits(bow):
    return [(w, np.float64(x).view(np.uint64)) for w, x in bow.items()]


def test_symbols_and_declarations(ctx):
    from cube_slam_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cubeslam_hip.h")).read(), flags=re.S)
    for name in ("cs_bow_vocab_create", "cs_bow_vocab_destroy", "cs_bow_vocab_info", "cs_bow_vocab_check", "cs_bow_transform", "cs_bow_score", "cs_bow_db_create", "cs_bow_db_add",
                 "cs_bow_db_erase", "cs_bow_db_clear", "cs_bow_db_size", "cs_bow_db_query", "cs_bow_db_destroy"):
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name


@pytest.mark.parametrize("voc", VOCS)
def test_transform_c_abi(ctx, voc):
    """cs_bow_transform on the mixed batch (an empty frame first, in the middle and last): per feature and per frame what the restatement gives."""
    dv = device_vocabulary(voc)
    assert dv.size() == P.vocabularies()[voc][0].n_words
    off, word, node, cnt, bw, bv = dv.transform_raw(P.batch(voc))
    for f, (bow, fv, w, n) in enumerate(expected(voc)):
        o, e = int(off[f]), int(off[f + 1])
        assert np.array_equal(word[o:e], w) and np.array_equal(node[o:e], n), (voc, f)
        rw, rx = R.bow_arrays(bow)
        assert cnt[f] == len(bow) and np.array_equal(bw[o:o + cnt[f]], rw), (voc, f)
        assert np.array_equal(R.bits(bv[o:o + cnt[f]]), R.bits(rx)), (voc, f)
        assert (bw[o + cnt[f]:e] == -1).all() and (bv[o + cnt[f]:e] == 0).all()


@pytest.mark.parametrize("voc", VOCS)
def test_transform_mirror_and_batch_equals_alone(ctx, voc):
    dv = device_vocabulary(voc)
    up = P.vocabularies()[voc][1]
    frames = P.batch(voc)
    got = dv.transform_batch(frames)
    raw = dv.transform_raw(frames)
    for f, ((bow, fv), (rbow, rfv, rword, rnode)) in enumerate(zip(got, expected(voc))):
        assert _bits(bow) == _bits(rbow) and list(fv.items()) == list(rfv.items()) and np.array_equal(fv.node, rnode), (voc, f)
        if f in (1, 3, 5, 8):  # a frame alone: byte for byte what the batch gave for it
            off, word, node, cnt, bw, bv = dv.transform_raw([frames[f]])
            o, e = int(raw[0][f]), int(raw[0][f + 1])
            assert cnt[0] == raw[3][f]
            for a, b in ((word, raw[1]), (node, raw[2]), (bw, raw[4]), (bv, raw[5])):
                assert a.tobytes() == b[o:e].tobytes(), (voc, f)
            abow, afv = dv.transform(frames[f], up)
            assert _bits(abow) == _bits(bow) and list(afv.items()) == list(fv.items())


def test_malformed_vocabularies_are_refused(ctx):
    from cube_slam_amd import _lib
    v, _ = P.vocabularies()["k5_L2_root"]
    for name, (k, L, parent, leaf, up, sc, we) in P.malformed().items():
        out = C.c_void_p(1)
        parent = np.ascontiguousarray(parent, np.int32); leaf = np.ascontiguousarray(leaf, np.uint8)
        u = P.vocabularies()["unbalanced"][0] if len(parent) != len(v.parent) else v
        r = _lib.lib().cs_bow_vocab_create(ctx.ptr, k, L, len(parent), _lib.ptr(parent), _lib.ptr(leaf), _lib.ptr(u.desc), _lib.ptr(u.weight), up, we, sc, C.byref(out))
        assert r == -2 and not out.value, name


@pytest.mark.parametrize("name", sorted(P.scenarios()))
def test_database_scenarios(ctx, name):
    """Every scenario through cube_slam_amd.bow.KeyFrameDatabase: the candidate lists of the restatement, and per query the (key frame, common words, smallest common word,
    score) of every key frame that shares a word."""
    from cube_slam_amd.bow import KeyFrameDatabase
    ops = P.scenarios()[name]
    db = KeyFrameDatabase(ctx=ctx)
    assert P.replay(ops, db) == P.replay(ops, R.KeyFrameDatabase(), R.KF)
    db.clear()
    live = {}
    for op in ops:
        if op[0] == "add":
            db.add(op[1], op[2]); live.pop(op[1], None); live[op[1]] = op[2]
        elif op[0] == "erase":
            db.erase(op[1]); live.pop(op[1], None)
        elif op[0] == "clear":
            db.clear(); live.clear()
        else:
            q = op[2]
            got = db.query([q])[0]
            want = [(i, len(set(q) & set(b)), min(set(q) & set(b)), R.score(q, b)) for i, b in live.items() if set(q) & set(b)]
            assert [(g[0], g[1], g[2], np.float64(g[4]).view(np.uint64)) for g in got] == [(i, c, m, np.float64(s).view(np.uint64)) for i, c, m, s in want]
            assert [g[3] for g in got] == sorted(g[3] for g in got)  # in add order
            assert db.size() == len(live)
    db.close()


def test_batched_query_equals_queries_alone_and_scores(ctx):
    from cube_slam_amd.bow import KeyFrameDatabase, ORBVocabulary
    ops = P.scenarios()["k65"]
    db = KeyFrameDatabase(ctx=ctx)
    bows = [op[2] for op in ops if op[0] == "add"]
    for op in ops:
        if op[0] == "add":
            db.add(op[1], op[2])
    queries = [op[2] for op in ops if op[0] in ("loop", "reloc")] + [{}, bows[3], {100000: 1.0}]
    together = db.query(queries)
    assert together == [db.query([q])[0] for q in queries]
    assert together[-3] == [] and together[-1] == [] and len(together[0]) > 32
    db.close()
    # cs_bow_score for explicit pairs (the minScore loop of LoopClosing::DetectLoop), a pair without a common word (-0.0) and a vector against itself among them
    voc = ORBVocabulary(ctx=ctx)
    vectors = bows[:12] + [{7: 1.0}, {}]
    pairs = [(a, b) for a in range(len(vectors)) for b in range(len(vectors))]
    got = voc.score_pairs(vectors, pairs)
    want = np.array([R.score(vectors[a], vectors[b]) for a, b in pairs])
    assert np.array_equal(R.bits(got), R.bits(want))
    assert np.float64(voc.score(vectors[0], vectors[-1])).view(np.uint64) == np.float64(-0.0).view(np.uint64)


def test_node_array_feeds_search_by_bow(ctx):
    """`node` of cs_bow_transform is the array cs_match_by_bow takes: the match list it gives is the one the restatement's FeatureVector gives."""
    from cube_slam_amd.matcher import ORBmatcher
    from cube_slam_amd.orb import KEYPOINT_DTYPE
    voc = "k10_L3_up1"
    v, up = P.vocabularies()[voc]
    rng = np.random.default_rng(5)
    descF = P.frames(voc)["n2000"][:600]
    descKF = np.stack([P._flip(rng, d, int(rng.integers(0, 20))) for d in descF[rng.permutation(600)[:500]]])
    got = device_vocabulary(voc).transform_batch([descKF, descF])
    def node_of(fv, n):
        a = np.full(n, -1, np.int32)
        for k, idx in fv.items():
            a[idx] = k
        return a
    ref = [node_of(R.transform(v, d, up)[1], len(d)) for d in (descKF, descF)]
    assert np.array_equal(got[0][1].node, ref[0]) and np.array_equal(got[1][1].node, ref[1])
    keys = lambda n: np.array([(rng.uniform(0, 640), rng.uniform(0, 480), 31, rng.uniform(0, 360), 1, 0, -1) for _ in range(n)], KEYPOINT_DTYPE)
    kK, kF = keys(len(descKF)), keys(len(descF))
    skip = (rng.random(len(descKF)) < 0.1).astype(np.uint8)
    m = ORBmatcher(0.9, False, ctx=ctx)
    a, na = m.SearchByBoW(kK, descKF, got[0][1].node, skip, kF, descF, got[1][1].node)
    b, nb = m.SearchByBoW(kK, descKF, ref[0], skip, kF, descF, ref[1])
    m.close()
    assert na == nb and np.array_equal(a, b) and na > 100
