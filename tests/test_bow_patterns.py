"""Preconditions of tests/bow_patterns.py, asserted on the CPU through the restatement: every pattern really contains what it is named for."""
import numpy as np
import pytest

from tests import bow_patterns as P
from tests import bow_restatement as R

VOCS = sorted(P.vocabularies())


def test_vocabulary_shapes():
    V = P.vocabularies()
    v, up = V["k10_L3_full"]
    assert len(v.parent) == 1111 and v.n_words == 1000 and v.L - up <= 0
    v, up = V["k20_L2"]
    assert len(v.parent) == 421 and max(len(c) for c in v.children) == 20
    v, up = V["k3_L5_up4"]
    assert (v.k, v.L, up) == (3, 5, 4) and v.L - up == 1
    v, up = V["k5_L2_root"]
    assert v.L == 2 and up == 4
    v, up = V["unbalanced"]
    nid_level = v.L - up
    counts = {len(c) for c in v.children if c}
    leaf_depths = set(v.depth[v.is_leaf > 0].tolist())
    assert min(counts) < v.k and len(counts) > 2 and leaf_depths == set(range(nid_level, v.L + 1)) and nid_level > 0
    for name, (v, up) in V.items():
        assert R.refusal(v.k, v.L, v.parent, v.is_leaf, up) is None, name
        leaves = v.weight[v.is_leaf > 0]
        assert 0.1 < np.mean(leaves == 0) < 0.3, name  # about a fifth of the leaves are stop words


def test_ties_at_every_level():
    v, up = P.vocabularies()["ties"]
    f = P.frames("ties")
    seen = set()
    for d in np.concatenate([f["node_equal_and_midpoints"], f["n65"]]):
        node, level = 0, 0
        while v.children[node]:
            level += 1
            dist = R.POP[np.bitwise_xor(v.desc[v.children[node]], d[None, :])].sum(axis=1)
            if (dist == dist.min()).sum() > 1:
                seen.add(level)
            node = v.children[node][int(np.argmin(dist))]
    assert seen == {1, 2, 3}
    equal = sum(np.array_equal(v.desc[a], v.desc[b]) for c in v.children for a, b in zip(c, c[1:]))
    assert equal > 10


def test_malformed_inputs_are_the_five_kinds():
    kinds = {name: R.refusal(k, L, p, l, up, sc, we) for name, (k, L, p, l, up, sc, we) in P.malformed().items()}
    assert None not in kinds.values()
    assert set(kinds.values()) == {"leaf flag", "shallow leaf", "bounds", "parent", "weighting"}


@pytest.mark.parametrize("voc", VOCS)
def test_frames_contain_what_they_are_named_for(voc):
    v, up = P.vocabularies()[voc]
    f = P.frames(voc)
    assert [len(f["n%d" % n]) for n in (0, 1, 63, 64, 65, 2000)] == [0, 1, 63, 64, 65, 2000]
    bow, fv, word, node = R.transform(v, f["one_word"], up)
    assert len(bow) == 1 and len(word) > 64 and (word == word[0]).all() and word[0] >= 0 and list(bow.values()) == [1.0]
    bow, fv, word, node = R.transform(v, f["all_stopped"], up)
    assert len(bow) == 0 and len(fv) == 0 and len(word) > 64 and (word == -1).all() and (node == -1).all()
    d = f["node_equal_and_midpoints"]
    assert sum(any(np.array_equal(x, y) for y in v.desc[1:]) for x in d) >= 40
    bow, fv, word, node = R.transform(v, f["n2000"], up)
    assert (word >= 0).sum() > 1000 and (word < 0).sum() > 50 and len(bow) < (word >= 0).sum()  # kept and stopped features, and words met more than once
    nid_level = v.L - up
    assert all((v.depth[n] == max(nid_level, 0)) for n in fv)
    names = P.BATCH_ORDER
    assert names[0] == "n0" and names[-1] == "n0" and "n0" in names[1:-1] and {"one_word", "all_stopped", "n63", "n64", "n65", "n2000"} <= set(names)


def test_float_and_double_truncate_alike():
    """The issue asks for maxCommonWords values at which `* 0.8f` in float truncates differently from `* 0.8` in double.  The search finds none below 2^22 words, far beyond
    what a BowVector can hold; the scenario covers the multiples of 5 instead, where the product is a whole number and one word decides `>`."""
    m = np.arange(0, 1 << 22)
    f = (m.astype(np.float32) * np.float32(0.8)).astype(np.int64)
    assert np.array_equal(f, (m * 0.8).astype(np.int64)) and np.array_equal(f, (m * float(np.float32(0.8))).astype(np.int64))


def _replay_with_traces(name):
    db = R.KeyFrameDatabase()
    got, traces = [], []
    ops = P.scenarios()[name]
    kfs = {}
    for op in ops:
        if op[0] == "add":
            kfs.setdefault(op[1], R.KF(op[1], op[2]))
            db.add(kfs[op[1]])
        elif op[0] == "erase":
            db.erase(kfs[op[1]])
        elif op[0] == "clear":
            db.clear()
        else:
            if op[0] == "loop":
                ms = op[5]
                if isinstance(ms, tuple):
                    ms = float(np.float32(R.score(op[2], kfs[ms[1]].mBowVec)))
                got.append(db.DetectLoopCandidates(op[1], op[2], op[3], op[4], ms))
            else:
                got.append(db.DetectRelocalizationCandidates(op[1], op[2], op[3]))
            traces.append((op, dict(db.trace)))
    assert got == P.replay(ops, R.KeyFrameDatabase(), R.KF)
    return got, traces


def test_database_scenarios_contain_what_they_are_named_for():
    S = P.scenarios()
    assert {"empty", "one_key_frame", "k65", "erase_and_add_again", "no_common_word", "query_id_0", "score_at_minScore", "min_common_words", "reloc_twice", "same_best_twice"} == set(S)
    got, _ = _replay_with_traces("empty")
    assert got == [[], []]
    got, _ = _replay_with_traces("one_key_frame")
    assert got == [[1], [1]]
    got, tr = _replay_with_traces("k65")
    assert sum(o[0] == "add" for o in S["k65"]) == 65 and all(len(g) >= 1 for g in got[:3])
    assert all(len(t["sharing"]) > len(t["scored"]) > len(g) for g, (_, t) in zip(got[:3], tr[:3]))          # every filter removes something
    assert not set(tr[0][1]["sharing"]) & {2, 3, 5, 8}                                                       # the connected key frames are left out
    got, tr = _replay_with_traces("erase_and_add_again")
    assert got == [[11, 12], [12], [12, 11], [], [12]]
    got, tr = _replay_with_traces("no_common_word")
    assert got == [[], []] and tr[0][1]["sharing"] == []
    got, tr = _replay_with_traces("query_id_0")
    assert got[0] == [] and got[1] == [] and got[2] and got[3] and tr[0][1]["sharing"] == []
    assert tr[4][1]["sharing"] == [] and got[4] == []                                                        # a query id met again lists nothing
    got, tr = _replay_with_traces("score_at_minScore")
    for (op, t), kf in zip(tr, (2, 3)):
        ms = np.float32(R.score(op[2], [o for o in S["score_at_minScore"] if o[0] == "add" and o[1] == kf][0][2]))
        assert any(np.float32(si) == ms and i == kf for si, i in t["scored"]) and any(np.float32(si) > ms for si, i in t["scored"])
    got, tr = _replay_with_traces("min_common_words")
    assert [t["max"] for _, t in tr[::2]] == [5, 10, 15, 35, 34, 36] and [t["min"] for _, t in tr[::2]] == [4, 8, 12, 28, 27, 28]
    for _, t in tr:
        w = sorted(t["words"].values())
        assert t["min"] in w and t["min"] + 1 in w and len(t["scored"]) < len(t["sharing"])                # a key frame exactly at minCommonWords is dropped, the next kept
    got, tr = _replay_with_traces("reloc_twice")
    left = tr[1][1]["left_by_earlier_query"]
    assert left and all(s != 0.0 for _, s in left) and {i for i, _ in left} <= {i for _, i in tr[0][1]["scored"]}
    assert tr[0][1]["left_by_earlier_query"] == [(1, 0.0)]  # ... and the first reads a value no query has written: the reference's constructor leaves it uninitialised, here it is 0
    got, tr = _replay_with_traces("same_best_twice")
    for g, (_, t) in zip(got, tr):
        best = [i for _, i in t["acc"]]
        assert best.count(3) >= 2 and g.count(3) == 1
