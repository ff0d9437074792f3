"""CPU: what cube_slam_amd.bow and cube_slam_amd/host/bow.hpp do on the host -- the reference's text format, the vocabularies cs_bow_vocab_create refuses, and the logic of
DetectLoopCandidates / DetectRelocalizationCandidates behind the scores, fed with the restatement's scores -- against tests/bow_restatement.py."""
import numpy as np
import pytest

from tests import bow_cpp_driver as D
from tests import bow_patterns as P
from tests import bow_restatement as R


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return D.build(tmp_path_factory.mktemp("bow_mirror"))


def test_symbols_and_declarations():
    import os
    import re
    from cube_slam_amd import _lib
    import cube_slam_amd
    assert hasattr(cube_slam_amd, "ORBVocabulary") and hasattr(cube_slam_amd, "KeyFrameDatabase")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(D.ROOT, "include", "cubeslam_hip.h")).read(), flags=re.S)
    for name in ("cs_bow_vocab_create", "cs_bow_vocab_destroy", "cs_bow_vocab_info", "cs_bow_vocab_check", "cs_bow_transform", "cs_bow_score", "cs_bow_db_create", "cs_bow_db_add",
                 "cs_bow_db_erase", "cs_bow_db_clear", "cs_bow_db_size", "cs_bow_db_query", "cs_bow_db_destroy"):
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name


@pytest.mark.parametrize("voc", ["k5_L2_root", "unbalanced", "ties", "k20_L2"])
def test_text_loader(exe, tmp_path, voc):
    from cube_slam_amd.bow import parse_vocabulary_text
    v, up = P.vocabularies()[voc]
    lines = []
    for newline in (False, True):  # a final empty line is ignored (the reference turns it into one more node; tests/test_bow_restatement_pins.py)
        text = R.to_text(v, trailing_newline=newline)
        k, L, n1, n2, parent, leaf, desc, weight = parse_vocabulary_text(text)
        assert (k, L, n1, n2) == (v.k, v.L, 0, 0)
        assert np.array_equal(parent, v.parent) and np.array_equal(leaf, v.is_leaf) and np.array_equal(desc, v.desc) and np.array_equal(R.bits(weight), R.bits(v.weight))
        r = R.load_text(text)
        assert np.array_equal(r.parent, v.parent) and np.array_equal(R.bits(r.weight), R.bits(v.weight)) and np.array_equal(r.word_id, v.word_id)
        path = tmp_path / ("voc%d.txt" % newline)
        path.write_text(text)
        lines.append("voc %s %d" % (path, up))
    want = "voc 1 %d %d 0 0 %d %s 0" % (v.k, v.L, len(v.parent), D.fnv(v.parent.astype(np.int32), v.is_leaf, v.desc, v.weight))
    assert D.run(exe, "host", lines, tmp_path) == [want, want]


def test_refused_vocabularies(exe, tmp_path):
    from cube_slam_amd.bow import ORBVocabulary
    from cube_slam_amd._lib import CubeSlamError
    v, _ = P.vocabularies()["k5_L2_root"]
    u, _ = P.vocabularies()["unbalanced"]
    lines = []
    for name, (k, L, parent, leaf, up, sc, we) in P.malformed().items():
        src = v if len(parent) == len(v.parent) else u
        assert R.refusal(k, L, parent, leaf, up, sc, we) is not None
        with pytest.raises(CubeSlamError):
            ORBVocabulary(k, L, parent, leaf, src.desc, src.weight, levelsup=up, scoring=sc, weighting=we)
        path = tmp_path / ("bad%d.txt" % len(lines))
        path.write_text(R.arrays_to_text(k, L, sc, we, parent, leaf, src.desc, src.weight))
        lines.append("voc %s %d" % (path, up))
    out = D.run(exe, "host", lines, tmp_path)
    assert len(out) == len(lines) and all(o.split()[-1] == "1" for o in out), out


@pytest.mark.parametrize("name", sorted(P.scenarios()))
def test_candidate_logic(exe, tmp_path, name):
    """The host logic behind the scores, in Python and in C++, fed with what cs_bow_db_query has to return (computed by the restatement)."""
    import collections
    from cube_slam_amd import bow
    ops = P.scenarios()[name]
    want = P.replay(ops, R.KeyFrameDatabase(), R.KF)
    shared = D.shared_words(ops)
    queries = [op for op in ops if op[0] in ("loop", "reloc")]
    state = collections.defaultdict(bow._KFState)
    got, lines = [], []
    for op, sh in zip(queries, shared):
        sh_txt = ",".join("%d.%d.%d.%d.%s" % (i, c, m, o, D.hex64(s)) for i, c, m, o, s in sh) or "-"
        if op[0] == "loop":
            ms = D.min_score(ops, op)
            got.append(bow.candidates_loop(state, sh, op[1], op[3], op[4], ms))
            lines.append("cloop %d %s %s %s %s" % (op[1], D.hex32(ms), D.ids(op[3]), D.cov(op[4]), sh_txt))
        else:
            got.append(bow.candidates_reloc(state, sh, op[1], op[3]))
            lines.append("creloc %d %s %s" % (op[1], D.cov(op[3]), sh_txt))
    assert got == want
    assert [D.cand(x) for x in D.run(exe, "host", lines, tmp_path)] == want
