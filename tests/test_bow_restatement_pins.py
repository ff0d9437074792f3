"""The judge of the place-recognition tests (tests/bow_restatement.py) against the reference's own text: FORB::distance and fromString, BowVector.cpp, FeatureVector.cpp,
L1Scoring::score, both TemplatedVocabulary::transform overloads, loadFromTextFile and the two KeyFrameDatabase::Detect* functions, cut out of / compiled from the reference at
test time into tmp_path around tests/cpp/ref_bow_standins.cpp (R.build_reference).  No tolerance: words, nodes and FeatureVectors equal entry for entry, BowVector values and
scores equal as 64-bit patterns, candidate lists equal in content and order.  Nothing cut or compiled is written inside the repository."""
import ctypes as C

import numpy as np
import pytest

from tests import bow_patterns as P
from tests import bow_restatement as R

pytestmark = pytest.mark.skipif(not R.reference_available(), reason="needs the reference under /root/reference")
VOCS = sorted(P.vocabularies())


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build_reference(tmp_path_factory.mktemp("ref_bow"))


@pytest.fixture(scope="module")
def loaded(ref, tmp_path_factory):
    """{vocabulary name: the reference's vocabulary loaded from our text, without a final newline}"""
    d = tmp_path_factory.mktemp("ref_bow_voc")
    out = {}
    for name, (v, up) in P.vocabularies().items():
        path = d / (name + ".txt")
        path.write_text(R.to_text(v))
        out[name] = ref.pin_voc_load(str(path).encode())
        assert out[name]
    return out


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _nodes(ref, h):
    k, L, n, nw, sc, we = (C.c_int() for _ in range(6))
    ref.pin_voc_info(C.c_void_p(h), *[C.byref(x) for x in (k, L, n, nw, sc, we)])
    n = n.value
    parent, nch, cols, word = (np.zeros(n, np.int32) for _ in range(4))
    desc, weight = np.zeros((n, 32), np.uint8), np.zeros(n, np.float64)
    ref.pin_voc_nodes(C.c_void_p(h), _p(parent, C.c_int), _p(nch, C.c_int), _p(desc, C.c_uint8), _p(cols, C.c_int), _p(weight, C.c_double), _p(word, C.c_int))
    return (k.value, L.value, n, nw.value, sc.value, we.value), parent, nch, desc, cols, weight, word


def test_cut_takes_the_whole_definition():
    text = "template<class TDescriptor, class F>\nvoid A<TDescriptor,F>::f(int a) const;\ntemplate<class TDescriptor, class F>\nvoid A<TDescriptor,F>::f(int a) const\n{\n  if (a) { g(); }\n}\nint h;"
    assert R._cut_template(text, "::f(int a) const") == "template<class TDescriptor, class F>\nvoid A<TDescriptor,F>::f(int a) const\n{\n  if (a) { g(); }\n}"


def test_distance_and_from_string(ref):
    rng = np.random.default_rng(3)
    for _ in range(200):
        a, b = rng.integers(0, 256, 32).astype(np.uint8), rng.integers(0, 256, 32).astype(np.uint8)
        assert ref.pin_distance(_p(a, C.c_uint8), _p(b, C.c_uint8)) == R.distance(a, b)
        out = np.zeros(32, np.uint8)
        ref.pin_from_string((" ".join(str(int(x)) for x in a) + " ").encode(), _p(out, C.c_uint8))
        assert np.array_equal(out, a)
    z = np.zeros(32, np.uint8)
    assert ref.pin_distance(_p(z, C.c_uint8), _p(~z, C.c_uint8)) == 256


@pytest.mark.parametrize("voc", VOCS)
def test_load_from_text_file(ref, loaded, voc):
    v, up = P.vocabularies()[voc]
    head, parent, nch, desc, cols, weight, word = _nodes(ref, loaded[voc])
    assert head == (v.k, v.L, len(v.parent), v.n_words, 0, 0)
    assert np.array_equal(parent[1:], v.parent[1:]) and np.array_equal(nch, [len(c) for c in v.children]) and np.array_equal(desc[1:], v.desc[1:]) and (cols[1:] == 32).all()
    assert np.array_equal(R.bits(weight[1:]), R.bits(v.weight[1:]))
    leaf = v.is_leaf > 0
    assert np.array_equal(word[leaf], v.word_id[leaf])
    node_of_word = np.zeros(v.n_words, np.int32)
    ref.pin_voc_words(C.c_void_p(loaded[voc]), _p(node_of_word, C.c_int))
    assert np.array_equal(node_of_word, np.flatnonzero(leaf))  # word ids in node-id order


def test_a_final_newline_adds_a_node_under_the_root(ref, tmp_path):
    """What the reference does with a vocabulary file that ends with a newline: its `while(!f.eof())` reads one more, empty, line and appends one more node.  The
    extractions from the empty line fail before they write (the stream is at its end), so `pid` and `nIsLeaf` are read uninitialised: the node hangs under whatever node the
    stack slot names (observed with this build: the parent of the last real line) and is or is not given a word id (observed: it is, the flag of the last real line, a leaf).
    What does not depend on that: one node more, childless, with weight 0 and a 32-byte descriptor no value was written to, so a descent that ends there is stopped.
    Recorded here and in DESIGN 7.12; the restatement and the mirrors ignore a final empty line instead."""
    v, up = P.vocabularies()["k5_L2_root"]
    path = tmp_path / "newline.txt"
    path.write_text(R.to_text(v, trailing_newline=True))
    h = ref.pin_voc_load(str(path).encode())
    head, parent, nch, desc, cols, weight, word = _nodes(ref, h)
    n = len(v.parent)
    print("the extra node: parent %d, word id %d, %d words (%d without it)" % (parent[n], word[n], head[3], v.n_words))
    assert head[:3] == (v.k, v.L, n + 1) and head[3] in (v.n_words, v.n_words + 1)
    assert nch[n] == 0 and weight[n] == 0.0 and cols[n] == 32 and nch.sum() == n
    assert np.array_equal(parent[1:n], v.parent[1:]) and np.array_equal(desc[1:n], v.desc[1:])


def _ref_transform(ref, h, d, up):
    n = len(d)
    d = np.ascontiguousarray(d if n else np.zeros((1, 32), np.uint8))
    bw, bv, fn, ff, nfv = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.float64), np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), C.c_int()
    nb = ref.pin_transform(C.c_void_p(h), n, _p(d, C.c_uint8), up, _p(bw, C.c_int), _p(bv, C.c_double), C.byref(nfv), _p(fn, C.c_int), _p(ff, C.c_int))
    return bw[:nb], bv[:nb], fn[:nfv.value], ff[:nfv.value]


@pytest.mark.parametrize("voc", VOCS)
def test_transform(ref, loaded, voc):
    v, up = P.vocabularies()[voc]
    h = loaded[voc]
    for name, d in P.frames(voc).items():
        bow, fv, word, node = R.transform(v, d, up)
        bw, bv, fn, ff = _ref_transform(ref, h, d, up)
        rw, rx = R.bow_arrays(bow)
        assert np.array_equal(bw, rw) and np.array_equal(R.bits(bv), R.bits(rx)), (voc, name)
        assert [(k, i) for k, idx in fv.items() for i in idx] == list(zip(fn.tolist(), ff.tolist())), (voc, name)
        for i in range(0, len(d), max(1, len(d) // 60)):  # the per-feature overload, stopped features included
            w, wt, nid = C.c_int(), C.c_double(), C.c_int()
            ref.pin_transform_feature(C.c_void_p(h), _p(np.ascontiguousarray(d[i]), C.c_uint8), up, C.byref(w), C.byref(wt), C.byref(nid))
            assert (w.value, wt.value, nid.value) == R.transform_feature(v, d[i], up), (voc, name, i)


def test_score(ref, loaded):
    h = loaded["k5_L2_root"]
    bows = [op[2] for op in P.scenarios()["k65"] if op[0] == "add"][:14] + [{7: 1.0}, {}]
    for a in bows:
        for b in bows:
            (wa, xa), (wb, xb) = R.bow_arrays(a), R.bow_arrays(b)
            wa, xa, wb, xb = (np.concatenate([t, t[:0] if len(t) else np.zeros(1, t.dtype)]) for t in (wa, xa, wb, xb))
            s = ref.pin_score(C.c_void_p(h), len(a), _p(wa, C.c_int), _p(xa, C.c_double), len(b), _p(wb, C.c_int), _p(xb, C.c_double))
            assert np.float64(s).view(np.uint64) == np.float64(R.score(a, b)).view(np.uint64)


class _RefDB:
    """The reference's KeyFrameDatabase behind the interface P.replay drives."""

    def __init__(self, ref, voc):
        self.ref, self.db, self.kfs = ref, C.c_void_p(ref.pin_db_create(C.c_void_p(voc))), {}

    def _kf(self, i, bow=None):
        if i not in self.kfs:
            w, x = R.bow_arrays(bow or {})
            self.kfs[i] = C.c_void_p(self.ref.pin_kf_create(C.c_long(i), len(w), _p(w, C.c_int), _p(x, C.c_double)))
        return self.kfs[i]

    def add(self, i, bow):
        self.ref.pin_db_add(self.db, self._kf(i, bow))

    def erase(self, i):
        self.ref.pin_db_erase(self.db, self._kf(i))

    def clear(self):
        self.ref.pin_db_clear(self.db)

    def _neighbours(self, cov):
        for i, lst in cov.items():
            arr = (C.c_void_p * max(len(lst), 1))(*[self._kf(j).value for j in lst])
            self.ref.pin_kf_set_neighbours(self._kf(i), 0, None, len(lst), arr)

    def DetectLoopCandidates(self, qid, bow, connected, cov, minScore):
        self._neighbours(cov)
        w, x = R.bow_arrays(bow)
        q = C.c_void_p(self.ref.pin_kf_create(C.c_long(qid), len(w), _p(w, C.c_int), _p(x, C.c_double)))  # the query key frame is not in the database
        arr = (C.c_void_p * max(len(connected), 1))(*[self._kf(j).value for j in connected])
        self.ref.pin_kf_set_neighbours(q, len(connected), arr, 0, None)
        out = np.zeros(len(self.kfs) + 1, np.int64)
        n = self.ref.pin_detect_loop(self.db, q, C.c_float(minScore), _p(out, C.c_long))
        return out[:n].tolist()

    def DetectRelocalizationCandidates(self, qid, bow, cov):
        self._neighbours(cov)
        w, x = R.bow_arrays(bow)
        out = np.zeros(len(self.kfs) + 1, np.int64)
        n = self.ref.pin_detect_reloc(self.db, C.c_long(qid), len(w), _p(w, C.c_int), _p(x, C.c_double), _p(out, C.c_long))
        return out[:n].tolist()


@pytest.mark.parametrize("name", sorted(P.scenarios()))
def test_detect_candidates(ref, loaded, name):
    ops = P.scenarios()[name]
    # the inverted file has one list per word of the vocabulary: the scenarios' word ids (< 2000) need a vocabulary that large
    assert max(max(op[2]) for op in ops if op[0] in ("add", "loop", "reloc")) < 2000 <= _big(ref, loaded)[1]
    assert P.replay(ops, _RefDB(ref, _big(ref, loaded)[0])) == P.replay(ops, R.KeyFrameDatabase(), R.KF)


_BIG = {}


def _big(ref, loaded):
    """A vocabulary of the reference with at least 2 000 words (k = 13, L = 3, 2 197 leaves) for the database's inverted file; its tree is not used."""
    if not _BIG:
        import tempfile
        rng = np.random.default_rng(1)
        v = P._tree(rng, 13, 3, lambda depth, r: 13, lambda depth, r: False)
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.write(R.to_text(v))
        _BIG["v"] = (ref.pin_voc_load(f.name.encode()), v.n_words)
        import os
        os.unlink(f.name)
    return _BIG["v"]
