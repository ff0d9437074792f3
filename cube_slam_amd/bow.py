"""Place recognition with the reference's names: ORBVocabulary (DBoW2's TemplatedVocabulary<FORB>: loadFromTextFile, transform, score) and KeyFrameDatabase
(orb_object_slam/src/KeyFrameDatabase.cc).  The vocabulary descent, the BowVector accumulation and every score run on the device (cs_bow_* in include/cubeslam_hip.h,
csrc/bow.hip); what follows the scores in DetectLoopCandidates / DetectRelocalizationCandidates is the reference's host logic, statement by statement in float."""
import collections
import ctypes as C

import numpy as np

from ._lib import Context, CubeSlamError, Handle, check, lib, ptr

F32 = np.float32


class BowVector(dict):
    """DBoW2::BowVector: {word id: value}, iterated in ascending word id."""

    def arrays(self):
        return np.fromiter(self.keys(), np.int32, len(self)), np.fromiter(self.values(), np.float64, len(self))


class FeatureVector(dict):
    """DBoW2::FeatureVector: {node id: [feature index, ...]}, iterated in ascending node id.  `node` is the per-feature array the device searches take (-1: stopped)."""
    node = None


def parse_vocabulary_text(text):
    """The arrays TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1350-1437) leaves in m_nodes, from the reference's text format:
    (k, L, scoring, weighting, parent, is_leaf, desc, weight).  A final empty line is ignored (the reference's eof loop turns it into one more node)."""
    lines = text.split("\n")
    if lines and lines[-1].strip() == "":
        lines.pop()
    head = lines[0].split()
    if len(head) < 4:
        raise CubeSlamError("vocabulary text: the first line is 'k L scoring weighting'")
    k, L, n1, n2 = (int(x) for x in head[:4])
    if k < 0 or k > 20 or L < 1 or L > 10 or n1 < 0 or n1 > 5 or n2 < 0 or n2 > 3:
        raise CubeSlamError("Vocabulary loading failure: This is not a correct text file!")
    n = len(lines)
    rows = np.array([ln.split() for ln in lines[1:]]) if n > 1 else np.zeros((0, 35), "U1")
    if rows.ndim != 2 or rows.shape[1] != 35:
        raise CubeSlamError("vocabulary text: a node line is 'parent is_leaf 32 bytes weight'")
    parent = np.zeros(n, np.int32); is_leaf = np.zeros(n, np.uint8); desc = np.zeros((n, 32), np.uint8); weight = np.zeros(n, np.float64)
    parent[1:] = rows[:, 0].astype(np.int64)
    is_leaf[1:] = rows[:, 1].astype(np.int64) > 0
    desc[1:] = rows[:, 2:34].astype(np.int64).astype(np.uint8)
    weight[1:] = rows[:, 34].astype(np.float64)
    return k, L, n1, n2, parent, is_leaf, desc, weight


class ORBVocabulary(Handle):
    HANDLE, DESTROY = "_v", "cs_bow_vocab_destroy"

    def __init__(self, k=None, L=None, parent=None, is_leaf=None, desc=None, weight=None, levelsup=4, scoring=0, weighting=0, ctx=None):
        self.ctx = ctx
        self._v = C.c_void_p()
        self.levelsup = int(levelsup)
        if k is not None:
            self._create(k, L, parent, is_leaf, desc, weight, scoring, weighting)

    def _create(self, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0):
        self.close()
        parent = np.ascontiguousarray(parent, np.int32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); weight = np.ascontiguousarray(weight, np.float64)
        n = len(parent)
        if not (len(is_leaf) == len(desc) == len(weight) == n):
            raise CubeSlamError("ORBVocabulary: parent, is_leaf, desc and weight are one entry per node")
        if lib().cs_bow_vocab_check(int(k), int(L), n, ptr(parent), ptr(is_leaf), self.levelsup, int(weighting), int(scoring)) != 0:  # needs no device
            raise CubeSlamError("cs_bow_vocab_create refuses this vocabulary: CS_ERR_BAD_ARG (only TF_IDF / L1; k 2..20, L 1..10; parent < node; leaf flag = no children; "
                                "no leaf above level L - levelsup; at most k children)")
        if self.ctx is None:
            self.ctx = Context(0)
        check(self.ctx.ptr, lib().cs_bow_vocab_create(self.ctx.ptr, int(k), int(L), n, ptr(parent), ptr(is_leaf), ptr(desc), ptr(weight),
                                                      self.levelsup, int(weighting), int(scoring), C.byref(self._v)), "cs_bow_vocab_create")
        self.k, self.L, self.n_nodes = int(k), int(L), n
        nw = C.c_int()
        lib().cs_bow_vocab_info(self._v, None, None, None, C.byref(nw), None)
        self.n_words = nw.value

    def loadFromTextFile(self, filename):
        with open(filename) as f:
            k, L, n1, n2, parent, is_leaf, desc, weight = parse_vocabulary_text(f.read())
        self._create(k, L, parent, is_leaf, desc, weight, scoring=n1, weighting=n2)
        return True

    def size(self):
        return self.n_words

    def transform_raw(self, descriptors_per_frame):
        """cs_bow_transform on a list of (n_i, 32) uint8 arrays -> offsets, word, node, bow_count, bow_word, bow_value."""
        frames = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descriptors_per_frame]
        off = np.zeros(len(frames) + 1, np.int32)
        off[1:] = np.cumsum([len(d) for d in frames])
        n = int(off[-1])
        desc = np.concatenate(frames) if n else np.zeros((1, 32), np.uint8)
        word = np.zeros(max(n, 1), np.int32); node = np.zeros(max(n, 1), np.int32); cnt = np.zeros(max(len(frames), 1), np.int32)
        bw = np.zeros(max(n, 1), np.int32); bv = np.zeros(max(n, 1), np.float64)
        check(self.ctx.ptr, lib().cs_bow_transform(self.ctx.ptr, self._v, len(frames), ptr(off), ptr(desc), ptr(word), ptr(node), ptr(cnt),
                                                   ptr(bw), ptr(bv)), "cs_bow_transform")
        return off, word[:n], node[:n], cnt[:len(frames)], bw[:n], bv[:n]

    def transform_batch(self, descriptors_per_frame):
        """[(BowVector, FeatureVector)] of TemplatedVocabulary::transform(features, v, fv, levelsup) for every frame, in one device pass."""
        off, _, node, cnt, bw, bv = self.transform_raw(descriptors_per_frame)
        out = []
        for f in range(len(cnt)):
            o = int(off[f])
            bow = BowVector(zip(bw[o:o + cnt[f]].tolist(), bv[o:o + cnt[f]].tolist()))
            nf = node[o:off[f + 1]]
            fv = FeatureVector()
            kept = np.flatnonzero(nf >= 0)
            order = kept[np.argsort(nf[kept], kind="stable")]
            for i in order.tolist():
                fv.setdefault(int(nf[i]), []).append(i)
            fv.node = nf.copy()
            out.append((bow, fv))
        return out

    def transform(self, descriptors, levelsup=4):
        if int(levelsup) != self.levelsup:
            raise CubeSlamError("ORBVocabulary.transform: the vocabulary was created for levelsup = %d" % self.levelsup)
        return self.transform_batch([descriptors])[0]

    def score_pairs(self, vectors, pairs):
        """L1Scoring::score(vectors[a], vectors[b]) for every (a, b) of `pairs`, as float64."""
        arrs = [BowVector(v).arrays() for v in vectors]
        off = np.zeros(len(arrs) + 1, np.int32)
        off[1:] = np.cumsum([len(a[0]) for a in arrs])
        w = np.concatenate([a[0] for a in arrs] + [np.zeros(1, np.int32)]); x = np.concatenate([a[1] for a in arrs] + [np.zeros(1, np.float64)])
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        pa = np.ascontiguousarray(pairs[:, 0]); pb = np.ascontiguousarray(pairs[:, 1])
        out = np.zeros(max(len(pairs), 1), np.float64)
        check(self.ctx.ptr, lib().cs_bow_score(self.ctx.ptr, len(arrs), ptr(off), ptr(w), ptr(x), len(pairs), ptr(pa), ptr(pb), ptr(out)), "cs_bow_score")
        return out[:len(pairs)]

    def score(self, v1, v2):
        return float(self.score_pairs([v1, v2], [(0, 1)])[0])


class _KFState:
    """The per-key-frame fields the reference keeps across queries.  KeyFrame's constructor (KeyFrame.cc:48) never initialises mRelocScore; it starts at 0 here."""
    __slots__ = ("mnLoopQuery", "mnLoopWords", "mLoopScore", "mnRelocQuery", "mnRelocWords", "mRelocScore")

    def __init__(self):
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = 0, 0, F32(0)
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, F32(0)


def candidates_loop(state, shared, query_id, connected_ids, best_covisibles, minScore):
    """KeyFrameDatabase::DetectLoopCandidates (KeyFrameDatabase.cc:74-194) behind the scores.  shared = [(kf id, common words, smallest common word, add order, score f64)]
    for the key frames that share a word with the query; state = {kf id: _KFState}.  The reference meets the key frames word by word through the inverted file: that is
    the order of (smallest common word, add order)."""
    minScore = F32(minScore)
    connected = set(connected_ids)
    sharing = []
    for kf, common, _, _, sc in sorted(shared, key=lambda r: (r[2], r[3])):
        s = state[kf]
        if s.mnLoopQuery != query_id:
            if kf in connected:
                s.mnLoopWords = 1  # reset at every word it is met through (:93), then counted
                continue
            s.mnLoopWords = 0
            s.mnLoopQuery = query_id
            sharing.append((kf, sc))
        s.mnLoopWords += common
    if not sharing:
        return []
    maxCommonWords = max(0, max(state[kf].mnLoopWords for kf, _ in sharing))
    minCommonWords = int(F32(maxCommonWords) * F32(0.8))
    scored = []
    for kf, sc in sharing:
        s = state[kf]
        if s.mnLoopWords > minCommonWords:
            si = F32(sc)
            s.mLoopScore = si
            if si >= minScore:
                scored.append((si, kf))
    if not scored:
        return []
    acc, bestAcc = [], minScore
    for si, kf in scored:
        bestScore, accScore, best = si, si, kf
        for kf2 in best_covisibles.get(kf, []):
            s2 = state[kf2]
            if s2.mnLoopQuery == query_id and s2.mnLoopWords > minCommonWords:
                accScore = F32(accScore + s2.mLoopScore)
                if s2.mLoopScore > bestScore:
                    best, bestScore = kf2, s2.mLoopScore
        acc.append((accScore, best))
        if accScore > bestAcc:
            bestAcc = accScore
    return _retain(acc, bestAcc)


def candidates_reloc(state, shared, query_id, best_covisibles):
    """KeyFrameDatabase::DetectRelocalizationCandidates (:196-305) behind the scores; arguments as candidates_loop."""
    sharing = []
    for kf, common, _, _, sc in sorted(shared, key=lambda r: (r[2], r[3])):
        s = state[kf]
        if s.mnRelocQuery != query_id:
            s.mnRelocWords = 0
            s.mnRelocQuery = query_id
            sharing.append((kf, sc))
        s.mnRelocWords += common
    if not sharing:
        return []
    maxCommonWords = max(0, max(state[kf].mnRelocWords for kf, _ in sharing))
    minCommonWords = int(F32(maxCommonWords) * F32(0.8))
    scored = []
    for kf, sc in sharing:
        s = state[kf]
        if s.mnRelocWords > minCommonWords:
            s.mRelocScore = F32(sc)
            scored.append((s.mRelocScore, kf))
    if not scored:
        return []
    acc, bestAcc = [], F32(0)
    for si, kf in scored:
        bestScore, accScore, best = si, si, kf
        for kf2 in best_covisibles.get(kf, []):
            s2 = state[kf2]
            if s2.mnRelocQuery != query_id:
                continue
            accScore = F32(accScore + s2.mRelocScore)  # of a neighbour not scored in this query: what an earlier query left (:270-273)
            if s2.mRelocScore > bestScore:
                best, bestScore = kf2, s2.mRelocScore
        acc.append((accScore, best))
        if accScore > bestAcc:
            bestAcc = accScore
    return _retain(acc, bestAcc)


def _retain(acc, bestAcc):
    minScoreToRetain = F32(F32(0.75) * bestAcc)
    out = []
    for a, kf in acc:
        if a > minScoreToRetain and kf not in out:
            out.append(kf)
    return out


class KeyFrameDatabase(Handle):
    """The key frames' BowVectors resident on the device (cs_bow_db_*), with the reference's per-key-frame query fields on the host."""
    HANDLE, DESTROY = "_db", "cs_bow_db_destroy"

    def __init__(self, ctx=None):
        self.ctx = ctx if ctx is not None else Context(0)
        self._db = C.c_void_p()
        check(self.ctx.ptr, lib().cs_bow_db_create(self.ctx.ptr, C.byref(self._db)), "cs_bow_db_create")
        self.state = collections.defaultdict(_KFState)  # a key frame keeps its fields when it is erased, as the KeyFrame object does

    def add(self, kf_id, bow):
        w, x = BowVector(bow).arrays()
        check(self.ctx.ptr, lib().cs_bow_db_add(self.ctx.ptr, self._db, int(kf_id), len(w), ptr(w), ptr(x)), "cs_bow_db_add")
        self.state[int(kf_id)]

    def erase(self, kf_id):
        check(self.ctx.ptr, lib().cs_bow_db_erase(self._db, int(kf_id)), "cs_bow_db_erase")

    def clear(self):
        check(self.ctx.ptr, lib().cs_bow_db_clear(self._db), "cs_bow_db_clear")

    def size(self):
        n = C.c_int()
        check(self.ctx.ptr, lib().cs_bow_db_size(self._db, C.byref(n)), "cs_bow_db_size")
        return n.value

    def query_raw(self, bows):
        """cs_bow_db_query for a batch of BowVectors -> arrays (query, kf id, add order, common words, smallest common word, score f64), one entry per (query, key frame)
        that share a word, queries ascending and key frames in add order."""
        arrs = [BowVector(b).arrays() for b in bows]
        off = np.zeros(len(arrs) + 1, np.int32)
        off[1:] = np.cumsum([len(a[0]) for a in arrs])
        w = np.concatenate([a[0] for a in arrs] + [np.zeros(1, np.int32)]); x = np.concatenate([a[1] for a in arrs] + [np.zeros(1, np.float64)])
        cap = max(len(arrs) * self.size(), 1)
        oq = np.zeros(cap, np.int32); oid = np.zeros(cap, np.int64); oord = np.zeros(cap, np.int64); oc = np.zeros(cap, np.int32); om = np.zeros(cap, np.int32)
        osc = np.zeros(cap, np.float64)
        n = C.c_long()
        check(self.ctx.ptr, lib().cs_bow_db_query(self.ctx.ptr, self._db, len(arrs), ptr(off), ptr(w), ptr(x), cap, C.byref(n), ptr(oq),
                                                  ptr(oid), ptr(oord), ptr(oc), ptr(om), ptr(osc)), "cs_bow_db_query")
        n = n.value
        return oq[:n], oid[:n], oord[:n], oc[:n], om[:n], osc[:n]

    def query(self, bows):
        """Per query [(kf id, common words, smallest common word, add order, score f64)] for the key frames that share a word with it, in add order."""
        oq, oid, oord, oc, om, osc = self.query_raw(bows)
        out = [[] for _ in bows]
        for q, i, c, m, o, s in zip(oq.tolist(), oid.tolist(), oc.tolist(), om.tolist(), oord.tolist(), osc.tolist()):
            out[q].append((i, c, m, o, s))
        return out

    def DetectLoopCandidates(self, query_id, bow, connected_ids, best_covisibles, minScore):
        return candidates_loop(self.state, self.query([bow])[0], int(query_id), connected_ids, best_covisibles, minScore)

    def DetectRelocalizationCandidates(self, query_id, bow, best_covisibles):
        return candidates_reloc(self.state, self.query([bow])[0], int(query_id), best_covisibles)
