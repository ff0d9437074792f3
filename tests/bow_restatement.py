"""The judge of the place-recognition tests: a plain Python / numpy float64 restatement of the reference's DBoW2 transform and key-frame database
(orb_object_slam/Thirdparty/DBoW2/DBoW2: FORB::distance and fromString FORB.cpp:81-135, BowVector.cpp:34-84, FeatureVector.cpp, L1Scoring::score ScoringObject.cpp:23-68,
TemplatedVocabulary::transform TemplatedVocabulary.h:1139-1271 and loadFromTextFile :1350-1437; orb_object_slam/src/KeyFrameDatabase.cc:38-305).  Python floats are IEEE
doubles and every sum below is written in the reference's order, so doubles compare as 64-bit patterns; the float steps of the Detect* functions go through np.float32.
tests/test_bow_restatement_pins.py pins it to the reference's own text compiled at test time (build_reference below); nothing cut or compiled is written into the repository."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
DBOW = os.path.join(REF, "orb_object_slam", "Thirdparty", "DBoW2", "DBoW2")
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
F32 = np.float32


class Vocabulary:
    """m_nodes as loadFromTextFile leaves it: children in file order, word ids to the flagged leaves in node-id order."""

    def __init__(self, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0):
        self.k, self.L, self.scoring, self.weighting = int(k), int(L), int(scoring), int(weighting)
        self.parent = np.asarray(parent, np.int32)
        self.is_leaf = np.asarray(is_leaf, np.uint8)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.weight = np.asarray(weight, np.float64)
        n = len(self.parent)
        self.children = [[] for _ in range(n)]
        for i in range(1, n):
            self.children[int(self.parent[i])].append(i)
        self.word_id = np.full(n, -1, np.int32)
        self.word_id[self.is_leaf > 0] = np.arange(int((self.is_leaf > 0).sum()))
        self.n_words = int((self.is_leaf > 0).sum())
        self.depth = np.zeros(n, np.int32)
        for i in range(1, n):
            self.depth[i] = self.depth[self.parent[i]] + 1

    def arrays(self):
        return self.k, self.L, self.parent, self.is_leaf, self.desc, self.weight


def refusal(k, L, parent, is_leaf, levelsup, scoring=0, weighting=0):
    """Why cs_bow_vocab_create must refuse these arrays (None: it must not): what leaves the reference undefined, and what only other vocabularies than ORBvoc use."""
    if scoring != 0 or weighting != 0:
        return "weighting"
    if k < 2 or k > 20 or L < 1 or L > 10:
        return "bounds"
    n = len(parent)
    nchild, depth = [0] * n, [0] * n
    for i in range(1, n):
        if not 0 <= parent[i] < i:
            return "parent"
        nchild[parent[i]] += 1
        depth[i] = depth[parent[i]] + 1
    for i in range(n):
        if bool(is_leaf[i]) != (nchild[i] == 0):
            return "leaf flag"
        if nchild[i] == 0 and L - levelsup > 0 and depth[i] < L - levelsup:
            return "shallow leaf"
        if nchild[i] > k:
            return "children"
    return None


def distance(a, b):
    """FORB::distance: the population count of the xor (the bit trick of :92-98 is one)."""
    return int(POP[np.bitwise_xor(a, b)].sum())


def transform_feature(v, d, levelsup):
    """transform(feature, word_id, weight, nid, levelsup) (:1230-1271) -> (word, weight, nid)."""
    nid_level = v.L - levelsup
    nid = 0 if nid_level <= 0 else None
    final, level = 0, 0
    while True:
        level += 1
        nodes = v.children[final]
        dist = POP[np.bitwise_xor(v.desc[nodes], d[None, :])].sum(axis=1)
        final = nodes[int(np.argmin(dist))]  # the first minimum: `d < best_d` is strict
        if level == nid_level:
            nid = final
        if not v.children[final]:
            break
    return int(v.word_id[final]), float(v.weight[final]), nid


def transform(v, descs, levelsup=4):
    """transform(features, v, fv, levelsup) (:1139-1206) for TF_IDF / L1 -> (bow {word: value} in ascending word order, fv {node: [feature, ...]} in ascending node
    order, word[n], node[n] with -1 where stopped)."""
    descs = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
    bow, fv = {}, {}
    word, node = np.full(len(descs), -1, np.int32), np.full(len(descs), -1, np.int32)
    if len(v.parent) > 1:
        for i, d in enumerate(descs):
            w_id, w, nid = transform_feature(v, d, levelsup)
            if w > 0:
                bow[w_id] = bow[w_id] + w if w_id in bow else w  # BowVector::addWeight
                fv.setdefault(nid, []).append(i)                # FeatureVector::addFeature
                word[i], node[i] = w_id, nid
    bow = dict(sorted(bow.items()))
    norm = 0.0
    for x in bow.values():  # BowVector::normalize(L1)
        norm += abs(x)
    if norm > 0.0:
        bow = {k: x / norm for k, x in bow.items()}
    return bow, dict(sorted(fv.items())), word, node


def score(v1, v2):
    """L1Scoring::score: the common words in ascending id (the lower_bound jumps of :47-58 visit exactly them)."""
    s = 0.0
    for w in sorted(set(v1) & set(v2)):
        vi, wi = v1[w], v2[w]
        s += abs(vi - wi) - abs(vi) - abs(wi)
    return -s / 2.0


def bow_arrays(bow):
    return np.fromiter(bow.keys(), np.int32, len(bow)), np.fromiter(bow.values(), np.float64, len(bow))


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the text format
def arrays_to_text(k, L, scoring, weighting, parent, is_leaf, desc, weight, trailing_newline=False):
    """What TemplatedVocabulary::saveToTextFile writes: 'k L scoring weighting', then per node 'parent is_leaf 32 bytes weight'."""
    lines = ["%d %d %d %d" % (k, L, scoring, weighting)]
    for i in range(1, len(parent)):
        lines.append("%d %d %s %s" % (parent[i], 1 if is_leaf[i] else 0, " ".join(str(int(b)) for b in desc[i]), repr(float(weight[i]))))
    return "\n".join(lines) + ("\n" if trailing_newline else "")


def to_text(v, trailing_newline=False):
    return arrays_to_text(v.k, v.L, v.scoring, v.weighting, v.parent, v.is_leaf, v.desc, v.weight, trailing_newline)


def load_text(text):
    """loadFromTextFile for a file that ends without a newline -> Vocabulary.  (With a final newline the reference's `while(!f.eof())` reads one more, empty, line and appends
    a node under whatever `pid` then holds; the pin test records that, and neither this restatement nor the mirrors copy it: a final empty line is ignored.)"""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    k, L, n1, n2 = (int(x) for x in lines[0].split()[:4])
    parent, leaf, desc, weight = [0], [0], [np.zeros(32, np.uint8)], [0.0]
    for ln in lines[1:]:
        t = ln.split()
        parent.append(int(t[0]))
        leaf.append(1 if int(t[1]) > 0 else 0)
        desc.append(np.array([int(x) & 255 for x in t[2:34]], np.uint8))
        weight.append(float(t[34]))
    return Vocabulary(k, L, parent, leaf, np.stack(desc), weight, scoring=n1, weighting=n2)


# ---------------------------------------------------------------------------------------------------------------- KeyFrameDatabase
class KF:
    """The fields of KeyFrame the database touches.  mRelocScore is not initialised by the reference's constructor (KeyFrame.cc:48); it starts at 0 here."""

    def __init__(self, mnId, bow):
        self.mnId, self.mBowVec = mnId, bow
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = 0, 0, F32(0)
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, F32(0)


class KeyFrameDatabase:
    """KeyFrameDatabase.cc line by line over an inverted file of Python lists.  best_covisibles: {kf id: [kf id, ...]} = GetBestCovisibilityKeyFrames(10)."""

    def __init__(self):
        self.inv = {}
        self.kfs = {}
        self.trace = {}  # of the last query, for the precondition checks of tests/test_bow_patterns.py: nothing below reads it

    def add(self, kf):
        self.kfs[kf.mnId] = kf
        for w in kf.mBowVec:
            self.inv.setdefault(w, []).append(kf)

    def erase(self, kf):
        for w in kf.mBowVec:
            lst = self.inv.get(w, [])
            for i, x in enumerate(lst):
                if x is kf:
                    del lst[i]
                    break

    def clear(self):
        self.inv = {}

    def DetectLoopCandidates(self, mnId, bow, connected, best_covisibles, minScore):
        minScore = F32(minScore)
        connected = set(connected)
        sharing = []
        for w in bow:
            for kf in self.inv.get(w, []):
                if kf.mnLoopQuery != mnId:
                    kf.mnLoopWords = 0
                    if kf.mnId not in connected:
                        kf.mnLoopQuery = mnId
                        sharing.append(kf)
                kf.mnLoopWords += 1
        self.trace = {"sharing": [kf.mnId for kf in sharing]}
        if not sharing:
            return []
        maxCommonWords = max(0, max(kf.mnLoopWords for kf in sharing))
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        self.trace.update(max=maxCommonWords, min=minCommonWords, words={kf.mnId: kf.mnLoopWords for kf in sharing})
        scored = []
        for kf in sharing:
            if kf.mnLoopWords > minCommonWords:
                si = F32(score(bow, kf.mBowVec))
                kf.mLoopScore = si
                if si >= minScore:
                    scored.append((si, kf))
        self.trace["scored"] = [(float(si), kf.mnId) for si, kf in scored]
        if not scored:
            return []
        acc, bestAcc = [], minScore
        for si, kf in scored:
            bestScore, accScore, best = si, si, kf
            for i2 in best_covisibles.get(kf.mnId, []):
                kf2 = self.kfs[i2]
                if kf2.mnLoopQuery == mnId and kf2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + kf2.mLoopScore)
                    if kf2.mLoopScore > bestScore:
                        best, bestScore = kf2, kf2.mLoopScore
            acc.append((accScore, best))
            if accScore > bestAcc:
                bestAcc = accScore
        return self._retain(acc, bestAcc)

    def DetectRelocalizationCandidates(self, mnId, bow, best_covisibles):
        sharing = []
        for w in bow:
            for kf in self.inv.get(w, []):
                if kf.mnRelocQuery != mnId:
                    kf.mnRelocWords = 0
                    kf.mnRelocQuery = mnId
                    sharing.append(kf)
                kf.mnRelocWords += 1
        self.trace = {"sharing": [kf.mnId for kf in sharing]}
        if not sharing:
            return []
        maxCommonWords = max(0, max(kf.mnRelocWords for kf in sharing))
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        self.trace.update(max=maxCommonWords, min=minCommonWords, words={kf.mnId: kf.mnRelocWords for kf in sharing})
        scored = []
        for kf in sharing:
            if kf.mnRelocWords > minCommonWords:
                si = F32(score(bow, kf.mBowVec))
                kf.mRelocScore = si
                scored.append((si, kf))
        self.trace["scored"] = [(float(si), kf.mnId) for si, kf in scored]
        self.trace["left_by_earlier_query"] = []
        if not scored:
            return []
        acc, bestAcc = [], F32(0)
        for si, kf in scored:
            bestScore, accScore, best = si, si, kf
            for i2 in best_covisibles.get(kf.mnId, []):
                kf2 = self.kfs[i2]
                if kf2.mnRelocQuery != mnId:
                    continue
                if kf2.mnId not in [i for _, i in self.trace["scored"]]:
                    self.trace["left_by_earlier_query"].append((kf2.mnId, float(kf2.mRelocScore)))
                accScore = F32(accScore + kf2.mRelocScore)
                if kf2.mRelocScore > bestScore:
                    best, bestScore = kf2, kf2.mRelocScore
            acc.append((accScore, best))
            if accScore > bestAcc:
                bestAcc = accScore
        return self._retain(acc, bestAcc)

    def _retain(self, acc, bestAcc):
        self.trace["acc"] = [(float(a), kf.mnId) for a, kf in acc]
        minScoreToRetain = F32(F32(0.75) * bestAcc)
        out = []
        for a, kf in acc:
            if a > minScoreToRetain and kf.mnId not in out:
                out.append(kf.mnId)
        return out


# ---------------------------------------------------------------------------------------------------------------- the pin: the reference's own text
def reference_available():
    return os.path.isdir(DBOW) and os.path.isfile(os.path.join(REF, "orb_object_slam", "src", "KeyFrameDatabase.cc"))


def _cut(text, sig):
    """The function definition that starts with `sig`, up to the brace that closes its body."""
    a = text.index(sig)
    i = text.index("{", a)
    depth = 0
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
        if depth == 0:
            return text[a:i]


def _cut_template(text, marker):
    """The member-function template definition whose signature contains `marker`, from its `template<...>` line to the brace that closes its body."""
    m = text.rindex(marker)  # the definition follows the declaration
    a = text.rindex("template<class TDescriptor, class F>", 0, m)
    return _cut(text[a:], "template<class TDescriptor, class F>")


def build_reference(directory):
    """The reference's own text compiled into `directory` (outside the repository) around tests/cpp/ref_bow_standins.cpp: both transform overloads and
    loadFromTextFile cut out of TemplatedVocabulary.h, L1Scoring::score out of ScoringObject.cpp, the database's functions out of KeyFrameDatabase.cc; FORB.cpp, BowVector.cpp
    and FeatureVector.cpp where they lie; oracle/ref_shim/cvshim.hpp for cv::Mat."""
    d = str(directory)
    assert not os.path.abspath(d).startswith(ROOT + os.sep)
    text = open(os.path.join(DBOW, "TemplatedVocabulary.h")).read()
    with open(os.path.join(d, "ref_bow_voc_extracted.inc"), "w") as f:
        for marker in ("BowVector &v, FeatureVector &fv, int levelsup) const", "WordId &word_id, WordValue &weight, NodeId *nid, int levelsup) const",
                       "::loadFromTextFile(const std::string &filename)"):
            f.write(_cut_template(text, marker) + "\n")
    with open(os.path.join(d, "ref_bow_score_extracted.inc"), "w") as f:
        f.write(_cut(open(os.path.join(DBOW, "ScoringObject.cpp")).read(), "double L1Scoring::score(const BowVector &v1, const BowVector &v2) const") + "\n")
    text = open(os.path.join(REF, "orb_object_slam", "src", "KeyFrameDatabase.cc")).read()
    with open(os.path.join(d, "ref_bow_db_extracted.inc"), "w") as f:
        for sig in ("KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary &voc)", "void KeyFrameDatabase::add(KeyFrame *pKF)", "void KeyFrameDatabase::erase(KeyFrame *pKF)",
                    "void KeyFrameDatabase::clear()", "vector<KeyFrame *> KeyFrameDatabase::DetectLoopCandidates(KeyFrame *pKF, float minScore)",
                    "vector<KeyFrame *> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F)"):
            f.write(_cut(text, sig) + "\n")
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++14", "-fPIC", "-w", "-fvisibility=hidden", "-I" + shim, "-I" + d, "-I" + DBOW]
    objs = []
    for src in [os.path.join(ROOT, "tests", "cpp", "ref_bow_standins.cpp")] + [os.path.join(DBOW, n) for n in ("FORB.cpp", "BowVector.cpp", "FeatureVector.cpp")]:
        objs.append(os.path.join(d, os.path.basename(src)[:-4] + ".o"))
        subprocess.check_call(["g++"] + flags + ["-c", src, "-o", objs[-1]])
    so = os.path.join(d, "libref_bow.so")
    subprocess.check_call(["g++", "-shared", "-o", so] + objs + ["-Wl,--no-undefined", "-lpthread"])
    lib = C.CDLL(so)
    for name in ("pin_voc_load", "pin_db_create", "pin_kf_create"):
        getattr(lib, name).restype = C.c_void_p
    lib.pin_score.restype = C.c_double
    return lib
