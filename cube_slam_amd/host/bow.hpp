// bow.hpp -- place recognition with the reference's names, over the C-ABI (cs_bow_* in include/cubeslam_hip.h):
//   cubeslam::ORBVocabulary     DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h): loadFromTextFile, transform, score
//   cubeslam::KeyFrameDatabase  ORB_SLAM2::KeyFrameDatabase (orb_object_slam/src/KeyFrameDatabase.cc): add, erase, clear, DetectLoopCandidates, DetectRelocalizationCandidates
// The descent, the BowVector accumulation and every score run on the device; what follows the scores in the two Detect* functions is the reference's host logic in float.
// Key frames are ids: best_covisibles[kf] is what pKF->GetBestCovisibilityKeyFrames(10) returns and is the caller's input.
#pragma once
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context

namespace cubeslam {

typedef std::map<int, double> BowVector;                     // DBoW2::BowVector: word id -> value
typedef std::map<int, std::vector<unsigned int>> FeatureVector; // DBoW2::FeatureVector: node id -> feature indices

// m_nodes as TemplatedVocabulary::loadFromTextFile (:1350-1437) leaves it: node 0 is the root, children keep file order
struct VocabularyArrays {
    int k = 0, L = 0, scoring = 0, weighting = 0;
    std::vector<int> parent;
    std::vector<uint8_t> is_leaf, desc; // desc: 32 bytes per node
    std::vector<double> weight;
    int n_nodes() const { return (int)parent.size(); }
    // what cs_bow_vocab_create refuses (host code, needs no device)
    bool refused(int levelsup = 4) const { return cs_bow_vocab_check(k, L, n_nodes(), parent.data(), is_leaf.data(), levelsup, weighting, scoring) != CS_OK; }
};

// The reference's text format: "k L scoring weighting", then one line per node "parent is_leaf b0 .. b31 weight".  A final empty line is ignored (the reference's
// `while(!f.eof())` turns it into one more node with an empty descriptor).  false: not a vocabulary text (the loader's own bounds, :1371).
inline bool parseVocabularyText(std::istream &f, VocabularyArrays &v) {
    std::string s;
    if (!std::getline(f, s)) return false;
    std::stringstream ss(s);
    int n1 = -1, n2 = -1;
    v = VocabularyArrays();
    if (!(ss >> v.k >> v.L >> n1 >> n2)) return false;
    if (v.k < 0 || v.k > 20 || v.L < 1 || v.L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3) return false;
    v.scoring = n1; v.weighting = n2;
    v.parent.push_back(0); v.is_leaf.push_back(0); v.desc.assign(32, 0); v.weight.push_back(0.0);
    while (std::getline(f, s)) {
        if (s.find_first_not_of(" \t\r") == std::string::npos) {
            if (f.peek() == EOF) break; // the final empty line
            return false;
        }
        std::stringstream sn(s);
        int pid = 0, leaf = 0;
        double w = 0;
        if (!(sn >> pid >> leaf)) return false;
        v.parent.push_back(pid); v.is_leaf.push_back(leaf > 0 ? 1 : 0);
        for (int i = 0; i < 32; ++i) {
            int b = 0;
            if (!(sn >> b)) return false;
            v.desc.push_back((uint8_t)b);
        }
        if (!(sn >> w)) return false;
        v.weight.push_back(w);
    }
    return true;
}

class ORBVocabulary {
  public:
    explicit ORBVocabulary(Context &c, int levelsup = 4) : ctx_(c), levelsup_(levelsup) {}
    ~ORBVocabulary() { cs_bow_vocab_destroy(v_); }
    ORBVocabulary(const ORBVocabulary &) = delete;
    ORBVocabulary &operator=(const ORBVocabulary &) = delete;
    void create(const VocabularyArrays &a) {
        cs_bow_vocab_destroy(v_); v_ = nullptr;
        const int r = cs_bow_vocab_create(ctx_.ctx, a.k, a.L, a.n_nodes(), a.parent.data(), a.is_leaf.data(), a.desc.data(), a.weight.data(), levelsup_, a.weighting, a.scoring, &v_);
        if (r != CS_OK) throw std::runtime_error("cs_bow_vocab_create failed (" + std::to_string(r) + "): " + cs_last_error(ctx_.ctx));
    }
    bool loadFromTextFile(const std::string &filename) {
        std::ifstream f(filename.c_str());
        VocabularyArrays a;
        if (!f || !parseVocabularyText(f, a)) return false;
        create(a);
        return true;
    }
    unsigned int size() const { int n = 0; cs_bow_vocab_info(v_, nullptr, nullptr, nullptr, &n, nullptr); return (unsigned int)n; }
    // transform(features, v, fv, levelsup) for a batch of frames: frame f has the descriptors desc[32 * offsets[f]] .. desc[32 * offsets[f + 1]); node (optional) receives the
    // per-feature array cs_match_by_bow / cs_match_by_bow_kf / cs_match_for_triangulation take
    void transform_batch(const std::vector<int> &offsets, const uint8_t *desc, std::vector<BowVector> &v, std::vector<FeatureVector> &fv, std::vector<int> *node = nullptr) {
        const int nf = (int)offsets.size() - 1;
        const size_t n = nf > 0 ? (size_t)offsets[nf] : 0;
        std::vector<int> word(n + 1), nd(n + 1), cnt((size_t)std::max(nf, 0) + 1), bw(n + 1);
        std::vector<double> bv(n + 1);
        v.assign((size_t)std::max(nf, 0), BowVector()); fv.assign((size_t)std::max(nf, 0), FeatureVector());
        if (nf <= 0) return;
        const int r = cs_bow_transform(ctx_.ctx, v_, nf, offsets.data(), desc, word.data(), nd.data(), cnt.data(), bw.data(), bv.data());
        if (r != CS_OK) throw std::runtime_error("cs_bow_transform failed (" + std::to_string(r) + "): " + cs_last_error(ctx_.ctx));
        for (int f = 0; f < nf; ++f) {
            for (int j = 0; j < cnt[f]; ++j) v[f].insert(v[f].end(), BowVector::value_type(bw[offsets[f] + j], bv[offsets[f] + j]));
            for (int i = offsets[f]; i < offsets[f + 1]; ++i)
                if (nd[i] >= 0) fv[f][nd[i]].push_back((unsigned int)(i - offsets[f]));
        }
        if (node) node->assign(nd.begin(), nd.begin() + (long)n);
    }
    void transform(const std::vector<uint8_t> &descriptors, BowVector &v, FeatureVector &fv, int levelsup = 4, std::vector<int> *node = nullptr) {
        if (levelsup != levelsup_) throw std::runtime_error("ORBVocabulary::transform: the vocabulary was created for another levelsup");
        std::vector<BowVector> vs;
        std::vector<FeatureVector> fvs;
        transform_batch({0, (int)(descriptors.size() / 32)}, descriptors.data(), vs, fvs, node);
        v.swap(vs[0]); fv.swap(fvs[0]);
    }
    double score(const BowVector &v1, const BowVector &v2) {
        std::vector<int> off{0, (int)v1.size(), (int)(v1.size() + v2.size())}, w;
        std::vector<double> x;
        for (const BowVector *b : {&v1, &v2})
            for (const auto &e : *b) { w.push_back(e.first); x.push_back(e.second); }
        w.push_back(0); x.push_back(0);
        const int pa = 0, pb = 1;
        double s = 0;
        const int r = cs_bow_score(ctx_.ctx, 2, off.data(), w.data(), x.data(), 1, &pa, &pb, &s);
        if (r != CS_OK) throw std::runtime_error("cs_bow_score failed (" + std::to_string(r) + "): " + cs_last_error(ctx_.ctx));
        return s;
    }

  private:
    Context &ctx_;
    int levelsup_;
    cs_bow_vocab *v_ = nullptr;
};

// The fields of KeyFrame the database keeps across queries.  The reference's constructor (KeyFrame.cc:48) never initialises mRelocScore; it starts at 0 here.
struct KeyFrameFields {
    long mnLoopQuery = 0; int mnLoopWords = 0; float mLoopScore = 0;
    long mnRelocQuery = 0; int mnRelocWords = 0; float mRelocScore = 0;
};
// one key frame that shares a word with the query: what cs_bow_db_query returns
struct SharedWords { long id; int common, minword; long order; double score; };
typedef std::map<long, KeyFrameFields> KeyFrameState;
typedef std::map<long, std::vector<long>> Covisibles;

namespace bow_detail {
inline void first_encounter_order(std::vector<SharedWords> &s) { // the reference meets the key frames word by word through the inverted file
    std::stable_sort(s.begin(), s.end(), [](const SharedWords &a, const SharedWords &b) { return a.minword != b.minword ? a.minword < b.minword : a.order < b.order; });
}
inline std::vector<long> retain(const std::vector<std::pair<float, long>> &acc, float bestAccScore) {
    const float minScoreToRetain = 0.75f * bestAccScore;
    std::vector<long> out;
    for (const auto &a : acc)
        if (a.first > minScoreToRetain && std::find(out.begin(), out.end(), a.second) == out.end()) out.push_back(a.second);
    return out;
}
} // namespace bow_detail

// KeyFrameDatabase::DetectLoopCandidates (KeyFrameDatabase.cc:74-194) behind the scores
inline std::vector<long> DetectLoopCandidatesFromShared(KeyFrameState &state, std::vector<SharedWords> shared, long query_id, const std::set<long> &connected,
                                                        const Covisibles &best_covisibles, float minScore) {
    bow_detail::first_encounter_order(shared);
    std::vector<std::pair<long, double>> sharing;
    for (const SharedWords &e : shared) {
        KeyFrameFields &s = state[e.id];
        if (s.mnLoopQuery != query_id) {
            if (connected.count(e.id)) { s.mnLoopWords = 1; continue; } // reset at every word it is met through (:93), then counted
            s.mnLoopWords = 0;
            s.mnLoopQuery = query_id;
            sharing.push_back({e.id, e.score});
        }
        s.mnLoopWords += e.common;
    }
    if (sharing.empty()) return {};
    int maxCommonWords = 0;
    for (const auto &p : sharing) maxCommonWords = std::max(maxCommonWords, state[p.first].mnLoopWords);
    const int minCommonWords = maxCommonWords * 0.8f;
    std::vector<std::pair<float, long>> scored, acc;
    for (const auto &p : sharing) {
        KeyFrameFields &s = state[p.first];
        if (s.mnLoopWords > minCommonWords) {
            const float si = (float)p.second;
            s.mLoopScore = si;
            if (si >= minScore) scored.push_back({si, p.first});
        }
    }
    if (scored.empty()) return {};
    float bestAccScore = minScore;
    for (const auto &it : scored) {
        float bestScore = it.first, accScore = it.first;
        long best = it.second;
        const auto cv = best_covisibles.find(it.second);
        if (cv != best_covisibles.end())
            for (long kf2 : cv->second) {
                const KeyFrameFields &s2 = state[kf2];
                if (s2.mnLoopQuery == query_id && s2.mnLoopWords > minCommonWords) {
                    accScore += s2.mLoopScore;
                    if (s2.mLoopScore > bestScore) { best = kf2; bestScore = s2.mLoopScore; }
                }
            }
        acc.push_back({accScore, best});
        if (accScore > bestAccScore) bestAccScore = accScore;
    }
    return bow_detail::retain(acc, bestAccScore);
}

// KeyFrameDatabase::DetectRelocalizationCandidates (:196-305) behind the scores
inline std::vector<long> DetectRelocalizationCandidatesFromShared(KeyFrameState &state, std::vector<SharedWords> shared, long query_id, const Covisibles &best_covisibles) {
    bow_detail::first_encounter_order(shared);
    std::vector<std::pair<long, double>> sharing;
    for (const SharedWords &e : shared) {
        KeyFrameFields &s = state[e.id];
        if (s.mnRelocQuery != query_id) {
            s.mnRelocWords = 0;
            s.mnRelocQuery = query_id;
            sharing.push_back({e.id, e.score});
        }
        s.mnRelocWords += e.common;
    }
    if (sharing.empty()) return {};
    int maxCommonWords = 0;
    for (const auto &p : sharing) maxCommonWords = std::max(maxCommonWords, state[p.first].mnRelocWords);
    const int minCommonWords = maxCommonWords * 0.8f;
    std::vector<std::pair<float, long>> scored, acc;
    for (const auto &p : sharing) {
        KeyFrameFields &s = state[p.first];
        if (s.mnRelocWords > minCommonWords) {
            s.mRelocScore = (float)p.second;
            scored.push_back({s.mRelocScore, p.first});
        }
    }
    if (scored.empty()) return {};
    float bestAccScore = 0;
    for (const auto &it : scored) {
        float bestScore = it.first, accScore = bestScore;
        long best = it.second;
        const auto cv = best_covisibles.find(it.second);
        if (cv != best_covisibles.end())
            for (long kf2 : cv->second) {
                const KeyFrameFields &s2 = state[kf2];
                if (s2.mnRelocQuery != query_id) continue;
                accScore += s2.mRelocScore; // of a neighbour not scored in this query: what an earlier query left (:270-273)
                if (s2.mRelocScore > bestScore) { best = kf2; bestScore = s2.mRelocScore; }
            }
        acc.push_back({accScore, best});
        if (accScore > bestAccScore) bestAccScore = accScore;
    }
    return bow_detail::retain(acc, bestAccScore);
}

class KeyFrameDatabase {
  public:
    explicit KeyFrameDatabase(Context &c) : ctx_(c) {
        const int r = cs_bow_db_create(ctx_.ctx, &db_);
        if (r != CS_OK) throw std::runtime_error("cs_bow_db_create failed");
    }
    ~KeyFrameDatabase() { cs_bow_db_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;
    void add(long kf, const BowVector &bow) {
        std::vector<int> w;
        std::vector<double> x;
        for (const auto &e : bow) { w.push_back(e.first); x.push_back(e.second); }
        ok(cs_bow_db_add(ctx_.ctx, db_, kf, (int)w.size(), w.data(), x.data()), "cs_bow_db_add");
        state[kf];
    }
    void erase(long kf) { ok(cs_bow_db_erase(db_, kf), "cs_bow_db_erase"); }
    void clear() { ok(cs_bow_db_clear(db_), "cs_bow_db_clear"); }
    // cs_bow_db_query for one BowVector: the key frames that share a word with it, in add order
    std::vector<SharedWords> query(const BowVector &bow) {
        int nk = 0;
        ok(cs_bow_db_size(db_, &nk), "cs_bow_db_size");
        std::vector<int> off{0, (int)bow.size()}, w, oq((size_t)nk + 1), oc((size_t)nk + 1), om((size_t)nk + 1);
        std::vector<double> x, os((size_t)nk + 1);
        std::vector<long> oid((size_t)nk + 1), oo((size_t)nk + 1);
        for (const auto &e : bow) { w.push_back(e.first); x.push_back(e.second); }
        w.push_back(0); x.push_back(0);
        long n = 0;
        ok(cs_bow_db_query(ctx_.ctx, db_, 1, off.data(), w.data(), x.data(), nk, &n, oq.data(), oid.data(), oo.data(), oc.data(), om.data(), os.data()), "cs_bow_db_query");
        std::vector<SharedWords> out;
        for (long i = 0; i < n; ++i) out.push_back({oid[i], oc[i], om[i], oo[i], os[i]});
        return out;
    }
    std::vector<long> DetectLoopCandidates(long query_id, const BowVector &bow, const std::set<long> &connected, const Covisibles &best_covisibles, float minScore) {
        return DetectLoopCandidatesFromShared(state, query(bow), query_id, connected, best_covisibles, minScore);
    }
    std::vector<long> DetectRelocalizationCandidates(long query_id, const BowVector &bow, const Covisibles &best_covisibles) {
        return DetectRelocalizationCandidatesFromShared(state, query(bow), query_id, best_covisibles);
    }
    KeyFrameState state; // a key frame keeps its fields when it is erased, as the KeyFrame object does

  private:
    void ok(int r, const char *what) {
        if (r != CS_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(r) + "): " + cs_last_error(ctx_.ctx));
    }
    Context &ctx_;
    cs_bow_db *db_ = nullptr;
};

} // namespace cubeslam
