// Stand-ins around the reference's own DBoW2 / KeyFrameDatabase text for tests/test_bow_restatement_pins.py.  Compiled at test time, outside the repository, with
//   ref_bow_voc_extracted.inc   both TemplatedVocabulary::transform overloads and loadFromTextFile, cut out of TemplatedVocabulary.h
//                               (the header itself needs cv::FileStorage for its save / load, which nothing here uses)
//   ref_bow_score_extracted.inc L1Scoring::score, cut out of ScoringObject.cpp (whose other scoring classes include the whole vocabulary header)
//   ref_bow_db_extracted.inc    KeyFrameDatabase's constructor, add, erase, clear, DetectLoopCandidates and DetectRelocalizationCandidates, cut out of KeyFrameDatabase.cc
// and linked with the reference's FORB.cpp, BowVector.cpp and FeatureVector.cpp compiled where they lie.  What is declared here is ours: the class shells the cut functions
// are members of (the fields and the four one-line accessors they touch), KeyFrame / Frame with the fields the database reads and writes, and a flat C interface.
#include <cmath>
#include <cstring>
#include <fstream>
#include <iostream>
#include <list>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "cvshim.hpp"

#include "BowVector.h"
#include "FORB.h"
#include "FeatureVector.h"
#include "ScoringObject.h"

using namespace std;

namespace DBoW2 {

template <class TDescriptor, class F> class TemplatedVocabulary {
  public:
    struct Node {
        NodeId id;
        WordValue weight;
        vector<NodeId> children;
        NodeId parent;
        TDescriptor descriptor;
        WordId word_id;
        Node() : id(0), weight(0), parent(0), word_id(0) {}
        Node(NodeId _id) : id(_id), weight(0), parent(0), word_id(0) {}
        inline bool isLeaf() const { return children.empty(); }
    };
    TemplatedVocabulary() : m_k(0), m_L(0), m_weighting(TF_IDF), m_scoring(L1_NORM), m_scoring_object(NULL) {}
    ~TemplatedVocabulary() { delete m_scoring_object; }
    inline bool empty() const { return m_words.empty(); }
    inline unsigned int size() const { return (unsigned int)m_words.size(); }
    inline double score(const BowVector &a, const BowVector &b) const { return m_scoring_object->score(a, b); }
    void createScoringObject() { // the reference's switch over six scoring classes; five of them live in ScoringObject.cpp beside code that needs the whole header
        delete m_scoring_object;
        m_scoring_object = m_scoring == L1_NORM ? new L1Scoring : NULL;
    }
    void transform(const std::vector<TDescriptor> &features, BowVector &v, FeatureVector &fv, int levelsup) const;
    void transform(const TDescriptor &feature, WordId &id, WordValue &weight, NodeId *nid = NULL, int levelsup = 0) const;
    bool loadFromTextFile(const std::string &filename);
    int m_k, m_L;
    WeightingType m_weighting;
    ScoringType m_scoring;
    GeneralScoring *m_scoring_object;
    std::vector<Node> m_nodes;
    std::vector<Node *> m_words;
};

#include "ref_bow_voc_extracted.inc"
#include "ref_bow_score_extracted.inc"

} // namespace DBoW2

namespace ORB_SLAM2 {

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> ORBVocabulary;

class KeyFrame {
  public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    long unsigned int mnLoopQuery = 0; int mnLoopWords = 0; float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0; int mnRelocWords = 0; float mRelocScore = 0; // the reference's constructor leaves mRelocScore uninitialised
    std::set<KeyFrame *> connected;
    std::vector<KeyFrame *> covisibles;
    std::set<KeyFrame *> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) {
        return (int)covisibles.size() < N ? covisibles : std::vector<KeyFrame *>(covisibles.begin(), covisibles.begin() + N);
    }
};
class Frame {
  public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};
class KeyFrameDatabase {
  public:
    KeyFrameDatabase(const ORBVocabulary &voc);
    void add(KeyFrame *pKF);
    void erase(KeyFrame *pKF);
    void clear();
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore);
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F);
    const ORBVocabulary *mpVoc;
    std::vector<std::list<KeyFrame *>> mvInvertedFile;
    std::mutex mMutex;
};

#include "ref_bow_db_extracted.inc"

} // namespace ORB_SLAM2

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::ORBVocabulary;

static DBoW2::BowVector bow_of(int n, const int *w, const double *x) {
    DBoW2::BowVector b;
    for (int i = 0; i < n; ++i) b[(DBoW2::WordId)w[i]] = x[i];
    return b;
}
static cv::Mat mat_of(const uint8_t *d) {
    cv::Mat m(1, 32, CV_8U);
    memcpy(m.ptr<unsigned char>(), d, 32);
    return m;
}

#define PIN extern "C" __attribute__((visibility("default")))

PIN void *pin_voc_load(const char *file) {
    ORBVocabulary *v = new ORBVocabulary;
    if (!v->loadFromTextFile(file)) { delete v; return NULL; }
    return v;
}
PIN void pin_voc_info(void *p, int *k, int *L, int *n_nodes, int *n_words, int *scoring, int *weighting) {
    ORBVocabulary *v = (ORBVocabulary *)p;
    *k = v->m_k; *L = v->m_L; *n_nodes = (int)v->m_nodes.size(); *n_words = (int)v->m_words.size(); *scoring = (int)v->m_scoring; *weighting = (int)v->m_weighting;
}
PIN void pin_voc_nodes(void *p, int *parent, int *n_children, uint8_t *desc, int *desc_cols, double *weight, int *word_id) {
    ORBVocabulary *v = (ORBVocabulary *)p;
    for (size_t i = 0; i < v->m_nodes.size(); ++i) {
        const ORBVocabulary::Node &n = v->m_nodes[i];
        parent[i] = (int)n.parent; n_children[i] = (int)n.children.size(); weight[i] = n.weight; word_id[i] = (int)n.word_id; desc_cols[i] = n.descriptor.cols;
        if (n.descriptor.cols == 32) memcpy(desc + 32 * i, n.descriptor.ptr<unsigned char>(), 32);
    }
}
PIN void pin_voc_words(void *p, int *node_of_word) {
    ORBVocabulary *v = (ORBVocabulary *)p;
    for (size_t i = 0; i < v->m_words.size(); ++i) node_of_word[i] = (int)v->m_words[i]->id;
}
PIN int pin_distance(const uint8_t *a, const uint8_t *b) { return DBoW2::FORB::distance(mat_of(a), mat_of(b)); }
PIN void pin_from_string(const char *s, uint8_t *out) {
    cv::Mat m;
    DBoW2::FORB::fromString(m, s);
    memcpy(out, m.ptr<unsigned char>(), 32);
}
PIN void pin_transform_feature(void *p, const uint8_t *d, int levelsup, int *word, double *weight, int *nid) {
    DBoW2::WordId id; DBoW2::WordValue w; DBoW2::NodeId n = 0xffffffffu;
    ((ORBVocabulary *)p)->transform(mat_of(d), id, w, &n, levelsup);
    *word = (int)id; *weight = w; *nid = (int)n;
}
// transform(features, v, fv, levelsup): the BowVector in map order, the FeatureVector as (node, feature) pairs in map / vector order; returns the BowVector's size
PIN int pin_transform(void *p, int n, const uint8_t *desc, int levelsup, int *bow_word, double *bow_value, int *n_fv, int *fv_node, int *fv_feature) {
    std::vector<cv::Mat> f;
    for (int i = 0; i < n; ++i) f.push_back(mat_of(desc + 32 * i));
    DBoW2::BowVector v;
    DBoW2::FeatureVector fv;
    ((ORBVocabulary *)p)->transform(f, v, fv, levelsup);
    int i = 0, j = 0;
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it, ++i) { bow_word[i] = (int)it->first; bow_value[i] = it->second; }
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it)
        for (size_t q = 0; q < it->second.size(); ++q, ++j) { fv_node[j] = (int)it->first; fv_feature[j] = (int)it->second[q]; }
    *n_fv = j;
    return i;
}
PIN double pin_score(void *p, int n1, const int *w1, const double *x1, int n2, const int *w2, const double *x2) {
    return ((ORBVocabulary *)p)->score(bow_of(n1, w1, x1), bow_of(n2, w2, x2));
}
PIN void *pin_db_create(void *voc) { return new ORB_SLAM2::KeyFrameDatabase(*(ORBVocabulary *)voc); }
PIN void *pin_kf_create(long id, int n, const int *w, const double *x) {
    KeyFrame *k = new KeyFrame;
    k->mnId = (long unsigned int)id; k->mBowVec = bow_of(n, w, x);
    return k;
}
PIN void pin_kf_set_neighbours(void *kf, int n_connected, void **connected, int n_covisibles, void **covisibles) {
    KeyFrame *k = (KeyFrame *)kf;
    k->connected.clear(); k->covisibles.clear();
    for (int i = 0; i < n_connected; ++i) k->connected.insert((KeyFrame *)connected[i]);
    for (int i = 0; i < n_covisibles; ++i) k->covisibles.push_back((KeyFrame *)covisibles[i]);
}
PIN void pin_db_add(void *db, void *kf) { ((ORB_SLAM2::KeyFrameDatabase *)db)->add((KeyFrame *)kf); }
PIN void pin_db_erase(void *db, void *kf) { ((ORB_SLAM2::KeyFrameDatabase *)db)->erase((KeyFrame *)kf); }
PIN void pin_db_clear(void *db) { ((ORB_SLAM2::KeyFrameDatabase *)db)->clear(); }
PIN int pin_detect_loop(void *db, void *query_kf, float minScore, long *out) {
    const std::vector<KeyFrame *> r = ((ORB_SLAM2::KeyFrameDatabase *)db)->DetectLoopCandidates((KeyFrame *)query_kf, minScore);
    for (size_t i = 0; i < r.size(); ++i) out[i] = (long)r[i]->mnId;
    return (int)r.size();
}
PIN int pin_detect_reloc(void *db, long id, int n, const int *w, const double *x, long *out) {
    ORB_SLAM2::Frame F;
    F.mnId = (long unsigned int)id; F.mBowVec = bow_of(n, w, x);
    const std::vector<KeyFrame *> r = ((ORB_SLAM2::KeyFrameDatabase *)db)->DetectRelocalizationCandidates(&F);
    for (size_t i = 0; i < r.size(); ++i) out[i] = (long)r[i]->mnId;
    return (int)r.size();
}
