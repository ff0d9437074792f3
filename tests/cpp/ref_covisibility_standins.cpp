// TEST INFRASTRUCTURE: stand-ins for the SLAM classes that the reference's covisibility functions touch -- KeyFrame::UpdateConnections, AddConnection, UpdateBestCovisibles and
// SetBadFlag (orb_object_slam/src/KeyFrame.cc:345-437, :140-180, :511-604), MapPoint::EraseObservation and SetBadFlag (MapPoint.cc:178-205, :287-307),
// LocalMapping::KeyFrameCulling and MapPointCulling (LocalMapping.cc:833-902, :249-302).  tests/test_covisibility_restatement_pins.py cuts those functions out of the reference at
// test time into a temporary directory (ref_covisibility_extracted.inc), compiles this file around them there and runs them next to tests/covisibility_restatement.py on the
// same tables.  The classes carry just the members those functions read, under the reference's names; every statement of the functions is the reference's.
// The key frames live in ONE array: the pointer order of the reference's std::map<KeyFrame *, ...> is then their index order.
// A key frame's per-key-point arrays hold its slots first (mvpMapPoints, mvDepth, and mvKeysUn[i].octave = slot_octave) and behind them one key point per observation entry
// that names the key frame (octave = obs_octave, mvuRight >= 0 where obs_stereo): the table gives the two octaves separately, so they live at separate indices.
#include <algorithm>
#include <cstdint>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <vector>

namespace ORB_SLAM2 {
using namespace std;

bool whether_dynamic_object = false, use_dynamic_klt_features = false, mono_allframe_Obj_depth_init = false; // Parameters.h:38-44

struct KeyPoint { int octave = 0; };
struct Pose { Pose operator*(const Pose &) const { return Pose(); } }; // Tcw, mTcp: not observed here

class KeyFrame;
class MapPoint;
class Map {
  public:
    void EraseMapPoint(MapPoint *) {}
    void EraseKeyFrame(KeyFrame *) {}
};
class KeyFrameDatabase {
  public:
    void erase(KeyFrame *) {}
};

class MapPoint {
  public:
    std::map<KeyFrame *, size_t> mObservations;
    int nObs = 0, mnFound = 1, mnVisible = 1;
    long int mnFirstKFid = 0;
    bool mbBad = false, is_dynamic = false;
    KeyFrame *mpRefKF = nullptr;
    Map *mpMap = nullptr;
    std::mutex mMutexFeatures, mMutexPos;
    bool isBad() { return mbBad; }
    int Observations() { return nObs; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    float GetFoundRatio() { return static_cast<float>(mnFound) / mnVisible; } // MapPoint.cc:375-379
    void EraseObservation(KeyFrame *pKF);
    void SetBadFlag();
};

class KeyFrame {
  public:
    long unsigned int mnId = 0;
    std::vector<MapPoint *> mvpMapPoints, mvpMapPointsHarris;
    std::vector<float> mvuRight, mvDepth;
    std::vector<KeyPoint> mvKeysUn;
    float mThDepth = 0;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = true, mbNotErase = false, mbToBeErased = false, mbBad = false;
    KeyFrame *mpParent = nullptr;
    std::set<KeyFrame *> mspChildrens;
    Pose Tcw, mTcp;
    Map *mpMap = nullptr;
    KeyFrameDatabase *mpKeyFrameDB = nullptr;
    std::mutex mMutexConnections, mMutexFeatures;
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    int GetWeight(KeyFrame *pKF) { return mConnectedKeyFrameWeights.count(pKF) ? mConnectedKeyFrameWeights[pKF] : 0; }
    bool isBad() { return mbBad; }
    void AddChild(KeyFrame *pKF) { mspChildrens.insert(pKF); }
    void EraseChild(KeyFrame *pKF) { mspChildrens.erase(pKF); }
    void ChangeParent(KeyFrame *pKF) { mpParent = pKF; pKF->AddChild(this); }
    Pose GetPoseInverse() { return Pose(); }
    void EraseMapPointMatch(const size_t &idx) { if (idx < mvpMapPoints.size()) mvpMapPoints[idx] = nullptr; } // (an observation's key point lies behind the slots here)
    void EraseHarrisMapPointMatch(const size_t &) {}
    void EraseConnection(KeyFrame *pKF) { // KeyFrame.cc:611-625
        if (mConnectedKeyFrameWeights.count(pKF)) { mConnectedKeyFrameWeights.erase(pKF); UpdateBestCovisibles(); }
    }
    void AddConnection(KeyFrame *pKF, const int &weight);
    void UpdateBestCovisibles();
    void UpdateConnections();
    void SetBadFlag();
};

class LocalMapping {
  public:
    bool mbMonocular = false;
    KeyFrame *mpCurrentKeyFrame = nullptr;
    std::list<MapPoint *> mlpRecentAddedMapPoints;
    void MapPointCulling();
    void KeyFrameCulling();
};

#include "ref_covisibility_extracted.inc"

} // namespace ORB_SLAM2

using namespace ORB_SLAM2;

namespace {
struct World {
    std::vector<KeyFrame> kfs; // [n_kf] and one more: the parent every key frame hangs on while KeyFrame::SetBadFlag runs (it is in no list and observes nothing)
    std::vector<MapPoint> mps;
    std::vector<std::vector<std::pair<int, int>>> entry_of; // per point: (key frame, entry) of the table
    Map map;
    KeyFrameDatabase db;
};
// the table as objects.  Slot lists: list i belongs to key frame list_kf[i]
void build(World &w, int n_kf, int n_points, const int *obs_off, const int *obs_kf, const int *obs_octave, const uint8_t *obs_stereo, const int *mp_nobs, const uint8_t *mp_flags,
           int n_lists, const int *list_kf, const int *kf_off, const int *kf_mp, const int *slot_octave, const float *slot_depth) {
    w.kfs = std::vector<KeyFrame>((size_t)n_kf + 1);
    w.mps = std::vector<MapPoint>((size_t)n_points);
    w.entry_of.assign((size_t)n_points, {});
    for (int k = 0; k <= n_kf; k++) { w.kfs[(size_t)k].mnId = (long unsigned)k + 1; w.kfs[(size_t)k].mpMap = &w.map; w.kfs[(size_t)k].mpKeyFrameDB = &w.db; }
    for (int i = 0; i < n_lists; i++) {
        KeyFrame &kf = w.kfs[(size_t)list_kf[i]];
        if (!kf.mvpMapPoints.empty() || kf_off[i + 1] == kf_off[i]) continue; // (a key frame queried twice has one list)
        for (int s = kf_off[i]; s < kf_off[i + 1]; s++) {
            kf.mvpMapPoints.push_back(kf_mp[s] < 0 ? nullptr : &w.mps[(size_t)kf_mp[s]]);
            KeyPoint kp; kp.octave = slot_octave ? slot_octave[s] : 0;
            kf.mvKeysUn.push_back(kp); kf.mvuRight.push_back(-1.f); kf.mvDepth.push_back(slot_depth ? slot_depth[s] : 1.f);
        }
    }
    for (int p = 0; p < n_points; p++) {
        MapPoint &mp = w.mps[(size_t)p];
        mp.nObs = mp_nobs[p]; mp.mbBad = mp_flags[p] & 1; mp.is_dynamic = mp_flags[p] & 2; mp.mpMap = &w.map;
        if (mp.mbBad || !obs_off) continue; // MapPoint::SetBadFlag has cleared its observations
        for (int e = obs_off[p]; e < obs_off[p + 1]; e++) {
            KeyFrame &kf = w.kfs[(size_t)obs_kf[e]];
            KeyPoint kp; kp.octave = obs_octave[e];
            mp.mObservations[&kf] = kf.mvKeysUn.size();
            kf.mvKeysUn.push_back(kp); kf.mvuRight.push_back(obs_stereo[e] ? 1.f : -1.f);
            w.entry_of[(size_t)p].push_back(std::make_pair(obs_kf[e], e));
        }
        if (!mp.mObservations.empty()) mp.mpRefKF = mp.mObservations.begin()->first;
    }
}
void point_state(World &w, int n_points, int *out_nobs, uint8_t *out_flags, uint8_t *out_alive) {
    for (int p = 0; p < n_points; p++) {
        MapPoint &mp = w.mps[(size_t)p];
        out_nobs[p] = mp.nObs; out_flags[p] = (uint8_t)((mp.mbBad ? 1 : 0) | (mp.is_dynamic ? 2 : 0));
        for (const auto &ke : w.entry_of[(size_t)p]) out_alive[ke.second] = mp.mObservations.count(&w.kfs[(size_t)ke.first]) ? 1 : 0;
    }
}
} // namespace

extern "C" {

// UpdateConnections of the queries in order.  out: per key frame that has a connection or a parent: k, n, ordered key frames[n], ordered weights[n], m, (key frame, weight)[m]
// ascending, parent, mbFirstConnection, the children ascending preceded by their number.  Returns the number of words (or -1: out is too small).
int pin_update_connections(int n_kf, int n_points, const int *obs_off, const int *obs_kf, const int *obs_octave, const uint8_t *obs_stereo, const int *mp_nobs, const uint8_t *mp_flags,
                           int n_query, const int *query_kf, const int *kf_off, const int *kf_mp, const int *mn_id, int skip_dynamic, int *out, int cap) {
    World w;
    build(w, n_kf, n_points, obs_off, obs_kf, obs_octave, obs_stereo, mp_nobs, mp_flags, 0, nullptr, kf_off, nullptr, nullptr, nullptr); // (the lists: per query, below)
    for (int k = 0; k < n_kf; k++) w.kfs[(size_t)k].mnId = (long unsigned)mn_id[k];
    whether_dynamic_object = skip_dynamic != 0;
    for (int q = 0; q < n_query; q++) {
        KeyFrame &kf = w.kfs[(size_t)query_kf[q]];
        kf.mvpMapPoints.clear(); // (a key frame may be queried twice, with another list)
        for (int s = kf_off[q]; s < kf_off[q + 1]; s++) kf.mvpMapPoints.push_back(kf_mp[s] < 0 ? nullptr : &w.mps[(size_t)kf_mp[s]]);
        kf.UpdateConnections();
    }
    std::vector<int> o;
    auto index = [&](KeyFrame *p) { return p ? (int)(p - w.kfs.data()) : -1; };
    for (int k = 0; k < n_kf; k++) {
        KeyFrame &kf = w.kfs[(size_t)k];
        if (kf.mConnectedKeyFrameWeights.empty() && !kf.mpParent) continue;
        o.push_back(k); o.push_back((int)kf.mvpOrderedConnectedKeyFrames.size());
        for (KeyFrame *c : kf.mvpOrderedConnectedKeyFrames) o.push_back(index(c));
        for (int v : kf.mvOrderedWeights) o.push_back(v);
        o.push_back((int)kf.mConnectedKeyFrameWeights.size());
        for (const auto &kv : kf.mConnectedKeyFrameWeights) { o.push_back(index(kv.first)); o.push_back(kv.second); }
        o.push_back(index(kf.mpParent)); o.push_back(kf.mbFirstConnection ? 1 : 0);
        o.push_back((int)kf.mspChildrens.size());
        for (KeyFrame *c : kf.mspChildrens) o.push_back(index(c));
    }
    if ((int)o.size() > cap) return -1;
    std::copy(o.begin(), o.end(), out);
    return (int)o.size();
}

// KeyFrameCulling over local_kf (the current key frame's GetVectorCovisibleKeyFrames).  state[i]: bit 0 mbBad, bit 1 mbToBeErased of local_kf[i] afterwards
void pin_keyframe_culling(int n_kf, int n_points, const int *obs_off, const int *obs_kf, const int *obs_octave, const uint8_t *obs_stereo, const int *mp_nobs, const uint8_t *mp_flags,
                          int n_local, const int *local_kf, const int *kf_off, const int *kf_mp, const int *slot_octave, const float *slot_depth, const float *kf_th_depth,
                          int monocular, const uint8_t *kf_flags, uint8_t *state, int *out_nobs, uint8_t *out_flags, uint8_t *out_alive) {
    World w;
    build(w, n_kf, n_points, obs_off, obs_kf, obs_octave, obs_stereo, mp_nobs, mp_flags, n_local, local_kf, kf_off, kf_mp, slot_octave, slot_depth);
    KeyFrame &root = w.kfs[(size_t)n_kf];
    LocalMapping lm;
    lm.mbMonocular = monocular != 0;
    lm.mpCurrentKeyFrame = &root;
    for (int i = 0; i < n_local; i++) {
        KeyFrame &kf = w.kfs[(size_t)local_kf[i]];
        kf.mThDepth = kf_th_depth[i];
        if (kf_flags[i] & 1) kf.mnId = 0;
        kf.mbNotErase = (kf_flags[i] & 2) != 0;
        kf.mpParent = &root; // KeyFrame::SetBadFlag reads its parent (:598-599)
        root.mvpOrderedConnectedKeyFrames.push_back(&kf);
    }
    lm.KeyFrameCulling();
    for (int i = 0; i < n_local; i++) { KeyFrame &kf = w.kfs[(size_t)local_kf[i]]; state[i] = (uint8_t)((kf.mbBad ? 1 : 0) | (kf.mbToBeErased ? 2 : 0)); }
    point_state(w, n_points, out_nobs, out_flags, out_alive);
}

// MapPointCulling.  th_obs selects the reference's branch (:258-268): 3 stereo, 2 monocular, 1 monocular with mono_allframe_Obj_depth_init.  remains[i] = the entry is still in
// the list; out_flags: the points' flags afterwards
void pin_mappoint_culling(int n_points, const int *mp_nobs, const uint8_t *mp_flags, int n_recent, const int *recent, const int *mp_found, const int *mp_visible,
                          const int *mp_first_kf_id, int current_kf_id, int th_obs, uint8_t *remains, uint8_t *out_flags) {
    World w;
    const int zero = 0;
    build(w, 1, n_points, nullptr, nullptr, nullptr, nullptr, mp_nobs, mp_flags, 0, nullptr, &zero, nullptr, nullptr, nullptr);
    for (int p = 0; p < n_points; p++) { w.mps[(size_t)p].mnFound = mp_found[p]; w.mps[(size_t)p].mnVisible = mp_visible[p]; w.mps[(size_t)p].mnFirstKFid = mp_first_kf_id[p]; }
    LocalMapping lm;
    lm.mbMonocular = th_obs != 3;
    mono_allframe_Obj_depth_init = th_obs == 1;
    w.kfs[0].mnId = (long unsigned)current_kf_id;
    lm.mpCurrentKeyFrame = &w.kfs[0];
    // an entry is known by its address in the list's nodes: a point may stand in the list twice
    for (int i = 0; i < n_recent; i++) lm.mlpRecentAddedMapPoints.push_back(&w.mps[(size_t)recent[i]]);
    std::vector<const MapPoint *const *> nodes;
    for (auto it = lm.mlpRecentAddedMapPoints.begin(); it != lm.mlpRecentAddedMapPoints.end(); ++it) nodes.push_back(&*it);
    lm.MapPointCulling();
    std::set<const MapPoint *const *> left;
    for (auto it = lm.mlpRecentAddedMapPoints.begin(); it != lm.mlpRecentAddedMapPoints.end(); ++it) left.insert(&*it);
    for (int i = 0; i < n_recent; i++) remains[i] = left.count(nodes[(size_t)i]) ? 1 : 0;
    for (int p = 0; p < n_points; p++) out_flags[p] = (uint8_t)((w.mps[(size_t)p].mbBad ? 1 : 0) | (w.mps[(size_t)p].is_dynamic ? 2 : 0));
}

} // extern "C"
