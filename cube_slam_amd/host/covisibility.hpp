// covisibility.hpp -- the graph work at both ends of ORB_SLAM2::LocalMapping's key-frame cycle with the reference's names, over the C-ABI extension
// (include/cubeslam_hip/covisibility.h) and plain arrays:
//   cubeslam::Covisibility::UpdateConnections   KeyFrame::UpdateConnections (orb_object_slam/src/KeyFrame.cc:345-437) for a batch of key frames, then the AddConnection /
//                                               UpdateBestCovisibles calls (:140-180) and the first-connection parent (:424-429) in query order
//   cubeslam::Covisibility::KeyFrameCulling     LocalMapping::KeyFrameCulling (LocalMapping.cc:833-902) with the EraseObservation chain of every culled key frame
//   cubeslam::Covisibility::MapPointCulling     LocalMapping::MapPointCulling (:249-302): one case per entry of the recent list
// A null Context pointer takes the library's host forms.  The caller keeps the new mpRefKF of a point (its lowest alive index) and the connection and spanning-tree repair of
// KeyFrame::SetBadFlag :524-604.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/cubeslam_hip/covisibility.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context

namespace cubeslam {

// mObservations of every point as runs of ascending key-frame index, MapPoint::nObs and the point flags (bit 0 isBad, bit 1 is_dynamic)
struct ObsTable {
    int n_kf = 0;
    std::vector<int> obs_off{0}, obs_kf, obs_octave; // octave: pKFi->mvKeysUn[idx].octave of the observation
    std::vector<uint8_t> obs_stereo;                 // pKFi->mvuRight[idx] >= 0
    std::vector<int> mp_nobs;
    std::vector<uint8_t> mp_flags;
    int n_points() const { return (int)mp_nobs.size(); }
    cs_obs_table c_struct() const {
        if (obs_off.size() != mp_nobs.size() + 1 || mp_flags.size() != mp_nobs.size() || obs_octave.size() != obs_kf.size() || obs_stereo.size() != obs_kf.size())
            throw std::invalid_argument("ObsTable: arrays disagree in length");
        return cs_obs_table{n_kf, n_points(), obs_off.data(), obs_kf.data(), obs_octave.data(), obs_stereo.data(), mp_nobs.data(), mp_flags.data()};
    }
};

// key-frame lists: GetMapPointMatches() of list entry i = mp[off[i] .. off[i + 1]), indices into the point table, -1 no point
struct SlotLists {
    std::vector<int> off{0}, mp;
};

struct ConnectionVotes { // cs_covisibility_update's results
    std::vector<int> cnt_off, cnt_kf, cnt_w, kf_max, w_max, ord_off, ord_kf, ord_w;
};

// the connection side of the key-frame table as KeyFrame holds it
struct Connections {
    std::vector<std::map<int, int>> mConnectedKeyFrameWeights;
    std::vector<std::vector<int>> mvpOrderedConnectedKeyFrames, mvOrderedWeights, mspChildrens;
    std::vector<int> mpParent, mnId;
    std::vector<uint8_t> mbFirstConnection;
    explicit Connections(int n_kf)
        : mConnectedKeyFrameWeights((size_t)n_kf), mvpOrderedConnectedKeyFrames((size_t)n_kf), mvOrderedWeights((size_t)n_kf), mspChildrens((size_t)n_kf), mpParent((size_t)n_kf, -1),
          mnId((size_t)n_kf), mbFirstConnection((size_t)n_kf, 1) {
        for (int k = 0; k < n_kf; k++) mnId[(size_t)k] = k;
    }
    void AddConnection(int k, int pKF, int weight) { // :140-156
        auto &w = mConnectedKeyFrameWeights[(size_t)k];
        auto it = w.find(pKF);
        if (it != w.end() && it->second == weight) return;
        w[pKF] = weight;
        UpdateBestCovisibles(k);
    }
    void UpdateBestCovisibles(int k) { // :158-178: sort ascending on (weight, pointer), then push_front
        std::vector<std::pair<int, int>> vPairs;
        for (const auto &kv : mConnectedKeyFrameWeights[(size_t)k]) vPairs.push_back(std::make_pair(kv.second, kv.first));
        std::sort(vPairs.begin(), vPairs.end());
        auto &kfs = mvpOrderedConnectedKeyFrames[(size_t)k];
        auto &ws = mvOrderedWeights[(size_t)k];
        kfs.clear(); ws.clear();
        for (auto it = vPairs.rbegin(); it != vPairs.rend(); ++it) { kfs.push_back(it->second); ws.push_back(it->first); }
    }
};

struct KeyFrameCullingResult {
    std::vector<uint8_t> verdict;                    // 0 kept, 1 culled and erased, 2 mbToBeErased only, 3 mnId == 0
    std::vector<int> n_mps, n_redundant, mp_nobs;    // nMPs / nRedundantObservations per key frame; the final nObs
    std::vector<uint8_t> mp_flags, alive;            // the final point flags; one alive byte per observation entry
    int n_rounds = 0;
};

class Covisibility {
  public:
    explicit Covisibility(Context *c = nullptr) : ctx_(c) {}

    ConnectionVotes Votes(const ObsTable &table, const std::vector<int> &queries, const SlotLists &lists, bool whether_dynamic_object = false, int th = 15) const {
        const cs_obs_table t = table.c_struct();
        const int n = (int)queries.size();
        if (lists.off.size() != queries.size() + 1) throw std::invalid_argument("UpdateConnections: one slot list per query");
        ConnectionVotes v;
        v.cnt_off.assign((size_t)n + 1, 0); v.ord_off.assign((size_t)n + 1, 0); v.kf_max.assign((size_t)n, -1); v.w_max.assign((size_t)n, 0);
        int cap = 0;
        for (int pass = 0; pass < 2; pass++) { // a first call without room reports the sizes
            v.cnt_kf.assign((size_t)cap + 1, 0); v.cnt_w.assign((size_t)cap + 1, 0); v.ord_kf.assign((size_t)cap + 1, 0); v.ord_w.assign((size_t)cap + 1, 0);
            const int r = ctx_ ? cs_covisibility_update(ctx_->ctx, &t, n, queries.data(), lists.off.data(), lists.mp.data(), whether_dynamic_object, th, cap, v.cnt_off.data(),
                                                        v.cnt_kf.data(), v.cnt_w.data(), v.kf_max.data(), v.w_max.data(), v.ord_off.data(), v.ord_kf.data(), v.ord_w.data())
                               : cs_covisibility_update_host(&t, n, queries.data(), lists.off.data(), lists.mp.data(), whether_dynamic_object, th, cap, v.cnt_off.data(),
                                                             v.cnt_kf.data(), v.cnt_w.data(), v.kf_max.data(), v.w_max.data(), v.ord_off.data(), v.ord_kf.data(), v.ord_w.data());
            if (r == CS_OK) break;
            if (r != CS_ERR_CAPACITY || pass == 1) fail("cs_covisibility_update", r);
            cap = v.cnt_off[(size_t)n];
        }
        v.cnt_kf.resize((size_t)v.cnt_off[(size_t)n]); v.cnt_w.resize(v.cnt_kf.size());
        v.ord_kf.resize((size_t)v.ord_off[(size_t)n]); v.ord_w.resize(v.ord_kf.size());
        return v;
    }

    // one library call for the batch, then what the reference does with each result, in query order.  A query with an empty counter leaves everything as it is (:382).
    ConnectionVotes UpdateConnections(const ObsTable &table, const std::vector<int> &queries, const SlotLists &lists, Connections &c, bool whether_dynamic_object = false,
                                      int th = 15) const {
        const ConnectionVotes v = Votes(table, queries, lists, whether_dynamic_object, th);
        for (size_t q = 0; q < queries.size(); q++) {
            const int kf = queries[q], c0 = v.cnt_off[q], c1 = v.cnt_off[q + 1], o0 = v.ord_off[q], o1 = v.ord_off[q + 1];
            if (c1 == c0) continue;
            std::vector<std::pair<int, int>> calls; // (key frame, weight): the walk over KFcounter is ascending
            for (int i = o0; i < o1; i++) calls.push_back(std::make_pair(v.ord_kf[(size_t)i], v.ord_w[(size_t)i]));
            std::sort(calls.begin(), calls.end());
            for (const auto &p : calls) c.AddConnection(p.first, kf, p.second);
            auto &w = c.mConnectedKeyFrameWeights[(size_t)kf];
            w.clear();
            for (int i = c0; i < c1; i++) w[v.cnt_kf[(size_t)i]] = v.cnt_w[(size_t)i];
            c.mvpOrderedConnectedKeyFrames[(size_t)kf].assign(v.ord_kf.begin() + o0, v.ord_kf.begin() + o1);
            c.mvOrderedWeights[(size_t)kf].assign(v.ord_w.begin() + o0, v.ord_w.begin() + o1);
            if (c.mbFirstConnection[(size_t)kf] && c.mnId[(size_t)kf] != 0) {
                c.mpParent[(size_t)kf] = v.ord_kf[(size_t)o0];
                c.mspChildrens[(size_t)v.ord_kf[(size_t)o0]].push_back(kf);
                c.mbFirstConnection[(size_t)kf] = 0;
            }
        }
        return v;
    }

    // vpLocalKeyFrames with their slot lists; slot_octave / slot_depth per slot, mThDepth and kf_flags (bit 0 mnId == 0, bit 1 mbNotErase) per key frame
    KeyFrameCullingResult KeyFrameCulling(const ObsTable &table, const std::vector<int> &vpLocalKeyFrames, const SlotLists &lists, const std::vector<int> &slot_octave,
                                          const std::vector<float> &slot_depth, const std::vector<float> &mThDepth, bool mbMonocular, const std::vector<uint8_t> &kf_flags,
                                          int thObs = 3) const {
        const cs_obs_table t = table.c_struct();
        const size_t n = vpLocalKeyFrames.size();
        if (lists.off.size() != n + 1 || slot_octave.size() != lists.mp.size() || slot_depth.size() != lists.mp.size() || mThDepth.size() != n || kf_flags.size() != n)
            throw std::invalid_argument("KeyFrameCulling: per-slot and per-key-frame arrays disagree with the lists");
        KeyFrameCullingResult r;
        r.verdict.assign(n + 1, 0); r.n_mps.assign(n + 1, 0); r.n_redundant.assign(n + 1, 0);
        r.mp_nobs.assign(table.mp_nobs.size() + 1, 0); r.mp_flags.assign(table.mp_nobs.size() + 1, 0); r.alive.assign(table.obs_kf.size() + 1, 0);
        const int s = ctx_ ? cs_keyframe_culling(ctx_->ctx, &t, (int)n, vpLocalKeyFrames.data(), lists.off.data(), lists.mp.data(), slot_octave.data(), slot_depth.data(), mThDepth.data(),
                                                 mbMonocular, kf_flags.data(), thObs, r.verdict.data(), r.n_mps.data(), r.n_redundant.data(), r.mp_nobs.data(), r.mp_flags.data(),
                                                 r.alive.data(), &r.n_rounds)
                           : cs_keyframe_culling_host(&t, (int)n, vpLocalKeyFrames.data(), lists.off.data(), lists.mp.data(), slot_octave.data(), slot_depth.data(), mThDepth.data(),
                                                      mbMonocular, kf_flags.data(), thObs, r.verdict.data(), r.n_mps.data(), r.n_redundant.data(), r.mp_nobs.data(),
                                                      r.mp_flags.data(), r.alive.data(), &r.n_rounds);
        if (s != CS_OK) fail("cs_keyframe_culling", s);
        r.verdict.resize(n); r.n_mps.resize(n); r.n_redundant.resize(n);
        r.mp_nobs.resize(table.mp_nobs.size()); r.mp_flags.resize(table.mp_nobs.size()); r.alive.resize(table.obs_kf.size());
        return r;
    }

    // mlpRecentAddedMapPoints as indices; mnFound / mnVisible / mnFirstKFid per point.  Cases 2 and 3 are the reference's SetBadFlag calls; every case but 0 leaves the list.
    std::vector<uint8_t> MapPointCulling(const ObsTable &table, const std::vector<int> &mlpRecentAddedMapPoints, const std::vector<int> &mnFound, const std::vector<int> &mnVisible,
                                         const std::vector<int> &mnFirstKFid, int nCurrentKFid, int cnThObs) const {
        const cs_obs_table t = table.c_struct();
        if (mnFound.size() != table.mp_nobs.size() || mnVisible.size() != mnFound.size() || mnFirstKFid.size() != mnFound.size())
            throw std::invalid_argument("MapPointCulling: one entry per point");
        const size_t n = mlpRecentAddedMapPoints.size();
        std::vector<uint8_t> cases(n + 1, 0);
        const int s = ctx_ ? cs_mappoint_culling(ctx_->ctx, &t, (int)n, mlpRecentAddedMapPoints.data(), mnFound.data(), mnVisible.data(), mnFirstKFid.data(), nCurrentKFid, cnThObs,
                                                 cases.data())
                           : cs_mappoint_culling_host(&t, (int)n, mlpRecentAddedMapPoints.data(), mnFound.data(), mnVisible.data(), mnFirstKFid.data(), nCurrentKFid, cnThObs,
                                                      cases.data());
        if (s != CS_OK) fail("cs_mappoint_culling", s);
        cases.resize(n);
        return cases;
    }

  private:
    Context *ctx_;
    void fail(const char *what, int r) const {
        throw std::runtime_error(std::string(what) + " failed (" + std::to_string(r) + ")" + (ctx_ ? std::string(": ") + cs_last_error(ctx_->ctx) : std::string()));
    }
};

} // namespace cubeslam
