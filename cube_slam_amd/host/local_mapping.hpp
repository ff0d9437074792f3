// local_mapping.hpp -- the middle of ORB_SLAM2::LocalMapping's key-frame cycle with the reference's names, over the C-ABI (include/cubeslam_hip.h) and plain arrays:
//   cubeslam::LocalMapping::CreateNewMapPoints       the neighbour loop of LocalMapping::CreateNewMapPoints (orb_object_slam/src/LocalMapping.cc:319-570): the baseline tests
//                                                    :356-372, one SearchForTriangulation per surviving neighbour with the initial skip, one cs_create_new_map_points
//   cubeslam::LocalMapping::ComputeDistinctiveDescriptors / UpdateNormalAndDepth   MapPoint.cc:381-446 / :469-510 for many points per call
// The caller keeps GetBestCovisibilityKeyFrames, ComputeF12, new MapPoint / AddObservation / AddMapPoint and the object-depth tail :571-652.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context

namespace cubeslam {

// What CreateNewMapPoints reads of a KeyFrame; desc / node / skip only for the search (node: cs_bow_transform's, skip[i]: the key point has a map point or is not static)
struct KeyFrameView {
    std::vector<cs_keypoint> keysUn;                    // mvKeysUn
    std::vector<float> keys_xy, u_right, depth;         // mvKeys[i].pt, mvuRight, mvDepth
    float Rcw[9] = {0}, tcw[3] = {0}, Ow[3] = {0};      // as stored
    float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mbf = 0, mb = 0;
    std::vector<float> scale_factors, level_sigma2;     // mvScaleFactors, mvLevelSigma2
    float scale_factor = 0;                             // mfScaleFactor
    std::vector<uint8_t> desc, skip;
    std::vector<int> node;
    int N() const { return (int)keysUn.size(); }
    cs_lm_frame c_struct() const {
        cs_lm_frame f;
        f.keysUn = keysUn.data(); f.keys_xy = keys_xy.data(); f.u_right = u_right.data(); f.depth = depth.data(); f.N = N();
        for (int k = 0; k < 9; k++) f.Rcw[k] = Rcw[k];
        for (int k = 0; k < 3; k++) { f.tcw[k] = tcw[k]; f.Ow[k] = Ow[k]; }
        f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy; f.invfx = invfx; f.invfy = invfy; f.mbf = mbf; f.mb = mb;
        f.scale_factors = scale_factors.data(); f.level_sigma2 = level_sigma2.data(); f.n_levels = (int)scale_factors.size(); f.scale_factor = scale_factor;
        return f;
    }
};

struct NewMapPoints {
    std::vector<int> kept;                                   // the neighbours that passed the baseline test, as indices into the caller's list
    std::vector<int> pair_off, idx1, idx2, pair_neighbour;   // every pair, in neighbour order and then idx1 ascending (vMatchedPairs)
    std::vector<float> x3D;
    std::vector<uint8_t> status;                             // cs_create_new_map_points' status byte
    std::vector<int> new_pair_of_idx1;
    int nnew = 0;
    std::vector<int> new_neighbour, new_idx1, new_idx2;      // the created points in the reference's creation order
    std::vector<float> new_x3D;
    // what a reference that returns at `i > 0 && CheckNewKeyFrames()` (:351) before neighbour i has created: a neighbour's pairs depend on earlier neighbours only
    int points_before(int i) const { int n = 0; while (n < (int)new_neighbour.size() && new_neighbour[n] < i) n++; return n; }
};

class LocalMapping {
  public:
    // matches12[N1] of ORBmatcher(0.6, false).SearchForTriangulation(kf, nb, F12, vMatchedIndices, false)
    typedef std::function<std::vector<int>(const KeyFrameView &kf, const KeyFrameView &nb, int neighbour, const float *F12, float ex, float ey)> Search;
    bool mbMonocular;
    explicit LocalMapping(Context &c, bool monocular = false) : mbMonocular(monocular), ctx_(c) {}

    bool BaselineOk(const KeyFrameView &kf, const KeyFrameView &nb, float medianDepthKF2 = 0.f) const { // :356-372
        double s = 0;
        for (int k = 0; k < 3; k++) { const float d = nb.Ow[k] - kf.Ow[k]; s += (double)d * (double)d; }
        const float baseline = (float)std::sqrt(s);
        if (!mbMonocular) return !(baseline < nb.mb);
        const float ratioBaselineDepth = baseline / medianDepthKF2;
        return !(ratioBaselineDepth < 0.01);
    }

    // neighbours = GetBestCovisibilityKeyFrames(nn) in order; F12s: 9 floats per neighbour (ComputeF12); epipoles: ex, ey per neighbour (ORBmatcher.cc:686-692); median_depths
    // (monocular only): ComputeSceneMedianDepth(2) per neighbour.  `search` replaces cs_match_for_triangulation.
    NewMapPoints CreateNewMapPoints(const KeyFrameView &kf, const std::vector<KeyFrameView> &neighbours, const std::vector<float> &F12s, const std::vector<float> &epipoles,
                                    const std::vector<float> &median_depths = {}, Search search = Search()) {
        if (neighbours.size() > CS_LM_MAX_NEIGHBOURS) throw std::runtime_error("CreateNewMapPoints: more than 32 neighbours");
        NewMapPoints r;
        const int N1 = kf.N();
        if (mbMonocular && median_depths.size() != neighbours.size()) throw std::invalid_argument("CreateNewMapPoints: monocular needs median_depths, one ComputeSceneMedianDepth(2) per neighbour");
        for (size_t i = 0; i < neighbours.size(); i++) if (BaselineOk(kf, neighbours[i], mbMonocular ? median_depths.at(i) : 0.f)) r.kept.push_back((int)i);
        const int n = (int)r.kept.size();
        std::vector<int> m((size_t)n * N1, -1);
        std::vector<cs_lm_frame> frames;
        long cap = 0;
        for (int k = 0; k < n; k++) {
            const int i = r.kept[k];
            const KeyFrameView &nb = neighbours[i];
            const float *F = F12s.empty() ? nullptr : &F12s[9 * (size_t)i];
            const float ex = epipoles.empty() ? 0.f : epipoles[2 * (size_t)i], ey = epipoles.empty() ? 0.f : epipoles[2 * (size_t)i + 1];
            std::vector<int> mi = search ? search(kf, nb, i, F, ex, ey) : device_search(kf, nb, F, ex, ey);
            if ((int)mi.size() != N1) throw std::runtime_error("CreateNewMapPoints: a search returned a vector of another length than N1");
            for (int j = 0; j < N1; j++) { m[(size_t)k * N1 + j] = mi[j]; cap += mi[j] != -1; }
            frames.push_back(nb.c_struct());
        }
        const cs_lm_frame cur = kf.c_struct();
        r.pair_off.assign((size_t)n + 1, 0); r.idx1.assign((size_t)cap, 0); r.idx2.assign((size_t)cap, 0); r.x3D.assign(3 * (size_t)cap, 0.f); r.status.assign((size_t)cap, 0);
        r.new_pair_of_idx1.assign((size_t)N1, -1);
        check(cs_create_new_map_points(ctx_.ctx, &cur, frames.data(), n, m.data(), (int)cap, r.pair_off.data(), r.idx1.data(), r.idx2.data(), r.x3D.data(), r.status.data(),
                                       r.new_pair_of_idx1.data(), &r.nnew), "cs_create_new_map_points");
        for (int k = 0; k < n; k++) for (int p = r.pair_off[k]; p < r.pair_off[k + 1]; p++) r.pair_neighbour.push_back(r.kept[k]);
        for (long p = 0; p < cap; p++) // pair order = creation order
            if (r.status[p] == 0) {
                r.new_neighbour.push_back(r.pair_neighbour[p]); r.new_idx1.push_back(r.idx1[p]); r.new_idx2.push_back(r.idx2[p]);
                for (int c = 0; c < 3; c++) r.new_x3D.push_back(r.x3D[3 * p + c]);
            }
        return r;
    }

    // best[p]: index within the run of the descriptor that becomes mDescriptor, -1 for an empty run
    std::vector<int> ComputeDistinctiveDescriptors(const std::vector<int> &obs_off, const std::vector<uint8_t> &desc) {
        const int n = (int)obs_off.size() - 1;
        std::vector<int> best((size_t)std::max(n, 0));
        check(cs_mappoint_distinctive_descriptors(ctx_.ctx, std::max(n, 0), obs_off.data(), desc.data(), best.data()), "cs_mappoint_distinctive_descriptors");
        return best;
    }

    // normal / min_distance / max_distance hold the current values on entry (kept for points without observations) and the new ones on return; updated[p] = 1 where written
    std::vector<uint8_t> UpdateNormalAndDepth(const std::vector<float> &world_pos, const std::vector<int> &obs_off, const std::vector<int> &obs_kf, const std::vector<float> &kf_Ow,
                                              const std::vector<int> &ref_kf, const std::vector<int> &ref_octave, const std::vector<float> &scale_factors, std::vector<float> &normal,
                                              std::vector<float> &min_distance, std::vector<float> &max_distance) {
        const int n = (int)(world_pos.size() / 3);
        if ((int)obs_off.size() != n + 1 || (int)ref_kf.size() != n || (int)ref_octave.size() != n) throw std::runtime_error("UpdateNormalAndDepth: one entry per point");
        normal.resize(3 * (size_t)n); min_distance.resize((size_t)n); max_distance.resize((size_t)n);
        std::vector<uint8_t> updated((size_t)n);
        check(cs_mappoint_update_normal_and_depth(ctx_.ctx, n, world_pos.data(), obs_off.data(), obs_kf.data(), (int)(kf_Ow.size() / 3), kf_Ow.data(), ref_kf.data(),
                                                  ref_octave.data(), scale_factors.data(), (int)scale_factors.size(), normal.data(), min_distance.data(), max_distance.data(),
                                                  updated.data()), "cs_mappoint_update_normal_and_depth");
        return updated;
    }

  private:
    Context &ctx_;
    void check(int r, const char *what) const {
        if (r != CS_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(r) + "): " + cs_last_error(ctx_.ctx));
    }
    std::vector<int> device_search(const KeyFrameView &kf, const KeyFrameView &nb, const float *F12, float ex, float ey) {
        std::vector<int> m((size_t)kf.N(), -1);
        int nmatches = 0;
        check(cs_match_for_triangulation(ctx_.ctx, kf.keysUn.data(), kf.desc.data(), kf.N(), kf.node.data(), kf.skip.data(), kf.u_right.data(), nb.keysUn.data(), nb.desc.data(),
                                         nb.N(), nb.node.data(), nb.skip.data(), nb.u_right.data(), F12, ex, ey, nb.scale_factors.data(), nb.level_sigma2.data(),
                                         (int)nb.scale_factors.size(), 0, 0, m.data(), &nmatches), "cs_match_for_triangulation");
        return m;
    }
};

} // namespace cubeslam
