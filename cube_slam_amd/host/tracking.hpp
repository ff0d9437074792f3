// tracking.hpp -- ORB_SLAM2::Tracking::TrackLocalMap (orb_object_slam/src/Tracking.cc:1356-1416) and what it calls, with the reference's member names over the C-ABI
// (include/cubeslam_hip.h) and plain arrays:
//   cubeslam::Tracking::UpdateLocalKeyFrames  :2766-2874, the host walk of csrc/track_local_walk.h (what cs_track_local_keyframes runs)
//   UpdateLocalPoints                         :2740-2764, cs_track_local_points
//   SearchLocalPoints                         :2673-2728, Frame::isInFrustum and ORBmatcher::SearchByProjection(F, vpMapPoints, th) in cs_match_local_map_frustum
//   TrackLocalMap                             the chain with cs_pose_optimization and the statistics loop (:1372-1397), which stays on the host with the two thresholds
//   CreateNewHarrisFeatures                   :2258-2337, the new dynamic-object points of CreateNewKeyFrame: csrc/gftt_math.h on the host, cs_track_new_harris_features
// The map is a table of points and a table of key frames (TrackMap); what the reference keeps as pointers are indices into them, -1 for NULL.  With CUBESLAM_HOST_ONLY defined
// the header needs neither the library nor a context type; only UpdateLocalKeyFrames and CreateNewHarrisFeatures on its path without a context are there.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/gftt_math.h"
#include "../csrc/track_local_walk.h"
#ifndef CUBESLAM_HOST_ONLY
#include "../../include/cubeslam_hip.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context
#else
namespace cubeslam { struct Context; }
#endif

namespace cubeslam {

struct TrackMap {
    // map points: GetWorldPos / GetNormal (3 per point), mfMinDistance / mfMaxDistance, GetDescriptor (32 per point), isBad, is_dynamic, Observations(), the key frames of GetObservations()
    std::vector<float> world_pos, normal, min_distance, max_distance;
    std::vector<uint8_t> desc, bad, dynamic;
    std::vector<int> n_obs, obs_off, obs_kf;
    std::vector<long> last_frame_seen, visible, found; // mnLastFrameSeen, mnVisible, mnFound
    // key frames: GetMapPointMatches(), isBad, mvpOrderedConnectedKeyFrames, GetChilds(), GetParent()
    std::vector<int> kf_off, kf_mp, cov_off, cov_kf, child_off, child_kf, parent;
    std::vector<uint8_t> kf_bad;
    int n_points() const { return (int)bad.size(); }
    int n_kf() const { return (int)kf_bad.size(); }
};

#ifndef CUBESLAM_HOST_ONLY
struct TrackFrame { // mCurrentFrame as TrackLocalMap reads and writes it
    long mnId = 0;
    std::vector<cs_keypoint> mvKeysUn;
    std::vector<uint8_t> mDescriptors, mvbOutlier, KeysStatic /* empty: every key point is static */;
    std::vector<int> mvpMapPoints;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2, mvuRight /* empty: monocular */;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0, mRcw[9] = {0}, mtcw[3] = {0}, mOw[3] = {0}, fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mfLogScaleFactor = 0;
    double pose[7] = {0}; // mTcw as [t, qx qy qz qw], what PoseOptimization refines
    int N() const { return (int)mvKeysUn.size(); }
};
#endif

class Tracking {
  public:
    enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2 };
    std::vector<int> mvpLocalKeyFrames, mvpLocalMapPoints;
    int mpReferenceKF = -1, mnMatchesInliers = 0, mSensor = MONOCULAR, mMaxFrames = 30;
    long mnLastRelocFrameId = -1000000000;
    bool whether_dynamic_object = false, whether_detect_object = false, mbOnlyTracking = false;

    // (mvpMapPoints: mCurrentFrame.mvpMapPoints; a bad point's slot is cleared, :2785)
    void UpdateLocalKeyFrames(std::vector<int> &mvpMapPoints, const TrackMap &m) {
        for (int &p : mvpMapPoints) if (p >= 0 && m.bad[(size_t)p]) p = -1;
        const std::vector<uint8_t> skip = skip_of(m);
        std::vector<int> local((size_t)m.n_kf() + 1);
        int kf_max = -1;
        const int n = track_local_keyframes((int)mvpMapPoints.size(), mvpMapPoints.data(), m.n_points(), skip.data(), m.obs_off.data(), m.obs_kf.data(), m.n_kf(), m.kf_bad.data(),
                                            m.cov_off.data(), m.cov_kf.data(), m.child_off.data(), m.child_kf.data(), m.parent.data(), local.data(), &kf_max);
        if (n == -2) throw std::invalid_argument("Tracking::UpdateLocalKeyFrames: an index outside its table");
        if (n < 0) return; // :2790
        local.resize((size_t)n);
        mvpLocalKeyFrames = local;
        if (kf_max >= 0) mpReferenceKF = kf_max;
    }

    // The new-feature loop of CreateNewKeyFrame with use_dynamic_klt_features (:2258-2337) over raw_img (width x height, rows `stride` bytes apart) and objmask_img
    // (dense).  exist_pts / exist_obs: pt and Observations() of the current frame's Harris points with `pMP && pMP->is_dynamic`; K4 = fx, fy, cx, cy; Twc = the 3 x 4 rows
    // of the key frame's pose; cuboid_depth[id] = local_cuboids[id]->cube_meas.translation()[2].  `new MapPoint`, SetupSimpleMapPoints and the copies of :2300-2305 and
    // :2335-2337 stay the caller's.  Without a context the host runs csrc/gftt_math.h, byte-equal to the device.
    struct NewHarrisFeatures {
        std::vector<float> pts, x3D;        // the new corners (x, y) and their world positions
        std::vector<int> object_id;         // keypoint_associate_objectID_harris of the new points
        std::vector<uint8_t> x3D_valid;     // 0: the cuboid's depth is not > 0 (the reference's empty Mat)
        std::vector<uint8_t> good_mask;     // the mask goodFeaturesToTrack ran on
        int n_mask_outside = 0, n_candidates = 0;
    };
    static NewHarrisFeatures CreateNewHarrisFeatures(Context *ctx, const uint8_t *raw_img, int width, int height, long stride, const uint8_t *objmask_img,
                                                     const std::vector<float> &exist_pts, const std::vector<int> &exist_obs, const float K4[4], const float Twc[12],
                                                     const std::vector<float> &cuboid_depth) {
        const int n_exist = (int)exist_obs.size(), n_cub = (int)cuboid_depth.size();
        if (!raw_img || !objmask_img || width < 1 || height < 1 || stride < width || exist_pts.size() != 2 * exist_obs.size())
            throw std::invalid_argument("CreateNewHarrisFeatures: an image, a mask and (x, y) pairs with one observation count each");
        for (float v : exist_pts) if (!gftt_point_ok(v)) throw std::invalid_argument("CreateNewHarrisFeatures: an existing point that is not finite");
        NewHarrisFeatures r;
        r.pts.assign(400, 0.f); r.x3D.assign(600, 0.f); r.object_id.assign(200, 0); r.x3D_valid.assign(200, 0); r.good_mask.assign((size_t)width * height, 0);
        const float none = 0;
        const int zero = 0;
        int n_new = 0;
        if (!ctx) {
            const int rc = gftt_new_harris_features_host(raw_img, stride, width, height, objmask_img, n_exist, n_exist ? exist_pts.data() : &none, n_exist ? exist_obs.data() : &zero, K4, Twc,
                                                         n_cub, n_cub ? cuboid_depth.data() : &none, r.good_mask.data(), r.pts.data(), r.object_id.data(), r.x3D.data(),
                                                         r.x3D_valid.data(), &n_new, &r.n_candidates, &r.n_mask_outside);
            if (rc == 1) throw std::length_error("CreateNewHarrisFeatures: more candidates than GFTT_MAX_CANDIDATES");
            if (rc == 2) throw std::invalid_argument("CreateNewHarrisFeatures: a corner's object id is at or beyond the cuboid count");
        } else {
#ifndef CUBESLAM_HOST_ONLY
            std::vector<uint8_t> dense((size_t)width * height);
            for (int y = 0; y < height; y++) std::copy(raw_img + (long)y * stride, raw_img + (long)y * stride + width, dense.begin() + (size_t)y * width);
            cs_klt *h = nullptr;
            int rc = cs_klt_create(ctx->ctx, 1, width, height, 1, &h);
            if (rc == CS_OK) rc = cs_klt_set_frames(ctx->ctx, h, 1, width, height, dense.data(), width);
            const int frame = 0, ef[2] = {0, n_exist}, cf[2] = {0, n_cub};
            int nf[2] = {0, 0};
            if (rc == CS_OK)
                rc = cs_track_new_harris_features(ctx->ctx, h, 1, &frame, objmask_img, ef, n_exist ? exist_pts.data() : &none, n_exist ? exist_obs.data() : &zero, K4, Twc, cf,
                                                  n_cub ? cuboid_depth.data() : &none, nf, r.pts.data(), r.object_id.data(), r.x3D.data(), r.x3D_valid.data(), &r.n_mask_outside,
                                                  r.good_mask.data(), &r.n_candidates);
            cs_klt_destroy(ctx->ctx, h);
            if (rc != CS_OK) throw std::runtime_error(std::string("cs_track_new_harris_features failed (") + std::to_string(rc) + "): " + cs_last_error(ctx->ctx));
            n_new = nf[1];
#else
            throw std::runtime_error("CreateNewHarrisFeatures: built without the library");
#endif
        }
        r.pts.resize(2 * (size_t)n_new); r.x3D.resize(3 * (size_t)n_new); r.object_id.resize((size_t)n_new); r.x3D_valid.resize((size_t)n_new);
        return r;
    }

#ifndef CUBESLAM_HOST_ONLY
    explicit Tracking(Context &c, int max_keypoints = 8192, int max_queries = 16384, long max_candidates = 4000000) : ctx_(&c) {
        chk(cs_matcher_create(c.ctx, max_keypoints, max_queries, max_candidates, &m_), "cs_matcher_create");
    }
    ~Tracking() { if (m_) cs_matcher_destroy(ctx_->ctx, m_); }
    Tracking(const Tracking &) = delete;
    Tracking &operator=(const Tracking &) = delete;

    void UpdateLocalPoints(const TrackMap &m) {
        std::vector<int> off{0}, mp;
        for (int kf : mvpLocalKeyFrames) { mp.insert(mp.end(), m.kf_mp.begin() + m.kf_off[(size_t)kf], m.kf_mp.begin() + m.kf_off[(size_t)kf + 1]); off.push_back((int)mp.size()); }
        const std::vector<uint8_t> skip = skip_of(m);
        mvpLocalMapPoints.assign(mp.size() + 1, 0);
        int n = 0;
        chk(cs_track_local_points(ctx_->ctx, (int)off.size() - 1, off.data(), mp.data(), m.n_points(), skip.data(), mvpLocalMapPoints.data(), &n), "cs_track_local_points");
        mvpLocalMapPoints.resize((size_t)n);
    }
    void UpdateLocalMap(TrackFrame &F, const TrackMap &m) { UpdateLocalKeyFrames(F.mvpMapPoints, m); UpdateLocalPoints(m); }

    // what the last SearchLocalPoints left: per local point mbTrackInView, (mTrackProjX, mTrackProjY, mTrackProjXR), mnTrackScaleLevel, mTrackViewCos; per key point the local point it received
    std::vector<uint8_t> in_view; std::vector<float> proj, view_cos; std::vector<int> pred_level, train_match;
    int nmatches = 0, nToMatch = 0, n_level_outside = 0;

    void SearchLocalPoints(TrackFrame &F, TrackMap &m) {
        const int N = F.N();
        for (int &p : F.mvpMapPoints) { // :2676-2694
            if (p < 0) continue;
            if (m.bad[(size_t)p]) { p = -1; continue; }
            if (m.dynamic[(size_t)p]) continue;
            m.visible[(size_t)p]++; m.last_frame_seen[(size_t)p] = F.mnId;
        }
        const std::vector<int> &lp = mvpLocalMapPoints;
        const size_t n = lp.size();
        std::vector<float> wp(n * 3), nr(n * 3), mn(n), mx(n);
        std::vector<uint8_t> skip(n), blocks(n), desc(n * 32), tb((size_t)N, 0);
        for (size_t i = 0; i < n; i++) {
            const size_t p = (size_t)lp[i];
            for (int k = 0; k < 3; k++) { wp[i * 3 + k] = m.world_pos[p * 3 + k]; nr[i * 3 + k] = m.normal[p * 3 + k]; }
            mn[i] = m.min_distance[p]; mx[i] = m.max_distance[p];
            for (int k = 0; k < 32; k++) desc[i * 32 + k] = m.desc[p * 32 + k];
            skip[i] = m.last_frame_seen[p] == F.mnId || m.bad[p] || m.dynamic[p]; // :2702-2707
            blocks[i] = m.n_obs[p] > 0;
        }
        for (int i = 0; i < N; i++) { // ORBmatcher.cc:96-102
            if (F.mvpMapPoints[(size_t)i] >= 0 && m.n_obs[(size_t)F.mvpMapPoints[(size_t)i]] > 0) tb[(size_t)i] = 1;
            if (!F.KeysStatic.empty() && !F.KeysStatic[(size_t)i]) tb[(size_t)i] = 1;
        }
        int th = 1; // :2720-2725
        if (mSensor == RGBD) th = 3;
        if (F.mnId < mnLastRelocFrameId + 2) th = 5;
        chk(cs_matcher_set_frame(ctx_->ctx, m_, F.mvKeysUn.data(), F.mDescriptors.data(), N, F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY), "cs_matcher_set_frame");
        in_view.assign(n + 1, 0); proj.assign(n * 3 + 1, 0.0f); view_cos.assign(n + 1, 0.0f); pred_level.assign(n + 1, -1); train_match.assign((size_t)N + 1, -1);
        chk(cs_match_local_map_frustum(ctx_->ctx, m_, F.mRcw, F.mtcw, F.mOw, (int)n, wp.data(), nr.data(), mn.data(), mx.data(), skip.data(), blocks.data(), desc.data(), tb.data(), F.fx, F.fy,
                                       F.cx, F.cy, F.mbf, F.mfLogScaleFactor, F.mvScaleFactors.data(), (int)F.mvScaleFactors.size(), 0.5f, (float)th, 0.8f, train_match.data(), &nmatches,
                                       &nToMatch, &n_level_outside, in_view.data(), proj.data(), pred_level.data(), view_cos.data()),
            "cs_match_local_map_frustum");
        in_view.resize(n); proj.resize(n * 3); view_cos.resize(n); pred_level.resize(n); train_match.resize((size_t)N);
        for (size_t i = 0; i < n; i++) if (in_view[i]) m.visible[(size_t)lp[i]]++; // :2712
        for (int i = 0; i < N; i++) if (train_match[(size_t)i] >= 0) F.mvpMapPoints[(size_t)i] = lp[(size_t)train_match[(size_t)i]]; // ORBmatcher.cc:136
    }

    bool TrackLocalMap(TrackFrame &F, TrackMap &m) {
        UpdateLocalMap(F, m);
        SearchLocalPoints(F, m);
        std::vector<int> idx;
        std::vector<double> Xw, obs, w;
        for (int i = 0; i < F.N(); i++) {
            const int p = F.mvpMapPoints[(size_t)i];
            if (p < 0) continue;
            idx.push_back(i);
            for (int k = 0; k < 3; k++) Xw.push_back((double)m.world_pos[(size_t)p * 3 + k]);
            obs.push_back((double)F.mvKeysUn[(size_t)i].x); obs.push_back((double)F.mvKeysUn[(size_t)i].y); obs.push_back(F.mvuRight.empty() ? -1.0 : (double)F.mvuRight[(size_t)i]);
            w.push_back((double)F.mvInvLevelSigma2[(size_t)F.mvKeysUn[(size_t)i].octave]);
        }
        const int ne = (int)idx.size(), off[2] = {0, ne};
        const double intr[5] = {F.fx, F.fy, F.cx, F.cy, F.mbf};
        std::vector<uint8_t> flags((size_t)ne + 1, 0);
        double pose_out[7];
        int n_inl = 0;
        Xw.resize(Xw.size() + 3); obs.resize(obs.size() + 3); w.resize(w.size() + 1); // (never empty)
        chk(cs_pose_optimization(ctx_->ctx, 1, off, Xw.data(), obs.data(), w.data(), intr, F.pose, pose_out, flags.data(), &n_inl), "cs_pose_optimization"); // :1366
        for (int k = 0; k < 7; k++) F.pose[k] = pose_out[k];
        F.mvbOutlier.assign((size_t)F.N(), 0);
        mnMatchesInliers = 0;
        for (int e = 0; e < ne; e++) { // :1372-1397
            const int i = idx[(size_t)e], p = F.mvpMapPoints[(size_t)i];
            F.mvbOutlier[(size_t)i] = flags[(size_t)e];
            if (!flags[(size_t)e]) {
                if (whether_dynamic_object && m.dynamic[(size_t)p]) continue;
                m.found[(size_t)p]++;
                if (!mbOnlyTracking) { if (m.n_obs[(size_t)p] > 0) mnMatchesInliers++; }
                else mnMatchesInliers++;
            } else if (mSensor == STEREO) F.mvpMapPoints[(size_t)i] = -1;
        }
        if (F.mnId < mnLastRelocFrameId + mMaxFrames && mnMatchesInliers < 50) return false; // :1402
        return mnMatchesInliers >= (whether_detect_object ? 20 : 30);                          // :1405-1415
    }

  private:
    void chk(int r, const char *what) const { if (r != CS_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(r) + "): " + cs_last_error(ctx_->ctx)); }
    Context *ctx_ = nullptr;
    cs_matcher *m_ = nullptr;
#else
    Tracking() = default;
#endif

  private:
    std::vector<uint8_t> skip_of(const TrackMap &m) const { // isBad, or is_dynamic under whether_dynamic_object (:2755-2758, :2775-2778)
        std::vector<uint8_t> s((size_t)m.n_points() + 1, 0);
        for (int i = 0; i < m.n_points(); i++) s[(size_t)i] = m.bad[(size_t)i] || (whether_dynamic_object && m.dynamic[(size_t)i]);
        return s;
    }
};

} // namespace cubeslam
