// tracking.hpp -- ORB_SLAM2::Tracking::TrackWithMotionModel (orb_object_slam/src/Tracking.cc:1276-1354) and TrackLocalMap (:1356-1416) and what they call, with the reference's
// member names over the C-ABI (include/cubeslam_hip.h, include/cubeslam_hip/stereo_search.h) and plain arrays:
//   cubeslam::Tracking::TrackWithMotionModel  UpdateLastFrame (:1215-1273, cubeslam::ClosePoints), ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) with its stereo
//                                             branch and the retry at 2 th, cs_pose_optimization, the outlier loop and both return rules; the predicted pose is an input
//   cubeslam::Tracking::UpdateLocalKeyFrames  :2766-2874, the host walk of csrc/track_local_walk.h (what cs_track_local_keyframes runs)
//   UpdateLocalPoints                         :2740-2764, cs_track_local_points
//   SearchLocalPoints                         :2673-2728, Frame::isInFrustum and ORBmatcher::SearchByProjection(F, vpMapPoints, th) in cs_match_local_map_frustum -- for a frame with
//                                             mvuRight and a sensor that is not monocular in cs_match_local_map_frustum_stereo (the mvuRight test of ORBmatcher.cc:104-109)
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
#include <cmath>

#include "../../include/cubeslam_hip.h"
#include "../../include/cubeslam_hip/stereo_search.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context
#include "orb_slam_mirrors.hpp" // cubeslam::ClosePoints, cubeslam::ORBmatcher
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
    // `new MapPoint(x3D, mpMap, &mLastFrame, i)` (Tracking.cc:1259): a point without observations behind the table's last; its descriptor is the creating key point's
    int append_point(const float x3D[3], const uint8_t d[32]) {
        const int id = n_points();
        world_pos.insert(world_pos.end(), x3D, x3D + 3); normal.insert(normal.end(), 3, 0.0f); min_distance.push_back(0.0f); max_distance.push_back(0.0f);
        desc.insert(desc.end(), d, d + 32); bad.push_back(0); dynamic.push_back(0); n_obs.push_back(0); obs_off.push_back(obs_off.back());
        last_frame_seen.push_back(-1); visible.push_back(0); found.push_back(0);
        return id;
    }
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
    // Frame::SetPose / UpdatePoseMatrices (Frame.cc:320-344) for a 3 x 4 float pose: mOw = -mRcw.t() * mtcw, one gemm per row (double accumulation, one rounding)
    void SetPose(const float Tcw[12]) {
        for (int r = 0; r < 3; r++) { for (int k = 0; k < 3; k++) mRcw[r * 3 + k] = Tcw[r * 4 + k]; mtcw[r] = Tcw[r * 4 + 3]; }
        for (int r = 0; r < 3; r++) {
            double acc = 0;
            for (int k = 0; k < 3; k++) acc += (double)Tcw[k * 4 + r] * (double)Tcw[k * 4 + 3];
            mOw[r] = (float)(-acc);
        }
    }
    void Tcw(float out[12]) const { for (int r = 0; r < 3; r++) { for (int k = 0; k < 3; k++) out[r * 4 + k] = mRcw[r * 3 + k]; out[r * 4 + 3] = mtcw[r]; } }
};
struct TrackLastFrame { // mLastFrame as TrackWithMotionModel reads it; is_keyframe: it is the reference key frame's own frame (UpdateLastFrame creates nothing, :1215)
    std::vector<cs_keypoint> mvKeysUn;
    std::vector<uint8_t> mDescriptors, mvbOutlier;
    std::vector<int> mvpMapPoints;
    std::vector<float> mvDepth;
    float mTcw[12] = {0};
    bool is_keyframe = false;
};
// (t, qx, qy, qz, qw) of a 3 x 4 pose and back: cube_slam_amd.tracking.Tcw_to_pose7 / pose7_to_Tcw, step by step (compile with -ffp-contract=off)
inline void Tcw_to_pose7(const float T[12], double p[7]) {
    double R[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = (double)T[i * 4 + j];
    const double tr = R[0][0] + R[1][1] + R[2][2];
    double q[4] = {0, 0, 0, 0};
    if (tr > 0) {
        const double s = std::sqrt(tr + 1.0) * 2;
        q[0] = (R[2][1] - R[1][2]) / s; q[1] = (R[0][2] - R[2][0]) / s; q[2] = (R[1][0] - R[0][1]) / s; q[3] = 0.25 * s;
    } else {
        int i = 0;
        if (R[1][1] > R[i][i]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        const double s = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0) * 2;
        q[i] = 0.25 * s; q[3] = (R[k][j] - R[j][k]) / s; q[j] = (R[j][i] + R[i][j]) / s; q[k] = (R[k][i] + R[i][k]) / s;
    }
    if (q[3] < 0) for (double &v : q) v = -v;
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int r = 0; r < 3; r++) p[r] = (double)T[r * 4 + 3];
    for (int c = 0; c < 4; c++) p[3 + c] = q[c] / n;
}
inline void pose7_to_Tcw(const double p[7], float T[12]) {
    const double x = p[3], y = p[4], z = p[5], w = p[6];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int r = 0; r < 3; r++) { for (int k = 0; k < 3; k++) T[r * 4 + k] = (float)R[r * 3 + k]; T[r * 4 + 3] = (float)p[r]; }
}
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
        const bool stereo = mSensor != MONOCULAR && !F.mvuRight.empty(); // ORBmatcher.cc:104-109: a frame with right coordinates tests them
        if (stereo) ORBmatcher::set_u_right(ctx_, m_, F.mvuRight);
        chk((stereo ? cs_match_local_map_frustum_stereo : cs_match_local_map_frustum)(ctx_->ctx, m_, F.mRcw, F.mtcw, F.mOw, (int)n, wp.data(), nr.data(), mn.data(), mx.data(), skip.data(), blocks.data(), desc.data(), tb.data(), F.fx, F.fy,
                                       F.cx, F.cy, F.mbf, F.mfLogScaleFactor, F.mvScaleFactors.data(), (int)F.mvScaleFactors.size(), 0.5f, (float)th, 0.8f, train_match.data(), &nmatches,
                                       &nToMatch, &n_level_outside, in_view.data(), proj.data(), pred_level.data(), view_cos.data()),
            "cs_match_local_map_frustum");
        in_view.resize(n); proj.resize(n * 3); view_cos.resize(n); pred_level.resize(n); train_match.resize((size_t)N);
        for (size_t i = 0; i < n; i++) if (in_view[i]) m.visible[(size_t)lp[i]]++; // :2712
        for (int i = 0; i < N; i++) if (train_match[(size_t)i] >= 0) F.mvpMapPoints[(size_t)i] = lp[(size_t)train_match[(size_t)i]]; // ORBmatcher.cc:136
    }

    // Tracking::UpdateLastFrame's point creation (:1215-1273): "visual odometry" points for the close key points without a map point (or whose point has no observations);
    // they enter the map's table (TrackMap::append_point), the last frame's slots and mlpTemporalPoints in creation order
    std::vector<int> mlpTemporalPoints;
    void UpdateLastFrame(TrackLastFrame &last, TrackMap &m, const float K4[4], float mThDepth) {
        if (last.is_keyframe || mSensor == MONOCULAR) return;
        const size_t n = last.mvpMapPoints.size();
        std::vector<uint8_t> need_new(n);
        for (size_t i = 0; i < n; i++) need_new[i] = last.mvpMapPoints[i] < 0 || m.n_obs[(size_t)last.mvpMapPoints[i]] < 1;
        const ClosePointsResult r = ClosePoints(ctx_, last.mvDepth, last.mvKeysUn, need_new, last.mTcw, K4, mThDepth, CS_CLOSE_POINTS_NEAREST);
        for (size_t k = 0; k < r.new_idx.size(); k++) {
            const size_t i = (size_t)r.new_idx[k];
            const int id = m.append_point(&r.new_x3D[3 * k], &last.mDescriptors[32 * i]);
            last.mvpMapPoints[i] = id;
            mlpTemporalPoints.push_back(id);
        }
    }

    // what the last TrackWithMotionModel left
    int nmatchesMap = 0, nmatches_tracked = 0, last_direction = 0;
    bool retried = false, mbVO = false;
    std::vector<uint8_t> last_outliers;

    // Tracking::TrackWithMotionModel (:1276-1354).  predicted = mVelocity * mLastFrame.mTcw (3 x 4); the velocity model and the SearchByTracking* step (:1306-1312) stay the caller's
    bool TrackWithMotionModel(TrackFrame &F, TrackLastFrame &last, TrackMap &m, const float predicted[12], const float K4[4], float mThDepth) {
        UpdateLastFrame(last, m, K4, mThDepth); // :1282
        F.SetPose(predicted);                   // :1284
        float Tcw[12];
        F.Tcw(Tcw);
        Tcw_to_pose7(Tcw, F.pose);
        const int N = F.N(), n_last = (int)last.mvKeysUn.size();
        F.mvpMapPoints.assign((size_t)N, -1);   // :1287
        const int th = mSensor != STEREO ? 15 : 7; // :1293-1296
        const bool bMono = mSensor == MONOCULAR;
        std::vector<uint8_t> valid((size_t)n_last), blocks((size_t)n_last), desc(32 * (size_t)n_last), tb;
        std::vector<float> wp(3 * (size_t)n_last);
        for (int i = 0; i < n_last; i++) { // :1398-1405
            const int p = last.mvpMapPoints[(size_t)i];
            const size_t q = (size_t)(p < 0 ? 0 : p);
            valid[(size_t)i] = p >= 0 && !last.mvbOutlier[(size_t)i] && !m.dynamic[q];
            blocks[(size_t)i] = m.n_obs[q] > 0;
            for (int k = 0; k < 3; k++) wp[(size_t)i * 3 + k] = m.world_pos[q * 3 + k];
            for (int k = 0; k < 32; k++) desc[(size_t)i * 32 + k] = m.desc[q * 32 + k];
        }
        if (!F.KeysStatic.empty()) { tb.resize((size_t)N); for (int i = 0; i < N; i++) tb[(size_t)i] = !F.KeysStatic[(size_t)i]; } // :1456 (the frame holds no map point yet, :1451)
        const float mb = F.mbf / F.fx; // Frame.cc:141
        chk(cs_matcher_set_frame(ctx_->ctx, m_, F.mvKeysUn.data(), F.mDescriptors.data(), N, F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY), "cs_matcher_set_frame");
        if (!bMono) ORBmatcher::set_u_right(ctx_, m_, F.mvuRight);
        const ORBmatcher::CurrentFrameView cur{Tcw, F.fx, F.fy, F.cx, F.cy, F.mbf, mb, &F.mvScaleFactors, tb.empty() ? nullptr : &tb, N};
        const ORBmatcher::LastFrameView lst{last.mTcw, &last.mvKeysUn, &valid, &blocks, &desc, &wp};
        auto search = [&](int radius) {
            const ORBmatcher::ProjectionResult r = ORBmatcher::SearchByProjection(ctx_, m_, cur, lst, (float)radius, bMono); // ORBmatcher matcher(0.9, true), :1278
            for (int i = 0; i < N; i++) F.mvpMapPoints[(size_t)i] = r.train_match[(size_t)i] >= 0 ? last.mvpMapPoints[(size_t)r.train_match[(size_t)i]] : -1;
            last_direction = r.direction;
            return r.nmatches;
        };
        int nmatches = search(th);
        retried = nmatches < 20;
        if (nmatches < 20) nmatches = search(2 * th); // :1300-1304
        nmatches_tracked = nmatches; nmatchesMap = 0;
        if (nmatches < 20) return false; // :1314-1318
        std::vector<int> idx;
        std::vector<double> Xw, obs, w;
        for (int i = 0; i < N; i++) {
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
        chk(cs_pose_optimization(ctx_->ctx, 1, off, Xw.data(), obs.data(), w.data(), intr, F.pose, pose_out, flags.data(), &n_inl), "cs_pose_optimization"); // :1321
        for (int k = 0; k < 7; k++) F.pose[k] = pose_out[k];
        pose7_to_Tcw(F.pose, Tcw);
        F.SetPose(Tcw); // Optimizer.cc:468-469
        F.mvbOutlier.assign((size_t)N, 0);
        last_outliers.assign((size_t)N, 0);
        for (int e = 0; e < ne; e++) { // :1326-1345
            const int i = idx[(size_t)e], p = F.mvpMapPoints[(size_t)i];
            last_outliers[(size_t)i] = flags[(size_t)e];
            if (flags[(size_t)e]) {
                F.mvpMapPoints[(size_t)i] = -1;
                m.last_frame_seen[(size_t)p] = F.mnId; // (mbTrackInView = false: the search's own field)
                nmatches--;
            } else if (m.n_obs[(size_t)p] > 0 && !(whether_dynamic_object && m.dynamic[(size_t)p])) nmatchesMap++;
        }
        nmatches_tracked = nmatches;
        if (mbOnlyTracking) { mbVO = nmatchesMap < 10; return nmatches > 20; } // :1347-1351
        return nmatchesMap >= 10;
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
