// orb_slam_mirrors.hpp -- dependency-free C++ host-side mirrors of the orb_object_slam / line_lbd entry points on the hot path, over
// the C-ABI (include/cubeslam_hip.h): same class names, constructor arguments, method names and member defaults as the reference;
// plain arrays where the reference passes cv::Mat / KeyFrame*.  The adapters with the reference's exact signatures
// are thin wrappers around these and compile only in a tree that provides OpenCV / Eigen / the ORB-SLAM2 map classes.
//   cubeslam::ORBextractor      ORB_SLAM2::ORBextractor      (orb_object_slam/include/ORBextractor.h:44-112)
//   cubeslam::Frame             ORB_SLAM2::Frame, the stereo members (orb_object_slam/include/Frame.h, src/Frame.cc:94-144, :611-783):
//                               ComputeStereoMatches over two extractors, mvuRight / mvDepth; the RGB-D members (:146-199, :334-344, :785-822):
//                               ComputeStereoFromRGBD, UpdatePoseMatrices, UnprojectStereo
//   cubeslam::ClosePoints       the creation of map points from measured depth in Tracking::StereoInitialization, UpdateLastFrame and CreateNewKeyFrame
//                               (src/Tracking.cc:783-850, :1207-1274, :2067-2130)
//   cubeslam::ORBmatcher        ORB_SLAM2::ORBmatcher: set_u_right and SearchByProjection(CurrentFrame, LastFrame, th, bMono) with its stereo branch (src/ORBmatcher.cc:1373-1522,
//                               include/cubeslam_hip/stereo_search.h) over a cs_matcher that holds the current frame; the dynamic-object KLT (src/ORBmatcher.cc:1524-1580): SearchByTrackingHarris over two gray frames, with the
//                               cv::calcOpticalFlowPyrLK call of :1548 / :1620 as ORBmatcher::calcOpticalFlowPyrLK, and SearchByTracking (:1582-1725) over the current
//                               frame's mvKeysUn
//   cubeslam::goodFeaturesToTrack   cv::goodFeaturesToTrack as Tracking::CreateNewKeyFrame calls it (src/Tracking.cc:2292), csrc/gftt_math.h
//   cubeslam::line_lbd_detect   line_lbd_detect              (line_lbd/include/line_lbd/line_lbd_allclass.h:22-70)
//   cubeslam::Optimizer         ORB_SLAM2::Optimizer         (orb_object_slam/include/Optimizer.h:39-62): BundleAdjustment over the
//                               flattened graph (cs_ba_problem), PoseOptimization over flattened matches, OptimizeSim3 over flattened correspondences,
//                               LocalBACameraPointObjectsDynamic over the flattened dynamic graph (cs_ba_dyn_problem)
// With CUBESLAM_HOST_ONLY defined the header holds the RGB-D members of Frame, ClosePoints ORBmatcher's KLT and goodFeaturesToTrack alone, on their path without a context (csrc/rgbd_math.h,
// csrc/klt_math.h and csrc/gftt_math.h, the text the kernels run; compile with -ffp-contract=off): of the C header only the types are used and nothing of the library is linked.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "../../include/cubeslam_hip/stereo_search.h"
#include "../csrc/gftt_math.h"
#include "../csrc/klt_math.h"
#include "../csrc/rgbd_math.h"
#ifndef CUBESLAM_HOST_ONLY
#include "detect_3d_cuboid.hpp" // cubeslam::Context
#else
namespace cubeslam { struct Context; class ORBextractor; }
#endif

namespace cubeslam {

#ifndef CUBESLAM_HOST_ONLY
inline void check(cs_ctx *ctx, int r, const char *what) {
    if (r != CS_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(r) + "): " + cs_last_error(ctx));
}

class ORBextractor {
  public:
    // ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST) + the image size the device buffers are for
    ORBextractor(Context &c, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int width, int height)
        : ctx_(c), nfeatures_(nfeatures), nlevels_(nlevels), W_(width), H_(height) {
        check(ctx_.ctx, cs_orb_create(ctx_.ctx, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, 1, &e_), "cs_orb_create");
    }
    ~ORBextractor() { cs_orb_destroy(ctx_.ctx, e_); }
    ORBextractor(const ORBextractor &) = delete;
    ORBextractor &operator=(const ORBextractor &) = delete;
    // operator()(InputArray image, InputArray mask, vector<KeyPoint>& keypoints, OutputArray descriptors): mask is ignored like in the
    // reference (:1036-1040); descriptors = keypoints.size() x 32 bytes
    void operator()(const uint8_t *gray, int stride, std::vector<cs_keypoint> &keypoints, std::vector<uint8_t> &descriptors) {
        const int cap = nfeatures_ + 4 * nlevels_ + 64;
        keypoints.resize((size_t)cap); descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(ctx_.ctx, cs_orb_extract(ctx_.ctx, e_, gray, 1, stride, keypoints.data(), descriptors.data(), cap, &n), "cs_orb_extract");
        keypoints.resize((size_t)n); descriptors.resize((size_t)n * 32);
    }
    int GetLevels() const { return nlevels_; }
    std::vector<float> GetScaleFactors() const { return table(0); }
    std::vector<float> GetInverseScaleFactors() const { return table(1); }
    std::vector<float> GetScaleSigmaSquares() const { return table(2); }
    std::vector<float> GetInverseScaleSigmaSquares() const { return table(3); }
    cs_orb *handle() { return e_; }

  private:
    std::vector<float> table(int which) const { std::vector<float> t((size_t)nlevels_); cs_orb_get_table(e_, which, t.data()); return t; }
    Context &ctx_;
    cs_orb *e_ = nullptr;
    int nfeatures_, nlevels_, W_, H_;
};

#endif // CUBESLAM_HOST_ONLY

// The stereo part of ORB_SLAM2::Frame: what the stereo constructor (Frame.cc:94-144) does between the two extractions (:106-110) and
// AssignFeaturesToGrid: ComputeStereoMatches (:118, :611-783) on the device, from what the two extractors' last operator() left there.
// The RGB-D part: what the RGB-D constructor (:146-199) does behind UndistortKeyPoints, ComputeStereoFromRGBD (:173, :785-806), and the pose and
// unprojection members the close-point rule reads (:334-344, :808-822).
class Frame {
  public:
#ifndef CUBESLAM_HOST_ONLY
    // Frame(..., ORBextractor *extractorLeft, ORBextractor *extractorRight, ..., const float &bf, ...).  mb: the reference's constructor sets
    // mb = mbf / fx at :141, after ComputeStereoMatches ran at :118, so its first frame runs with whatever the member held; set mb to the value meant.
    Frame(Context &c, ORBextractor *extractorLeft, ORBextractor *extractorRight, float bf, float b, int max_keypoints)
        : mbf(bf), mb(b), mpORBextractorLeft(extractorLeft), mpORBextractorRight(extractorRight), ctx_(&c) {
        check(ctx_->ctx, cs_stereo_create(ctx_->ctx, max_keypoints, 1, &s_), "cs_stereo_create");
    }
#endif
    // The RGB-D frame over the caller's mvKeys / mvKeysUn (fill them before ComputeStereoFromRGBD): K4 = fx fy cx cy, the size of the depth image.  Without a context
    // (c == nullptr) every member runs on the host, byte-equal to the device.
    Frame(Context *c, const float K4[4], float bf, int width, int height)
        : mbf(bf), mb(bf / K4[0]), mpORBextractorLeft(nullptr), mpORBextractorRight(nullptr), fx(K4[0]), fy(K4[1]), cx(K4[2]), cy(K4[3]), invfx(1.0f / K4[0]), invfy(1.0f / K4[1]),
          width_(width), height_(height), ctx_(c) {}
    ~Frame() {
#ifndef CUBESLAM_HOST_ONLY
        if (s_) cs_stereo_destroy(ctx_->ctx, s_);
        if (r_) cs_rgbd_destroy(ctx_->ctx, r_);
#endif
    }
    Frame(const Frame &) = delete;
    Frame &operator=(const Frame &) = delete;
#ifndef CUBESLAM_HOST_ONLY
    // void Frame::ComputeStereoMatches(): fills mvuRight / mvDepth (N values, -1 where unmatched); returns the number of matches kept
    int ComputeStereoMatches() {
        check(ctx_->ctx, cs_stereo_match_from_orb(ctx_->ctx, s_, mpORBextractorLeft->handle(), 0, mpORBextractorRight->handle(), 0, 1, mbf, mb), "cs_stereo_match_from_orb");
        int first[2] = {0, 0}, n_matched = 0;
        long total = 0;
        check(ctx_->ctx, cs_stereo_read_packed(ctx_->ctx, s_, nullptr, nullptr, 0, first, &total, nullptr), "cs_stereo_read_packed");
        N = (int)total;
        mvuRight.assign((size_t)N + 1, -1.0f); mvDepth.assign((size_t)N + 1, -1.0f);
        check(ctx_->ctx, cs_stereo_read_packed(ctx_->ctx, s_, mvuRight.data(), mvDepth.data(), total, first, &total, &n_matched), "cs_stereo_read_packed");
        mvuRight.resize((size_t)N); mvDepth.resize((size_t)N);
        return n_matched;
    }
    // mvuRight / mvDepth where they were computed, for cs_match_fuse / cs_pose_optimization callers that keep them on the device
    void device(const float **d_uRight, const float **d_depth) const {
        int n = 0;
        if (r_) check(ctx_->ctx, cs_rgbd_device_frame(r_, 0, d_uRight, d_depth, nullptr, &n), "cs_rgbd_device_frame");
        else check(ctx_->ctx, cs_stereo_device_pair(s_, 0, d_uRight, d_depth, &n), "cs_stereo_device_pair");
    }
#endif
    // void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepth) on the RAW depth image (type CS_DEPTH_U16 / CS_DEPTH_F32, rows `stride` bytes apart) with the factor of
    // Tracking::GrabImageRGBD's convertTo (Tracking.cc:388): fills mvuRight / mvDepth for mvKeys / mvKeysUn; returns the number of key points with depth
    int ComputeStereoFromRGBD(const void *depth, int type, long stride, float factor) {
        N = (int)mvKeys.size();
        if (mvKeysUn.size() != mvKeys.size()) throw std::invalid_argument("Frame::ComputeStereoFromRGBD: mvKeys and mvKeysUn differ in length");
        mvuRight.assign((size_t)N + 1, -1.0f); mvDepth.assign((size_t)N + 1, -1.0f);
        int n_with = 0;
        n_outside = 0;
        if (!ctx_) {
            if (cs_rgbd_host_status(depth, type, stride) != CS_OK) throw std::invalid_argument("Frame::ComputeStereoFromRGBD: no image, an unknown type or rows that overlap");
            rgbd_frame_host(depth, type, width_, height_, stride, N, N ? &mvKeys[0].x : nullptr, N ? &mvKeysUn[0].x : nullptr, 7, mbf, factor, mvuRight.data(), mvDepth.data(),
                            &n_with, &n_outside);
        } else {
#ifndef CUBESLAM_HOST_ONLY
            if (!r_ || N > r_cap_) {
                if (r_) cs_rgbd_destroy(ctx_->ctx, r_);
                r_ = nullptr; r_cap_ = N > 0 ? N : 1;
                check(ctx_->ctx, cs_rgbd_create(ctx_->ctx, width_, height_, r_cap_, 1, &r_), "cs_rgbd_create");
            }
            const int first[2] = {0, N};
            int f2[2];
            long total = 0;
            check(ctx_->ctx, cs_rgbd_upload_depth(ctx_->ctx, r_, depth, type, 1, stride), "cs_rgbd_upload_depth");
            check(ctx_->ctx, cs_rgbd_from_keys(ctx_->ctx, r_, 1, first, mvKeys.data(), mvKeysUn.data(), mbf, factor), "cs_rgbd_from_keys");
            check(ctx_->ctx, cs_rgbd_read_packed(ctx_->ctx, r_, mvuRight.data(), mvDepth.data(), (long)N + 1, f2, &total, &n_with, &n_outside), "cs_rgbd_read_packed");
#else
            throw std::runtime_error("Frame: built without the library");
#endif
        }
        mvuRight.resize((size_t)N); mvDepth.resize((size_t)N);
        return n_with;
    }
    // void Frame::SetPose(cv::Mat Tcw) / UpdatePoseMatrices(): Tcw = the rows of [Rcw | tcw]
    void SetPose(const float Tcw[12]) { for (int k = 0; k < 12; k++) mTcw[k] = Tcw[k]; UpdatePoseMatrices(); }
    void UpdatePoseMatrices() { rgbd_pose_matrices(mTcw, mRwc, mOw); }
    // cv::Mat Frame::UnprojectStereo(const int &i): false = the empty Mat of z <= 0
    bool UnprojectStereo(int i, float x3D[3]) const {
        const float z = mvDepth[(size_t)i];
        if (!(z > 0)) return false;
        rgbd_unproject(mvKeysUn[(size_t)i].x, mvKeysUn[(size_t)i].y, z, cx, cy, invfx, invfy, mRwc, mOw, x3D);
        return true;
    }
    int N = 0;
    std::vector<float> mvuRight, mvDepth;
    float mbf, mb;
    ORBextractor *mpORBextractorLeft, *mpORBextractorRight;
    // the RGB-D frame
    std::vector<cs_keypoint> mvKeys, mvKeysUn;
    float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0;
    float mTcw[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, mRwc[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, mOw[3] = {0, 0, 0};
    int n_outside = 0; // key points whose sample lies outside the image (undefined in the reference; they end without depth)

  private:
    static int cs_rgbd_host_status(const void *depth, int type, long stride) { return depth && (type == CS_DEPTH_U16 || type == CS_DEPTH_F32) && stride > 0 ? CS_OK : CS_ERR_BAD_ARG; }
    int width_ = 0, height_ = 0;
    Context *ctx_;
#ifndef CUBESLAM_HOST_ONLY
    cs_stereo *s_ = nullptr;
    cs_rgbd *r_ = nullptr;
    int r_cap_ = 0;
#endif
};

// The close-point rule over one frame's mvDepth (from either depth sensor) and mvKeysUn: what Tracking::UpdateLastFrame (Tracking.cc:1221-1273) and CreateNewKeyFrame
// (:2075-2128) do with mode CS_CLOSE_POINTS_NEAREST, StereoInitialization (:804-819) with CS_CLOSE_POINTS_ALL.  need_new[i] = `!pMP || pMP->Observations() < 1`.
// Without a context the host runs the reference's loop (csrc/rgbd_math.h), byte-equal to the device's closed form.
struct ClosePointsResult {
    int n_valid = 0, n_walked = 0;  // key points with z > 0; nPoints when the loop ends
    std::vector<int> order;         // vDepthIdx after the sort: the indices of all key points with z > 0
    std::vector<int> new_idx;       // the key points a point is created for, in creation order
    std::vector<float> new_x3D;     // Frame::UnprojectStereo of each
};
inline ClosePointsResult ClosePoints(Context *ctx, const std::vector<float> &mvDepth, const std::vector<cs_keypoint> &mvKeysUn, const std::vector<uint8_t> &need_new,
                                     const float Tcw[12], const float K4[4], float thDepth, int mode) {
    const int n = (int)mvDepth.size();
    if (mvKeysUn.size() != (size_t)n || (mode != CS_CLOSE_POINTS_ALL && need_new.size() != (size_t)n) || (mode != CS_CLOSE_POINTS_ALL && mode != CS_CLOSE_POINTS_NEAREST))
        throw std::invalid_argument("ClosePoints: one entry per key point in every array, and a known mode");
    ClosePointsResult r;
    r.order.resize((size_t)n + 1); r.new_idx.resize((size_t)n + 1); r.new_x3D.resize(3 * (size_t)n + 3);
    int n_new = 0;
    if (!ctx) {
        rgbd_close_points_host(n, mvDepth.data(), n ? &mvKeysUn[0].x : nullptr, 7, need_new.data(), Tcw, K4, thDepth, mode, &r.n_valid, r.order.data(), &r.n_walked, &n_new,
                               r.new_idx.data(), r.new_x3D.data());
    } else {
#ifndef CUBESLAM_HOST_ONLY
        const int first[2] = {0, n};
        int new_first[2] = {0, 0};
        check(ctx->ctx, cs_close_points(ctx->ctx, 1, first, mvDepth.data(), mvKeysUn.data(), mode == CS_CLOSE_POINTS_ALL ? nullptr : need_new.data(), Tcw, K4, thDepth, mode, &r.n_valid,
                                        r.order.data(), &r.n_walked, new_first, r.new_idx.data(), r.new_x3D.data()), "cs_close_points");
        n_new = new_first[1];
#else
        throw std::runtime_error("ClosePoints: built without the library");
#endif
    }
    r.order.resize((size_t)r.n_valid); r.new_idx.resize((size_t)n_new); r.new_x3D.resize(3 * (size_t)n_new);
    return r;
}

// The dynamic-object KLT of ORBmatcher (ORBmatcher.cc:1524-1580) over two 8-bit frames of width x height (rows `stride` bytes apart).  Without a context the host
// runs the reference's loop (csrc/klt_math.h), byte-equal to the device.
struct ORBmatcher {
    struct Flow { std::vector<float> nextPts; std::vector<uint8_t> status; std::vector<float> err; }; // currobjpts (x, y per point), status, err
    struct HarrisResult {
        Flow flow;                    // featuresklt_thisframe and the tracker's flags for every point of LastFrame.mvKeysHarris
        std::vector<int> kept;        // indices into LastFrame.mvKeysHarris / mvpMapPointsHarris of the points the current frame keeps, in order
        std::vector<float> pts;       // CurrentFrame.mvKeysHarris (x, y)
        std::vector<int> object_id;   // keypoint_associate_objectID_harris
        int goodmatches = 0, n_mask_outside = 0;
    };
    // cv::calcOpticalFlowPyrLK(last, current, lastobjpts, currobjpts, status, err, cv::Size(21, 21), 3)
    static Flow calcOpticalFlowPyrLK(Context *ctx, const uint8_t *last, const uint8_t *current, int width, int height, long stride, const std::vector<float> &lastobjpts) {
        HarrisResult r;
        run(ctx, last, current, width, height, stride, lastobjpts, nullptr, r);
        return r.flow;
    }
    // objmask = CurrentFrame.objmask_img, width x height, dense
    static HarrisResult SearchByTrackingHarris(Context *ctx, const uint8_t *last, const uint8_t *current, int width, int height, long stride, const std::vector<float> &lastobjpts,
                                               const uint8_t *objmask) {
        if (!objmask) throw std::invalid_argument("SearchByTrackingHarris: no object mask");
        HarrisResult r;
        run(ctx, last, current, width, height, stride, lastobjpts, objmask, r);
        return r;
    }
    // ORBmatcher::SearchByTracking (ORBmatcher.cc:1582-1725).  mvKeysLast = LastFrame.mvKeys, eligible[i] = `mvpMapPoints[i] && !KeysStatic[i] && is_dynamic`,
    // objectID = keypoint_associate_objectID; mvKeysUn and bounds (mnMinX, mnMaxX, mnMinY, mnMaxY) describe the current frame, KeysStatic / hadMapPoint may be empty.
    struct TrackingResult {
        std::vector<int> train_match;   // per key point of the current frame: the last frame's key index whose map point it takes, or -1
        std::vector<int> lastptsinds;   // the last frame's key points that were tracked
        std::vector<float> featuresklt_lastframe, featuresklt_thisframe; // (x, y) per tracked point; (0, 0) for a rejected one
        int kltmatches = 0, goodmatches = 0, findfeaturematches = 0, uniquematches = 0;
    };
    static TrackingResult SearchByTracking(Context *ctx, const uint8_t *last, const uint8_t *current, int width, int height, long stride, const std::vector<cs_keypoint> &mvKeysLast,
                                           const std::vector<uint8_t> &eligible, const std::vector<int> &objectID, int numobject, float th, const std::vector<float> &mvScaleFactors,
                                           const std::vector<cs_keypoint> &mvKeysUn, const float bounds[4], const std::vector<uint8_t> &KeysStatic, const std::vector<uint8_t> &hadMapPoint) {
        const int n_last = (int)mvKeysLast.size(), N = (int)mvKeysUn.size();
        if (!last || !current || width <= KLT_WIN || height <= KLT_WIN || stride < width || eligible.size() != (size_t)n_last || objectID.size() != (size_t)n_last ||
            mvScaleFactors.size() < 3 || (!KeysStatic.empty() && KeysStatic.size() != (size_t)N) || (!hadMapPoint.empty() && hadMapPoint.size() != (size_t)N) || !(bounds[1] > bounds[0]) ||
            !(bounds[3] > bounds[2]))
            throw std::invalid_argument("SearchByTracking: one entry per key point in every array, three scale factors, images of more than 21 pixels a side");
        for (int i = 0; i < n_last; i++)
            if (eligible[(size_t)i] && mvKeysLast[(size_t)i].octave < 3 && (mvKeysLast[(size_t)i].octave < 0 || !(mvKeysLast[(size_t)i].x - mvKeysLast[(size_t)i].x == 0) || !(mvKeysLast[(size_t)i].y - mvKeysLast[(size_t)i].y == 0)))
                throw std::invalid_argument("SearchByTracking: a key point that is not finite or has a negative octave");
        TrackingResult r;
        r.train_match.assign((size_t)N + 1, -1); r.lastptsinds.assign((size_t)n_last + 1, 0);
        r.featuresklt_lastframe.assign(2 * (size_t)n_last + 2, 0.f); r.featuresklt_thisframe.assign(2 * (size_t)n_last + 2, 0.f);
        int counters[4] = {0, 0, 0, 0}, n = 0;
        const cs_keypoint none{};
        const cs_keypoint *lk = n_last ? mvKeysLast.data() : &none, *ck = N ? mvKeysUn.data() : &none;
        const uint8_t *ks = KeysStatic.empty() ? nullptr : KeysStatic.data(), *hm = hadMapPoint.empty() ? nullptr : hadMapPoint.data();
        if (!ctx) {
            n = klt_search_by_tracking_host(last, current, width, height, stride, n_last, &lk->x, &lk->octave, 7, eligible.data(), objectID.data(), numobject, th, mvScaleFactors.data(),
                                            klt_grid_params(N, bounds[0], bounds[1], bounds[2], bounds[3]), &ck->x, &ck->octave, 7, ks, hm, r.train_match.data(), r.lastptsinds.data(),
                                            r.featuresklt_lastframe.data(), r.featuresklt_thisframe.data(), counters);
            if (n < 0) throw std::invalid_argument("SearchByTracking: a tracked point's object id is outside [0, numobject)");
        } else {
#ifndef CUBESLAM_HOST_ONLY
            std::vector<uint8_t> two((size_t)2 * width * height), desc((size_t)32 * (N > 0 ? N : 1), 0);
            for (int f = 0; f < 2; f++)
                for (int y = 0; y < height; y++) std::copy((f ? current : last) + (long)y * stride, (f ? current : last) + (long)y * stride + width, two.begin() + ((size_t)f * height + y) * width);
            cs_klt *h = nullptr;
            cs_matcher *m = nullptr;
            check(ctx->ctx, cs_klt_create(ctx->ctx, 2, width, height, n_last > 0 ? n_last : 1, &h), "cs_klt_create");
            int rc = cs_matcher_create(ctx->ctx, N > 0 ? N : 1, 1, 1, &m);
            if (rc == CS_OK) rc = cs_klt_set_frames(ctx->ctx, h, 2, width, height, two.data(), width);
            if (rc == CS_OK) rc = cs_matcher_set_frame(ctx->ctx, m, ck, desc.data(), N, bounds[0], bounds[1], bounds[2], bounds[3]);
            if (rc == CS_OK)
                rc = cs_match_by_tracking(ctx->ctx, m, h, 0, 1, n_last, lk, n_last ? eligible.data() : (const uint8_t *)&none, n_last ? objectID.data() : &none.octave,
                                          numobject, th, mvScaleFactors.data(), (int)mvScaleFactors.size(), ks, hm, r.train_match.data(), &n, r.lastptsinds.data(),
                                          r.featuresklt_lastframe.data(), r.featuresklt_thisframe.data(), counters);
            cs_matcher_destroy(ctx->ctx, m);
            cs_klt_destroy(ctx->ctx, h);
            check(ctx->ctx, rc, "cs_match_by_tracking");
#else
            throw std::runtime_error("SearchByTracking: built without the library");
#endif
        }
        r.train_match.resize((size_t)N); r.lastptsinds.resize((size_t)n); r.featuresklt_lastframe.resize(2 * (size_t)n); r.featuresklt_thisframe.resize(2 * (size_t)n);
        r.kltmatches = counters[0]; r.goodmatches = counters[1]; r.findfeaturematches = counters[2]; r.uniquematches = counters[3];
        return r;
    }

#ifndef CUBESLAM_HOST_ONLY
    // ---- the stereo / RGB-D branch of the frame-to-frame search (include/cubeslam_hip/stereo_search.h) over a cs_matcher that holds CurrentFrame
    // (cs_matcher_set_frame / cs_matcher_set_frame_from_orb)
    // CurrentFrame.mvuRight for the searches below: one value per key point of the frame the matcher holds, from the host ...
    static void set_u_right(Context *ctx, cs_matcher *m, const std::vector<float> &mvuRight) {
        const float none = -1.0f;
        check(ctx->ctx, cs_matcher_set_u_right(ctx->ctx, m, mvuRight.empty() ? &none : mvuRight.data(), (int)mvuRight.size(), 0), "cs_matcher_set_u_right");
    }
    // ... or from the device pointer cs_rgbd_device_frame / cs_stereo_device_pair hands out (no host round trip; valid until the next search returns)
    static void set_u_right(Context *ctx, cs_matcher *m, const float *d_mvuRight, int n) { check(ctx->ctx, cs_matcher_set_u_right(ctx->ctx, m, d_mvuRight, n, 1), "cs_matcher_set_u_right"); }

    // What SearchByProjection(CurrentFrame, LastFrame, th, bMono) reads of its two frames.  CurrentFrame's key points, descriptors and mvuRight are the matcher's.
    struct CurrentFrameView {
        const float *mTcw;                              // 3 x 4 row-major
        float fx, fy, cx, cy, mbf, mb;
        const std::vector<float> *mvScaleFactors;
        const std::vector<uint8_t> *train_blocked;     // nullable: per key point, `mvpMapPoints[i2] with Observations() > 0` from before, or !KeysStatic[i2] (:1451-1457)
        int N;
    };
    struct LastFrameView {
        const float *mTcw;                              // 3 x 4 row-major
        const std::vector<cs_keypoint> *mvKeysUn;       // level (mvKeys[i].octave) and angle
        // per key point i: valid[i] = `pMP && !mvbOutlier[i] && !pMP->is_dynamic`, GetWorldPos (3 floats), `Observations() > 0`, GetDescriptor (32 bytes)
        const std::vector<uint8_t> *valid, *blocks, *mp_desc;
        const std::vector<float> *world_pos;
    };
    struct ProjectionResult { std::vector<int> train_match; int nmatches = 0, direction = 0; }; // per key point of CurrentFrame the last frame's key point, -1 none; 0 neither, 1 forward, 2 backward
    // ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono) (ORBmatcher.cc:1373-1522)
    static ProjectionResult SearchByProjection(Context *ctx, cs_matcher *m, const CurrentFrameView &CurrentFrame, const LastFrameView &LastFrame, const float th, const bool bMono,
                                               bool mbCheckOrientation = true) {
        const int n_last = (int)LastFrame.mvKeysUn->size();
        if (LastFrame.valid->size() != (size_t)n_last || LastFrame.blocks->size() != (size_t)n_last || LastFrame.mp_desc->size() != 32 * (size_t)n_last ||
            LastFrame.world_pos->size() != 3 * (size_t)n_last || (CurrentFrame.train_blocked && CurrentFrame.train_blocked->size() != (size_t)CurrentFrame.N))
            throw std::invalid_argument("SearchByProjection: one entry per key point in every array");
        std::vector<int> octave((size_t)n_last + 1, 0);
        std::vector<float> angle((size_t)n_last + 1, 0.0f), wp(*LastFrame.world_pos);
        std::vector<uint8_t> valid(*LastFrame.valid), blocks(*LastFrame.blocks), desc(*LastFrame.mp_desc);
        for (int i = 0; i < n_last; i++) { octave[(size_t)i] = (*LastFrame.mvKeysUn)[(size_t)i].octave; angle[(size_t)i] = (*LastFrame.mvKeysUn)[(size_t)i].angle; }
        wp.resize(wp.size() + 3); valid.resize(valid.size() + 1); blocks.resize(blocks.size() + 1); desc.resize(desc.size() + 32); // (never empty)
        ProjectionResult r;
        r.train_match.assign((size_t)CurrentFrame.N + 1, -1);
        check(ctx->ctx, cs_match_by_projection_frame_stereo(ctx->ctx, m, n_last, wp.data(), valid.data(), blocks.data(), desc.data(), octave.data(), angle.data(), CurrentFrame.mTcw,
                                                            CurrentFrame.fx, CurrentFrame.fy, CurrentFrame.cx, CurrentFrame.cy, CurrentFrame.mvScaleFactors->data(),
                                                            (int)CurrentFrame.mvScaleFactors->size(), th, mbCheckOrientation ? 1 : 0,
                                                            CurrentFrame.train_blocked ? CurrentFrame.train_blocked->data() : nullptr, r.train_match.data(), &r.nmatches, LastFrame.mTcw,
                                                            CurrentFrame.mbf, CurrentFrame.mb, bMono ? 1 : 0, &r.direction),
              "cs_match_by_projection_frame_stereo");
        r.train_match.resize((size_t)CurrentFrame.N);
        return r;
    }
#endif

  private:
    static void run(Context *ctx, const uint8_t *last, const uint8_t *current, int width, int height, long stride, const std::vector<float> &pts, const uint8_t *mask,
                    HarrisResult &r) {
        const int n = (int)(pts.size() / 2);
        if (!last || !current || width <= KLT_WIN || height <= KLT_WIN || stride < width || pts.size() % 2) throw std::invalid_argument("ORBmatcher KLT: images of more than 21 pixels a side and (x, y) pairs");
        for (float v : pts) if (!(v - v == 0)) throw std::invalid_argument("ORBmatcher KLT: a point that is not finite");
        r.flow.nextPts.assign(2 * (size_t)n + 2, 0.f); r.flow.status.assign((size_t)n + 1, 0); r.flow.err.assign((size_t)n + 1, 0.f);
        r.kept.assign((size_t)n + 1, 0); r.pts.assign(2 * (size_t)n + 2, 0.f); r.object_id.assign((size_t)n + 1, 0);
        const int first[2] = {0, n}, pp[1] = {0}, pn[1] = {1};
        std::vector<uint8_t> two((size_t)2 * width * height); // the two frames one behind the other, dense
        for (int f = 0; f < 2; f++)
            for (int y = 0; y < height; y++) std::copy((f ? current : last) + (long)y * stride, (f ? current : last) + (long)y * stride + width, two.begin() + ((size_t)f * height + y) * width);
        if (!ctx) {
            klt_track_host(two.data(), 2, width, height, width, (long)width * height, 1, pp, pn, first, pts.data(), r.flow.nextPts.data(), r.flow.status.data(), r.flow.err.data());
            if (mask) r.goodmatches = klt_harris_select_host(n, r.flow.nextPts.data(), r.flow.status.data(), mask, width, height, r.kept.data(), r.pts.data(), r.object_id.data(), &r.n_mask_outside);
        } else {
#ifndef CUBESLAM_HOST_ONLY
            cs_klt *h = nullptr;
            check(ctx->ctx, cs_klt_create(ctx->ctx, 2, width, height, n > 0 ? n : 1, &h), "cs_klt_create");
            int rc = cs_klt_set_frames(ctx->ctx, h, 2, width, height, two.data(), width);
            int kf[2] = {0, 0};
            if (rc == CS_OK)
                rc = mask ? cs_match_by_tracking_harris(ctx->ctx, h, 1, pp, pn, first, pts.data(), mask, r.flow.nextPts.data(), r.flow.status.data(), r.flow.err.data(), kf, r.kept.data(),
                                                        r.pts.data(), r.object_id.data(), &r.goodmatches, &r.n_mask_outside)
                          : cs_klt_track(ctx->ctx, h, 1, pp, pn, first, pts.data(), r.flow.nextPts.data(), r.flow.status.data(), r.flow.err.data());
            cs_klt_destroy(ctx->ctx, h);
            check(ctx->ctx, rc, "ORBmatcher KLT");
#else
            throw std::runtime_error("ORBmatcher KLT: built without the library");
#endif
        }
        r.flow.nextPts.resize(2 * (size_t)n); r.flow.status.resize((size_t)n); r.flow.err.resize((size_t)n);
        r.kept.resize((size_t)r.goodmatches); r.pts.resize(2 * (size_t)r.goodmatches); r.object_id.resize((size_t)r.goodmatches);
    }
};

// cv::goodFeaturesToTrack(image, corners, maxCorners, qualityLevel, minDistance, mask) with blockSize 3 and the minimum eigenvalue (Tracking.cc:2292) over one 8-bit
// image of width x height (rows `stride` bytes apart); mask: dense width x height, or nullptr.  Without a context the host runs csrc/gftt_math.h, byte-equal to the device.
struct GoodFeatures {
    std::vector<float> corners, quality; // (x, y) per corner in the order of acceptance, and its thresholded eigenvalue
    int n_candidates = 0;
};
inline GoodFeatures goodFeaturesToTrack(Context *ctx, const uint8_t *image, int width, int height, long stride, const uint8_t *mask, int maxCorners, double qualityLevel,
                                        double minDistance) {
    if (!image || width < 1 || height < 1 || stride < width || maxCorners < 1 || !(minDistance >= 1) || !(qualityLevel > 0 && qualityLevel <= 1))
        throw std::invalid_argument("goodFeaturesToTrack: an image, maxCorners >= 1, minDistance >= 1 and 0 < qualityLevel <= 1");
    const int cap = maxCorners < GFTT_MAX_CANDIDATES ? maxCorners : GFTT_MAX_CANDIDATES;
    GoodFeatures r;
    r.corners.assign(2 * (size_t)cap, 0.f); r.quality.assign((size_t)cap, 0.f);
    int count = 0;
    if (!ctx) {
        if (!gftt_good_features_host(image, stride, width, height, mask, cap, qualityLevel, minDistance, r.corners.data(), r.quality.data(), &count, &r.n_candidates))
            throw std::length_error("goodFeaturesToTrack: more candidates than GFTT_MAX_CANDIDATES");
    } else {
#ifndef CUBESLAM_HOST_ONLY
        check(ctx->ctx, cs_good_features_images(ctx->ctx, image, 1, width, height, stride, mask, cap, qualityLevel, minDistance, r.corners.data(), r.quality.data(), &count, &r.n_candidates),
              "cs_good_features_images");
#else
        throw std::runtime_error("goodFeaturesToTrack: built without the library");
#endif
    }
    r.corners.resize(2 * (size_t)count); r.quality.resize((size_t)count);
    return r;
}

#ifndef CUBESLAM_HOST_ONLY
class line_lbd_detect {
  public:
    line_lbd_detect(Context &c, int width, int height) : ctx_(c), W_(width), H_(height) { check(ctx_.ctx, cs_lsd_create(ctx_.ctx, width, height, 1, &l_), "cs_lsd_create"); }
    ~line_lbd_detect() { cs_lsd_destroy(ctx_.ctx, l_); }
    line_lbd_detect(const line_lbd_detect &) = delete;
    line_lbd_detect &operator=(const line_lbd_detect &) = delete;
    // detect_raw_lines(const cv::Mat& gray_img, std::vector<KeyLine>& keylines_out)
    void detect_raw_lines(const uint8_t *gray, int stride, std::vector<cs_keyline> &keylines_out) {
        keylines_out.resize(cap_);
        int n = 0;
        check(ctx_.ctx, cs_lsd_detect(ctx_.ctx, l_, gray, 1, stride, keylines_out.data(), (int)cap_, &n), "cs_lsd_detect");
        keylines_out.resize((size_t)n);
    }
    // detect_filter_lines(const cv::Mat& gray_img, cv::Mat& linesmat_out): rows of x1 y1 x2 y2 (CV_32F), lineLength > line_length_thres
    void detect_filter_lines(const uint8_t *gray, int stride, std::vector<float> &linesmat_out) {
        linesmat_out.resize(cap_ * 4);
        int n = 0;
        check(ctx_.ctx, cs_lsd_detect_filter_lines(ctx_.ctx, l_, gray, 1, stride, (float)line_length_thres, linesmat_out.data(), (int)cap_, &n), "cs_lsd_detect_filter_lines");
        linesmat_out.resize((size_t)n * 4);
    }
    // get_line_descriptors(gray, keylines, descriptors): 32-byte LBD per KeyLine
    void get_line_descriptors(const uint8_t *gray, int stride, const std::vector<cs_keyline> &keylines, std::vector<uint8_t> &line_descrips) {
        line_descrips.assign(keylines.size() * 32, 0);
        if (keylines.empty()) return;
        check(ctx_.ctx, cs_lbd_compute(ctx_.ctx, gray, W_, H_, stride, keylines.data(), (int)keylines.size(), line_descrips.data(), nullptr), "cs_lbd_compute");
    }
    // public members of the reference class, same names and defaults (line_lbd_allclass.h:27-31, constructor line_lbd/class/line_lbd_allclass.cpp:117-123)
    bool use_LSD = false; // the EDLine detector is not on the hot path: every method here runs the LSD detector
    float line_length_thres = 50;
    int numoctaves_ = 1;
    float octaveratio_ = 2.0f;

  private:
    Context &ctx_;
    cs_lsd *l_ = nullptr;
    int W_, H_;
    size_t cap_ = 20000;
};

struct Optimizer {
    // Optimizer::BundleAdjustment / LocalBACameraPointObjects: the caller flattens key frames, map points, objects and their edges into
    // cs_ba_problem; estimates come back in the same order.  pbStopFlag is polled where g2o polls forceStopFlag.
    static cs_ba_stats BundleAdjustment(Context &c, const cs_ba_problem &problem, int nIterations, const volatile int *pbStopFlag, std::vector<double> &cam_pose,
                                        std::vector<double> &points, std::vector<double> &cuboid_pose) {
        cs_ba *b = nullptr;
        check(c.ctx, cs_ba_create(c.ctx, &problem, 0, 1, &b), "cs_ba_create");
        cs_ba_stats st{};
        int r = cs_ba_optimize(c.ctx, b, nIterations, pbStopFlag, &st);
        cam_pose.assign((size_t)problem.n_cams * 7, 0.0); points.assign((size_t)problem.n_points * 3, 0.0); cuboid_pose.assign((size_t)(problem.n_cuboids > 0 ? problem.n_cuboids : 1) * 7, 0.0);
        if (r == CS_OK) r = cs_ba_read(c.ctx, b, cam_pose.data(), points.data(), cuboid_pose.data());
        cs_ba_destroy(c.ctx, b);
        check(c.ctx, r, "cs_ba_optimize");
        cuboid_pose.resize((size_t)problem.n_cuboids * 7);
        return st;
    }
    // Optimizer::PoseOptimization(Frame*): matched map points Xw (n x 3), observations (u, v, u_right or < 0) (n x 3), invSigma2 (n),
    // intrinsics (fx fy cx cy bf), pose [t, q] in / out, mvbOutlier out; returns nInitialCorrespondences - nBad
    static int PoseOptimization(Context &c, int n, const double *Xw, const double *obs, const double *inv_sigma2, const double intr[5], const double pose_in[7],
                                double pose_out[7], std::vector<uint8_t> &mvbOutlier) {
        const int off[2] = {0, n};
        int n_inl = 0;
        mvbOutlier.assign((size_t)n + 1, 0);
        check(c.ctx, cs_pose_optimization(c.ctx, 1, off, Xw, obs, inv_sigma2, intr, pose_in, pose_out, mvbOutlier.data(), &n_inl), "cs_pose_optimization");
        mvbOutlier.resize((size_t)n);
        return n_inl;
    }
    // Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (Optimizer.cc:2838-3033) over the n correspondences that survive its filter (:2893-2928):
    // P1c / P2c (n x 3) are its float R * P + t products, obs1 / obs2 (n x 2) the undistorted key points, inv_sigma2_* their mvInvLevelSigma2[octave], intr
    // (fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2), sim3 [t, qx qy qz qw, s] in / out (out = in where the reference returns before writing g2oS12); removed[c] = 1 where it sets
    // vpMatches1[idx] = NULL; returns nIn
    static int OptimizeSim3(Context &c, int n, const double *P1c, const double *P2c, const double *obs1, const double *obs2, const double *inv_sigma2_1, const double *inv_sigma2_2,
                            const double intr[8], const double sim3_in[8], float th2, bool bFixScale, double sim3_out[8], std::vector<uint8_t> &removed) {
        const int off[2] = {0, n};
        const uint8_t fix = bFixScale ? 1 : 0;
        int n_in = 0;
        removed.assign((size_t)n + 1, 0);
        check(c.ctx, cs_sim3_optimization(c.ctx, 1, off, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, intr, sim3_in, &th2, &fix, sim3_out, removed.data(), &n_in), "cs_sim3_optimization");
        removed.resize((size_t)n);
        return n_in;
    }
    // Optimizer::LocalBACameraPointObjectsDynamic (Optimizer.cc:2353-2415) on a graph the caller flattened from the map (:1684-2344):
    // optimize(5); reprojection edges with chi2 > 5.991 / 7.815 or a non-positive depth and dynamic-point edges with chi2 > 8 go to level 1
    // and all of them lose their kernel, camera-object edges with |error| > 80 go to level 1; optimize(10).  The estimates in `g` are
    // updated in place; the returned levels are what :2418-2447 turns into vToErase.
    struct DynamicGraph { // owns the arrays cs_ba_dyn_problem points into
        cs_ba_dyn_problem P{};
        std::vector<double> cam_pose, obj_pose, vel, points, dpoints;
        std::vector<uint8_t> obs_level, dobs_level, cobs_level;
        void bind() {
            P.cam_pose = cam_pose.data(); P.obj_pose = obj_pose.data(); P.vel = vel.data(); P.points = points.data(); P.dpoints = dpoints.data();
            P.obs_level = obs_level.data(); P.dobs_level = dobs_level.data(); P.cobs_level = cobs_level.data();
        }
    };
    static void LocalBACameraPointObjectsDynamic(Context &c, DynamicGraph &g, const volatile int *pbStopFlag = nullptr, cs_ba_stats *st1 = nullptr, cs_ba_stats *st2 = nullptr) {
        cs_ba_dyn_problem &P = g.P;
        g.obs_level.resize((size_t)P.n_obs + 1, 0); g.dobs_level.resize((size_t)P.n_dobs + 1, 0); g.cobs_level.resize((size_t)P.n_cobs + 1, 0);
        g.bind();
        auto stage = [&](int iterations, cs_ba_stats *st, std::vector<double> &eo, std::vector<double> &ed, std::vector<double> &ec) {
            cs_ba_dyn *ba = nullptr;
            check(c.ctx, cs_ba_dyn_create(c.ctx, &P, &ba), "cs_ba_dyn_create");
            int r = cs_ba_dyn_optimize(c.ctx, ba, iterations, pbStopFlag, st);
            if (!r) r = cs_ba_dyn_read(c.ctx, ba, g.cam_pose.data(), g.obj_pose.data(), g.vel.data(), g.points.data(), g.dpoints.data());
            eo.assign((size_t)P.n_obs * 3 + 1, 0.0); ed.assign((size_t)P.n_dobs * 2 + 1, 0.0); ec.assign((size_t)P.n_cobs * 4 + 1, 0.0);
            if (!r) r = cs_ba_dyn_errors(c.ctx, ba, nullptr, eo.data(), ed.data(), nullptr, ec.data(), nullptr, nullptr);
            cs_ba_dyn_destroy(c.ctx, ba);
            check(c.ctx, r, "cs_ba_dyn stage");
        };
        std::vector<double> eo, ed, ec;
        stage(5, st1, eo, ed, ec);
        if (pbStopFlag && *pbStopFlag) return; // bDoMore = false
        for (int o = 0; o < P.n_obs; o++) { // :2366-2394
            const double *e = &eo[(size_t)o * 3], w = P.obs_inv_sigma2[o];
            const bool stereo = P.obs_ur && P.obs_ur[o] >= 0;
            const double chi2 = stereo ? ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) * w : (e[0] * e[0] + e[1] * e[1]) * w;
            const double *T = &g.cam_pose[(size_t)P.obs_cam[o] * 7], *X = &g.points[(size_t)P.obs_point[o] * 3];
            const double qx = T[3], qy = T[4], qz = T[5], qw = T[6]; // third row of R(q) times X plus t_z: isDepthPositive
            const double z = (2 * (qx * qz - qy * qw)) * X[0] + (2 * (qy * qz + qx * qw)) * X[1] + (1 - 2 * (qx * qx + qy * qy)) * X[2] + T[2];
            if (chi2 > (stereo ? 7.815 : 5.991) || !(z > 0)) g.obs_level[o] = 1;
        }
        for (int o = 0; o < P.n_dobs; o++) { const double *e = &ed[(size_t)o * 2]; if ((e[0] * e[0] + e[1] * e[1]) * P.dobs_inv_sigma2[o] > 8) g.dobs_level[o] = 1; } // :2396-2404
        for (int o = 0; o < P.n_cobs; o++) { const double *e = &ec[(size_t)o * 4]; if (((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3] > 80.0 * 80.0) g.cobs_level[o] = 1; } // :2406-2411
        P.huber_mono = P.huber_stereo = P.huber_dyn = 0; // setRobustKernel(0)
        stage(10, st2, eo, ed, ec);
    }
};

#endif // CUBESLAM_HOST_ONLY

} // namespace cubeslam
