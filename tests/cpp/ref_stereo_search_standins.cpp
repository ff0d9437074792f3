// TEST INFRASTRUCTURE: stand-ins for the SLAM classes that the reference's two tracking searches touch -- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)
// (orb_object_slam/src/ORBmatcher.cc:1373-1522) and ORBmatcher::SearchByProjection(F, vpMapPoints, th) (:50-142) with RadiusByViewingCos, DescriptorDistance,
// ComputeThreeMaxima and Frame::GetFeaturesInArea (Frame.cc:404-459).  tests/test_stereo_search_restatement_pins.py cuts those functions out of the reference at test time into a
// temporary directory (ref_stereo_search_extracted.inc), compiles this file around them there and runs them next to tests/stereo_search_restatement.py on the same inputs.  The
// classes carry just the members those functions read, under the reference's names; every statement of the functions is the reference's.
#include <cassert>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "cvshim.hpp"

// ---- float matrices the way cv::MatExpr evaluates them: alpha * A * B + C is one gemm with double accumulation over k ascending and a single rounding to float; -A.t() is the
// scale -1 on the product (cv::gemm applies alpha to the double sum)
namespace cv {
struct NegMat { Mat m; };
inline NegMat operator-(const Mat &m) { return NegMat{m}; }
struct MulExpr {
    Mat a, b; double alpha;
    Mat eval(const Mat *c) const {
        Mat r(a.rows, b.cols, CV_32F);
        for (int i = 0; i < a.rows; i++) for (int j = 0; j < b.cols; j++) {
            double s = 0;
            for (int k = 0; k < a.cols; k++) s += (double)a.at<float>(i, k) * (double)b.at<float>(k, j);
            r.at<float>(i, j) = (float)(s * alpha + (c ? (double)c->at<float>(i, j) * 1.0 : 0.0));
        }
        return r;
    }
    operator Mat() const { return eval(nullptr); }
};
inline MulExpr operator*(const Mat &a, const Mat &b) { return MulExpr{a, b, 1.0}; }
inline MulExpr operator*(const NegMat &a, const Mat &b) { return MulExpr{a.m, b, -1.0}; }
inline Mat operator+(const MulExpr &e, const Mat &c) { return e.eval(&c); }
} // namespace cv

namespace ORB_SLAM2 {
using namespace std;
#define FRAME_GRID_ROWS 48 // Frame.h:32-33
#define FRAME_GRID_COLS 64

class MapPoint {
  public:
    cv::Mat mWorldPos, mDescriptor;
    bool bad = false, is_dynamic = false;
    int index = -1, nObs = 0;
    float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackViewCos = 0; // MapPoint.h:110-118
    bool mbTrackInView = false;
    int mnTrackScaleLevel = 0;
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    bool isBad() { return bad; }
    int Observations() { return nObs; }
};
class Frame {
  public:
    int N = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mb = 0, mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0, mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    cv::Mat mTcw, mDescriptors;
    std::vector<float> mvScaleFactors, mvuRight;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<bool> KeysStatic, mvbOutlier;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel = -1, const int maxLevel = -1) const;
};
class ORBmatcher {
  public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b);
    int SearchByProjection(Frame &F, const std::vector<MapPoint *> &vpMapPoints, const float th = 3);
    int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono);
    static const int TH_LOW, TH_HIGH, HISTO_LENGTH;
  protected:
    float RadiusByViewingCos(const float &viewCos);
    void ComputeThreeMaxima(std::vector<int> *histo, const int L, int &ind1, int &ind2, int &ind3);
    float mfNNratio;
    bool mbCheckOrientation;
};

#include "ref_stereo_search_extracted.inc"

} // namespace ORB_SLAM2

namespace {
using namespace ORB_SLAM2;
struct FrameIn { int N; const float *x, *y, *angle; const int *octave; const unsigned char *desc, *dynamic /* nullable: !KeysStatic */; float minX, maxX, minY, maxY; };
struct CamIn { float fx, fy, cx, cy, bf, mb; const float *scale_factors; int n_levels; };

cv::Mat mat(int r, int c, const float *v) { cv::Mat m(r, c, CV_32F); for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.at<float>(i, j) = v[i * c + j]; return m; }
cv::Mat pose44(const float *T34) { cv::Mat m = cv::Mat(4, 4, CV_32F); for (int i = 0; i < 16; i++) m.at<float>(i / 4, i % 4) = i < 12 ? T34[i] : (i == 15 ? 1.0f : 0.0f); return m; }
// AssignFeaturesToGrid / PosInGrid (Frame.cc:303-318, :525-535): our text -- the window function that reads the grid is the reference's
void fill(Frame &F, const FrameIn &I, const CamIn &C, const float *u_right, const unsigned char *pre_blocked, MapPoint *before) {
    F.N = I.N; F.fx = C.fx; F.fy = C.fy; F.cx = C.cx; F.cy = C.cy; F.mbf = C.bf; F.mb = C.mb; F.mnMinX = I.minX; F.mnMaxX = I.maxX; F.mnMinY = I.minY; F.mnMaxY = I.maxY;
    F.mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(F.mnMaxX - F.mnMinX);
    F.mfGridElementHeightInv = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(F.mnMaxY - F.mnMinY);
    F.mvScaleFactors.assign(C.scale_factors, C.scale_factors + C.n_levels);
    F.mDescriptors = cv::Mat(I.N > 0 ? I.N : 1, 32, CV_8U);
    if (I.N) memcpy(F.mDescriptors.data, I.desc, (size_t)I.N * 32);
    F.mvpMapPoints.assign((size_t)I.N, nullptr);
    F.mvbOutlier.assign((size_t)I.N, false);
    F.mvuRight.assign((size_t)I.N, -1.0f);
    if (u_right) F.mvuRight.assign(u_right, u_right + I.N);
    if (I.dynamic) { F.KeysStatic.resize((size_t)I.N); for (int i = 0; i < I.N; i++) F.KeysStatic[i] = !I.dynamic[i]; }
    for (int i = 0; i < I.N; i++) {
        F.mvKeysUn.push_back(cv::KeyPoint(I.x[i], I.y[i], 31.f, I.angle[i], 0.f, I.octave[i]));
        F.mvKeys.push_back(F.mvKeysUn.back());
        if (pre_blocked && pre_blocked[i]) F.mvpMapPoints[i] = before;
        const int px = (int)std::round((I.x[i] - F.mnMinX) * F.mfGridElementWidthInv), py = (int)std::round((I.y[i] - F.mnMinY) * F.mfGridElementHeightInv);
        if (px < 0 || px >= FRAME_GRID_COLS || py < 0 || py >= FRAME_GRID_ROWS) continue;
        F.mGrid[px][py].push_back((size_t)i);
    }
}
MapPoint *point(int i, const float *world_pos, const unsigned char *desc, int n_obs, std::vector<std::unique_ptr<MapPoint>> &own) {
    own.emplace_back(new MapPoint());
    MapPoint *p = own.back().get();
    p->index = i; p->nObs = n_obs;
    if (world_pos) p->mWorldPos = mat(3, 1, world_pos + 3 * i);
    p->mDescriptor = cv::Mat(1, 32, CV_8U); memcpy(p->mDescriptor.data, desc + 32 * (size_t)i, 32);
    return p;
}
void read_back(const Frame &F, const MapPoint *before, int *train_match) {
    for (int i = 0; i < F.N; i++) train_match[i] = (F.mvpMapPoints[i] && F.mvpMapPoints[i] != before) ? F.mvpMapPoints[i]->index : -1;
}
} // namespace

extern "C" {
// SearchByProjection(CurrentFrame, LastFrame, th, bMono).  The last frame's key point i carries level last_octave[i], angle last_angle[i] and, with valid[i], a map point at
// world_pos[i] with descriptor mp_desc[i] and Observations() = blocks[i] ? 2 : 0.  u_right[N] = CurrentFrame.mvuRight; pre_blocked[N] (nullable): the key point holds a map point
// with observations from before.  Out: train_match[N] (the last frame's index, -1 none or from before), *direction (0 neither, 1 forward, 2 backward, read off the same two
// statements :1393-1394 on a copy of the matrices).  Returns nmatches.
int pin_search_by_projection_frame(const FrameIn *CUR, const CamIn *C, const float *u_right, const unsigned char *pre_blocked, int n_last, const float *world_pos, const unsigned char *valid,
                                   const unsigned char *blocks, const unsigned char *mp_desc, const int *last_octave, const float *last_angle, const float *Tcw, const float *Tlw, float th,
                                   int mono, int check_orientation, int *train_match, float *tlc_z) {
    static Frame F, L; F = Frame(); L = Frame(); // (the grid is a large array: not on the stack)
    MapPoint before; before.nObs = 1;
    fill(F, *CUR, *C, u_right, pre_blocked, &before);
    F.mTcw = pose44(Tcw); L.mTcw = pose44(Tlw);
    L.N = n_last;
    std::vector<std::unique_ptr<MapPoint>> own;
    for (int i = 0; i < n_last; i++) {
        L.mvKeys.push_back(cv::KeyPoint(0.f, 0.f, 31.f, last_angle[i], 0.f, last_octave[i]));
        L.mvKeysUn.push_back(L.mvKeys.back());
        L.mvbOutlier.push_back(false);
        L.mvpMapPoints.push_back(valid[i] ? point(i, world_pos, mp_desc, blocks[i] ? 2 : 0, own) : nullptr);
    }
    {   // tlc.z as the function computes it (:1383-1391), for the caller to compare
        const cv::Mat Rcw = F.mTcw.rowRange(0, 3).colRange(0, 3), tcw = F.mTcw.rowRange(0, 3).col(3);
        const cv::Mat twc = -Rcw.t() * tcw;
        const cv::Mat Rlw = L.mTcw.rowRange(0, 3).colRange(0, 3), tlw = L.mTcw.rowRange(0, 3).col(3);
        const cv::Mat tlc = Rlw * twc + tlw;
        *tlc_z = tlc.at<float>(2);
    }
    ORBmatcher m(0.9f, check_orientation != 0);
    const int n = m.SearchByProjection(F, L, th, mono != 0);
    read_back(F, &before, train_match);
    return n;
}

// SearchByProjection(F, vpMapPoints, th) over the fields isInFrustum left: proj (mTrackProjX, mTrackProjY, mTrackProjXR per point), view_cos, level, in_view.
int pin_search_local_map(const FrameIn *CUR, const CamIn *C, const float *u_right, const unsigned char *pre_blocked, int n_mp, const float *proj, const float *view_cos, const int *level,
                         const unsigned char *in_view, const unsigned char *blocks, const unsigned char *mp_desc, float th, float nnratio, int *train_match) {
    static Frame F; F = Frame();
    MapPoint before; before.nObs = 1;
    fill(F, *CUR, *C, u_right, pre_blocked, &before);
    std::vector<std::unique_ptr<MapPoint>> own;
    std::vector<MapPoint *> v;
    for (int i = 0; i < n_mp; i++) {
        MapPoint *p = point(i, nullptr, mp_desc, blocks[i] ? 2 : 0, own);
        p->mbTrackInView = in_view[i] != 0; p->mTrackProjX = proj[3 * i]; p->mTrackProjY = proj[3 * i + 1]; p->mTrackProjXR = proj[3 * i + 2];
        p->mTrackViewCos = view_cos[i]; p->mnTrackScaleLevel = level[i];
        v.push_back(p);
    }
    ORBmatcher m(nnratio, true);
    const int n = m.SearchByProjection(F, v, th);
    read_back(F, &before, train_match);
    return n;
}
}
