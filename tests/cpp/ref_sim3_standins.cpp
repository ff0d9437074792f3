// TEST INFRASTRUCTURE: stand-ins for the SLAM classes that the reference's Sim3 / relocalisation searches touch -- ORBmatcher::SearchByProjection(pKF, Scw, ...)
// (orb_object_slam/src/ORBmatcher.cc:309-427), Fuse(pKF, Scw, ...) (:1010-1139), SearchBySim3 (:1141-1371), SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
// (:1727-1858) with ComputeThreeMaxima / DescriptorDistance, MapPoint::PredictScale and the two distance getters, KeyFrame::GetFeaturesInArea / IsInImage and
// Frame::GetFeaturesInArea.  tests/test_sim3_restatement_pins.py cuts those functions out of the reference at test time into a temporary directory (ref_sim3_extracted.inc),
// compiles this file around them there and runs them next to tests/sim3_restatement.py on the same inputs.  MapPoint, KeyFrame, Frame and the ORBmatcher declaration carry just
// the members those functions read, under the reference's names; every statement of the searches is the reference's.
#include <cassert>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <set>
#include <vector>

#include "cvshim.hpp"

// ---- float matrices the way cv::MatExpr evaluates them: A * B (+ C) is one gemm with double accumulation and a single rounding to float; a scalar scales every element
// (the pins use scales of 1, 2 and 0.5 only: exact under any reading); Mat - Mat is float; cv::norm and Mat::dot (cvshim.hpp) accumulate in double
namespace cv {
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
struct NegExpr { Mat m; };
inline MulExpr operator*(const Mat &a, const Mat &b) { return MulExpr{a, b, 1.0}; }
inline MulExpr operator*(const NegExpr &a, const Mat &b) { return MulExpr{a.m, b, -1.0}; }
inline Mat operator+(const MulExpr &e, const Mat &c) { return e.eval(&c); }
inline NegExpr operator-(const Mat &m) { return NegExpr{m}; }
inline Mat scaled(const Mat &m, double s) { Mat r(m.rows, m.cols, CV_32F); for (int i = 0; i < m.rows; i++) for (int j = 0; j < m.cols; j++) r.at<float>(i, j) = (float)((double)m.at<float>(i, j) * s); return r; }
inline Mat operator*(double s, const Mat &m) { return scaled(m, s); }
inline Mat operator/(const Mat &m, double s) { return scaled(m, 1.0 / s); }
inline Mat operator-(const Mat &a, const Mat &b) { Mat r(a.rows, a.cols, CV_32F); for (int i = 0; i < a.rows * a.cols; i++) r.at<float>(i) = a.at<float>(i) - b.at<float>(i); return r; } // CV_32F vectors
inline double norm(const Mat &m) { double s = 0; for (int i = 0; i < m.rows * m.cols; i++) s += (double)m.at<float>(i) * (double)m.at<float>(i); return std::sqrt(s); }
} // namespace cv

namespace ORB_SLAM2 {
using namespace std;
#define FRAME_GRID_ROWS 48 // Frame.h:32-33
#define FRAME_GRID_COLS 64

class KeyFrame;
class MapPoint {
  public:
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    std::mutex mMutexPos;
    bool bad = false, is_dynamic = false;
    int index = -1;          // its place in the caller's list
    long added_idx = -1;     // AddObservation's key point
    static MapPoint *&current() { static MapPoint *p = nullptr; return p; } // the map point whose descriptor was fetched last (Fuse: the one being searched for)
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { current() = this; return mDescriptor.clone(); }
    bool isBad() { return bad; }
    int GetIndexInKeyFrame(KeyFrame *) { return -1; }
    void AddObservation(KeyFrame *, size_t idx) { added_idx = (long)idx; }
    float GetMinDistanceInvariance();
    float GetMaxDistanceInvariance();
    int PredictScale(const float &currentDist, const float &logScaleFactor);
};
struct GridFrame { // what Frame and KeyFrame share here
    int N = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0, mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0, mfGridElementWidthInv = 0, mfGridElementHeightInv = 0, mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<bool> KeysStatic;
    cv::Mat mDescriptors;
    std::vector<MapPoint *> mvpMapPoints;
};
class Frame : public GridFrame {
  public:
    cv::Mat mTcw;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel = -1, const int maxLevel = -1) const;
};
class KeyFrame : public GridFrame {
  public:
    int mnGridCols = FRAME_GRID_COLS, mnGridRows = FRAME_GRID_ROWS;
    std::vector<std::vector<std::vector<size_t>>> mGrid;
    cv::Mat Rcw, tcw;
    std::vector<std::pair<int, size_t>> queried; // (map point being fused, the key point GetMapPoint was asked for): Fuse asks once per fused map point, with its bestIdx
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::set<MapPoint *> GetMapPoints() { std::set<MapPoint *> s; for (MapPoint *p : mvpMapPoints) if (p && !p->isBad()) s.insert(p); return s; }
    MapPoint *GetMapPoint(const size_t &idx) { queried.push_back(std::make_pair(MapPoint::current() ? MapPoint::current()->index : -1, idx)); return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r) const;
    bool IsInImage(const float &x, const float &y) const;
};
class ORBmatcher {
  public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b);
    int SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const std::set<MapPoint *> &sAlreadyFound, const float th, const int ORBdist);
    int SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const std::vector<MapPoint *> &vpPoints, std::vector<MapPoint *> &vpMatched, int th);
    int SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches12, const float &s12, const cv::Mat &R12, const cv::Mat &t12, const float th);
    int Fuse(KeyFrame *pKF, cv::Mat Scw, const std::vector<MapPoint *> &vpPoints, float th, std::vector<MapPoint *> &vpReplacePoint);
    static const int TH_LOW, TH_HIGH, HISTO_LENGTH;
  protected:
    void ComputeThreeMaxima(std::vector<int> *histo, const int L, int &ind1, int &ind2, int &ind3);
    float mfNNratio;
    bool mbCheckOrientation;
};

#include "ref_sim3_extracted.inc"

} // namespace ORB_SLAM2

namespace {
using namespace ORB_SLAM2;
struct FrameIn { int N; const float *x, *y, *angle; const int *octave; const unsigned char *desc, *dynamic /* nullable: !KeysStatic */; float minX, maxX, minY, maxY; };
struct PointsIn { int n; const float *world_pos, *normal /* nullable */, *min_distance, *max_distance; const unsigned char *skip, *desc; };
struct CamIn { float fx, fy, cx, cy, log_sf; const float *scale_factors; int n_levels; };

cv::Mat mat(int r, int c, const float *v) { cv::Mat m(r, c, CV_32F); for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.at<float>(i, j) = v[i * c + j]; return m; }
// AssignFeaturesToGrid / PosInGrid (Frame.cc:303-318, :525-535; KeyFrame copies the Frame's grid): our text -- the window functions that read the grid are the reference's
template <class G> void fill(GridFrame &F, const FrameIn &I, const CamIn &C, G &&cell) {
    F.N = I.N; F.fx = C.fx; F.fy = C.fy; F.cx = C.cx; F.cy = C.cy; F.mnMinX = I.minX; F.mnMaxX = I.maxX; F.mnMinY = I.minY; F.mnMaxY = I.maxY; F.mfLogScaleFactor = C.log_sf;
    F.mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(F.mnMaxX - F.mnMinX);
    F.mfGridElementHeightInv = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(F.mnMaxY - F.mnMinY);
    F.mvScaleFactors.assign(C.scale_factors, C.scale_factors + C.n_levels);
    F.mDescriptors = cv::Mat(I.N, 32, CV_8U);
    if (I.N) memcpy(F.mDescriptors.data, I.desc, (size_t)I.N * 32);
    F.mvpMapPoints.assign((size_t)I.N, nullptr);
    if (I.dynamic) { F.KeysStatic.resize((size_t)I.N); for (int i = 0; i < I.N; i++) F.KeysStatic[i] = !I.dynamic[i]; }
    for (int i = 0; i < I.N; i++) {
        F.mvKeysUn.push_back(cv::KeyPoint(I.x[i], I.y[i], 31.f, I.angle[i], 0.f, I.octave[i]));
        const int px = (int)std::round((I.x[i] - F.mnMinX) * F.mfGridElementWidthInv), py = (int)std::round((I.y[i] - F.mnMinY) * F.mfGridElementHeightInv);
        if (px < 0 || px >= FRAME_GRID_COLS || py < 0 || py >= FRAME_GRID_ROWS) continue;
        cell(px, py).push_back((size_t)i);
    }
}
void fill(KeyFrame &K, const FrameIn &I, const CamIn &C) {
    K.mGrid.assign(FRAME_GRID_COLS, std::vector<std::vector<size_t>>(FRAME_GRID_ROWS));
    fill(K, I, C, [&](int px, int py) -> std::vector<size_t> & { return K.mGrid[px][py]; });
}
void fill(Frame &F, const FrameIn &I, const CamIn &C) { fill(F, I, C, [&](int px, int py) -> std::vector<size_t> & { return F.mGrid[px][py]; }); }
// the map points of a list; skip_as_null: a skipped point is a NULL entry (the lists that come from GetMapPointMatches), otherwise a bad one
std::vector<MapPoint *> points(const PointsIn &P, std::vector<std::unique_ptr<MapPoint>> &own, bool skip_as_null) {
    std::vector<MapPoint *> v((size_t)P.n, nullptr);
    for (int i = 0; i < P.n; i++) {
        if (P.skip[i] && skip_as_null) continue;
        own.emplace_back(new MapPoint());
        MapPoint *p = own.back().get();
        p->index = i; p->bad = P.skip[i] != 0;
        p->mWorldPos = mat(3, 1, P.world_pos + 3 * i);
        if (P.normal) p->mNormalVector = mat(3, 1, P.normal + 3 * i);
        p->mDescriptor = cv::Mat(1, 32, CV_8U); memcpy(p->mDescriptor.data, P.desc + 32 * (size_t)i, 32);
        p->mfMinDistance = P.min_distance[i]; p->mfMaxDistance = P.max_distance[i];
        v[i] = p;
    }
    return v;
}
} // namespace

extern "C" {
// :309-427.  pre_matched[N]: vpMatched[idx] != NULL on entry.  train_match[N]: the index into vpPoints that vpMatched[idx] holds afterwards, -1 none or from before.
int pin_search_by_projection_sim3(const FrameIn *KF, const CamIn *C, const float *Scw16, const PointsIn *P, const unsigned char *pre_matched, int th, int *train_match) {
    KeyFrame K; fill(K, *KF, *C);
    std::vector<std::unique_ptr<MapPoint>> own;
    std::vector<MapPoint *> vpPoints = points(*P, own, false);
    MapPoint before; before.index = -1;
    std::vector<MapPoint *> vpMatched((size_t)K.N, nullptr);
    for (int i = 0; i < K.N; i++) if (pre_matched && pre_matched[i]) vpMatched[i] = &before;
    ORBmatcher m(0.75f, true);
    const int n = m.SearchByProjection(&K, mat(4, 4, Scw16), vpPoints, vpMatched, th);
    for (int i = 0; i < K.N; i++) train_match[i] = vpMatched[i] ? vpMatched[i]->index : -1;
    return n;
}
// :1010-1139.  fused_mp / fused_idx (capacity P->n): per fused map point, in order, its index and the key point GetMapPoint was asked for (= bestIdx); *n_rec of them.
int pin_fuse_sim3(const FrameIn *KF, const CamIn *C, const float *Scw16, const PointsIn *P, float th, int *fused_mp, int *fused_idx, int *n_rec) {
    KeyFrame K; fill(K, *KF, *C);
    std::vector<std::unique_ptr<MapPoint>> own;
    std::vector<MapPoint *> vpPoints = points(*P, own, false);
    std::vector<MapPoint *> vpReplacePoint((size_t)P->n, nullptr);
    ORBmatcher m(0.75f, true);
    const int n = m.Fuse(&K, mat(4, 4, Scw16), vpPoints, th, vpReplacePoint);
    *n_rec = (int)K.queried.size();
    for (size_t k = 0; k < K.queried.size() && (int)k < P->n; k++) { fused_mp[k] = K.queried[k].first; fused_idx[k] = (int)K.queried[k].second; }
    return n;
}
// :1141-1371.  matches12[N1]: the key point of KF2 whose map point vpMatches12[i1] holds afterwards, -1 none.
int pin_search_by_sim3(const FrameIn *KF1, const FrameIn *KF2, const CamIn *C, const float *R1w, const float *t1w, const float *R2w, const float *t2w, float s12, const float *R12,
                       const float *t12, const PointsIn *P1, const PointsIn *P2, float th, int *matches12) {
    KeyFrame K1, K2; fill(K1, *KF1, *C); fill(K2, *KF2, *C);
    K1.Rcw = mat(3, 3, R1w); K1.tcw = mat(3, 1, t1w); K2.Rcw = mat(3, 3, R2w); K2.tcw = mat(3, 1, t2w);
    std::vector<std::unique_ptr<MapPoint>> own;
    K1.mvpMapPoints = points(*P1, own, true); K2.mvpMapPoints = points(*P2, own, true);
    std::vector<MapPoint *> vpMatches12((size_t)K1.N, nullptr);
    ORBmatcher m(0.75f, true);
    const int n = m.SearchBySim3(&K1, &K2, vpMatches12, s12, mat(3, 3, R12), mat(3, 1, t12), th);
    for (int i = 0; i < K1.N; i++) matches12[i] = vpMatches12[i] ? vpMatches12[i]->index : -1;
    return n;
}
// :1727-1858.  pre_matched[N]: CurrentFrame.mvpMapPoints[i2] != NULL on entry.  train_match[N]: the index of pKF's map point the key point holds afterwards.
int pin_search_by_projection_reloc(const FrameIn *CUR, const CamIn *C, const float *Tcw16, const PointsIn *P, const float *kf_angle, const unsigned char *pre_matched, float th, int orb_dist,
                                   int check_orientation, int *train_match) {
    static Frame F; F = Frame(); // (the grid is a large array: not on the stack)
    fill(F, *CUR, *C);
    F.mTcw = mat(4, 4, Tcw16);
    KeyFrame K;
    std::vector<std::unique_ptr<MapPoint>> own;
    K.mvpMapPoints = points(*P, own, true);
    for (int i = 0; i < P->n; i++) K.mvKeysUn.push_back(cv::KeyPoint(0.f, 0.f, 31.f, kf_angle[i]));
    MapPoint before; before.index = -1;
    for (int i = 0; i < F.N; i++) if (pre_matched && pre_matched[i]) F.mvpMapPoints[i] = &before;
    ORBmatcher m(0.75f, check_orientation != 0);
    const int n = m.SearchByProjection(F, &K, std::set<MapPoint *>(), th, orb_dist);
    for (int i = 0; i < F.N; i++) train_match[i] = F.mvpMapPoints[i] ? F.mvpMapPoints[i]->index : -1;
    return n;
}
}
