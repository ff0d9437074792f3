// TEST INFRASTRUCTURE: stand-ins for the SLAM classes that the reference's TrackLocalMap functions touch -- Frame::isInFrustum (orb_object_slam/src/Frame.cc:346-402) and
// Frame::GetFeaturesInArea, Tracking::SearchLocalPoints / UpdateLocalPoints / UpdateLocalKeyFrames (Tracking.cc:2673-2728, :2740-2764, :2766-2874),
// ORBmatcher::SearchByProjection(F, vpMapPoints, th), RadiusByViewingCos, Fuse(pKF, vpMapPoints, th) and DescriptorDistance, MapPoint::PredictScale with the two distance getters,
// KeyFrame::GetFeaturesInArea / IsInImage.  tests/test_track_local_map_restatement_pins.py cuts those functions out of the reference at test time into a temporary directory
// (ref_track_local_map_extracted.inc), compiles this file around them there and runs them next to tests/track_local_map_restatement.py on the same inputs.  The classes carry just
// the members those functions read, under the reference's names; every statement of the functions is the reference's.
// The key frames of a graph live in ONE array: the pointer order of the reference's std::map<KeyFrame *, int> and std::set<KeyFrame *> is then their index order.
#include <cassert>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <vector>

#include "cvshim.hpp"

// ---- float matrices the way cv::MatExpr evaluates them: A * B + C is one gemm with double accumulation and a single rounding to float; Mat - Mat is float; cv::norm and
// Mat::dot (cvshim.hpp) accumulate in double
namespace cv {
struct MulExpr {
    Mat a, b;
    Mat eval(const Mat *c) const {
        Mat r(a.rows, b.cols, CV_32F);
        for (int i = 0; i < a.rows; i++) for (int j = 0; j < b.cols; j++) {
            double s = 0;
            for (int k = 0; k < a.cols; k++) s += (double)a.at<float>(i, k) * (double)b.at<float>(k, j);
            r.at<float>(i, j) = (float)(s * 1.0 + (c ? (double)c->at<float>(i, j) * 1.0 : 0.0));
        }
        return r;
    }
    operator Mat() const { return eval(nullptr); }
};
inline MulExpr operator*(const Mat &a, const Mat &b) { return MulExpr{a, b}; }
inline Mat operator+(const MulExpr &e, const Mat &c) { return e.eval(&c); }
inline Mat operator-(const Mat &a, const Mat &b) { Mat r(a.rows, a.cols, CV_32F); for (int i = 0; i < a.rows * a.cols; i++) r.at<float>(i) = a.at<float>(i) - b.at<float>(i); return r; } // CV_32F vectors
inline double norm(const Mat &m) { double s = 0; for (int i = 0; i < m.rows * m.cols; i++) s += (double)m.at<float>(i) * (double)m.at<float>(i); return std::sqrt(s); }
} // namespace cv

namespace ORB_SLAM2 {
using namespace std;
#define FRAME_GRID_ROWS 48 // Frame.h:32-33
#define FRAME_GRID_COLS 64
bool whether_dynamic_object = false; // Parameters.h:38

class KeyFrame;
class MapPoint {
  public:
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    std::mutex mMutexPos;
    bool bad = false, is_dynamic = false;
    int index = -1, nObs = 0, visible = 0;
    bool in_kf = false; // IsInKeyFrame of the one key frame a Fuse call has
    long added_idx = -1;
    std::map<KeyFrame *, size_t> mObservations;
    // what isInFrustum leaves (MapPoint.h:110-118)
    float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackViewCos = 0;
    bool mbTrackInView = false;
    int mnTrackScaleLevel = 0;
    long unsigned int mnTrackReferenceForFrame = 0, mnLastFrameSeen = 0;
    static MapPoint *&current() { static MapPoint *p = nullptr; return p; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { current() = this; return mDescriptor.clone(); }
    bool isBad() { return bad; }
    int Observations() { return nObs; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    void IncreaseVisible(int n = 1) { visible += n; }
    bool IsInKeyFrame(KeyFrame *) { return in_kf; }
    void Replace(MapPoint *) {}
    void AddObservation(KeyFrame *, size_t idx) { added_idx = (long)idx; }
    float GetMinDistanceInvariance();
    float GetMaxDistanceInvariance();
    int PredictScale(const float &currentDist, const float &logScaleFactor);
};
struct GridFrame { // what Frame and KeyFrame share here
    int N = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0, mfGridElementWidthInv = 0, mfGridElementHeightInv = 0, mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2, mvuRight;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<bool> KeysStatic;
    cv::Mat mDescriptors;
    std::vector<MapPoint *> mvpMapPoints;
};
class Frame : public GridFrame {
  public:
    long unsigned int mnId = 1;
    cv::Mat mRcw, mtcw, mOw;
    KeyFrame *mpReferenceKF = nullptr;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
    bool isInFrustum(MapPoint *pMP, float viewingCosLimit);
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel = -1, const int maxLevel = -1) const;
};
class KeyFrame : public GridFrame {
  public:
    int index = -1;
    bool bad = false;
    long unsigned int mnTrackReferenceForFrame = 0;
    int mnGridCols = FRAME_GRID_COLS, mnGridRows = FRAME_GRID_ROWS;
    std::vector<std::vector<std::vector<size_t>>> mGrid;
    cv::Mat Rcw, tcw, Ow;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::set<KeyFrame *> mspChildrens;
    KeyFrame *mpParent = nullptr;
    std::vector<std::pair<int, size_t>> queried; // (map point being fused, the key point GetMapPoint was asked for)
    bool isBad() { return bad; }
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) { // KeyFrame.cc: the first N of the ordered list
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    std::set<KeyFrame *> GetChilds() { return mspChildrens; }
    KeyFrame *GetParent() { return mpParent; }
    MapPoint *GetMapPoint(const size_t &idx) { queried.push_back(std::make_pair(MapPoint::current() ? MapPoint::current()->index : -1, idx)); return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r) const;
    bool IsInImage(const float &x, const float &y) const;
};
class ORBmatcher {
  public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b);
    int SearchByProjection(Frame &F, const std::vector<MapPoint *> &vpMapPoints, const float th = 3);
    int Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, const float th = 3.0);
    static const int TH_LOW, TH_HIGH, HISTO_LENGTH;
  protected:
    float RadiusByViewingCos(const float &viewCos);
    float mfNNratio;
    bool mbCheckOrientation;
};
struct System { enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2 }; };
class Tracking {
  public:
    Frame mCurrentFrame;
    std::vector<KeyFrame *> mvpLocalKeyFrames;
    std::vector<MapPoint *> mvpLocalMapPoints;
    KeyFrame *mpReferenceKF = nullptr;
    int mSensor = System::MONOCULAR;
    long unsigned int mnLastRelocFrameId = 0;
    void SearchLocalPoints();
    void UpdateLocalPoints();
    void UpdateLocalKeyFrames();
};

#include "ref_track_local_map_extracted.inc"

} // namespace ORB_SLAM2

namespace {
using namespace ORB_SLAM2;
struct FrameIn { int N; const float *x, *y, *angle; const int *octave; const unsigned char *desc, *dynamic /* nullable: !KeysStatic */; float minX, maxX, minY, maxY; };
struct PointsIn { int n; const float *world_pos, *normal, *min_distance, *max_distance; const unsigned char *skip, *desc; };
struct CamIn { float fx, fy, cx, cy, bf, log_sf; const float *scale_factors; int n_levels; };

cv::Mat mat(int r, int c, const float *v) { cv::Mat m(r, c, CV_32F); for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.at<float>(i, j) = v[i * c + j]; return m; }
// AssignFeaturesToGrid / PosInGrid (Frame.cc:303-318, :525-535; KeyFrame copies the Frame's grid): our text -- the window functions that read the grid are the reference's
template <class G> void fill(GridFrame &F, const FrameIn &I, const CamIn &C, G &&cell) {
    F.N = I.N; F.fx = C.fx; F.fy = C.fy; F.cx = C.cx; F.cy = C.cy; F.mbf = C.bf; F.mnMinX = I.minX; F.mnMaxX = I.maxX; F.mnMinY = I.minY; F.mnMaxY = I.maxY; F.mfLogScaleFactor = C.log_sf;
    F.mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(F.mnMaxX - F.mnMinX);
    F.mfGridElementHeightInv = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(F.mnMaxY - F.mnMinY);
    F.mvScaleFactors.assign(C.scale_factors, C.scale_factors + C.n_levels);
    F.mDescriptors = cv::Mat(I.N, 32, CV_8U);
    if (I.N) memcpy(F.mDescriptors.data, I.desc, (size_t)I.N * 32);
    F.mvpMapPoints.assign((size_t)I.N, nullptr);
    F.mvuRight.assign((size_t)I.N, -1.0f);
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
MapPoint *point(const PointsIn &P, int i, std::vector<std::unique_ptr<MapPoint>> &own) {
    own.emplace_back(new MapPoint());
    MapPoint *p = own.back().get();
    p->index = i;
    p->mWorldPos = mat(3, 1, P.world_pos + 3 * i); p->mNormalVector = mat(3, 1, P.normal + 3 * i);
    p->mDescriptor = cv::Mat(1, 32, CV_8U); memcpy(p->mDescriptor.data, P.desc + 32 * (size_t)i, 32);
    p->mfMinDistance = P.min_distance[i]; p->mfMaxDistance = P.max_distance[i];
    return p;
}
} // namespace

extern "C" {
// Tracking::SearchLocalPoints on a frame that holds no map point of its own.  skip[i]: the point is bad (the reference `continue`s at :2704).  blocks[i] = Observations() > 0.
// pre_blocked[N]: the key point holds a map point with observations from before.  th_sel: 0 = monocular (th 1), 1 = RGBD (3), 2 = just relocalised (5).
// Out: train_match[N] (index of the local point, -1 none or from before), per point in_view / proj (u, v, uR) / level / view_cos / visible; returns the number of points in view.
int pin_search_local_points(const FrameIn *CUR, const CamIn *C, const float *Rcw, const float *tcw, const float *Ow, const PointsIn *P, const unsigned char *blocks,
                            const unsigned char *pre_blocked, int th_sel, int *train_match, unsigned char *in_view, float *proj, int *level, float *view_cos, int *visible) {
    static Tracking T; T = Tracking(); // (the frame's grid is a large array: not on the stack)
    Frame &F = T.mCurrentFrame;
    fill(F, *CUR, *C);
    F.mnId = 10; F.mRcw = mat(3, 3, Rcw); F.mtcw = mat(3, 1, tcw); F.mOw = mat(3, 1, Ow);
    T.mSensor = th_sel == 1 ? System::RGBD : System::MONOCULAR;
    T.mnLastRelocFrameId = th_sel == 2 ? 9 : 0;
    std::vector<std::unique_ptr<MapPoint>> own;
    for (int i = 0; i < P->n; i++) { MapPoint *p = point(*P, i, own); p->bad = P->skip[i] != 0; p->nObs = blocks[i] ? 2 : 0; T.mvpLocalMapPoints.push_back(p); }
    MapPoint before; before.index = -1; before.nObs = 1; before.is_dynamic = true; // (dynamic: the loop over the frame's own points leaves it alone, :2687)
    for (int i = 0; i < F.N; i++) if (pre_blocked && pre_blocked[i]) F.mvpMapPoints[i] = &before;
    T.SearchLocalPoints();
    int n = 0;
    for (int i = 0; i < P->n; i++) {
        MapPoint *p = T.mvpLocalMapPoints[i];
        in_view[i] = p->mbTrackInView; visible[i] = p->visible; n += p->mbTrackInView;
        proj[3 * i] = p->mTrackProjX; proj[3 * i + 1] = p->mTrackProjY; proj[3 * i + 2] = p->mTrackProjXR; level[i] = p->mnTrackScaleLevel; view_cos[i] = p->mTrackViewCos;
    }
    for (int i = 0; i < F.N; i++) train_match[i] = F.mvpMapPoints[i] ? F.mvpMapPoints[i]->index : -1;
    return n;
}

// Tracking::UpdateLocalPoints over the lists of n_kf key frames; skip[n_points] = isBad.  Returns the length of out.
int pin_update_local_points(int n_kf, const int *kf_off, const int *kf_mp, int n_points, const unsigned char *skip, int *out) {
    static Tracking T; T = Tracking();
    T.mCurrentFrame.mnId = 10;
    std::vector<MapPoint> pts((size_t)n_points);
    for (int i = 0; i < n_points; i++) { pts[i].index = i; pts[i].bad = skip[i] != 0; }
    std::vector<KeyFrame> kfs((size_t)n_kf);
    for (int j = 0; j < n_kf; j++) {
        for (int e = kf_off[j]; e < kf_off[j + 1]; e++) kfs[j].mvpMapPoints.push_back(kf_mp[e] < 0 ? nullptr : &pts[kf_mp[e]]);
        T.mvpLocalKeyFrames.push_back(&kfs[j]);
    }
    T.UpdateLocalPoints();
    for (size_t k = 0; k < T.mvpLocalMapPoints.size(); k++) out[k] = T.mvpLocalMapPoints[k]->index;
    return (int)T.mvpLocalMapPoints.size();
}

// Tracking::UpdateLocalKeyFrames.  Returns the length of local_kf, -1 when mvpLocalKeyFrames was left alone; *kf_max = the index of mpReferenceKF or -1.
int pin_update_local_keyframes(int n_frame, const int *frame_mp, int n_points, const unsigned char *mp_skip, const int *obs_off, const int *obs_kf, int n_kf, const unsigned char *kf_bad,
                               const int *cov_off, const int *cov_kf, const int *child_off, const int *child_kf, const int *parent, int *local_kf, int *kf_max) {
    static Tracking T; T = Tracking();
    T.mCurrentFrame.mnId = 10; T.mCurrentFrame.N = n_frame;
    std::vector<KeyFrame> kfs((size_t)n_kf); // one array: pointer order = index order
    for (int j = 0; j < n_kf; j++) {
        kfs[j].index = j; kfs[j].bad = kf_bad[j] != 0;
        for (int c = cov_off[j]; c < cov_off[j + 1]; c++) kfs[j].mvpOrderedConnectedKeyFrames.push_back(&kfs[cov_kf[c]]);
        for (int c = child_off[j]; c < child_off[j + 1]; c++) kfs[j].mspChildrens.insert(&kfs[child_kf[c]]);
        kfs[j].mpParent = parent[j] < 0 ? nullptr : &kfs[parent[j]];
    }
    std::vector<MapPoint> pts((size_t)n_points);
    for (int i = 0; i < n_points; i++) {
        pts[i].index = i; pts[i].bad = mp_skip[i] != 0;
        for (int o = obs_off[i]; o < obs_off[i + 1]; o++) pts[i].mObservations[&kfs[obs_kf[o]]] = 0;
    }
    for (int i = 0; i < n_frame; i++) T.mCurrentFrame.mvpMapPoints.push_back(frame_mp[i] < 0 ? nullptr : &pts[frame_mp[i]]);
    KeyFrame sentinel; sentinel.index = -7;
    T.mvpLocalKeyFrames.push_back(&sentinel);
    T.UpdateLocalKeyFrames();
    *kf_max = T.mpReferenceKF ? T.mpReferenceKF->index : -1;
    if (T.mvpLocalKeyFrames.size() == 1 && T.mvpLocalKeyFrames[0] == &sentinel) return -1;
    for (size_t k = 0; k < T.mvpLocalKeyFrames.size(); k++) local_kf[k] = T.mvpLocalKeyFrames[k]->index;
    return (int)T.mvpLocalKeyFrames.size();
}

// ORBmatcher::Fuse(pKF, vpMapPoints, th).  u_right[N], inv_level_sigma2[n_levels].  fused_mp / fused_idx (capacity P->n): per fused map point, in order, its index and the key point
// GetMapPoint was asked for (= bestIdx); *n_rec of them.  Returns nFused.
int pin_fuse_map(const FrameIn *KF, const CamIn *C, const float *Rcw, const float *tcw, const float *Ow, const float *u_right, const float *inv_level_sigma2, const PointsIn *P, float th,
                 int *fused_mp, int *fused_idx, int *n_rec) {
    KeyFrame K; fill(K, *KF, *C);
    K.Rcw = mat(3, 3, Rcw); K.tcw = mat(3, 1, tcw); K.Ow = mat(3, 1, Ow);
    K.mvuRight.assign(u_right, u_right + K.N);
    K.mvInvLevelSigma2.assign(inv_level_sigma2, inv_level_sigma2 + C->n_levels);
    std::vector<std::unique_ptr<MapPoint>> own;
    std::vector<MapPoint *> v;
    for (int i = 0; i < P->n; i++) { MapPoint *p = point(*P, i, own); p->bad = P->skip[i] != 0; v.push_back(p); }
    ORBmatcher m(0.6f, true);
    const int n = m.Fuse(&K, v, th);
    *n_rec = (int)K.queried.size();
    for (size_t k = 0; k < K.queried.size() && (int)k < P->n; k++) { fused_mp[k] = K.queried[k].first; fused_idx[k] = (int)K.queried[k].second; }
    return n;
}
}
