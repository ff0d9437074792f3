// TEST INFRASTRUCTURE: stand-ins for everything the dynamic-point triangulation of Tracking::CreateNewKeyFrame (orb_object_slam/src/Tracking.cc:2144-2244) and the three
// object-depth initialisations (Tracking.cc:876-898, :2339-2424, LocalMapping.cc:574-652) touch.  tests/test_object_points_restatement_pins.py cuts those blocks out of the
// reference at test time into a temporary directory -- between anchor lines where they sit inside CreateNewKeyFrame --, with random_unique / random_unique2,
// Frame::UnprojectDepth, KeyFrame::UnprojectDepth, KeyFrame::PosInGrid and five Converter functions, compiles this file around them there and runs them next to
// tests/object_points_restatement.py on the same patterns.  g2o::SE3Quat is the reference's own (Thirdparty/g2o/g2o/types/se3quat.h, found through the test's include path) on
// the Eigen stand-in of oracle/ref_shim/eigen_full.  Every statement of the blocks is the reference's.
//
// cv::Mat is the float matrix with views of tests/cpp/ref_local_mapping_loop_standins.cpp, not oracle/ref_shim/cvshim.hpp: `A.row(0) = <expression>` has to write through the
// view, which needs Mat::operator=(const MatExpr &), and cvshim's Mat has none.  The expression forms, as OpenCV 2.4 - 3.x evaluates them on CV_32F:
//   A * B (+ C)          one gemm: double accumulation over k ascending, one rounding
//   s * M - N            cv::addWeighted(M, s, N, -1, 0): float(M * float(s)) + float(N * -1.f) + 0.f per element, in float, no fused multiply-add
//   M / s                every element times 1.0 / s in double, one rounding (the library's stated definition of the cv::MatExpr scale)
// cv::SVD::compute is a one-sided Jacobi in FLOAT: the distance it puts between the reference and the restatement's stated f64 Jacobi is what the test measures.
// rand() replays the pattern's draws; srand and time do nothing.
#include <cmath>
#include <cstring>
#include <iostream>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "Thirdparty/g2o/g2o/types/se3quat.h"

#define CV_32F 5
namespace cv {
struct Expr { int rows = 0, cols = 0; std::vector<float> v; }; // an evaluated expression
class Mat {
  public:
    int rows = 0, cols = 0, step = 0, off = 0;
    std::shared_ptr<std::vector<float>> buf;
    Mat() {}
    Mat(int r, int c, int) { create(r, c); }
    Mat(const Expr &e) { *this = e; }
    void create(int r, int c) { rows = r; cols = c; step = c; off = 0; buf = std::make_shared<std::vector<float>>((size_t)r * c, 0.f); }
    Mat &operator=(const Expr &e) { // cv::Mat::operator=(const MatExpr &): into the existing buffer where the size fits
        if (!buf || rows != e.rows || cols != e.cols) create(e.rows, e.cols);
        for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) el(r, c) = e.v[(size_t)r * cols + c];
        return *this;
    }
    float &el(int r, int c) { return (*buf)[(size_t)off + (size_t)r * step + c]; }
    float el(int r, int c) const { return (*buf)[(size_t)off + (size_t)r * step + c]; }
    template <class T> T &at(int i) { return cols == 1 ? el(i, 0) : el(0, i); }
    template <class T> const T &at(int i) const { return (*buf)[(size_t)off + (cols == 1 ? (size_t)i * step : (size_t)i)]; }
    template <class T> T &at(int r, int c) { return el(r, c); }
    bool empty() const { return !buf || rows == 0 || cols == 0; }
    Mat view(int r0, int c0, int r, int c) const { Mat m; m.rows = r; m.cols = c; m.step = step; m.off = off + r0 * step + c0; m.buf = buf; return m; }
    Mat row(int r) const { return view(r, 0, 1, cols); }
    Mat col(int c) const { return view(0, c, rows, 1); }
    Mat rowRange(int a, int b) const { return view(a, 0, b - a, cols); }
    Mat colRange(int a, int b) const { return view(0, a, rows, b - a); }
    Expr value() const { Expr e; e.rows = rows; e.cols = cols; for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) e.v.push_back(el(r, c)); return e; }
    Mat clone() const { return empty() ? Mat() : Mat(value()); }
    Mat t() const { Expr e; e.rows = cols; e.cols = rows; for (int c = 0; c < cols; c++) for (int r = 0; r < rows; r++) e.v.push_back(el(r, c)); return Mat(e); }
};
template <class T> struct Mat_ : Mat { // only (cv::Mat_<float>(3, 1) << a, b, c)
    Mat_(int r, int c) : Mat(r, c, CV_32F) {}
};
struct CommaInit {
    Mat m; int i = 0;
    CommaInit &operator,(double v) { m.el(i / m.cols, i % m.cols) = (float)v; i++; return *this; }
    operator Mat() const { return m; }
};
template <class T> CommaInit operator<<(const Mat_<T> &m, double v) { CommaInit c; c.m = m; c.m.el(0, 0) = (float)v; c.i = 1; return c; }

struct MulExpr { Mat a, b; operator Mat() const; };
inline Expr gemm(const Mat &a, const Mat &b, const Mat *c) {
    Expr e; e.rows = a.rows; e.cols = b.cols;
    for (int i = 0; i < a.rows; i++) for (int j = 0; j < b.cols; j++) {
        double s = 0;
        for (int k = 0; k < a.cols; k++) s += (double)a.el(i, k) * (double)b.el(k, j);
        e.v.push_back((float)(s * 1.0 + (c ? (double)c->el(i, j) * 1.0 : 0.0)));
    }
    return e;
}
inline MulExpr::operator Mat() const { return Mat(gemm(a, b, nullptr)); }
inline MulExpr operator*(const Mat &a, const Mat &b) { return MulExpr{a, b}; }
inline Mat operator+(const MulExpr &e, const Mat &c) { return Mat(gemm(e.a, e.b, &c)); }
struct ScaledMat { Mat m; double s; };
inline ScaledMat operator*(double s, const Mat &m) { return ScaledMat{m, s}; }
inline Expr operator-(const ScaledMat &a, const Mat &b) { // addWeighted(a.m, a.s, b, -1, 0) on CV_32F
    Expr e; e.rows = b.rows; e.cols = b.cols;
    const float alpha = (float)a.s, beta = -1.f, gamma = 0.f;
    for (int r = 0; r < b.rows; r++) for (int c = 0; c < b.cols; c++) {
        const float t0 = a.m.el(r, c) * alpha, t1 = b.el(r, c) * beta;
        e.v.push_back(t0 + t1 + gamma);
    }
    return e;
}
inline Expr operator/(const Mat &m, double s) { Expr e; e.rows = m.rows; e.cols = m.cols; const double inv = 1.0 / s; for (int r = 0; r < m.rows; r++) for (int c = 0; c < m.cols; c++) e.v.push_back((float)((double)m.el(r, c) * inv)); return e; }

struct Point2f { float x = 0, y = 0; };
struct KeyPoint { Point2f pt; int octave = 0; };

struct SVD {
    enum { MODIFY_A = 1, FULL_UV = 4 };
    // vt: the right singular vectors as rows, singular values descending -- a one-sided Jacobi on the columns of A in float
    static void compute(const Mat &A, Mat &w, Mat &u, Mat &vt, int) {
        const int n = 4;
        float W[4][4], V[4][4];
        for (int r = 0; r < n; r++) for (int c = 0; c < n; c++) { W[r][c] = A.el(r, c); V[r][c] = r == c ? 1.f : 0.f; }
        for (int sweep = 0; sweep < 30; sweep++) {
            bool rotated = false;
            for (int p = 0; p < n - 1; p++) for (int q = p + 1; q < n; q++) {
                float alpha = 0, beta = 0, gamma = 0;
                for (int r = 0; r < n; r++) { alpha += W[r][p] * W[r][p]; beta += W[r][q] * W[r][q]; gamma += W[r][p] * W[r][q]; }
                if (std::fabs(gamma) <= 1.1920929e-7f * std::sqrt(alpha * beta)) continue;
                rotated = true;
                const float zeta = (beta - alpha) / (2.f * gamma);
                const float t = (zeta < 0 ? -1.f : 1.f) / (std::fabs(zeta) + std::sqrt(1.f + zeta * zeta));
                const float c = 1.f / std::sqrt(1.f + t * t), s = c * t;
                for (int r = 0; r < n; r++) {
                    const float wp = W[r][p], wq = W[r][q]; W[r][p] = c * wp - s * wq; W[r][q] = s * wp + c * wq;
                    const float vp = V[r][p], vq = V[r][q]; V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
                }
            }
            if (!rotated) break;
        }
        float sv[4]; int order[4] = {0, 1, 2, 3};
        for (int k = 0; k < n; k++) { float s = 0; for (int r = 0; r < n; r++) s += W[r][k] * W[r][k]; sv[k] = std::sqrt(s); }
        for (int i = 0; i < n; i++) for (int j = i + 1; j < n; j++) if (sv[order[j]] > sv[order[i]]) std::swap(order[i], order[j]);
        w.create(n, 1); vt.create(n, n); u.create(n, n);
        for (int i = 0; i < n; i++) { w.el(i, 0) = sv[order[i]]; for (int r = 0; r < n; r++) vt.el(i, r) = V[r][order[i]]; }
    }
};
} // namespace cv

namespace g2o {
struct cuboid { SE3Quat pose; };
} // namespace g2o

#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64
static std::vector<std::pair<int, std::string>> g_errors; // (loop index, text) of every ROS_ERROR_STREAM
#define ROS_ERROR_STREAM(x) do { std::ostringstream o__; o__ << x; g_errors.push_back(std::make_pair((int)i, o__.str())); } while (0)

namespace ORB_SLAM2 {
using namespace std;
static std::ostringstream cout; // the blocks print their counts
bool use_dynamic_klt_features = false, use_truth_trackid = false, triangulate_dynamic_pts = true, whether_detect_object = true, mono_firstframe_Obj_depth_init = true,
     associate_point_with_object = true, mono_allframe_Obj_depth_init = true, whether_dynamic_object = false;

static const int *g_draws = nullptr;
static int g_n_draws = 0, g_draw_pos = 0;
inline void srand(unsigned) {}
inline unsigned time(void *) { return 0; }
inline int rand() { if (g_draw_pos >= g_n_draws) throw std::runtime_error("out of draws"); return g_draws[g_draw_pos++]; }

class Converter {
  public:
    static cv::Mat toCvMat(const g2o::SE3Quat &SE3);
    static cv::Mat toCvMat(const Eigen::Matrix<double, 4, 4> &m);
    static cv::Mat toCvMat(const Eigen::Matrix<double, 3, 1> &m);
    static Eigen::Matrix<double, 3, 1> toVector3d(const cv::Mat &cvVector);
    static Eigen::Matrix<float, 3, 1> toVector3f(const cv::Mat &cvVector);
};

class KeyFrame;
class MapPoint;
class Map {
  public:
    std::vector<std::pair<MapPoint *, int>> created; // (point, key point) in creation order, as SetupSimpleMapPoints sees them
};
struct CubeMeas { Eigen::Vector3d t; Eigen::Vector3d translation() const { return t; } };
class MapObject {
  public:
    bool already_associated = false;
    MapObject *associated_landmark = nullptr;
    std::map<KeyFrame *, std::pair<g2o::cuboid, bool>> allDynamicPoses;
    g2o::cuboid pose;
    int truth_tracklet_id = 0;
    CubeMeas cube_meas;
    g2o::cuboid GetWorldPos() { return pose; }
};
class MapPoint {
  public:
    cv::Mat pos, PosToObj;
    bool is_dynamic = false, is_triangulated = false;
    std::map<KeyFrame *, int> index_in;
    MapPoint() {}
    MapPoint(const cv::Mat &Pos, KeyFrame *, Map *) : pos(Pos.clone()) {}
    int GetIndexInKeyFrame(KeyFrame *pKF) { auto it = index_in.find(pKF); return it == index_in.end() ? -1 : it->second; }
    Eigen::Vector3f GetWorldPosVec() { return Converter::toVector3f(pos); }
    void SetWorldPos(const cv::Mat &p) { pos = p.clone(); }
};
class KeyFrame {
  public:
    float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0;
    int mnMinX = 0, mnMinY = 0; // KeyFrame.h:229-230: const int, initialised from Frame's floats
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn, mvKeysHarris;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<int> keypoint_associate_objectID, keypoint_associate_objectID_harris;
    std::vector<MapObject *> local_cuboids;
    cv::Mat Tcw, Twc;
    std::mutex mMutexPose;
    Map *map = nullptr;
    cv::Mat GetPose() { return Tcw.clone(); }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    void SetupSimpleMapPoints(MapPoint *pNewMP, int point_ind) { mvpMapPoints[point_ind] = pNewMP; map->created.push_back(std::make_pair(pNewMP, point_ind)); }
    cv::Mat UnprojectDepth(int i, float depth);
    bool PosInGrid(const cv::KeyPoint &kp, int &posX, int &posY);
};
class Frame {
  public:
    int N = 0;
    float cx = 0, cy = 0, invfx = 0, invfy = 0;
    std::vector<cv::KeyPoint> mvKeysUn, mvKeysHarris;
    std::vector<MapPoint *> mvpMapPoints, mvpMapPointsHarris;
    std::vector<bool> mvbOutlier;
    std::vector<int> keypoint_associate_objectID_harris;
    cv::Mat mRwc, mOw;
    cv::Mat UnprojectDepth(const int &i, float depth);
};

#include "ref_object_points_functions.inc" // random_unique, random_unique2, Frame / KeyFrame::UnprojectDepth, KeyFrame::PosInGrid, the Converter functions

class Tracking {
  public:
    Frame mCurrentFrame;
    KeyFrame *mpLastKeyFrame = nullptr;
    Map *mpMap = nullptr;
    void TriangulateDynamicPoints(KeyFrame *pKF) { // Tracking.cc:2135, then :2144-2244
        KeyFrame *mpCurrentKeyFrame = pKF;
#include "ref_object_points_triangulate.inc"
    }
    void MonoObjDepthInitialization(KeyFrame *pKFini) { // :876-898
#include "ref_object_points_first_frame.inc"
    }
    void CreateNewKeyFrameObjectDepth(KeyFrame *pKF, int *n_candidates, int *raw, int *max_init, std::vector<int> *before, std::vector<int> *after) { // :2135-2141, then :2341-2423
        KeyFrame *mpCurrentKeyFrame = pKF;
        const vector<MapPoint *> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
        double total_feature_pts = vpMapPointMatches.size();
        double raw_depth_pts = 0;
        double plane_object_initialized_pts = 0;
        {
#include "ref_object_points_tracking.inc"
            *n_candidates = (int)has_object_depth_pixel_inds.size(); *raw = (int)raw_depth_pts; *max_init = whether_actually_planeobj_init_pt ? max_initialize_pts : -1;
            *after = has_object_depth_pixel_inds;
        }
        (void)plane_object_initialized_pts; (void)before;
    }
};
class LocalMapping {
  public:
    KeyFrame *mpCurrentKeyFrame = nullptr;
    Map *mpMap = nullptr;
    std::list<MapPoint *> mlpRecentAddedMapPoints;
    void CreateNewMapPointsTail() { // LocalMapping.cc:574-652
#include "ref_object_points_local_mapping.inc"
    }
};

} // namespace ORB_SLAM2

extern "C" {
using namespace ORB_SLAM2;

static g2o::SE3Quat se3(const double *p) { // the seven numbers as they are: the constructor from a quaternion would normalise them once more
    g2o::SE3Quat T;
    T.setRotation(Eigen::Quaterniond(p[6], p[3], p[4], p[5]));
    T.setTranslation(Eigen::Vector3d(p[0], p[1], p[2]));
    return T;
}
static cv::Mat mat34(const float *T, bool four) {
    cv::Mat m(four ? 4 : 3, 4, CV_32F);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) m.el(r, c) = T[r * 4 + c];
    if (four) m.el(3, 3) = 1.f;
    return m;
}

// Tracking.cc:2144-2244 for one key-frame pair.  already_associated[row] of the last key frame's table: the pose comes from allDynamicPoses[mpLastKeyFrame] (and GetWorldPos()
// holds another one).  Outputs per point: triangulated, PosToObj, and the ROS_ERROR_STREAM the point raised (0 none, 1 no observation, 2 tracklet).
int pin_triangulate(int n, const float *Tcw_last, const float *Tcw_now, const float *K4, int n_last, const double *pose_last, int n_now, const double *pose_now,
                    const int *tracklet_last, const int *tracklet_now, const unsigned char *already_associated, int harris, const float *kp1, const float *kp2, const int *obj_last,
                    const int *obj_now, const int *idx_last, const float *world_pos, unsigned char *triangulated, float *pos_to_obj, int *error) {
    use_dynamic_klt_features = harris != 0; use_truth_trackid = tracklet_last != nullptr;
    g_errors.clear();
    KeyFrame last, now;
    now.Tcw = mat34(Tcw_now, true); last.Tcw = mat34(Tcw_last, true);
    now.cx = K4[2]; now.cy = K4[3]; now.invfx = 1.0f / K4[0]; now.invfy = 1.0f / K4[1];
    std::vector<MapObject> ol((size_t)n_last), on((size_t)n_now), landmarks((size_t)n_last);
    for (int k = 0; k < n_last; k++) {
        ol[k].truth_tracklet_id = tracklet_last ? tracklet_last[k] : 0;
        if (already_associated && already_associated[k]) {
            ol[k].already_associated = true; ol[k].associated_landmark = &landmarks[k];
            landmarks[k].allDynamicPoses[&last] = std::make_pair(g2o::cuboid{se3(pose_last + 7 * k)}, true);
            ol[k].pose.pose = se3(pose_now + 7 * (k % (n_now ? n_now : 1))); // something else: it must not be read
        } else
            ol[k].pose.pose = se3(pose_last + 7 * k);
        last.local_cuboids.push_back(&ol[k]);
    }
    for (int k = 0; k < n_now; k++) { on[k].pose.pose = se3(pose_now + 7 * k); on[k].truth_tracklet_id = tracklet_now ? tracklet_now[k] : 0; now.local_cuboids.push_back(&on[k]); }
    // the last key frame's key points: one per point that has an observation there, at idx_last
    int n_last_keys = 0;
    for (int i = 0; i < n; i++) if (idx_last[i] + 1 > n_last_keys) n_last_keys = idx_last[i] + 1;
    std::vector<cv::KeyPoint> keys_last((size_t)n_last_keys), keys_now((size_t)n);
    std::vector<int> ids_last((size_t)n_last_keys, 0), ids_now((size_t)n, 0);
    std::vector<MapPoint> pts((size_t)n);
    Tracking tr;
    tr.mpLastKeyFrame = &last;
    now.mvpMapPoints.assign((size_t)n, nullptr);
    for (int i = 0; i < n; i++) {
        pts[i].is_dynamic = true;
        pts[i].pos = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) pts[i].pos.el(k, 0) = world_pos[3 * i + k];
        if (idx_last[i] >= 0) {
            pts[i].index_in[&last] = idx_last[i];
            keys_last[idx_last[i]].pt.x = kp1[2 * i]; keys_last[idx_last[i]].pt.y = kp1[2 * i + 1];
            ids_last[idx_last[i]] = obj_last[i];
        }
        keys_now[i].pt.x = kp2[2 * i]; keys_now[i].pt.y = kp2[2 * i + 1];
        ids_now[i] = obj_now[i];
        now.mvpMapPoints[i] = &pts[i];
    }
    if (harris) {
        last.mvKeysHarris = keys_last; last.keypoint_associate_objectID_harris = ids_last;
        tr.mCurrentFrame.mvKeysHarris = keys_now; tr.mCurrentFrame.keypoint_associate_objectID_harris = ids_now; tr.mCurrentFrame.mvpMapPointsHarris = now.mvpMapPoints;
    } else {
        last.mvKeysUn = keys_last; last.keypoint_associate_objectID = ids_last;
        now.mvKeysUn = keys_now; now.keypoint_associate_objectID = ids_now;
    }
    tr.TriangulateDynamicPoints(&now);
    for (int i = 0; i < n; i++) {
        triangulated[i] = pts[i].is_triangulated; error[i] = 0;
        for (int k = 0; k < 3; k++) pos_to_obj[3 * i + k] = pts[i].is_triangulated ? pts[i].PosToObj.el(k, 0) : 0.f;
    }
    for (const auto &e : g_errors) error[e.first] = e.second.find("not added yet") != std::string::npos ? 1 : (e.second.find("tracklet") != std::string::npos ? 2 : 9);
    return 0;
}

// the three object-depth initialisations for one key frame.  keys: x y octave per key point.  Outputs: the candidate list after the draws (modes 1, 2), the counts, the
// created points' key points in creation order with their positions.  Returns the number of created points, -1 when the draws ran out.
int pin_object_depth(int mode, int N, const float *xy, const int *octave, const unsigned char *has_mp, const int *object_id, int n_cub, const float *cub_depth, const float *K4,
                     const float *bounds, const float *Twc, int n_draws, const int *draws, int *n_candidates, int *raw, int *max_init, int *shuffled, int *new_idx, float *new_x3D) {
    g_draws = draws; g_n_draws = n_draws; g_draw_pos = 0;
    whether_dynamic_object = mode == 1;
    Map map;
    KeyFrame kf;
    kf.map = &map;
    kf.cx = K4[2]; kf.cy = K4[3]; kf.invfx = 1.0f / K4[0]; kf.invfy = 1.0f / K4[1];
    kf.Twc = mat34(Twc, true);
    std::vector<MapObject> cubs((size_t)n_cub);
    for (int k = 0; k < n_cub; k++) { cubs[k].cube_meas.t = Eigen::Vector3d(0.0, 0.0, (double)cub_depth[k]); kf.local_cuboids.push_back(&cubs[k]); }
    std::vector<cv::KeyPoint> keys((size_t)N);
    for (int i = 0; i < N; i++) { keys[i].pt.x = xy[2 * i]; keys[i].pt.y = xy[2 * i + 1]; keys[i].octave = octave[i]; }
    kf.keypoint_associate_objectID.assign(object_id, object_id + N);
    MapPoint existing;
    kf.mvpMapPoints.assign((size_t)N, nullptr);
    std::vector<int> after;
    *n_candidates = *raw = 0; *max_init = -1;
    try {
        if (mode == 0) {
            Tracking tr;
            tr.mpMap = &map;
            tr.mCurrentFrame.N = N; tr.mCurrentFrame.mvKeysUn = keys;
            tr.mCurrentFrame.cx = kf.cx; tr.mCurrentFrame.cy = kf.cy; tr.mCurrentFrame.invfx = kf.invfx; tr.mCurrentFrame.invfy = kf.invfy;
            tr.mCurrentFrame.mRwc = kf.Twc.rowRange(0, 3).colRange(0, 3).clone(); tr.mCurrentFrame.mOw = kf.Twc.rowRange(0, 3).col(3).clone();
            tr.mCurrentFrame.mvpMapPoints.assign((size_t)N, nullptr); tr.mCurrentFrame.mvbOutlier.assign((size_t)N, true);
            tr.MonoObjDepthInitialization(&kf);
        } else {
            kf.mvKeys = keys;
            for (int i = 0; i < N; i++) if (has_mp[i]) kf.mvpMapPoints[i] = &existing;
            if (mode == 1) {
                kf.mnMinX = (int)bounds[0]; kf.mnMinY = (int)bounds[2]; // KeyFrame.cc:54
                kf.mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(bounds[1] - bounds[0]); // Frame.cc
                kf.mfGridElementHeightInv = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(bounds[3] - bounds[2]);
                Tracking tr;
                tr.mpMap = &map;
                tr.CreateNewKeyFrameObjectDepth(&kf, n_candidates, raw, max_init, nullptr, &after);
            } else {
                LocalMapping lm;
                lm.mpCurrentKeyFrame = &kf; lm.mpMap = &map;
                lm.CreateNewMapPointsTail();
                int k = 0;
                for (MapPoint *p : lm.mlpRecentAddedMapPoints) if (k >= (int)map.created.size() || map.created[k++].first != p) return -3; // the order of mlpRecentAddedMapPoints is the creation order
            }
        }
    } catch (const std::runtime_error &) { return -1; }
    for (size_t k = 0; k < after.size(); k++) shuffled[k] = after[k];
    for (size_t k = 0; k < map.created.size(); k++) {
        new_idx[k] = map.created[k].second;
        for (int j = 0; j < 3; j++) new_x3D[3 * k + j] = map.created[k].first->pos.el(j, 0);
    }
    const int n_new = (int)map.created.size();
    for (auto &c : map.created) delete c.first;
    return n_new;
}
}
