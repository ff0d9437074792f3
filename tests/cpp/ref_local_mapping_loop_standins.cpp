// TEST INFRASTRUCTURE: stand-ins for everything LocalMapping::CreateNewMapPoints (orb_object_slam/src/LocalMapping.cc:319-570) and KeyFrame::UnprojectStereo (KeyFrame.cc:675-691)
// touch.  tests/test_local_mapping_restatement_pins.py cuts the two functions out of the reference at test time into a temporary directory (ref_local_mapping_loop_extracted.inc;
// CreateNewMapPoints up to the line that prints nnew, :570 -- the object-depth tail :571-652 is the caller's), compiles this file around them there and runs them next to
// tests/local_mapping_restatement.py on the same scenes.  Every statement of the loop is the reference's: the sequential neighbours, the skip through GetMapPoint(idx1) at the
// moment of each search, the order of the tests.
//
// cv::Mat here is a float matrix with views (row / col / rowRange / colRange share the buffer; assigning an EXPRESSION to a view writes through it, as cv::Mat::operator=(const
// MatExpr &) does; assigning a Mat rebinds the header).  The expression forms, as OpenCV 2.4 - 3.x evaluates them on CV_32F:
//   A * B (+ C)          one gemm: double accumulation over k ascending, one rounding
//   s * M - N            cv::addWeighted(M, s, N, -1, 0): float(M * float(s)) + float(N * -1.f) + 0.f per element, in float, no fused multiply-add
//   M - N, M + N         float
//   M / s                every element times 1.0 / s in double, one rounding (the library's stated definition of the cv::MatExpr scale)
//   Mat::dot, cv::norm   double accumulation
// cv::SVD::compute is a one-sided Jacobi in FLOAT (the reference's is OpenCV's float JacobiSVD; which one exactly depends on the OpenCV it was built with): the distance this and
// libm's cosf / atan2f put between the reference and the restatement's stated definitions is what the test measures as D_REF_X3D.
// ORBmatcher::SearchForTriangulation looks up a per-neighbour table of best matches and applies pKF1->GetMapPoint(idx1) itself, at call time (ORBmatcher.cc:721-725).
#include <cmath>
#include <cstring>
#include <iostream>
#include <list>
#include <memory>
#include <mutex>
#include <vector>

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
    Mat clone() const { return Mat(value()); }
    Mat t() const { Expr e; e.rows = cols; e.cols = rows; for (int c = 0; c < cols; c++) for (int r = 0; r < rows; r++) e.v.push_back(el(r, c)); return Mat(e); }
    void copyTo(Mat dst) const { dst = value(); } // (dst is a view of the caller's matrix with the same size: written through)
    double dot(const Mat &m) const { const Expr a = value(), b = m.value(); double s = 0; for (size_t i = 0; i < a.v.size(); i++) s += (double)a.v[i] * (double)b.v[i]; return s; }
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
inline Expr operator-(const Mat &a, const Mat &b) { Expr e; e.rows = a.rows; e.cols = a.cols; for (int r = 0; r < a.rows; r++) for (int c = 0; c < a.cols; c++) e.v.push_back(a.el(r, c) - b.el(r, c)); return e; }
inline Expr operator/(const Mat &m, double s) { Expr e; e.rows = m.rows; e.cols = m.cols; const double inv = 1.0 / s; for (int r = 0; r < m.rows; r++) for (int c = 0; c < m.cols; c++) e.v.push_back((float)((double)m.el(r, c) * inv)); return e; }
inline double norm(const Mat &m) { return std::sqrt(m.dot(m)); }
inline double norm(const Expr &e) { return norm(Mat(e)); }

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

namespace ORB_SLAM2 {
using namespace std;
bool whether_dynamic_object = false;

class KeyFrame;
class Map;
class MapPoint {
  public:
    cv::Mat pos; KeyFrame *ref;
    std::vector<std::pair<KeyFrame *, size_t>> obs;
    MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map *) : pos(Pos.clone()), ref(pRefKF) {}
    void AddObservation(KeyFrame *pKF, size_t idx) { obs.push_back(std::make_pair(pKF, idx)); }
    void ComputeDistinctiveDescriptors() {}
    void UpdateNormalAndDepth() {}
};
class Map {
  public:
    std::vector<MapPoint *> points; // in creation order
    void AddMapPoint(MapPoint *p) { points.push_back(p); }
};
class KeyFrame {
  public:
    int index = -1; // -1: the current key frame, else its place among the neighbours
    float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mbf = 0, mb = 0, mfScaleFactor = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth, mvScaleFactors, mvLevelSigma2;
    std::vector<bool> KeysStatic;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat Rcw, tcw, Ow, Twc;
    std::mutex mMutexPose;
    float median_depth = 1.f;
    std::vector<int> best2; // of a neighbour: the best match of every key point of the current key frame
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    float ComputeSceneMedianDepth(int) { return median_depth; }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    cv::Mat UnprojectStereo(int i);
    std::vector<KeyFrame *> neighbours;
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(int) { return neighbours; }
};
struct PairRecord { int neighbour, idx1, idx2; };
std::vector<PairRecord> g_pairs; // every pair every search returned, in order
class ORBmatcher {
  public:
    ORBmatcher(float, bool) {}
    int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat, std::vector<std::pair<size_t, size_t>> &vMatchedPairs, const bool) {
        vMatchedPairs.clear();
        for (size_t idx1 = 0; idx1 < pKF2->best2.size(); idx1++) {
            if (pKF1->GetMapPoint(idx1)) continue; // ORBmatcher.cc:721-725, at the moment of this call
            if (pKF2->best2[idx1] < 0) continue;
            vMatchedPairs.push_back(std::make_pair(idx1, (size_t)pKF2->best2[idx1]));
            g_pairs.push_back(PairRecord{pKF2->index, (int)idx1, pKF2->best2[idx1]});
        }
        return (int)vMatchedPairs.size();
    }
};
class LocalMapping {
  public:
    bool mbMonocular = false;
    KeyFrame *mpCurrentKeyFrame = nullptr;
    Map *mpMap = nullptr;
    std::list<MapPoint *> mlpRecentAddedMapPoints;
    bool CheckNewKeyFrames() { return false; }
    cv::Mat ComputeF12(KeyFrame *&, KeyFrame *&) { return cv::Mat(); }
    void CreateNewMapPoints();
};

#include "ref_local_mapping_loop_extracted.inc"

} // namespace ORB_SLAM2

namespace {
using namespace ORB_SLAM2;
struct FrameIn { int N; const float *ux, *uy, *kx, *ky, *ur, *depth; const int *octave; const float *pose /* Rcw tcw Ow */, *cam /* fx fy cx cy invfx invfy mbf mb */; int n_levels; const float *sf, *sigma2; float scale_factor; };
cv::Mat mat(int r, int c, const float *v) { cv::Mat m(r, c, CV_32F); for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.el(i, j) = v[i * c + j]; return m; }
void fill(KeyFrame &K, const FrameIn &I) {
    K.mvKeys.resize(I.N); K.mvKeysUn.resize(I.N);
    for (int i = 0; i < I.N; i++) { K.mvKeysUn[i].pt.x = I.ux[i]; K.mvKeysUn[i].pt.y = I.uy[i]; K.mvKeysUn[i].octave = I.octave[i]; K.mvKeys[i].pt.x = I.kx[i]; K.mvKeys[i].pt.y = I.ky[i]; K.mvKeys[i].octave = I.octave[i]; }
    K.mvuRight.assign(I.ur, I.ur + I.N); K.mvDepth.assign(I.depth, I.depth + I.N);
    K.mvScaleFactors.assign(I.sf, I.sf + I.n_levels); K.mvLevelSigma2.assign(I.sigma2, I.sigma2 + I.n_levels);
    K.mvpMapPoints.assign((size_t)I.N, nullptr);
    K.Rcw = mat(3, 3, I.pose); K.tcw = mat(3, 1, I.pose + 9); K.Ow = mat(3, 1, I.pose + 12);
    K.Twc = cv::Mat(4, 4, CV_32F); // as KeyFrame::SetPose leaves it: [Rwc | Ow]
    K.Rcw.t().copyTo(K.Twc.rowRange(0, 3).colRange(0, 3)); K.Ow.copyTo(K.Twc.rowRange(0, 3).col(3)); K.Twc.el(3, 3) = 1.f;
    K.fx = I.cam[0]; K.fy = I.cam[1]; K.cx = I.cam[2]; K.cy = I.cam[3]; K.invfx = I.cam[4]; K.invfy = I.cam[5]; K.mbf = I.cam[6]; K.mb = I.cam[7]; K.mfScaleFactor = I.scale_factor;
}
} // namespace

extern "C" {
// :431 / :433 as the reference writes it, with the float overloads its `using namespace std` selects
float pin_cos_stereo(float mb, float depth) { using namespace std; return cos(2 * atan2(mb / 2, depth)); }
// Runs the loop.  median_depth[n_neigh]: what ComputeSceneMedianDepth(2) returns (read in the monocular case only; with 0 the baseline test :367-371 drops no neighbour: the
// quotient is inf or NaN).  skip1[N1]: the key points of the current key frame that have a map point on entry.  best2: n_neigh x N1.  Outputs: the pairs the searches returned
// (capacity n_neigh * N1: neighbour, idx1, idx2) and the created points in creation order (capacity N1: neighbour, idx1, idx2, x3D).  Returns the number of created points.
int pin_create_new_map_points(const FrameIn *cur, const FrameIn *nbs, int n_neigh, int monocular, const float *median_depth, const unsigned char *skip1, const int *best2, int *n_pairs, int *pairs3, int *new3,
                              float *new_x3D) {
    KeyFrame K1; fill(K1, *cur);
    std::vector<std::unique_ptr<KeyFrame>> own;
    MapPoint before(mat(3, 1, cur->pose), &K1, nullptr);
    for (int i = 0; i < cur->N; i++) if (skip1[i]) K1.mvpMapPoints[i] = &before;
    for (int n = 0; n < n_neigh; n++) {
        own.emplace_back(new KeyFrame());
        fill(*own.back(), nbs[n]);
        own.back()->index = n;
        own.back()->median_depth = median_depth[n];
        own.back()->best2.assign(best2 + (size_t)n * cur->N, best2 + (size_t)(n + 1) * cur->N);
        K1.neighbours.push_back(own.back().get());
    }
    Map map;
    LocalMapping lm; lm.mbMonocular = monocular != 0; lm.mpCurrentKeyFrame = &K1; lm.mpMap = &map;
    g_pairs.clear();
    std::cout.setstate(std::ios_base::failbit); // (the loop prints nnew)
    lm.CreateNewMapPoints();
    std::cout.clear();
    *n_pairs = (int)g_pairs.size();
    for (size_t p = 0; p < g_pairs.size(); p++) { pairs3[3 * p] = g_pairs[p].neighbour; pairs3[3 * p + 1] = g_pairs[p].idx1; pairs3[3 * p + 2] = g_pairs[p].idx2; }
    for (size_t k = 0; k < map.points.size(); k++) {
        MapPoint *p = map.points[k];
        new3[3 * k] = p->obs[1].first->index; new3[3 * k + 1] = (int)p->obs[0].second; new3[3 * k + 2] = (int)p->obs[1].second;
        for (int c = 0; c < 3; c++) new_x3D[3 * k + c] = p->pos.at<float>(c);
        delete p;
    }
    return (int)map.points.size();
}
}
