// TEST INFRASTRUCTURE: stand-ins for what Sim3Solver::SetRansacParameters, iterate, ComputeCentroid, ComputeSim3, CheckInliers, Project and FromCameraToImage
// (orb_object_slam/src/Sim3Solver.cc:112-205, :213-360, :377-418) touch.  tests/test_sim3_solver_restatement_pins.py cuts those functions out of the reference at test time into
// a temporary directory (ref_sim3_solver_extracted.inc), compiles this file around them there and runs them next to tests/sim3_solver_restatement.py on the same inputs.  Every
// statement of the seven functions is the reference's; this file supplies
//   * a cv::Mat sufficient for them: CV_32F only, shared storage with row / column views, and the cv::MatExpr forms they use, evaluated the way csrc/horn_math.h states them
//     (a product is one gemm with double accumulation, an optional scale and addend and a single rounding; s * Mat and Mat / n scale by a double with one rounding; Mat - Mat
//     is float; Mat::dot accumulates in double; cv::reduce(SUM) adds left to right in float; cv::pow(., 2) multiplies in float; an expression assigned to a Mat of its size
//     is written in place, which `Pr.col(i) = P.col(i) - C` relies on);
//   * cv::eigen as a cyclic Jacobi in FLOAT with the eigenvalues in descending order and the eigenvectors as rows (what cv::eigen does on CV_32F), and cv::Rodrigues as OpenCV's
//     formula R = cos(th) I + (1 - cos(th)) r r^T + sin(th) [r]x in double over libm: the two operations the library replaces by stated definitions, here in the form the
//     reference's build has them, so that the distance between the two can be measured;
//   * DUtils::Random::RandomInt replaying the pattern's triples: it returns the position of the wanted index in the reference's vAvailableIndices, which it tracks;
//   * the class declaration with the members those functions read, under the reference's names and types (mvnMaxError1 / 2 are std::vector<size_t> there).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define CV_32F 5
#define CV_REDUCE_SUM 0

namespace cv {
struct Size { int width = 0, height = 0; };
struct MatExpr;
struct ScaleExpr;
struct MulExpr;
class Mat {
  public:
    int rows = 0, cols = 0;
    Mat() {}
    Mat(int r, int c, int) { create(r, c, CV_32F); }
    Mat(Size s, int) { create(s.height, s.width, CV_32F); }
    Mat(const MatExpr &e);
    Mat(const ScaleExpr &e);
    Mat(const MulExpr &e);
    void create(int r, int c, int) {
        if (r == rows && c == cols && buf) return;
        rows = r; cols = c; step = c; off = 0; buf = std::make_shared<std::vector<float>>((size_t)r * c, 0.f);
    }
    bool empty() const { return !buf || rows * cols == 0; }
    Size size() const { Size s; s.width = cols; s.height = rows; return s; }
    int type() const { return CV_32F; }
    template <class T> T &at(int i, int j) { return (*buf)[off + (size_t)i * step + j]; }
    template <class T> const T &at(int i, int j) const { return (*buf)[off + (size_t)i * step + j]; }
    template <class T> T &at(int i) { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }
    template <class T> const T &at(int i) const { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }
    Mat view(int r0, int c0, int r, int c) const { Mat m; m.buf = buf; m.step = step; m.off = off + (size_t)r0 * step + c0; m.rows = r; m.cols = c; return m; }
    Mat row(int r) const { return view(r, 0, 1, cols); }
    Mat col(int c) const { return view(0, c, rows, 1); }
    Mat rowRange(int a, int b) const { return view(a, 0, b - a, cols); }
    Mat colRange(int a, int b) const { return view(0, a, rows, b - a); }
    void copyTo(const Mat &dst_) const { // into the storage of dst when the sizes agree (views included), a fresh block otherwise
        Mat &dst = const_cast<Mat &>(dst_);
        if (dst.rows != rows || dst.cols != cols || !dst.buf) { dst.rows = 0; dst.buf.reset(); dst.create(rows, cols, CV_32F); }
        for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) dst.at<float>(i, j) = at<float>(i, j);
    }
    Mat clone() const { Mat m; if (!empty()) copyTo(m); return m; }
    Mat t() const { Mat m(cols, rows, CV_32F); for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) m.at<float>(j, i) = at<float>(i, j); return m; }
    double dot(const Mat &o) const { double s = 0; for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) s += (double)at<float>(i, j) * (double)o.at<float>(i, j); return s; }
    static Mat eye(int r, int c, int) { Mat m(r, c, CV_32F); for (int i = 0; i < r && i < c; i++) m.at<float>(i, i) = 1.f; return m; }
    Mat &operator=(const Mat &o) = default; // a header copy: the storage is shared
    Mat &assign_values(const Mat &v) { // Mat = MatExpr: in place when the sizes agree
        if (v.rows == rows && v.cols == cols && buf) v.copyTo(*this); else *this = v;
        return *this;
    }
    Mat &operator=(const MatExpr &e);
    Mat &operator=(const ScaleExpr &e);
    Mat &operator=(const MulExpr &e);

  private:
    std::shared_ptr<std::vector<float>> buf;
    size_t step = 0, off = 0;
};
struct MatExpr { Mat m; };                        // an evaluated element-wise expression
struct ScaleExpr { Mat m; double alpha; Mat eval() const { Mat r(m.rows, m.cols, CV_32F); for (int i = 0; i < m.rows; i++) for (int j = 0; j < m.cols; j++) r.at<float>(i, j) = (float)((double)m.at<float>(i, j) * alpha); return r; } };
struct MulExpr {
    Mat a, b; double alpha;
    Mat eval(const Mat *c, double beta) const {
        Mat r(a.rows, b.cols, CV_32F);
        for (int i = 0; i < a.rows; i++) for (int j = 0; j < b.cols; j++) {
            double s = 0;
            for (int k = 0; k < a.cols; k++) s += (double)a.at<float>(i, k) * (double)b.at<float>(k, j);
            r.at<float>(i, j) = c ? (float)(s * alpha + (double)c->at<float>(i, j) * beta) : (float)(s * alpha);
        }
        return r;
    }
};
inline Mat::Mat(const MatExpr &e) { *this = e.m; }
inline Mat::Mat(const ScaleExpr &e) { *this = e.eval(); }
inline Mat::Mat(const MulExpr &e) { *this = e.eval(nullptr, 0); }
inline Mat &Mat::operator=(const MatExpr &e) { return assign_values(e.m); }
inline Mat &Mat::operator=(const ScaleExpr &e) { return assign_values(e.eval()); }
inline Mat &Mat::operator=(const MulExpr &e) { return assign_values(e.eval(nullptr, 0)); }

struct NegExpr { Mat m; };
inline MulExpr operator*(const Mat &a, const Mat &b) { return MulExpr{a, b, 1.0}; }
inline MulExpr operator*(const ScaleExpr &a, const Mat &b) { return MulExpr{a.m, b, a.alpha}; }
inline MulExpr operator*(const NegExpr &a, const Mat &b) { return MulExpr{a.m, b, -1.0}; }
inline NegExpr operator-(const Mat &m) { return NegExpr{m}; }
inline ScaleExpr operator*(double s, const Mat &m) { return ScaleExpr{m, s}; }
inline ScaleExpr operator/(const Mat &m, double s) { return ScaleExpr{m, 1.0 / s}; }
inline ScaleExpr operator/(const ScaleExpr &e, double s) { return ScaleExpr{e.m, e.alpha * (1.0 / s)}; }
inline MatExpr operator+(const MulExpr &e, const Mat &c) { return MatExpr{e.eval(&c, 1.0)}; }
inline MatExpr operator-(const Mat &c, const MulExpr &e) { MulExpr n = e; n.alpha = -e.alpha; return MatExpr{n.eval(&c, 1.0)}; }
inline MatExpr operator-(const Mat &a, const Mat &b) {
    Mat r(a.rows, a.cols, CV_32F);
    for (int i = 0; i < a.rows; i++) for (int j = 0; j < a.cols; j++) r.at<float>(i, j) = a.at<float>(i, j) - b.at<float>(i, j);
    return MatExpr{r};
}
inline double norm(const Mat &m) { return std::sqrt(m.dot(m)); }

template <class T> struct MatInit { // cv::Mat_<T>(r, c) << a, b, ...
    Mat m; int k = 0;
    template <class U> MatInit &operator,(U v) { m.at<T>(k / m.cols, k % m.cols) = (T)v; k++; return *this; }
    operator Mat() const { return m; }
};
template <class T> struct Mat_ {
    Mat m;
    Mat_(int r, int c) : m(r, c, CV_32F) {}
    template <class U> MatInit<T> operator<<(U v) { MatInit<T> i; i.m = m; i, v; return i; }
};

inline void reduce(const Mat &src, Mat &dst, int dim, int) { // dim == 1: every row to one column
    (void)dim;
    dst.create(src.rows, 1, CV_32F);
    for (int i = 0; i < src.rows; i++) { float s = src.at<float>(i, 0); for (int j = 1; j < src.cols; j++) s = s + src.at<float>(i, j); dst.at<float>(i, 0) = s; }
}
inline void pow(const Mat &src, double p, Mat &dst) {
    (void)p; // 2
    Mat r(src.rows, src.cols, CV_32F);
    for (int i = 0; i < src.rows; i++) for (int j = 0; j < src.cols; j++) r.at<float>(i, j) = src.at<float>(i, j) * src.at<float>(i, j);
    r.copyTo(dst);
}
// CV_32F symmetric: cyclic Jacobi in float, eigenvalues descending, eigenvectors as rows
inline bool eigen(const Mat &src, Mat &evals, Mat &evecs) {
    const int n = src.rows;
    std::vector<float> A((size_t)n * n), V((size_t)n * n, 0.f);
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) A[i * n + j] = src.at<float>(i, j); V[i * n + i] = 1.f; }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const float apq = A[p * n + q];
                if (std::fabs(apq) <= FLT_EPSILON * 0.25f * std::sqrt(std::fabs(A[p * n + p] * A[q * n + q])) || apq == 0.f) continue;
                rotated = true;
                const float zeta = (A[q * n + q] - A[p * n + p]) / (2.f * apq);
                const float t = (zeta < 0 ? -1.f : 1.f) / (std::fabs(zeta) + std::sqrt(1.f + zeta * zeta));
                const float c = 1.f / std::sqrt(1.f + t * t), s = c * t;
                A[p * n + p] -= t * apq; A[q * n + q] += t * apq; A[p * n + q] = A[q * n + p] = 0.f;
                for (int r = 0; r < n; r++) {
                    const float vp = V[r * n + p], vq = V[r * n + q];
                    V[r * n + p] = c * vp - s * vq; V[r * n + q] = s * vp + c * vq;
                    if (r == p || r == q) continue;
                    const float ap = A[r * n + p], aq = A[r * n + q];
                    A[r * n + p] = A[p * n + r] = c * ap - s * aq; A[r * n + q] = A[q * n + r] = s * ap + c * aq;
                }
            }
        if (!rotated) break;
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    for (int i = 0; i < n; i++) for (int j = i + 1; j < n; j++) if (A[order[j] * n + order[j]] > A[order[i] * n + order[i]]) std::swap(order[i], order[j]);
    evals.create(n, 1, CV_32F); evecs.create(n, n, CV_32F);
    for (int i = 0; i < n; i++) { evals.at<float>(i, 0) = A[order[i] * n + order[i]]; for (int r = 0; r < n; r++) evecs.at<float>(i, r) = V[r * n + order[i]]; }
    return true;
}
// a rotation vector (1 x 3 or 3 x 1, CV_32F) to a 3 x 3 matrix: OpenCV's cvRodrigues2 in double
inline void Rodrigues(const Mat &src, Mat &dst) {
    const double rx0 = src.at<float>(0), ry0 = src.at<float>(1), rz0 = src.at<float>(2);
    const double theta = std::sqrt(rx0 * rx0 + ry0 * ry0 + rz0 * rz0);
    double R[9];
    if (theta < DBL_EPSILON) { for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    else {
        const double c = std::cos(theta), s = std::sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
        const double rx = rx0 * itheta, ry = ry0 * itheta, rz = rz0 * itheta;
        const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
        const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
        for (int k = 0; k < 9; k++) R[k] = c * ((k % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[k] + s * r_x[k];
    }
    dst.create(3, 3, CV_32F);
    for (int k = 0; k < 9; k++) dst.at<float>(k / 3, k % 3) = (float)R[k];
}
} // namespace cv

// ---- RandomInt: replays the wanted triples through the reference's own Fisher-Yates
namespace DUtils {
struct Random {
    static std::vector<int> &want() { static std::vector<int> w; return w; }   // the indices the test wants drawn, 3 per iteration, of the solver that iterates now
    static size_t &pos() { static size_t p = 0; return p; }
    static std::vector<int> &avail() { static std::vector<int> a; return a; }
    static int &n_all() { static int n = 0; return n; }
    static int RandomInt(int min, int max) {
        std::vector<int> &a = avail();
        if (pos() % 3 == 0) { a.resize((size_t)n_all()); for (int i = 0; i < n_all(); i++) a[i] = i; }
        const int idx = want().at(pos()++);
        int r = -1;
        for (size_t i = 0; i < a.size(); i++) if (a[i] == idx) r = (int)i;
        if (r < min || r > max) std::abort(); // (a repeated or foreign index: the patterns have none)
        a[r] = a.back(); a.pop_back();
        return r;
    }
};
} // namespace DUtils

namespace ORB_SLAM2 {
using namespace std;
class KeyFrame;
class MapPoint;
class Sim3Solver {
  public:
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);
    void ComputeCentroid(cv::Mat &P, cv::Mat &Pr, cv::Mat &C);
    void ComputeSim3(cv::Mat &P1, cv::Mat &P2);
    void CheckInliers();
    void Project(const std::vector<cv::Mat> &vP3Dw, std::vector<cv::Mat> &vP2D, cv::Mat Tcw, cv::Mat K);
    void FromCameraToImage(const std::vector<cv::Mat> &vP3Dc, std::vector<cv::Mat> &vP2D, cv::Mat K);

    std::vector<cv::Mat> mvX3Dc1, mvX3Dc2;
    std::vector<MapPoint *> mvpMapPoints1;
    std::vector<size_t> mvnIndices1, mvnMaxError1, mvnMaxError2;
    int N = 0, mN1 = 0;
    cv::Mat mR12i, mt12i;
    float ms12i = 0;
    cv::Mat mT12i, mT21i;
    std::vector<bool> mvbInliersi;
    int mnInliersi = 0;
    int mnIterations = 0;
    std::vector<bool> mvbBestInliers;
    int mnBestInliers = 0;
    cv::Mat mBestT12, mBestRotation, mBestTranslation;
    float mBestScale = 0;
    bool mbFixScale = false;
    std::vector<size_t> mvAllIndices;
    std::vector<cv::Mat> mvP1im1, mvP2im2;
    double mRansacProb = 0;
    int mRansacMinInliers = 0, mRansacMaxIts = 0;
    cv::Mat mK1, mK2;
    std::vector<int> triples; // (the test's)
    size_t drawn = 0;
};

#include "ref_sim3_solver_extracted.inc"

} // namespace ORB_SLAM2

extern "C" {
using namespace ORB_SLAM2;
static cv::Mat K_of(const float *k) { cv::Mat K = cv::Mat::eye(3, 3, CV_32F); K.at<float>(0, 0) = k[0]; K.at<float>(1, 1) = k[1]; K.at<float>(0, 2) = k[2]; K.at<float>(1, 2) = k[3]; return K; }
static cv::Mat point(const float *p) { cv::Mat m(3, 1, CV_32F); for (int k = 0; k < 3; k++) m.at<float>(k, 0) = p[k]; return m; }

// the state the constructor leaves (:36-110) from the filtered correspondences; max_err are the size_t values of mvnMaxError1 / 2
void *pin_solver_new(int N, int mN1, const float *X1, const float *X2, const float *max_err1, const float *max_err2, const float *K8, const int *idx1, int fix_scale,
                     double probability, int minInliers, int maxIterations, const int *triples, int n_triples) {
    Sim3Solver *s = new Sim3Solver;
    s->mN1 = mN1; s->mbFixScale = fix_scale != 0;
    for (int i = 0; i < N; i++) {
        s->mvnMaxError1.push_back((size_t)max_err1[i]); s->mvnMaxError2.push_back((size_t)max_err2[i]);
        s->mvpMapPoints1.push_back(nullptr); s->mvnIndices1.push_back((size_t)idx1[i]);
        s->mvX3Dc1.push_back(point(X1 + 3 * i)); s->mvX3Dc2.push_back(point(X2 + 3 * i));
        s->mvAllIndices.push_back((size_t)i);
    }
    s->mK1 = K_of(K8); s->mK2 = K_of(K8 + 4);
    s->FromCameraToImage(s->mvX3Dc1, s->mvP1im1, s->mK1);
    s->FromCameraToImage(s->mvX3Dc2, s->mvP2im2, s->mK2);
    s->SetRansacParameters();
    s->SetRansacParameters(probability, minInliers, maxIterations);
    s->triples.assign(triples, triples + 3 * (size_t)n_triples);
    return s;
}
void pin_solver_delete(void *h) { delete (Sim3Solver *)h; }
int pin_solver_max_its(void *h) { return ((Sim3Solver *)h)->mRansacMaxIts; }

// iterate(nIterations, ...) -> 1 when a matrix came back; T12[16], vbInliers[mN1] bytes, state[4] = bNoMore, nInliers, mnIterations, mnBestInliers
int pin_solver_iterate(void *h, int nIterations, float *T12, unsigned char *vbInliers, int *state) {
    Sim3Solver *s = (Sim3Solver *)h;
    DUtils::Random::want() = s->triples; DUtils::Random::pos() = s->drawn; DUtils::Random::n_all() = s->N;
    bool bNoMore = false; std::vector<bool> vb; int nInliers = 0;
    cv::Mat T = s->iterate(nIterations, bNoMore, vb, nInliers);
    s->drawn = DUtils::Random::pos();
    for (size_t i = 0; i < vb.size(); i++) vbInliers[i] = vb[i];
    state[0] = bNoMore; state[1] = nInliers; state[2] = s->mnIterations; state[3] = s->mnBestInliers;
    if (T.empty()) return 0;
    for (int k = 0; k < 16; k++) T12[k] = T.at<float>(k / 4, k % 4);
    return 1;
}
// what the iteration just run left in the members: sRt[13] = ms12i, mR12i, mt12i; mnInliersi; mvbInliersi[N]; and err[2 N] = err1, err2 of every correspondence, recomputed
// from mT12i / mT21i through the reference's Project with the three statements of CheckInliers :346-350
int pin_solver_last(void *h, float *sRt, unsigned char *inl, float *err) {
    Sim3Solver *s = (Sim3Solver *)h;
    sRt[0] = s->ms12i;
    for (int k = 0; k < 9; k++) sRt[1 + k] = s->mR12i.at<float>(k / 3, k % 3);
    for (int k = 0; k < 3; k++) sRt[10 + k] = s->mt12i.at<float>(k);
    for (int i = 0; i < s->N; i++) inl[i] = s->mvbInliersi[i];
    std::vector<cv::Mat> vP1im2, vP2im1;
    s->Project(s->mvX3Dc2, vP2im1, s->mT12i, s->mK1);
    s->Project(s->mvX3Dc1, vP1im2, s->mT21i, s->mK2);
    for (int i = 0; i < s->N; i++) {
        cv::Mat dist1 = s->mvP1im1[i] - vP2im1[i];
        cv::Mat dist2 = vP1im2[i] - s->mvP2im2[i];
        err[i] = dist1.dot(dist1); err[s->N + i] = dist2.dot(dist2);
    }
    return s->mnInliersi;
}
}
