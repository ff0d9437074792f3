// TEST INFRASTRUCTURE: stand-ins for what the members of ORB_SLAM2::Initializer (orb_object_slam/src/Initializer.cc:45-933) touch.  tests/test_initializer_reference_pins.py
// cuts Initialize, FindHomography, FindFundamental, ComputeH21, ComputeF21, CheckHomography, CheckFundamental, ReconstructF, ReconstructH, Triangulate, Normalize, CheckRT and
// DecomposeE out of the reference at test time into a temporary directory (ref_initializer_extracted.inc), compiles this file around them there and runs it as a child
// process on the patterns of tests/initializer_patterns.py.  Every statement of the thirteen members is the reference's; this file supplies
//   * a cv::Mat sufficient for them: CV_32F only, shared storage with row / column views, and the cv::MatExpr forms they use, evaluated the way csrc/initializer_math.h states
//     them (a product is one gemm with double accumulation, an optional scale and addend and a single rounding; s * Mat, Mat / n and Mat *= d scale by a double with one
//     rounding; s * row - row is a float multiply and a float subtraction; Mat - Mat is float; Mat::dot and cv::norm accumulate in double; an expression assigned to a Mat of
//     its size is written in place, which `A.row(0) = ...` relies on);
//   * cv::SVDecomp / cv::SVD::compute, Mat::inv and cv::determinant forwarding to the library's stated definitions (csrc/initializer_math.h, INTEGRATION.md 8b''');
//   * DUtils::Random::RandomInt replaying the pattern's sets: it returns the position of the wanted index in the reference's vAvailableIndices, which it tracks;
//   * Frame, and the class declaration with the members those functions read, under the reference's names and types.
//   ref_initializer <in> <out>
// <in>: the format of tests/cpp/initializer_mirror.cpp.  <out>, per case: per hypothesis and model the score, whether the reference kept a matrix (score > 0), the matrix and
// the mask -- from FindHomography / FindFundamental run on that one set --; then SH, SF of the two run on the whole table, and of Initialize the branch (read off its own
// std::cout line), the return value, R21, t21, vP3D and vbTriangulated.  Initialize is not run where no hypothesis scores (the reference goes on with an empty matrix) or
// where there are fewer than 8 matches (its drawing is undefined).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <memory>
#include <sstream>
#include <thread>
#include <vector>

#include "cube_slam_amd/csrc/initializer_math.h"

#define CV_32F 5
#define CV_PI 3.1415926535897932384626433832795

namespace cv {
struct Point2f { float x = 0, y = 0; };
struct Point3f { float x = 0, y = 0, z = 0; Point3f() {} Point3f(float a, float b, float c) : x(a), y(b), z(c) {} };
struct KeyPoint { Point2f pt; };
struct Scalar { double v; Scalar(double a) : v(a) {} };
struct MatExpr;
struct ScaleExpr;
struct MulExpr;
struct NegExpr;
class Mat {
  public:
    int rows = 0, cols = 0;
    Mat() {}
    Mat(int r, int c, int) { create(r, c); }
    Mat(int r, int c, int, const Scalar &s) { create(r, c); for (float &v : *buf) v = (float)s.v; }
    Mat(const MatExpr &e);
    Mat(const ScaleExpr &e);
    Mat(const MulExpr &e);
    Mat(const NegExpr &e);
    void create(int r, int c) { rows = r; cols = c; step = (size_t)c; off = 0; buf = std::make_shared<std::vector<float>>((size_t)r * c, 0.f); }
    bool empty() const { return !buf || rows * cols == 0; }
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
        if (dst.rows != rows || dst.cols != cols || !dst.buf) dst.create(rows, cols);
        for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) dst.at<float>(i, j) = at<float>(i, j);
    }
    Mat clone() const { Mat m; if (!empty()) copyTo(m); return m; }
    Mat t() const { Mat m(cols, rows, CV_32F); for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) m.at<float>(j, i) = at<float>(i, j); return m; }
    Mat reshape(int, int r) const { Mat m(r, rows * cols / r, CV_32F); for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) m.at<float>((i * cols + j) / m.cols, (i * cols + j) % m.cols) = at<float>(i, j); return m; }
    Mat inv() const { // 3 x 3: the stated definition
        float a[9], b[9];
        get9(a); im_inv3(a, b);
        Mat m(3, 3, CV_32F); m.set9(b);
        return m;
    }
    double dot(const Mat &o) const { double s = 0; for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) s += (double)at<float>(i, j) * (double)o.at<float>(i, j); return s; }
    static Mat eye(int r, int c, int) { Mat m(r, c, CV_32F); for (int i = 0; i < r && i < c; i++) m.at<float>(i, i) = 1.f; return m; }
    static Mat zeros(int r, int c, int) { return Mat(r, c, CV_32F); }
    static Mat diag(const Mat &d) { const int n = d.rows * d.cols; Mat m(n, n, CV_32F); for (int i = 0; i < n; i++) m.at<float>(i, i) = d.at<float>(i); return m; }
    Mat &operator=(const Mat &o) = default; // a header copy: the storage is shared
    Mat &assign_values(const Mat &v) { // Mat = MatExpr: in place when the sizes agree
        if (v.rows == rows && v.cols == cols && buf) v.copyTo(*this); else *this = v;
        return *this;
    }
    Mat &operator=(const MatExpr &e);
    Mat &operator=(const ScaleExpr &e);
    Mat &operator=(const MulExpr &e);
    Mat &operator=(const NegExpr &e);
    Mat &operator*=(double d) { for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) at<float>(i, j) = (float)((double)at<float>(i, j) * d); return *this; }
    void get9(float *a) const { for (int k = 0; k < 9; k++) a[k] = at<float>(k / 3, k % 3); }
    void set9(const float *a) { for (int k = 0; k < 9; k++) at<float>(k / 3, k % 3) = a[k]; }

  private:
    std::shared_ptr<std::vector<float>> buf;
    size_t step = 0, off = 0;
};
struct MatExpr { Mat m; }; // an evaluated element-wise expression
struct ScaleExpr {
    Mat m; double alpha;
    Mat eval() const { Mat r(m.rows, m.cols, CV_32F); for (int i = 0; i < m.rows; i++) for (int j = 0; j < m.cols; j++) r.at<float>(i, j) = (float)((double)m.at<float>(i, j) * alpha); return r; }
};
struct NegExpr { Mat m; Mat eval() const { Mat r(m.rows, m.cols, CV_32F); for (int i = 0; i < m.rows; i++) for (int j = 0; j < m.cols; j++) r.at<float>(i, j) = -m.at<float>(i, j); return r; } };
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
inline Mat::Mat(const NegExpr &e) { *this = e.eval(); }
inline Mat &Mat::operator=(const MatExpr &e) { return assign_values(e.m); }
inline Mat &Mat::operator=(const ScaleExpr &e) { return assign_values(e.eval()); }
inline Mat &Mat::operator=(const MulExpr &e) { return assign_values(e.eval(nullptr, 0)); }
inline Mat &Mat::operator=(const NegExpr &e) { return assign_values(e.eval()); }

inline MulExpr operator*(const Mat &a, const Mat &b) { return MulExpr{a, b, 1.0}; }
inline MulExpr operator*(const MulExpr &a, const Mat &b) { return MulExpr{a.eval(nullptr, 0), b, 1.0}; } // A * B * C: the first product is rounded
inline MulExpr operator*(const ScaleExpr &a, const Mat &b) { return MulExpr{a.m, b, a.alpha}; }           // s * U * Rp: the scale stays inside the product's rounding
inline MulExpr operator*(const NegExpr &a, const Mat &b) { return MulExpr{a.m, b, -1.0}; }                 // -R.t() * t
inline NegExpr operator-(const Mat &m) { return NegExpr{m}; }
inline ScaleExpr operator*(double s, const Mat &m) { return ScaleExpr{m, s}; }
inline ScaleExpr operator/(const Mat &m, double s) { return ScaleExpr{m, 1.0 / s}; }
inline MatExpr operator+(const MulExpr &e, const Mat &c) { return MatExpr{e.eval(&c, 1.0)}; } // R * p + t
inline MatExpr operator-(const Mat &a, const Mat &b) {
    Mat r(a.rows, a.cols, CV_32F);
    for (int i = 0; i < a.rows; i++) for (int j = 0; j < a.cols; j++) r.at<float>(i, j) = a.at<float>(i, j) - b.at<float>(i, j);
    return MatExpr{r};
}
inline MatExpr operator-(const ScaleExpr &a, const Mat &b) { return a.eval() - b; } // kp.pt.x * P.row(2) - P.row(0): a float multiply, a float subtraction
inline double norm(const Mat &m) { return std::sqrt(m.dot(m)); }
inline double determinant(const Mat &m) { float a[9]; m.get9(a); return im_det3(a); }

struct SVD {
    enum { MODIFY_A = 1, NO_UV = 2, FULL_UV = 4 };
    // the shapes Initializer hands it, each through the library's stated definition
    static void compute(const Mat &A, Mat &w, Mat &u, Mat &vt, int = 0) {
        InitSvdWork wk;
        const CvxSeq x;
        if (A.rows == 16 && A.cols == 9) { // the Jacobi on the rows of A transposed; u is not read
            for (int r = 0; r < 16; r++) for (int c = 0; c < 9; c++) wk.At[c * 16 + r] = A.at<float>(r, c);
            cvx_jacobi_rows(x, wk.At, 16, 9, wk.W, wk.Vt);
            vt = Mat(9, 9, CV_32F); w = Mat(9, 1, CV_32F); u = Mat();
            for (int k = 0; k < 81; k++) vt.at<float>(k / 9, k % 9) = wk.Vt[k];
            for (int k = 0; k < 9; k++) w.at<float>(k) = (float)wk.W[k];
        } else if (A.rows == 8 && A.cols == 9) { // m < n: the Jacobi on the 8 rows of A, vt.row(8) the completion; u is not read
            for (int r = 0; r < 8; r++) for (int c = 0; c < 9; c++) wk.At[r * 9 + c] = A.at<float>(r, c);
            cvx_jacobi_rows(x, wk.At, 9, 8, wk.W, wk.Vt);
            cvx_unit_rows(x, wk.At, 9, 8, wk.W);
            im_complete_row9(wk.At, wk.row);
            vt = Mat(9, 9, CV_32F); w = Mat(8, 1, CV_32F); u = Mat();
            for (int k = 0; k < 72; k++) vt.at<float>(k / 9, k % 9) = wk.At[k];
            for (int k = 0; k < 9; k++) vt.at<float>(8, k) = wk.row[k];
            for (int k = 0; k < 8; k++) w.at<float>(k) = (float)wk.W[k];
        } else if (A.rows == 3 && A.cols == 3) {
            float a[9], U[9], wf[3], Vt[9];
            A.get9(a);
            im_svd3(x, a, &wk, U, wf, Vt);
            u = Mat(3, 3, CV_32F); vt = Mat(3, 3, CV_32F); w = Mat(3, 1, CV_32F);
            u.set9(U); vt.set9(Vt);
            for (int k = 0; k < 3; k++) w.at<float>(k) = wf[k];
        } else if (A.rows == 4 && A.cols == 4) { // Triangulate: jacobi_vmin4 gives vt.row(3), the one row that is read
            double a[16], v[4];
            for (int k = 0; k < 16; k++) a[k] = (double)A.at<float>(k / 4, k % 4);
            jacobi_vmin4(a, v);
            vt = Mat(4, 4, CV_32F); w = Mat(); u = Mat();
            for (int k = 0; k < 4; k++) vt.at<float>(3, k) = (float)v[k];
        } else { fprintf(stderr, "cv::SVD::compute: a %d x %d matrix\n", A.rows, A.cols); exit(4); }
    }
};
inline void SVDecomp(const Mat &A, Mat &w, Mat &u, Mat &vt, int flags = 0) { SVD::compute(A, w, u, vt, flags); }
} // namespace cv

// ---- DUtils::Random replaying the sets
static std::vector<int> g_want;
static std::vector<int> g_avail;
static size_t g_pos = 0;
static int g_N = 0;
namespace DUtils { namespace Random {
inline void SeedRandOnce(int) {}
inline int RandomInt(int lo, int hi) {
    if (g_pos % 8 == 0) { g_avail.resize((size_t)g_N); for (int i = 0; i < g_N; i++) g_avail[i] = i; }
    if (g_pos >= g_want.size()) { fprintf(stderr, "RandomInt: past the case's sets\n"); exit(3); }
    const int at = (int)(std::find(g_avail.begin(), g_avail.end(), g_want[g_pos++]) - g_avail.begin());
    if (lo != 0 || hi != (int)g_avail.size() - 1 || at > hi) { fprintf(stderr, "RandomInt: not the Fisher-Yates of :83-98\n"); exit(3); }
    g_avail[at] = g_avail.back(); g_avail.pop_back();
    return at;
}
} } // namespace DUtils::Random

namespace ORB_SLAM2 {
using namespace std;

class Frame {
  public:
    std::vector<cv::KeyPoint> mvKeysUn;
};

class Initializer { // the declaration of orb_object_slam/include/Initializer.h, everything public
  public:
    typedef pair<int, int> Match;
    Initializer(const std::vector<cv::KeyPoint> &keys1, const cv::Mat &K, float sigma, int iterations) { // :34-43
        mK = K.clone();
        mvKeys1 = keys1;
        mSigma = sigma;
        mSigma2 = sigma * sigma;
        mMaxIterations = iterations;
    }
    bool Initialize(const Frame &CurrentFrame, const vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21, vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated);
    void FindHomography(vector<bool> &vbMatchesInliers, float &score, cv::Mat &H21);
    void FindFundamental(vector<bool> &vbInliers, float &score, cv::Mat &F21);
    cv::Mat ComputeH21(const vector<cv::Point2f> &vP1, const vector<cv::Point2f> &vP2);
    cv::Mat ComputeF21(const vector<cv::Point2f> &vP1, const vector<cv::Point2f> &vP2);
    float CheckHomography(const cv::Mat &H21, const cv::Mat &H12, vector<bool> &vbMatchesInliers, float sigma);
    float CheckFundamental(const cv::Mat &F21, vector<bool> &vbMatchesInliers, float sigma);
    bool ReconstructF(vector<bool> &vbMatchesInliers, cv::Mat &F21, cv::Mat &K, cv::Mat &R21, cv::Mat &t21, vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated, float minParallax,
                      int minTriangulated);
    bool ReconstructH(vector<bool> &vbMatchesInliers, cv::Mat &H21, cv::Mat &K, cv::Mat &R21, cv::Mat &t21, vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated, float minParallax,
                      int minTriangulated);
    void Triangulate(const cv::KeyPoint &kp1, const cv::KeyPoint &kp2, const cv::Mat &P1, const cv::Mat &P2, cv::Mat &x3D);
    void Normalize(const vector<cv::KeyPoint> &vKeys, vector<cv::Point2f> &vNormalizedPoints, cv::Mat &T);
    int CheckRT(const cv::Mat &R, const cv::Mat &t, const vector<cv::KeyPoint> &vKeys1, const vector<cv::KeyPoint> &vKeys2, const vector<Match> &vMatches12,
                vector<bool> &vbInliers, const cv::Mat &K, vector<cv::Point3f> &vP3D, float th2, vector<bool> &vbGood, float &parallax);
    void DecomposeE(const cv::Mat &E, cv::Mat &R1, cv::Mat &R2, cv::Mat &t);

    vector<cv::KeyPoint> mvKeys1, mvKeys2;
    vector<Match> mvMatches12;
    vector<bool> mvbMatched1;
    cv::Mat mK;
    float mSigma, mSigma2;
    int mMaxIterations;
    vector<vector<size_t>> mvSets;
};

#include "ref_initializer_extracted.inc"

} // namespace ORB_SLAM2

static FILE *in, *out;
template <class T> static std::vector<T> rd(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
template <class T> static void wr(const T *p, size_t n) { if (n) fwrite(p, sizeof(T), n, out); }
static void wr_mat(const cv::Mat &m, int n) { // n floats: the matrix row-major, zeros where it is empty
    std::vector<float> v((size_t)n, 0.f);
    if (!m.empty()) for (int k = 0; k < n; k++) v[k] = m.at<float>(k / m.cols, k % m.cols);
    wr(v.data(), v.size());
}
static void wr_mask(const std::vector<bool> &m, size_t n) { std::vector<unsigned char> v(n, 0); for (size_t i = 0; i < m.size() && i < n; i++) v[i] = m[i]; wr(v.data(), n); }

int main(int argc, char **argv) {
    if (argc < 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    const int n = rd<int>(1)[0];
    for (int s = 0; s < n; s++) {
        const std::vector<int> h = rd<int>(3);
        const std::vector<float> sk = rd<float>(10), keys1 = rd<float>(2 * (size_t)h[0]), keys2 = rd<float>(2 * (size_t)h[1]);
        const std::vector<int> vMatches12 = rd<int>((size_t)h[0]), sets = rd<int>(8 * (size_t)h[2]);
        const int H = h[2];
        std::vector<cv::KeyPoint> k1((size_t)h[0]);
        ORB_SLAM2::Frame F2;
        F2.mvKeysUn.resize((size_t)h[1]);
        for (int i = 0; i < h[0]; i++) { k1[i].pt.x = keys1[2 * i]; k1[i].pt.y = keys1[2 * i + 1]; }
        for (int i = 0; i < h[1]; i++) { F2.mvKeysUn[i].pt.x = keys2[2 * i]; F2.mvKeysUn[i].pt.y = keys2[2 * i + 1]; }
        cv::Mat K(3, 3, CV_32F);
        K.set9(sk.data() + 1);
        ORB_SLAM2::Initializer init(k1, K, sk[0], H);
        init.mvKeys2 = F2.mvKeysUn; // :50-64, for the members run on their own
        for (size_t i = 0; i < vMatches12.size(); i++) if (vMatches12[i] >= 0) init.mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
        const size_t N = init.mvMatches12.size();
        float S[2] = {0, 0};
        for (int pass = 0; pass <= H; pass++) { // one set at a time, then (pass == H) the whole table
            const int h0 = pass < H ? pass : 0, h1 = pass < H ? pass + 1 : H;
            init.mMaxIterations = h1 - h0;
            init.mvSets.assign((size_t)(h1 - h0), std::vector<size_t>(8, 0));
            for (int it = h0; it < h1; it++) for (int j = 0; j < 8; j++) init.mvSets[it - h0][j] = (size_t)sets[8 * it + j];
            for (int model = 0; model < 2; model++) {
                std::vector<bool> inl; // (Initialize hands both an empty vector, :101)
                float score = -1;
                cv::Mat M;
                if (init.mMaxIterations) { if (model == 0) init.FindHomography(inl, score, M); else init.FindFundamental(inl, score, M); } else score = 0;
                if (pass == H) { S[model] = score; continue; }
                const int kept = !M.empty();
                wr(&score, 1); wr(&kept, 1); wr_mat(M, 9); wr_mask(inl, N);
            }
        }
        wr(S, 2);
        int branch = -1, ret = -1;
        cv::Mat R21, t21;
        std::vector<cv::Point3f> vP3D;
        std::vector<bool> vbTriangulated;
        if (N >= 8 && H && (S[0] > 0 || S[1] > 0)) {
            init.mMaxIterations = H;
            g_want = sets; g_pos = 0; g_N = (int)N;
            std::ostringstream said;
            std::streambuf *old = std::cout.rdbuf(said.rdbuf());
            ret = init.Initialize(F2, vMatches12, R21, t21, vP3D, vbTriangulated) ? 1 : 0;
            std::cout.rdbuf(old);
            branch = said.str().find("Homography") != std::string::npos ? 0 : 1;
        }
        wr(&branch, 1); wr(&ret, 1); wr_mat(R21, 9); wr_mat(t21, 3);
        const int np = (int)vP3D.size(), nb = (int)vbTriangulated.size();
        wr(&np, 1);
        for (const cv::Point3f &p : vP3D) { const float v[3] = {p.x, p.y, p.z}; wr(v, 3); }
        wr(&nb, 1); wr_mask(vbTriangulated, (size_t)nb);
    }
    fclose(out);
    return 0;
}
