// TEST INFRASTRUCTURE: stand-ins for the SLAM classes that the reference's Optimizer::OptimizeSim3 (orb_object_slam/src/Optimizer.cc:2838-3033) touches.
// tests/test_sim3_opt_restatement_pins.py cuts that function out of the reference at test time into a temporary directory (ref_sim3_opt_extracted.inc), compiles this file
// around it there against the reference's vendored g2o headers (with oracle/ref_shim/eigen_full for Eigen and oracle/ref_shim/cvshim.hpp for cv::Mat), links it with
// types_seven_dof_expmap.cpp and the g2o objects of oracle/_ref, and runs it next to tests/sim3_opt_restatement.py on the same inputs.  KeyFrame, MapPoint and Converter
// carry just the members that function reads, under the reference's names; every statement of the optimisation is the reference's.
#include <cmath>
#include <cstdint>
#include <iostream>
#include <vector>

#include "cvshim.hpp"

#include <Eigen/Core>
#include <Eigen/Dense>
#include <Eigen/Geometry>
#include <Eigen/StdVector>

#include "Thirdparty/g2o/g2o/core/block_solver.h"
#include "Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.h"
#include "Thirdparty/g2o/g2o/core/robust_kernel_impl.h"
#include "Thirdparty/g2o/g2o/solvers/linear_solver_dense.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"

// R * P + t the way cv::MatExpr evaluates it: one gemm with double accumulation over k ascending and a single rounding to float
namespace cv {
struct MulExpr { Mat a, b; };
inline MulExpr operator*(const Mat &a, const Mat &b) { return MulExpr{a, b}; }
inline Mat operator+(const MulExpr &e, const Mat &c) {
    Mat r(e.a.rows, e.b.cols, CV_32F);
    for (int i = 0; i < e.a.rows; i++) for (int j = 0; j < e.b.cols; j++) {
        double s = 0;
        for (int k = 0; k < e.a.cols; k++) s += (double)e.a.at<float>(i, k) * (double)e.b.at<float>(k, j);
        r.at<float>(i, j) = (float)(s * 1.0 + (double)c.at<float>(i, j) * 1.0);
    }
    return r;
}
} // namespace cv

namespace ORB_SLAM2 {
using namespace std;

class KeyFrame;
class MapPoint {
  public:
    cv::Mat mWorldPos;
    bool bad = false;
    int index_in_kf2 = -1;
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return bad; }
    int GetIndexInKeyFrame(KeyFrame *) { return index_in_kf2; }
};
class KeyFrame {
  public:
    cv::Mat mK, Rcw, tcw;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
};
class Converter {
  public:
    static Eigen::Matrix<double, 3, 1> toVector3d(const cv::Mat &v) { // Converter.cc: v << cvVector.at<float>(0), cvVector.at<float>(1), cvVector.at<float>(2)
        Eigen::Matrix<double, 3, 1> r;
        r << v.at<float>(0), v.at<float>(1), v.at<float>(2);
        return r;
    }
};
class Optimizer {
  public:
    int static OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale);
};

#include "ref_sim3_opt_extracted.inc"
} // namespace ORB_SLAM2

using namespace ORB_SLAM2;

static cv::Mat mat_f(int r, int c, const float *v) { cv::Mat m(r, c, CV_32F); for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) m.at<float>(i, j) = v[i * c + j]; return m; }

// One problem in the arrays of cs_sim3_optimization.  Both key frames sit at the identity pose, so R * P + t of the reference's :2910 / :2918 returns the float
// points handed in; every correspondence has a key point of its own in either frame, on a level of its own whose invSigma2 is the one handed in.
extern "C" __attribute__((visibility("default"))) int pin_optimize_sim3(int n, const double *P1c, const double *P2c, const double *obs1, const double *obs2, const double *inv_sigma2_1,
                                                                        const double *inv_sigma2_2, const double *intr8, const double *sim3_in, float th2, int fix_scale, int repeats,
                                                                        double *sim3_out, uint8_t *removed) {
    const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0};
    int ret = 0;
    for (int rep = 0; rep < (repeats > 0 ? repeats : 1); rep++) {
        KeyFrame kf[2];
        std::vector<MapPoint> mp1((size_t)n), mp2((size_t)n);
        for (int f = 0; f < 2; f++) {
            const float K[9] = {(float)intr8[f * 4], 0, (float)intr8[f * 4 + 2], 0, (float)intr8[f * 4 + 1], (float)intr8[f * 4 + 3], 0, 0, 1};
            kf[f].mK = mat_f(3, 3, K); kf[f].Rcw = mat_f(3, 3, eye); kf[f].tcw = mat_f(3, 1, zero);
            kf[f].mvKeysUn.resize((size_t)n); kf[f].mvInvLevelSigma2.resize((size_t)n);
            const double *obs = f ? obs2 : obs1, *w = f ? inv_sigma2_2 : inv_sigma2_1;
            for (int i = 0; i < n; i++) {
                cv::KeyPoint &k = kf[f].mvKeysUn[(size_t)i];
                k.pt.x = (float)obs[i * 2]; k.pt.y = (float)obs[i * 2 + 1]; k.octave = i;
                kf[f].mvInvLevelSigma2[(size_t)i] = (float)w[i];
            }
        }
        std::vector<MapPoint *> matches((size_t)n);
        for (int i = 0; i < n; i++) {
            const float a[3] = {(float)P1c[i * 3], (float)P1c[i * 3 + 1], (float)P1c[i * 3 + 2]}, b[3] = {(float)P2c[i * 3], (float)P2c[i * 3 + 1], (float)P2c[i * 3 + 2]};
            mp1[(size_t)i].mWorldPos = mat_f(3, 1, a); mp2[(size_t)i].mWorldPos = mat_f(3, 1, b); mp2[(size_t)i].index_in_kf2 = i;
            kf[0].mvpMapPoints.push_back(&mp1[(size_t)i]); matches[(size_t)i] = &mp2[(size_t)i];
        }
        g2o::Sim3 S(Eigen::Quaterniond(sim3_in[6], sim3_in[3], sim3_in[4], sim3_in[5]), Eigen::Vector3d(sim3_in[0], sim3_in[1], sim3_in[2]), sim3_in[7]);
        std::streambuf *was = std::cerr.rdbuf(nullptr); // optimize() complains on std::cerr when there is no vertex to optimise (n = 0)
        ret = Optimizer::OptimizeSim3(&kf[0], &kf[1], matches, S, th2, fix_scale != 0);
        std::cerr.rdbuf(was);
        for (int k = 0; k < 3; k++) sim3_out[k] = S.translation()[k];
        for (int k = 0; k < 4; k++) sim3_out[3 + k] = S.rotation().coeffs()[k];
        sim3_out[7] = S.scale();
        for (int i = 0; i < n; i++) removed[i] = matches[(size_t)i] ? 0 : 1;
    }
    return ret;
}
