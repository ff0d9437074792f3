// TEST INFRASTRUCTURE: stand-ins for the SLAM classes that the reference's Optimizer::OptimizeEssentialGraph (orb_object_slam/src/Optimizer.cc:2575-2836) touches.
// tests/test_essential_graph_restatement_pins.py cuts that function out of the reference at test time into a temporary directory (ref_essential_graph_extracted.inc),
// compiles this file around it there against the reference's vendored g2o headers (oracle/ref_shim/eigen_full for Eigen, oracle/ref_shim/cvshim.hpp for cv::Mat,
// oracle/ref_shim/g2o_shadow for linear_solver_eigen.h), links it with types_seven_dof_expmap.cpp and the g2o objects of oracle/_ref, and runs it next to
// tests/essential_graph_restatement.py on the same maps.  KeyFrame, MapPoint, Map, LoopClosing and Converter carry just the members that function reads, under the
// reference's names; every statement of the optimisation is the reference's.  Key frames live in one array, so a std::set<KeyFrame *> iterates in array order.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <map>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "cvshim.hpp"

#include <Eigen/Core>
#include <Eigen/Dense>
#include <Eigen/Geometry>
#include <Eigen/StdVector>

#include "Thirdparty/g2o/g2o/core/block_solver.h"
#include "Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.h"
#include "Thirdparty/g2o/g2o/solvers/linear_solver_eigen.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"

namespace ORB_SLAM2 {
using namespace std;

class KeyFrame {
  public:
    long unsigned int mnId = 0;
    cv::Mat Rcw, tcw, Tiw; // Tiw: what SetPose received
    KeyFrame *parent = nullptr;
    std::set<KeyFrame *> children, loop_edges;
    std::vector<KeyFrame *> covisibles;
    std::map<KeyFrame *, int> weights;
    bool bad = false;
    bool isBad() { return bad; }
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    KeyFrame *GetParent() { return parent; }
    std::set<KeyFrame *> GetLoopEdges() { return loop_edges; }
    std::vector<KeyFrame *> GetCovisiblesByWeight(const int &) { return covisibles; } // the caller hands over the list at weight 100
    bool hasChild(KeyFrame *pKF) { return children.count(pKF) != 0; }
    int GetWeight(KeyFrame *pKF) { return weights.count(pKF) ? weights[pKF] : 0; } // KeyFrame.cc
    g2o::Sim3 estimate; // the vertex estimate the pose was recovered from
    void SetPoseLogged(const g2o::Sim3 &S, const cv::Mat &T) { estimate = S; Tiw = T.clone(); }
};
class MapPoint {
  public:
    cv::Mat mWorldPos;
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    KeyFrame *ref = nullptr;
    bool bad = false;
    bool isBad() { return bad; }
    KeyFrame *GetReferenceKeyFrame() { return ref; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &p) { mWorldPos = p.clone(); }
    void UpdateNormalAndDepth() {}
};
class Map {
  public:
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> mps;
    std::mutex mMutexMapUpdate;
    std::vector<KeyFrame *> GetAllKeyFrames() { return kfs; }
    std::vector<MapPoint *> GetAllMapPoints() { return mps; }
    long unsigned int GetMaxKFid() { long unsigned int m = 0; for (KeyFrame *k : kfs) m = std::max(m, k->mnId); return m; }
};
class LoopClosing {
  public:
    typedef map<KeyFrame *, g2o::Sim3, std::less<KeyFrame *>, Eigen::aligned_allocator<std::pair<KeyFrame *const, g2o::Sim3>>> KeyFrameAndPose;
};
class Converter {
  public:
    static Eigen::Matrix<double, 3, 3> toMatrix3d(const cv::Mat &m) {
        Eigen::Matrix<double, 3, 3> M;
        M << m.at<float>(0, 0), m.at<float>(0, 1), m.at<float>(0, 2), m.at<float>(1, 0), m.at<float>(1, 1), m.at<float>(1, 2), m.at<float>(2, 0), m.at<float>(2, 1), m.at<float>(2, 2);
        return M;
    }
    static Eigen::Matrix<double, 3, 1> toVector3d(const cv::Mat &v) {
        Eigen::Matrix<double, 3, 1> r;
        r << v.at<float>(0), v.at<float>(1), v.at<float>(2);
        return r;
    }
    static cv::Mat toCvSE3(const Eigen::Matrix<double, 3, 3> &R, const Eigen::Matrix<double, 3, 1> &t) {
        cv::Mat m(4, 4, CV_32F);
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) m.at<float>(i, j) = i == j ? 1.f : 0.f;
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) m.at<float>(i, j) = R(i, j); m.at<float>(i, 3) = t(i); }
        return m.clone();
    }
    static cv::Mat toCvMat(const Eigen::Matrix<double, 3, 1> &v) {
        cv::Mat m(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) m.at<float>(i) = v(i);
        return m.clone();
    }
};
class Optimizer {
  public:
    void static OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3, const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                       const map<KeyFrame *, set<KeyFrame *>> &LoopConnections, const bool &bFixScale);
};

// every edge the function hands to optimizer.addEdge, in that order: (id of vertex 0, id of vertex 1)
static std::vector<std::pair<int, int>> g_edge_log;
static g2o::EdgeSim3 *pin_log_edge(g2o::EdgeSim3 *e) {
    g_edge_log.push_back(std::make_pair(e->vertex(0) ? e->vertex(0)->id() : -1, e->vertex(1) ? e->vertex(1)->id() : -1));
    return e;
}
#define addEdge(e) addEdge(pin_log_edge(e))
#define setVerbose(v) setVerbose(true) // g2o then prints one line per iteration on std::cerr (levenbergIter= the trials it took) and computes nothing else differently
#define SetPose(T) SetPoseLogged(CorrectedSiw, T) // pKFi->SetPose(Tiw) at :2802, where CorrectedSiw is the vertex estimate: the function hands the Sim3 out nowhere else
#include "ref_essential_graph_extracted.inc"
#undef SetPose
#undef setVerbose
#undef addEdge
} // namespace ORB_SLAM2

using namespace ORB_SLAM2;

static g2o::Sim3 sim3_of(const double *p) { return g2o::Sim3(Eigen::Quaterniond(p[6], p[3], p[4], p[5]), Eigen::Vector3d(p[0], p[1], p[2]), p[7]); }

// One map in flat arrays; key frame k of the arrays is &kf[k], so "address order" is array order.  Lists are CSR (off, values) of array indices.
extern "C" __attribute__((visibility("default"))) int pin_essential_graph(
    int n, int n_extra /* bad key frames behind the n of the map: only covisibles point at them */, const int *mnid, const float *pose /* n x 12: Rcw row-major, tcw */, const int *parent, const int *ch_off, const int *ch, const int *le_off, const int *le, const int *cv_off,
    const int *cvl, const int *w_off, const int *w_kf, const int *w_val, int n_lc, const int *lc_keys, const int *lc_off, const int *lc, int n_cor, const int *cor_idx, const double *cor,
    int n_nc, const int *nc_idx, const double *nc, int loop_kf, int cur_kf, int fix_scale, int n_pts, const float *ppos, const int *pref, const int *pby, const int *pcr, int repeats,
    double *sim3_out, float *Tiw_out, float *pts_out, int edge_cap, int *edges, int *n_edges, double *seconds,
    int *n_iterations, int *trials_per_iteration /* 64 */) {
    double best = 1e300;
    int overflow = 0;
    for (int rep = 0; rep < (repeats > 0 ? repeats : 1); rep++) {
        std::vector<KeyFrame> kf((size_t)(n + n_extra));
        for (int k = n; k < n + n_extra; k++) { kf[(size_t)k].mnId = (long unsigned int)mnid[k]; kf[(size_t)k].bad = true; }
        std::vector<MapPoint> mp((size_t)n_pts);
        Map map;
        for (int k = 0; k < n; k++) {
            KeyFrame &K = kf[(size_t)k];
            K.mnId = (long unsigned int)mnid[k];
            K.Rcw = cv::Mat(3, 3, CV_32F); K.tcw = cv::Mat(3, 1, CV_32F);
            for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) K.Rcw.at<float>(i, j) = pose[k * 12 + i * 3 + j]; K.tcw.at<float>(i) = pose[k * 12 + 9 + i]; }
            if (parent[k] >= 0) K.parent = &kf[(size_t)parent[k]];
            for (int q = ch_off[k]; q < ch_off[k + 1]; q++) K.children.insert(&kf[(size_t)ch[q]]);
            for (int q = le_off[k]; q < le_off[k + 1]; q++) K.loop_edges.insert(&kf[(size_t)le[q]]);
            for (int q = cv_off[k]; q < cv_off[k + 1]; q++) K.covisibles.push_back(&kf[(size_t)cvl[q]]);
            for (int q = w_off[k]; q < w_off[k + 1]; q++) K.weights[&kf[(size_t)w_kf[q]]] = w_val[q];
            map.kfs.push_back(&K);
        }
        for (int p = 0; p < n_pts; p++) {
            MapPoint &M = mp[(size_t)p];
            M.mWorldPos = cv::Mat(3, 1, CV_32F);
            for (int i = 0; i < 3; i++) M.mWorldPos.at<float>(i) = ppos[p * 3 + i];
            M.ref = &kf[(size_t)pref[p]]; M.mnCorrectedByKF = (long unsigned int)(long)pby[p]; M.mnCorrectedReference = (long unsigned int)(long)pcr[p];
            map.mps.push_back(&M);
        }
        LoopClosing::KeyFrameAndPose corrected, non_corrected;
        for (int q = 0; q < n_cor; q++) corrected[&kf[(size_t)cor_idx[q]]] = sim3_of(cor + q * 8);
        for (int q = 0; q < n_nc; q++) non_corrected[&kf[(size_t)nc_idx[q]]] = sim3_of(nc + q * 8);
        std::map<KeyFrame *, std::set<KeyFrame *>> connections;
        for (int q = 0; q < n_lc; q++) for (int s = lc_off[q]; s < lc_off[q + 1]; s++) connections[&kf[(size_t)lc_keys[q]]].insert(&kf[(size_t)lc[s]]);
        g_edge_log.clear();
        const bool fix = fix_scale != 0;
        std::ostringstream said;
        std::streambuf *was = std::cerr.rdbuf(said.rdbuf());
        const auto t0 = std::chrono::steady_clock::now();
        Optimizer::OptimizeEssentialGraph(&map, &kf[(size_t)loop_kf], &kf[(size_t)cur_kf], non_corrected, corrected, connections, fix);
        best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        std::cerr.rdbuf(was);
        *n_iterations = 0;
        const std::string text = said.str(), key = "levenbergIter= ";
        for (size_t at = text.find(key); at != std::string::npos; at = text.find(key, at + 1)) {
            if (*n_iterations < 64) trials_per_iteration[*n_iterations] = std::atoi(text.c_str() + at + key.size());
            (*n_iterations)++;
        }
        for (int k = 0; k < n; k++) for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) Tiw_out[k * 12 + i * 4 + j] = kf[(size_t)k].Tiw.at<float>(i, j);
        for (int k = 0; k < n; k++) {
            const g2o::Sim3 &S = kf[(size_t)k].estimate;
            for (int i = 0; i < 3; i++) sim3_out[k * 8 + i] = S.translation()[i];
            for (int i = 0; i < 4; i++) sim3_out[k * 8 + 3 + i] = S.rotation().coeffs()[i];
            sim3_out[k * 8 + 7] = S.scale();
        }
        for (int p = 0; p < n_pts; p++) for (int i = 0; i < 3; i++) pts_out[p * 3 + i] = mp[(size_t)p].mWorldPos.at<float>(i);
        *n_edges = (int)g_edge_log.size();
        if (*n_edges > edge_cap) overflow = 1;
        for (int e = 0; e < *n_edges && e < edge_cap; e++) { edges[e * 2] = g_edge_log[(size_t)e].first; edges[e * 2 + 1] = g_edge_log[(size_t)e].second; }
    }
    *seconds = best;
    return overflow;
}
