// TEST INFRASTRUCTURE: stand-ins for the SLAM classes that MapPoint::ComputeDistinctiveDescriptors (orb_object_slam/src/MapPoint.cc:381-446) and MapPoint::UpdateNormalAndDepth
// (:469-510) touch.  tests/test_local_mapping_restatement_pins.py cuts the two methods and ORBmatcher::DescriptorDistance out of the reference at test time into a temporary
// directory (ref_local_mapping_extracted.inc), compiles this file around them there and runs them next to tests/local_mapping_restatement.py on the same inputs.  MapPoint and
// KeyFrame carry just the members those methods read, under the reference's names; every statement of the two methods is the reference's.  Key frames live in one array, so the
// pointer order of std::map<KeyFrame *, size_t> is their index order: the caller's observation order.
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "cvshim.hpp"

// ---- float matrices the way cv::MatExpr evaluates them: Mat +- Mat in float; Mat / s scales every element by 1.0 / s in double with one rounding (the library's stated
// definition of that operation); cv::norm accumulates in double
namespace cv {
inline Mat scaled(const Mat &m, double s) { Mat r(m.rows, m.cols, CV_32F); for (int i = 0; i < m.rows; i++) r.at<float>(i, 0) = (float)((double)m.at<float>(i, 0) * s); return r; }
inline Mat operator/(const Mat &m, double s) { return scaled(m, 1.0 / s); }
inline Mat operator-(const Mat &a, const Mat &b) { Mat r(a.rows, a.cols, CV_32F); for (int i = 0; i < a.rows; i++) r.at<float>(i, 0) = a.at<float>(i, 0) - b.at<float>(i, 0); return r; } // 3 x 1 CV_32F
inline Mat operator+(const Mat &a, const Mat &b) { Mat r(a.rows, a.cols, CV_32F); for (int i = 0; i < a.rows; i++) r.at<float>(i, 0) = a.at<float>(i, 0) + b.at<float>(i, 0); return r; }
inline double norm(const Mat &m) { double s = 0; for (int i = 0; i < m.rows; i++) s += (double)m.at<float>(i, 0) * (double)m.at<float>(i, 0); return std::sqrt(s); }
} // namespace cv

namespace ORB_SLAM2 {
using namespace std;

class KeyFrame {
  public:
    cv::Mat Ow, mDescriptors;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    bool bad = false;
    bool isBad() { return bad; }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
};
class ORBmatcher {
  public:
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b);
};
class MapPoint {
  public:
    std::map<KeyFrame *, size_t> mObservations;
    KeyFrame *mpRefKF = nullptr;
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    bool mbBad = false;
    std::mutex mMutexFeatures, mMutexPos;
    void ComputeDistinctiveDescriptors();
    void UpdateNormalAndDepth();
};

#include "ref_local_mapping_extracted.inc"

} // namespace ORB_SLAM2

extern "C" {
using namespace ORB_SLAM2;
// :381-446 for n_points points; the observations of point p are rows obs_off[p] .. obs_off[p + 1] of desc (32 bytes each), bad[row] = pKF->isBad().  best[p] = the row within
// the run's NOT-bad rows whose descriptor mDescriptor equals afterwards (the first such row), -1 when mDescriptor stayed empty.
void pin_distinctive(int n_points, const int *obs_off, const unsigned char *desc, const unsigned char *bad, int *best) {
    for (int p = 0; p < n_points; p++) {
        const int n = obs_off[p + 1] - obs_off[p];
        std::vector<KeyFrame> kfs((size_t)n);
        MapPoint mp;
        for (int j = 0; j < n; j++) {
            kfs[j].mDescriptors = cv::Mat(1, 32, CV_8U);
            memcpy(kfs[j].mDescriptors.data, desc + 32 * (size_t)(obs_off[p] + j), 32);
            kfs[j].bad = bad && bad[obs_off[p] + j];
            mp.mObservations[&kfs[j]] = 0;
        }
        mp.ComputeDistinctiveDescriptors();
        best[p] = -1;
        if (mp.mDescriptor.empty()) continue;
        int k = 0;
        for (int j = 0; j < n; j++) {
            if (kfs[j].bad) continue;
            if (!memcmp(mp.mDescriptor.data, kfs[j].mDescriptors.data, 32)) { best[p] = k; break; }
            k++;
        }
    }
}
// :469-510 for n_points points over a table of n_kf key frames (camera centres kf_Ow, one scale table for all); outputs are left as they are for a point without observations
void pin_normal_depth(int n_points, const float *world_pos, const int *obs_off, const int *obs_kf, int n_kf, const float *kf_Ow, const int *ref_kf, const int *ref_octave,
                      const float *scale_factors, int n_levels, float *normal, float *min_distance, float *max_distance) {
    std::vector<KeyFrame> kfs((size_t)n_kf);
    for (int k = 0; k < n_kf; k++) {
        kfs[k].Ow = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) kfs[k].Ow.at<float>(c, 0) = kf_Ow[3 * k + c];
        kfs[k].mvScaleFactors.assign(scale_factors, scale_factors + n_levels);
        kfs[k].mnScaleLevels = n_levels;
        kfs[k].mvKeysUn.resize(1);
    }
    for (int p = 0; p < n_points; p++) {
        MapPoint mp;
        mp.mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) mp.mWorldPos.at<float>(c, 0) = world_pos[3 * p + c];
        for (int o = obs_off[p]; o < obs_off[p + 1]; o++) mp.mObservations[&kfs[obs_kf[o]]] = 0; // (key point 0 of every key frame; its octave is set below for the reference one)
        if (mp.mObservations.empty()) { mp.UpdateNormalAndDepth(); continue; }
        mp.mpRefKF = &kfs[ref_kf[p]];
        mp.mpRefKF->mvKeysUn[0].octave = ref_octave[p];
        mp.UpdateNormalAndDepth();
        for (int c = 0; c < 3; c++) normal[3 * p + c] = mp.mNormalVector.at<float>(c, 0);
        min_distance[p] = mp.mfMinDistance; max_distance[p] = mp.mfMaxDistance;
    }
}
}
