// rgbd_math.h -- the arithmetic of the RGB-D frame and of the close-point rule, one text for the kernels of rgbd.hip, the library's path without a context and
// cubeslam::Frame / cubeslam::ClosePoints (host/orb_slam_mirrors.hpp, with or without the library).  Reference: orb_object_slam/src/Frame.cc:334-344
// (UpdatePoseMatrices), :785-806 (ComputeStereoFromRGBD), :808-822 (UnprojectStereo); src/Tracking.cc:388 (convertTo), :783-850, :1207-1274, :2067-2130 (the three
// callers of the close-point rule).  Every statement is one float operation in the written order or one double accumulation with one rounding (cv_math.h); the
// library is built with -ffp-contract=off, and so is everything that includes this header for a comparison.
#pragma once
#include <stdint.h>

#include "cv_math.h"

#include <algorithm>
#include <utility>
#include <vector>

enum { RGBD_DEPTH_U16 = 0, RGBD_DEPTH_F32 = 1 };     // = CS_DEPTH_U16 / CS_DEPTH_F32
enum { RGBD_CLOSE_NEAREST = 0, RGBD_CLOSE_ALL = 1 }; // = CS_CLOSE_POINTS_NEAREST / CS_CLOSE_POINTS_ALL
constexpr int RGBD_MIN_WALK = 100;                   // `nPoints > 100` of Tracking.cc:1271 / :2126

// imDepth.at<float>(v, u) with float v, u (Frame.cc:795-798): both convert to int by truncation toward zero, so (-1, 0) is row / column 0.  false: the sample lies
// outside the image (the reference reads beyond the Mat) or a coordinate is NaN.
HD bool rgbd_sample_index(float u, float v, int width, int height, int *col, int *row) {
    if (!(u > -1.0f && u < (float)width && v > -1.0f && v < (float)height)) return false; // NaN fails every comparison
    *col = (int)u; *row = (int)v;
    return true;
}
// imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (Tracking.cc:388) for the one sample that is read: saturate_cast<float>(raw * alpha + 0) -- one float multiply
HD float rgbd_convert_u16(uint16_t raw, float factor) { return (float)raw * factor; }
HD float rgbd_convert_f32(float raw, float factor) { return raw * factor; }
HD float rgbd_sample(const void *image, int type, long pitch_bytes, int col, int row, float factor) {
    const char *r = (const char *)image + (long)row * pitch_bytes;
    return type == RGBD_DEPTH_U16 ? rgbd_convert_u16(((const uint16_t *)r)[col], factor) : rgbd_convert_f32(((const float *)r)[col], factor);
}
// Frame.cc:800-804: d > 0 (NaN is not, +inf is), mvDepth = d, mvuRight = kpU.pt.x - mbf / d; -1 / -1 otherwise (:787-788)
HD bool rgbd_associate(float d, float xu, float bf, float *u_right, float *depth) {
    if (d > 0) { *depth = d; *u_right = xu - bf / d; return true; }
    *depth = -1.0f; *u_right = -1.0f;
    return false;
}

// Frame::UpdatePoseMatrices (Frame.cc:334-344) from the rows of Tcw (3 x 4): mRwc = mRcw.t(), mOw = -mRcw.t() * mtcw = gemm(mRcw, mtcw, -1, GEMM_1_T): per row the
// double sum over k ascending, times -1, one rounding
HD void rgbd_pose_matrices(const float *Tcw, float *Rwc, float *Ow) {
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) { Rwc[r * 3 + k] = Tcw[k * 4 + r]; s += (double)Tcw[k * 4 + r] * (double)Tcw[k * 4 + 3]; }
        Ow[r] = (float)(s * -1.0);
    }
}
// Frame::UnprojectStereo (Frame.cc:808-822) for z > 0: u, v of mvKeysUn; invfx = 1.0f / fx.  z = +inf ends in 0 * inf or inf - inf; the NaN of such an operation is
// the x86 default NaN (sign set), what the reference's host writes, where the GPU would write the one with the sign clear.
HD void rgbd_unproject(float u, float v, float z, float cx, float cy, float invfx, float invfy, const float *Rwc, const float *Ow, float *x3D) {
    const float xc[3] = {(u - cx) * z * invfx, (v - cy) * z * invfy, z};
    gemm3(Rwc, xc, Ow, x3D); // mRwc * x3Dc + mOw
    union { uint32_t u; float f; } nan; nan.u = 0xffc00000u;
    for (int r = 0; r < 3; r++) if (x3D[r] != x3D[r]) x3D[r] = nan.f;
}

// The order of sort(vDepthIdx) on pair<float, int> for z > 0: positive floats, +inf included, order as their bit patterns, and the index breaks ties
HD unsigned long long rgbd_sort_key(float z, int i) {
    union { float f; uint32_t u; } b; b.f = z;
    return ((unsigned long long)b.u << 32) | (uint32_t)i;
}
// How many entries of the sorted list the loops of Tracking.cc:1241-1273 / :2092-2128 process (= nPoints when they end).  nPoints grows by one in either branch,
// so it is j + 1 behind entry j; the depths ascend, so `first > mThDepth` holds exactly from position c = #{z : !(z > mThDepth)} on.  The break is taken behind the
// first j with j >= c and j + 1 > 100, j = max(c, 100), which itself is still processed; without such a j the loop runs to the end.
HD int rgbd_walked(int n_valid, int c) {
    const int stop = (c > RGBD_MIN_WALK ? c : RGBD_MIN_WALK) + 1;
    return n_valid < stop ? n_valid : stop;
}

// ---- host ----
// Frame::ComputeStereoFromRGBD (Frame.cc:785-806) for one frame on the host.  xy / xyU: pt of mvKeys[i] / mvKeysUn[i] at xy[i * stride_floats], [.. + 1].
inline void rgbd_frame_host(const void *image, int type, int width, int height, long pitch_bytes, int n, const float *xy, const float *xyU, int stride_floats, float bf,
                            float factor, float *u_right, float *depth, int *n_with_depth, int *n_outside) {
    int nd = 0, no = 0;
    for (int i = 0; i < n; i++) {
        int col, row;
        float d = -1.0f;
        if (rgbd_sample_index(xy[(size_t)i * stride_floats], xy[(size_t)i * stride_floats + 1], width, height, &col, &row)) d = rgbd_sample(image, type, pitch_bytes, col, row, factor);
        else no++;
        nd += rgbd_associate(d, xyU[(size_t)i * stride_floats], bf, u_right + i, depth + i);
    }
    *n_with_depth = nd; *n_outside = no;
}
// The close-point rule for one frame on the host, written as the reference's loop (the kernel takes rgbd_walked instead).  order: room for n ints; new_idx: n; new_x3D: 3 n.
inline void rgbd_close_points_host(int n, const float *depth, const float *xyU, int stride_floats, const uint8_t *need_new, const float *Tcw, const float *K4, float th_depth,
                                   int mode, int *n_valid, int *order, int *n_walked, int *n_new, int *new_idx, float *new_x3D) {
    float Rwc[9], Ow[3];
    rgbd_pose_matrices(Tcw, Rwc, Ow);
    const float invfx = 1.0f / K4[0], invfy = 1.0f / K4[1];
    std::vector<std::pair<float, int>> vDepthIdx;
    vDepthIdx.reserve((size_t)n);
    for (int i = 0; i < n; i++) if (depth[i] > 0) vDepthIdx.push_back(std::make_pair(depth[i], i));
    if (mode == RGBD_CLOSE_NEAREST) std::sort(vDepthIdx.begin(), vDepthIdx.end());
    int nPoints = 0, created = 0;
    for (size_t j = 0; j < vDepthIdx.size(); j++) {
        const int i = vDepthIdx[j].second;
        order[j] = i;
        if (mode == RGBD_CLOSE_ALL || need_new[i]) {
            new_idx[created] = i;
            rgbd_unproject(xyU[(size_t)i * stride_floats], xyU[(size_t)i * stride_floats + 1], depth[i], K4[2], K4[3], invfx, invfy, Rwc, Ow, new_x3D + 3 * (size_t)created);
            created++;
        }
        nPoints++;
        if (mode == RGBD_CLOSE_NEAREST && vDepthIdx[j].first > th_depth && nPoints > RGBD_MIN_WALK) {
            for (size_t k = j + 1; k < vDepthIdx.size(); k++) order[k] = vDepthIdx[k].second;
            break;
        }
    }
    *n_valid = (int)vDepthIdx.size(); *n_walked = nPoints; *n_new = created;
}
