// object_points_math.h -- the two ways Tracking::CreateNewKeyFrame makes point coordinates out of cuboids, statement by statement in the reference's arithmetic
// (-ffp-contract=off).  HD: the kernels of object_points.hip, its host forms and tests/cpp/object_points_driver.cpp run this text.
//
//   dyn_triangulate_point    one dynamic point of Tracking.cc:2158-2243: the object's motion between the two key frames folded into the second camera, the linear
//                            triangulation of :2217-2232, the distance test of :2235 and PosToObj of :2240
//   od_*                     the object-depth initialisation (Tracking.cc:876-898, :2339-2424, LocalMapping.cc:574-652): candidate test, the limits of :2373-2378, the
//                            Fisher-Yates draws of random_unique / random_unique2 with the walk of :2390-2420, Frame / KeyFrame::UnprojectDepth
//
// Stated definitions, as in triangulate_math.h: cv::SVD::compute is jacobi_vmin4 and x3D / w is float(x_k * (1.0 / w)).  The float norm of :2235 is Eigen's
// Matrix<float, 3, 1>::norm(): sqrt(d0 * d0 + (d1 * d1 + d2 * d2)) in float (the unrolled reduction of a fixed size 3 splits 1 + 2).
#pragma once
#include <stdint.h>

#include <vector>

#include "se3_math.h"
#include "triangulate_math.h"

enum { // the status byte of a dynamic point: 0 = triangulated, or the first test that failed
    DYN_TRIANGULATED = 0,
    DYN_NO_OBSERVATION = 1, // :2167 pixelindLastKf == -1
    DYN_TRACKLET = 2,       // :2191 truth_tracklet_id differs
    DYN_W_ZERO = 3,         // :2228
    DYN_TOO_FAR = 4         // :2235
};

struct DynCam { float Tl[12], Tn[12]; float cx, cy, invfx, invfy; }; // one key-frame pair: the rows of Tcw_last and Tcw_now, the current key frame's intrinsics

HD void dyn_make_cam(const float *Tcw_last, const float *Tcw_now, const float *K4, DynCam *c) {
    for (int i = 0; i < 12; i++) { c->Tl[i] = Tcw_last[i]; c->Tn[i] = Tcw_now[i]; }
    c->cx = K4[2]; c->cy = K4[3];
    c->invfx = 1.0f / K4[0]; c->invfy = 1.0f / K4[1]; // Frame.cc: invfx = 1.0f / fx
}

// :2196-2197  Tcw_now * Converter::toCvMat(cube_pose_now.pose * cube_pose_lastkf.pose.inverse()): rows 0..2 of the product (row 3 is not read)
HD void dyn_object_camera(const float *Tn, const double *pose_now, const double *pose_last, float *Td) {
    const SE3 ot = se3_mul(se3_load(pose_now), se3_inv(se3_load(pose_last)));
    double R[3][3];
    qtoR(ot.r, R); // SE3Quat::to_homogeneous_matrix
    float M[16];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) M[r * 4 + c] = (float)R[r][c]; M[r * 4 + 3] = (float)ot.t[r]; }
    M[12] = 0.f; M[13] = 0.f; M[14] = 0.f; M[15] = 1.f;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += (double)(k < 3 ? Tn[r * 4 + k] : Tn[r * 4 + 3]) * (double)M[k * 4 + c];
            Td[r * 4 + c] = (float)s;
        }
}

// :2217-2221 in float, as cv::addWeighted evaluates the MatExpr on CV_32F
HD void dyn_rows(const DynCam &c, const float *Td, const float *kp1, const float *kp2, double *A) {
    const float xn1[2] = {(kp1[0] - c.cx) * c.invfx, (kp1[1] - c.cy) * c.invfy};
    const float xn2[2] = {(kp2[0] - c.cx) * c.invfx, (kp2[1] - c.cy) * c.invfy};
    for (int k = 0; k < 4; k++) {
        A[k] = (double)(xn1[0] * c.Tl[8 + k] - c.Tl[k]);
        A[4 + k] = (double)(xn1[1] * c.Tl[8 + k] - c.Tl[4 + k]);
        A[8 + k] = (double)(xn2[0] * Td[8 + k] - Td[k]);
        A[12 + k] = (double)(xn2[1] * Td[8 + k] - Td[4 + k]);
    }
}

HD float dyn_norm3f(const float *a, const float *b) {
    const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return sqrtf(d0 * d0 + (d1 * d1 + d2 * d2));
}

// :2226-2240 behind the SVD: v = vt.row(3) in double.  x3D, pto (3 floats each) are zeros unless the status is DYN_TRIANGULATED.
HD int dyn_point_from_v(const double *v, const double *pose_now, const float *world_pos, float *x3D, float *pto) {
    for (int k = 0; k < 3; k++) { x3D[k] = 0.f; pto[k] = 0.f; }
    const float x4[4] = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    if (x4[3] == 0) return DYN_W_ZERO;
    const double invw = 1.0 / (double)x4[3];
    const float x[3] = {(float)((double)x4[0] * invw), (float)((double)x4[1] * invw), (float)((double)x4[2] * invw)};
    if (dyn_norm3f(x, world_pos) > 5) return DYN_TOO_FAR; // (a NaN is not > 5, as in the reference)
    const double xd[3] = {(double)x[0], (double)x[1], (double)x[2]};
    double o[3];
    se3_map(se3_inv(se3_load(pose_now)), xd, o);
    for (int k = 0; k < 3; k++) { x3D[k] = x[k]; pto[k] = (float)o[k]; }
    return DYN_TRIANGULATED;
}

// pose_last / pose_now: 7 doubles (t, qx qy qz qw) of the two cuboids; track_last / track_now: truth_tracklet_id, compared when use_truth is set
HD int dyn_triangulate_point(const DynCam &c, const float *kp1, const float *kp2, int idx_last, const double *pose_last, const double *pose_now, bool use_truth, int track_last,
                             int track_now, const float *world_pos, float *x3D, float *pto) {
    for (int k = 0; k < 3; k++) { x3D[k] = 0.f; pto[k] = 0.f; }
    if (idx_last == -1) return DYN_NO_OBSERVATION;
    if (use_truth && track_last != track_now) return DYN_TRACKLET;
    float Td[12];
    dyn_object_camera(c.Tn, pose_now, pose_last, Td);
    double A[16], v[4];
    dyn_rows(c, Td, kp1, kp2, A);
    jacobi_vmin4(A, v);
    return dyn_point_from_v(v, pose_now, world_pos, x3D, pto);
}

struct DynTables { const int *cub_first_last, *cub_first_now; const double *pose_last, *pose_now; const int *tracklet_last, *tracklet_now; };

// one point; status / x3D / pto / dp are the point's own outputs
HD void dyn_one(const DynCam &cam, int f, const DynTables &T, const float *kp1, const float *kp2, int obj_last, int obj_now, int idx_last, const float *world_pos,
                uint8_t *status, float *x3D, float *pto, double *dp) {
    float x[3], o[3];
    int st;
    if (idx_last == -1) { // the rows of such a point are not read
        st = DYN_NO_OBSERVATION;
        x[0] = x[1] = x[2] = o[0] = o[1] = o[2] = 0.f;
    } else {
        const long rl = (long)T.cub_first_last[f] + obj_last, rn = (long)T.cub_first_now[f] + obj_now;
        const bool use_truth = T.tracklet_last != nullptr;
        st = dyn_triangulate_point(cam, kp1, kp2, idx_last, T.pose_last + 7 * rl, T.pose_now + 7 * rn, use_truth, use_truth ? T.tracklet_last[rl] : 0,
                                   use_truth ? T.tracklet_now[rn] : 0, world_pos, x, o);
    }
    *status = (uint8_t)st;
    for (int k = 0; k < 3; k++) { x3D[k] = x[k]; pto[k] = o[k]; dp[k] = (double)o[k]; }
}

// ---- object-depth initialisation
enum { OD_FIRST_FRAME = 0, OD_TRACKING = 1, OD_LOCAL_MAPPING = 2 };
constexpr int OD_GRID_COLS = 64, OD_GRID_ROWS = 48, OD_NCELL = OD_GRID_COLS * OD_GRID_ROWS; // FRAME_GRID_COLS / FRAME_GRID_ROWS
constexpr int OD_MAX_NEW_TRACKING = 80;                                                       // :2378

struct OdKey { float x, y, size, angle, response; int octave, class_id; }; // cs_keypoint (cv::KeyPoint), 28 bytes
struct OdGrid { float minX, minY, wInv, hInv; };
// bounds = Frame's mnMinX mnMaxX mnMinY mnMaxY (floats).  mfGridElementWidthInv / HeightInv are Frame's (Frame.cc, from the float bounds); KeyFrame::mnMinX and mnMinY are
// `const int` members initialised from them (KeyFrame.h:229-230, KeyFrame.cc:54): KeyFrame::PosInGrid subtracts the TRUNCATED values.  (The entry point refuses bounds that are
// not finite or beyond 1e9.)
HD OdGrid od_make_grid(const float *bounds) {
    OdGrid g;
    g.minX = (float)(int)bounds[0]; g.minY = (float)(int)bounds[2];
    g.wInv = static_cast<float>(OD_GRID_COLS) / static_cast<float>(bounds[1] - bounds[0]);
    g.hInv = static_cast<float>(OD_GRID_ROWS) / static_cast<float>(bounds[3] - bounds[2]);
    return g;
}
// KeyFrame::PosInGrid (KeyFrame.cc:792-802): the cell gridx * ROWS + gridy, or -1 outside
HD int od_cell(const OdGrid &g, float x, float y) {
    const float fx = roundf((x - g.minX) * g.wInv), fy = roundf((y - g.minY) * g.hInv);
    if (!(fx >= 0.f && fx < (float)OD_GRID_COLS && fy >= 0.f && fy < (float)OD_GRID_ROWS)) return -1; // (the comparison in float: the int conversion of a value outside int is not defined)
    return (int)fx * OD_GRID_ROWS + (int)fy;
}
// a key point that may enter has_object_depth_pixel_inds, the grid gate aside (:2350-2362, LocalMapping.cc:596-598); first-frame mode: :883
HD bool od_qualifies(int mode, int has_map_point, int object_id, int octave) {
    if (mode == OD_FIRST_FRAME) return object_id > -1;
    if (has_map_point) return false;
    return object_id > -1 && (mode != OD_TRACKING || octave < 3);
}
// :2373-2378 / LocalMapping.cc:606-611: max_initialize_pts, or -1 when depth_point_ration_now < 0.30 is false
HD int od_max_initialize(int mode, int total, int raw, int n_candidates) {
    const double total_feature_pts = (double)total, raw_depth_pts = (double)raw;
    const double depth_point_ration_now = raw_depth_pts / total_feature_pts;
    if (!(depth_point_ration_now < 0.30)) return -1;
    int m = (int)(total_feature_pts * 0.30) - (int)raw_depth_pts;
    if (n_candidates < m) m = n_candidates;
    if (mode == OD_TRACKING && OD_MAX_NEW_TRACKING < m) m = OD_MAX_NEW_TRACKING;
    return m < 0 ? 0 : m; // (never negative when the test above holds; the reference's loops do not end on a negative count)
}
// random_unique / random_unique2 over cand[0 .. n) with the caller's rand() values (n_shuffle of them, each >= 0), then the walk of :2390-2420 up to max_init points:
// returns the number of points, their key points in new_idx.  object_id, cub_depth: the frame's own.
HD int od_shuffle_walk(int *cand, int n, int n_shuffle, int max_init, const int *draws, const int *object_id, const float *cub_depth, int *new_idx) {
    int left = n;
    for (int b = 0; b < n_shuffle; b++, left--) {
        const int r = b + (int)((unsigned)draws[b] % (unsigned)left);
        const int t = cand[b]; cand[b] = cand[r]; cand[r] = t;
    }
    int nPoints = 0;
    for (int vc = 0; nPoints < max_init && vc < n; vc++) {
        const int pixel_ind = cand[vc];
        if (cub_depth[object_id[pixel_ind]] > 0) new_idx[nPoints++] = pixel_ind;
    }
    return nPoints;
}
// Frame::UnprojectDepth (Frame.cc:824-838) / KeyFrame::UnprojectDepth (KeyFrame.cc:693-709) for z > 0: Twc = the 3 x 4 rows of [Rwc | Ow]
HD void od_unproject(float u, float v, float z, const float *K4, const float *Twc, float *x3D) {
    const float invfx = 1.0f / K4[0], invfy = 1.0f / K4[1];
    const float xc[3] = {(u - K4[2]) * z * invfx, (v - K4[3]) * z * invfy, z};
    for (int r = 0; r < 3; r++) {
        double sacc = 0;
        for (int k = 0; k < 3; k++) sacc += (double)Twc[r * 4 + k] * (double)xc[k];
        x3D[r] = (float)(sacc * 1.0 + (double)Twc[r * 4 + 3] * 1.0);
    }
}

// one frame's counts as the kernel and the host walk leave them
struct OdFrameOut { int n_candidates, raw_depth_pts, max_initialize_pts, n_new, short_of_draws; };

// the same frame as the reference walks it (the comparison side): the sequential loop with gridsHasMappt
inline void od_frame_host(int mode, int N, const OdKey *keys, const uint8_t *has_mp, const int *object_id, const float *cub_depth, const float *K4, const float *bounds,
                          const float *Twc, int n_draws, const int *draws, OdFrameOut *out, int *candidates, int *shuffled, int *new_idx, float *new_x3D) {
    std::vector<uint8_t> taken(mode == OD_TRACKING ? OD_NCELL : 0, 0);
    const OdGrid G = mode == OD_TRACKING ? od_make_grid(bounds) : OdGrid{0.f, 0.f, 0.f, 0.f};
    int n_cand = 0, raw = 0;
    for (int i = 0; i < N; i++) {
        const int mp = has_mp ? has_mp[i] : 0;
        if (mode != OD_FIRST_FRAME && mp) { raw++; continue; }
        int c = -1;
        if (mode == OD_TRACKING) {
            c = od_cell(G, keys[i].x, keys[i].y);
            if (c < 0 || taken[c]) continue;
        }
        if (!od_qualifies(mode, mp, object_id[i], keys[i].octave)) continue;
        candidates[n_cand] = shuffled[n_cand] = i; n_cand++;
        if (c >= 0) taken[c] = 1;
    }
    int max_init, nn = 0, lacking = 0;
    if (mode == OD_FIRST_FRAME) {
        max_init = n_cand;
        nn = od_shuffle_walk(shuffled, n_cand, 0, n_cand, nullptr, object_id, cub_depth, new_idx);
    } else {
        max_init = od_max_initialize(mode, N, raw, n_cand);
        if (max_init > n_draws) lacking = 1;
        else if (max_init > 0) nn = od_shuffle_walk(shuffled, n_cand, max_init, max_init, draws, object_id, cub_depth, new_idx);
    }
    *out = OdFrameOut{n_cand, raw, max_init, nn, lacking};
    for (int j = 0; j < nn; j++) od_unproject(keys[new_idx[j]].x, keys[new_idx[j]].y, cub_depth[object_id[new_idx[j]]], K4, Twc, new_x3D + 3 * (size_t)j);
}

