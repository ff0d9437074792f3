// triangulate_math.h -- one matched pair of LocalMapping::CreateNewMapPoints (LocalMapping.cc:410-549), statement by statement in the reference's float arithmetic (cv_math.h
// for the cv::Mat forms; -ffp-contract=off).  HD: the kernel of localmap.hip and tests/cpp/local_mapping_driver.cpp run this text.
//
// Two operations are the library's own definition, because the reference's result depends on the OpenCV and libm it was built with:
//   * cv::SVD::compute (:448): the right singular vector of the smallest singular value of A, by a one-sided Jacobi in double with a fixed sweep order, a fixed convergence
//     test and + - * / sqrt only (jacobi_vmin4), rounded to float; :452-456 then run in float with x3D / w as float(x_k * (1.0 / w)).
//   * cos(2 * atan2(mb / 2, depth)) (:431, :433): (d^2 - h^2) / (d^2 + h^2) with h = mb / 2 in double, rounded once (cos_stereo).
#pragma once
#include "cv_math.h"

enum { // the status byte of a pair: 0 = a point is created, or the first test that failed
    TRI_CREATED = 0,
    TRI_PARALLAX = 1,       // :467 no stereo and very low parallax
    TRI_W_ZERO = 2,         // :452
    TRI_Z1 = 3,             // :473
    TRI_Z2 = 4,             // :477
    TRI_REPROJ1 = 5,        // :492 / :503
    TRI_REPROJ2 = 6,        // :518 / :529
    TRI_ZERO_DIST = 7,      // :540
    TRI_SCALE = 8,          // :548
    TRI_CLAIMED = 9,        // an earlier neighbour created the point of this idx1 (the reference's search would have skipped idx1)
    TRI_STEREO_NO_DEPTH = 10 // :460 / :464 with mvDepth <= 0: KeyFrame::UnprojectStereo returns an empty Mat, which the reference goes on to read
};

struct TriCam { float Rcw[9], tcw[3], Ow[3], Rwc[9]; float fx, fy, cx, cy, invfx, invfy, mbf, mb; };
struct TriObs { float ux, uy;        // mvKeysUn[idx].pt
                float kx, ky;        // mvKeys[idx].pt (KeyFrame::UnprojectStereo reads the distorted key point)
                float ur, depth;     // mvuRight[idx], mvDepth[idx]
                float sigma2, scale; // mvLevelSigma2[octave], mvScaleFactors[octave]
};

HD void tri_make_cam(const float *Rcw, const float *tcw, const float *Ow, float fx, float fy, float cx, float cy, float invfx, float invfy, float mbf, float mb, TriCam *c) {
    for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) { c->Rcw[r * 3 + k] = Rcw[r * 3 + k]; c->Rwc[k * 3 + r] = Rcw[r * 3 + k]; } // Rwc = Rcw.t(): a copy
    for (int k = 0; k < 3; k++) { c->tcw[k] = tcw[k]; c->Ow[k] = Ow[k]; }
    c->fx = fx; c->fy = fy; c->cx = cx; c->cy = cy; c->invfx = invfx; c->invfy = invfy; c->mbf = mbf; c->mb = mb;
}

// Right singular vector of the smallest singular value of the row-major 4x4 A (Hestenes' one-sided Jacobi on the columns).  Sweeps visit (p, q) = (0,1) (0,2) (0,3) (1,2)
// (1,3) (2,3); a pair is rotated unless |a_p . a_q| <= 2^-50 sqrt(|a_p|^2 |a_q|^2); the iteration ends with the first sweep that rotates nothing, or after 30.  The smallest
// column norm wins, the first one among equals.  The sign of the vector is whatever the rotations leave: :452-456 do not depend on it.
constexpr int TRI_JACOBI_MAX_SWEEPS = 30;
HD void jacobi_vmin4(const double *A, double *v) {
    double W[16], V[16];
    for (int i = 0; i < 16; i++) { W[i] = A[i]; V[i] = (i % 5 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < TRI_JACOBI_MAX_SWEEPS; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int r = 0; r < 4; r++) { alpha += W[r * 4 + p] * W[r * 4 + p]; beta += W[r * 4 + q] * W[r * 4 + q]; gamma += W[r * 4 + p] * W[r * 4 + q]; }
                const double ag = gamma < 0 ? -gamma : gamma;
                if (ag <= 8.8817841970012523e-16 * sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double az = zeta < 0 ? -zeta : zeta;
                const double t = (zeta < 0 ? -1.0 : 1.0) / (az + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 4; r++) {
                    const double wp = W[r * 4 + p], wq = W[r * 4 + q];
                    W[r * 4 + p] = c * wp - s * wq; W[r * 4 + q] = s * wp + c * wq;
                    const double vp = V[r * 4 + p], vq = V[r * 4 + q];
                    V[r * 4 + p] = c * vp - s * vq; V[r * 4 + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    int best = 0; double nbest = 0;
    for (int k = 0; k < 4; k++) {
        double n = 0;
        for (int r = 0; r < 4; r++) n += W[r * 4 + k] * W[r * 4 + k];
        if (k == 0 || n < nbest) { best = k; nbest = n; }
    }
    for (int r = 0; r < 4; r++) v[r] = V[r * 4 + best];
}

HD float cos_stereo(float mb, float depth) {
    const double h = (double)mb / 2.0, d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}

// u, v (and u_r) of x3D in one key frame against its key point: true = the chi-square test fails (:480-505 / :507-531; mbf is the CURRENT key frame's in both, :498 and :524)
HD bool tri_reproj_fails(const TriCam &c, const TriObs &o, bool stereo, const float *x3D, float z, float mbf) {
    const float x = (float)(dot3_f64(c.Rcw + 0, x3D) + (double)c.tcw[0]);
    const float y = (float)(dot3_f64(c.Rcw + 3, x3D) + (double)c.tcw[1]);
    const float invz = (float)(1.0 / (double)z);
    const float u = c.fx * x * invz + c.cx;
    const float v = c.fy * y * invz + c.cy;
    const float errX = u - o.ux, errY = v - o.uy;
    if (!stereo) return (double)(errX * errX + errY * errY) > 5.991 * (double)o.sigma2;
    const float u_r = u - mbf * invz;
    const float errX_r = u_r - o.ur;
    return (double)(errX * errX + errY * errY + errX_r * errX_r) > 7.8 * (double)o.sigma2;
}

// x3D is written where the reference has one (every status but TRI_PARALLAX, TRI_W_ZERO and TRI_STEREO_NO_DEPTH, where it is 0 0 0)
HD int triangulate_pair(const TriCam &c1, const TriObs &o1, const TriCam &c2, const TriObs &o2, float ratioFactor, float *x3D) {
    x3D[0] = x3D[1] = x3D[2] = 0.f;
    const bool bStereo1 = o1.ur >= 0, bStereo2 = o2.ur >= 0;
    const float xn1[3] = {(o1.ux - c1.cx) * c1.invfx, (o1.uy - c1.cy) * c1.invfy, 1.0f};
    const float xn2[3] = {(o2.ux - c2.cx) * c2.invfx, (o2.uy - c2.cy) * c2.invfy, 1.0f};
    const float zero[3] = {0.f, 0.f, 0.f};
    float ray1[3], ray2[3];
    gemm3(c1.Rwc, xn1, zero, ray1);
    gemm3(c2.Rwc, xn2, zero, ray2);
    const float cosParallaxRays = (float)(dot3_f64(ray1, ray2) / (norm3_f64(ray1) * norm3_f64(ray2)));
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = cos_stereo(c1.mb, o1.depth);
    else if (bStereo2) cosParallaxStereo2 = cos_stereo(c2.mb, o2.depth);
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1; // std::min
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        double A[16];
        for (int k = 0; k < 4; k++) { // rows of Tcw = [Rcw | tcw]; xn * row(2) - row(r) as cv::addWeighted evaluates the MatExpr on CV_32F (OpenCV 2.4 - 3.x): float multiply, float add
            const float T1_0 = k < 3 ? c1.Rcw[k] : c1.tcw[0], T1_1 = k < 3 ? c1.Rcw[3 + k] : c1.tcw[1], T1_2 = k < 3 ? c1.Rcw[6 + k] : c1.tcw[2];
            const float T2_0 = k < 3 ? c2.Rcw[k] : c2.tcw[0], T2_1 = k < 3 ? c2.Rcw[3 + k] : c2.tcw[1], T2_2 = k < 3 ? c2.Rcw[6 + k] : c2.tcw[2];
            A[k] = (double)(xn1[0] * T1_2 - T1_0);
            A[4 + k] = (double)(xn1[1] * T1_2 - T1_1);
            A[8 + k] = (double)(xn2[0] * T2_2 - T2_0);
            A[12 + k] = (double)(xn2[1] * T2_2 - T2_1);
        }
        double vd[4];
        jacobi_vmin4(A, vd);
        const float x4[4] = {(float)vd[0], (float)vd[1], (float)vd[2], (float)vd[3]};
        if (x4[3] == 0) return TRI_W_ZERO;
        const double invw = 1.0 / (double)x4[3];
        for (int k = 0; k < 3; k++) x3D[k] = (float)((double)x4[k] * invw);
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        if (!(o1.depth > 0)) return TRI_STEREO_NO_DEPTH;
        const float xc[3] = {(o1.kx - c1.cx) * o1.depth * c1.invfx, (o1.ky - c1.cy) * o1.depth * c1.invfy, o1.depth};
        gemm3(c1.Rwc, xc, c1.Ow, x3D); // Twc.rowRange(0, 3).colRange(0, 3) * x3Dc + Twc.rowRange(0, 3).col(3)
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        if (!(o2.depth > 0)) return TRI_STEREO_NO_DEPTH;
        const float xc[3] = {(o2.kx - c2.cx) * o2.depth * c2.invfx, (o2.ky - c2.cy) * o2.depth * c2.invfy, o2.depth};
        gemm3(c2.Rwc, xc, c2.Ow, x3D);
    } else
        return TRI_PARALLAX;

    const float z1 = (float)(dot3_f64(c1.Rcw + 6, x3D) + (double)c1.tcw[2]);
    if (z1 <= 0) return TRI_Z1;
    const float z2 = (float)(dot3_f64(c2.Rcw + 6, x3D) + (double)c2.tcw[2]);
    if (z2 <= 0) return TRI_Z2;
    if (tri_reproj_fails(c1, o1, bStereo1, x3D, z1, c1.mbf)) return TRI_REPROJ1;
    if (tri_reproj_fails(c2, o2, bStereo2, x3D, z2, c1.mbf)) return TRI_REPROJ2;

    const float normal1[3] = {x3D[0] - c1.Ow[0], x3D[1] - c1.Ow[1], x3D[2] - c1.Ow[2]};
    const float dist1 = norm3(normal1);
    const float normal2[3] = {x3D[0] - c2.Ow[0], x3D[1] - c2.Ow[1], x3D[2] - c2.Ow[2]};
    const float dist2 = norm3(normal2);
    if (dist1 == 0 || dist2 == 0) return TRI_ZERO_DIST;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = o1.scale / o2.scale;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return TRI_SCALE;
    return TRI_CREATED;
}

// MapPoint::UpdateNormalAndDepth (MapPoint.cc:487-509) for one point: obs = the key-frame indices of its observations in the order of mObservations.  normali / cv::norm and
// normal / n are cv::MatExpr scale operations: float(v_k * (1.0 / s)) with s in double (the same stated definition as x3D / w above).
HD void mappoint_normal_depth(const float *pos, const int *obs, int n_obs, const float *kf_Ow, int ref_kf, float level_scale, float top_scale, float *normal, float *min_distance,
                              float *max_distance) {
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < n_obs; j++) {
        const float *Owi = kf_Ow + 3 * (long)obs[j];
        const float normali[3] = {pos[0] - Owi[0], pos[1] - Owi[1], pos[2] - Owi[2]};
        const double inv = 1.0 / norm3_f64(normali);
        for (int k = 0; k < 3; k++) acc[k] = acc[k] + (float)((double)normali[k] * inv);
    }
    const float *Or = kf_Ow + 3 * (long)ref_kf;
    const float PC[3] = {pos[0] - Or[0], pos[1] - Or[1], pos[2] - Or[2]};
    const float dist = norm3(PC);
    const float maxd = dist * level_scale;
    *max_distance = maxd;
    *min_distance = maxd / top_scale;
    const double invn = 1.0 / (double)n_obs;
    for (int k = 0; k < 3; k++) normal[k] = (float)((double)acc[k] * invn);
}
