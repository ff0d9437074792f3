// horn_math.h -- one hypothesis and one correspondence test of Sim3Solver (orb_object_slam/src/Sim3Solver.cc): ComputeCentroid (:213-222), ComputeSim3 (Horn 1987, :224-334),
// Project (:377-398), FromCameraToImage (:400-418) and the test of CheckInliers (:346-352), statement by statement in the reference's float arithmetic (cv_math.h for the cv::Mat
// forms; -ffp-contract=off).  HD: the kernel of sim3solver.hip, its CPU path and the g++ builds of the tests run this text.
//
// The cv::Mat forms as they are evaluated here: cv::reduce(SUM) of a CV_32F row adds left to right in float; Mat / n and s * Mat scale every element by a double with one
// rounding, float(v * (1.0 / n)) and float(v * s); a product with a scale and an addend, O1 - s * R * O2, is one gemm, float(-s * sum_k + O1_r), the sum in double over k
// ascending; Mat::dot accumulates in double in row-major order; cv::pow(P, 2) multiplies in float.
//
// Two operations are the library's own definition, because the reference's result depends on the OpenCV and libm it was built with (INTEGRATION.md 8b'):
//   * cv::eigen (:269): the eigenvector of the largest eigenvalue of the float symmetric 4x4 N, by a cyclic two-sided Jacobi in double with a fixed pair order, the
//     rotate-unless-negligible test and the stop rule of jacobi_vmin4 (triangulate_math.h) and + - * / sqrt only (jacobi_vmax4_sym); the largest diagonal entry wins, the first
//     among equals.  The vector stays in double.
//   * atan2 + cv::Rodrigues (:275-281): R = I + (2 w [v]x + 2 [v]x^2) / (q . q) from that eigenvector q = (w, v) in double, each element rounded once to float (horn_rotation).
//     That is what :275-281 compute, it does not depend on the sign of q and evaluates no transcendental.  Where v is exactly zero the reference divides 0 by 0 at :277: R is NaN.
#pragma once
#include "cv_math.h"

constexpr int HORN_JACOBI_MAX_SWEEPS = 30;

// Eigenvector of the largest eigenvalue of the symmetric row-major 4x4 A.  Sweeps visit (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair is rotated unless
// |a_pq| <= 2^-50 sqrt(|a_p|^2 |a_q|^2) with a_p, a_q the columns p and q of the current matrix; the iteration ends with the first sweep that rotates nothing, or after 30.
HD void jacobi_vmax4_sym(const double *A, double *v) {
    double W[16], V[16];
    for (int i = 0; i < 16; i++) { W[i] = A[i]; V[i] = (i % 5 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < HORN_JACOBI_MAX_SWEEPS; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0, beta = 0;
                for (int r = 0; r < 4; r++) { alpha += W[r * 4 + p] * W[r * 4 + p]; beta += W[r * 4 + q] * W[r * 4 + q]; }
                const double gamma = W[p * 4 + q];
                const double ag = gamma < 0 ? -gamma : gamma;
                if (ag <= 8.8817841970012523e-16 * sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (W[q * 4 + q] - W[p * 4 + p]) / (2.0 * gamma);
                const double az = zeta < 0 ? -zeta : zeta;
                const double t = (zeta < 0 ? -1.0 : 1.0) / (az + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                const double app = W[p * 4 + p] - t * gamma, aqq = W[q * 4 + q] + t * gamma;
                for (int r = 0; r < 4; r++) {
                    const double vp = V[r * 4 + p], vq = V[r * 4 + q];
                    V[r * 4 + p] = c * vp - s * vq; V[r * 4 + q] = s * vp + c * vq;
                    if (r == p || r == q) continue;
                    const double wp = W[r * 4 + p], wq = W[r * 4 + q];
                    const double np_ = c * wp - s * wq, nq_ = s * wp + c * wq;
                    W[r * 4 + p] = np_; W[p * 4 + r] = np_; W[r * 4 + q] = nq_; W[q * 4 + r] = nq_;
                }
                W[p * 4 + p] = app; W[q * 4 + q] = aqq; W[p * 4 + q] = 0.0; W[q * 4 + p] = 0.0;
            }
        if (!rotated) break;
    }
    double dbest = W[0];
    for (int r = 0; r < 4; r++) v[r] = V[r * 4];
    for (int k = 1; k < 4; k++)
        if (W[k * 4 + k] > dbest) { dbest = W[k * 4 + k]; for (int r = 0; r < 4; r++) v[r] = V[r * 4 + k]; }
}

// R (row-major, float) of the quaternion q = (w, x, y, z) of any length and sign; NaN where x = y = z = 0 (:277)
HD void horn_rotation(const double *q, float *R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double vv = x * x + y * y + z * z;
    if (vv == 0.0) { const double nan = vv / vv; for (int i = 0; i < 9; i++) R[i] = (float)nan; return; }
    const double qq = w * w + vv;
    R[0] = (float)(1.0 - 2.0 * (y * y + z * z) / qq); R[1] = (float)(2.0 * (x * y - w * z) / qq);       R[2] = (float)(2.0 * (x * z + w * y) / qq);
    R[3] = (float)(2.0 * (x * y + w * z) / qq);       R[4] = (float)(1.0 - 2.0 * (x * x + z * z) / qq); R[5] = (float)(2.0 * (y * z - w * x) / qq);
    R[6] = (float)(2.0 * (x * z - w * y) / qq);       R[7] = (float)(2.0 * (y * z + w * x) / qq);       R[8] = (float)(1.0 - 2.0 * (x * x + y * y) / qq);
}

struct HornSim3 {
    float s;                      // ms12i
    float R[9], t[3];             // mR12i, mt12i
    float sR[9];                  // mT12i = [sR | t]
    float sRinv[9], tinv[3];      // mT21i = [sRinv | tinv]
};

// ComputeCentroid: P holds the three points as its columns, given here as p[i] = column i
HD void horn_centroid(const float *p0, const float *p1, const float *p2, float *Pr /* [r * 3 + i]: row r, column i */, float *C) {
    for (int r = 0; r < 3; r++) {
        const float sum = (p0[r] + p1[r]) + p2[r];          // cv::reduce(P, C, 1, CV_REDUCE_SUM)
        C[r] = (float)((double)sum * (1.0 / 3.0));          // C = C / P.cols
        Pr[r * 3 + 0] = p0[r] - C[r]; Pr[r * 3 + 1] = p1[r] - C[r]; Pr[r * 3 + 2] = p2[r] - C[r];
    }
}

// ComputeSim3(P3Dc1i, P3Dc2i): a[i], b[i] = mvX3Dc1 / mvX3Dc2 of the i-th drawn correspondence
HD void horn_sim3(const float *a0, const float *a1, const float *a2, const float *b0, const float *b1, const float *b2, bool fix_scale, HornSim3 *h) {
    float Pr1[9], Pr2[9], O1[3], O2[3];
    horn_centroid(a0, a1, a2, Pr1, O1);
    horn_centroid(b0, b1, b2, Pr2, O2);
    float M[9]; // M = Pr2 * Pr1.t()
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double sacc = 0;
            for (int k = 0; k < 3; k++) sacc += (double)Pr2[r * 3 + k] * (double)Pr1[c * 3 + k];
            M[r * 3 + c] = (float)sacc;
        }
    const float N11 = M[0] + M[4] + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3];
    const float N22 = M[0] - M[4] - M[8], N23 = M[1] + M[3], N24 = M[6] + M[2];
    const float N33 = -M[0] + M[4] - M[8], N34 = M[5] + M[7];
    const float N44 = -M[0] - M[4] + M[8];
    const double Nd[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    double q[4];
    jacobi_vmax4_sym(Nd, q);
    horn_rotation(q, h->R);
    float P3[9]; // P3 = mR12i * Pr2
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double sacc = 0;
            for (int k = 0; k < 3; k++) sacc += (double)h->R[r * 3 + k] * (double)Pr2[k * 3 + c];
            P3[r * 3 + c] = (float)sacc;
        }
    if (!fix_scale) {
        double nom = 0, den = 0;
        for (int i = 0; i < 9; i++) nom += (double)Pr1[i] * (double)P3[i]; // Pr1.dot(P3)
        for (int i = 0; i < 9; i++) { const float sq = P3[i] * P3[i]; den += (double)sq; }
        h->s = (float)(nom / den);
    } else
        h->s = 1.0f;
    const double sd = (double)h->s;
    for (int r = 0; r < 3; r++) { // mt12i = O1 - ms12i * mR12i * O2
        const double sacc = dot3_f64(h->R + 3 * r, O2);
        h->t[r] = (float)(-sd * sacc + (double)O1[r] * 1.0);
    }
    const double inv = 1.0 / sd;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            h->sR[r * 3 + c] = (float)((double)h->R[r * 3 + c] * sd);     // sR = ms12i * mR12i
            h->sRinv[r * 3 + c] = (float)((double)h->R[c * 3 + r] * inv); // sRinv = (1.0 / ms12i) * mR12i.t()
        }
    for (int r = 0; r < 3; r++) h->tinv[r] = (float)(-1.0 * dot3_f64(h->sRinv + 3 * r, h->t)); // tinv = -sRinv * mt12i
}

// FromCameraToImage: K = fx fy cx cy
HD void horn_to_image(const float *X, const float *K, float *uv) {
    const float invz = 1 / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    uv[0] = K[0] * x + K[2]; uv[1] = K[1] * y + K[3];
}
// Project: Tcw = [Rcw | tcw]
HD void horn_project(const float *Rcw, const float *tcw, const float *X, const float *K, float *uv) {
    float P3Dc[3];
    gemm3(Rcw, X, tcw, P3Dc);
    horn_to_image(P3Dc, K, uv);
}
// mvbInliersi[i] of CheckInliers for one correspondence: X1, X2 = mvX3Dc1[i], mvX3Dc2[i]; K8 = fx fy cx cy of mK1, then of mK2.  err (when given) receives err1, err2.
HD bool horn_is_inlier(const HornSim3 &h, const float *X1, const float *X2, float max_err1, float max_err2, const float *K8, float *err) {
    float p1im1[2], p2im2[2], p2im1[2], p1im2[2];
    horn_to_image(X1, K8, p1im1);
    horn_to_image(X2, K8 + 4, p2im2);
    horn_project(h.sR, h.t, X2, K8, p2im1);
    horn_project(h.sRinv, h.tinv, X1, K8 + 4, p1im2);
    const float d1[2] = {p1im1[0] - p2im1[0], p1im1[1] - p2im1[1]};
    const float d2[2] = {p1im2[0] - p2im2[0], p1im2[1] - p2im2[1]};
    const float err1 = (float)((double)d1[0] * (double)d1[0] + (double)d1[1] * (double)d1[1]);
    const float err2 = (float)((double)d2[0] * (double)d2[0] + (double)d2[1] * (double)d2[1]);
    if (err) { err[0] = err1; err[1] = err2; }
    return err1 < max_err1 && err2 < max_err2;
}
