// initializer_math.h -- ORB_SLAM2::Initializer (orb_object_slam/src/Initializer.cc), statement by statement in the reference's float arithmetic (cv_math.h for the cv::Mat
// forms; -ffp-contract=off).  HD: the kernels of initializer.hip, the host path (initializer_host.h) and the g++ builds of the tests run this text.
//
// cv::Mat forms (INTEGRATION.md 8e / 8b'): a product is one gemm, every entry a double sum over k ascending rounded once; a scale inside a MatExpr (s * U * Rp, -R.t() * t,
// t / cv::norm(t), tp *= d) stays inside that rounding; kp.pt.x * P.row(2) - P.row(0) is a float multiply and a float add; x3D / w is float(x_k * (1.0 / w)).
// The library's stated definitions (OpenCV is no part of the reference tree; INTEGRATION.md 8b'''):
//   cv::SVDecomp / cv::SVD::compute on CV_32F, FULL_UV   OpenCV's one-sided Jacobi with float storage (cvx_jacobi_rows<float>, cv_svd_math.h): 16 x 9 -> vt.row(8) is the Jacobi
//                     row of the smallest value (im_compute_H21); 8 x 9 -> the Jacobi runs on the 8 rows of A, vt.row(8) is the completion of their span (im_complete_row9);
//                     3 x 3 -> im_svd3.  A left vector of a singular value <= FLT_MIN is zero (OpenCV draws one; no pattern reaches it).
//   Triangulate's 4 x 4 SVD   jacobi_vmin4 (triangulate_math.h), the definition of 8e
//   Mat::inv() of a float 3 x 3, cv::determinant   the closed form in double, rounded once per element; a zero determinant gives the zero matrix
//   acos   none here: CheckRT returns the cosine at the order statistic (im_cos_select) and the walk (initializer_walk.h) takes acosf on the host
//   std::sort over vCosParallax   ascending by <, a NaN after every number, equal values in their order of arrival (-0 and +0 are equal)
//
// Functions taking an executor X (cv_svd_math.h) are called by all its lanes; the rest are one thread's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "cv_svd_math.h"
#include "triangulate_math.h"

// ---- cv::Mat forms on row-major float 3 x 3
HD void im_gemm(const float *A, const float *B, int n, double alpha, float *C) { // C (3 x n) = alpha * A * B
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < n; c++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)A[r * 3 + k] * (double)B[k * n + c];
            C[r * n + c] = (float)(s * alpha);
        }
}
HD void im_transpose(const float *A, float *At) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) At[c * 3 + r] = A[r * 3 + c];
}
HD double im_det3(const float *M) { // cv::determinant
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
}
HD void im_inv3(const float *S, float *D) { // Mat::inv()
    const double s00 = S[0], s01 = S[1], s02 = S[2], s10 = S[3], s11 = S[4], s12 = S[5], s20 = S[6], s21 = S[7], s22 = S[8];
    double d = im_det3(S);
    if (d == 0) { // (a NaN determinant goes on and gives NaNs)
        for (int k = 0; k < 9; k++) D[k] = 0.f;
        return;
    }
    d = 1. / d;
    D[0] = (float)((s11 * s22 - s12 * s21) * d); D[1] = (float)((s02 * s21 - s01 * s22) * d); D[2] = (float)((s01 * s12 - s02 * s11) * d);
    D[3] = (float)((s12 * s20 - s10 * s22) * d); D[4] = (float)((s00 * s22 - s02 * s20) * d); D[5] = (float)((s02 * s10 - s00 * s12) * d);
    D[6] = (float)((s10 * s21 - s11 * s20) * d); D[7] = (float)((s01 * s20 - s00 * s21) * d); D[8] = (float)((s00 * s11 - s01 * s10) * d);
}
HD float im_sqrt(float v) { return (float)sqrt((double)v); }                   // sqrt(float): the correctly rounded root either way
HD bool im_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; } // isfinite
HD void im_unit3(const float *t, float *o) { // t / cv::norm(t)
    const double inv = 1.0 / norm3_f64(t);
    for (int k = 0; k < 3; k++) o[k] = (float)((double)t[k] * inv);
}

// ---- Normalize :754-800.  The four sums are one thread's, ascending; the points follow from them one by one (im_normalize_point)
struct InitNorm { float meanX, meanY, sX, sY; };
HD InitNorm im_normalize_sums(const float *keys, int N) {
    float meanX = 0, meanY = 0;
    for (int i = 0; i < N; i++) { meanX += keys[2 * i]; meanY += keys[2 * i + 1]; }
    meanX = meanX / N; meanY = meanY / N;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < N; i++) { meanDevX += fabsf(keys[2 * i] - meanX); meanDevY += fabsf(keys[2 * i + 1] - meanY); }
    meanDevX = meanDevX / N; meanDevY = meanDevY / N;
    return InitNorm{meanX, meanY, (float)(1.0 / (double)meanDevX), (float)(1.0 / (double)meanDevY)};
}
HD void im_normalize_point(const InitNorm &n, const float *key, float *pn) {
    pn[0] = (key[0] - n.meanX) * n.sX;
    pn[1] = (key[1] - n.meanY) * n.sY;
}
HD void im_normalize_T(const InitNorm &n, float *T) {
    for (int k = 0; k < 9; k++) T[k] = (k % 4 == 0) ? 1.f : 0.f;
    T[0] = n.sX; T[4] = n.sY; T[2] = -n.meanX * n.sX; T[5] = -n.meanY * n.sY;
}

// ---- the SVDs.  One hypothesis's working set: under 2 KB, in LDS on the device
struct InitSvdWork {
    float At[16 * 9], Vt[9 * 9];
    double W[9];
    float row[9], At3[9], Vt3[9];
    double W3[3];
    float p1[16], p2[16]; // the 8 normalised pairs of a hypothesis, x y each
};

// cv::SVD::compute of a 3 x 3: U, w (descending) and Vt
template <class X> HD void im_svd3(X x, const float *A, InitSvdWork *w, float *U, float *wf, float *Vt) {
    if (x.lane == 0) im_transpose(A, w->At3);
    x.sync();
    cvx_jacobi_rows(x, w->At3, 3, 3, w->W3, w->Vt3);
    cvx_unit_rows(x, w->At3, 3, 3, w->W3);
    for (int k = 0; k < 9; k++) { U[k] = w->At3[(k % 3) * 3 + k / 3]; Vt[k] = w->Vt3[k]; }
    for (int k = 0; k < 3; k++) wf[k] = (float)w->W3[k];
    x.sync(); // (the work may be written again)
}

// the DLT matrix of ComputeH21 :235-263 on 8 pairs, as the rows of its transpose (At[c * 16 + r] = A(r, c)): what the Jacobi runs on
HD void im_fill_H21(const float *p1, const float *p2, float *At) {
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
        for (int c = 0; c < 9; c++) { At[c * 16 + 2 * i] = r0[c]; At[c * 16 + 2 * i + 1] = r1[c]; }
    }
}
// ... and of ComputeF21 :276-294, row-major 8 x 9 (m < n: the Jacobi runs on the 8 rows of A itself)
HD void im_fill_F21(const float *p1, const float *p2, float *A) {
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
        for (int c = 0; c < 9; c++) A[i * 9 + c] = r[c];
    }
}

// ComputeH21 :231-270 on the 8 normalised pairs w->p1, w->p2
template <class X> HD void im_compute_H21(X x, InitSvdWork *w, float *Hn) {
    if (x.lane == 0) im_fill_H21(w->p1, w->p2, w->At);
    x.sync();
    cvx_jacobi_rows(x, w->At, 16, 9, w->W, w->Vt);
    for (int k = 0; k < 9; k++) Hn[k] = w->Vt[8 * 9 + k];
    x.sync();
}

// vt.row(8) of an 8 x 9 A whose 8 unit rows (singular values descending) are rows: OpenCV's completion -- the row starts as +-1/9 from its generator (seed 0x12345678,
// state = (uint32)state * 4294883355 + (state >> 32), bit 8 of the low word set -> +), is orthogonalised twice against the rows above, one by one, each followed by an L1
// rescale (which leaves zeros where the remainder's L1 norm is <= 200 FLT_EPSILON: a start vector with next to nothing along the null space), and is normalised; while its
// norm is <= FLT_MIN the same is done again with the generator's next nine draws, at most 100 times.  The products of the projection are float products summed in double,
// as OpenCV writes them.
HD void im_complete_row9(const float *rows, float *row) {
    uint64_t state = 0x12345678u;
    const float val0 = (float)(1. / 9);
    const float eps100 = 2.384185791015625e-07f * 100;
    double sd = 0;
    for (int ii = 0; ii < 100 && sd <= CvxType<float>::minval; ii++) {
        for (int k = 0; k < 9; k++) {
            state = (uint64_t)(uint32_t)state * 4294883355u + (uint32_t)(state >> 32);
            row[k] = ((uint32_t)state & 256u) != 0 ? val0 : -val0;
        }
        for (int iter = 0; iter < 2; iter++)
            for (int j = 0; j < 8; j++) {
                double pd = 0;
                for (int k = 0; k < 9; k++) pd += row[k] * rows[j * 9 + k];
                float asum = 0;
                for (int k = 0; k < 9; k++) {
                    const float t = (float)(row[k] - pd * rows[j * 9 + k]);
                    row[k] = t;
                    asum += fabsf(t);
                }
                asum = asum > eps100 ? 1 / asum : 0;
                for (int k = 0; k < 9; k++) row[k] *= asum;
            }
        sd = 0;
        for (int k = 0; k < 9; k++) sd += (double)row[k] * row[k];
        sd = sqrt(sd);
    }
    const float s = (float)(sd > CvxType<float>::minval ? 1 / sd : 0.);
    for (int k = 0; k < 9; k++) row[k] *= s;
}

// ComputeF21 :272-307
template <class X> HD void im_compute_F21(X x, InitSvdWork *w, float *Fn) {
    if (x.lane == 0) im_fill_F21(w->p1, w->p2, w->At);
    x.sync();
    cvx_jacobi_rows(x, w->At, 9, 8, w->W, w->Vt);
    cvx_unit_rows(x, w->At, 9, 8, w->W);
    if (x.lane == 0) im_complete_row9(w->At, w->row);
    x.sync();
    float Fpre[9], U[9], wf[3], Vt[9];
    for (int k = 0; k < 9; k++) Fpre[k] = w->row[k];
    im_svd3(x, Fpre, w, U, wf, Vt);
    wf[2] = 0;
    const float D[9] = {wf[0], 0.f, 0.f, 0.f, wf[1], 0.f, 0.f, 0.f, wf[2]};
    float UD[9];
    im_gemm(U, D, 3, 1.0, UD);
    im_gemm(UD, Vt, 3, 1.0, Fn);
}

// H21i = T2inv * Hn * T1 and H12i = H21i.inv() (:167-168); F21i = T2t * Fn * T1 (:218)
HD void im_denormalise(const float *T2x, const float *Mn, const float *T1, float *M) {
    float t[9];
    im_gemm(T2x, Mn, 3, 1.0, t);
    im_gemm(t, T1, 3, 1.0, M);
}

// ---- CheckHomography :309-392 / CheckFundamental :394-472 for one correspondence: bIn, and the two terms of `score += th - chiSquare` in the order written; a term that
// is not added is IM_NO_TERM (a term that is added is >= 0 or a NaN)
constexpr float IM_NO_TERM = -1.f;
HD float im_inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }
HD bool im_check_h(const float *H21, const float *H12, float u1, float v1, float u2, float v2, float invSigmaSquare, float *t1, float *t2) {
    const float th = 5.991f;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; *t1 = IM_NO_TERM; }
    else *t1 = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; *t2 = IM_NO_TERM; }
    else *t2 = th - chiSquare2;
    return bIn;
}
HD bool im_check_f(const float *F, float u1, float v1, float u2, float v2, float invSigmaSquare, float *t1, float *t2) {
    const float th = 3.841f, thScore = 5.991f;
    bool bIn = true;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; *t1 = IM_NO_TERM; }
    else *t1 = thScore - chiSquare1;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; *t2 = IM_NO_TERM; }
    else *t2 = thScore - chiSquare2;
    return bIn;
}
HD float im_score_add(float score, float t1, float t2) {
    if (!(t1 < 0)) score += t1;
    if (!(t2 < 0)) score += t2;
    return score;
}

// ---- the motion candidates: rows of 12 floats, R row-major then t
// DecomposeE :913-933 on E21 = K.t() * F21 * K (:483), and the four of :498-501
template <class X> HD int im_candidates_F(X x, const float *F21, const float *K, InitSvdWork *w, float *cand) {
    float Kt[9], t0[9], E[9], u[9], wf[3], vt[9];
    im_transpose(K, Kt);
    im_gemm(Kt, F21, 3, 1.0, t0);
    im_gemm(t0, K, 3, 1.0, E);
    im_svd3(x, E, w, u, wf, vt);
    const float ucol[3] = {u[2], u[5], u[8]};
    float t[3];
    im_unit3(ucol, t);
    const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float Wt[9], R1[9], R2[9];
    im_transpose(Wm, Wt);
    im_gemm(u, Wm, 3, 1.0, t0); im_gemm(t0, vt, 3, 1.0, R1);
    if (im_det3(R1) < 0) for (int k = 0; k < 9; k++) R1[k] = -R1[k];
    im_gemm(u, Wt, 3, 1.0, t0); im_gemm(t0, vt, 3, 1.0, R2);
    if (im_det3(R2) < 0) for (int k = 0; k < 9; k++) R2[k] = -R2[k];
    for (int c = 0; c < 4; c++)
        for (int k = 0; k < 12; k++) cand[c * 12 + k] = k < 9 ? ((c & 1) ? R2[k] : R1[k]) : (c < 2 ? t[k - 9] : -t[k - 9]);
    return 4;
}

// ReconstructH :591-693: 0 candidates at the return of :604.  (vn, the plane normals, are computed by the reference and read by nothing.)
template <class X> HD int im_candidates_H(X x, const float *H21, const float *K, InitSvdWork *w, float *cand) {
    float invK[9], t0[9], A[9], U[9], wf[3], Vt[9];
    im_inv3(K, invK);
    im_gemm(invK, H21, 3, 1.0, t0);
    im_gemm(t0, K, 3, 1.0, A);
    im_svd3(x, A, w, U, wf, Vt);
    const float s = (float)(im_det3(U) * im_det3(Vt));
    const float d1 = wf[0], d2 = wf[1], d3 = wf[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return 0;
    const float aux1 = im_sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = im_sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = im_sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = im_sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    for (int i = 0; i < 8; i++) {
        const int q = i & 3;
        float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tp[3];
        float scale;
        if (i < 4) { // case d' = d2
            Rp[0] = ctheta; Rp[2] = -stheta[q]; Rp[6] = stheta[q]; Rp[8] = ctheta;
            tp[0] = x1[q]; tp[1] = 0; tp[2] = -x3[q];
            scale = d1 - d3;
        } else { // case d' = -d2
            Rp[0] = cphi; Rp[2] = sphi[q]; Rp[4] = -1; Rp[6] = sphi[q]; Rp[8] = -cphi;
            tp[0] = x1[q]; tp[1] = 0; tp[2] = x3[q];
            scale = d1 + d3;
        }
        float *R = cand + 12 * i, t[3];
        im_gemm(U, Rp, 3, (double)s, t0); // s * U * Rp
        im_gemm(t0, Vt, 3, 1.0, R);
        for (int k = 0; k < 3; k++) tp[k] = (float)((double)tp[k] * (double)scale); // tp *= d1 -+ d3
        im_gemm(U, tp, 1, 1.0, t);
        im_unit3(t, R + 9);
    }
    return 8;
}

// ---- CheckRT :802-911.  What does not depend on the correspondence
struct InitCam { float fx, fy, cx, cy, P1[12], P2[12], R[9], t[3], O2[3], th2; };
HD void im_make_cam(const float *K, const float *Rt, float sigma, InitCam *c) {
    c->fx = K[0]; c->fy = K[4]; c->cx = K[2]; c->cy = K[5];
    float Rt34[12];
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) { c->P1[r * 4 + k] = K[r * 3 + k]; c->R[r * 3 + k] = Rt[r * 3 + k]; Rt34[r * 4 + k] = Rt[r * 3 + k]; }
        c->P1[r * 4 + 3] = 0.f; c->t[r] = Rt[9 + r]; Rt34[r * 4 + 3] = Rt[9 + r];
    }
    im_gemm(K, Rt34, 4, 1.0, c->P2); // P2 = K * [R | t]
    float Rtr[9];
    im_transpose(c->R, Rtr);
    im_gemm(Rtr, c->t, 1, -1.0, c->O2); // O2 = -R.t() * t
    const float mSigma2 = sigma * sigma;
    c->th2 = (float)(4.0 * (double)mSigma2);
}

enum { IM_SKIPPED = 0, IM_COUNTED = 1, IM_GOOD = 2 }; // not counted; counted in nGood (:892-894); counted and vbGood (:896)
// one inlier correspondence: Triangulate :739-752 and the tests of :845-890 in order.  p3d and cosParallax are written where the status is not IM_SKIPPED
HD int im_check_point(const InitCam &c, float u1, float v1, float u2, float v2, float *p3d, float *cosParallax_out) {
    double A[16];
    for (int k = 0; k < 4; k++) {
        A[k] = (double)(u1 * c.P1[8 + k] - c.P1[k]);
        A[4 + k] = (double)(v1 * c.P1[8 + k] - c.P1[4 + k]);
        A[8 + k] = (double)(u2 * c.P2[8 + k] - c.P2[k]);
        A[12 + k] = (double)(v2 * c.P2[8 + k] - c.P2[4 + k]);
    }
    double vd[4];
    jacobi_vmin4(A, vd);
    const double invw = 1.0 / (double)(float)vd[3];
    const float p3dC1[3] = {(float)((double)(float)vd[0] * invw), (float)((double)(float)vd[1] * invw), (float)((double)(float)vd[2] * invw)};
    if (!im_finite(p3dC1[0]) || !im_finite(p3dC1[1]) || !im_finite(p3dC1[2])) return IM_SKIPPED;
    const float dist1 = norm3(p3dC1); // normal1 = p3dC1 - O1, O1 = 0
    const float normal2[3] = {p3dC1[0] - c.O2[0], p3dC1[1] - c.O2[1], p3dC1[2] - c.O2[2]};
    const float dist2 = norm3(normal2);
    const float cosParallax = (float)(dot3_f64(p3dC1, normal2) / (double)(dist1 * dist2));
    if (p3dC1[2] <= 0 && (double)cosParallax < 0.99998) return IM_SKIPPED;
    float p3dC2[3];
    gemm3(c.R, p3dC1, c.t, p3dC2);
    if (p3dC2[2] <= 0 && (double)cosParallax < 0.99998) return IM_SKIPPED;
    const float invZ1 = (float)(1.0 / (double)p3dC1[2]);
    const float im1x = c.fx * p3dC1[0] * invZ1 + c.cx, im1y = c.fy * p3dC1[1] * invZ1 + c.cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > c.th2) return IM_SKIPPED;
    const float invZ2 = (float)(1.0 / (double)p3dC2[2]);
    const float im2x = c.fx * p3dC2[0] * invZ2 + c.cx, im2y = c.fy * p3dC2[1] * invZ2 + c.cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > c.th2) return IM_SKIPPED;
    p3d[0] = p3dC1[0]; p3d[1] = p3dC1[1]; p3d[2] = p3dC1[2];
    *cosParallax_out = cosParallax;
    return (double)cosParallax < 0.99998 ? IM_GOOD : IM_COUNTED;
}

// the element std::sort would leave at position idx of list[0..n): by counting, for every element, those that sort before it (the order stated at the top).  Exactly one
// element has rank idx; the lane that holds it writes *out.
HD bool im_cos_before(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na == nb ? ia < ib : nb;
    return a < b || (a == b && ia < ib);
}
template <class X> HD void im_cos_select(X x, const float *list, int n, int idx, float *out) {
    for (int j = x.lane; j < n; j += x.lanes) {
        const float v = list[j];
        int rank = 0;
        for (int i = 0; i < n; i++) rank += im_cos_before(list[i], i, v, j) ? 1 : 0;
        if (rank == idx) *out = v;
    }
}
