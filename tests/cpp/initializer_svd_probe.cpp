// TEST INFRASTRUCTURE: the stated float SVD and inverse of cube_slam_amd/csrc/initializer_math.h and the matrices Initializer hands them, for tests/test_initializer_svd.py
// (compiled there into a temporary directory, g++ -O2 -ffp-contract=off, and called over ctypes).
#include "cube_slam_amd/csrc/initializer_math.h"

extern "C" {
// Normalize :754-800 -> the points and T
void probe_normalize(const float *keys, int n, float *pn, float *T) {
    const InitNorm nm = im_normalize_sums(keys, n);
    for (int i = 0; i < n; i++) im_normalize_point(nm, keys + 2 * i, pn + 2 * i);
    im_normalize_T(nm, T);
}
// ComputeH21 on 8 pairs: A (16 x 9 row-major, as the reference fills it), W[9], Vt[81]
void probe_h21(const float *p1, const float *p2, float *A, double *W, float *Vt) {
    InitSvdWork w;
    for (int k = 0; k < 16; k++) { w.p1[k] = p1[k]; w.p2[k] = p2[k]; }
    float At[144]; // the library's own fill, handed to LAPACK as the A it is the transpose of
    im_fill_H21(p1, p2, At);
    for (int r = 0; r < 16; r++) for (int c = 0; c < 9; c++) A[r * 9 + c] = At[c * 16 + r];
    float Hn[9];
    im_compute_H21(CvxSeq(), &w, Hn);
    for (int k = 0; k < 9; k++) W[k] = w.W[k];
    for (int k = 0; k < 81; k++) Vt[k] = w.Vt[k];
}
// ComputeF21 on 8 pairs: A (8 x 9), W[8], the full vt (9 x 9: the 8 unit rows and the completion), Fpre's U, w, Vt, and Fn
void probe_f21(const float *p1, const float *p2, float *A, double *W, float *vt, float *U3, float *w3, float *Vt3, float *Fn) {
    InitSvdWork w;
    for (int k = 0; k < 16; k++) { w.p1[k] = p1[k]; w.p2[k] = p2[k]; }
    im_fill_F21(p1, p2, A); // the library's own fill
    im_compute_F21(CvxSeq(), &w, Fn);
    for (int k = 0; k < 8; k++) W[k] = w.W[k];
    for (int k = 0; k < 72; k++) vt[k] = w.At[k];
    for (int k = 0; k < 9; k++) vt[72 + k] = w.row[k];
    float Fpre[9];
    for (int k = 0; k < 9; k++) Fpre[k] = w.row[k];
    im_svd3(CvxSeq(), Fpre, &w, U3, w3, Vt3);
}
void probe_svd3(const float *A, float *U, float *w3, float *Vt) { InitSvdWork w; im_svd3(CvxSeq(), A, &w, U, w3, Vt); }
void probe_inv3(const float *A, float *Ainv) { im_inv3(A, Ainv); }
double probe_det3(const float *A) { return im_det3(A); }
// the 3 x 3 that ReconstructH (model 0: invK * H21 * K) or ReconstructF (model 1: K.t() * F21 * K) decomposes
void probe_recon_matrix(int model, const float *M, const float *K, float *A) {
    float L[9], t[9];
    if (model == 0) im_inv3(K, L); else im_transpose(K, L);
    im_gemm(L, M, 3, 1.0, t);
    im_gemm(t, K, 3, 1.0, A);
}
}
