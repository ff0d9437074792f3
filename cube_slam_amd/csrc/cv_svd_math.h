// cv_svd_math.h -- the OpenCV primitives PnPsolver (orb_object_slam/src/PnPsolver.cc) calls on double matrices -- cvMulTransposed, cvSVD, cvInvert(CV_SVD),
// cvSolve(CV_SVD) -- as the library's stated definitions (INTEGRATION.md 8b''): OpenCV is no part of the reference tree, and its result depends on the build (LAPACK or its
// own Jacobi).  The model is OpenCV's one-sided Hestenes Jacobi (JacobiSVDImpl_) with SVBkSb's back substitution, in IEEE add, mul, div and sqrt only: no libm call but sqrt
// and fabs (hypot(p, beta) is stated as sqrt(p * p + beta * beta)); -ffp-contract=off.  HD: the kernels of pnpsolver.hip, its host path and the tests' g++ builds run this text.
//
// Every function is called by all lanes of an executor X { int lane, lanes; void sync(); }: CvxSeq is one host thread, the kernels pass a wave whose sync() is the
// workgroup barrier.  A value that decides a branch is computed by every lane from the same memory in the same order, so control flow is uniform; element updates are spread
// over the lanes, and every sum is one lane's, over ascending index.  The result does not depend on the executor.
//
//   cvx_jacobi_rows   the n rows (length m) of At are rotated pairwise, pairs (i, j) in the order (0,1) (0,2) .. (0,n-1) (1,2) .. (n-2,n-1), until a sweep rotates nothing or
//                     after max(m, 30) sweeps; a pair is skipped where |p| <= 10 DBL_EPSILON sqrt(a b) (p = row_i . row_j, a, b = the rows' squared norms as last summed);
//                     the rotations accumulate in the rows of Vt (from the identity).  W = the rows' norms, sorted descending by selection (the first largest wins), rows of At
//                     and Vt moved with them.
//   cvx_unit_rows     row_i of At times 1 / W_i -> the left vectors; 0 where W_i <= DBL_MIN (OpenCV draws a random vector there; no statement of the reference reads one)
//   cvx_svd_sym_ut    cvSVD(A, D, Ut, 0, CV_SVD_MODIFY_A | CV_SVD_U_T) of a symmetric positive semidefinite A (:400, :498: a Gram matrix): D = W and Ut = Vt.  For such a matrix
//                     U = V; the rows of A V scaled by 1 / W lose the null space to rounding where W is a rounding residue, and the 4-point MtM has four such values, so
//                     the left vectors are stated as the accumulated rotations, whose rows stay orthonormal.
//   cvx_svd_uv        cvSVD(A, D, U, V, CV_SVD_MODIFY_A) of a square n x n A (:621): Jacobi on At = A transposed; U[r][i] = unit row_i[r], V[r][i] = Vt[i][r]
//   back substitution SVBkSb (in cvx_solve_svd, cvx_invert3_svd): x = sum over i ascending (W descending) of v_i ((u_i . b) (1 / W_i)), the terms with |W_i| <= 2 DBL_EPSILON sum(W) left out
//   cvx_solve_svd     cvSolve(A, b, x, CV_SVD), A m x n, m >= n (:698, :733, :772)
//   cvx_invert3_svd   cvInvert(A, Ainv, CV_SVD) 3 x 3 (:422): Ainv[r][c] = sum over i of v_i[r] (u_i[c] (1 / W_i)), same threshold
//   cvx_gram_entry    one entry of cvMulTransposed(A, dst, 1) = At A: the sum over the rows of A ascending
// cvx_jacobi_rows and cvx_unit_rows are generic over the storage type (CvxType below): double for the above, float for cv::SVDecomp on CV_32F (initializer_math.h,
// INTEGRATION.md 8b''').
#pragma once
#include <math.h>

#include "hd.h"

// Loops stay rolled: the kernels run this text with its state in LDS, and unrolled it takes more registers than a wave has (scratch); the arithmetic is the same either way.
#if defined(__clang__)
#define CVX_NOUNROLL _Pragma("nounroll")
#else
#define CVX_NOUNROLL _Pragma("GCC unroll 1")
#endif

struct CvxSeq { // one thread
    static constexpr int lane = 0, lanes = 1;
    HD void sync() const {}
};

constexpr double CVX_EPS = 2.2204460492503131e-15;     // 10 DBL_EPSILON
constexpr double CVX_MINVAL = 2.2250738585072014e-308; // DBL_MIN
constexpr double CVX_BK_EPS = 4.4408920985006262e-16;  // 2 DBL_EPSILON

// The storage type T of At and Vt: OpenCV's JacobiSVDImpl_<_Tp> keeps the elements and the rotation's c and s in _Tp and every sum in double.  For double the casts below
// are no operation; for float (Initializer.cc, initializer_math.h) an element is rounded to float after each rotation, the skip threshold is 2 FLT_EPSILON (as a float,
// widened) and a row is a zero row where its norm is <= FLT_MIN.
template <class T> struct CvxType;
template <> struct CvxType<double> { static constexpr double eps = CVX_EPS, minval = CVX_MINVAL; };
template <> struct CvxType<float> { static constexpr double eps = 2.384185791015625e-07 /* 2 FLT_EPSILON = 2^-22 */, minval = 1.1754943508222875e-38 /* FLT_MIN */; };

template <class X, class T> HD void cvx_jacobi_rows(X x, T *At, int m, int n, double *W, T *Vt) {
    if (x.lane == 0)
        CVX_NOUNROLL for (int i = 0; i < n; i++) {
            double sd = 0;
            CVX_NOUNROLL for (int k = 0; k < m; k++) sd += (double)At[i * m + k] * At[i * m + k];
            W[i] = sd;
            CVX_NOUNROLL for (int k = 0; k < n; k++) Vt[i * n + k] = (k == i) ? (T)1 : (T)0;
        }
    x.sync();
    const int max_iter = m > 30 ? m : 30;
    CVX_NOUNROLL for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        CVX_NOUNROLL for (int i = 0; i < n - 1; i++)
            CVX_NOUNROLL for (int j = i + 1; j < n; j++) {
                T *Ai = At + i * m, *Aj = At + j * m;
                double a = W[i], b = W[j], p = 0;
                CVX_NOUNROLL for (int k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (fabs(p) <= CvxType<T>::eps * sqrt(a * b)) continue; // (false for a NaN: the pair is rotated, as in the model)
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                T c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (T)sqrt(delta / gamma);
                    c = (T)(p / (gamma * s * 2));
                } else {
                    c = (T)sqrt((gamma + beta) / (gamma * 2));
                    s = (T)(p / (gamma * c * 2));
                }
                x.sync(); // (every lane has read the two rows and W)
                CVX_NOUNROLL for (int k = x.lane; k < m + n; k += x.lanes) {
                    T *Pi = k < m ? Ai + k : Vt + i * n + (k - m), *Pj = k < m ? Aj + k : Vt + j * n + (k - m);
                    const T t0 = c * *Pi + s * *Pj, t1 = -s * *Pi + c * *Pj;
                    *Pi = t0; *Pj = t1;
                }
                x.sync();
                a = b = 0;
                CVX_NOUNROLL for (int k = 0; k < m; k++) { a += (double)Ai[k] * Ai[k]; b += (double)Aj[k] * Aj[k]; }
                if (x.lane == 0) { W[i] = a; W[j] = b; }
                changed = true;
                x.sync();
            }
        if (!changed) break;
    }
    if (x.lane == 0) {
        CVX_NOUNROLL for (int i = 0; i < n; i++) {
            double sd = 0;
            CVX_NOUNROLL for (int k = 0; k < m; k++) sd += (double)At[i * m + k] * At[i * m + k];
            W[i] = sqrt(sd);
        }
        CVX_NOUNROLL for (int i = 0; i < n - 1; i++) {
            int j = i;
            CVX_NOUNROLL for (int k = i + 1; k < n; k++)
                if (W[j] < W[k]) j = k;
            if (i != j) {
                double t = W[i]; W[i] = W[j]; W[j] = t;
                CVX_NOUNROLL for (int k = 0; k < m; k++) { const T u = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = u; }
                CVX_NOUNROLL for (int k = 0; k < n; k++) { const T u = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = u; }
            }
        }
    }
    x.sync();
}

template <class X, class T> HD void cvx_unit_rows(X x, T *At, int m, int n, const double *W) {
    if (x.lane == 0)
        CVX_NOUNROLL for (int i = 0; i < n; i++) {
            const double sd = W[i];
            const T s = (T)(sd > CvxType<T>::minval ? 1 / sd : 0.);
            CVX_NOUNROLL for (int k = 0; k < m; k++) At[i * m + k] *= s;
        }
    x.sync();
}

template <class X> HD void cvx_svd_sym_ut(X x, double *A, int n, double *D, double *Ut) { cvx_jacobi_rows(x, A, n, n, D, Ut); }

// work: (n * n) doubles for At and n * n for Vt
template <class X> HD void cvx_svd_uv(X x, const double *A, int n, double *D, double *U, double *V, double *work) {
    double *At = work, *Vt = work + n * n;
    if (x.lane == 0)
        CVX_NOUNROLL for (int r = 0; r < n; r++)
            CVX_NOUNROLL for (int c = 0; c < n; c++) At[c * n + r] = A[r * n + c];
    x.sync();
    cvx_jacobi_rows(x, At, n, n, D, Vt);
    cvx_unit_rows(x, At, n, n, D);
    if (x.lane == 0)
        CVX_NOUNROLL for (int r = 0; r < n; r++)
            CVX_NOUNROLL for (int i = 0; i < n; i++) { U[r * n + i] = At[i * n + r]; V[r * n + i] = Vt[i * n + r]; }
    x.sync();
}

HD double cvx_backsubst_threshold(const double *W, int n) {
    double threshold = 0;
    CVX_NOUNROLL for (int i = 0; i < n; i++) threshold += W[i];
    return threshold * CVX_BK_EPS;
}

// work: m * n doubles for At, n * n for Vt, n for W
template <class X> HD void cvx_solve_svd(X x, const double *A, int m, int n, const double *b, double *xs, double *work) {
    double *At = work, *Vt = work + m * n, *W = Vt + n * n;
    if (x.lane == 0)
        CVX_NOUNROLL for (int r = 0; r < m; r++)
            CVX_NOUNROLL for (int c = 0; c < n; c++) At[c * m + r] = A[r * n + c];
    x.sync();
    cvx_jacobi_rows(x, At, m, n, W, Vt);
    cvx_unit_rows(x, At, m, n, W);
    if (x.lane == 0) {
        const double threshold = cvx_backsubst_threshold(W, n);
        CVX_NOUNROLL for (int j = 0; j < n; j++) xs[j] = 0;
        CVX_NOUNROLL for (int i = 0; i < n; i++) {
            double wi = W[i];
            if (fabs(wi) <= threshold) continue;
            wi = 1 / wi;
            double s = 0;
            CVX_NOUNROLL for (int j = 0; j < m; j++) s += At[i * m + j] * b[j];
            s *= wi;
            CVX_NOUNROLL for (int j = 0; j < n; j++) xs[j] = xs[j] + s * Vt[i * n + j];
        }
    }
    x.sync();
}

// work: 9 doubles for At, 9 for Vt, 3 for W
template <class X> HD void cvx_invert3_svd(X x, const double *A, double *Ainv, double *work) {
    double *At = work, *Vt = work + 9, *W = work + 18;
    if (x.lane == 0)
        CVX_NOUNROLL for (int r = 0; r < 3; r++)
            CVX_NOUNROLL for (int c = 0; c < 3; c++) At[c * 3 + r] = A[r * 3 + c];
    x.sync();
    cvx_jacobi_rows(x, At, 3, 3, W, Vt);
    cvx_unit_rows(x, At, 3, 3, W);
    if (x.lane == 0) {
        const double threshold = cvx_backsubst_threshold(W, 3);
        CVX_NOUNROLL for (int j = 0; j < 9; j++) Ainv[j] = 0;
        CVX_NOUNROLL for (int i = 0; i < 3; i++) {
            double wi = W[i];
            if (fabs(wi) <= threshold) continue;
            wi = 1 / wi;
            CVX_NOUNROLL for (int r = 0; r < 3; r++)
                CVX_NOUNROLL for (int c = 0; c < 3; c++) Ainv[r * 3 + c] = Ainv[r * 3 + c] + Vt[i * 3 + r] * (At[i * 3 + c] * wi);
        }
    }
    x.sync();
}

// (At A)[a][b] of the rows x cols row-major A
HD double cvx_gram_entry(const double *A, int rows, int cols, int a, int b) {
    double s = 0;
    CVX_NOUNROLL for (int k = 0; k < rows; k++) s += A[k * cols + a] * A[k * cols + b];
    return s;
}
