// epnp_math.h -- EPnP as PnPsolver runs it (orb_object_slam/src/PnPsolver.cc): compute_pose (:482-532) with choose_control_points (:376-410),
// compute_barycentric_coordinates (:412-436), fill_M (:438-454), compute_L_6x10 (:790-834), compute_rho (:836-844), find_betas_approx_1 / 2 / 3 (:683-788),
// compute_A_and_b_gauss_newton (:846-861), gauss_newton (:863-882), qr_solve (:884-991), compute_ccs (:456-468), compute_pcs (:470-480), solve_for_sign (:650-665),
// estimate_R_and_t (:577-641), reprojection_error (:557-575), compute_R_and_t (:667-678), the choice of N (:523-527), and the test of CheckInliers (:311-326): statement by
// statement in the reference's arithmetic -- double, with the float literals (1.0f - a[1] - .., 2.0f * dot(..)) and the mixed float / double of CheckInliers as written;
// -ffp-contract=off.  The OpenCV calls are the stated definitions of cv_svd_math.h.  HD: the kernels of pnpsolver.hip, its host path, cubeslam::PnPsolver without a context
// and the tests' g++ builds run this text.
//
// All state is in one EpnpWork (the kernels keep it in LDS; there is no local array), the per-point arrays pws, us, alphas, pcs, terms are the caller's (5 n + .. doubles:
// 3 n, 2 n, 4 n, 3 n, n).  Every function is called by all lanes of an executor (cv_svd_math.h): sums over correspondences are one lane per entry over ascending i, per-point
// stages one point per lane, the rest is lane 0's.  M (2 n x 12) and PW0 (n x 3) are never stored: an entry of MtM or PW0tPW0 forms its factors as fill_M and :397 do.
//
// Where the reference is undefined or degenerate:
//   * qr_solve returns at eta == 0 with X unwritten (:916-921): the increment is then the previous iteration's x, zeros before the first solve of a gauss_newton, and
//     EPNP_QR_SINGULAR is set in the status.
//   * betas[0] == 0, coplanar / collinear / coincident points: inf and NaN propagate as the statements make them; a NaN comparison is false (rep_errors, CheckInliers).
#pragma once
#include "cv_svd_math.h"

constexpr unsigned EPNP_QR_SINGULAR = 1u;

struct EpnpWork {
    double fu, fv, uc, vc;
    int n; // number_of_correspondences
    unsigned status;
    double *pws, *us, *alphas, *pcs, *terms;
    double cws[4][3], ccs[4][3];
    double pw0tpw0[9], dc[3], uct[9];
    double cc[9], cc_inv[9];
    double mtm[144], d[12], ut[144];
    double l_6x10[60], rho[6];
    double Betas[4][4], rep_errors[4], Rs[4][3][3], ts[4][3];
    double dv[4][6][3];
    double lk[30], bk[5];
    double a[24], b[6], x[4], A1[6], A2[6];
    double pc0[3], pw0[3], abt[9], abt_d[3], abt_u[9], abt_v[9];
    double svd[72]; // the small systems' At, Vt, W (6 x 5: 30 + 25 + 5)
    int sign;
};

HD double epnp_dist2(const double *p1, const double *p2) {
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}
HD double epnp_dot(const double *v1, const double *v2) { return v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]; }

template <class X> HD void epnp_choose_control_points(X x, EpnpWork *w) {
    const int n = w->n;
    CVX_NOUNROLL for (int j = x.lane; j < 3; j += x.lanes) { // C0: the centroid
        double s = 0;
        CVX_NOUNROLL for (int i = 0; i < n; i++) s += w->pws[3 * i + j];
        w->cws[0][j] = s / n;
    }
    x.sync();
    CVX_NOUNROLL for (int e = x.lane; e < 9; e += x.lanes) { // cvMulTransposed(PW0, &PW0tPW0, 1)
        const int a = e / 3, b = e % 3;
        if (a > b) continue;
        double s = 0;
        CVX_NOUNROLL for (int i = 0; i < n; i++) s += (w->pws[3 * i + a] - w->cws[0][a]) * (w->pws[3 * i + b] - w->cws[0][b]);
        w->pw0tpw0[3 * a + b] = s; w->pw0tpw0[3 * b + a] = s;
    }
    x.sync();
    cvx_svd_sym_ut(x, w->pw0tpw0, 3, w->dc, w->uct);
    if (x.lane == 0)
        CVX_NOUNROLL for (int i = 1; i < 4; i++) {
            const double k = sqrt(w->dc[i - 1] / n);
            CVX_NOUNROLL for (int j = 0; j < 3; j++) w->cws[i][j] = w->cws[0][j] + k * w->uct[3 * (i - 1) + j];
        }
    x.sync();
}

template <class X> HD void epnp_compute_barycentric_coordinates(X x, EpnpWork *w) {
    if (x.lane == 0)
        CVX_NOUNROLL for (int i = 0; i < 3; i++)
            CVX_NOUNROLL for (int j = 1; j < 4; j++) w->cc[3 * i + j - 1] = w->cws[j][i] - w->cws[0][i];
    x.sync();
    cvx_invert3_svd(x, w->cc, w->cc_inv, w->svd);
    const double *ci = w->cc_inv;
    CVX_NOUNROLL for (int i = x.lane; i < w->n; i += x.lanes) {
        const double *pi = w->pws + 3 * i;
        double *a = w->alphas + 4 * i;
        CVX_NOUNROLL for (int j = 0; j < 3; j++)
            a[1 + j] = ci[3 * j] * (pi[0] - w->cws[0][0]) + ci[3 * j + 1] * (pi[1] - w->cws[0][1]) + ci[3 * j + 2] * (pi[2] - w->cws[0][2]);
        a[0] = 1.0f - a[1] - a[2] - a[3];
    }
    x.sync();
}

// M[row][col] as fill_M writes it
HD double epnp_M(const EpnpWork *w, int row, int col) {
    const int i = row >> 1, q = col / 3, r = col % 3;
    const double as = w->alphas[4 * i + q];
    if (!(row & 1)) return r == 0 ? as * w->fu : r == 1 ? 0.0 : as * (w->uc - w->us[2 * i]);
    return r == 0 ? 0.0 : r == 1 ? as * w->fv : as * (w->vc - w->us[2 * i + 1]);
}

template <class X> HD void epnp_compute_MtM(X x, EpnpWork *w) { // cvMulTransposed(M, &MtM, 1)
    CVX_NOUNROLL for (int e = x.lane; e < 144; e += x.lanes) {
        const int a = e / 12, b = e % 12;
        if (a > b) continue;
        double s = 0;
        CVX_NOUNROLL for (int row = 0; row < 2 * w->n; row++) s += epnp_M(w, row, a) * epnp_M(w, row, b);
        w->mtm[12 * a + b] = s; w->mtm[12 * b + a] = s;
    }
    x.sync();
}

HD void epnp_compute_L_6x10(EpnpWork *w) {
    const double *ut = w->ut;
    CVX_NOUNROLL for (int i = 0; i < 4; i++) {
        const double *v = ut + 12 * (11 - i);
        int a = 0, b = 1;
        CVX_NOUNROLL for (int j = 0; j < 6; j++) {
            w->dv[i][j][0] = v[3 * a] - v[3 * b];
            w->dv[i][j][1] = v[3 * a + 1] - v[3 * b + 1];
            w->dv[i][j][2] = v[3 * a + 2] - v[3 * b + 2];
            b++;
            if (b > 3) { a++; b = a + 1; }
        }
    }
    CVX_NOUNROLL for (int i = 0; i < 6; i++) {
        double *row = w->l_6x10 + 10 * i;
        row[0] = epnp_dot(w->dv[0][i], w->dv[0][i]);
        row[1] = 2.0f * epnp_dot(w->dv[0][i], w->dv[1][i]);
        row[2] = epnp_dot(w->dv[1][i], w->dv[1][i]);
        row[3] = 2.0f * epnp_dot(w->dv[0][i], w->dv[2][i]);
        row[4] = 2.0f * epnp_dot(w->dv[1][i], w->dv[2][i]);
        row[5] = epnp_dot(w->dv[2][i], w->dv[2][i]);
        row[6] = 2.0f * epnp_dot(w->dv[0][i], w->dv[3][i]);
        row[7] = 2.0f * epnp_dot(w->dv[1][i], w->dv[3][i]);
        row[8] = 2.0f * epnp_dot(w->dv[2][i], w->dv[3][i]);
        row[9] = epnp_dot(w->dv[3][i], w->dv[3][i]);
    }
}

HD void epnp_compute_rho(EpnpWork *w) {
    w->rho[0] = epnp_dist2(w->cws[0], w->cws[1]);
    w->rho[1] = epnp_dist2(w->cws[0], w->cws[2]);
    w->rho[2] = epnp_dist2(w->cws[0], w->cws[3]);
    w->rho[3] = epnp_dist2(w->cws[1], w->cws[2]);
    w->rho[4] = epnp_dist2(w->cws[1], w->cws[3]);
    w->rho[5] = epnp_dist2(w->cws[2], w->cws[3]);
}

// find_betas_approx_1 / 2 / 3 (which = 1, 2, 3): the columns of L_6x10 taken, cvSolve, the betas
template <class X> HD void epnp_find_betas_approx(X x, EpnpWork *w, int which, double *betas) {
    const int nc = which == 1 ? 4 : which == 2 ? 3 : 5;
    if (x.lane == 0)
        CVX_NOUNROLL for (int i = 0; i < 6; i++)
            CVX_NOUNROLL for (int c = 0; c < nc; c++) {
                const int src = which == 1 ? (c == 0 ? 0 : c == 1 ? 1 : c == 2 ? 3 : 6) : c;
                w->lk[i * nc + c] = w->l_6x10[10 * i + src];
            }
    x.sync();
    cvx_solve_svd(x, w->lk, 6, nc, w->rho, w->bk, w->svd);
    if (x.lane == 0) {
        const double *b = w->bk;
        if (which == 1) {
            if (b[0] < 0) {
                betas[0] = sqrt(-b[0]);
                betas[1] = -b[1] / betas[0];
                betas[2] = -b[2] / betas[0];
                betas[3] = -b[3] / betas[0];
            } else {
                betas[0] = sqrt(b[0]);
                betas[1] = b[1] / betas[0];
                betas[2] = b[2] / betas[0];
                betas[3] = b[3] / betas[0];
            }
        } else {
            if (b[0] < 0) {
                betas[0] = sqrt(-b[0]);
                betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
            } else {
                betas[0] = sqrt(b[0]);
                betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
            }
            if (b[1] < 0) betas[0] = -betas[0];
            betas[2] = which == 2 ? 0.0 : b[3] / betas[0];
            betas[3] = 0.0;
        }
    }
    x.sync();
}

HD void epnp_compute_A_and_b_gauss_newton(EpnpWork *w, const double *betas) {
    CVX_NOUNROLL for (int i = 0; i < 6; i++) {
        const double *rowL = w->l_6x10 + i * 10;
        double *rowA = w->a + i * 4;
        rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
        rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
        rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
        rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
        w->b[i] = w->rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                               rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                               rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
    }
}

// qr_solve of the 6 x 4 w->a, w->b into w->x; false (x untouched) where a column is zero
HD bool epnp_qr_solve(EpnpWork *w) {
    const int nr = 6, nc = 4;
    double *pA = w->a, *pb = w->b, *pX = w->x, *A1 = w->A1, *A2 = w->A2;
    CVX_NOUNROLL for (int k = 0; k < nc; k++) {
        double eta = fabs(pA[k * nc + k]);
        CVX_NOUNROLL for (int i = k + 1; i < nr; i++) { // (the reference reads element (i - 1, k) in step i: its pointer moves after the comparison)
            const double elt = fabs(pA[(i - 1) * nc + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) {
            A1[k] = A2[k] = 0.0;
            return false;
        }
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        CVX_NOUNROLL for (int i = k; i < nr; i++) {
            pA[i * nc + k] *= inv_eta;
            sum += pA[i * nc + k] * pA[i * nc + k];
        }
        double sigma = sqrt(sum);
        if (pA[k * nc + k] < 0) sigma = -sigma;
        pA[k * nc + k] += sigma;
        A1[k] = sigma * pA[k * nc + k];
        A2[k] = -eta * sigma;
        CVX_NOUNROLL for (int j = k + 1; j < nc; j++) {
            double s2 = 0;
            CVX_NOUNROLL for (int i = k; i < nr; i++) s2 += pA[i * nc + k] * pA[i * nc + j];
            const double tau = s2 / A1[k];
            CVX_NOUNROLL for (int i = k; i < nr; i++) pA[i * nc + j] -= tau * pA[i * nc + k];
        }
    }
    CVX_NOUNROLL for (int j = 0; j < nc; j++) { // b <- Qt b
        double tau = 0;
        CVX_NOUNROLL for (int i = j; i < nr; i++) tau += pA[i * nc + j] * pb[i];
        tau /= A1[j];
        CVX_NOUNROLL for (int i = j; i < nr; i++) pb[i] -= tau * pA[i * nc + j];
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1]; // X = R-1 b
    CVX_NOUNROLL for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
        CVX_NOUNROLL for (int j = i + 1; j < nc; j++) sum += pA[i * nc + j] * pX[j];
        pX[i] = (pb[i] - sum) / A2[i];
    }
    return true;
}

HD void epnp_gauss_newton(EpnpWork *w, double *betas) {
    CVX_NOUNROLL for (int i = 0; i < 4; i++) w->x[i] = 0.0;
    CVX_NOUNROLL for (int k = 0; k < 5; k++) {
        epnp_compute_A_and_b_gauss_newton(w, betas);
        if (!epnp_qr_solve(w)) w->status |= EPNP_QR_SINGULAR;
        CVX_NOUNROLL for (int i = 0; i < 4; i++) betas[i] += w->x[i];
    }
}

HD void epnp_compute_ccs(EpnpWork *w, const double *betas) {
    CVX_NOUNROLL for (int i = 0; i < 4; i++) w->ccs[i][0] = w->ccs[i][1] = w->ccs[i][2] = 0.0f;
    CVX_NOUNROLL for (int i = 0; i < 4; i++) {
        const double *v = w->ut + 12 * (11 - i);
        CVX_NOUNROLL for (int j = 0; j < 4; j++)
            CVX_NOUNROLL for (int k = 0; k < 3; k++) w->ccs[j][k] += betas[i] * v[3 * j + k];
    }
}

// compute_R_and_t: ccs, pcs, the sign, estimate_R_and_t, reprojection_error -> w->Rs[which], w->ts[which], w->rep_errors[which]
template <class X> HD void epnp_compute_R_and_t(X x, EpnpWork *w, int which) {
    const int n = w->n;
    double(*R)[3] = w->Rs[which];
    double *t = w->ts[which];
    if (x.lane == 0) epnp_compute_ccs(w, w->Betas[which]);
    x.sync();
    CVX_NOUNROLL for (int i = x.lane; i < n; i += x.lanes) { // compute_pcs
        const double *a = w->alphas + 4 * i;
        double *pc = w->pcs + 3 * i;
        CVX_NOUNROLL for (int j = 0; j < 3; j++) pc[j] = a[0] * w->ccs[0][j] + a[1] * w->ccs[1][j] + a[2] * w->ccs[2][j] + a[3] * w->ccs[3][j];
    }
    x.sync();
    if (x.lane == 0) w->sign = w->pcs[2] < 0.0; // solve_for_sign
    x.sync();
    if (w->sign) {
        if (x.lane == 0)
            CVX_NOUNROLL for (int i = 0; i < 4; i++)
                CVX_NOUNROLL for (int j = 0; j < 3; j++) w->ccs[i][j] = -w->ccs[i][j];
        CVX_NOUNROLL for (int i = x.lane; i < n; i += x.lanes) {
            w->pcs[3 * i] = -w->pcs[3 * i];
            w->pcs[3 * i + 1] = -w->pcs[3 * i + 1];
            w->pcs[3 * i + 2] = -w->pcs[3 * i + 2];
        }
    }
    x.sync();
    CVX_NOUNROLL for (int e = x.lane; e < 6; e += x.lanes) { // estimate_R_and_t
        const int j = e % 3;
        const double *src = e < 3 ? w->pcs : w->pws;
        double s = 0.0;
        CVX_NOUNROLL for (int i = 0; i < n; i++) s += src[3 * i + j];
        (e < 3 ? w->pc0 : w->pw0)[j] = s / n;
    }
    x.sync();
    CVX_NOUNROLL for (int e = x.lane; e < 9; e += x.lanes) {
        const int j = e / 3, c = e % 3;
        double s = 0.0;
        CVX_NOUNROLL for (int i = 0; i < n; i++) s += (w->pcs[3 * i + j] - w->pc0[j]) * (w->pws[3 * i + c] - w->pw0[c]);
        w->abt[e] = s;
    }
    x.sync();
    cvx_svd_uv(x, w->abt, 3, w->abt_d, w->abt_u, w->abt_v, w->svd);
    if (x.lane == 0) {
        CVX_NOUNROLL for (int i = 0; i < 3; i++)
            CVX_NOUNROLL for (int j = 0; j < 3; j++) R[i][j] = epnp_dot(w->abt_u + 3 * i, w->abt_v + 3 * j);
        const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] -
                           R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
        if (det < 0) {
            R[2][0] = -R[2][0];
            R[2][1] = -R[2][1];
            R[2][2] = -R[2][2];
        }
        t[0] = w->pc0[0] - epnp_dot(R[0], w->pw0);
        t[1] = w->pc0[1] - epnp_dot(R[1], w->pw0);
        t[2] = w->pc0[2] - epnp_dot(R[2], w->pw0);
    }
    x.sync();
    CVX_NOUNROLL for (int i = x.lane; i < n; i += x.lanes) { // reprojection_error
        const double *pw = w->pws + 3 * i;
        const double Xc = epnp_dot(R[0], pw) + t[0];
        const double Yc = epnp_dot(R[1], pw) + t[1];
        const double inv_Zc = 1.0 / (epnp_dot(R[2], pw) + t[2]);
        const double ue = w->uc + w->fu * Xc * inv_Zc;
        const double ve = w->vc + w->fv * Yc * inv_Zc;
        const double u = w->us[2 * i], v = w->us[2 * i + 1];
        w->terms[i] = sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    x.sync();
    if (x.lane == 0) {
        double sum2 = 0.0;
        CVX_NOUNROLL for (int i = 0; i < n; i++) sum2 += w->terms[i];
        w->rep_errors[which] = sum2 / n;
    }
    x.sync();
}

// compute_pose on the w->n correspondences in w->pws / w->us -> R[9] row-major, t[3] (written by lane 0); returns the index N chosen at :523-527
template <class X> HD __attribute__((always_inline)) int epnp_compute_pose(X x, EpnpWork *w, double *R, double *t) {
    epnp_choose_control_points(x, w);
    epnp_compute_barycentric_coordinates(x, w);
    epnp_compute_MtM(x, w);
    cvx_svd_sym_ut(x, w->mtm, 12, w->d, w->ut);
    if (x.lane == 0) {
        epnp_compute_L_6x10(w);
        epnp_compute_rho(w);
    }
    x.sync();
    CVX_NOUNROLL for (int which = 1; which <= 3; which++) {
        epnp_find_betas_approx(x, w, which, w->Betas[which]);
        if (x.lane == 0) epnp_gauss_newton(w, w->Betas[which]);
        x.sync();
        epnp_compute_R_and_t(x, w, which);
    }
    int N = 1;
    if (w->rep_errors[2] < w->rep_errors[1]) N = 2;
    if (w->rep_errors[3] < w->rep_errors[N]) N = 3;
    if (x.lane == 0) { // copy_R_and_t
        CVX_NOUNROLL for (int i = 0; i < 3; i++) {
            CVX_NOUNROLL for (int j = 0; j < 3; j++) R[3 * i + j] = w->Rs[N][i][j];
            t[i] = w->ts[N][i];
        }
    }
    x.sync();
    return N;
}

// mvbInliersi[i] of CheckInliers (:311-326): mRi row-major, mti; K = fu fv uc vc
HD bool epnp_is_inlier(const double *mRi, const double *mti, const double *K, const float *P3Dw, const float *P2D, float max_error) {
    const float Xc = (float)(mRi[0] * P3Dw[0] + mRi[1] * P3Dw[1] + mRi[2] * P3Dw[2] + mti[0]);
    const float Yc = (float)(mRi[3] * P3Dw[0] + mRi[4] * P3Dw[1] + mRi[5] * P3Dw[2] + mti[1]);
    const float invZc = (float)(1 / (mRi[6] * P3Dw[0] + mRi[7] * P3Dw[1] + mRi[8] * P3Dw[2] + mti[2]));
    const double ue = K[2] + K[0] * Xc * invZc;
    const double ve = K[3] + K[1] * Yc * invZc;
    const float distX = (float)(P2D[0] - ue);
    const float distY = (float)(P2D[1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_error;
}
