// g2o::Sim3 (vendored g2o types/sim3.h) spelled out in Eigen's evaluation order, for the Sim3 refinement kernel (sim3opt.hip) and the pose graph (posegraph.hip): the
// exponential and the logarithm with their four branches each, product, inverse and map.  No function renormalises the quaternion -- Sim3 never does.  Quat, qmul, qrot
// and qtoR are se3_math.h's.
#pragma once
#include "se3_math.h"

namespace {

struct Sim3 { Quat r; double t[3]; double s; };

// Eigen Quaterniond(Matrix3d) as qfromR, with the three cyclic cases of its second branch written out so that no index is a run-time value
HD Quat sim3_qfromR(const double m[3][3]) {
    Quat q;
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = sqrt(t + 1.0); q.w = 0.5 * t; t = 0.5 / t;
        q.x = (m[2][1] - m[1][2]) * t; q.y = (m[0][2] - m[2][0]) * t; q.z = (m[1][0] - m[0][1]) * t;
        return q;
    }
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > (i == 1 ? m[1][1] : m[0][0])) i = 2;
    if (i == 0) {
        t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0); q.x = 0.5 * t; t = 0.5 / t;
        q.w = (m[2][1] - m[1][2]) * t; q.y = (m[1][0] + m[0][1]) * t; q.z = (m[2][0] + m[0][2]) * t;
    } else if (i == 1) {
        t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0); q.y = 0.5 * t; t = 0.5 / t;
        q.w = (m[0][2] - m[2][0]) * t; q.z = (m[2][1] + m[1][2]) * t; q.x = (m[0][1] + m[1][0]) * t;
    } else {
        t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0); q.z = 0.5 * t; t = 0.5 / t;
        q.w = (m[1][0] - m[0][1]) * t; q.x = (m[0][2] + m[2][0]) * t; q.y = (m[1][2] + m[2][1]) * t;
    }
    return q;
}

// Sim3(const Vector7d &update) (sim3.h:70-142): update = (omega, upsilon, sigma)
HD Sim3 sim3_exp(const double *u) {
    const double omega[3] = {u[0], u[1], u[2]}, sigma = u[6];
    const double theta = sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
    const double Om[3][3] = {{0.0, -omega[2], omega[1]}, {omega[2], 0.0, -omega[0]}, {-omega[1], omega[0], 0.0}}; // skew (se3_ops.hpp:27-38)
    Sim3 S;
    S.s = exp(sigma);
    double Om2[3][3], R[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { double v = Om[i][0] * Om[0][j]; v += Om[i][1] * Om[1][j]; v += Om[i][2] * Om[2][j]; Om2[i][j] = v; }
    const double eps = 0.00001;
    double A, B, C;
    const bool small_theta = theta < eps;
    if (small_theta) { // R = I + Omega + Omega * Omega: not orthonormal
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + Om[i][j]) + Om2[i][j];
    } else {
        const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + a * Om[i][j]) + b * Om2[i][j];
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) { A = 1. / 2.; B = 1. / 6.; }
        else { const double theta2 = theta * theta; A = (1 - cos(theta)) / (theta2); B = (theta - sin(theta)) / (theta2 * theta); }
    } else {
        C = (S.s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double a = S.s * sin(theta), b = S.s * cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    S.r = sim3_qfromR(R);
    for (int i = 0; i < 3; i++) { // t = (A * Omega + B * Omega2 + C * I) * upsilon
        double W[3];
        for (int j = 0; j < 3; j++) W[j] = (A * Om[i][j] + B * Om2[i][j]) + C * (i == j ? 1.0 : 0.0);
        double v = W[0] * u[3]; v += W[1] * u[4]; v += W[2] * u[5];
        S.t[i] = v;
    }
    return S;
}
HD void sim3_map(const Sim3 &S, const double *p, double *o) { // s * (r * xyz) + t
    double r[3];
    qrot(S.r, p, r);
    o[0] = S.s * r[0] + S.t[0]; o[1] = S.s * r[1] + S.t[1]; o[2] = S.s * r[2] + S.t[2];
}
HD Sim3 sim3_inverse(const Sim3 &S) { // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    Sim3 I;
    I.r = Quat{-S.r.x, -S.r.y, -S.r.z, S.r.w};
    const double k = -1. / S.s, v[3] = {k * S.t[0], k * S.t[1], k * S.t[2]};
    qrot(I.r, v, I.t);
    I.s = 1. / S.s;
    return I;
}
HD Sim3 sim3_mul(const Sim3 &a, const Sim3 &b) {
    Sim3 c;
    double r[3];
    c.r = qmul(a.r, b.r);
    qrot(a.r, b.t, r);
    c.t[0] = a.s * r[0] + a.t[0]; c.t[1] = a.s * r[1] + a.t[1]; c.t[2] = a.s * r[2] + a.t[2];
    c.s = a.s * b.s;
    return c;
}
// W.lu().solve(t) for a 3 x 3 W: PartialPivLU's unblocked elimination (the first row of largest magnitude is the pivot, the column is divided by it, the corner
// gets its rank-1 update), then the unit-lower and the upper substitution on the permuted right-hand side.  Rows are swapped whole under compile-time indices.
HD void sim3_lu_solve3(const double W[3][3], const double *t, double *x) {
    double a0[3] = {W[0][0], W[0][1], W[0][2]}, a1[3] = {W[1][0], W[1][1], W[1][2]}, a2[3] = {W[2][0], W[2][1], W[2][2]};
    double b0 = t[0], b1 = t[1], b2 = t[2], v;
    int p = 0;
    if (fabs(a1[0]) > fabs(a0[0])) p = 1;
    if (fabs(a2[0]) > fabs(p == 1 ? a1[0] : a0[0])) p = 2;
    if (p == 1) { for (int j = 0; j < 3; j++) { v = a0[j]; a0[j] = a1[j]; a1[j] = v; } v = b0; b0 = b1; b1 = v; }
    if (p == 2) { for (int j = 0; j < 3; j++) { v = a0[j]; a0[j] = a2[j]; a2[j] = v; } v = b0; b0 = b2; b2 = v; }
    a1[0] /= a0[0]; a1[1] -= a1[0] * a0[1]; a1[2] -= a1[0] * a0[2];
    a2[0] /= a0[0]; a2[1] -= a2[0] * a0[1]; a2[2] -= a2[0] * a0[2];
    if (fabs(a2[1]) > fabs(a1[1])) { for (int j = 0; j < 3; j++) { v = a1[j]; a1[j] = a2[j]; a2[j] = v; } v = b1; b1 = b2; b2 = v; }
    a2[1] /= a1[1]; a2[2] -= a2[1] * a1[2];
    b1 -= a1[0] * b0;
    b2 -= a2[0] * b0; b2 -= a2[1] * b1;
    x[2] = b2 / a2[2];
    b1 -= a1[2] * x[2]; x[1] = b1 / a1[1];
    b0 -= a0[1] * x[1]; b0 -= a0[2] * x[2]; x[0] = b0 / a0[0];
}
// Sim3::log (sim3.h:148-230) -> (omega, upsilon, sigma): the four branches on |sigma| < eps and d > 1 - eps, deltaR (se3_ops.hpp:40-47)
HD void sim3_log(const Sim3 &S, double *res) {
    const double sigma = log(S.s), eps = 0.00001;
    double R[3][3];
    qtoR(S.r, R);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    double omega[3], A, B, C;
    const bool small_angle = d > 1 - eps;
    if (small_angle) { omega[0] = 0.5 * dR[0]; omega[1] = 0.5 * dR[1]; omega[2] = 0.5 * dR[2]; }
    const double theta = small_angle ? 0.0 : acos(d);
    if (!small_angle) { const double k = theta / (2 * sqrt(1 - d * d)); omega[0] = k * dR[0]; omega[1] = k * dR[1]; omega[2] = k * dR[2]; }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_angle) { A = 1. / 2.; B = 1. / 6.; }
        else { const double theta2 = theta * theta; A = (1 - cos(theta)) / (theta2); B = (theta - sin(theta)) / (theta2 * theta); }
    } else {
        C = (S.s - 1) / sigma;
        if (small_angle) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta2 = theta * theta, a = S.s * sin(theta), b = S.s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const double Om[3][3] = {{0.0, -omega[2], omega[1]}, {omega[2], 0.0, -omega[0]}, {-omega[1], omega[0], 0.0}};
    double W[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { // W = A * Omega + B * Omega * Omega + C * I
        double v = (B * Om[i][0]) * Om[0][j]; v += (B * Om[i][1]) * Om[1][j]; v += (B * Om[i][2]) * Om[2][j];
        W[i][j] = (A * Om[i][j] + v) + C * (i == j ? 1.0 : 0.0);
    }
    sim3_lu_solve3(W, S.t, res + 3);
    res[0] = omega[0]; res[1] = omega[1]; res[2] = omega[2]; res[6] = sigma;
}
// tx ty tz qx qy qz qw s, the coefficients as they are
HD Sim3 sim3_load(const double *p) { Sim3 S; S.t[0] = p[0]; S.t[1] = p[1]; S.t[2] = p[2]; S.r = Quat{p[3], p[4], p[5], p[6]}; S.s = p[7]; return S; }
HD void sim3_store(const Sim3 &S, double *p) { p[0] = S.t[0]; p[1] = S.t[1]; p[2] = S.t[2]; p[3] = S.r.x; p[4] = S.r.y; p[5] = S.r.z; p[6] = S.r.w; p[7] = S.s; }

} // namespace
