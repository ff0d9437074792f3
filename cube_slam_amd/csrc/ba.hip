// ba.hip -- g2o object bundle adjustment (Levenberg-Marquardt, BlockSolver_6_3 with Schur) on MI355X (gfx950).
//
// Replaces SparseOptimizer::optimize as driven by Optimizer::BundleAdjustment / LocalBACameraPointObjects (reference
// orb_object_slam/src/Optimizer.cc:64-251, :826-1534; vendored g2o core/optimization_algorithm_levenberg.cpp:61-189,
// core/block_solver.hpp:354-604, core/base_binary_edge.hpp:55-320, core/base_unary_edge.hpp:82-123; CubeSLAM types
// orb_object_slam/src/g2o_Object.cpp).  fp64 throughout, like g2o.  Deterministic: every reduction has a fixed order
// (thread per landmark, wave per pose block / Schur block with shuffle trees), no floating-point atomics.
//
//   ba_err_*          computeActiveErrors: reprojection / cuboid bbox / point-in-cuboid residuals + robust chi2 partials
//   ba_build_abc      one grid of three parts that read nothing of each other:
//     _lin_lm_body    thread per landmark: analytic 2x3 / 2x6 Jacobians of its observations, Hll, bl, Hpl blocks
//     _lin_pose_body  wave per pose block: sum_obs Jj^T W Jj and Jj^T W r (lane = observation, shuffle-tree reduce)
//     _num_cols_body  thread per (cuboid edge, perturbed dimension): central difference with delta 1e-9 through the same
//                     oplus (exp map, exptwist_norollpitch) as g2o's numeric linearizeOplus
//   ba_lin_pose_edges lane per element of a pose block: camera-cuboid and point-cuboid terms into Hpp / b
//   ba_lm_dinv        thread per landmark: (Hll + lambda I)^-1 and D^-1 b_l
//   ba_schur_slots    wave per block of the reduced camera system: Hpp - sum_l B D^-1 B^T (lane = contributing landmark)
//   ba_schur_b        wave per pose block: b_p - sum B D^-1 b_l
//   (all-reduce)      one sum over [Schur blocks | b | scalars] across ranks when landmarks are sharded (RCCL via callback)
//   ba_band_*         block-band Cholesky (reverse Cuthill-McKee order from the host) + two triangular sweeps, one workgroup (ba_band.h)
//   ba_backsub        thread per landmark: x_l = D^-1 (b_l - B^T x_p)
//   ba_update         oplus per vertex (cameras: exp(dx) * T; cuboids: T * exp(dx) with the fix-roll-pitch / height / scale flags)
// The graph plan (index mapping, Schur slots, band plan, ordering, symbolic factor) is host code in ba_plan.h; cs_ba_create checks, plans and uploads.
#include "common.h"
#include "ba_cr.h"
#include "ba_plan.h"
#include "lm_schedule.h"
#include "se3_math.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <type_traits>
#include <vector>

namespace {

struct Params { // device-side view of the graph
    int n_cams, L, n_cub, P, n_obs, n_cobs, n_pc, lm_b, lm_e, o_b, o_e, pose_edges; // this rank: landmarks [lm_b, lm_e), obs [o_b, o_e)
    double fx, fy, cx, cy, huber_mono, huber_obj, margin_ratio, K[9], bf, huber_stereo;
    double *cam, *pts, *cub, *cub_scale;           // estimates: 7 / 3 / 7 (+3)
    const int *cam_idx; const uint8_t *cub_flags;
    const int *o_cam, *o_pt; const double *o_uv, *o_w, *o_ur; const int *lm_off; // o_ur: right-image u of a stereo edge (< 0 or NULL array: monocular)
    const int *c_cam, *c_cub; const double *c_bbox, *c_info;
    const int *pc_cub, *pc_off; const double *pc_pts;
    double *e_obs, *e_cobs, *e_pc;
    double *Hpl, *HplD, *Hll, *bl, *Dinv, *db, *Hpp, *bp, *Hoff; // HplD: B D^-1 per observation (6x3), refreshed with every damping value; // Hoff: one 6x6 block per camera-cuboid edge (camera rows, cuboid cols)
    double *Jc, *Jp;                                       // numeric Jacobian columns: cobs x 12 x 4, pc x 6 x 3
    double *x;                                             // 6P + 3L
};

__device__ inline Cuboid load_cuboid(const Params &G, int i) {
    Cuboid c; c.pose = se3_load(G.cub + (long)i * 7);
    for (int k = 0; k < 3; k++) c.scale[k] = G.cub_scale[i * 3 + k];
    return c;
}
__device__ inline void err_cobs_eval(const Params &G, int o, const SE3 &T, const Cuboid &c, double *e) { // EdgeSE3CuboidFixScaleProj::computeError
    double bb[4];
    project_bbox(c, T, G.K, bb);
    for (int k = 0; k < 4; k++) e[k] = bb[k] - G.c_bbox[o * 4 + k];
}
__device__ inline void err_pc_eval(const Params &G, int o, const Cuboid &c, double *e) { // EdgePointCuboidOnlyObjectFixScale::computeError
    double acc[3] = {0, 0, 0};
    const int b0 = G.pc_off[o], b1 = G.pc_off[o + 1];
    const SE3 inv = se3_inv(c.pose);
    const double ratio = G.margin_ratio;
    for (int i = b0; i < b1; i++) {
        double lp[3];
        se3_map(inv, G.pc_pts + (long)i * 3, lp);
        for (int k = 0; k < 3; k++) { // cuboid::point_boundary_error g2o_Object.cpp:280-298
            const double a = fabs(lp[k]) * 1.0;
            double er;
            if (a < c.scale[k]) er = 0;
            else if (a < (ratio + 1) * c.scale[k]) er = a - c.scale[k];
            else er = ratio * c.scale[k];
            acc[k] += fabs(er);
        }
    }
    if (b1 > b0) for (int k = 0; k < 3; k++) acc[k] = acc[k] / (double)(b1 - b0);
    for (int k = 0; k < 3; k++) e[k] = 1.0 * (acc[k] / c.scale[k]);
}

__device__ inline bool obs_stereo(const Params &G, int o) { return G.o_ur && G.o_ur[o] >= 0; }
__device__ __forceinline__ void ba_err_obs_body(const Params &G, double *partials, const int bid) {
    const int o = G.o_b + bid * 256 + threadIdx.x;
    double chi = 0;
    if (o < G.o_e) { // EdgeSE3ProjectXYZ::computeError
        const SE3 T = se3_load(G.cam + (long)G.o_cam[o] * 7);
        double pc[3];
        se3_map(T, G.pts + (long)G.o_pt[o] * 3, pc);
        double e0, e1, e2 = 0.0, delta = G.huber_mono;
        if (obs_stereo(G, o)) { // EdgeStereoSE3ProjectXYZ::cam_project (types_six_dof_expmap.cpp:182-189): invz and bf are floats there
            const float invz = (float)(1.0 / pc[2]);
            const double u = pc[0] * invz * G.fx + G.cx;
            e0 = G.o_uv[o * 2] - u; e1 = G.o_uv[o * 2 + 1] - (pc[1] * invz * G.fy + G.cy); e2 = G.o_ur[o] - (u - (double)((float)G.bf * invz)); // (bf arrives as const float&: the product is a float product)
            chi = ((e0 * e0 + e1 * e1) + e2 * e2) * G.o_w[o];
            delta = G.huber_stereo;
        } else {
            e0 = G.o_uv[o * 2] - (pc[0] / pc[2] * G.fx + G.cx); e1 = G.o_uv[o * 2 + 1] - (pc[1] / pc[2] * G.fy + G.cy);
            chi = (e0 * e0 + e1 * e1) * G.o_w[o];
        }
        G.e_obs[(long)o * 3] = e0; G.e_obs[(long)o * 3 + 1] = e1; G.e_obs[(long)o * 3 + 2] = e2;
        if (delta > 0) { double rho[3]; huber(chi, delta, rho); chi = rho[0]; }
    }
    block_sum_store(chi, partials, bid);
}
__global__ void __launch_bounds__(256) ba_err_obs(Params G, double *partials) { ba_err_obs_body(G, partials, (int)blockIdx.x); }
__device__ __forceinline__ void ba_err_pose_edges_body(const Params &G, double *partials, const int bid) {
    const int t = bid * 256 + threadIdx.x;
    double chi = 0;
    if (t < G.n_cobs) {
        double e[4];
        err_cobs_eval(G, t, se3_load(G.cam + (long)G.c_cam[t] * 7), load_cuboid(G, G.c_cub[t]), e);
        const double *w = G.c_info + (long)t * 4;
        for (int k = 0; k < 4; k++) G.e_cobs[(long)t * 4 + k] = e[k];
        chi = ((e[0] * w[0] * e[0] + e[1] * w[1] * e[1]) + e[2] * w[2] * e[2]) + e[3] * w[3] * e[3];
        if (G.huber_obj > 0) { double rho[3]; huber(chi, G.huber_obj, rho); chi = rho[0]; }
    } else if (t < G.n_cobs + G.n_pc) {
        const int o = t - G.n_cobs;
        double e[3];
        err_pc_eval(G, o, load_cuboid(G, G.pc_cub[o]), e);
        for (int k = 0; k < 3; k++) G.e_pc[(long)o * 3 + k] = e[k];
        chi = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    }
    block_sum_store(chi, partials, bid);
}
__global__ void __launch_bounds__(256) ba_err_pose_edges(Params G, double *partials) { ba_err_pose_edges_body(G, partials, (int)blockIdx.x); }

// analytic Jacobians of one reprojection edge + weights.  Monocular: EdgeSE3ProjectXYZ::linearizeOplus (types_six_dof_expmap.cpp:135-171),
// third row exactly zero.  Stereo: EdgeStereoSE3ProjectXYZ::linearizeOplus (:220-266).
__device__ inline void obs_jac(const Params &G, int o, double Ji[3][3], double Jj[3][6], double omr[3], double &W) {
    const SE3 T = se3_load(G.cam + (long)G.o_cam[o] * 7);
    double pc[3], R[3][3];
    se3_map(T, G.pts + (long)G.o_pt[o] * 3, pc);
    qtoR(T.r, R);
    const double X = pc[0], Y = pc[1], Z = pc[2], Z2 = Z * Z, fx = G.fx, fy = G.fy;
    const bool st = obs_stereo(G, o);
    if (!st) {
        const double tmp[2][3] = {{fx, 0, -X / Z * fx}, {0, fy, -Y / Z * fy}};
        for (int r = 0; r < 2; r++) for (int c = 0; c < 3; c++) Ji[r][c] = ((-1. / Z * tmp[r][0]) * R[0][c] + (-1. / Z * tmp[r][1]) * R[1][c]) + (-1. / Z * tmp[r][2]) * R[2][c];
        for (int c = 0; c < 3; c++) Ji[2][c] = 0;
    } else {
        for (int c = 0; c < 3; c++) {
            Ji[0][c] = -fx * R[0][c] / Z + fx * X * R[2][c] / Z2;
            Ji[1][c] = -fy * R[1][c] / Z + fy * Y * R[2][c] / Z2;
            Ji[2][c] = Ji[0][c] - G.bf * R[2][c] / Z2;
        }
    }
    Jj[0][0] = X * Y / Z2 * fx; Jj[0][1] = -(1 + (X * X / Z2)) * fx; Jj[0][2] = Y / Z * fx; Jj[0][3] = -1. / Z * fx; Jj[0][4] = 0; Jj[0][5] = X / Z2 * fx;
    Jj[1][0] = (1 + Y * Y / Z2) * fy; Jj[1][1] = -X * Y / Z2 * fy; Jj[1][2] = -X / Z * fy; Jj[1][3] = 0; Jj[1][4] = -1. / Z * fy; Jj[1][5] = Y / Z2 * fy;
    if (st) { Jj[2][0] = Jj[0][0] - G.bf * Y / Z2; Jj[2][1] = Jj[0][1] + G.bf * X / Z2; Jj[2][2] = Jj[0][2]; Jj[2][3] = Jj[0][3]; Jj[2][4] = 0; Jj[2][5] = Jj[0][5] - G.bf / Z2; }
    else for (int c = 0; c < 6; c++) Jj[2][c] = 0;
    const double e0 = G.e_obs[(long)o * 3], e1 = G.e_obs[(long)o * 3 + 1], e2 = G.e_obs[(long)o * 3 + 2], w = G.o_w[o];
    const double delta = st ? G.huber_stereo : G.huber_mono;
    double rw = 1.0;
    if (delta > 0) { double rho[3]; huber(st ? ((e0 * e0 + e1 * e1) + e2 * e2) * w : (e0 * e0 + e1 * e1) * w, delta, rho); rw = rho[1]; }
    omr[0] = -w * e0 * rw; omr[1] = -w * e1 * rw; omr[2] = -w * e2 * rw; // omega_r = -Omega e, scaled by rho' (base_binary_edge.hpp:77,96)
    W = rw * w;                                                          // robustInformation = rho' * Omega (base_edge.h:96-102)
}

__device__ __forceinline__ void ba_lin_lm_body(const Params &G, const int bid) { // thread per landmark of this rank
    const int li = G.lm_b + bid * 256 + threadIdx.x;
    if (li >= G.lm_e) return;
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    for (int o = G.lm_off[li]; o < G.lm_off[li + 1]; o++) {
        double Ji[3][3], Jj[3][6], omr[3], W;
        obs_jac(G, o, Ji, Jj, omr, W);
        for (int a = 0; a < 3; a++) { // third row: zero for monocular edges, so their sums are unchanged by it
            b[a] += (Ji[0][a] * omr[0] + Ji[1][a] * omr[1]) + Ji[2][a] * omr[2];
            for (int c = 0; c < 3; c++) H[a * 3 + c] += ((Ji[0][a] * W) * Ji[0][c] + (Ji[1][a] * W) * Ji[1][c]) + (Ji[2][a] * W) * Ji[2][c];
        }
        double *hx = G.Hpl + (long)o * 18; // Hpl block (pose rows, landmark cols) = Jj^T W Ji
        for (int a = 0; a < 6; a++) for (int c = 0; c < 3; c++) hx[a * 3 + c] = ((Jj[0][a] * W) * Ji[0][c] + (Jj[1][a] * W) * Ji[1][c]) + (Jj[2][a] * W) * Ji[2][c];
    }
    for (int k = 0; k < 9; k++) G.Hll[(long)li * 9 + k] = H[k];
    for (int k = 0; k < 3; k++) G.bl[(long)li * 3 + k] = b[k];
}

// workgroup per pose block (four waves share the camera's observation list: a thousand single waves leave the SIMDs one wave deep and the
// Jacobian chain exposed): observations of this rank that involve the camera (CSR pose_off / pose_obs); wave sums by shuffles, then in wave order
__device__ __forceinline__ void ba_lin_pose_body(const Params &G, const int *pose_off, const int *pose_obs, const int bid) {
    __shared__ double part[4][42];
    const int pi = bid, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc[42];
#pragma unroll
    for (int k = 0; k < 42; k++) acc[k] = 0;
    for (int q = pose_off[pi] + (int)threadIdx.x; q < pose_off[pi + 1]; q += 256) {
        double Ji[3][3], Jj[3][6], omr[3], W;
        obs_jac(G, pose_obs[q], Ji, Jj, omr, W);
#pragma unroll
        for (int a = 0; a < 6; a++) {
            acc[36 + a] += (Jj[0][a] * omr[0] + Jj[1][a] * omr[1]) + Jj[2][a] * omr[2];
#pragma unroll
            for (int c = 0; c < 6; c++) acc[a * 6 + c] += ((Jj[0][a] * W) * Jj[0][c] + (Jj[1][a] * W) * Jj[1][c]) + (Jj[2][a] * W) * Jj[2][c];
        }
    }
#pragma unroll
    for (int k = 0; k < 42; k++) for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
    if (lane == 0) for (int k = 0; k < 42; k++) part[wv][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 42) {
        const int k = threadIdx.x;
        const double v = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
        if (k < 36) G.Hpp[(long)pi * 36 + k] = v; else G.bp[(long)pi * 6 + k - 36] = v;
    }
}

// numeric Jacobian columns (base_binary_edge.hpp:216-320, base_unary_edge.hpp:82-123): delta = 1e-9, central difference.  A lane per (edge, column,
// SIGN): the even lane evaluates the error at +delta, its odd neighbour at -delta (the two evaluations are the whole cost: se3 exponential, cuboid
// retraction, projection), the difference is taken by the even lane -- the same two values, the same subtraction.
__device__ __forceinline__ void ba_num_cols_body(const Params &G, const int bid) {
    const int tt = bid * 256 + threadIdx.x, t = tt >> 1;
    const bool minus = tt & 1;
    const double delta = 1e-9, scalar = 1.0 / (2 * delta), dd = minus ? -delta : delta;
    double ev[4] = {0, 0, 0, 0};
    int kind = 0, o = 0, d = 0; // 1: camera-cuboid column, 2: point-cuboid column
    if (t < G.n_cobs * 12) {
        o = t / 12; d = t % 12;
        const int ci = G.c_cam[o], oi = G.c_cub[o];
        if (d >= 6 || G.cam_idx[ci] >= 0) {
            kind = 1;
            const SE3 T = se3_load(G.cam + (long)ci * 7);
            const Cuboid C = load_cuboid(G, oi);
            double add[6] = {0, 0, 0, 0, 0, 0};
            if (d < 6) { add[d] = dd; err_cobs_eval(G, o, se3_mul(se3_exp(add), T), C, ev); } // camera: VertexSE3Expmap::oplusImpl = exp(update) * estimate
            else { add[d - 6] = dd; err_cobs_eval(G, o, T, cuboid_oplus(C, add, G.cub_flags[oi], G.cub_scale + (long)oi * 3), ev); }
        }
    } else if (t < G.n_cobs * 12 + G.n_pc * 6) {
        kind = 2;
        const int u = t - G.n_cobs * 12;
        o = u / 6; d = u % 6;
        const int oi = G.pc_cub[o];
        const Cuboid C = load_cuboid(G, oi);
        double add[6] = {0, 0, 0, 0, 0, 0};
        add[d] = dd; err_pc_eval(G, o, cuboid_oplus(C, add, G.cub_flags[oi], G.cub_scale + (long)oi * 3), ev);
    }
    double em[4];
#pragma unroll
    for (int k = 0; k < 4; k++) em[k] = __shfl_xor(ev[k], 1); // the other sign's errors (both lanes of a pair take the same branch)
    if (minus) return;
    if (kind == 1) for (int k = 0; k < 4; k++) G.Jc[((long)o * 12 + d) * 4 + k] = scalar * (ev[k] - em[k]);
    else if (kind == 2) for (int k = 0; k < 3; k++) G.Jp[((long)o * 6 + d) * 3 + k] = scalar * (ev[k] - em[k]);
}
// The three launches of buildSystem that read nothing of each other, as ONE grid: workgroups [0, n_pose) are ba_lin_pose's, the next n_cols ba_num_cols', the rest
// ba_lin_lm's (the longest first).  At 1 000 key frames each of them fills part of the chip for 30 - 65 us; in a row they were 141 us, side by side they are the longest
// of them.  (Two more streams with event joins were measured first: a join costs more than the kernels it orders, 1 040 -> 544 it/s.)
__global__ void __launch_bounds__(256) ba_build_abc(Params G, const int *pose_off, const int *pose_obs, int n_pose, int n_cols) {
    const int bid = (int)blockIdx.x;
    if (bid < n_pose) ba_lin_pose_body(G, pose_off, pose_obs, bid);
    else if (bid < n_pose + n_cols) ba_num_cols_body(G, bid - n_pose);
    else ba_lin_lm_body(G, bid - n_pose - n_cols);
}

// A lane per ELEMENT of a pose block (36 of H, 6 of b; a wave per pose): adds the camera-cuboid / point-cuboid terms (constructQuadraticForm) in edge
// order -- every element is the same sum in the same order as with a thread per block, 42 lanes wide instead of a chain of 42 accumulators per thread
// (1500 threads had the six workgroups of the launch walk their edge lists alone: 71 us).  The same for the off-diagonal Hpp block of a
// camera-cuboid edge: a lane per element.  pe_off/pe_list: per pose block, incident edges encoded as (edge << 2) | kind, kind 0 = cobs seen from
// the camera, 1 = cobs seen from the cuboid, 2 = point-cuboid edge
__global__ void __launch_bounds__(256) ba_lin_pose_edges(Params G, const int *pe_off, const int *pe_list) {
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave < G.P) {
        const int t = wave;
        if (lane >= 42) return;
        const bool isb = lane >= 36;
        const int a = isb ? lane - 36 : lane / 6, c = isb ? 0 : lane % 6;
        double acc = isb ? G.bp[(long)t * 6 + a] : G.Hpp[(long)t * 36 + lane];
        for (int q = pe_off[t]; q < pe_off[t + 1]; q++) {
            const int kind = pe_list[q] & 3, o = pe_list[q] >> 2;
            if (kind < 2) {
                const double *J = G.Jc + ((long)o * 12 + (kind ? 6 : 0)) * 4; // column-major: J[d*4 + k]
                const double *e = G.e_cobs + (long)o * 4, *w = G.c_info + (long)o * 4;
                double rw = 1.0;
                if (G.huber_obj > 0) { double rho[3]; huber(((e[0] * w[0] * e[0] + e[1] * w[1] * e[1]) + e[2] * w[2] * e[2]) + e[3] * w[3] * e[3], G.huber_obj, rho); rw = rho[1]; }
                if (isb) { double sb = 0; for (int k = 0; k < 4; k++) sb += J[a * 4 + k] * (-w[k] * e[k] * rw); acc += sb; }
                else { double sh = 0; for (int k = 0; k < 4; k++) sh += (J[a * 4 + k] * (rw * w[k])) * J[c * 4 + k]; acc += sh; }
            } else {
                const double *J = G.Jp + (long)o * 18, *e = G.e_pc + (long)o * 3; // information = I, no kernel
                if (isb) acc += ((J[a * 3] * -e[0]) + (J[a * 3 + 1] * -e[1])) + (J[a * 3 + 2] * -e[2]);
                else acc += ((J[a * 3] * J[c * 3]) + (J[a * 3 + 1] * J[c * 3 + 1])) + (J[a * 3 + 2] * J[c * 3 + 2]);
            }
        }
        if (isb) G.bp[(long)t * 6 + a] = acc; else G.Hpp[(long)t * 36 + lane] = acc;
    } else if (wave < G.P + G.n_cobs) {
        const int o = wave - G.P;
        if (lane >= 36 || G.cam_idx[G.c_cam[o]] < 0) return;
        const int a = lane / 6, c = lane % 6;
        const double *Ja = G.Jc + (long)o * 48, *Jb = Ja + 24, *e = G.e_cobs + (long)o * 4, *w = G.c_info + (long)o * 4;
        double rw = 1.0;
        if (G.huber_obj > 0) { double rho[3]; huber(((e[0] * w[0] * e[0] + e[1] * w[1] * e[1]) + e[2] * w[2] * e[2]) + e[3] * w[3] * e[3], G.huber_obj, rho); rw = rho[1]; }
        double sh = 0;
        for (int k = 0; k < 4; k++) sh += (Ja[a * 4 + k] * (rw * w[k])) * Jb[c * 4 + k];
        G.Hoff[(long)o * 36 + lane] = sh;
    }
}

__global__ void __launch_bounds__(256) ba_lm_dinv(Params G, double lambda) { // block_solver.hpp:383-395
    const int li = G.lm_b + blockIdx.x * 256 + threadIdx.x;
    if (li >= G.lm_e) return;
    double D[9], Di[9];
    for (int k = 0; k < 9; k++) D[k] = G.Hll[(long)li * 9 + k];
    D[0] += lambda; D[4] += lambda; D[8] += lambda;
    auto cf = [&](int i, int j) { int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3; return D[i1 * 3 + j1] * D[i2 * 3 + j2] - D[i1 * 3 + j2] * D[i2 * 3 + j1]; };
    const double c00 = cf(0, 0), c10 = cf(1, 0), c20 = cf(2, 0);
    const double det = (c00 * D[0] + c10 * D[3]) + c20 * D[6], inv = 1.0 / det;
    Di[0] = c00 * inv; Di[1] = c10 * inv; Di[2] = c20 * inv;
    Di[3] = cf(0, 1) * inv; Di[4] = cf(1, 1) * inv; Di[5] = cf(2, 1) * inv;
    Di[6] = cf(0, 2) * inv; Di[7] = cf(1, 2) * inv; Di[8] = cf(2, 2) * inv;
    const double *b = G.bl + (long)li * 3;
    for (int k = 0; k < 9; k++) G.Dinv[(long)li * 9 + k] = Di[k];
    for (int a = 0; a < 3; a++) G.db[(long)li * 3 + a] = (Di[a * 3] * b[0] + Di[a * 3 + 1] * b[1]) + Di[a * 3 + 2] * b[2];
}

// wave per block of the reduced system.  slot s < P: diagonal block of pose s; P <= s < P + n_cobs: camera-cuboid block;
// the rest: camera-camera blocks created by shared landmarks.  trip_*: contributing (obs_u, obs_v) pairs, this rank only.
// B D^-1 of every observation of this rank (6x3 per observation): each is used by all the pairs its observation takes part in
// (k(k+1)/2 pairs for a landmark seen k times), so it is formed once here instead of once per pair
__global__ void __launch_bounds__(256) ba_schur_bd(Params G, double *w) { // thread per row of a block: neighbouring lanes touch neighbouring 24-byte rows
    const long t = (long)G.o_b * 6 + (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)G.o_e * 6) return;
    const int u = (int)(t / 6);
    const long pt = G.o_pt[u];
    const double *Bi = G.Hpl + t * 3, *Di = G.Dinv + pt * 9, *d = G.db + pt * 3;
    const double b0 = Bi[0], b1 = Bi[1], b2 = Bi[2];
    double *o = G.HplD + t * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (b0 * Di[c] + b1 * Di[3 + c]) + b2 * Di[6 + c];
    w[t] = (b0 * d[0] + b1 * d[1]) + b2 * d[2]; // row of B (D^-1 b_l): summed per pose by ba_schur_b
}
// 18 doubles of a 6x3 block with nine 16-byte loads (blocks are 144 bytes apart in 256-byte-aligned arenas): the pair loop is bound by
// the number of gathered lanes per load instruction, not by their width
__device__ __forceinline__ void load_block18(const double *p, double (&v)[18]) {
    const double2 *q = reinterpret_cast<const double2 *>(__builtin_assume_aligned(p, 16));
#pragma unroll
    for (int k = 0; k < 9; k++) { const double2 t = q[k]; v[2 * k] = t.x; v[2 * k + 1] = t.y; }
}
// The 64 pairs of a wave iteration need 128 blocks of 144 bytes from arbitrary places.  A lane fetching its own two blocks makes
// every load instruction touch 64 different cache lines (the gather cost is per line touched per instruction: 18 instructions x 64
// lines); instead the wave fetches the 128 blocks cooperatively -- 16 bytes per lane, nine consecutive lanes on one block, so an
// instruction touches ~11 lines -- into LDS, and every lane then reads its pair from there.  Same arithmetic, same lane -> pair
// assignment and the same reduction as a per-lane gather, so the sums are bit-identical to it.
__global__ void __launch_bounds__(256) ba_schur_slots(Params G, int n_slots, const int *slot_perm, const int *slot_off, const int2 *trips, double lambda, double *S) {
    __shared__ double2 s_blk[4][64 * 9]; // one operand at a time (B D^-1 of the 64 pairs, then B): 9 KB per wave keeps 16 waves per CU
    __shared__ int s_idx[4][128];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (blockIdx.x * 4 + wv >= n_slots) return; // whole wave; no workgroup barrier below
    // slot_perm: workgroup b runs on XCD b % 8 (observed dispatch rule), and the permutation gives every XCD a contiguous range of
    // the trajectory, so the B / B D^-1 blocks of a camera's observations -- shared by the ~Bc slots of that camera -- are fetched
    // into one XCD's L2 instead of all eight (fabric reads 557 MB -> see DESIGN.md 7.5); speed only, the sums do not change
    const int s = slot_perm[blockIdx.x * 4 + wv];
    double2 *sb = s_blk[wv];
    int *si = s_idx[wv];
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; k++) acc[k] = 0;
    const int qe = slot_off[s + 1];
    int2 tn = (slot_off[s] + lane < qe) ? trips[slot_off[s] + lane] : make_int2(-1, -1); // the pair list is read one iteration ahead
    for (int q0 = slot_off[s]; q0 < qe; q0 += 64) {
        const int2 t = tn;
        const bool valid = t.x >= 0;
        if (q0 + 64 < qe) tn = (q0 + 64 + lane < qe) ? trips[q0 + 64 + lane] : make_int2(-1, -1);
        si[lane] = t.x; si[64 + lane] = t.y;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        double BD[18], Bj[18];
#pragma unroll
        for (int half = 0; half < 2; half++) {
            double2 pv[9]; // all requests first, then the LDS stores: a store right after its load would expose every round trip
#pragma unroll
            for (int it = 0; it < 9; it++) {
                const int p = it * 64 + lane, blk = (p * 7282) >> 16, piece = p - blk * 9; // p / 9 for p < 1152
                const int id = max(si[half * 64 + blk], 0); // pairs past the end of the list read block 0; their lanes do not accumulate
                pv[it] = reinterpret_cast<const double2 *>(__builtin_assume_aligned((half == 0 ? G.HplD : G.Hpl) + (long)id * 18, 16))[piece];
            }
#pragma unroll
            for (int it = 0; it < 9; it++) sb[it * 64 + lane] = pv[it];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < 9; k++) { const double2 a = sb[lane * 9 + k]; if (half == 0) { BD[2 * k] = a.x; BD[2 * k + 1] = a.y; } else { Bj[2 * k] = a.x; Bj[2 * k + 1] = a.y; } }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
        if (valid) {
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int c = 0; c < 6; c++) acc[a * 6 + c] -= (BD[a * 3] * Bj[c * 3] + BD[a * 3 + 1] * Bj[c * 3 + 1]) + BD[a * 3 + 2] * Bj[c * 3 + 2];
        }
    }
#pragma unroll
    for (int k = 0; k < 36; k++) for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
    if (lane == 0) {
        if (s < G.P) for (int k = 0; k < 36; k++) acc[k] += G.Hpp[(long)s * 36 + k] + ((G.pose_edges && (k % 7) == 0) ? lambda : 0.0); // setLambda on rank 0 only
        else if (s < G.P + G.n_cobs) { if (G.pose_edges && G.cam_idx[G.c_cam[s - G.P]] >= 0) for (int k = 0; k < 36; k++) acc[k] += G.Hoff[(long)(s - G.P) * 36 + k]; }
        for (int k = 0; k < 36; k++) S[(long)s * 36 + k] = acc[k];
    }
}
// per-pose sums of the rows w = B (D^-1 b_l) that ba_schur_bd wrote (48 bytes per observation instead of a 168-byte gather)
__global__ void __launch_bounds__(256) ba_schur_b(Params G, const int *pose_off, const int *pose_obs, const double *w, double *bs) { // workgroup per pose, as ba_lin_pose
    __shared__ double part[4][6];
    const int pi = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int q = pose_off[pi] + (int)threadIdx.x; q < pose_off[pi + 1]; q += 256) {
        const double2 *wo = reinterpret_cast<const double2 *>(__builtin_assume_aligned(w + (long)pose_obs[q] * 6, 16));
        const double2 w0 = wo[0], w1 = wo[1], w2 = wo[2];
        acc[0] -= w0.x; acc[1] -= w0.y; acc[2] -= w1.x; acc[3] -= w1.y; acc[4] -= w2.x; acc[5] -= w2.y;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
    if (lane == 0) for (int k = 0; k < 6; k++) part[wv][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 6) { const int k = threadIdx.x; bs[(long)pi * 6 + k] = G.bp[(long)pi * 6 + k] + (((part[0][k] + part[1][k]) + part[2][k]) + part[3][k]); }
}

// ------------------------------------------------------------------------------------------------ band path of the reduced solve
// When no two cuboids share a block of the reduced system (always true for the graphs Optimizer.cc builds: cuboids only meet
// cameras) the cuboids are eliminated like landmarks -- 6x6 blocks, independent, in parallel -- and what remains is a system
// over the cameras whose blocks couple cameras that share a landmark or a cuboid.  For a trajectory that is block-banded with a
// small half-width Bc (9 for the 1k-keyframe benchmark graph), and it is factored by ONE workgroup that keeps the active
// (Bc+1) x (Bc+1) window of blocks in LDS: no global-memory round trip on the critical path of a column (the sparse kernel
// below pays three per column).  Exact same system as BlockSolver::solve, different elimination order (round-off only).
struct CubInv { double D[36]; double g[6]; };

// D_q = (H_qq)^-1 (Cholesky inverse), g_q = D_q b_q.  S: slots, bs: right-hand side of the reduced system (6P)
__global__ void __launch_bounds__(64) ba_cub_inv(int C, int Q, const double *S, const double *bs, double *cubD, double *cubg, int *status) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= Q) return;
    double A[36], Li[36];
    const double *H = S + (long)(C + q) * 36;
    for (int k = 0; k < 36; k++) A[k] = H[k];
    bool fail = false;
    for (int c = 0; c < 6; c++) { // A = L L^T, in place (lower)
        double d = A[c * 6 + c];
        for (int t = 0; t < c; t++) d -= A[c * 6 + t] * A[c * 6 + t];
        if (!(d > 0)) { fail = true; d = 1; }
        d = sqrt(d);
        A[c * 6 + c] = d;
        for (int r = c + 1; r < 6; r++) { double v = A[r * 6 + c]; for (int t = 0; t < c; t++) v -= A[r * 6 + t] * A[c * 6 + t]; A[r * 6 + c] = v / d; }
    }
    for (int c = 0; c < 6; c++) // Li = L^-1 (lower)
        for (int r = 0; r < 6; r++) {
            if (r < c) { Li[r * 6 + c] = 0; continue; }
            double v = r == c ? 1.0 : 0.0;
            for (int t = c; t < r; t++) v -= A[r * 6 + t] * Li[t * 6 + c];
            Li[r * 6 + c] = v / A[r * 6 + r];
        }
    double *D = cubD + (long)q * 36, *g = cubg + (long)q * 6;
    for (int r = 0; r < 6; r++)
        for (int c = 0; c < 6; c++) { double v = 0; for (int t = (r > c ? r : c); t < 6; t++) v += Li[t * 6 + r] * Li[t * 6 + c]; D[r * 6 + c] = v; }
    const double *bq = bs + (long)(C + q) * 6;
    for (int r = 0; r < 6; r++) { double v = 0; for (int c = 0; c < 6; c++) v += D[r * 6 + c] * bq[c]; g[r] = v; }
    if (fail) *status = 1;
}
// band[target] = camera block of the reduced system - sum over the cuboids seen by both cameras of H_iq D_q H_kq^T.
// One thread per (target block, element); fixed summation order.  ct_list: (cuboid, slot of edge (i,q), slot of edge (k,q)).
__device__ __forceinline__ void ba_band_assemble_body(int n_targets, const int *tgt_slot, const uint8_t *tgt_tr, const int *ct_off, const int *ct_list, const double *S,
                                                        const double *cubD, double *band, const int bid) {
    const int t = bid * 256 + threadIdx.x;
    if (t >= n_targets * 36) return;
    const int tg = t / 36, k = t % 36, r = k / 6, c = k % 6;
    double acc = 0;
    const int sl = tgt_slot[tg];
    if (sl >= 0) acc = tgt_tr[tg] ? S[(long)sl * 36 + c * 6 + r] : S[(long)sl * 36 + k];
    for (int e = ct_off[tg]; e < ct_off[tg + 1]; e++) {
        const double *D = cubD + (long)ct_list[e * 3] * 36, *Hi = S + (long)ct_list[e * 3 + 1] * 36 + r * 6, *Hk = S + (long)ct_list[e * 3 + 2] * 36 + c * 6;
        double v = 0;
        for (int a = 0; a < 6; a++) { double w = 0; for (int bb = 0; bb < 6; bb++) w += D[a * 6 + bb] * Hk[bb]; v += Hi[a] * w; }
        acc -= v;
    }
    band[t] = acc;
}
__global__ void __launch_bounds__(256) ba_band_assemble(int n_targets, const int *tgt_slot, const uint8_t *tgt_tr, const int *ct_off, const int *ct_list, const double *S,
                                                        const double *cubD, double *band) { ba_band_assemble_body(n_targets, tgt_slot, tgt_tr, ct_off, ct_list, S, cubD, band, (int)blockIdx.x); }
// rhs_i = b_i - sum over the cuboids seen by camera i of H_iq g_q.  cr_list: (cuboid, slot)
__device__ __forceinline__ void ba_band_rhs_body(int C, const int *cr_off, const int *cr_list, const double *S, const double *bs, const double *cubg, double *rhs, const int bid) {
    const int t = bid * 256 + threadIdx.x;
    if (t >= C * 6) return;
    const int i = t / 6, r = t % 6;
    double acc = bs[t];
    for (int e = cr_off[i]; e < cr_off[i + 1]; e++) {
        const double *g = cubg + (long)cr_list[e * 2] * 6, *H = S + (long)cr_list[e * 2 + 1] * 36 + r * 6;
        double v = 0;
        for (int a = 0; a < 6; a++) v += H[a] * g[a];
        acc -= v;
    }
    rhs[t] = acc;
}
__global__ void __launch_bounds__(256) ba_band_rhs(int C, const int *cr_off, const int *cr_list, const double *S, const double *bs, const double *cubg, double *rhs) { ba_band_rhs_body(C, cr_off, cr_list, S, bs, cubg, rhs, (int)blockIdx.x); }
// x_q = g_q - D_q sum over the cameras that see cuboid q of H_iq^T x_i.  cq_list: (slot, camera)
__device__ __forceinline__ void ba_cub_back_body(int C, int Q, const int *cq_off, const int *cq_list, const double *S, const double *cubD, const double *cubg, double *x, const int q) {
    if (q >= Q) return;
    double w[6] = {0, 0, 0, 0, 0, 0};
    for (int e = cq_off[q]; e < cq_off[q + 1]; e++) {
        const double *H = S + (long)cq_list[e * 2] * 36, *xi = x + (long)cq_list[e * 2 + 1] * 6;
        for (int c = 0; c < 6; c++) { double v = 0; for (int r = 0; r < 6; r++) v += H[r * 6 + c] * xi[r]; w[c] += v; }
    }
    const double *D = cubD + (long)q * 36, *g = cubg + (long)q * 6;
    for (int r = 0; r < 6; r++) { double v = 0; for (int c = 0; c < 6; c++) v += D[r * 6 + c] * w[c]; x[(long)(C + q) * 6 + r] = g[r] - v; }
}
__global__ void __launch_bounds__(64) ba_cub_back(int C, int Q, const int *cq_off, const int *cq_list, const double *S, const double *cubD, const double *cubg, double *x) { ba_cub_back_body(C, Q, cq_off, cq_list, S, cubD, cubg, x, (int)(blockIdx.x * 64 + threadIdx.x)); }
// Pairs of small launches that read nothing of each other, as one grid each (every one of them is 10 - 40 us of mostly launch and tail at 1 000 key frames):
// the band's blocks and its right-hand side; the cuboids' and the landmarks' back-substitution; the scale of the step and the update of the estimates.
__global__ void __launch_bounds__(256) ba_band_both(int nb_a, int n_targets, const int *tgt_slot, const uint8_t *tgt_tr, const int *ct_off, const int *ct_list, const double *S, const double *cubD, double *band,
                                                    int C, const int *cr_off, const int *cr_list, const double *bs, const double *cubg, double *rhs) {
    const int bid = (int)blockIdx.x;
    if (bid < nb_a) ba_band_assemble_body(n_targets, tgt_slot, tgt_tr, ct_off, ct_list, S, cubD, band, bid);
    else ba_band_rhs_body(C, cr_off, cr_list, S, bs, cubg, rhs, bid - nb_a);
}
#include "ba_band.h" // block-band Cholesky of the camera system: BandView ... ba_band_twist_back

// scatter the (all-reduced) blocks of the reduced system into the factor storage Lb = [P diagonal blocks | off-diagonal
// blocks column by column in elimination order]; slot_dst[s] = destination block (-1: dead), slot_tr[s] = transpose
__global__ void ba_chol_fill(int n_slots, const int *slot_dst, const uint8_t *slot_tr, const double *S, double *Lb) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_slots * 36) return;
    const int s = t / 36, k = t % 36, r = k / 6, c = k % 6;
    if (slot_dst[s] < 0) return;
    Lb[(long)slot_dst[s] * 36 + k] = slot_tr[s] ? S[(long)s * 36 + c * 6 + r] : S[t];
}

// Right-looking sparse block Cholesky in a minimum-degree elimination order (symbolic factorisation on the host:
// col_off/rows = structure of every column of L, upd_tgt = destination block of every update pair).  One workgroup.
__global__ void __launch_bounds__(512) ba_chol_factor(int n, const int *col_off, const int *pair_off, const int *upd_tgt, double *Lb, int *status) {
    extern __shared__ double sh[];
    double *Ljj = sh, *Lcol = sh + 36;
    __shared__ int s_fail;
    const int tid = threadIdx.x;
    if (tid == 0) s_fail = 0;
    __syncthreads();
    for (int j = 0; j < n; j++) {
        double *Ajj = Lb + (long)j * 36;
        if (tid == 0) {
            double A[36];
            for (int k = 0; k < 36; k++) A[k] = Ajj[k];
            for (int c = 0; c < 6; c++) {
                double d = A[c * 6 + c];
                for (int t = 0; t < c; t++) d -= A[c * 6 + t] * A[c * 6 + t];
                if (!(d > 0)) { s_fail = 1; d = 1; }
                d = sqrt(d);
                A[c * 6 + c] = d;
                for (int r = c + 1; r < 6; r++) { double v = A[r * 6 + c]; for (int t = 0; t < c; t++) v -= A[r * 6 + t] * A[c * 6 + t]; A[r * 6 + c] = v / d; }
                for (int r = 0; r < c; r++) A[r * 6 + c] = 0;
            }
            for (int k = 0; k < 36; k++) { Ajj[k] = A[k]; Ljj[k] = A[k]; }
        }
        __syncthreads();
        const int c0 = col_off[j], m = col_off[j + 1] - c0;
        for (int t = tid; t < m * 6; t += 512) { // L_ij = A_ij Ljj^-T
            const int bi = t / 6, r = t % 6;
            double *Aij = Lb + ((long)n + c0 + bi) * 36;
            double row[6];
            for (int c = 0; c < 6; c++) { double v = Aij[r * 6 + c]; for (int q = 0; q < c; q++) v -= row[q] * Ljj[c * 6 + q]; row[c] = v / Ljj[c * 6 + c]; }
            for (int c = 0; c < 6; c++) { Aij[r * 6 + c] = row[c]; Lcol[bi * 36 + r * 6 + c] = row[c]; }
        }
        __syncthreads();
        const int npair = m * (m + 1) / 2, p0 = pair_off[j];
        for (int t = tid; t < npair * 36; t += 512) { // A(rows[bi], rows[bk]) -= L_bi L_bk^T, bk <= bi
            const int pr = t / 36, k = t % 36, r = k / 6, c = k % 6;
            int bi = (int)((sqrt(8.0 * pr + 1.0) - 1.0) * 0.5);
            while (bi * (bi + 1) / 2 > pr) bi--;
            while ((bi + 1) * (bi + 2) / 2 <= pr) bi++;
            const int bk = pr - bi * (bi + 1) / 2;
            const double *Li = Lcol + bi * 36 + r * 6, *Lk = Lcol + bk * 36 + c * 6;
            double v = 0;
#pragma unroll
            for (int q = 0; q < 6; q++) v += Li[q] * Lk[q];
            Lb[(long)upd_tgt[p0 + pr] * 36 + k] -= v;
        }
        __syncthreads();
    }
    if (tid == 0) *status = s_fail;
}
// L y = b (column sweep), then L^T x = y (gather per column); xp is the right-hand side in elimination order, in place
__global__ void __launch_bounds__(256) ba_chol_solve(int n, const int *col_off, const int *rows, const double *Lb, double *xp) {
    __shared__ double y[6];
    const int tid = threadIdx.x;
    for (int j = 0; j < n; j++) {
        const double *Ljj = Lb + (long)j * 36;
        if (tid == 0) { for (int r = 0; r < 6; r++) { double v = xp[(long)j * 6 + r]; for (int t = 0; t < r; t++) v -= Ljj[r * 6 + t] * y[t]; y[r] = v / Ljj[r * 6 + r]; } for (int r = 0; r < 6; r++) xp[(long)j * 6 + r] = y[r]; }
        __syncthreads();
        const int c0 = col_off[j], m = col_off[j + 1] - c0;
        for (int t = tid; t < m * 6; t += 256) {
            const int bi = t / 6, r = t % 6;
            const double *Lij = Lb + ((long)n + c0 + bi) * 36 + r * 6;
            double v = 0;
            for (int q = 0; q < 6; q++) v += Lij[q] * y[q];
            xp[(long)rows[c0 + bi] * 6 + r] -= v;
        }
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; j--) {
        const int c0 = col_off[j], m = col_off[j + 1] - c0;
        if (tid < 6) { // y_c = x_j[c] - sum_i (L_ij^T x_i)[c]
            double v = xp[(long)j * 6 + tid];
            for (int bi = 0; bi < m; bi++) {
                const double *Lij = Lb + ((long)n + c0 + bi) * 36, *xi = xp + (long)rows[c0 + bi] * 6;
                for (int q = 0; q < 6; q++) v -= Lij[q * 6 + tid] * xi[q];
            }
            y[tid] = v;
        }
        __syncthreads();
        if (tid == 0) {
            const double *Ljj = Lb + (long)j * 36;
            double x[6];
            for (int r = 5; r >= 0; r--) { double v = y[r]; for (int t = r + 1; t < 6; t++) v -= Ljj[t * 6 + r] * x[t]; x[r] = v / Ljj[r * 6 + r]; }
            for (int r = 0; r < 6; r++) xp[(long)j * 6 + r] = x[r];
        }
        __syncthreads();
    }
}
__global__ void ba_permute(int P, const int *pos, const double *src, double *dst, int forward) { // forward: dst[pos[i]] = src[i]
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P * 6) return;
    const int i = t / 6, k = t % 6;
    if (forward) dst[(long)pos[i] * 6 + k] = src[t]; else dst[t] = src[(long)pos[i] * 6 + k];
}

__device__ __forceinline__ void ba_backsub_body(const Params &G, const int bid) { // x_l = Dinv (b_l - B^T x_p), block_solver.hpp:459-485
    const int li = G.lm_b + bid * 256 + threadIdx.x;
    if (li >= G.lm_e) return;
    double cl[3] = {G.bl[(long)li * 3], G.bl[(long)li * 3 + 1], G.bl[(long)li * 3 + 2]};
    for (int o = G.lm_off[li]; o < G.lm_off[li + 1]; o++) {
        const int pi = G.cam_idx[G.o_cam[o]];
        if (pi < 0) continue;
        const double *Bi = G.Hpl + (long)o * 18, *xpp = G.x + (long)pi * 6;
        for (int c = 0; c < 3; c++) { double s = 0; for (int a = 0; a < 6; a++) s += Bi[a * 3 + c] * xpp[a]; cl[c] -= s; }
    }
    const double *Di = G.Dinv + (long)li * 9;
    for (int a = 0; a < 3; a++) G.x[(long)G.P * 6 + (long)li * 3 + a] = (Di[a * 3] * cl[0] + Di[a * 3 + 1] * cl[1]) + Di[a * 3 + 2] * cl[2];
}
__global__ void __launch_bounds__(256) ba_backsub(Params G) { ba_backsub_body(G, (int)blockIdx.x); }

// sum_j x_j (lambda x_j + b_j) (computeScale :182-189): landmark part of this rank + pose part (b_p partial; lambda term once)
__device__ __forceinline__ void ba_scale_body(const Params &G, double lambda, double *partials, const int bid) {
    const long t = (long)bid * 256 + threadIdx.x, nP = (long)G.P * 6, nL = (long)(G.lm_e - G.lm_b) * 3;
    double v = 0;
    if (t < nP) v = G.x[t] * ((G.pose_edges ? lambda * G.x[t] : 0.0) + G.bp[t]);
    else if (t < nP + nL) { const long k = (long)G.lm_b * 3 + (t - nP); v = G.x[nP + k] * (lambda * G.x[nP + k] + G.bl[k]); }
    block_sum_store(v, partials, bid);
}
__global__ void __launch_bounds__(256) ba_scale(Params G, double lambda, double *partials) { ba_scale_body(G, lambda, partials, (int)blockIdx.x); }
__device__ __forceinline__ void ba_update_body(const Params &G, const int bid) { // SparseOptimizer::update -> oplus per vertex
    const int t = bid * 256 + threadIdx.x;
    if (t < G.n_cams) {
        const int pi = G.cam_idx[t];
        if (pi < 0) return;
        SE3 T = se3_mul(se3_exp(G.x + (long)pi * 6), se3_load(G.cam + (long)t * 7)); // VertexSE3Expmap::oplusImpl types_six_dof_expmap.h:73-91
        se3_store(T, G.cam + (long)t * 7);
    } else if (t < G.n_cams + G.n_cub) {
        const int i = t - G.n_cams, pi = G.P - G.n_cub + i;
        Cuboid c = cuboid_oplus(load_cuboid(G, i), G.x + (long)pi * 6, G.cub_flags[i], G.cub_scale + (long)i * 3);
        se3_store(c.pose, G.cub + (long)i * 7);
    } else {
        const long k = (long)(t - G.n_cams - G.n_cub);
        if (k < (long)(G.lm_e - G.lm_b) * 3) { const long q = (long)G.lm_b * 3 + k; G.pts[q] += G.x[(long)G.P * 6 + q]; } // VertexSBAPointXYZ::oplusImpl
    }
}
__global__ void __launch_bounds__(256) ba_update(Params G) { ba_update_body(G, (int)blockIdx.x); }
__global__ void __launch_bounds__(256) ba_back_both(Params G, int nb_l, int C, int Q, const int *cq_off, const int *cq_list, const double *S, const double *cubD, const double *cubg) {
    const int bid = (int)blockIdx.x, nb_q = (Q + 255) / 256; // the cuboids' few workgroups first: theirs is the longer chain
    if (bid < nb_q) ba_cub_back_body(C, Q, cq_off, cq_list, S, cubD, cubg, G.x, bid * 256 + (int)threadIdx.x);
    else ba_backsub_body(G, bid - nb_q);
}
__global__ void __launch_bounds__(256) ba_scale_update(Params G, double lambda, double *partials, int nb_s) {
    const int bid = (int)blockIdx.x;
    if (bid < nb_s) ba_scale_body(G, lambda, partials, bid);
    else ba_update_body(G, bid - nb_s);
}
__global__ void __launch_bounds__(256) ba_maxdiag(Params G, double *partials) { // max |H_jj| of this rank's landmark blocks (computeLambdaInit)
    const int li = G.lm_b + blockIdx.x * 256 + threadIdx.x;
    double v = 0;
    if (li < G.lm_e) v = fmax(fmax(fabs(G.Hll[(long)li * 9]), fabs(G.Hll[(long)li * 9 + 4])), fabs(G.Hll[(long)li * 9 + 8]));
    __shared__ double s[4];
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = fmax(fmax(s[0], s[1]), fmax(s[2], s[3]));
}

} // namespace

// ------------------------------------------------------------------------------------------------ 9-dof g2o::cuboid (object_slam's graph)
// class cuboid / VertexCuboid / EdgeSE3Cuboid of object_slam/include/object_slam/g2o_Object.h:23-252, SE3Quat::log of
// Thirdparty/g2o/g2o/types/se3quat.h:229-266.  A cuboid is 10 doubles: [t, qx qy qz qw, half scale].
HD void se3_log(const SE3 &T, double *res) {
    double R[3][3]; qtoR(T.r, R);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    double om[3], coef;
    if (d > 0.99999) { for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i]; coef = 1. / 12.; }
    else {
        const double theta = acos(d);
        for (int i = 0; i < 3; i++) om[i] = theta / (2 * sqrt(1 - d * d)) * dR[i];
        coef = (1 - theta / (2 * tan(theta / 2))) / (theta * theta);
    }
    const double O[3][3] = {{0, -om[2], om[1]}, {om[2], 0, -om[0]}, {-om[1], om[0], 0}};
    double O2[3][3];
    mat3mul(O, O, O2);
    for (int i = 0; i < 3; i++) {
        double v[3];
        for (int j = 0; j < 3; j++) v[j] = ((i == j ? 1.0 : 0.0) - 0.5 * O[i][j]) + coef * O2[i][j];
        res[i] = om[i];
        res[i + 3] = (v[0] * T.t[0] + v[1] * T.t[1]) + v[2] * T.t[2];
    }
}
struct Cub9 { SE3 pose; double scale[3]; };
HD Cub9 cub9_load(const double *v) { Cub9 c; c.pose = se3_load(v); c.scale[0] = v[7]; c.scale[1] = v[8]; c.scale[2] = v[9]; return c; }
HD void cub9_store(const Cub9 &c, double *v) { se3_store(c.pose, v); v[7] = c.scale[0]; v[8] = c.scale[1]; v[9] = c.scale[2]; }
HD Cub9 cub9_oplus(Cub9 c, const double *upd) { // VertexCuboid::oplusImpl -> cuboid::exp_update
    Cub9 r;
    normalize_rotation(c.pose);
    r.pose = se3_mul(c.pose, se3_exp(upd));
    for (int k = 0; k < 3; k++) r.scale[k] = c.scale[k] + upd[6 + k];
    return r;
}
HD void cub9_edge_error(const SE3 &Tcw, Cub9 g, Cub9 m, double *err) { // EdgeSE3Cuboid::computeError
    const double PI_ = 3.14159265358979323846;
    normalize_rotation(g.pose); normalize_rotation(m.pose);
    Cub9 e;
    e.pose = se3_mul(se3_inv(Tcw), m.pose); // transform_from
    double best = 0; int lbl = -1;
    for (int i = 0; i < 4; i++) { // min_log_error over rotate_cuboid(-90, 0, 90, 180 degrees)
        const double yaw_angle = (double)(i - 1) * PI_ / 2.0;
        SE3 rot; rot.r = Quat{0, 0, sin(yaw_angle * 0.5), cos(yaw_angle * 0.5)}; rot.t[0] = rot.t[1] = rot.t[2] = 0;
        normalize_rotation(rot);
        Cub9 rc; rc.pose = se3_mul(e.pose, rot);
        const bool swp = (yaw_angle == PI_ / 2.0) || (yaw_angle == -PI_ / 2.0) || (yaw_angle == 3 * PI_ / 2.0);
        rc.scale[0] = swp ? m.scale[1] : m.scale[0]; rc.scale[1] = swp ? m.scale[0] : m.scale[1]; rc.scale[2] = m.scale[2];
        double ei[9];
        se3_log(se3_mul(se3_inv(rc.pose), g.pose), ei); // cube_log_error
        for (int k = 0; k < 3; k++) ei[6 + k] = g.scale[k] - rc.scale[k];
        double nn = 0; for (int k = 0; k < 9; k++) nn += ei[k] * ei[k];
        nn = sqrt(nn);
        if (lbl < 0 || nn < best) { best = nn; lbl = i; for (int k = 0; k < 9; k++) err[k] = ei[k]; }
    }
}
__global__ void __launch_bounds__(64) cub9_oplus_kernel(int n, const double *cub, const double *upd, double *out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    cub9_store(cub9_oplus(cub9_load(cub + (long)i * 10), upd + (long)i * 9), out + (long)i * 10);
}
// thread per (edge, column): column 0 = the error itself, 1..6 camera dofs, 7..15 cuboid dofs (central differences, delta 1e-9)
__global__ void __launch_bounds__(64) cub9_edge_kernel(int n, int with_jac, const double *cam_Tcw, const double *cub_global, const double *cub_meas, double *err, double *Jcam,
                                                       double *Jcub) {
    const int ncol = with_jac ? 16 : 1;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n * ncol) return;
    const int i = t / ncol, col = t % ncol;
    SE3 T = se3_load(cam_Tcw + (long)i * 7);
    normalize_rotation(T);
    const Cub9 G = cub9_load(cub_global + (long)i * 10), M = cub9_load(cub_meas + (long)i * 10);
    if (col == 0) { cub9_edge_error(T, G, M, err + (long)i * 9); return; }
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    double e1[9], e2[9];
    if (col <= 6) {
        double add[6] = {0, 0, 0, 0, 0, 0};
        add[col - 1] = delta; cub9_edge_error(se3_mul(se3_exp(add), T), G, M, e1);
        add[col - 1] = -delta; cub9_edge_error(se3_mul(se3_exp(add), T), G, M, e2);
        for (int k = 0; k < 9; k++) Jcam[(long)i * 54 + k * 6 + (col - 1)] = scalar * (e1[k] - e2[k]);
    } else {
        double add[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        add[col - 7] = delta; cub9_edge_error(T, cub9_oplus(G, add), M, e1);
        add[col - 7] = -delta; cub9_edge_error(T, cub9_oplus(G, add), M, e2);
        for (int k = 0; k < 9; k++) Jcub[(long)i * 81 + k * 9 + (col - 7)] = scalar * (e1[k] - e2[k]);
    }
}

struct cs_ba {
    Params G{};
    int rank = 0, world = 1, n_slots = 0, max_col = 0, max_part = 0;
    cs_allreduce_fn allreduce = nullptr; void *ar_user = nullptr;
    const volatile unsigned char *stop8 = nullptr; // the caller's bool (setForceStopFlag)
    cs_owner own;
    int *d_pose_off = nullptr, *d_pose_obs = nullptr, *d_pe_off = nullptr, *d_pe_list = nullptr, *d_slot_off = nullptr, *d_slot_perm = nullptr, *d_slot_dst = nullptr, *d_col_off = nullptr,
        *d_rows = nullptr, *d_pair_off = nullptr, *d_upd_tgt = nullptr, *d_pos = nullptr, *d_status = nullptr;
    int2 *d_trips = nullptr; uint8_t *d_slot_tr = nullptr;
    double *d_reduce = nullptr, *d_band = nullptr, *d_xperm = nullptr, *d_partials = nullptr, *d_scal = nullptr;
    double *d_bak_cam = nullptr, *d_bak_pts = nullptr, *d_bak_cub = nullptr;
    long reduce_len = 0, band_len = 0; // band_len: doubles of the factor storage
    // band path (see ba_band_chol): cuboids eliminated first, cameras block-banded with half-width band_bc
    bool use_band = false, band_twist = false, band_cr = false; int band_C = 0, band_Q = 0, band_bc = 0, band_targets = 0;
    BaCr *cr = nullptr; // nested-dissection solver of the band system (ba_cr.hip)
    int *d_tgt_slot = nullptr, *d_ct_off = nullptr, *d_ct_list = nullptr, *d_cr_off = nullptr, *d_cr_list = nullptr, *d_cq_off = nullptr, *d_cq_list = nullptr;
    uint8_t *d_tgt_tr = nullptr;
    double *d_bandA = nullptr, *d_bandL = nullptr, *d_cubD = nullptr, *d_cubg = nullptr, *d_brhs = nullptr, *d_ybuf = nullptr, *d_mid = nullptr, *d_xmid = nullptr, *d_bw = nullptr;
    std::vector<std::pair<int, int>> slot_rc; // block (rows, cols) of every slot in pose numbering, (-1, -1): dead (cs_ba_reduced_dense)
    std::vector<int> obs_perm; // sorted-by-landmark position -> caller's observation index
    std::vector<double> h_partials;
    double *h_pin = nullptr; size_t pin_cap = 0; hipEvent_t ev_trial = nullptr; // pinned [status | partials] of a trial and the event behind their copies (cs_ba_optimize)
};

namespace {
static int sum_partials(cs_ctx *ctx, cs_ba *b, int n, double *out, bool is_max = false) { // sum (or maximum) of the first n partials, in index order
    b->h_partials.resize((size_t)std::max(n, 1));
    CS_TRY(cs_d2h(ctx, b->h_partials.data(), b->d_partials, (size_t)n));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double s = 0;
    for (int i = 0; i < n; i++) s = is_max ? std::max(s, b->h_partials[i]) : s + b->h_partials[i];
    *out = s;
    return CS_OK;
}
// all-reduce(sum) of n doubles in device memory across the ranks: the caller's callback when one is registered (it may use another stream or
// library, so the context's stream is drained first), else RCCL on the context's own stream (cs_comm_init), which needs no host round trip
static int ba_allreduce(cs_ctx *ctx, cs_ba *b, double *dbuf, long n) {
    if (b->world <= 1) return CS_OK;
    if (b->allreduce) {
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (b->allreduce(b->ar_user, dbuf, n) != 0) { ctx->err = "all-reduce callback failed"; return CS_ERR_HIP; }
        return CS_OK;
    }
    return cs_comm_allreduce_sum_f64(ctx, dbuf, n);
}
// sum of k host scalars across ranks (k <= the size of d_scal: 6 P + world + 64)
static int allreduce_scalars(cs_ctx *ctx, cs_ba *b, double *v, int k) {
    if (b->world <= 1) return CS_OK;
    CS_TRY(cs_h2d(ctx, b->d_scal, v, (size_t)k));
    CS_TRY(ba_allreduce(ctx, b, b->d_scal, k));
    CS_TRY(cs_d2h(ctx, v, b->d_scal, (size_t)k));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}
static int ba_compute_errors(cs_ctx *ctx, cs_ba *b, double *chi2) { // computeActiveErrors + activeRobustChi2
    const Params &G = b->G;
    double chi = 0, part;
    const int nb1 = (G.o_e - G.o_b + 255) / 256;
    if (nb1 > 0) { CS_LAUNCH(ctx, "ba_err_obs", ba_err_obs, dim3(nb1), dim3(256), 0, G, b->d_partials); CS_TRY(sum_partials(ctx, b, nb1, &part)); chi += part; }
    if (G.pose_edges && G.n_cobs + G.n_pc > 0) {
        const int nb2 = (G.n_cobs + G.n_pc + 255) / 256;
        CS_LAUNCH(ctx, "ba_err_pose_edges", ba_err_pose_edges, dim3(nb2), dim3(256), 0, G, b->d_partials);
        CS_TRY(sum_partials(ctx, b, nb2, &part)); chi += part;
    }
    CS_TRY(allreduce_scalars(ctx, b, &chi, 1));
    *chi2 = chi;
    return CS_OK;
}
static int ba_build_system(cs_ctx *ctx, cs_ba *b) { // BlockSolver::buildSystem
    const Params &G = b->G;
    const int nl = G.lm_e - G.lm_b;
    const bool edges = G.pose_edges && G.n_cobs + G.n_pc > 0;
    const int n_pose = G.P, n_cols = edges ? (2 * (G.n_cobs * 12 + G.n_pc * 6) + 255) / 256 : 0, n_lm = (nl + 255) / 256;
    if (n_pose + n_cols + n_lm > 0) CS_LAUNCH(ctx, "ba_build_abc", ba_build_abc, dim3(n_pose + n_cols + n_lm), dim3(256), 0, G, b->d_pose_off, b->d_pose_obs, n_pose, n_cols);
    if (edges) CS_LAUNCH(ctx, "ba_lin_pose_edges", ba_lin_pose_edges, dim3((G.P + G.n_cobs + 3) / 4), dim3(256), 0, G, b->d_pe_off, b->d_pe_list); // a wave per pose block / per camera-cuboid edge: adds to what ba_lin_pose left
    return CS_OK;
}
static int ba_schur(cs_ctx *ctx, cs_ba *b, double lambda) { // Schur part of BlockSolver::solve, result in d_reduce = [slots | bschur]
    const Params &G = b->G;
    const int nl = G.lm_e - G.lm_b;
    if (nl > 0) CS_LAUNCH(ctx, "ba_lm_dinv", ba_lm_dinv, dim3((nl + 255) / 256), dim3(256), 0, G, lambda);
    if (G.o_e > G.o_b) CS_LAUNCH(ctx, "ba_schur_bd", ba_schur_bd, dim3((int)(((long)(G.o_e - G.o_b) * 6 + 255) / 256)), dim3(256), 0, G, b->d_bw);
    CS_LAUNCH(ctx, "ba_schur_slots", ba_schur_slots, dim3((b->n_slots + 3) / 4), dim3(256), 0, G, b->n_slots, b->d_slot_perm, b->d_slot_off, b->d_trips, lambda, b->d_reduce);
    CS_LAUNCH(ctx, "ba_schur_b", ba_schur_b, dim3(G.P), dim3(256), 0, G, b->d_pose_off, b->d_pose_obs, b->d_bw, b->d_reduce + (long)b->n_slots * 36);
    return CS_OK;
}
static int ba_solve(cs_ctx *ctx, cs_ba *b, double lambda, bool *ok, bool defer_status = false) { // BlockSolver::solve; defer_status: the caller reads d_status later
    const Params &G = b->G;
    CS_TRY(ba_schur(ctx, b, lambda));
    if (b->world > 1) { // one fused buffer [36 * slots | 6 * P] per LM trial
        ctx->begin("ba_allreduce");
        const int rc = ba_allreduce(ctx, b, b->d_reduce, b->reduce_len);
        ctx->end();
        if (rc != CS_OK) return rc;
    }
    const int nl = G.lm_e - G.lm_b;
    if (b->use_band) {
        const int C = b->band_C, Q = b->band_Q, Bc = b->band_bc;
        const double *S = b->d_reduce, *bs = b->d_reduce + (long)b->n_slots * 36;
        CS_HIP(ctx, hipMemsetAsync(b->d_status, 0, sizeof(int), ctx->stream));
        if (Q > 0) CS_LAUNCH(ctx, "ba_cub_inv", ba_cub_inv, dim3((Q + 63) / 64), dim3(64), 0, C, Q, S, bs, b->d_cubD, b->d_cubg, b->d_status);
        { const int nb_a = (b->band_targets * 36 + 255) / 256, nb_r = (C * 6 + 255) / 256;
          CS_LAUNCH(ctx, "ba_band_assemble", ba_band_both, dim3(nb_a + nb_r), dim3(256), 0, nb_a, b->band_targets, b->d_tgt_slot, b->d_tgt_tr, b->d_ct_off, b->d_ct_list, S, b->d_cubD, b->d_bandA,
                    C, b->d_cr_off, b->d_cr_list, bs, b->d_cubg, b->d_brhs); }
        const size_t lds = band_lds_bytes(Bc);
        if (b->band_cr) { // nested dissection over super-blocks of Bc cameras: log2(C / Bc) parallel levels (ba_cr.hip)
            CS_TRY(ba_cr_solve(ctx, &b->cr, C, Bc, b->d_bandA, b->d_brhs, G.x, b->d_status));
        } else if (b->band_twist) { // both ends at once (see the comment above band_factor)
            const size_t lds_mid = sizeof(double) * ((size_t)36 * Bc * Bc + 6 * (size_t)Bc);
            if (lds > 64 * 1024) {
                CS_HIP(ctx, hipFuncSetAttribute((const void *)ba_band_twist_factor, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                CS_HIP(ctx, hipFuncSetAttribute((const void *)ba_band_twist_back, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            }
            if (lds_mid > 64 * 1024) CS_HIP(ctx, hipFuncSetAttribute((const void *)ba_band_mid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_mid));
            CS_LAUNCH(ctx, "ba_band_twist_factor", ba_band_twist_factor, dim3(2), dim3(BAND_NT), lds, C, Bc, b->d_bandA, b->d_brhs, b->d_bandL, b->d_ybuf, b->d_mid, b->d_status);
            CS_LAUNCH(ctx, "ba_band_mid", ba_band_mid, dim3(1), dim3(256), lds_mid, C, Bc, b->d_mid, b->d_xmid, G.x, b->d_status);
            CS_LAUNCH(ctx, "ba_band_twist_back", ba_band_twist_back, dim3(2), dim3(BAND_NT), lds, C, Bc, b->d_bandL, b->d_ybuf, b->d_xmid, G.x);
        } else {
            if (lds > 64 * 1024) CS_HIP(ctx, hipFuncSetAttribute((const void *)ba_band_chol, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            CS_LAUNCH(ctx, "ba_band_chol", ba_band_chol, dim3(1), dim3(BAND_NT), lds, C, Bc, b->d_bandA, b->d_bandL, b->d_brhs, b->d_ybuf, b->d_status);
        }
        if (!b->band_twist && !b->band_cr) CS_HIP(ctx, hipMemcpyAsync(G.x, b->d_brhs, sizeof(double) * (size_t)C * 6, hipMemcpyDeviceToDevice, ctx->stream));
        if (nl > 0 || Q > 0) CS_LAUNCH(ctx, "ba_backsub", ba_back_both, dim3((nl + 255) / 256 + (Q + 255) / 256), dim3(256), 0, G, (nl + 255) / 256, C, Q, b->d_cq_off, b->d_cq_list, S, b->d_cubD, b->d_cubg);
        if (defer_status) return CS_OK;
        int status = 0;
        CS_TRY(cs_d2h(ctx, &status, b->d_status, 1));
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *ok = status == 0;
        return CS_OK;
    }
    CS_HIP(ctx, hipMemsetAsync(b->d_band, 0, sizeof(double) * (size_t)b->band_len, ctx->stream));
    CS_LAUNCH(ctx, "ba_chol_fill", ba_chol_fill, dim3((b->n_slots * 36 + 255) / 256), dim3(256), 0, b->n_slots, b->d_slot_dst, b->d_slot_tr, b->d_reduce, b->d_band);
    CS_LAUNCH(ctx, "ba_chol_factor", ba_chol_factor, dim3(1), dim3(512), sizeof(double) * (36 + (size_t)std::max(b->max_col, 1) * 36), G.P, b->d_col_off, b->d_pair_off,
              b->d_upd_tgt, b->d_band, b->d_status);
    CS_LAUNCH(ctx, "ba_permute", ba_permute, dim3((G.P * 6 + 255) / 256), dim3(256), 0, G.P, b->d_pos, b->d_reduce + (long)b->n_slots * 36, b->d_xperm, 1);
    CS_LAUNCH(ctx, "ba_chol_solve", ba_chol_solve, dim3(1), dim3(256), 0, G.P, b->d_col_off, b->d_rows, b->d_band, b->d_xperm);
    CS_LAUNCH(ctx, "ba_permute", ba_permute, dim3((G.P * 6 + 255) / 256), dim3(256), 0, G.P, b->d_pos, b->d_xperm, G.x, 0);
    if (nl > 0) CS_LAUNCH(ctx, "ba_backsub", ba_backsub, dim3((nl + 255) / 256), dim3(256), 0, G);
    if (defer_status) return CS_OK;
    int status = 0;
    CS_TRY(cs_d2h(ctx, &status, b->d_status, 1));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *ok = status == 0;
    return CS_OK;
}
} // namespace

extern "C" {

void cs_ba_destroy(cs_ctx *ctx, cs_ba *b) {
    if (!b) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    b->own.free_all(ctx);
    if (b->h_pin) hipHostFree(b->h_pin);
    if (b->ev_trial) hipEventDestroy(b->ev_trial);
    ba_cr_destroy(b->cr);
    delete b;
}
int cs_ba_set_allreduce(cs_ba *b, cs_allreduce_fn fn, void *user) {
    if (!b) return CS_ERR_BAD_ARG;
    b->allreduce = fn; b->ar_user = user;
    return CS_OK;
}

// check -> plan (ba_plan.h, host only) -> upload.  Nothing is allocated before the plan stands; after `new cs_ba` every failure leaves through cs_ba_destroy.
int cs_ba_create(cs_ctx *ctx, const cs_ba_problem *p, int rank, int world, cs_ba **out) {
    if (!ctx || !out) return CS_ERR_BAD_ARG;
    *out = nullptr;
    CS_TRY(ba_plan_check(p, rank, world));
    const char *force = getenv("CUBESLAM_BA_SOLVER"); // "sparse" / "band" / "band1" (band, one workgroup) / "cr": pick the path (tests run all)
    const BaSolverChoice choice = !force ? BA_SOLVER_NONE : !strcmp(force, "sparse") ? BA_SOLVER_SPARSE : !strcmp(force, "band") ? BA_SOLVER_BAND : !strcmp(force, "band1") ? BA_SOLVER_BAND1 :
                                  !strcmp(force, "cr") ? BA_SOLVER_CR : BA_SOLVER_OTHER;
    BaPlan X;
    const char *why = nullptr;
    const int rp = ba_plan_build(p, rank, world, choice, X, &why);
    if (rp != CS_OK) { if (why) ctx->err = why; return rp; }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_ba *b = new (std::nothrow) cs_ba();
    if (!b) return CS_ERR_NOMEM;
    b->rank = rank; b->world = world;
    Params &G = b->G;
    G.n_cams = p->n_cams; G.L = p->n_points; G.n_cub = p->n_cuboids; G.n_obs = p->n_obs; G.n_cobs = p->n_cobs; G.n_pc = p->n_pc;
    G.fx = p->fx; G.fy = p->fy; G.cx = p->cx; G.cy = p->cy; G.huber_mono = p->huber_mono; G.huber_obj = p->huber_obj; G.bf = p->bf; G.huber_stereo = p->huber_stereo; G.margin_ratio = p->max_outside_margin_ratio;
    for (int i = 0; i < 9; i++) G.K[i] = p->K[i];
    G.pose_edges = X.pose_edges;
    const int P = G.P = X.P;
    G.lm_b = X.lm_b; G.lm_e = X.lm_e; G.o_b = X.o_b; G.o_e = X.o_e;
    b->n_slots = X.n_slots; b->max_col = X.max_col; b->max_part = X.max_part; b->band_len = X.band_len; b->reduce_len = X.reduce_len;
    b->use_band = X.use_band; b->band_twist = X.band_twist; b->band_C = X.C; b->band_Q = X.Q; b->band_bc = X.band_bc; b->band_targets = X.band_targets;
    // nested dissection (ba_cr.hip) once there are enough super-blocks to split; CUBESLAM_BA_SOLVER=band keeps the two-sided chain, =cr forces this
    b->band_cr = X.use_band && ba_cr_supported(X.C, X.band_bc) && (choice == BA_SOLVER_CR || (choice == BA_SOLVER_NONE && X.C >= 16 * X.band_bc));
    b->slot_rc.swap(X.slot_rc); b->obs_perm.swap(X.obs_perm); // neither is uploaded
    // estimates enter through SE3Quat(Vector7d): normalizeRotation (se3quat.h:64-67) -- done on a host copy, which is what goes up
    std::vector<double> cam(p->cam_pose, p->cam_pose + (size_t)p->n_cams * 7), cub;
    if (p->n_cuboids) cub.assign(p->cuboid_pose, p->cuboid_pose + (size_t)p->n_cuboids * 7);
    for (std::vector<double> *v : {&cam, &cub}) for (size_t i = 0; i + 7 <= v->size(); i += 7) { SE3 T = se3_load(v->data() + i); normalize_rotation(T); se3_store(T, v->data() + i); }
    // Uploads: the first failure stands and the rest become no-ops.  up / upv copy exactly the elements that exist (cs_h2d skips an empty copy), work blocks
    // are not initialised; cs_dalloc alone turns an empty block into one element.
    int r = CS_OK;
    auto up = [&](auto *&d, const auto *h, size_t n) { // a caller's array
        using T = std::remove_const_t<std::remove_pointer_t<std::remove_reference_t<decltype(d)>>>;
        T *q = nullptr;
        if (r == CS_OK) r = b->own.upload(ctx, &q, reinterpret_cast<const T *>(h), n);
        d = q;
    };
    auto upv = [&](auto *&d, const auto &h) { static_assert(sizeof(*d) == sizeof(h[0]), "same layout on both sides"); up(d, h.data(), h.size()); }; // a plan array
    auto work = [&](auto *&d, size_t n) { if (r == CS_OK) r = b->own.alloc(ctx, &d, n); };                                                              // a work block
    auto n1 = [](long n) { return (size_t)std::max(n, 1L); };
    const size_t n_obs = p->n_obs, n_cobs = p->n_cobs, n_pc = p->n_pc, n_pts = p->n_points, n_cub = p->n_cuboids, n_pcp = p->n_pc ? p->pc_offsets[p->n_pc] : 0;
    upv(G.cam, cam); up(G.pts, p->points, n_pts * 3); upv(G.cub, cub); up(G.cub_scale, p->cuboid_scale, n_cub * 3); up(G.cub_flags, p->cuboid_flags, n_cub);
    upv(G.cam_idx, X.cam_idx); upv(G.o_cam, X.o_cam); upv(G.o_pt, X.o_pt); upv(G.o_uv, X.o_uv); upv(G.o_w, X.o_w); upv(G.lm_off, X.lm_off);
    if (!X.o_ur.empty()) upv(G.o_ur, X.o_ur); // (no array: monocular)
    up(G.c_cam, p->cobs_cam, n_cobs); up(G.c_cub, p->cobs_cuboid, n_cobs); up(G.c_bbox, p->cobs_bbox, n_cobs * 4); up(G.c_info, p->cobs_info, n_cobs * 4);
    up(G.pc_cub, p->pc_cuboid, n_pc); up(G.pc_off, p->pc_offsets, n_pc ? n_pc + 1 : 0); up(G.pc_pts, p->pc_points, n_pcp * 3);
    work(G.e_obs, n1(n_obs) * 3); work(G.e_cobs, n1(n_cobs) * 4); work(G.e_pc, n1(n_pc) * 3); work(G.Hpl, n1(n_obs) * 18); work(G.HplD, n1(n_obs) * 18); work(b->d_bw, n1(n_obs) * 6);
    work(G.Hll, n1(n_pts) * 9); work(G.bl, n1(n_pts) * 3); work(G.Dinv, n1(n_pts) * 9); work(G.db, n1(n_pts) * 3); work(G.Hpp, (size_t)P * 36); work(G.bp, (size_t)P * 6);
    work(G.Hoff, n1(n_cobs) * 36); work(G.Jc, n1(n_cobs) * 48); work(G.Jp, n1(n_pc) * 18); work(G.x, (size_t)P * 6 + n1(n_pts) * 3);
    upv(b->d_pose_off, X.pose_off); upv(b->d_pose_obs, X.pose_obs); upv(b->d_pe_off, X.pe_off); upv(b->d_pe_list, X.pe_list);
    upv(b->d_slot_off, X.slot_off); upv(b->d_slot_perm, X.slot_perm); upv(b->d_trips, X.trips); upv(b->d_slot_dst, X.slot_dst); upv(b->d_slot_tr, X.slot_tr);
    upv(b->d_col_off, X.col_off); upv(b->d_rows, X.rows); upv(b->d_pair_off, X.pair_off); upv(b->d_upd_tgt, X.upd_tgt); upv(b->d_pos, X.pos); work(b->d_status, 1);
    if (X.use_band) {
        const size_t nt = (size_t)X.band_targets, Bc = (size_t)X.band_bc;
        upv(b->d_tgt_slot, X.tgt_slot); upv(b->d_tgt_tr, X.tgt_tr); upv(b->d_ct_off, X.ct_off); upv(b->d_ct_list, X.ct_list);
        upv(b->d_cr_off, X.cr_off); upv(b->d_cr_list, X.cr_list); upv(b->d_cq_off, X.cq_off); upv(b->d_cq_list, X.cq_list);
        work(b->d_bandA, nt * 36); work(b->d_bandL, nt * 36); work(b->d_cubD, n1(X.Q) * 36); work(b->d_cubg, n1(X.Q) * 6); work(b->d_brhs, (size_t)X.C * 6);
        work(b->d_ybuf, (size_t)X.C * BAND_YB); work(b->d_mid, 2 * (Bc * (Bc + 1) * 36 + Bc * 6) + 8); work(b->d_xmid, Bc * 6 + 8);
    }
    work(b->d_reduce, (size_t)b->reduce_len); work(b->d_band, (size_t)b->band_len); work(b->d_xperm, (size_t)P * 6);
    work(b->d_partials, (size_t)b->max_part * 3); // three regions: scale | chi2 of the observations | chi2 of the pose edges
    work(b->d_scal, (size_t)P * 6 + (size_t)world + 64);
    work(b->d_bak_cam, (size_t)p->n_cams * 7); work(b->d_bak_pts, n1(n_pts) * 3); work(b->d_bak_cub, n1(n_cub) * 7);
    if (r == CS_OK) { const hipError_t e = hipStreamSynchronize(ctx->stream); if (e != hipSuccess) { ctx->err = hipGetErrorString(e); r = CS_ERR_HIP; } } // the one wait: the copies read X, cam and cub
    if (r != CS_OK) { cs_ba_destroy(ctx, b); return r; }
    *out = b;
    return CS_OK;
}

int cs_ba_errors(cs_ctx *ctx, cs_ba *b, double *chi2, double *err_obs, double *err_cobs, double *err_pc) {
    if (!ctx || !b || !chi2) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    CS_TRY(ba_compute_errors(ctx, b, chi2));
    const Params &G = b->G;
    if (err_obs) { // back to the caller's observation order
        std::vector<double> e((size_t)std::max(G.n_obs, 1) * 3);
        CS_TRY(cs_d2h(ctx, e.data(), G.e_obs, (size_t)G.n_obs * 3));
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int q = G.o_b; q < G.o_e; q++) for (int k = 0; k < 3; k++) err_obs[(size_t)b->obs_perm[q] * 3 + k] = e[(size_t)q * 3 + k];
    }
    if (err_cobs && G.pose_edges) CS_TRY(cs_d2h(ctx, err_cobs, G.e_cobs, (size_t)G.n_cobs * 4));
    if (err_pc && G.pose_edges) CS_TRY(cs_d2h(ctx, err_pc, G.e_pc, (size_t)G.n_pc * 3));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_ba_reduced_dense(cs_ctx *ctx, cs_ba *b, double lambda, double *H, double *bvec, int *Pout) {
    if (!ctx || !b || !H || !bvec || !Pout) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    double chi;
    CS_TRY(ba_compute_errors(ctx, b, &chi));
    CS_TRY(ba_build_system(ctx, b));
    CS_TRY(ba_schur(ctx, b, lambda));
    std::vector<double> red((size_t)b->reduce_len);
    CS_TRY(cs_d2h(ctx, red.data(), b->d_reduce, red.size()));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int P = b->G.P, n = P * 6;
    std::fill(H, H + (size_t)n * n, 0.0);
    for (int s = 0; s < b->n_slots; s++) {
        const int i = b->slot_rc[s].first, j = b->slot_rc[s].second; // the slot holds block (rows i, cols j) in pose numbering
        if (i < 0) continue; // dead block
        for (int a = 0; a < 6; a++) for (int c = 0; c < 6; c++) {
            const double v = red[(size_t)s * 36 + a * 6 + c];
            H[(size_t)(i * 6 + a) * n + j * 6 + c] += v;
            if (i != j) H[(size_t)(j * 6 + c) * n + i * 6 + a] += v;
        }
    }
    for (int i = 0; i < n; i++) bvec[i] = red[(size_t)b->n_slots * 36 + i];
    *Pout = P;
    return CS_OK;
}

int cs_ba_read(cs_ctx *ctx, cs_ba *b, double *cam_pose, double *points, double *cuboid_pose) {
    if (!ctx || !b) return CS_ERR_BAD_ARG;
    const Params &G = b->G;
    if (cam_pose) CS_TRY(cs_d2h(ctx, cam_pose, G.cam, (size_t)G.n_cams * 7));
    if (points) CS_TRY(cs_d2h(ctx, points + (size_t)G.lm_b * 3, G.pts + (size_t)G.lm_b * 3, (size_t)(G.lm_e - G.lm_b) * 3));
    if (cuboid_pose) CS_TRY(cs_d2h(ctx, cuboid_pose, G.cub, (size_t)G.n_cub * 7));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_ba_set_stop_flag_bool(cs_ba *b, const volatile unsigned char *flag) { if (!b) return CS_ERR_BAD_ARG; b->stop8 = flag; return CS_OK; }

int cs_ba_optimize(cs_ctx *ctx, cs_ba *b, int iterations, const volatile int *stop_flag, cs_ba_stats *st) {
    if (!ctx || !b || iterations < 0) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    if (b->world > 1 && !b->allreduce && !(ctx->comm && ctx->comm_world == b->world)) { ctx->err = "sharded BA needs cs_comm_init (RCCL) or cs_ba_set_allreduce"; return CS_ERR_BAD_ARG; }
    const Params &G = b->G;
    cs_ba_stats S;
    memset(&S, 0, sizeof(S));
    double currentChi = 0;
    LmSchedule lm;
    const int nl = G.lm_e - G.lm_b;
    auto terminate = [&]() { return (stop_flag && *stop_flag) || (b->stop8 && *b->stop8); }; // sparse_optimizer.cpp:376, optimization_algorithm_levenberg.cpp:149
    // A trial is accepted nearly always, and the next iteration then starts by linearising at the state the trial left.  So that system is BUILT AHEAD: enqueued behind the
    // trial's residual kernels before the host waits for their sums, and the GPU goes from one iteration into the next without the round trip (copy back, decision, launch)
    // in between.  A rejected trial restores the estimates and rebuilds what the build-ahead overwrote -- residuals, then the system -- from the restored state: the same
    // kernels on the same bits, so the retried solve sees the system it would have kept (CUBESLAM_BA_AHEAD=0: the plain order).
    const bool ahead_on = b->world == 1 && !(getenv("CUBESLAM_BA_AHEAD") && atoi(getenv("CUBESLAM_BA_AHEAD")) == 0);
    bool built_ahead = false;
    for (int it = 0; it < iterations && !terminate(); it++) { // OptimizationAlgorithmLevenberg::solve :61-164
        // computeActiveErrors: after an accepted trial the residual arrays and chi2 on the device are those of the current state (every
        // way out of the trial loop with a rejected last trial also leaves this loop), so only the first iteration evaluates them
        double tempChi;
        if (it == 0) CS_TRY(ba_compute_errors(ctx, b, &currentChi));
        tempChi = currentChi;
        const double iniChi = currentChi;
        if (it == 0) S.chi2_init = currentChi;
        if (!built_ahead) CS_TRY(ba_build_system(ctx, b));
        built_ahead = false;
        if (it == 0) { // computeLambdaInit :166-180: tau * max |diag(H)| over all active vertices
            std::vector<double> v((size_t)G.P * 6 + (size_t)b->world, 0.0), hpp((size_t)G.P * 36);
            CS_TRY(cs_d2h(ctx, hpp.data(), G.Hpp, hpp.size()));
            double mxl = 0;
            if (nl > 0) { CS_LAUNCH(ctx, "ba_maxdiag", ba_maxdiag, dim3((nl + 255) / 256), dim3(256), 0, G, b->d_partials); CS_TRY(sum_partials(ctx, b, (nl + 255) / 256, &mxl, true)); }
            CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
            double mx = mxl;
            if (b->world > 1) { // pose diagonals are sums over ranks; landmark maxima travel in per-rank slots of the same sum
                std::vector<double> buf((size_t)G.P * 6 + b->world, 0.0);
                for (int i = 0; i < G.P; i++) for (int k = 0; k < 6; k++) buf[(size_t)i * 6 + k] = hpp[(size_t)i * 36 + k * 7];
                buf[(size_t)G.P * 6 + b->rank] = mxl;
                CS_TRY(allreduce_scalars(ctx, b, buf.data(), (int)buf.size())); // one collective (it was one per 64 scalars)
                mx = 0;
                for (double d : buf) mx = std::max(mx, std::fabs(d));
            } else
                for (int i = 0; i < G.P; i++) for (int k = 0; k < 6; k++) mx = std::max(mx, std::fabs(hpp[(size_t)i * 36 + k * 7]));
            lm.start(1e-5 * mx);
        }
        lm.begin_iteration();
        do {
            // push(): back up the estimates
            CS_HIP(ctx, hipMemcpyAsync(b->d_bak_cam, G.cam, sizeof(double) * (size_t)G.n_cams * 7, hipMemcpyDeviceToDevice, ctx->stream));
            if (G.L) CS_HIP(ctx, hipMemcpyAsync(b->d_bak_pts, G.pts, sizeof(double) * (size_t)G.L * 3, hipMemcpyDeviceToDevice, ctx->stream));
            if (G.n_cub) CS_HIP(ctx, hipMemcpyAsync(b->d_bak_cub, G.cub, sizeof(double) * (size_t)G.n_cub * 7, hipMemcpyDeviceToDevice, ctx->stream));
            bool ok2 = true;
            const int nbs = (int)(((long)G.P * 6 + (long)nl * 3 + 255) / 256);
            double scale;
            if (b->world == 1) { // one host round trip per trial: solve, scale, update and the new residuals are enqueued back to back
                CS_TRY(ba_solve(ctx, b, lm.lambda, &ok2, true));
                const int nb1 = (G.o_e - G.o_b + 255) / 256, nb2 = (G.pose_edges && G.n_cobs + G.n_pc > 0) ? (G.n_cobs + G.n_pc + 255) / 256 : 0, mp = b->max_part;
                CS_LAUNCH(ctx, "ba_update", ba_scale_update, dim3(nbs + (G.n_cams + G.n_cub + nl * 3 + 255) / 256), dim3(256), 0, G, lm.lambda, b->d_partials, nbs);
                if (nb1 > 0) CS_LAUNCH(ctx, "ba_err_obs", ba_err_obs, dim3(nb1), dim3(256), 0, G, b->d_partials + mp);
                if (nb2 > 0) CS_LAUNCH(ctx, "ba_err_pose_edges", ba_err_pose_edges, dim3(nb2), dim3(256), 0, G, b->d_partials + 2 * mp); // (one grid for both measured no faster: 36 us against 14 + 20, the cuboid edges' registers halve the reprojection edges' occupancy)
                const size_t need = (size_t)mp * 3 + 1;
                if (b->pin_cap < need) {
                    if (b->h_pin) hipHostFree(b->h_pin);
                    b->h_pin = nullptr; b->pin_cap = 0;
                    CS_HIP(ctx, hipHostMalloc((void **)&b->h_pin, need * sizeof(double), hipHostMallocDefault));
                    b->pin_cap = need;
                }
                if (!b->ev_trial) CS_HIP(ctx, hipEventCreateWithFlags(&b->ev_trial, hipEventDisableTiming));
                int *h_status = reinterpret_cast<int *>(b->h_pin + (size_t)mp * 3);
                CS_TRY(cs_d2h(ctx, h_status, b->d_status, 1));
                CS_TRY(cs_d2h(ctx, b->h_pin, b->d_partials, (size_t)mp * 3));
                CS_HIP(ctx, hipEventRecord(b->ev_trial, ctx->stream));
                if (ahead_on && it + 1 < iterations) { CS_TRY(ba_build_system(ctx, b)); built_ahead = true; } // (the last iteration has no successor to build for)
                CS_HIP(ctx, hipEventSynchronize(b->ev_trial));
                const int status = *h_status;
                const double *hp = b->h_pin;
                ok2 = status == 0;
                scale = 0;
                for (int i = 0; i < nbs; i++) scale += hp[i];
                double chi = 0, c1 = 0, c2 = 0; // same order of additions as ba_compute_errors
                for (int i = 0; i < nb1; i++) c1 += hp[(size_t)mp + i];
                for (int i = 0; i < nb2; i++) c2 += hp[(size_t)2 * mp + i];
                if (nb1 > 0) chi += c1;
                if (nb2 > 0) chi += c2;
                tempChi = chi;
            } else {
                CS_TRY(ba_solve(ctx, b, lm.lambda, &ok2));
                CS_LAUNCH(ctx, "ba_scale", ba_scale, dim3(nbs), dim3(256), 0, G, lm.lambda, b->d_partials);
                CS_TRY(sum_partials(ctx, b, nbs, &scale));
                CS_TRY(allreduce_scalars(ctx, b, &scale, 1));
                CS_LAUNCH(ctx, "ba_update", ba_update, dim3((G.n_cams + G.n_cub + nl * 3 + 255) / 256), dim3(256), 0, G);
                CS_TRY(ba_compute_errors(ctx, b, &tempChi));
            }
            if (!lm.trial(currentChi, tempChi, ok2, scale)) { // pop(): restore (an accepted trial's state stands: discardTop)
                CS_HIP(ctx, hipMemcpyAsync(G.cam, b->d_bak_cam, sizeof(double) * (size_t)G.n_cams * 7, hipMemcpyDeviceToDevice, ctx->stream));
                if (G.L) CS_HIP(ctx, hipMemcpyAsync(G.pts, b->d_bak_pts, sizeof(double) * (size_t)G.L * 3, hipMemcpyDeviceToDevice, ctx->stream));
                if (G.n_cub) CS_HIP(ctx, hipMemcpyAsync(G.cub, b->d_bak_cub, sizeof(double) * (size_t)G.n_cub * 7, hipMemcpyDeviceToDevice, ctx->stream));
                if (built_ahead) { // the system in the buffers is the rejected state's: residuals and system of the restored one again (the retry solves that)
                    double unused; CS_TRY(ba_compute_errors(ctx, b, &unused));
                    CS_TRY(ba_build_system(ctx, b));
                    built_ahead = false;
                }
            }
            S.lm_trials++;
        } while (lm.retry() && !terminate());
        S.iterations = it + 1;
        if (it < 64) S.chi2_trace[it] = currentChi;
        S.chi2_final = currentChi;
        if (lm.stop(iniChi, currentChi)) break; // :151-161
    }
    S.lambda_final = lm.lambda;
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (st) *st = S;
    return CS_OK;
}

int cs_cuboid9_oplus(cs_ctx *ctx, int n, const double *cub, const double *upd, double *out) {
    if (!ctx || n < 0 || (n && (!cub || !upd || !out))) return CS_ERR_BAD_ARG;
    if (n == 0) return CS_OK;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    double *d_c = nullptr, *d_u = nullptr, *d_o = nullptr;
    CS_TRY(sc.alloc(ctx, &d_c, (size_t)n * 10)); CS_TRY(sc.alloc(ctx, &d_u, (size_t)n * 9)); CS_TRY(sc.alloc(ctx, &d_o, (size_t)n * 10));
    CS_TRY(cs_h2d(ctx, d_c, cub, (size_t)n * 10)); CS_TRY(cs_h2d(ctx, d_u, upd, (size_t)n * 9));
    hipLaunchKernelGGL(cub9_oplus_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, n, d_c, d_u, d_o);
    CS_TRY(cs_d2h(ctx, out, d_o, (size_t)n * 10));
    const hipError_t e = hipStreamSynchronize(ctx->stream); sc.drained = true;
    if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return CS_ERR_HIP; }
    return CS_OK;
}

int cs_cuboid9_edge_linearize(cs_ctx *ctx, int n, const double *cam_Tcw, const double *cub_global, const double *cub_meas_local, double *err, double *Jcam, double *Jcub) {
    if (!ctx || n < 0 || (n && (!cam_Tcw || !cub_global || !cub_meas_local || !err)) || ((Jcam == nullptr) != (Jcub == nullptr))) return CS_ERR_BAD_ARG;
    if (n == 0) return CS_OK;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const int with_jac = Jcam != nullptr;
    double *d_T = nullptr, *d_g = nullptr, *d_m = nullptr, *d_e = nullptr, *d_jc = nullptr, *d_jq = nullptr;
    cs_scratch sc(ctx);
    CS_TRY(sc.alloc(ctx, &d_T, (size_t)n * 7)); CS_TRY(sc.alloc(ctx, &d_g, (size_t)n * 10)); CS_TRY(sc.alloc(ctx, &d_m, (size_t)n * 10)); CS_TRY(sc.alloc(ctx, &d_e, (size_t)n * 9));
    if (with_jac) { CS_TRY(sc.alloc(ctx, &d_jc, (size_t)n * 54)); CS_TRY(sc.alloc(ctx, &d_jq, (size_t)n * 81)); }
    CS_TRY(cs_h2d(ctx, d_T, cam_Tcw, (size_t)n * 7)); CS_TRY(cs_h2d(ctx, d_g, cub_global, (size_t)n * 10)); CS_TRY(cs_h2d(ctx, d_m, cub_meas_local, (size_t)n * 10));
    const int nt = n * (with_jac ? 16 : 1);
    hipLaunchKernelGGL(cub9_edge_kernel, dim3((nt + 63) / 64), dim3(64), 0, ctx->stream, n, with_jac, d_T, d_g, d_m, d_e, d_jc, d_jq);
    CS_TRY(cs_d2h(ctx, err, d_e, (size_t)n * 9));
    if (with_jac) { CS_TRY(cs_d2h(ctx, Jcam, d_jc, (size_t)n * 54)); CS_TRY(cs_d2h(ctx, Jcub, d_jq, (size_t)n * 81)); }
    const hipError_t e = hipStreamSynchronize(ctx->stream); sc.drained = true;
    if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return CS_ERR_HIP; }
    return CS_OK;
}

} // extern "C"
