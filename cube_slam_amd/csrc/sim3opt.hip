// sim3opt.hip -- ORB_SLAM2::Optimizer::OptimizeSim3 on MI355X (gfx950), for a batch of problems.
//
// Replaces Optimizer::OptimizeSim3 (reference orb_object_slam/include/Optimizer.h, src/Optimizer.cc:2838-3033): the 7-dof refinement of the Sim3 between two key frames
// that LoopClosing::ComputeSim3 runs between SearchBySim3 and SearchByProjection(pKF, Scw, ...).  One free VertexSim3Expmap, two unary edges per correspondence (both
// point vertices are fixed), g2o's Levenberg-Marquardt in two stages with an outlier cut between them.  One workgroup of 256 threads runs the whole routine for one
// problem in one launch, as pose_opt_kernel (poseopt.hip) does for a frame.
//
//   * correspondences are strided over the threads; EdgeSim3ProjectXYZ is obs1 - cam_map1(project(S.map(P2c))), EdgeInverseSim3ProjectXYZ is
//     obs2 - cam_map2(project(S.inverse().map(P1c))) (types_seven_dof_expmap.h:130-171), information invSigma2 * I, Huber with delta = (float)sqrt(th2)
//   * neither edge overrides linearizeOplus: the Jacobian is g2o's central difference over the 7 update coordinates, delta = 1e-9, each perturbed estimate being
//     Sim3(update) * estimate (core/base_binary_edge.hpp:269-320, VertexSim3Expmap::oplusImpl).  The 14 perturbed transforms and their inverses do not depend on the
//     edge: 14 threads build them once per linearisation in LDS, every edge then does its 28 maps and projections
//   * under fix_scale oplusImpl zeroes update[6]: column 6 of every Jacobian is exactly zero, H(6,6) is lambda alone and the step's seventh component is dropped.  The
//     system stays 7 x 7
//   * the 28 lower-triangle entries of H (LinearSolverDense's L D L^T reads that triangle), the 7 of b and chi2 are reduced in a fixed order: thread partials in
//     correspondence order (e12 before e21), a shuffle tree, the four wave results (block_reduce, common.h).  Thread 0 solves the damped system; every LM decision
//     (lm_schedule.h) is taken by all threads from the same LDS values
//   * optimize(5); chi2 > th2 on either edge, on the _error the last trial left, removes the pair; fewer than 10 left: return 0 with the Sim3 as it came; otherwise
//     optimize(nBad > 0 ? 10 : 5) from the first stage's estimate and a second cut that only flags
// Every loop is bounded by those constants; no atomics, no waiting on other workgroups.
//
// cs_sim3_optimization_trace (include/cubeslam_hip/sim3_opt_trace.h) is a test probe: the same kernel with trace / n_trials / system0 set, which the product entry passes
// as NULL.  Thread 0 then stores the first system and one record per LM trial behind a workgroup-uniform test; nothing else in the kernel depends on those pointers.
#include "common.h"
#include "lm_schedule.h"
#include "sim3_math.h"
#include "../../include/cubeslam_hip/sim3_opt_trace.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

struct Sim3Problem { int e0, e1, fix_scale; double K[8]; double delta, dsqr, th2; }; // delta, dsqr: RobustKernelHuber's (dsqr is a float member there); th2 promoted from float

constexpr int SIM3_THREADS = 256, SIM3_NSYS = 36; // 28 of H + 7 of b + 1 scalar (chi2 or a count)

// obs - cam_map(project(S.map(p))) (se3_ops.hpp:49-55: a division per coordinate)
__device__ __forceinline__ void sim3_edge_error(const Sim3 &S, const double *p, const double *ob, const double *K, double *e) {
    double q[3];
    sim3_map(S, p, q);
    e[0] = ob[0] - (q[0] / q[2] * K[0] + K[2]);
    e[1] = ob[1] - (q[1] / q[2] * K[1] + K[3]);
}
__device__ __forceinline__ double sim3_edge_chi2(const double *e, double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); } // _error.dot(information() * _error)

__global__ void __launch_bounds__(SIM3_THREADS) sim3_opt_kernel(const Sim3Problem *problems, const double *P1c, const double *P2c, const double *obs1, const double *obs2, const double *w1,
                                                               const double *w2, const double *sim3_in, double *sim3_out, uint8_t *removed, int *n_inliers, double *err /* 4 per correspondence */,
                                                               int max_trials, double *trace, int *n_trials, double *system0 /* the probe's: NULL in the product */) {
    __shared__ double s_red[4 * SIM3_NSYS], s_sys[SIM3_NSYS];
    __shared__ double s_x[7], s_S[8], s_pert[28 * 8]; // s_pert: Sim3(+-delta e_d) * estimate for d = 0 .. 6 (14), then their inverses (14)
    __shared__ int s_flag;
    const Sim3Problem F = problems[blockIdx.x];
    const int n = F.e1 - F.e0, tid = threadIdx.x;
    const double *X1 = P1c + (long)F.e0 * 3, *X2 = P2c + (long)F.e0 * 3, *O1 = obs1 + (long)F.e0 * 2, *O2 = obs2 + (long)F.e0 * 2, *W1 = w1 + F.e0, *W2 = w2 + F.e0;
    double *E = err + (long)F.e0 * 4;
    uint8_t *rem = removed + F.e0;
    const double *in = sim3_in + (long)blockIdx.x * 8;
    double *out = sim3_out + (long)blockIdx.x * 8;
    if (n == 0) { // optimize() has no vertex to work on; nCorrespondences - nBad < 10.  The whole workgroup leaves here, before any barrier
        if (tid < 8) out[tid] = in[tid];
        if (tid == 0) n_inliers[blockIdx.x] = 0;
        if (trace && tid == 0) n_trials[blockIdx.x] = 0;
        if (trace && tid < SIM3_NSYS) system0[(long)blockIdx.x * SIM3_NSYS + tid] = 0;
        return;
    }
    for (int i = tid; i < n; i += SIM3_THREADS) rem[i] = 0;
    Sim3 S = sim3_load(in);
    __syncthreads();
    auto chi2_sum = [&](const Sim3 &Sc) -> double { // computeActiveErrors + activeRobustChi2
        const Sim3 Si = sim3_inverse(Sc);
        double v[1] = {0};
        for (int i = tid; i < n; i += SIM3_THREADS) {
            if (rem[i]) continue;
            double e[4];
            sim3_edge_error(Sc, X2 + (long)i * 3, O1 + (long)i * 2, F.K, e);
            sim3_edge_error(Si, X1 + (long)i * 3, O2 + (long)i * 2, F.K + 4, e + 2);
            E[(long)i * 4] = e[0]; E[(long)i * 4 + 1] = e[1]; E[(long)i * 4 + 2] = e[2]; E[(long)i * 4 + 3] = e[3];
            double c = sim3_edge_chi2(e, W1[i]);
            if (!(c <= F.dsqr)) c = 2 * sqrt(c) * F.delta - F.dsqr;
            v[0] += c;
            c = sim3_edge_chi2(e + 2, W2[i]);
            if (!(c <= F.dsqr)) c = 2 * sqrt(c) * F.delta - F.dsqr;
            v[0] += c;
        }
        block_reduce<1>(v, s_red, s_sys + 35);
        return s_sys[35];
    };
    int nBad = 0, nIn = 0, trials = 0;
    for (int stage = 0; stage < 2; stage++) {
        const int iterations = stage == 0 ? 5 : (nBad > 0 ? 10 : 5);
        LmSchedule lm;
        for (int it = 0; it < iterations; it++) { // OptimizationAlgorithmLevenberg::solve
            double currentChi = chi2_sum(S);
            const double iniChi = currentChi;
            if (tid < 14) { // the perturbed estimates of linearizeOplusXj, once for all edges
                double u[7] = {0, 0, 0, 0, 0, 0, 0};
                const int d = tid >> 1;
                const double step = (tid & 1) ? -1e-9 : 1e-9;
#pragma unroll
                for (int k = 0; k < 7; k++) if (k == d) u[k] = step;
                if (F.fix_scale) u[6] = 0;
                const Sim3 T = sim3_mul(sim3_exp(u), S);
                sim3_store(T, s_pert + tid * 8);
                sim3_store(sim3_inverse(T), s_pert + (14 + tid) * 8);
            }
            __syncthreads();
            double acc[35];
#pragma unroll
            for (int k = 0; k < 35; k++) acc[k] = 0;
            for (int i = tid; i < n; i += SIM3_THREADS) { // linearizeOplus + constructQuadraticForm (robust branch, base_binary_edge.hpp:91-113)
                if (rem[i]) continue;
#pragma unroll 1 // one body for both edges: unrolled, the two sets of 14 evaluations spill
                for (int edge = 0; edge < 2; edge++) {
                    const double *p = edge ? X1 + (long)i * 3 : X2 + (long)i * 3, *ob = edge ? O2 + (long)i * 2 : O1 + (long)i * 2, *K = problems[blockIdx.x].K + edge * 4; // read where it lies: indexing the copy F by `edge` would put F in scratch
                    const double pt[3] = {p[0], p[1], p[2]}, o2[2] = {ob[0], ob[1]};
                    const double scalar = 1.0 / (2 * 1e-9);
                    double J0[7], J1[7];
#pragma unroll
                    for (int d = 0; d < 7; d++) {
                        double ep[2], em[2];
                        sim3_edge_error(sim3_load(s_pert + (edge * 14 + 2 * d) * 8), pt, o2, K, ep);
                        sim3_edge_error(sim3_load(s_pert + (edge * 14 + 2 * d + 1) * 8), pt, o2, K, em);
                        J0[d] = scalar * (ep[0] - em[0]); J1[d] = scalar * (ep[1] - em[1]);
                    }
                    const double e[2] = {E[(long)i * 4 + edge * 2], E[(long)i * 4 + edge * 2 + 1]}, w = edge ? W2[i] : W1[i];
                    const double c = sim3_edge_chi2(e, w);
                    const double rho1 = (c <= F.dsqr) ? 1. : F.delta / sqrt(c);
                    const double r0 = (-(w * e[0])) * rho1, r1 = (-(w * e[1])) * rho1, wo = rho1 * w; // omega_r *= rho[1]; robustInformation = rho[1] * information
                    int k = 0;
#pragma unroll
                    for (int a = 0; a < 7; a++) {
#pragma unroll
                        for (int b = 0; b <= a; b++) { acc[k] += (J0[a] * wo) * J0[b] + (J1[a] * wo) * J1[b]; k++; }
                    }
#pragma unroll
                    for (int a = 0; a < 7; a++) acc[28 + a] += J0[a] * r0 + J1[a] * r1;
                }
            }
            block_reduce<35>(acc, s_red, s_sys);
            if (trace && stage == 0 && it == 0 && tid == 0) {
                for (int k = 0; k < 35; k++) system0[(long)blockIdx.x * SIM3_NSYS + k] = s_sys[k];
                system0[(long)blockIdx.x * SIM3_NSYS + 35] = currentChi;
            }
            if (it == 0) { double mx = 0; for (int a = 0; a < 7; a++) mx = fmax(fabs(s_sys[a * (a + 1) / 2 + a]), mx); lm.start(1e-5 * mx); }
            lm.begin_iteration();
            do {
                const Sim3 backup = S;
                if (tid == 0) { // (H + lambda I) x = b: LinearSolverDense, L D L^T from the lower triangle, solved where every D is positive
                    double L[7][7], D[7], x[7];
                    bool positive = true;
#pragma unroll
                    for (int j = 0; j < 7; j++) {
                        double d = s_sys[j * (j + 1) / 2 + j] + lm.lambda;
#pragma unroll
                        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * D[k];
                        D[j] = d;
                        if (!(d > 0)) positive = false;
#pragma unroll
                        for (int i = j + 1; i < 7; i++) {
                            double s = s_sys[i * (i + 1) / 2 + j];
#pragma unroll
                            for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k] * D[k];
                            L[i][j] = s / d;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 7; i++) {
                        double s = s_sys[28 + i];
#pragma unroll
                        for (int k = 0; k < i; k++) s -= L[i][k] * x[k];
                        x[i] = s;
                    }
#pragma unroll
                    for (int i = 0; i < 7; i++) x[i] = x[i] / D[i];
#pragma unroll
                    for (int i = 6; i >= 0; i--) {
                        double s = x[i];
#pragma unroll
                        for (int k = i + 1; k < 7; k++) s -= L[k][i] * x[k];
                        x[i] = s;
                    }
                    if (!positive) { for (int i = 0; i < 7; i++) x[i] = 0; }
                    if (F.fix_scale) x[6] = 0; // VertexSim3Expmap::oplusImpl writes through to the solver's x
#pragma unroll
                    for (int i = 0; i < 7; i++) s_x[i] = x[i];
                    s_flag = positive ? 1 : 0;
                    sim3_store(positive ? sim3_mul(sim3_exp(x), S) : S, s_S);
                }
                __syncthreads();
                const bool ok2 = s_flag != 0;
                S = sim3_load(s_S);
                double tempChi = chi2_sum(S);
                double scale = 0; // computeScale
                for (int j = 0; j < 7; j++) scale += s_x[j] * (lm.lambda * s_x[j] + s_sys[28 + j]);
                const bool record = trace && trials < max_trials; // the same in every thread; trials beyond max_trials are counted and not stored
                const long r0 = ((long)blockIdx.x * max_trials + trials) * CS_SIM3_TRACE_RECORD;
                if (record && tid == 0) { trace[r0] = stage; trace[r0 + 1] = it; trace[r0 + 2] = currentChi; trace[r0 + 3] = tempChi; trace[r0 + 4] = lm.lambda; trace[r0 + 5] = ok2 ? 1.0 : 0.0; }
                const bool accepted = lm.trial(currentChi, tempChi, ok2, scale);
                if (!accepted) S = backup;
                if (record && tid == 0) trace[r0 + 6] = accepted ? 1.0 : 0.0;
                trials++;
                __syncthreads(); // s_x / s_S are rewritten by the next trial
            } while (lm.retry());
            if (lm.stop(iniChi, currentChi)) break;
        }
        // the cut (Optimizer.cc:2976-2995, 3011-3026): on the _error the last trial left, accepted or not
        double cnt[1] = {0};
        for (int i = tid; i < n; i += SIM3_THREADS) {
            if (rem[i]) continue;
            const double e[4] = {E[(long)i * 4], E[(long)i * 4 + 1], E[(long)i * 4 + 2], E[(long)i * 4 + 3]};
            if (sim3_edge_chi2(e, W1[i]) > F.th2 || sim3_edge_chi2(e + 2, W2[i]) > F.th2) { rem[i] = 1; cnt[0] += 1.0; }
        }
        block_reduce<1>(cnt, s_red, s_sys + 35);
        const int flagged = (int)s_sys[35];
        __syncthreads();
        if (stage == 0) {
            nBad = flagged;
            if (n - nBad < 10) { // g2oS12 is not written: the Sim3 leaves as it came, the flags stay
                if (tid < 8) out[tid] = in[tid];
                if (tid == 0) n_inliers[blockIdx.x] = 0;
                if (trace && tid == 0) n_trials[blockIdx.x] = trials;
                return;
            }
        } else nIn = n - nBad - flagged;
    }
    if (tid == 0) { sim3_store(S, out); n_inliers[blockIdx.x] = nIn; }
    if (trace && tid == 0) n_trials[blockIdx.x] = trials;
}

__global__ void __launch_bounds__(SIM3_THREADS) sim3_exp_kernel(int n, const double *u, double *out) {
    const int v = blockIdx.x * SIM3_THREADS + threadIdx.x;
    if (v >= n) return;
    double w[7];
#pragma unroll
    for (int k = 0; k < 7; k++) w[k] = u[(long)v * 7 + k];
    sim3_store(sim3_exp(w), out + (long)v * 8);
}

// Both entries: the checks, the uploads, the one launch and the downloads.  probe == false is the product: the kernel then gets the trace pointers as NULL.
int sim3_run(cs_ctx *ctx, int n_problems, const int *corr_off, const double *P1c, const double *P2c, const double *obs1, const double *obs2, const double *inv_sigma2_1,
             const double *inv_sigma2_2, const double *intrinsics, const double *sim3_in, const float *th2, const uint8_t *fix_scale, double *sim3_out, uint8_t *removed,
             int *n_inliers, bool probe, int max_trials, double *trace, int *n_trials, double *system0) {
    if (!ctx || n_problems < 0 || (n_problems && (!corr_off || !intrinsics || !sim3_in || !th2 || !fix_scale || !sim3_out || !n_inliers))) return CS_ERR_BAD_ARG;
    if (probe && (max_trials < 0 || (n_problems && (!n_trials || !system0 || (max_trials > 0 && !trace))))) return CS_ERR_BAD_ARG;
    if (n_problems == 0) return CS_OK;
    if (corr_off[0] != 0) return CS_ERR_BAD_ARG;
    for (int f = 0; f < n_problems; f++) if (corr_off[f + 1] < corr_off[f]) return CS_ERR_BAD_ARG;
    const int ne = corr_off[n_problems];
    if (ne > 0 && (!P1c || !P2c || !obs1 || !obs2 || !inv_sigma2_1 || !inv_sigma2_2 || !removed)) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<Sim3Problem> pr((size_t)n_problems);
    for (int f = 0; f < n_problems; f++) {
        Sim3Problem &p = pr[(size_t)f];
        p.e0 = corr_off[f]; p.e1 = corr_off[f + 1]; p.fix_scale = fix_scale[f] ? 1 : 0;
        for (int k = 0; k < 8; k++) p.K[k] = intrinsics[(size_t)f * 8 + k];
        const float deltaHuber = std::sqrt(th2[f]); // Optimizer.cc:2887
        p.delta = deltaHuber;
        const float dsqr = (float)(p.delta * p.delta); // RobustKernelHuber::setDelta (robust_kernel_impl.cpp:65-69)
        p.dsqr = dsqr; p.th2 = th2[f];
    }
    Sim3Problem *d_pr = nullptr; double *d_p1 = nullptr, *d_p2 = nullptr, *d_o1 = nullptr, *d_o2 = nullptr, *d_w1 = nullptr, *d_w2 = nullptr, *d_in = nullptr, *d_out = nullptr, *d_err = nullptr;
    uint8_t *d_rem = nullptr; int *d_ni = nullptr;
    double *d_trace = nullptr, *d_sys0 = nullptr; int *d_nt = nullptr; // the probe's; they stay NULL in the product
    const size_t ne1 = (size_t)std::max(ne, 1), np = (size_t)n_problems, nz = (size_t)ne, ntr = np * (size_t)std::max(max_trials, 0) * CS_SIM3_TRACE_RECORD;
    cs_scratch sc(ctx); // (after the host array: it waits for the copy out of it before it goes)
    CS_TRY(sc.alloc(ctx, &d_pr, np));
    CS_TRY(sc.alloc(ctx, &d_p1, ne1 * 3)); CS_TRY(sc.alloc(ctx, &d_p2, ne1 * 3)); CS_TRY(sc.alloc(ctx, &d_o1, ne1 * 2)); CS_TRY(sc.alloc(ctx, &d_o2, ne1 * 2));
    CS_TRY(sc.alloc(ctx, &d_w1, ne1)); CS_TRY(sc.alloc(ctx, &d_w2, ne1)); CS_TRY(sc.alloc(ctx, &d_err, ne1 * 4)); CS_TRY(sc.alloc(ctx, &d_rem, ne1));
    CS_TRY(sc.alloc(ctx, &d_in, np * 8)); CS_TRY(sc.alloc(ctx, &d_out, np * 8)); CS_TRY(sc.alloc(ctx, &d_ni, np));
    if (probe) {
        CS_TRY(sc.alloc(ctx, &d_trace, std::max(ntr, (size_t)1))); CS_TRY(sc.alloc(ctx, &d_nt, np)); CS_TRY(sc.alloc(ctx, &d_sys0, np * CS_SIM3_TRACE_SYSTEM));
        CS_HIP(ctx, hipMemsetAsync(d_trace, 0, std::max(ntr, (size_t)1) * sizeof(double), ctx->stream));
    }
    CS_TRY(cs_h2d(ctx, d_pr, pr.data(), np));
    CS_TRY(cs_h2d(ctx, d_p1, P1c, nz * 3)); CS_TRY(cs_h2d(ctx, d_p2, P2c, nz * 3)); CS_TRY(cs_h2d(ctx, d_o1, obs1, nz * 2)); CS_TRY(cs_h2d(ctx, d_o2, obs2, nz * 2));
    CS_TRY(cs_h2d(ctx, d_w1, inv_sigma2_1, nz)); CS_TRY(cs_h2d(ctx, d_w2, inv_sigma2_2, nz));
    CS_TRY(cs_h2d(ctx, d_in, sim3_in, np * 8));
    CS_LAUNCH(ctx, "sim3_opt_kernel", sim3_opt_kernel, dim3(n_problems), dim3(SIM3_THREADS), 0, d_pr, d_p1, d_p2, d_o1, d_o2, d_w1, d_w2, d_in, d_out, d_rem, d_ni, d_err,
              max_trials, d_trace, d_nt, d_sys0);
    CS_TRY(cs_d2h(ctx, sim3_out, d_out, np * 8));
    CS_TRY(cs_d2h(ctx, removed, d_rem, nz));
    CS_TRY(cs_d2h(ctx, n_inliers, d_ni, np));
    if (probe) { CS_TRY(cs_d2h(ctx, trace, d_trace, ntr)); CS_TRY(cs_d2h(ctx, n_trials, d_nt, np)); CS_TRY(cs_d2h(ctx, system0, d_sys0, np * CS_SIM3_TRACE_SYSTEM)); }
    const hipError_t e = hipStreamSynchronize(ctx->stream); sc.drained = true;
    if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return CS_ERR_HIP; }
    return CS_OK;
}

} // namespace

extern "C" {

int cs_sim3_optimization(cs_ctx *ctx, int n_problems, const int *corr_off, const double *P1c, const double *P2c, const double *obs1, const double *obs2, const double *inv_sigma2_1,
                         const double *inv_sigma2_2, const double *intrinsics, const double *sim3_in, const float *th2, const uint8_t *fix_scale, double *sim3_out, uint8_t *removed,
                         int *n_inliers) {
    return sim3_run(ctx, n_problems, corr_off, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, intrinsics, sim3_in, th2, fix_scale, sim3_out, removed, n_inliers, false, 0, nullptr, nullptr,
                    nullptr);
}

// include/cubeslam_hip/sim3_opt_trace.h
int cs_sim3_opt_trace_version(void) { return CS_SIM3_OPT_TRACE_VERSION; }

int cs_sim3_optimization_trace(cs_ctx *ctx, int n_problems, const int *corr_off, const double *P1c, const double *P2c, const double *obs1, const double *obs2, const double *inv_sigma2_1,
                               const double *inv_sigma2_2, const double *intrinsics, const double *sim3_in, const float *th2, const uint8_t *fix_scale, double *sim3_out, uint8_t *removed,
                               int *n_inliers, int max_trials, double *trace, int *n_trials, double *system0) {
    return sim3_run(ctx, n_problems, corr_off, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, intrinsics, sim3_in, th2, fix_scale, sim3_out, removed, n_inliers, true, max_trials, trace,
                    n_trials, system0);
}

int cs_sim3_exp(cs_ctx *ctx, int n, const double *update7, double *sim3_out8) {
    if (!ctx || n < 0 || (n && (!update7 || !sim3_out8))) return CS_ERR_BAD_ARG;
    if (n == 0) return CS_OK;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    double *d_u = nullptr, *d_o = nullptr;
    CS_TRY(sc.alloc(ctx, &d_u, (size_t)n * 7)); CS_TRY(sc.alloc(ctx, &d_o, (size_t)n * 8));
    CS_TRY(cs_h2d(ctx, d_u, update7, (size_t)n * 7));
    CS_LAUNCH(ctx, "sim3_exp_kernel", sim3_exp_kernel, dim3((n + SIM3_THREADS - 1) / SIM3_THREADS), dim3(SIM3_THREADS), 0, n, d_u, d_o);
    CS_TRY(cs_d2h(ctx, sim3_out8, d_o, (size_t)n * 8));
    const hipError_t e = hipStreamSynchronize(ctx->stream); sc.drained = true;
    if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return CS_ERR_HIP; }
    return CS_OK;
}

} // extern "C"
