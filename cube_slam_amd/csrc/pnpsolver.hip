// pnpsolver.hip -- PnPsolver (orb_object_slam/src/PnPsolver.cc), the RANSAC over EPnP of Tracking::Relocalization (Tracking.cc:2876-3030), for all candidates of a
// relocalisation and all their hypotheses in one call.  A hypothesis is a function of its four correspondences alone and the quads are input (the reference draws them from a
// process-global stream interleaved across solvers); Refine() (:258-303) is a function of the best-so-far mask, so the distinct refinements are those of the record
// hypotheses -- the strict prefix maxima among the counts >= mRansacMinInliers -- and which hypotheses are records depends on the counts alone.  iterate()'s sequential rule is
// applied afterwards to the two tables n_inliers, refined_n (cs_pnp_solver_walk).
//
//   pnp_hypotheses   one wave (one workgroup) per hypothesis: EPnP on the quad (epnp_compute_pose, epnp_math.h) with its state in LDS -- the 12 x 12 Jacobi spreads a
//                    rotation's 24 element updates over the lanes, every dot product is summed by each lane over ascending k, the serial statements are lane 0's --, then the
//                    problem's N correspondences strided over the lanes (epnp_is_inlier): the mask words are the halves of __ballot, the count its popcount (ransac_wave_inliers,
//                    ransac_batch.h)
//   pnp_records      one wave per problem: the strict prefix maximum over the counts from best_in[p], by a max-scan over lane shuffles; integers only
//   pnp_refine       launched over all hypotheses, a non-record leaves at once: the record's inliers are gathered in ascending order (ballot ranks) into its slice of the
//                    call's scratch, EPnP on them -- the 3 + 6 + 78 + 6 + 9 sums over correspondences one lane per entry over ascending i, alphas, pcs and the
//                    reprojection terms one point per lane, the reprojection sum ascending in lane 0 --, then CheckInliers as above
//
// Integers, ballots and plain vector stores: no atomics, no order of evaluation that could change a result.  The entry point takes host pointers, checks every index on the
// host before anything is launched, launches the three kernels back to back and waits once.
#include "common.h"
#include "pnp_host.h"
#include "pnp_walk.h"

struct PnpWave { // the executor of cv_svd_math.h: the 64 lanes of a one-wave workgroup
    int lane;
    static constexpr int lanes = 64;
    __device__ void sync() const { __syncthreads(); }
};

// CheckInliers over the problem's correspondences with the pose in LDS; every lane returns the count
__device__ int pnp_check_inliers(const PnpProblem &P, const PnpCorr *C, const double *Rt_lds, int lane, uint32_t *m) {
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = Rt_lds[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = Rt_lds[9 + k];
    return ransac_wave_inliers(P.N, lane, [&](int i) { const PnpCorr x = C[i]; return epnp_is_inlier(R, t, P.K, x.X, x.u, x.e); }, m);
}

__global__ void __launch_bounds__(64) pnp_hypotheses(const int *hyp_problem, const PnpProblem *problems, const PnpCorr *corr, const int *quads, int *n_inliers, double *Rt,
                                                     uint32_t *status, uint32_t *mask) {
    __shared__ EpnpWork w;
    __shared__ double points[4 * PNP_POINT_DOUBLES];
    __shared__ double pose[12];
    const int lane = threadIdx.x, h = blockIdx.x;
    const PnpProblem &P = problems[hyp_problem[h]];
    const PnpCorr *C = corr + P.c0;
    const PnpWave x{lane};
    if (lane == 0) {
        pnp_work_init(&w, P.K, 4, points);
        for (int k = 0; k < 4; k++) { // add_correspondence
            const PnpCorr c = C[quads[4 * (size_t)h + k]];
            w.pws[3 * k] = c.X[0]; w.pws[3 * k + 1] = c.X[1]; w.pws[3 * k + 2] = c.X[2];
            w.us[2 * k] = c.u[0]; w.us[2 * k + 1] = c.u[1];
        }
    }
    x.sync();
    epnp_compute_pose(x, &w, pose, pose + 9);
    const int count = pnp_check_inliers(P, C, pose, lane, mask + P.w0 + (size_t)(h - P.h0) * ransac_words(P.N));
    if (lane < 12) Rt[12 * (size_t)h + lane] = pose[lane];
    if (lane == 0) { n_inliers[h] = count; status[h] = w.status; }
}

__global__ void __launch_bounds__(64) pnp_records(const PnpProblem *problems, const int *n_inliers, uint8_t *is_record) {
    const PnpProblem &P = problems[blockIdx.x];
    const int lane = threadIdx.x;
    int carry = P.best_in; // mnBestInliers
    for (int base = 0; base < P.nh; base += 64) {
        const int i = base + lane;
        const int c = i < P.nh ? n_inliers[P.h0 + i] : 0;
        const bool q = i < P.nh && c >= P.min_inliers; // :208
        int incl = q ? c : INT_MIN;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl = max(incl, o);
        }
        int before = __shfl_up(incl, 1);
        before = lane == 0 ? carry : max(carry, before);
        if (i < P.nh) is_record[P.h0 + i] = q && c > before; // :211
        carry = max(carry, __shfl(incl, 63));
    }
}

__global__ void __launch_bounds__(64) pnp_refine(const int *hyp_problem, const PnpProblem *problems, const PnpCorr *corr, const int *n_inliers, const uint32_t *mask,
                                                 const uint8_t *is_record, double *scratch, int *refined_n, double *refined_Rt, uint32_t *status, uint32_t *refined_mask) {
    __shared__ EpnpWork w;
    __shared__ double pose[12];
    const int lane = threadIdx.x, h = blockIdx.x;
    if (!is_record[h]) { // (the whole wave)
        if (lane == 0) refined_n[h] = -1;
        return;
    }
    const PnpProblem &P = problems[hyp_problem[h]];
    const PnpCorr *C = corr + P.c0;
    const int N = P.N, W = ransac_words(N), n = n_inliers[h];
    const uint32_t *m = mask + P.w0 + (size_t)(h - P.h0) * W;
    double *points = scratch + P.s0 + (size_t)(h - P.h0) * N * PNP_POINT_DOUBLES; // n <= N of them are used
    const PnpWave x{lane};
    if (lane == 0) pnp_work_init(&w, P.K, n, points);
    x.sync();
    int rank = 0; // Refine :263-279: the inliers in ascending order
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool in = i < N && ransac_mask_bit(m, i);
        const unsigned long long bal = __ballot(in);
        if (in) {
            const int k = rank + wave_rank(bal, lane);
            const PnpCorr c = C[i];
            w.pws[3 * (size_t)k] = c.X[0]; w.pws[3 * (size_t)k + 1] = c.X[1]; w.pws[3 * (size_t)k + 2] = c.X[2];
            w.us[2 * (size_t)k] = c.u[0]; w.us[2 * (size_t)k + 1] = c.u[1];
        }
        rank += __popcll(bal);
    }
    x.sync();
    epnp_compute_pose(x, &w, pose, pose + 9);
    const int count = pnp_check_inliers(P, C, pose, lane, refined_mask + P.w0 + (size_t)(h - P.h0) * W);
    if (lane < 12) refined_Rt[12 * (size_t)h + lane] = pose[lane];
    if (lane == 0) {
        refined_n[h] = count;
        status[h] = status[h] | PNP_RECORD | ((w.status & EPNP_QR_SINGULAR) ? PNP_REFINE_QR_SINGULAR : 0u);
    }
}

extern "C" {

int cs_pnp_solver_evaluate(cs_ctx *ctx, int n_problems, const int *corr_off, const float *P3Dw, const float *P2D, const float *max_err, const float *K4, const int *min_inliers,
                           const int *best_in, const int *hyp_off, const int *quads, int *n_inliers, double *Rt, uint32_t *status, uint32_t *inlier_mask, int *refined_n,
                           double *refined_Rt, uint32_t *refined_mask) {
    std::vector<PnpProblem> problems;
    std::vector<PnpCorr> corr;
    std::vector<int> hyp_problem;
    long words = 0, sdoubles = 0, at[2] = {-1, -1};
    if (const char *what = pnp_build(n_problems, corr_off, P3Dw, P2D, max_err, K4, min_inliers, best_in, hyp_off, quads,
                                     n_inliers && Rt && status && inlier_mask && refined_n && refined_Rt && refined_mask, problems, corr, hyp_problem, &words, &sdoubles, at))
        return ransac_bad(ctx, "cs_pnp_solver_evaluate", what, at[0], at[1]);
    if (n_problems == 0) return CS_OK;
    const int H = hyp_off[n_problems];
    if (H == 0) return CS_OK;
    if (!ctx) { // asked for by passing no context
        for (size_t k = 0; k < 12 * (size_t)H; k++) refined_Rt[k] = 0; // (what a non-record leaves)
        for (long k = 0; k < words; k++) refined_mask[k] = 0;
        pnp_host_evaluate(problems, corr, quads, n_inliers, Rt, status, inlier_mask, refined_n, refined_Rt, refined_mask);
        return CS_OK;
    }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx); // (after the host arrays: it waits for the copies out of them before they go)
    PnpProblem *d_prob = nullptr; PnpCorr *d_corr = nullptr; int *d_hp = nullptr, *d_quads = nullptr, *d_n = nullptr, *d_rn = nullptr; double *d_Rt = nullptr, *d_rRt = nullptr, *d_pts = nullptr;
    uint32_t *d_st = nullptr, *d_mask = nullptr, *d_rmask = nullptr; uint8_t *d_rec = nullptr;
    CS_TRY(sc.upload(ctx, &d_prob, problems.data(), problems.size())); CS_TRY(sc.upload(ctx, &d_corr, corr.data(), corr.size()));
    CS_TRY(sc.upload(ctx, &d_hp, hyp_problem.data(), hyp_problem.size())); CS_TRY(sc.upload(ctx, &d_quads, quads, 4 * (size_t)H));
    CS_TRY(sc.alloc(ctx, &d_n, (size_t)H)); CS_TRY(sc.alloc(ctx, &d_rn, (size_t)H)); CS_TRY(sc.alloc(ctx, &d_Rt, 12 * (size_t)H)); CS_TRY(sc.alloc(ctx, &d_st, (size_t)H));
    CS_TRY(sc.alloc(ctx, &d_mask, (size_t)words)); CS_TRY(sc.alloc(ctx, &d_rec, (size_t)H)); CS_TRY(sc.alloc(ctx, &d_pts, (size_t)sdoubles));
    CS_TRY(sc.alloc(ctx, &d_rRt, 12 * (size_t)H)); CS_TRY(sc.alloc(ctx, &d_rmask, (size_t)words));
    CS_HIP(ctx, hipMemsetAsync(d_rRt, 0, sizeof(double) * 12 * (size_t)H, ctx->stream)); // (what a non-record leaves: zeros)
    CS_HIP(ctx, hipMemsetAsync(d_rmask, 0, sizeof(uint32_t) * (size_t)words, ctx->stream));
    CS_LAUNCH(ctx, "pnp_hypotheses", pnp_hypotheses, dim3(H), dim3(64), 0, d_hp, d_prob, d_corr, d_quads, d_n, d_Rt, d_st, d_mask);
    CS_LAUNCH(ctx, "pnp_records", pnp_records, dim3(n_problems), dim3(64), 0, d_prob, d_n, d_rec);
    CS_LAUNCH(ctx, "pnp_refine", pnp_refine, dim3(H), dim3(64), 0, d_hp, d_prob, d_corr, d_n, d_mask, d_rec, d_pts, d_rn, d_rRt, d_st, d_rmask);
    CS_TRY(cs_d2h(ctx, n_inliers, d_n, (size_t)H)); CS_TRY(cs_d2h(ctx, Rt, d_Rt, 12 * (size_t)H)); CS_TRY(cs_d2h(ctx, status, d_st, (size_t)H));
    CS_TRY(cs_d2h(ctx, inlier_mask, d_mask, (size_t)words)); CS_TRY(cs_d2h(ctx, refined_n, d_rn, (size_t)H)); CS_TRY(cs_d2h(ctx, refined_Rt, d_rRt, 12 * (size_t)H));
    CS_TRY(cs_d2h(ctx, refined_mask, d_rmask, (size_t)words));
    return sc.drain();
}

int cs_pnp_solver_ransac_parameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, int N, int *mRansacMinInliers, int *mRansacMaxIts,
                                    float *mRansacEpsilon) {
    if (!mRansacMinInliers || !mRansacMaxIts || !mRansacEpsilon || N < 0) return CS_ERR_BAD_ARG;
    pnp_ransac_parameters(probability, minInliers, maxIterations, minSet, epsilon, N, mRansacMinInliers, mRansacMaxIts, mRansacEpsilon);
    return CS_OK;
}

int cs_pnp_solver_walk(const int *n_inliers, const int *refined_n, int n_hyp, int ransac_max_its, int min_inliers, int *mnIterations, int *mnBestInliers, int *best_hypothesis,
                       int nIterations, int *bNoMore, int *refined) {
    return pnp_walk(n_inliers, refined_n, n_hyp, ransac_max_its, min_inliers, mnIterations, mnBestInliers, best_hypothesis, nIterations, bNoMore, refined);
}

} // extern "C"
