// sim3solver.hip -- Sim3Solver (orb_object_slam/src/Sim3Solver.cc), the RANSAC of LoopClosing::ComputeSim3 (LoopClosing.cc:231-342), for all candidates of a loop and all
// their hypotheses in one launch.  A hypothesis is a function of its three correspondences alone, and the triples are input (the reference draws them from a process-global
// rand() interleaved across solvers), so the sequential rule of iterate() is applied afterwards to a table of counts (cs_sim3_solver_walk).
//
//   s3s_hypotheses   one wave per hypothesis, four per workgroup: every lane runs horn_sim3 (horn_math.h, :224-334) on the triple -- the same values in all lanes, no
//                    exchange; the problem's N correspondences are strided over the lanes (horn_is_inlier, :336-360), the mask words are the two halves of __ballot and the
//                    count is its popcount (ransac_wave_inliers, ransac_batch.h): integers and ballots, no atomics, no order of evaluation that could change a result
//
// The entry point takes host pointers, checks every index on the host before anything is launched (s3s_build, sim3_host.h), and waits once; without a context it runs
// s3s_host_evaluate instead.  The host-only rules are forwards to sim3_host.h.
#include "common.h"
#include "sim3_host.h"

constexpr int S3S_WAVES = 4;
__global__ void __launch_bounds__(64 * S3S_WAVES) s3s_hypotheses(int n_hyp, const int *hyp_problem, const S3sProblem *problems, const S3sCorr *corr, const int *triples,
                                                                 int *n_inliers, float *sRt, uint32_t *mask) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * S3S_WAVES + (threadIdx.x >> 6);
    if (h >= n_hyp) return; // (the whole wave)
    const S3sProblem &P = problems[hyp_problem[h]];
    const S3sCorr *C = corr + P.c0;
    const S3sCorr a = C[triples[3 * (size_t)h]], b = C[triples[3 * (size_t)h + 1]], c = C[triples[3 * (size_t)h + 2]];
    HornSim3 H;
    horn_sim3(a.X1, b.X1, c.X1, a.X2, b.X2, c.X2, P.fix != 0, &H);
    uint32_t *m = mask + P.w0 + (size_t)(h - P.h0) * ransac_words(P.N);
    const int count = ransac_wave_inliers(P.N, lane, [&](int i) { const S3sCorr x = C[i]; return horn_is_inlier(H, x.X1, x.X2, x.e1, x.e2, P.K8, nullptr); }, m);
    if (lane == 0) {
        n_inliers[h] = count;
        s3s_store(H, sRt + 13 * (size_t)h);
    }
}

extern "C" {

long cs_sim3_solver_mask_words(int n_problems, const int *corr_off, const int *hyp_off) {
    if (n_problems < 0 || (n_problems && (!corr_off || !hyp_off))) return -1;
    long w = 0;
    for (int p = 0; p < n_problems; p++) {
        if (corr_off[p + 1] < corr_off[p] || hyp_off[p + 1] < hyp_off[p]) return -1;
        w += (long)(hyp_off[p + 1] - hyp_off[p]) * ransac_words(corr_off[p + 1] - corr_off[p]);
    }
    return w;
}

int cs_sim3_solver_hypotheses(cs_ctx *ctx, int n_problems, const int *corr_off, const float *X3Dc1, const float *X3Dc2, const float *max_err1, const float *max_err2,
                              const float *K8, const uint8_t *fix_scale, const int *hyp_off, const int *triples, int *n_inliers, float *sRt, uint32_t *inlier_mask) {
    std::vector<S3sProblem> problems;
    std::vector<S3sCorr> corr;
    std::vector<int> hyp_problem;
    long words = 0, at[2] = {-1, -1};
    if (const char *what = s3s_build(n_problems, corr_off, X3Dc1, X3Dc2, max_err1, max_err2, K8, fix_scale, hyp_off, triples, n_inliers && sRt && inlier_mask, problems, corr,
                                     hyp_problem, &words, at))
        return ransac_bad(ctx, "cs_sim3_solver_hypotheses", what, at[0], at[1]);
    const int H = (int)hyp_problem.size();
    if (H == 0) return CS_OK;
    if (!ctx) { // asked for by passing no context
        s3s_host_evaluate(problems, hyp_problem, corr, triples, n_inliers, sRt, inlier_mask);
        return CS_OK;
    }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx); // (after the host arrays: it waits for the copies out of them before they go)
    S3sProblem *d_prob = nullptr; S3sCorr *d_corr = nullptr; int *d_hp = nullptr, *d_tri = nullptr, *d_n = nullptr; float *d_sRt = nullptr; uint32_t *d_mask = nullptr;
    CS_TRY(sc.upload(ctx, &d_prob, problems.data(), problems.size())); CS_TRY(sc.upload(ctx, &d_corr, corr.data(), corr.size()));
    CS_TRY(sc.upload(ctx, &d_hp, hyp_problem.data(), hyp_problem.size())); CS_TRY(sc.upload(ctx, &d_tri, triples, 3 * (size_t)H));
    CS_TRY(sc.alloc(ctx, &d_n, (size_t)H)); CS_TRY(sc.alloc(ctx, &d_sRt, 13 * (size_t)H)); CS_TRY(sc.alloc(ctx, &d_mask, (size_t)words));
    CS_LAUNCH(ctx, "s3s_hypotheses", s3s_hypotheses, dim3((H + S3S_WAVES - 1) / S3S_WAVES), dim3(64 * S3S_WAVES), 0, H, d_hp, d_prob, d_corr, d_tri, d_n, d_sRt, d_mask);
    CS_TRY(cs_d2h(ctx, n_inliers, d_n, (size_t)H)); CS_TRY(cs_d2h(ctx, sRt, d_sRt, 13 * (size_t)H)); CS_TRY(cs_d2h(ctx, inlier_mask, d_mask, (size_t)words));
    return sc.drain();
}

int cs_sim3_solver_max_iterations(double probability, int min_inliers, int max_iterations, int N) { return s3s_max_iterations(probability, min_inliers, max_iterations, N); }

int cs_sim3_solver_walk(const int *n_inliers, int ransac_max_its, int min_inliers, int *mnIterations, int *mnBestInliers, int *best_hypothesis, int nIterations, int *bNoMore) {
    return s3s_walk(n_inliers, ransac_max_its, min_inliers, mnIterations, mnBestInliers, best_hypothesis, nIterations, bNoMore);
}

} // extern "C"
