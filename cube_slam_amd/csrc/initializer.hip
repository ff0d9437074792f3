// initializer.hip -- ORB_SLAM2::Initializer (orb_object_slam/src/Initializer.cc), the two-view model selection and reconstruction of Tracking::MonocularInitialization
// (Tracking.cc:948-983), for all frame pairs of a call and all their RANSAC iterations at once.  A hypothesis is a function of its eight correspondences alone and the sets
// are input (the reference draws them from a process-global stream); the best-so-far rule of :172 / :222 is a first strict maximum over the scores; ReconstructF / H are
// CheckRT over 4 or 8 candidates followed by a rule over their (nGood, parallax), which the host applies afterwards (cs_initializer_walk).
//
//   init_normalize    one wave per (problem, image): the four sums of Normalize are lane 0's, ascending; the points are strided over the lanes; T, T2inv, T2t
//   init_hypotheses   one wave per (hypothesis, model): the DLT matrix, Vt and W in LDS, the Jacobi through the executor of cv_svd_math.h with a rotation's element updates
//                     spread over the lanes, for F the completion of the null space and the rank-2 projection, the denormalisation (and for H the inverse); then the
//                     problem's N correspondences strided over the lanes (ransac_wave_inliers for mask and count).  The two score terms of a correspondence go to LDS and
//                     lane 0 adds the 128 terms of a chunk in ascending order before the next chunk: the float sum of the reference, without a slice of device memory per
//                     hypothesis (16 N bytes each would be gigabytes at 512 pairs x 200 iterations)
//   init_select       one wave per problem: the first strict maximum above 0 of the H and of the F scores, RH and the branch of :117, the decomposition into candidates
//                     (DecomposeE, or Faugeras with the return of :604), the inliers of the chosen mask
//   init_check_rt     one wave per (problem, candidate): one inlier correspondence per lane triangulated with jacobi_vmin4 in registers, the tests of :845-890 in order,
//                     vbGood as ballot words, the surviving cosines compacted by ballot ranks, and of those the min(50, nGood - 1)-th smallest by rank counting
//
// Integers, ballots and plain vector stores: no atomics, no order of evaluation that could change a result, no transcendental.  The entry point takes host pointers, checks
// everything on the host before anything is launched, launches the four kernels back to back and waits once.
#include "common.h"
#include "initializer_host.h"

struct InitWave { // the executor of cv_svd_math.h: the 64 lanes of a one-wave workgroup
    int lane;
    static constexpr int lanes = 64;
    __device__ void sync() const { __syncthreads(); }
};

__global__ void __launch_bounds__(64) init_normalize(const InitProblem *problems, InitArrays a) {
    __shared__ InitNorm nm;
    const int lane = threadIdx.x, p = blockIdx.x >> 1, image = blockIdx.x & 1;
    const InitProblem &P = problems[p];
    const float *keys = image ? a.keys2 + 2 * (size_t)P.k2 : a.keys1 + 2 * (size_t)P.k1;
    float *pn = image ? a.pn2 + 2 * (size_t)P.k2 : a.pn1 + 2 * (size_t)P.k1;
    const int n = image ? P.n2 : P.n1;
    if (lane == 0) nm = im_normalize_sums(keys, n);
    __syncthreads();
    const InitNorm m = nm;
    for (int i = lane; i < n; i += 64) im_normalize_point(m, keys + 2 * i, pn + 2 * i);
    if (lane == 0) init_normalize_matrices(m, image, P, p, a);
}

__global__ void __launch_bounds__(64) init_hypotheses(const int *hyp_problem, const InitProblem *problems, InitArrays a) {
    __shared__ InitSvdWork w;
    __shared__ float terms[128];
    __shared__ float total;
    const int lane = threadIdx.x, model = blockIdx.x >= a.H ? INIT_MODEL_F : INIT_MODEL_H, h = blockIdx.x - model * a.H, p = hyp_problem[h];
    const InitProblem &P = problems[p];
    const InitWave x{lane};
    float M[9], Minv[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    init_hypothesis(x, P, p, h, model, a, &w, M, Minv);
    const float invSigmaSquare = im_inv_sigma_square(P.sigma);
    if (lane == 0) total = 0.f;
    ransac_wave_inliers(P.N, lane, [&](int i) { return init_check_corr(P, a, model, M, Minv, invSigmaSquare, i, &terms[2 * lane], &terms[2 * lane + 1]); },
                        a.mask + (size_t)model * a.words + P.w0 + (size_t)(h - P.h0) * ransac_words(P.N),
                        [&](int base) {
                            __syncthreads();
                            if (lane == 0) {
                                float score = total;
                                const int n = min(64, P.N - base);
                                for (int k = 0; k < n; k++) score = im_score_add(score, terms[2 * k], terms[2 * k + 1]);
                                total = score;
                            }
                            __syncthreads();
                        });
    const size_t hm = (size_t)model * a.H + h;
    if (lane == 0) {
        for (int k = 0; k < 9; k++) a.matrix[9 * hm + k] = M[k];
        a.score[hm] = total;
    }
}

__global__ void __launch_bounds__(64) init_select(const InitProblem *problems, InitArrays a) {
    __shared__ InitSvdWork w;
    const int lane = threadIdx.x, p = blockIdx.x;
    const InitProblem &P = problems[p];
    float S[2];
    int best[2];
    for (int model = 0; model < 2; model++) { // :172 / :222 from score 0: the first index of the largest score above 0
        float bs = 0.f;
        int bi = -1;
        for (int i = lane; i < P.nh; i += 64) {
            const float s = a.score[(size_t)model * a.H + P.h0 + i];
            if (s > bs) { bs = s; bi = i; }
        }
        for (int d = 32; d; d >>= 1) {
            const float os = __shfl_xor(bs, d);
            const int oi = __shfl_xor(bi, d);
            if (oi >= 0 && (bi < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
        }
        S[model] = bs; best[model] = bi;
    }
    init_choose(InitWave{lane}, P, p, a, &w, S[0], S[1], best[0], best[1]);
    __syncthreads();
    const int model = a.model[p];
    if (model == INIT_MODEL_NONE) return; // (n_inliers stays 0)
    const uint32_t *m = init_chosen_mask(P, p, a);
    int N = 0; // :477-480 / :582-585
    for (int k = lane; k < ransac_words(P.N); k += 64) N += __popc(m[k]);
    for (int d = 32; d; d >>= 1) N += __shfl_xor(N, d);
    if (lane == 0) a.n_inliers[p] = N;
}

__global__ void __launch_bounds__(64) init_check_rt(const InitProblem *problems, InitArrays a) {
    const int lane = threadIdx.x, p = blockIdx.x / INIT_MAX_CAND, c = blockIdx.x % INIT_MAX_CAND;
    if (a.model[p] == INIT_MODEL_NONE || c >= a.n_cand[p]) return; // (the whole wave; its outputs stay 0)
    const InitProblem &P = problems[p];
    InitCam cam;
    im_make_cam(P.K, a.cand + 12 * ((size_t)INIT_MAX_CAND * p + c), P.sigma, &cam);
    const uint32_t *m = init_chosen_mask(P, p, a);
    uint32_t *gm = init_cand_mask(P, a, c);
    float *pts = init_cand_points(P, a, c), *list = init_cand_cos_list(P, a, c);
    const int W = ransac_words(P.N);
    int nGood = 0;
    for (int base = 0; base < P.N; base += 64) {
        const int i = base + lane;
        float p3d[3], cosParallax = 0.f;
        int st = IM_SKIPPED;
        if (i < P.N && ransac_mask_bit(m, i)) st = init_check_rt_corr(P, a, cam, i, p3d, &cosParallax);
        const unsigned long long counted = __ballot(st != IM_SKIPPED), good = __ballot(st == IM_GOOD);
        if (st != IM_SKIPPED) {
            list[nGood + wave_rank(counted, lane)] = cosParallax; // vCosParallax.push_back in ascending i
            for (int k = 0; k < 3; k++) pts[3 * (size_t)i + k] = p3d[k];
        }
        if (lane == 0) {
            gm[base >> 5] = (uint32_t)good;
            if ((base >> 5) + 1 < W) gm[(base >> 5) + 1] = (uint32_t)(good >> 32);
        }
        nGood += __popcll(counted);
    }
    if (lane == 0) a.nGood[INIT_MAX_CAND * p + c] = nGood;
    __syncthreads(); // (the list is read by other lanes than wrote it)
    if (nGood > 0) im_cos_select(InitWave{lane}, list, nGood, min(50, nGood - 1), a.cosp + INIT_MAX_CAND * p + c); // :902-905
}

extern "C" {

int cs_initializer_evaluate(cs_ctx *ctx, int n_problems, const int *key1_off, const float *keys1, const int *key2_off, const float *keys2, const int *corr_off,
                            const int *matches12, const float *K9, const float *sigma, const int *hyp_off, const int *sets, float *score, float *matrix, uint32_t *inlier_mask,
                            int *model, int *best, float *S, float *RH, int *n_inliers, int *n_cand, float *cand_Rt, int *nGood, float *cos_parallax, uint32_t *good_mask,
                            float *points) {
    std::vector<InitProblem> problems;
    std::vector<int> hyp_problem;
    long words = 0, cwords = 0, at[2] = {-1, -1};
    const bool have_per_problem = model && best && S && RH && n_inliers && n_cand && cand_Rt && nGood && cos_parallax && good_mask && points; // (written without hypotheses too)
    if (const char *what = init_build(n_problems, key1_off, keys1, key2_off, keys2, corr_off, matches12, K9, sigma, hyp_off, sets,
                                      score && matrix && inlier_mask && good_mask && points, problems, hyp_problem, &words, &cwords, at))
        return ransac_bad(ctx, "cs_initializer_evaluate", what, at[0], at[1]);
    if (n_problems == 0) return CS_OK;
    if (!have_per_problem) return ransac_bad(ctx, "cs_initializer_evaluate", "NULL argument", -1, -1);
    const int H = hyp_off[n_problems], NC = corr_off[n_problems], NK1 = key1_off[n_problems], NK2 = key2_off[n_problems];
    const size_t np = (size_t)n_problems;
    if (!ctx) { // asked for by passing no context
        init_host_run(problems, keys1, keys2, matches12, sets, H, words, cwords, NK1, NK2, NC,
                      InitOutputs{score, matrix, inlier_mask, model, best, S, RH, n_inliers, n_cand, cand_Rt, nGood, cos_parallax, good_mask, points});
        return CS_OK;
    }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx); // (after the host arrays: it waits for the copies out of them before they go)
    InitProblem *d_prob = nullptr; int *d_hp = nullptr, *d_matches = nullptr, *d_sets = nullptr, *d_int = nullptr; float *d_keys1 = nullptr, *d_keys2 = nullptr, *d_f = nullptr;
    float *d_score = nullptr, *d_matrix = nullptr, *d_points = nullptr, *d_cos_list = nullptr; uint32_t *d_mask = nullptr, *d_gm = nullptr;
    CS_TRY(sc.upload(ctx, &d_prob, problems.data(), np)); CS_TRY(sc.upload(ctx, &d_hp, hyp_problem.data(), (size_t)H));
    CS_TRY(sc.upload(ctx, &d_keys1, keys1, 2 * (size_t)NK1)); CS_TRY(sc.upload(ctx, &d_keys2, keys2, 2 * (size_t)NK2));
    CS_TRY(sc.upload(ctx, &d_matches, matches12, 2 * (size_t)NC)); CS_TRY(sc.upload(ctx, &d_sets, sets, 8 * (size_t)H));
    // per problem, ints: model 1, best 2, n_inliers 1, n_cand 1, nGood 8; floats: T1 T2inv T2t 27, S 2, RH 1, cand 96, cosp 8; then pn1, pn2
    const size_t ni = 13 * np, nf = 134 * np;
    CS_TRY(sc.alloc(ctx, &d_int, ni)); CS_TRY(sc.alloc(ctx, &d_f, nf + 2 * (size_t)NK1 + 2 * (size_t)NK2));
    CS_TRY(sc.alloc(ctx, &d_score, 2 * (size_t)H)); CS_TRY(sc.alloc(ctx, &d_matrix, 18 * (size_t)H)); CS_TRY(sc.alloc(ctx, &d_mask, 2 * (size_t)words));
    CS_TRY(sc.alloc(ctx, &d_gm, (size_t)cwords)); CS_TRY(sc.alloc(ctx, &d_points, 3 * (size_t)INIT_MAX_CAND * NC)); CS_TRY(sc.alloc(ctx, &d_cos_list, (size_t)INIT_MAX_CAND * NC));
    CS_HIP(ctx, hipMemsetAsync(d_int, 0, sizeof(int) * ni, ctx->stream)); // (what a candidate that is not evaluated leaves: zeros)
    CS_HIP(ctx, hipMemsetAsync(d_f, 0, sizeof(float) * nf, ctx->stream));
    CS_HIP(ctx, hipMemsetAsync(d_gm, 0, sizeof(uint32_t) * std::max<size_t>((size_t)cwords, 1), ctx->stream));
    CS_HIP(ctx, hipMemsetAsync(d_points, 0, sizeof(float) * std::max<size_t>(3 * (size_t)INIT_MAX_CAND * NC, 1), ctx->stream));
    int *d_model = d_int, *d_best = d_int + np, *d_ninl = d_int + 3 * np, *d_ncand = d_int + 4 * np, *d_nGood = d_int + 5 * np;
    float *d_T = d_f, *d_S = d_f + 27 * np, *d_RH = d_f + 29 * np, *d_cand = d_f + 30 * np, *d_cosp = d_f + 126 * np, *d_pn1 = d_f + nf, *d_pn2 = d_pn1 + 2 * (size_t)NK1;
    const InitArrays a{d_keys1, d_keys2, d_matches, d_sets, d_pn1, d_pn2, d_T, d_T + 9 * np, d_T + 18 * np, H, words, d_score, d_matrix, d_mask,
                       d_model, d_best, d_ninl, d_ncand, d_nGood, d_S, d_RH, d_cand, d_cosp, d_points, d_cos_list, d_gm};
    CS_LAUNCH(ctx, "init_normalize", init_normalize, dim3(2 * n_problems), dim3(64), 0, d_prob, a);
    if (H) CS_LAUNCH(ctx, "init_hypotheses", init_hypotheses, dim3(2 * H), dim3(64), 0, d_hp, d_prob, a);
    CS_LAUNCH(ctx, "init_select", init_select, dim3(n_problems), dim3(64), 0, d_prob, a);
    CS_LAUNCH(ctx, "init_check_rt", init_check_rt, dim3(INIT_MAX_CAND * n_problems), dim3(64), 0, d_prob, a);
    CS_TRY(cs_d2h(ctx, score, d_score, 2 * (size_t)H)); CS_TRY(cs_d2h(ctx, matrix, d_matrix, 18 * (size_t)H)); CS_TRY(cs_d2h(ctx, inlier_mask, d_mask, 2 * (size_t)words));
    CS_TRY(cs_d2h(ctx, model, d_model, np)); CS_TRY(cs_d2h(ctx, best, d_best, 2 * np)); CS_TRY(cs_d2h(ctx, n_inliers, d_ninl, np)); CS_TRY(cs_d2h(ctx, n_cand, d_ncand, np));
    CS_TRY(cs_d2h(ctx, nGood, d_nGood, INIT_MAX_CAND * np)); CS_TRY(cs_d2h(ctx, S, d_S, 2 * np)); CS_TRY(cs_d2h(ctx, RH, d_RH, np));
    CS_TRY(cs_d2h(ctx, cand_Rt, d_cand, 12 * INIT_MAX_CAND * np)); CS_TRY(cs_d2h(ctx, cos_parallax, d_cosp, INIT_MAX_CAND * np));
    CS_TRY(cs_d2h(ctx, good_mask, d_gm, (size_t)cwords)); CS_TRY(cs_d2h(ctx, points, d_points, 3 * (size_t)INIT_MAX_CAND * NC));
    return sc.drain();
}

int cs_initializer_walk(int model, int n_cand, const int *nGood, const float *cos_parallax, int N, float minParallax, int minTriangulated, float *parallax) {
    if (!nGood || !cos_parallax) return CS_ERR_BAD_ARG;
    return init_walk(model, n_cand, nGood, cos_parallax, N, minParallax, minTriangulated, parallax);
}

} // extern "C"
