// sim3solver.hip -- Sim3Solver (orb_object_slam/src/Sim3Solver.cc), the RANSAC of LoopClosing::ComputeSim3 (LoopClosing.cc:231-342), for all candidates of a loop and all
// their hypotheses in one launch.  A hypothesis is a function of its three correspondences alone, and the triples are input (the reference draws them from a process-global
// rand() interleaved across solvers), so the sequential rule of iterate() is applied afterwards to a table of counts (cs_sim3_solver_walk).
//
//   s3s_hypotheses   one wave per hypothesis, four per workgroup: every lane runs horn_sim3 (horn_math.h, :224-334) on the triple -- the same values in all lanes, no
//                    exchange; the problem's N correspondences are strided over the lanes (horn_is_inlier, :336-360), the mask words are the two halves of __ballot and the
//                    count is its popcount: integers and ballots, no atomics, no order of evaluation that could change a result
//
// The entry point takes host pointers, checks every index on the host before anything is launched, and waits once.
#include "common.h"
#include "horn_math.h"

struct S3sProblem { int c0, N, h0, fix; long w0; float K8[8]; }; // first correspondence, their number, first hypothesis, mbFixScale, first mask word
struct S3sCorr { float X1[3], e1, X2[3], e2; };                  // mvX3Dc1[i], mvnMaxError1[i], mvX3Dc2[i], mvnMaxError2[i]: two 16-byte loads

constexpr int S3S_WAVES = 4;
__global__ void __launch_bounds__(64 * S3S_WAVES) s3s_hypotheses(int n_hyp, const int *hyp_problem, const S3sProblem *problems, const S3sCorr *corr, const int *triples,
                                                                 int *n_inliers, float *sRt, uint32_t *mask) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * S3S_WAVES + (threadIdx.x >> 6);
    if (h >= n_hyp) return; // (the whole wave)
    const S3sProblem &P = problems[hyp_problem[h]];
    const S3sCorr *C = corr + P.c0;
    const int N = P.N, W = (N + 31) >> 5;
    const S3sCorr a = C[triples[3 * (size_t)h]], b = C[triples[3 * (size_t)h + 1]], c = C[triples[3 * (size_t)h + 2]];
    HornSim3 H;
    horn_sim3(a.X1, b.X1, c.X1, a.X2, b.X2, c.X2, P.fix != 0, &H);
    uint32_t *m = mask + P.w0 + (size_t)(h - P.h0) * W;
    int count = 0;
    for (int base = 0; base < N; base += 64) { // (wave-uniform trip count: every lane reaches the ballot)
        const int i = base + lane;
        bool in = false;
        if (i < N) {
            const S3sCorr x = C[i];
            in = horn_is_inlier(H, x.X1, x.X2, x.e1, x.e2, P.K8, nullptr);
        }
        const unsigned long long bal = __ballot(in);
        count += __popcll(bal);
        if (lane == 0) {
            m[base >> 5] = (uint32_t)bal;
            if ((base >> 5) + 1 < W) m[(base >> 5) + 1] = (uint32_t)(bal >> 32);
        }
    }
    if (lane == 0) {
        n_inliers[h] = count;
        float *o = sRt + 13 * (size_t)h;
        o[0] = H.s;
        for (int k = 0; k < 9; k++) o[1 + k] = H.R[k];
        for (int k = 0; k < 3; k++) o[10 + k] = H.t[k];
    }
}

static int s3s_bad(cs_ctx *ctx, const char *what, long a = -1, long b = -1) {
    if (!ctx) return CS_ERR_BAD_ARG;
    char buf[256];
    if (a >= 0 && b >= 0) snprintf(buf, sizeof buf, "cs_sim3_solver_hypotheses: %s (%ld, %ld)", what, a, b);
    else if (a >= 0) snprintf(buf, sizeof buf, "cs_sim3_solver_hypotheses: %s (%ld)", what, a);
    else snprintf(buf, sizeof buf, "cs_sim3_solver_hypotheses: %s", what);
    ctx->err = buf;
    return CS_ERR_BAD_ARG;
}

extern "C" {

long cs_sim3_solver_mask_words(int n_problems, const int *corr_off, const int *hyp_off) {
    if (n_problems < 0 || (n_problems && (!corr_off || !hyp_off))) return -1;
    long w = 0;
    for (int p = 0; p < n_problems; p++) {
        if (corr_off[p + 1] < corr_off[p] || hyp_off[p + 1] < hyp_off[p]) return -1;
        w += (long)(hyp_off[p + 1] - hyp_off[p]) * ((corr_off[p + 1] - corr_off[p] + 31) / 32);
    }
    return w;
}

int cs_sim3_solver_hypotheses(cs_ctx *ctx, int n_problems, const int *corr_off, const float *X3Dc1, const float *X3Dc2, const float *max_err1, const float *max_err2,
                              const float *K8, const uint8_t *fix_scale, const int *hyp_off, const int *triples, int *n_inliers, float *sRt, uint32_t *inlier_mask) {
    if (n_problems < 0) return s3s_bad(ctx, "n_problems < 0");
    if (n_problems == 0) return CS_OK;
    if (!cs_offsets_ok(corr_off, n_problems, X3Dc1) || !cs_offsets_ok(hyp_off, n_problems, triples)) return s3s_bad(ctx, "offsets that do not start at 0 or decrease, or a NULL array");
    const int NC = corr_off[n_problems], H = hyp_off[n_problems];
    if (!K8 || !fix_scale || (NC && (!X3Dc2 || !max_err1 || !max_err2)) || (H && (!n_inliers || !sRt || !inlier_mask))) return s3s_bad(ctx, "NULL argument");
    std::vector<S3sProblem> problems((size_t)n_problems);
    std::vector<int> hyp_problem((size_t)H);
    long words = 0;
    for (int p = 0; p < n_problems; p++) {
        const int N = corr_off[p + 1] - corr_off[p], nh = hyp_off[p + 1] - hyp_off[p];
        if (nh && N < 3) return s3s_bad(ctx, "a problem with hypotheses and fewer than 3 correspondences", p);
        for (int h = hyp_off[p]; h < hyp_off[p + 1]; h++) {
            const int *t = triples + 3 * (size_t)h;
            for (int k = 0; k < 3; k++) if (t[k] < 0 || t[k] >= N) return s3s_bad(ctx, "a triple index outside its problem (problem, hypothesis)", p, h);
            if (t[0] == t[1] || t[0] == t[2] || t[1] == t[2]) return s3s_bad(ctx, "two equal indices in a triple (problem, hypothesis)", p, h);
            hyp_problem[h] = p;
        }
        S3sProblem &P = problems[p];
        P.c0 = corr_off[p]; P.N = N; P.h0 = hyp_off[p]; P.fix = fix_scale[p] != 0; P.w0 = words;
        for (int k = 0; k < 8; k++) P.K8[k] = K8[8 * (size_t)p + k];
        words += (long)nh * ((N + 31) / 32);
    }
    if (H == 0) return CS_OK;
    std::vector<S3sCorr> corr((size_t)NC);
    for (int i = 0; i < NC; i++) {
        S3sCorr &c = corr[i];
        for (int k = 0; k < 3; k++) { c.X1[k] = X3Dc1[3 * (size_t)i + k]; c.X2[k] = X3Dc2[3 * (size_t)i + k]; }
        c.e1 = max_err1[i]; c.e2 = max_err2[i];
    }
    if (!ctx) { // the host evaluation of the same text, asked for by passing no context
        for (int h = 0; h < H; h++) {
            const S3sProblem &P = problems[hyp_problem[h]];
            const S3sCorr *C = corr.data() + P.c0;
            const int W = (P.N + 31) >> 5;
            const S3sCorr &a = C[triples[3 * (size_t)h]], &b = C[triples[3 * (size_t)h + 1]], &c = C[triples[3 * (size_t)h + 2]];
            HornSim3 Hs;
            horn_sim3(a.X1, b.X1, c.X1, a.X2, b.X2, c.X2, P.fix != 0, &Hs);
            uint32_t *m = inlier_mask + P.w0 + (size_t)(h - P.h0) * W;
            for (int w = 0; w < W; w++) m[w] = 0;
            int count = 0;
            for (int i = 0; i < P.N; i++)
                if (horn_is_inlier(Hs, C[i].X1, C[i].X2, C[i].e1, C[i].e2, P.K8, nullptr)) { m[i >> 5] |= 1u << (i & 31); count++; }
            n_inliers[h] = count;
            float *o = sRt + 13 * (size_t)h;
            o[0] = Hs.s;
            for (int k = 0; k < 9; k++) o[1 + k] = Hs.R[k];
            for (int k = 0; k < 3; k++) o[10 + k] = Hs.t[k];
        }
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

int cs_sim3_solver_max_iterations(double probability, int min_inliers, int max_iterations, int N) { // SetRansacParameters :118-133
    if (N < min_inliers) return 0; // iterate returns at :144
    float epsilon = (float)min_inliers / N;
    int nIterations;
    if (min_inliers == N) nIterations = 1;
    else {
        // (pow(float, int) is the double pow.)  Where the quotient does not fit an int -- N in the thousands at small min_inliers, or pow() below 2^-53, where log(1 - 0) = +0
        // makes it -inf -- the reference's conversion is undefined (x86 yields INT_MIN, hence one iteration); the library takes the bound: max_iterations
        const double q = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0)));
        nIterations = (q > -2147483648.0 && q < 2147483648.0) ? (int)q : max_iterations;
    }
    return std::max(1, std::min(nIterations, max_iterations));
}

int cs_sim3_solver_walk(const int *n_inliers, int ransac_max_its, int min_inliers, int *mnIterations, int *mnBestInliers, int *best_hypothesis, int nIterations, int *bNoMore) {
    *bNoMore = 0;
    int nCurrentIterations = 0;
    while (*mnIterations < ransac_max_its && nCurrentIterations < nIterations) { // :156
        nCurrentIterations++;
        const int t = (*mnIterations)++;
        const int mnInliersi = n_inliers[t];
        if (mnInliersi >= *mnBestInliers) { // :181
            *mnBestInliers = mnInliersi;
            *best_hypothesis = t;
            if (mnInliersi > min_inliers) return t; // :190
        }
    }
    if (*mnIterations >= ransac_max_its) *bNoMore = 1; // :201
    return -1;
}

} // extern "C"
