// initializer_host.h -- the records of cs_initializer_evaluate, its checks, and its evaluation on one host thread over initializer_math.h: the path of initializer.hip
// without a context, and of cubeslam::Initializer with or without the library (host/initializer.hpp).  The kernels of initializer.hip make the same statements with a wave
// as the executor.  The batch, its checks and the mask layout are ransac_batch.h's, shared with sim3_host.h and pnp_host.h.
#pragma once
#include "initializer_math.h"
#include "initializer_walk.h"
#include "ransac_batch.h"

// One frame pair: first key point of frame 1 / 2 and their numbers, first match and their number, first hypothesis and their number, first mask word of its hypotheses (per
// model), first mask word of its candidates
struct InitProblem { int k1, n1, k2, n2, c0, N, h0, nh; long w0, cw0; float K[9], sigma; };

constexpr int INIT_MAX_CAND = 8;

// the arrays of a call, the caller's on the host or their images on the device (layout: include/cubeslam_hip.h)
struct InitArrays {
    const float *keys1, *keys2; // x y per key point
    const int *matches;         // first, second per correspondence, indices into the problem's key points
    const int *sets;            // 8 per hypothesis
    float *pn1, *pn2;           // vPn1, vPn2 of every key point
    float *T1, *T2inv, *T2t;    // 9 per problem
    int H; long words;          // hypotheses and mask words of the call, per model
    float *score, *matrix; uint32_t *mask;
    int *model, *best, *n_inliers, *n_cand, *nGood;
    float *S, *RH, *cand, *cosp, *points, *cos_list;
    uint32_t *good_mask;
};

// ---- what the kernels and the host path share
// Normalize of one image's n key points by one lane after the sums; T (and for image 2 its inverse and transpose)
HD void init_normalize_matrices(const InitNorm &nm, int image, const InitProblem &P, int p, const InitArrays &a) {
    float T[9];
    im_normalize_T(nm, T);
    if (image == 0) for (int k = 0; k < 9; k++) a.T1[9 * (size_t)p + k] = T[k];
    else {
        im_inv3(T, a.T2inv + 9 * (size_t)p);    // :141
        im_transpose(T, a.T2t + 9 * (size_t)p); // :191
    }
}

// the matrices of hypothesis h under one model, by all lanes of x: M = H21i or F21i, Minv = H12i (model H)
template <class X> HD void init_hypothesis(X x, const InitProblem &P, int p, int h, int model, const InitArrays &a, InitSvdWork *w, float *M, float *Minv) {
    float Mn[9];
    const int *set = a.sets + 8 * (size_t)h, *mt = a.matches + 2 * (size_t)P.c0;
    for (int j = x.lane; j < 8; j += x.lanes) { // :158-164
        const int idx = set[j], i1 = mt[2 * idx], i2 = mt[2 * idx + 1];
        w->p1[2 * j] = a.pn1[2 * (size_t)(P.k1 + i1)]; w->p1[2 * j + 1] = a.pn1[2 * (size_t)(P.k1 + i1) + 1];
        w->p2[2 * j] = a.pn2[2 * (size_t)(P.k2 + i2)]; w->p2[2 * j + 1] = a.pn2[2 * (size_t)(P.k2 + i2) + 1];
    }
    x.sync();
    if (model == INIT_MODEL_H) {
        im_compute_H21(x, w, Mn);
        im_denormalise(a.T2inv + 9 * (size_t)p, Mn, a.T1 + 9 * (size_t)p, M);
        im_inv3(M, Minv);
    } else {
        im_compute_F21(x, w, Mn);
        im_denormalise(a.T2t + 9 * (size_t)p, Mn, a.T1 + 9 * (size_t)p, M);
    }
}

// CheckHomography / CheckFundamental for correspondence i
HD bool init_check_corr(const InitProblem &P, const InitArrays &a, int model, const float *M, const float *Minv, float invSigmaSquare, int i, float *t1, float *t2) {
    const int *mt = a.matches + 2 * (size_t)(P.c0 + i);
    const float *k1 = a.keys1 + 2 * (size_t)(P.k1 + mt[0]), *k2 = a.keys2 + 2 * (size_t)(P.k2 + mt[1]);
    return model == INIT_MODEL_H ? im_check_h(M, Minv, k1[0], k1[1], k2[0], k2[1], invSigmaSquare, t1, t2) : im_check_f(M, k1[0], k1[1], k2[0], k2[1], invSigmaSquare, t1, t2);
}

// After the two maxima (bestH, bestF: the first strict maximum above 0 of each model, -1 without one; S their scores, 0 without one): RH, the branch of :117 and the
// candidates of the chosen model.  By all lanes of x; lane 0 writes.  No model: the chosen model has no hypothesis (RH is a NaN and the reference's F is empty).
template <class X> HD void init_choose(X x, const InitProblem &P, int p, const InitArrays &a, InitSvdWork *w, float SH, float SF, int bestH, int bestF) {
    const float RH = SH / (SH + SF); // :113
    int model = (double)RH > 0.40 ? INIT_MODEL_H : INIT_MODEL_F;
    const int b = model == INIT_MODEL_H ? bestH : bestF;
    if (b < 0) model = INIT_MODEL_NONE;
    float cand[12 * INIT_MAX_CAND];
    for (int k = 0; k < 12 * INIT_MAX_CAND; k++) cand[k] = 0.f;
    int n_cand = 0;
    if (model != INIT_MODEL_NONE) {
        const float *M = a.matrix + 9 * ((size_t)model * a.H + P.h0 + b);
        n_cand = model == INIT_MODEL_H ? im_candidates_H(x, M, P.K, w, cand) : im_candidates_F(x, M, P.K, w, cand);
    }
    if (x.lane == 0) {
        a.S[2 * p] = SH; a.S[2 * p + 1] = SF; a.best[2 * p] = bestH; a.best[2 * p + 1] = bestF;
        a.RH[p] = RH; a.model[p] = model; a.n_cand[p] = n_cand;
        for (int k = 0; k < 12 * INIT_MAX_CAND; k++) a.cand[12 * INIT_MAX_CAND * (size_t)p + k] = cand[k];
    }
}

// the mask of the chosen model's best hypothesis (model != INIT_MODEL_NONE)
HD const uint32_t *init_chosen_mask(const InitProblem &P, int p, const InitArrays &a) {
    const int model = a.model[p];
    return a.mask + (size_t)model * a.words + P.w0 + (size_t)a.best[2 * p + model] * ransac_words(P.N);
}

// CheckRT for correspondence i under a candidate's camera
HD int init_check_rt_corr(const InitProblem &P, const InitArrays &a, const InitCam &cam, int i, float *p3d, float *cosParallax) {
    const int *mt = a.matches + 2 * (size_t)(P.c0 + i);
    const float *k1 = a.keys1 + 2 * (size_t)(P.k1 + mt[0]), *k2 = a.keys2 + 2 * (size_t)(P.k2 + mt[1]);
    return im_check_point(cam, k1[0], k1[1], k2[0], k2[1], p3d, cosParallax);
}
// where candidate c of problem p keeps its mask, its points and its list of cosines
HD uint32_t *init_cand_mask(const InitProblem &P, const InitArrays &a, int c) { return a.good_mask + P.cw0 + (size_t)c * ransac_words(P.N); }
HD float *init_cand_points(const InitProblem &P, const InitArrays &a, int c) { return a.points + 3 * ((size_t)INIT_MAX_CAND * P.c0 + (size_t)c * P.N); }
HD float *init_cand_cos_list(const InitProblem &P, const InitArrays &a, int c) { return a.cos_list + (size_t)INIT_MAX_CAND * P.c0 + (size_t)c * P.N; }

// ---- the host evaluation of the same text.  The caller has zeroed good_mask, points, nGood, cosp and n_inliers
inline void init_host_evaluate(const std::vector<InitProblem> &problems, const InitArrays &a) {
    const CvxSeq x;
    InitSvdWork w;
    for (size_t pp = 0; pp < problems.size(); pp++) {
        const InitProblem &P = problems[pp];
        const int p = (int)pp, W = ransac_words(P.N);
        for (int image = 0; image < 2; image++) {
            const float *keys = image ? a.keys2 + 2 * (size_t)P.k2 : a.keys1 + 2 * (size_t)P.k1;
            float *pn = image ? a.pn2 + 2 * (size_t)P.k2 : a.pn1 + 2 * (size_t)P.k1;
            const int n = image ? P.n2 : P.n1;
            const InitNorm nm = im_normalize_sums(keys, n);
            for (int i = 0; i < n; i++) im_normalize_point(nm, keys + 2 * i, pn + 2 * i);
            init_normalize_matrices(nm, image, P, p, a);
        }
        const float invSigmaSquare = im_inv_sigma_square(P.sigma);
        float S[2];
        int best2[2];
        for (int model = 0; model < 2; model++) {
            float best_score = 0.f; // :144 / :194
            int best = -1;
            for (int h = P.h0; h < P.h0 + P.nh; h++) {
                float M[9], Minv[9] = {0};
                init_hypothesis(x, P, p, h, model, a, &w, M, Minv);
                float score = 0;
                int count;
                ransac_host_inliers(P.N, [&](int i) {
                    float t1, t2;
                    const bool in = init_check_corr(P, a, model, M, Minv, invSigmaSquare, i, &t1, &t2);
                    score = im_score_add(score, t1, t2);
                    return in;
                }, a.mask + (size_t)model * a.words + P.w0 + (size_t)(h - P.h0) * W, &count);
                const size_t hm = (size_t)model * a.H + h;
                a.score[hm] = score;
                for (int k = 0; k < 9; k++) a.matrix[9 * hm + k] = M[k];
                if (score > best_score) { best_score = score; best = h - P.h0; } // :172 / :222
            }
            S[model] = best_score; best2[model] = best;
        }
        init_choose(x, P, p, a, &w, S[0], S[1], best2[0], best2[1]);
        if (a.model[p] == INIT_MODEL_NONE) continue;
        const uint32_t *m = init_chosen_mask(P, p, a);
        int N = 0;
        for (int i = 0; i < P.N; i++) N += ransac_mask_bit(m, i) ? 1 : 0;
        a.n_inliers[p] = N;
        for (int c = 0; c < a.n_cand[p]; c++) {
            InitCam cam;
            im_make_cam(P.K, a.cand + 12 * ((size_t)INIT_MAX_CAND * p + c), P.sigma, &cam);
            uint32_t *gm = init_cand_mask(P, a, c);
            float *pts = init_cand_points(P, a, c), *list = init_cand_cos_list(P, a, c);
            int nGood = 0;
            for (int i = 0; i < P.N; i++) {
                if (!ransac_mask_bit(m, i)) continue;
                float p3d[3], cosParallax;
                const int st = init_check_rt_corr(P, a, cam, i, p3d, &cosParallax);
                if (st == IM_SKIPPED) continue;
                list[nGood++] = cosParallax;
                for (int k = 0; k < 3; k++) pts[3 * (size_t)i + k] = p3d[k];
                if (st == IM_GOOD) gm[i >> 5] |= 1u << (i & 31);
            }
            a.nGood[INIT_MAX_CAND * p + c] = nGood;
            if (nGood > 0) im_cos_select(x, list, nGood, std::min(50, nGood - 1), a.cosp + INIT_MAX_CAND * p + c); // :902-905
        }
    }
}

// the caller's output arrays of cs_initializer_evaluate, in the order of its arguments
struct InitOutputs {
    float *score, *matrix; uint32_t *mask;
    int *model, *best; float *S, *RH; int *n_inliers, *n_cand; float *cand_Rt; int *nGood; float *cos_parallax;
    uint32_t *good_mask; float *points;
};

// the host evaluation into the caller's arrays, with the intermediate ones of its own
inline void init_host_run(const std::vector<InitProblem> &problems, const float *keys1, const float *keys2, const int *matches, const int *sets, int H, long words, long cwords,
                          int NK1, int NK2, int NC, const InitOutputs &o) {
    const size_t np = problems.size();
    std::vector<float> pn1(2 * (size_t)NK1 + 1), pn2(2 * (size_t)NK2 + 1), T(27 * np + 1), cos_list((size_t)INIT_MAX_CAND * NC + 1);
    for (long k = 0; k < cwords; k++) o.good_mask[k] = 0;
    for (size_t k = 0; k < 3 * (size_t)INIT_MAX_CAND * NC; k++) o.points[k] = 0.f;
    for (size_t k = 0; k < INIT_MAX_CAND * np; k++) { o.nGood[k] = 0; o.cos_parallax[k] = 0.f; }
    for (size_t k = 0; k < np; k++) o.n_inliers[k] = 0;
    const InitArrays a{keys1, keys2, matches, sets, pn1.data(), pn2.data(), T.data(), T.data() + 9 * np, T.data() + 18 * np, H, words, o.score, o.matrix, o.mask,
                       o.model, o.best, o.n_inliers, o.n_cand, o.nGood, o.S, o.RH, o.cand_Rt, o.cos_parallax, o.points, cos_list.data(), o.good_mask};
    init_host_evaluate(problems, a);
}

// ---- the checks of cs_initializer_evaluate and its records: nullptr, or what is wrong (ransac_batch_build<8>); nothing is written to the caller's arrays
inline const char *init_build(int n_problems, const int *key1_off, const float *keys1, const int *key2_off, const float *keys2, const int *corr_off, const int *matches,
                              const float *K9, const float *sigma, const int *hyp_off, const int *sets, bool have_outputs, std::vector<InitProblem> &problems,
                              std::vector<int> &hyp_problem, long *words_out, long *cand_words_out, long at[2]) {
    std::vector<RansacSlot> slots;
    if (const char *what = ransac_batch_build<8>(n_problems, corr_off, hyp_off, sets, K9 && sigma && key1_off && key2_off, matches != nullptr, have_outputs, slots, hyp_problem,
                                                 words_out, at))
        return what;
    problems.resize(slots.size());
    *cand_words_out = 0;
    if (n_problems == 0) return nullptr;
    if (key1_off[0] != 0 || key2_off[0] != 0) return "key-point offsets that do not start at 0";
    for (int p = 0; p < n_problems; p++)
        if (key1_off[p + 1] < key1_off[p] || key2_off[p + 1] < key2_off[p]) return "key-point offsets that decrease";
    if ((key1_off[n_problems] && !keys1) || (key2_off[n_problems] && !keys2)) return "NULL argument";
    long cw = 0;
    for (size_t p = 0; p < slots.size(); p++) {
        const RansacSlot &s = slots[p];
        InitProblem &P = problems[p];
        P.k1 = key1_off[p]; P.n1 = key1_off[p + 1] - key1_off[p]; P.k2 = key2_off[p]; P.n2 = key2_off[p + 1] - key2_off[p];
        P.c0 = s.c0; P.N = s.N; P.h0 = s.h0; P.nh = s.nh; P.w0 = s.w0; P.cw0 = cw;
        for (int k = 0; k < 9; k++) P.K[k] = K9[9 * p + k];
        P.sigma = sigma[p];
        for (int i = 0; i < s.N; i++) {
            const int *mt = matches + 2 * (size_t)(s.c0 + i);
            if (mt[0] < 0 || mt[0] >= P.n1 || mt[1] < 0 || mt[1] >= P.n2) { at[0] = (long)p; at[1] = i; return "a match outside the key points of its frame (problem, match)"; }
        }
        cw += (long)INIT_MAX_CAND * ransac_words(s.N);
    }
    *cand_words_out = cw;
    return nullptr;
}
