// ransac_batch.h -- what the batched RANSACs of the library share (sim3solver.hip over sim3_host.h, pnpsolver.hip over pnp_host.h, initializer.hip over initializer_host.h, and
// their mirrors under host/): a CSR batch
// of problems (corr_off, hyp_off) whose minimal sets of K indices are input, one mask of ceil(N / 32) words per hypothesis, and the rules that need no arithmetic of a
// hypothesis.  Nothing here knows a solver.  Plain C++ for the g++ builds of the mirrors and the tests; the wave's part and the error text of an entry point under hipcc.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hd.h"
#if defined(__HIPCC__)
#include "common.h"
#endif

// ---- the mask of a hypothesis: correspondence i is bit i & 31 of word i >> 5, ransac_words(N) words, the bits from N up 0
HD int ransac_words(int N) { return (N + 31) >> 5; }
HD bool ransac_mask_bit(const uint32_t *m, int i) { return (m[i >> 5] >> (i & 31)) & 1u; }

// pred(i) over i ascending on one thread -> the mask and the count
template <class Pred> inline void ransac_host_inliers(int N, Pred pred, uint32_t *m, int *count) {
    for (int w = 0; w < ransac_words(N); w++) m[w] = 0;
    int c = 0;
    for (int i = 0; i < N; i++)
        if (pred(i)) { m[i >> 5] |= 1u << (i & 31); c++; }
    *count = c;
}

#if defined(__HIPCC__)
// pred(i) with the N correspondences strided over the 64 lanes of a wave: the mask words are the two halves of __ballot, the count its popcount, returned to every lane.
// after_chunk(base), where given, is called by every lane after the 64 correspondences from base: for what a solver accumulates in their order (Initializer's score)
template <class Pred, class Chunk> __device__ __forceinline__ int ransac_wave_inliers(int N, int lane, Pred pred, uint32_t *m, Chunk after_chunk) {
    const int W = ransac_words(N);
    int count = 0;
    for (int base = 0; base < N; base += 64) { // (wave-uniform trip count: every lane reaches the ballot)
        const int i = base + lane;
        bool in = false;
        if (i < N) in = pred(i);
        const unsigned long long bal = __ballot(in);
        count += __popcll(bal);
        if (lane == 0) {
            m[base >> 5] = (uint32_t)bal;
            if ((base >> 5) + 1 < W) m[(base >> 5) + 1] = (uint32_t)(bal >> 32);
        }
        after_chunk(base);
    }
    return count;
}
template <class Pred> __device__ __forceinline__ int ransac_wave_inliers(int N, int lane, Pred pred, uint32_t *m) {
    return ransac_wave_inliers(N, lane, pred, m, [](int) {});
}
#endif

// ---- the batch.  One problem's place in the flat arrays: first correspondence, their number, first hypothesis, their number, first mask word
struct RansacSlot { int c0, N, h0, nh; long w0; };

// The checks every entry point makes before it writes or launches anything, and the slots: nullptr, or what is wrong (at[] = the problem and hypothesis it is wrong at, -1
// where there is none).  sets: K indices per hypothesis.  have_problem_arrays / have_corr_arrays / have_outputs: the solver's own per-problem arrays, per-correspondence arrays
// and output arrays are all given; the second is asked for only where there are correspondences, the third and sets only where there are hypotheses.
template <int K> inline const char *ransac_batch_build(int n_problems, const int *corr_off, const int *hyp_off, const int *sets, bool have_problem_arrays, bool have_corr_arrays,
                                                       bool have_outputs, std::vector<RansacSlot> &slots, std::vector<int> &hyp_problem, long *words_out, long at[2]) {
    static_assert(K == 3 || K == 4 || K == 8, "triples, quads or sets of eight");
    at[0] = at[1] = -1;
    slots.clear(); hyp_problem.clear(); *words_out = 0;
    if (n_problems < 0) return "n_problems < 0";
    if (n_problems == 0) return nullptr;
    if (!corr_off || !hyp_off || corr_off[0] != 0 || hyp_off[0] != 0) return "offsets that do not start at 0, or a NULL array";
    for (int p = 0; p < n_problems; p++)
        if (corr_off[p + 1] < corr_off[p] || hyp_off[p + 1] < hyp_off[p]) return "offsets that decrease";
    const int NC = corr_off[n_problems], H = hyp_off[n_problems];
    if (!have_problem_arrays || (NC && !have_corr_arrays) || (H && (!sets || !have_outputs))) return "NULL argument";
    slots.resize((size_t)n_problems);
    hyp_problem.resize((size_t)H);
    long words = 0;
    for (int p = 0; p < n_problems; p++) {
        const int N = corr_off[p + 1] - corr_off[p], nh = hyp_off[p + 1] - hyp_off[p];
        at[0] = p;
        if (nh && N < K)
            return K == 3 ? "a problem with hypotheses and fewer than 3 correspondences"
                 : K == 4 ? "a problem with hypotheses and fewer than 4 correspondences" : "a problem with hypotheses and fewer than 8 correspondences";
        for (int h = hyp_off[p]; h < hyp_off[p + 1]; h++) {
            const int *s = sets + K * (size_t)h;
            at[1] = h;
            for (int k = 0; k < K; k++) {
                if (s[k] < 0 || s[k] >= N) return K == 3 ? "a triple index outside its problem (problem, hypothesis)"
                         : K == 4 ? "a quad index outside its problem (problem, hypothesis)" : "a set index outside its problem (problem, hypothesis)";
                for (int l = 0; l < k; l++)
                    if (s[l] == s[k])
                        return K == 3 ? "two equal indices in a triple (problem, hypothesis)"
                             : K == 4 ? "two equal indices in a quad (problem, hypothesis)" : "two equal indices in a set of eight (problem, hypothesis)";
            }
            hyp_problem[h] = p;
        }
        at[1] = -1;
        slots[p] = RansacSlot{corr_off[p], N, hyp_off[p], nh, words};
        words += (long)nh * ransac_words(N);
    }
    at[0] = -1;
    *words_out = words;
    return nullptr;
}

#if defined(__HIPCC__)
// what an entry point answers to a refusal of its build: the text in the context, if there is one
inline int ransac_bad(cs_ctx *ctx, const char *fn_name, const char *what, long a, long b) {
    if (!ctx) return CS_ERR_BAD_ARG;
    char buf[256];
    if (a >= 0 && b >= 0) snprintf(buf, sizeof buf, "%s: %s (%ld, %ld)", fn_name, what, a, b);
    else if (a >= 0) snprintf(buf, sizeof buf, "%s: %s (%ld)", fn_name, what, a);
    else snprintf(buf, sizeof buf, "%s: %s", fn_name, what);
    ctx->err = buf;
    return CS_ERR_BAD_ARG;
}
#endif

// ---- the rules without arithmetic of a hypothesis
// The iterations that reach `probability` at an inlier ratio epsilon with minimal sets of three (both SetRansacParameters write the 3), within 1..max_iterations.
// (pow(float, int) is the double pow.)  Where the quotient does not fit an int -- pow() below 2^-53, where log(1 - 0) = +0 makes it -inf -- or is a NaN (epsilon > 1), the
// reference's conversion is undefined (x86 yields INT_MIN, hence one iteration); the library takes the bound: max_iterations
inline int ransac_iterations(double probability, float epsilon, int max_iterations) {
    const double q = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0)));
    const int nIterations = (q > -2147483648.0 && q < 2147483648.0) ? (int)q : max_iterations;
    return std::max(1, std::min(nIterations, max_iterations));
}

// `count` minimal sets of K distinct indices below N appended to out: the reference's partial Fisher-Yates over RandomInt(min, max), K calls per set
template <int K, class RandomInt> inline void ransac_draw(int N, int count, RandomInt &&random_int, std::vector<int> &out) {
    for (int it = 0; it < count; it++) {
        std::vector<int> vAvailableIndices((size_t)N);
        for (int i = 0; i < N; i++) vAvailableIndices[i] = i;
        for (short i = 0; i < K; ++i) {
            const int randi = random_int(0, (int)vAvailableIndices.size() - 1);
            out.push_back(vAvailableIndices[randi]);
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }
}
