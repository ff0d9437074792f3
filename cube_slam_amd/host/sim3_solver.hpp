// sim3_solver.hpp -- ORB_SLAM2::Sim3Solver (orb_object_slam/src/Sim3Solver.cc), the RANSAC of LoopClosing::ComputeSim3 (LoopClosing.cc:231-342), with the reference's member
// names over the C-ABI (include/cubeslam_hip.h) and plain arrays:
//   cubeslam::Sim3Solver::evaluate_many   the hypotheses of all candidates of one ComputeSim3 in one cs_sim3_solver_hypotheses call
//   iterate / find                        the reference's sequential rule (:138-205) walked over the table of counts (s3s_walk, what cs_sim3_solver_walk runs)
//   draw_triples                          the partial Fisher-Yates of :161-175 over a caller's RandomInt(min, max); or set_triples with a table
// The constructor's filter (:60-101) stays the caller's: the solver is built over its results (INTEGRATION.md 8b').  Without a context (ctx == nullptr) the tables are evaluated
// on the host by s3s_host_evaluate (csrc/sim3_host.h, the library's own path without a context; compile with -ffp-contract=off), byte-equal to the device: the comparison side
// of tests and bench.  With CUBESLAM_HOST_ONLY defined the header needs neither the library nor a context type.
#pragma once
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/sim3_host.h"
#ifndef CUBESLAM_HOST_ONLY
#include "../../include/cubeslam_hip.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context
#else
namespace cubeslam { struct Context; }
#endif

namespace cubeslam {

class Sim3Solver {
  public:
    struct Result { bool found = false; float T12[16] = {0}; bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = 0; }; // found == false: cv::Mat()

    // X3Dc1 / X3Dc2: 3 floats per correspondence (mvX3Dc1 / mvX3Dc2); max_err1 / 2 = mvnMaxError1 / 2; K1 / K2 = fx fy cx cy of mK1 / mK2
    Sim3Solver(std::vector<float> X3Dc1, std::vector<float> X3Dc2, std::vector<float> max_err1, std::vector<float> max_err2, const float K1[4], const float K2[4],
               std::vector<int> mvnIndices1_, int mN1_, bool bFixScale = false, Context *ctx = nullptr)
        : mvX3Dc1(std::move(X3Dc1)), mvX3Dc2(std::move(X3Dc2)), mvnMaxError1(std::move(max_err1)), mvnMaxError2(std::move(max_err2)), mvnIndices1(std::move(mvnIndices1_)),
          mN1(mN1_), mbFixScale(bFixScale), ctx_(ctx) {
        N = (int)mvnMaxError1.size();
        if (mvX3Dc1.size() != 3 * (size_t)N || mvX3Dc2.size() != 3 * (size_t)N || mvnMaxError2.size() != (size_t)N || mvnIndices1.size() != (size_t)N)
            throw std::invalid_argument("Sim3Solver: one entry per correspondence in every array");
        for (int i : mvnIndices1) if (i < 0 || i >= mN1) throw std::invalid_argument("Sim3Solver: mvnIndices1 outside 0..mN1 - 1");
        for (int k = 0; k < 4; k++) { K8[k] = K1[k]; K8[4 + k] = K2[k]; }
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability; mRansacMinInliers = minInliers;
        mRansacMaxIts = s3s_max_iterations(probability, minInliers, maxIterations, N);
        mnIterations = 0;
        triples.clear(); evaluated_ = false;
    }

    void set_triples(std::vector<int> t) { // 3 per iteration, in drawing order
        if (t.size() != 3 * (size_t)mRansacMaxIts) throw std::invalid_argument("Sim3Solver: set_triples wants 3 * mRansacMaxIts indices");
        triples = std::move(t); evaluated_ = false;
    }
    void draw_triples(const std::function<int(int, int)> &RandomInt) { // :161-175 for every iteration
        std::vector<int> t;
        ransac_draw<3>(N, mRansacMaxIts, RandomInt, t);
        set_triples(std::move(t));
    }

    // the tables of all solvers in one call: on the device of ctx, or on the host without one
    static void evaluate_many(const std::vector<Sim3Solver *> &solvers, Context *ctx) {
        std::vector<int> corr_off{0}, hyp_off{0}, tri;
        std::vector<float> X1, X2, e1, e2, K;
        std::vector<uint8_t> fix;
        for (const Sim3Solver *s : solvers) {
            if (s->mRansacMaxIts && s->triples.empty()) throw std::runtime_error("Sim3Solver: no triples (set_triples or draw_triples)");
            corr_off.push_back(corr_off.back() + s->N); hyp_off.push_back(hyp_off.back() + s->mRansacMaxIts);
            X1.insert(X1.end(), s->mvX3Dc1.begin(), s->mvX3Dc1.end()); X2.insert(X2.end(), s->mvX3Dc2.begin(), s->mvX3Dc2.end());
            e1.insert(e1.end(), s->mvnMaxError1.begin(), s->mvnMaxError1.end()); e2.insert(e2.end(), s->mvnMaxError2.begin(), s->mvnMaxError2.end());
            K.insert(K.end(), s->K8, s->K8 + 8); fix.push_back(s->mbFixScale);
            tri.insert(tri.end(), s->triples.begin(), s->triples.end());
        }
        std::vector<S3sProblem> problems;
        std::vector<S3sCorr> corr;
        std::vector<int> hyp_problem;
        long words = 0, at[2];
        const char *what = s3s_build((int)solvers.size(), corr_off.data(), X1.data(), X2.data(), e1.data(), e2.data(), K.data(), fix.data(), hyp_off.data(), tri.data(), true, problems,
                                     corr, hyp_problem, &words, at);
        if (what) throw std::invalid_argument(std::string("Sim3Solver: ") + what);
        const int H = hyp_off.back();
        std::vector<int> ni((size_t)H);
        std::vector<float> sRt(13 * (size_t)H);
        std::vector<uint32_t> mask((size_t)words);
        if (ctx) {
#ifndef CUBESLAM_HOST_ONLY
            const int r = cs_sim3_solver_hypotheses(ctx->ctx, (int)solvers.size(), corr_off.data(), X1.data(), X2.data(), e1.data(), e2.data(), K.data(), fix.data(), hyp_off.data(),
                                                    tri.data(), ni.data(), sRt.data(), mask.data());
            if (r != CS_OK) throw std::runtime_error("cs_sim3_solver_hypotheses failed (" + std::to_string(r) + "): " + cs_last_error(ctx->ctx));
#else
            throw std::runtime_error("Sim3Solver: built without the library");
#endif
        } else
            s3s_host_evaluate(problems, hyp_problem, corr, tri.data(), ni.data(), sRt.data(), mask.data());
        for (size_t p = 0; p < solvers.size(); p++) {
            Sim3Solver *s = solvers[p];
            const long w0 = problems[p].w0, nw = (long)s->mRansacMaxIts * ransac_words(s->N);
            s->n_inliers.assign(ni.begin() + hyp_off[p], ni.begin() + hyp_off[p + 1]);
            s->sRt.assign(sRt.begin() + 13 * (size_t)hyp_off[p], sRt.begin() + 13 * (size_t)hyp_off[p + 1]);
            s->inlier_mask.assign(mask.begin() + w0, mask.begin() + w0 + nw);
            s->evaluated_ = true;
        }
    }

    Result iterate(int nIterations) {
        Result r;
        r.vbInliers.assign((size_t)mN1, false);
        if (N < mRansacMinInliers) { r.bNoMore = true; return r; } // :144
        if (!evaluated_) evaluate_many({this}, ctx_);
        int nomore = 0;
        const int t = s3s_walk(n_inliers.data(), mRansacMaxIts, mRansacMinInliers, &mnIterations, &mnBestInliers, &best_, nIterations, &nomore);
        r.bNoMore = nomore != 0;
        if (t < 0) return r;
        r.found = true; r.nInliers = n_inliers[t];
        const uint32_t *m = &inlier_mask[(size_t)t * ransac_words(N)];
        for (int i = 0; i < N; i++) if (ransac_mask_bit(m, i)) r.vbInliers[mvnIndices1[i]] = true;
        const float *h = &sRt[13 * (size_t)t];
        for (int k = 0; k < 16; k++) r.T12[k] = (k % 5 == 0) ? 1.f : 0.f;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) r.T12[4 * a + b] = (float)((double)h[1 + 3 * a + b] * (double)h[0]); // sR = ms12i * mR12i
            r.T12[4 * a + 3] = h[10 + a];
        }
        return r;
    }
    Result find() { return iterate(mRansacMaxIts); }

    const float *GetEstimatedRotation() const { return &sRt[13 * (size_t)checked_best() + 1]; } // 9 floats, row-major
    const float *GetEstimatedTranslation() const { return &sRt[13 * (size_t)checked_best() + 10]; }
    float GetEstimatedScale() const { return sRt[13 * (size_t)checked_best()]; }

    std::vector<float> mvX3Dc1, mvX3Dc2, mvnMaxError1, mvnMaxError2;
    std::vector<int> mvnIndices1;
    int N = 0, mN1 = 0;
    bool mbFixScale = false;
    float K8[8];
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300, mnIterations = 0, mnBestInliers = 0;
    std::vector<int> triples;
    std::vector<int> n_inliers;          // per hypothesis
    std::vector<float> sRt;              // 13 per hypothesis: ms12i, mR12i, mt12i
    std::vector<uint32_t> inlier_mask;   // (N + 31) / 32 words per hypothesis

  private:
    Context *ctx_;
    bool evaluated_ = false;
    int best_ = -1;
    int checked_best() const { if (best_ < 0 || !evaluated_) throw std::runtime_error("Sim3Solver: no best hypothesis yet"); return best_; }
};

} // namespace cubeslam
