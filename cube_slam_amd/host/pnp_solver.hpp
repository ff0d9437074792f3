// pnp_solver.hpp -- ORB_SLAM2::PnPsolver (orb_object_slam/src/PnPsolver.cc), the RANSAC over EPnP of Tracking::Relocalization (Tracking.cc:2876-3030), with the reference's
// member names over the C-ABI (include/cubeslam_hip.h) and plain arrays:
//   cubeslam::PnPsolver::evaluate_many    the hypotheses not yet evaluated of all candidates of one Relocalization, and their distinct refinements, in one
//                                         cs_pnp_solver_evaluate call
//   iterate / find                        the reference's sequential rule (:164-256) walked over the two tables of counts (pnp_walk.h, what cs_pnp_solver_walk runs)
//   draw_quads                            the partial Fisher-Yates of :187-200 over a caller's RandomInt(min, max), which is kept for the quads a later iterate() reads past the
//                                         table (:181 runs past mRansacMaxIts after a success); or set_quads with a table
// The constructor's filter (:79-101) stays the caller's: the solver is built over its results (INTEGRATION.md 8b'').  Without a context (ctx == nullptr) the tables are
// evaluated on the host over the text the kernels run (csrc/epnp_math.h, csrc/cv_svd_math.h; compile with -ffp-contract=off), byte-equal to the device: the comparison side of
// tests and bench.  With CUBESLAM_HOST_ONLY defined the header needs neither the library nor a context type.
#pragma once
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/pnp_host.h"
#include "../csrc/pnp_walk.h"
#ifndef CUBESLAM_HOST_ONLY
#include "../../include/cubeslam_hip.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context
#else
namespace cubeslam { struct Context; }
#endif

namespace cubeslam {

class PnPsolver {
  public:
    struct Result { bool found = false; float Tcw[16] = {0}; bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = 0; }; // found == false: cv::Mat()

    // P3Dw: 3 floats per correspondence (mvP3Dw); P2D: 2 (mvP2D); sigma2 = mvSigma2; K = fu fv uc vc; n_matches = mvpMapPointMatches.size()
    PnPsolver(std::vector<float> P3Dw, std::vector<float> P2D, std::vector<float> sigma2, const float K[4], std::vector<int> mvKeyPointIndices_, int n_matches_, Context *ctx = nullptr)
        : mvP3Dw(std::move(P3Dw)), mvP2D(std::move(P2D)), mvSigma2(std::move(sigma2)), mvKeyPointIndices(std::move(mvKeyPointIndices_)), n_matches(n_matches_), ctx_(ctx) {
        N = (int)mvSigma2.size();
        if (mvP3Dw.size() != 3 * (size_t)N || mvP2D.size() != 2 * (size_t)N || mvKeyPointIndices.size() != (size_t)N) throw std::invalid_argument("PnPsolver: one entry per correspondence in every array");
        for (int i : mvKeyPointIndices) if (i < 0 || i >= n_matches) throw std::invalid_argument("PnPsolver: mvKeyPointIndices outside 0..n_matches - 1");
        for (int k = 0; k < 4; k++) K4[k] = K[k];
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991) {
        if (minSet != 4) throw std::invalid_argument("PnPsolver: EPnP hypotheses are drawn from 4 correspondences (minSet == 4)");
        mRansacProb = probability; mRansacMinSet = minSet;
        pnp_ransac_parameters(probability, minInliers, maxIterations, minSet, epsilon, N, &mRansacMinInliers, &mRansacMaxIts, &mRansacEpsilon);
        mvMaxError.resize((size_t)N);
        for (int i = 0; i < N; i++) mvMaxError[i] = mvSigma2[i] * th2; // :155
        mnIterations = 0; mnBestInliers = 0; best_ = -1;
        quads.clear(); clear_tables();
    }

    bool live() const { return N >= mRansacMinInliers && N >= 4; } // (:172)
    void set_quads(std::vector<int> q) { // 4 per iteration, in drawing order: at least mRansacMaxIts of them
        if (q.size() % 4 || (live() && q.size() < 4 * (size_t)mRansacMaxIts)) throw std::invalid_argument("PnPsolver: set_quads wants 4 indices for at least mRansacMaxIts iterations");
        quads = std::move(q); clear_tables();
    }
    void draw_quads(std::function<int(int, int)> RandomInt, int extra = 5) {
        random_int_ = std::move(RandomInt);
        std::vector<int> q;
        if (live()) ransac_draw<4>(N, mRansacMaxIts + extra, random_int_, q);
        set_quads(std::move(q));
    }

    // the tables of all solvers in one call: on the device of ctx, or on the host without one
    static void evaluate_many(const std::vector<PnPsolver *> &solvers, Context *ctx) {
        std::vector<int> corr_off{0}, hyp_off{0}, q, mi, bi;
        std::vector<float> X, U, E, K;
        for (const PnPsolver *s : solvers) {
            const size_t done = s->n_inliers.size();
            corr_off.push_back(corr_off.back() + s->N);
            hyp_off.push_back(hyp_off.back() + (s->live() ? (int)(s->quads.size() / 4 - done) : 0));
            X.insert(X.end(), s->mvP3Dw.begin(), s->mvP3Dw.end()); U.insert(U.end(), s->mvP2D.begin(), s->mvP2D.end()); E.insert(E.end(), s->mvMaxError.begin(), s->mvMaxError.end());
            K.insert(K.end(), s->K4, s->K4 + 4); mi.push_back(s->mRansacMinInliers);
            int best = 0;
            for (int c : s->n_inliers) if (c >= s->mRansacMinInliers && c > best) best = c;
            bi.push_back(best);
            if (s->live()) q.insert(q.end(), s->quads.begin() + 4 * done, s->quads.end());
        }
        const int H = hyp_off.back();
        if (H == 0) return;
        std::vector<PnpProblem> problems;
        std::vector<PnpCorr> corr;
        std::vector<int> hyp_problem;
        long words = 0, sdoubles = 0, at[2];
        const char *what = pnp_build((int)solvers.size(), corr_off.data(), X.data(), U.data(), E.data(), K.data(), mi.data(), bi.data(), hyp_off.data(), q.data(), true, problems, corr,
                                     hyp_problem, &words, &sdoubles, at);
        if (what) throw std::invalid_argument(std::string("PnPsolver: ") + what);
        std::vector<int> ni((size_t)H), rn((size_t)H);
        std::vector<double> Rt(12 * (size_t)H), rRt(12 * (size_t)H, 0.0);
        std::vector<uint32_t> st((size_t)H), mask((size_t)words), rmask((size_t)words, 0u);
        if (ctx) {
#ifndef CUBESLAM_HOST_ONLY
            const int r = cs_pnp_solver_evaluate(ctx->ctx, (int)solvers.size(), corr_off.data(), X.data(), U.data(), E.data(), K.data(), mi.data(), bi.data(), hyp_off.data(), q.data(),
                                                 ni.data(), Rt.data(), st.data(), mask.data(), rn.data(), rRt.data(), rmask.data());
            if (r != CS_OK) throw std::runtime_error("cs_pnp_solver_evaluate failed (" + std::to_string(r) + "): " + cs_last_error(ctx->ctx));
#else
            throw std::runtime_error("PnPsolver: built without the library");
#endif
        } else
            pnp_host_evaluate(problems, corr, q.data(), ni.data(), Rt.data(), st.data(), mask.data(), rn.data(), rRt.data(), rmask.data());
        for (size_t p = 0; p < solvers.size(); p++) {
            PnPsolver *s = solvers[p];
            const long W = ransac_words(s->N), w0 = problems[p].w0, nh = hyp_off[p + 1] - hyp_off[p];
            s->n_inliers.insert(s->n_inliers.end(), ni.begin() + hyp_off[p], ni.begin() + hyp_off[p + 1]);
            s->refined_n.insert(s->refined_n.end(), rn.begin() + hyp_off[p], rn.begin() + hyp_off[p + 1]);
            s->status.insert(s->status.end(), st.begin() + hyp_off[p], st.begin() + hyp_off[p + 1]);
            s->Rt.insert(s->Rt.end(), Rt.begin() + 12 * (size_t)hyp_off[p], Rt.begin() + 12 * (size_t)hyp_off[p + 1]);
            s->refined_Rt.insert(s->refined_Rt.end(), rRt.begin() + 12 * (size_t)hyp_off[p], rRt.begin() + 12 * (size_t)hyp_off[p + 1]);
            s->inlier_mask.insert(s->inlier_mask.end(), mask.begin() + w0, mask.begin() + w0 + nh * W);
            s->refined_mask.insert(s->refined_mask.end(), rmask.begin() + w0, rmask.begin() + w0 + nh * W);
        }
    }

    Result iterate(int nIterations) {
        Result r;
        r.vbInliers.assign((size_t)n_matches, false);
        if (N < mRansacMinInliers) { r.bNoMore = true; return r; } // :172
        int left = nIterations, t, nomore = 0, refined = 0;
        for (;;) {
            if (n_inliers.size() < quads.size() / 4) evaluate_many({this}, ctx_);
            const int before = mnIterations;
            t = pnp_walk(n_inliers.data(), refined_n.data(), (int)n_inliers.size(), mRansacMaxIts, mRansacMinInliers, &mnIterations, &mnBestInliers, &best_, left, &nomore, &refined);
            if (t != -2) break;
            if (!random_int_) throw std::runtime_error("PnPsolver: iterate() reads past the table of quads (:181 runs past mRansacMaxIts after a success)");
            left -= mnIterations - before;
            ransac_draw<4>(N, 5, random_int_, quads);
        }
        r.bNoMore = nomore != 0;
        if (t < 0) return r;
        r.found = true;
        const uint32_t *m = (refined ? refined_mask.data() : inlier_mask.data()) + (size_t)t * ransac_words(N);
        const double *p = (refined ? refined_Rt.data() : Rt.data()) + 12 * (size_t)t;
        r.nInliers = refined ? refined_n[t] : n_inliers[t];
        for (int i = 0; i < N; i++) if (ransac_mask_bit(m, i)) r.vbInliers[mvKeyPointIndices[i]] = true;
        for (int k = 0; k < 16; k++) r.Tcw[k] = (k % 5 == 0) ? 1.f : 0.f; // :216-222 / :292-298
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) r.Tcw[4 * a + b] = (float)p[3 * a + b];
            r.Tcw[4 * a + 3] = (float)p[9 + a];
        }
        return r;
    }
    Result find() { return iterate(mRansacMaxIts); }

    std::vector<float> mvP3Dw, mvP2D, mvSigma2, mvMaxError;
    std::vector<int> mvKeyPointIndices;
    int N = 0, n_matches = 0;
    float K4[4];
    double mRansacProb = 0.99;
    int mRansacMinInliers = 8, mRansacMaxIts = 300, mRansacMinSet = 4, mnIterations = 0, mnBestInliers = 0;
    float mRansacEpsilon = 0.4f;
    std::vector<int> quads;
    std::vector<int> n_inliers, refined_n;           // per hypothesis
    std::vector<uint32_t> status;
    std::vector<double> Rt, refined_Rt;              // 12 per hypothesis: mRi row-major, mti
    std::vector<uint32_t> inlier_mask, refined_mask; // (N + 31) / 32 words per hypothesis

  private:
    Context *ctx_;
    int best_ = -1;
    std::function<int(int, int)> random_int_;
    void clear_tables() { n_inliers.clear(); refined_n.clear(); status.clear(); Rt.clear(); refined_Rt.clear(); inlier_mask.clear(); refined_mask.clear(); }
};

} // namespace cubeslam
