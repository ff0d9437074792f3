// initializer.hpp -- ORB_SLAM2::Initializer (orb_object_slam/src/Initializer.cc), the two-view initialisation of Tracking::MonocularInitialization (Tracking.cc:948-983), with
// the reference's member names over the C-ABI (include/cubeslam_hip.h) and plain arrays:
//   cubeslam::Initializer::evaluate_many   the 2 x mMaxIterations hypotheses of every prepared frame pair, the choice of the model and the CheckRT passes of its candidates in
//                                          one cs_initializer_evaluate call
//   Initialize / result                    the decisions of ReconstructF / ReconstructH walked over the candidates' counts (initializer_walk.h, what cs_initializer_walk runs)
//   draw_sets                              the partial Fisher-Yates of :83-98 over a caller's RandomInt(min, max) (the reference seeds DUtils::Random once per process and every
//                                          Initialize continues the stream: the caller's function carries that state); or set_sets with a table
// Without a context (ctx == nullptr) the tables are evaluated on the host over the text the kernels run (csrc/initializer_math.h; compile with -ffp-contract=off), byte-equal to
// the device: the comparison side of tests and bench.  With CUBESLAM_HOST_ONLY defined the header needs neither the library nor a context type.
#pragma once
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/initializer_host.h"
#ifndef CUBESLAM_HOST_ONLY
#include "../../include/cubeslam_hip.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context
#else
namespace cubeslam { struct Context; }
#endif

namespace cubeslam {

class Initializer {
  public:
    struct Result { bool success = false; float R21[9] = {0}, t21[3] = {0}; std::vector<float> vP3D; std::vector<bool> vbTriangulated; float parallax = 0; int candidate = -1; };
    // what one evaluation leaves for a frame pair
    struct Table {
        int N = 0, nh = 0, model = INIT_MODEL_NONE, best[2] = {-1, -1}, n_inliers = 0, n_cand = 0, nGood[INIT_MAX_CAND] = {0};
        float S[2] = {0, 0}, RH = 0, cand_Rt[12 * INIT_MAX_CAND] = {0}, cos_parallax[INIT_MAX_CAND] = {0};
        std::vector<float> score, matrix, points; // 2 x nh, 2 x nh x 9, 8 x N x 3
        std::vector<uint32_t> mask, good_mask;    // 2 x nh x W, 8 x W
    };

    // ReferenceFrame_keys: x y of ReferenceFrame.mvKeysUn; K row-major 3 x 3
    Initializer(std::vector<float> ReferenceFrame_keys, const float K[9], float sigma = 1.0f, int iterations = 200, Context *ctx = nullptr)
        : mvKeys1(std::move(ReferenceFrame_keys)), mSigma(sigma), mMaxIterations(iterations), ctx_(ctx) {
        if (mvKeys1.size() % 2) throw std::invalid_argument("Initializer: x y per key point");
        for (int k = 0; k < 9; k++) mK[k] = K[k];
    }

    void set_sets(std::vector<int> sets) { // 8 per iteration, in drawing order, for the next Initialize
        if (sets.size() % 8) throw std::invalid_argument("Initializer: set_sets wants 8 indices per iteration");
        mvSets = std::move(sets); have_sets_ = true;
    }
    void draw_sets(std::function<int(int, int)> RandomInt, int N) {
        std::vector<int> s;
        ransac_draw<8>(N, mMaxIterations, RandomInt, s);
        set_sets(std::move(s));
    }
    void set_random_int(std::function<int(int, int)> RandomInt) { random_int_ = std::move(RandomInt); }

    // :50-66.  vMatches12[i] = the index in the current frame matched to key point i of the reference frame, or < 0
    void prepare(std::vector<float> CurrentFrame_keys, const std::vector<int> &vMatches12) {
        if (CurrentFrame_keys.size() % 2 || 2 * vMatches12.size() > mvKeys1.size()) throw std::invalid_argument("Initializer: key points and matches do not fit");
        mvKeys2 = std::move(CurrentFrame_keys);
        mvMatches12.clear();
        for (size_t i = 0; i < vMatches12.size(); i++)
            if (vMatches12[i] >= 0) { mvMatches12.push_back((int)i); mvMatches12.push_back(vMatches12[i]); }
        const int N = (int)(mvMatches12.size() / 2);
        if (N >= 8 && !have_sets_ && random_int_) draw_sets(random_int_, N);
        if (N >= 8 && !have_sets_) throw std::runtime_error("Initializer: no sets (set_sets, draw_sets or set_random_int)");
        pending_ = N >= 8 ? mvSets : std::vector<int>();
        mvSets.clear(); have_sets_ = false; // (a table serves one Initialize: the reference draws anew every time)
        prepared_ = true; evaluated_ = false;
    }

    // every prepared initializer in one call: on the device of ctx, or on the host without one
    static void evaluate_many(const std::vector<Initializer *> &all, Context *ctx) {
        std::vector<Initializer *> its;
        for (Initializer *i : all) if (i->prepared_ && !i->evaluated_) its.push_back(i);
        if (its.empty()) return;
        std::vector<int> k1o{0}, k2o{0}, co{0}, ho{0}, mt, sets;
        std::vector<float> keys1, keys2, K, sigma;
        for (const Initializer *i : its) {
            k1o.push_back(k1o.back() + (int)(i->mvKeys1.size() / 2)); k2o.push_back(k2o.back() + (int)(i->mvKeys2.size() / 2));
            co.push_back(co.back() + (int)(i->mvMatches12.size() / 2)); ho.push_back(ho.back() + (int)(i->pending_.size() / 8));
            keys1.insert(keys1.end(), i->mvKeys1.begin(), i->mvKeys1.end()); keys2.insert(keys2.end(), i->mvKeys2.begin(), i->mvKeys2.end());
            mt.insert(mt.end(), i->mvMatches12.begin(), i->mvMatches12.end()); sets.insert(sets.end(), i->pending_.begin(), i->pending_.end());
            K.insert(K.end(), i->mK, i->mK + 9); sigma.push_back(i->mSigma);
        }
        const int n = (int)its.size(), H = ho.back(), NC = co.back();
        std::vector<InitProblem> problems;
        std::vector<int> hyp_problem;
        long words = 0, cwords = 0, at[2];
        mt.push_back(0); sets.push_back(0); keys1.push_back(0); keys2.push_back(0); // (no NULL for an empty array)
        const char *what = init_build(n, k1o.data(), keys1.data(), k2o.data(), keys2.data(), co.data(), mt.data(), K.data(), sigma.data(), ho.data(), sets.data(), true, problems,
                                      hyp_problem, &words, &cwords, at);
        if (what) throw std::invalid_argument(std::string("Initializer: ") + what);
        std::vector<float> score(2 * (size_t)H + 1), matrix(18 * (size_t)H + 1), S(2 * (size_t)n), RH((size_t)n), cand(96 * (size_t)n), cosp(8 * (size_t)n), points(24 * (size_t)NC + 1);
        std::vector<uint32_t> mask(2 * (size_t)words + 1), gm((size_t)cwords + 1);
        std::vector<int> model((size_t)n), best(2 * (size_t)n), ninl((size_t)n), ncand((size_t)n), nGood(8 * (size_t)n);
        if (ctx) {
#ifndef CUBESLAM_HOST_ONLY
            const int r = cs_initializer_evaluate(ctx->ctx, n, k1o.data(), keys1.data(), k2o.data(), keys2.data(), co.data(), mt.data(), K.data(), sigma.data(), ho.data(), sets.data(),
                                                  score.data(), matrix.data(), mask.data(), model.data(), best.data(), S.data(), RH.data(), ninl.data(), ncand.data(), cand.data(),
                                                  nGood.data(), cosp.data(), gm.data(), points.data());
            if (r != CS_OK) throw std::runtime_error("cs_initializer_evaluate failed (" + std::to_string(r) + "): " + cs_last_error(ctx->ctx));
#else
            throw std::runtime_error("Initializer: built without the library");
#endif
        } else
            init_host_run(problems, keys1.data(), keys2.data(), mt.data(), sets.data(), H, words, cwords, k1o.back(), k2o.back(), NC,
                          InitOutputs{score.data(), matrix.data(), mask.data(), model.data(), best.data(), S.data(), RH.data(), ninl.data(), ncand.data(), cand.data(), nGood.data(),
                                      cosp.data(), gm.data(), points.data()});
        for (int p = 0; p < n; p++) {
            Table &t = its[p]->table;
            const InitProblem &P = problems[p];
            const size_t W = (size_t)ransac_words(P.N);
            t = Table();
            t.N = P.N; t.nh = P.nh; t.model = model[p]; t.n_inliers = ninl[p]; t.n_cand = ncand[p]; t.RH = RH[p];
            for (int m = 0; m < 2; m++) {
                t.best[m] = best[2 * p + m]; t.S[m] = S[2 * p + m];
                t.score.insert(t.score.end(), score.begin() + (size_t)m * H + P.h0, score.begin() + (size_t)m * H + P.h0 + P.nh);
                t.matrix.insert(t.matrix.end(), matrix.begin() + 9 * ((size_t)m * H + P.h0), matrix.begin() + 9 * ((size_t)m * H + P.h0 + P.nh));
                t.mask.insert(t.mask.end(), mask.begin() + (size_t)m * words + P.w0, mask.begin() + (size_t)m * words + P.w0 + P.nh * W);
            }
            for (int c = 0; c < INIT_MAX_CAND; c++) { t.nGood[c] = nGood[8 * p + c]; t.cos_parallax[c] = cosp[8 * p + c]; }
            for (int k = 0; k < 12 * INIT_MAX_CAND; k++) t.cand_Rt[k] = cand[96 * (size_t)p + k];
            t.good_mask.assign(gm.begin() + P.cw0, gm.begin() + P.cw0 + INIT_MAX_CAND * W);
            t.points.assign(points.begin() + 24 * (size_t)P.c0, points.begin() + 24 * ((size_t)P.c0 + P.N));
            its[p]->evaluated_ = true;
        }
    }

    // the reference's return values for the prepared pair.  Fewer than 8 matches: false (the reference's set drawing is undefined there; Tracking.cc:954 asks for 100)
    Result result(float minParallax = 1.0f, int minTriangulated = 50) {
        if (!prepared_) throw std::runtime_error("Initializer: nothing prepared");
        if (!evaluated_) evaluate_many({this}, ctx_);
        Result r;
        const Table &t = table;
        r.candidate = init_walk(t.model, t.n_cand, t.nGood, t.cos_parallax, t.n_inliers, minParallax, minTriangulated, &r.parallax);
        if (r.candidate < 0) return r;
        r.success = true;
        const size_t n1 = mvKeys1.size() / 2, W = (size_t)ransac_words(t.N);
        r.vP3D.assign(3 * n1, 0.f); r.vbTriangulated.assign(n1, false);
        const float *pts = t.points.data() + 3 * (size_t)r.candidate * t.N;
        const uint32_t *gm = t.good_mask.data() + (size_t)r.candidate * W;
        for (int i = 0; i < t.N; i++) { // vP3D[vMatches12[i].first], vbGood[vMatches12[i].first] (:893, :897)
            const size_t first = (size_t)mvMatches12[2 * (size_t)i];
            for (int k = 0; k < 3; k++) r.vP3D[3 * first + k] = pts[3 * (size_t)i + k];
            r.vbTriangulated[first] = ransac_mask_bit(gm, i);
        }
        for (int k = 0; k < 9; k++) r.R21[k] = t.cand_Rt[12 * r.candidate + k];
        for (int k = 0; k < 3; k++) r.t21[k] = t.cand_Rt[12 * r.candidate + 9 + k];
        return r;
    }
    Result Initialize(std::vector<float> CurrentFrame_keys, const std::vector<int> &vMatches12) {
        prepare(std::move(CurrentFrame_keys), vMatches12);
        return result();
    }

    std::vector<float> mvKeys1, mvKeys2;
    std::vector<int> mvMatches12; // first, second per match
    std::vector<int> mvSets;      // 8 per iteration
    float mK[9], mSigma;
    int mMaxIterations;
    Table table;

  private:
    Context *ctx_;
    std::vector<int> pending_;
    std::function<int(int, int)> random_int_;
    bool have_sets_ = false, prepared_ = false, evaluated_ = false;
};

} // namespace cubeslam
