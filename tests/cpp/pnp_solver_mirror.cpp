// TEST INFRASTRUCTURE: driver of cube_slam_amd/host/pnp_solver.hpp for tests/test_pnp_solver_mirrors.py: cubeslam::PnPsolver without a context, the g++ build of
// csrc/epnp_math.h and csrc/cv_svd_math.h (built with -DCUBESLAM_HOST_ONLY it links nothing of the library, and a second time with -fsanitize=address,undefined).
//   pnp_solver_mirror <in> <out> [draw]
// <in>, <out>: the formats of tests/pnp_solver_patterns.py (driver_input, driver_output), those of tests/cpp/ref_pnp_solver_standins.cpp.  `draw`: every solver gets only its
// first mRansacMaxIts quads as a table and a RandomInt that replays the others, so iterate() draws past the table (-2 from the walk, then resumed); the tables written are
// those it has at the end: a prefix of the pattern's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "cube_slam_amd/host/pnp_solver.hpp"

static FILE *in, *out;
template <class T> static std::vector<T> rd(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
template <class T> static void wr(const T *p, size_t n) { if (n) fwrite(p, sizeof(T), n, out); }

struct Replay { // RandomInt over the wanted indices: the position of each in the Fisher-Yates' vAvailableIndices
    std::vector<int> want, avail;
    size_t pos = 0;
    int N = 0;
    int operator()(int lo, int hi) {
        if (pos % 4 == 0) { avail.resize((size_t)N); for (int i = 0; i < N; i++) avail[i] = i; }
        if (pos >= want.size()) { fprintf(stderr, "RandomInt: past the pattern's quads\n"); exit(3); }
        const int at = (int)(std::find(avail.begin(), avail.end(), want[pos++]) - avail.begin());
        if (lo != 0 || hi != (int)avail.size() - 1 || at > hi) { fprintf(stderr, "RandomInt: not the Fisher-Yates of :187-200\n"); exit(3); }
        avail[at] = avail.back(); avail.pop_back();
        return at;
    }
};

int main(int argc, char **argv) {
    if (argc < 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    const bool draw = argc > 3 && !strcmp(argv[3], "draw");
    const int n = rd<int>(1)[0];
    std::vector<std::unique_ptr<cubeslam::PnPsolver>> solvers;
    std::vector<std::shared_ptr<Replay>> replays;
    for (int s = 0; s < n; s++) {
        const std::vector<int> h = rd<int>(6);
        const double prob = rd<double>(1)[0];
        const std::vector<float> ef = rd<float>(2), K = rd<float>(4);
        const int N = h[0];
        std::vector<float> X = rd<float>(3 * (size_t)N), U = rd<float>(2 * (size_t)N), S = rd<float>((size_t)N);
        std::vector<int> idx = rd<int>((size_t)N), quads = rd<int>(4 * (size_t)h[2]);
        solvers.emplace_back(new cubeslam::PnPsolver(X, U, S, K.data(), idx, h[1], nullptr));
        cubeslam::PnPsolver &p = *solvers.back();
        p.SetRansacParameters(prob, h[3], h[4], h[5], ef[0], ef[1]);
        replays.emplace_back(new Replay);
        if (draw && p.live()) {
            Replay &r = *replays.back();
            r.N = N; r.want = quads;
            std::shared_ptr<Replay> keep = replays.back();
            p.draw_quads([keep](int lo, int hi) { return (*keep)(lo, hi); }, 0);
        } else if (!quads.empty())
            p.set_quads(quads);
    }
    const int n_calls = rd<int>(1)[0];
    const std::vector<int> calls = rd<int>(2 * (size_t)n_calls);
    std::vector<cubeslam::PnPsolver *> all;
    for (auto &s : solvers) all.push_back(s.get());
    cubeslam::PnPsolver::evaluate_many(all, nullptr); // one call for every candidate
    std::vector<cubeslam::PnPsolver::Result> results;
    std::vector<int> state;
    for (int c = 0; c < n_calls; c++) {
        cubeslam::PnPsolver &p = *solvers[(size_t)calls[2 * c]];
        results.push_back(p.iterate(calls[2 * c + 1]));
        state.push_back(p.mnIterations); state.push_back(p.mnBestInliers);
    }
    for (auto &sp : solvers) {
        cubeslam::PnPsolver &p = *sp;
        const int par[2] = {p.mRansacMinInliers, p.mRansacMaxIts};
        wr(par, 2); wr(&p.mRansacEpsilon, 1);
        const int H = (int)p.n_inliers.size();
        wr(&H, 1);
        const int W = (p.N + 31) / 32;
        std::vector<unsigned char> m((size_t)p.N);
        for (size_t h = 0; h < p.n_inliers.size(); h++) {
            wr(&p.Rt[12 * h], 12); wr(&p.n_inliers[h], 1);
            for (int i = 0; i < p.N; i++) m[i] = p.inlier_mask[h * W + (i >> 5)] >> (i & 31) & 1u;
            wr(m.data(), m.size());
            const int record = (p.status[h] & PNP_RECORD) != 0;
            if (p.status[h] & ~PNP_RECORD) { fprintf(stderr, "qr_solve status %u at hypothesis %zu\n", p.status[h], h); }
            wr(&record, 1);
            if (record) {
                wr(&p.refined_Rt[12 * h], 12); wr(&p.refined_n[h], 1);
                for (int i = 0; i < p.N; i++) m[i] = p.refined_mask[h * W + (i >> 5)] >> (i & 31) & 1u;
                wr(m.data(), m.size());
            }
        }
    }
    for (int c = 0; c < n_calls; c++) {
        const cubeslam::PnPsolver::Result &r = results[(size_t)c];
        const int res[5] = {(int)r.found, (int)r.bNoMore, r.nInliers, state[2 * (size_t)c], state[2 * (size_t)c + 1]};
        wr(res, 5);
        wr(r.Tcw, 16);
        std::vector<unsigned char> vb(r.vbInliers.begin(), r.vbInliers.end());
        wr(vb.data(), vb.size());
    }
    fclose(out);
    return 0;
}
