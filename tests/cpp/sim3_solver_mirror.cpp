// TEST INFRASTRUCTURE: driver of cube_slam_amd/host/sim3_solver.hpp for tests/test_sim3_solver_host_cpp_gpu.py (on the device) and tests/test_sim3_solver_mirrors.py (`host`:
// no context, the g++ build of csrc/sim3_host.h over csrc/horn_math.h; built with -DCUBESLAM_HOST_ONLY it links nothing of the library and runs `host` only, and a second
// time with -fsanitize=address,undefined).
//   sim3_solver_mirror <in> <out> [host]
// <in>: int32 n_solvers; per solver int32 N, mN1, fix_scale, minInliers, maxIterations, double probability, X3Dc1[3N], X3Dc2[3N], max_err1[N], max_err2[N], K1[4], K2[4],
// mvnIndices1[N], then int32 3 * mRansacMaxIts as the test expects it and that many triple indices; int32 n_reject and n_reject pairs (solver, hypothesis): the successes the
// scripted ComputeSim3 round-robin lets fail; int32 n_rand and n_rand values: what RandomInt returns, in order, to draw_triples on a copy of solver 0.
// <out>: per solver int32 mRansacMaxIts, n_inliers, sRt, mask words; then per iterate(5) call of the round-robin int32 solver, found, bNoMore, nInliers, mnIterations,
// mnBestInliers, T12[16] and vbInliers as mN1 bytes; then int32 -1 and the triples drawn.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

#include "cube_slam_amd/host/sim3_solver.hpp"

static FILE *in, *out;
template <class T> static std::vector<T> rd(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static int rd_int() { return rd<int>(1)[0]; }
template <class T> static void wr(const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), out); }

int main(int argc, char **argv) {
    if (argc < 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    const bool host = argc > 3 && !strcmp(argv[3], "host");
    cubeslam::Context *ctx = nullptr;
#ifndef CUBESLAM_HOST_ONLY
    std::unique_ptr<cubeslam::Context> device;
    if (!host) { device.reset(new cubeslam::Context(0)); ctx = device.get(); }
#else
    if (!host) { fprintf(stderr, "built without the library: `host` only\n"); return 2; }
#endif
    const int n = rd_int();
    std::vector<std::unique_ptr<cubeslam::Sim3Solver>> solvers;
    for (int s = 0; s < n; s++) {
        const int N = rd_int(), mN1 = rd_int(), fix = rd_int(), minInliers = rd_int(), maxIterations = rd_int();
        const double prob = rd<double>(1)[0];
        std::vector<float> X1 = rd<float>(3 * (size_t)N), X2 = rd<float>(3 * (size_t)N), e1 = rd<float>(N), e2 = rd<float>(N), K1 = rd<float>(4), K2 = rd<float>(4);
        std::vector<int> idx1 = rd<int>(N);
        solvers.emplace_back(new cubeslam::Sim3Solver(X1, X2, e1, e2, K1.data(), K2.data(), idx1, mN1, fix != 0, ctx));
        solvers.back()->SetRansacParameters(prob, minInliers, maxIterations);
        const int nt = rd_int();
        std::vector<int> tri = rd<int>(nt);
        if (nt != 3 * solvers.back()->mRansacMaxIts) { fprintf(stderr, "solver %d: mRansacMaxIts %d, the test expects %d\n", s, solvers.back()->mRansacMaxIts, nt / 3); return 3; }
        solvers.back()->set_triples(tri);
    }
    std::set<std::pair<int, int>> reject;
    const int n_reject = rd_int();
    for (int k = 0; k < n_reject; k++) { const int a = rd_int(), b = rd_int(); reject.insert({a, b}); }

    std::vector<cubeslam::Sim3Solver *> all;
    for (auto &s : solvers) all.push_back(s.get());
    cubeslam::Sim3Solver::evaluate_many(all, ctx); // one call for every candidate
    for (auto &s : solvers) { wr(std::vector<int>{s->mRansacMaxIts}); wr(s->n_inliers); wr(s->sRt); wr(s->inlier_mask); }

    // LoopClosing::ComputeSim3 :283-342 with iterate(5)
    std::vector<bool> discarded((size_t)n, false);
    int nCandidates = n;
    bool bMatch = false;
    while (nCandidates > 0 && !bMatch) {
        for (int i = 0; i < n; i++) {
            if (discarded[i]) continue;
            cubeslam::Sim3Solver::Result r = solvers[i]->iterate(5);
            wr(std::vector<int>{i, (int)r.found, (int)r.bNoMore, r.nInliers, solvers[i]->mnIterations, solvers[i]->mnBestInliers});
            wr(std::vector<float>(r.T12, r.T12 + 16));
            std::vector<uint8_t> vb(r.vbInliers.begin(), r.vbInliers.end());
            wr(vb);
            if (r.bNoMore) { discarded[i] = true; nCandidates--; }
            if (r.found && !reject.count({i, solvers[i]->mnIterations - 1})) { bMatch = true; break; }
        }
    }

    const int n_rand = rd_int();
    const std::vector<int> rnd = rd<int>(n_rand);
    wr(std::vector<int>{-1});
    if (n && n_rand) {
        cubeslam::Sim3Solver copy = *solvers[0];
        size_t k = 0;
        copy.draw_triples([&](int lo, int hi) { const int v = rnd.at(k++); if (v < lo || v > hi) { fprintf(stderr, "RandomInt value outside its range\n"); exit(4); } return v; });
        wr(copy.triples);
    }
    fclose(out);
    return 0;
}
