// Host side of tools/initializer_bench.py: the evaluation of cs_initializer_evaluate without a context (csrc/initializer_host.h over csrc/initializer_math.h; g++ -O2
// -ffp-contract=off -pthread, -DCUBESLAM_HOST_ONLY) over the frame pairs of the input, on `threads` threads (the pairs are independent: each thread takes every threads-th).
//   initializer_bench_host <in> <out> <threads> <reps>
// <in>: int n; per pair int n1, n2, N, H; float sigma, K[9]; keys1[2 n1], keys2[2 n2]; int matches[2 N], sets[8 H].  Prints the wall milliseconds of each repetition;
// <out>: per pair the tables in the order of tests/cpp/initializer_mirror.cpp.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "cube_slam_amd/csrc/initializer_host.h"

static FILE *in, *out;
template <class T> static std::vector<T> rd(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
template <class T> static void wr(const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), out); }

struct Pair {
    int n1, n2, N, H;
    std::vector<float> sk, keys1, keys2;
    std::vector<int> matches, sets;
    std::vector<InitProblem> problems;
    long words = 0, cwords = 0;
    std::vector<int> ints;            // model 1, best 2, n_inliers 1, n_cand 1, nGood 8
    std::vector<float> floats;        // S 2, RH 1, cand 96, cos 8
    std::vector<float> score, matrix, points;
    std::vector<uint32_t> mask, good_mask;
    void run() {
        init_host_run(problems, keys1.data(), keys2.data(), matches.data(), sets.data(), H, words, cwords, n1, n2, N,
                      InitOutputs{score.data(), matrix.data(), mask.data(), ints.data(), ints.data() + 1, floats.data(), floats.data() + 2, ints.data() + 3, ints.data() + 4,
                                  floats.data() + 3, ints.data() + 5, floats.data() + 99, good_mask.data(), points.data()});
    }
};

int main(int argc, char **argv) {
    if (argc < 5 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    const int threads = atoi(argv[3]), reps = atoi(argv[4]);
    const int n = rd<int>(1)[0];
    std::vector<Pair> pairs((size_t)n);
    for (Pair &p : pairs) {
        const std::vector<int> h = rd<int>(4);
        p.n1 = h[0]; p.n2 = h[1]; p.N = h[2]; p.H = h[3];
        p.sk = rd<float>(10); p.keys1 = rd<float>(2 * (size_t)p.n1); p.keys2 = rd<float>(2 * (size_t)p.n2); p.matches = rd<int>(2 * (size_t)p.N); p.sets = rd<int>(8 * (size_t)p.H);
        const int k1o[2] = {0, p.n1}, k2o[2] = {0, p.n2}, co[2] = {0, p.N}, ho[2] = {0, p.H};
        std::vector<int> hyp_problem;
        long at[2];
        if (const char *what = init_build(1, k1o, p.keys1.data(), k2o, p.keys2.data(), co, p.matches.data(), p.sk.data() + 1, p.sk.data(), ho, p.sets.data(), true, p.problems,
                                          hyp_problem, &p.words, &p.cwords, at)) { fprintf(stderr, "%s\n", what); return 3; }
        p.ints.assign(13, 0); p.floats.assign(107, 0.f);
        p.score.assign(2 * (size_t)p.H, 0.f); p.matrix.assign(18 * (size_t)p.H, 0.f); p.mask.assign(2 * (size_t)p.words, 0u);
        p.good_mask.assign((size_t)p.cwords, 0u); p.points.assign(24 * (size_t)p.N, 0.f);
    }
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++)
            pool.emplace_back([&, t] { for (size_t i = (size_t)t; i < pairs.size(); i += (size_t)threads) pairs[i].run(); });
        for (std::thread &t : pool) t.join();
        printf("%.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    for (const Pair &p : pairs) { wr(p.ints); wr(p.floats); wr(p.score); wr(p.matrix); wr(p.mask); wr(p.good_mask); wr(p.points); }
    fclose(out);
    return 0;
}
