// cubeslam::ORBmatcher::calcOpticalFlowPyrLK on the host (cube_slam_amd/host/orb_slam_mirrors.hpp built with -DCUBESLAM_HOST_ONLY -O2 -ffp-contract=off -pthread) over the
// pairs of the input, on `threads` threads (the pairs are independent: each thread takes every threads-th): the comparison side of tools/klt_bench.py.
//   klt_bench_host <in> <threads> <reps> <warmup>
// <in>: int32 n_pairs, width, height, n (points per pair), n_pairs + 1 dense frames, the points (2 n floats per pair); pair p tracks from frame p to frame p + 1.
// Prints the wall time of every repetition in ms, then the number of points tracked (a checksum for the caller).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "cube_slam_amd/host/orb_slam_mirrors.hpp"

static FILE *in;
template <class T> static std::vector<T> rd(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main(int argc, char **argv) {
    if (argc < 5 || !(in = fopen(argv[1], "rb"))) return 2;
    const int threads = atoi(argv[2]), reps = atoi(argv[3]), warmup = atoi(argv[4]);
    const std::vector<int> h = rd<int>(4);
    const int P = h[0], W = h[1], H = h[2], n = h[3];
    const std::vector<uint8_t> gray = rd<uint8_t>((size_t)(P + 1) * W * H);
    std::vector<std::vector<float>> pts((size_t)P);
    for (int p = 0; p < P; p++) pts[(size_t)p] = rd<float>(2 * (size_t)n);
    std::vector<long> tracked((size_t)threads);
    for (int r = 0; r < warmup + reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++)
            pool.emplace_back([&, t] {
                long c = 0;
                for (int p = t; p < P; p += threads) {
                    const cubeslam::ORBmatcher::Flow f = cubeslam::ORBmatcher::calcOpticalFlowPyrLK(nullptr, &gray[(size_t)p * W * H], &gray[(size_t)(p + 1) * W * H], W, H, W, pts[(size_t)p]);
                    for (uint8_t s : f.status) c += s;
                }
                tracked[(size_t)t] = c;
            });
        for (auto &p : pool) p.join();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (r >= warmup) printf("%.4f\n", ms);
    }
    long total = 0;
    for (long c : tracked) total += c;
    printf("%ld\n", total);
    return 0;
}
