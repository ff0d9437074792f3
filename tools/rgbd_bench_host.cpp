// The close-point rule of cubeslam::ClosePoints on the host (cube_slam_amd/host/orb_slam_mirrors.hpp built with -DCUBESLAM_HOST_ONLY -O2 -ffp-contract=off -pthread)
// over the frames of the input, on `threads` threads (the frames are independent: each thread takes every threads-th): the comparison side of tools/rgbd_bench.py.
//   rgbd_bench_host <in> <threads> <reps> <warmup>
// <in>: int32 n_frames, first[n_frames + 1], float K4[4], th_depth, Tcw[12 n_frames], mvDepth[total], mvKeysUn (total records of 28 bytes), need_new[total].
// Prints the wall time of every repetition in ms, then the number of points created (a checksum for the caller).
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
    const int F = rd<int>(1)[0];
    const std::vector<int> first = rd<int>((size_t)F + 1);
    const std::vector<float> K4 = rd<float>(4), th = rd<float>(1), Tcw = rd<float>(12 * (size_t)F), depth = rd<float>((size_t)first[F]);
    const std::vector<cs_keypoint> keysUn = rd<cs_keypoint>((size_t)first[F]);
    const std::vector<uint8_t> need = rd<uint8_t>((size_t)first[F]);
    std::vector<std::vector<float>> d((size_t)F);
    std::vector<std::vector<cs_keypoint>> k((size_t)F);
    std::vector<std::vector<uint8_t>> nn((size_t)F);
    for (int f = 0; f < F; f++) {
        d[f].assign(depth.begin() + first[f], depth.begin() + first[f + 1]);
        k[f].assign(keysUn.begin() + first[f], keysUn.begin() + first[f + 1]);
        nn[f].assign(need.begin() + first[f], need.begin() + first[f + 1]);
    }
    std::vector<long> created((size_t)threads);
    for (int r = 0; r < warmup + reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++)
            pool.emplace_back([&, t] {
                long c = 0;
                for (int f = t; f < F; f += threads)
                    c += (long)cubeslam::ClosePoints(nullptr, d[f], k[f], nn[f], &Tcw[12 * (size_t)f], K4.data(), th[0], CS_CLOSE_POINTS_NEAREST).new_idx.size();
                created[(size_t)t] = c;
            });
        for (auto &p : pool) p.join();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (r >= warmup) printf("%.4f\n", ms);
    }
    long total = 0;
    for (long c : created) total += c;
    printf("%ld\n", total);
    return 0;
}
