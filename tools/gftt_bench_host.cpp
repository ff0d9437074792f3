// cubeslam::goodFeaturesToTrack and cubeslam::Tracking::CreateNewHarrisFeatures on the host (cube_slam_amd/host/ built with -DCUBESLAM_HOST_ONLY -O2 -ffp-contract=off
// -pthread) over the frames of the input, on `threads` threads (the frames are independent: each thread takes every threads-th): the comparison side of
// tools/gftt_bench.py.
//   gftt_bench_host <in> <threads> <reps> <warmup>
// <in>: int32 n_frames, width, height, n (existing points per frame), the dense frames, the object masks, the points (2 n floats per frame), the observation counts
// (n int32 per frame), K4, Twc (12 floats); the cuboid depths are 3 and 5.
// Prints per repetition the wall time in ms of goodFeaturesToTrack(frame, mask, 200, 0.1, 10) over all frames and of CreateNewHarrisFeatures over all frames, then the
// corners of the one and the new points of the other (checksums for the caller).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "cube_slam_amd/host/orb_slam_mirrors.hpp"
#include "cube_slam_amd/host/tracking.hpp"

static FILE *in;
template <class T> static std::vector<T> rd(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main(int argc, char **argv) {
    if (argc < 5 || !(in = fopen(argv[1], "rb"))) return 2;
    const int threads = atoi(argv[2]), reps = atoi(argv[3]), warmup = atoi(argv[4]);
    const std::vector<int> h = rd<int>(4);
    const int F = h[0], W = h[1], H = h[2], n = h[3];
    const size_t px = (size_t)W * H;
    const std::vector<uint8_t> gray = rd<uint8_t>(px * F), masks = rd<uint8_t>(px * F);
    std::vector<std::vector<float>> pts((size_t)F);
    std::vector<std::vector<int>> obs((size_t)F);
    for (int f = 0; f < F; f++) pts[(size_t)f] = rd<float>(2 * (size_t)n);
    for (int f = 0; f < F; f++) obs[(size_t)f] = rd<int>((size_t)n);
    const std::vector<float> K4 = rd<float>(4), Twc = rd<float>(12), depth = {3.f, 5.f};
    std::vector<long> count((size_t)threads);
    long sums[2] = {0, 0};
    for (int r = 0; r < warmup + reps; r++)
        for (int what = 0; what < 2; what++) {
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<std::thread> pool;
            for (int t = 0; t < threads; t++)
                pool.emplace_back([&, t] {
                    long c = 0;
                    for (int f = t; f < F; f += threads) {
                        if (what == 0) c += (long)cubeslam::goodFeaturesToTrack(nullptr, &gray[px * f], W, H, W, &masks[px * f], 200, 0.1, 10.0).quality.size();
                        else c += (long)cubeslam::Tracking::CreateNewHarrisFeatures(nullptr, &gray[px * f], W, H, W, &masks[px * f], pts[(size_t)f], obs[(size_t)f], K4.data(), Twc.data(), depth).object_id.size();
                    }
                    count[(size_t)t] = c;
                });
            for (auto &p : pool) p.join();
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (r >= warmup) printf("%.4f\n", ms);
            sums[what] = 0;
            for (long c : count) sums[what] += c;
        }
    printf("%ld\n%ld\n", sums[0], sums[1]);
    return 0;
}
