// TEST INFRASTRUCTURE: driver of cubeslam::goodFeaturesToTrack (cube_slam_amd/host/orb_slam_mirrors.hpp) and cubeslam::Tracking::CreateNewHarrisFeatures
// (cube_slam_amd/host/tracking.hpp) for tests/test_gftt_mirrors.py (`host`: no context, the g++ build of csrc/gftt_math.h; built with -DCUBESLAM_HOST_ONLY it links
// nothing of the library and runs `host` only, and a second time with -fsanitize=address,undefined) and tests/test_gftt_host_cpp_gpu.py (the device path).
//   gftt_mirror <in> <out> [host]
// The two files are described in tests/gftt_patterns.py (write_mirror_input / read_mirror_output).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "cube_slam_amd/host/orb_slam_mirrors.hpp"
#include "cube_slam_amd/host/tracking.hpp"

static FILE *in, *out;
template <class T> static std::vector<T> rd(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
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
    const int n_records = rd<int>(1)[0];
    for (int p = 0; p < n_records; p++) {
        const std::vector<int> h = rd<int>(3);
        const int kind = h[0], W = h[1], H = h[2];
        const std::vector<uint8_t> img = rd<uint8_t>((size_t)W * H);
        if (kind == 0) {
            const std::vector<int> a = rd<int>(2);
            const std::vector<double> d = rd<double>(2);
            const std::vector<uint8_t> mask = rd<uint8_t>(a[0] ? (size_t)W * H : 0);
            int status = 0;
            cubeslam::GoodFeatures r;
            try { r = cubeslam::goodFeaturesToTrack(ctx, img.data(), W, H, W, a[0] ? mask.data() : nullptr, a[1], d[0], d[1]); }
            catch (const std::length_error &) { status = 1; }
            wr(std::vector<int>{status, (int)r.quality.size(), r.n_candidates});
            wr(r.corners); wr(r.quality);
            continue;
        }
        const std::vector<uint8_t> objmask = rd<uint8_t>((size_t)W * H);
        const std::vector<int> a = rd<int>(2);
        const std::vector<float> pts = rd<float>(2 * (size_t)a[0]);
        const std::vector<int> obs = rd<int>((size_t)a[0]);
        const std::vector<float> K4 = rd<float>(4), Twc = rd<float>(12), depth = rd<float>((size_t)a[1]);
        int status = 0;
        cubeslam::Tracking::NewHarrisFeatures r;
        r.good_mask.assign((size_t)W * H, 0);
        try { r = cubeslam::Tracking::CreateNewHarrisFeatures(ctx, img.data(), W, H, W, objmask.data(), pts, obs, K4.data(), Twc.data(), depth); }
        catch (const std::length_error &) { status = 1; }
        catch (const std::invalid_argument &) { status = 2; }
        catch (const std::runtime_error &) { status = 2; } // (the device path reports the library's status)
        wr(std::vector<int>{status, (int)r.object_id.size(), r.n_candidates, r.n_mask_outside});
        wr(r.good_mask); wr(r.pts); wr(r.object_id); wr(r.x3D); wr(r.x3D_valid);
    }
    fclose(out);
    return 0;
}
