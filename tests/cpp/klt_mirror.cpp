// TEST INFRASTRUCTURE: driver of cubeslam::ORBmatcher's dynamic-object KLT (cube_slam_amd/host/orb_slam_mirrors.hpp) for tests/test_klt_mirrors.py (`host`: no context,
// the g++ build of csrc/klt_math.h; built with -DCUBESLAM_HOST_ONLY it links nothing of the library and runs `host` only, and a second time with
// -fsanitize=address,undefined).
//   klt_mirror <in> <out> [host]
// <in>: int32 n_pairs; per pair int32 width, height, stride, n, has_mask (2: a SearchByTracking record, below), the two images (height * stride bytes each), the points (2 n floats), the mask
// (width * height bytes, when has_mask).
// <out>: per pair nextPts[2 n], status[n], err[n]; with a mask also int32 goodmatches, n_mask_outside, kept[goodmatches], pts[2 goodmatches], object_id[goodmatches].
// A SearchByTracking record continues behind the images with int32 N, numobject, has_static, has_had, float th, bounds[4], scale_factors[8], mvKeys (n records of
// 28 bytes), eligible[n], object ids (n int32), mvKeysUn (N records), KeysStatic[N] and hadMapPoint[N] when present; its output is int32 n_tracked, four counters,
// train_match[N], lastptsinds, featuresklt_lastframe, featuresklt_thisframe.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "cube_slam_amd/host/orb_slam_mirrors.hpp"

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
    const int n_pairs = rd<int>(1)[0];
    for (int p = 0; p < n_pairs; p++) {
        const std::vector<int> h = rd<int>(5);
        const int W = h[0], H = h[1], stride = h[2], n = h[3], has_mask = h[4];
        const std::vector<uint8_t> last = rd<uint8_t>((size_t)H * stride), cur = rd<uint8_t>((size_t)H * stride);
        if (has_mask == 2) {
            const std::vector<int> t = rd<int>(4);
            const std::vector<float> f = rd<float>(1 + 4 + 8);
            const std::vector<cs_keypoint> lk = rd<cs_keypoint>((size_t)n);
            const std::vector<uint8_t> elig = rd<uint8_t>((size_t)n);
            const std::vector<int> obj = rd<int>((size_t)n);
            const std::vector<cs_keypoint> ck = rd<cs_keypoint>((size_t)t[0]);
            const std::vector<uint8_t> ks = rd<uint8_t>(t[2] ? (size_t)t[0] : 0), hm = rd<uint8_t>(t[3] ? (size_t)t[0] : 0);
            const cubeslam::ORBmatcher::TrackingResult r = cubeslam::ORBmatcher::SearchByTracking(ctx, last.data(), cur.data(), W, H, stride, lk, elig, obj, t[1], f[0],
                                                                                                   std::vector<float>(f.begin() + 5, f.end()), ck, &f[1], ks, hm);
            wr(std::vector<int>{(int)r.lastptsinds.size(), r.kltmatches, r.goodmatches, r.findfeaturematches, r.uniquematches});
            wr(r.train_match); wr(r.lastptsinds); wr(r.featuresklt_lastframe); wr(r.featuresklt_thisframe);
            continue;
        }
        const std::vector<float> pts = rd<float>(2 * (size_t)n);
        if (!has_mask) {
            const cubeslam::ORBmatcher::Flow f = cubeslam::ORBmatcher::calcOpticalFlowPyrLK(ctx, last.data(), cur.data(), W, H, stride, pts);
            wr(f.nextPts); wr(f.status); wr(f.err);
            continue;
        }
        const std::vector<uint8_t> mask = rd<uint8_t>((size_t)W * H);
        const cubeslam::ORBmatcher::HarrisResult r = cubeslam::ORBmatcher::SearchByTrackingHarris(ctx, last.data(), cur.data(), W, H, stride, pts, mask.data());
        wr(r.flow.nextPts); wr(r.flow.status); wr(r.flow.err);
        wr(std::vector<int>{r.goodmatches, r.n_mask_outside});
        wr(r.kept); wr(r.pts); wr(r.object_id);
    }
    fclose(out);
    return 0;
}
