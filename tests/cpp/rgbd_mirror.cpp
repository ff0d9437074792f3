// TEST INFRASTRUCTURE: driver of the RGB-D members of cubeslam::Frame and of cubeslam::ClosePoints (cube_slam_amd/host/orb_slam_mirrors.hpp) for
// tests/test_rgbd_host_cpp_gpu.py (on the device) and tests/test_rgbd_mirrors.py (`host`: no context, the g++ build of csrc/rgbd_math.h; built with
// -DCUBESLAM_HOST_ONLY it links nothing of the library and runs `host` only, and a second time with -fsanitize=address,undefined).
//   rgbd_mirror <in> <out> [host]
// <in>: int32 n_frames; per frame int32 type, width, height, stride_bytes, mode, N, float factor, bf, th_depth, K4[4], Tcw[12], the image (height * stride_bytes bytes),
// mvKeys (N records of 28 bytes), mvKeysUn (N records), need_new (N bytes).
// <out>: per frame int32 n_with_depth, n_outside, mvuRight[N], mvDepth[N], int32 n_valid, n_walked, n_new, order[n_valid], new_idx[n_new], new_x3D[3 n_new], and
// Frame::UnprojectStereo of every new_idx once more (3 n_new floats).
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
    const int n_frames = rd<int>(1)[0];
    for (int f = 0; f < n_frames; f++) {
        const std::vector<int> h = rd<int>(6);
        const int type = h[0], W = h[1], H = h[2], stride = h[3], mode = h[4], N = h[5];
        const std::vector<float> p = rd<float>(3 + 4 + 12);
        const float factor = p[0], bf = p[1], th = p[2], *K4 = &p[3], *Tcw = &p[7];
        const std::vector<uint8_t> image = rd<uint8_t>((size_t)H * stride);
        cubeslam::Frame F(ctx, K4, bf, W, H);
        F.mvKeys = rd<cs_keypoint>(N);
        F.mvKeysUn = rd<cs_keypoint>(N);
        const std::vector<uint8_t> need_new = rd<uint8_t>(N);
        const int n_with = F.ComputeStereoFromRGBD(image.data(), type, stride, factor);
        wr(std::vector<int>{n_with, F.n_outside});
        wr(F.mvuRight); wr(F.mvDepth);
        F.SetPose(Tcw);
        const cubeslam::ClosePointsResult r = cubeslam::ClosePoints(ctx, F.mvDepth, F.mvKeysUn, need_new, Tcw, K4, th, mode);
        wr(std::vector<int>{r.n_valid, r.n_walked, (int)r.new_idx.size()});
        wr(r.order); wr(r.new_idx); wr(r.new_x3D);
        std::vector<float> again;
        for (int i : r.new_idx) {
            float x3D[3];
            if (!F.UnprojectStereo(i, x3D)) { fprintf(stderr, "frame %d: a point was created for key point %d, which has no depth\n", f, i); return 3; }
            again.insert(again.end(), x3D, x3D + 3);
        }
        wr(again);
        for (int i = 0; i < N; i++) {
            float x3D[3];
            if (F.UnprojectStereo(i, x3D) != (F.mvDepth[(size_t)i] > 0)) { fprintf(stderr, "frame %d: UnprojectStereo(%d) and mvDepth disagree\n", f, i); return 3; }
        }
    }
    fclose(out);
    return 0;
}
