// Exercises cubeslam::Frame::ComputeStereoMatches (cube_slam_amd/host/orb_slam_mirrors.hpp) on one rectified pair read from two raw files; prints what
// tests/test_stereo_host_cpp_gpu.py compares with the Python mirror's result: N, the matches kept and checksums of mvuRight / mvDepth.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cube_slam_amd/host/orb_slam_mirrors.hpp"

static unsigned long long fnv(const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

static bool read_raw(const char *path, std::vector<uint8_t> &img) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(img.data(), 1, img.size(), f) == img.size();
    fclose(f);
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 8) return 2;
    const int W = atoi(argv[3]), H = atoi(argv[4]), nfeatures = atoi(argv[5]);
    const float bf = (float)atof(argv[6]), b = (float)atof(argv[7]);
    std::vector<uint8_t> left((size_t)W * H), right((size_t)W * H);
    if (!read_raw(argv[1], left) || !read_raw(argv[2], right)) return 3;
    try {
        cubeslam::Context ctx(0);
        cubeslam::ORBextractor extractorLeft(ctx, nfeatures, 1.2f, 8, 20, 7, W, H), extractorRight(ctx, nfeatures, 1.2f, 8, 20, 7, W, H);
        std::vector<cs_keypoint> mvKeys, mvKeysRight;
        std::vector<uint8_t> mDescriptors, mDescriptorsRight;
        extractorLeft(left.data(), W, mvKeys, mDescriptors);     // Frame.cc:106-110
        extractorRight(right.data(), W, mvKeysRight, mDescriptorsRight);
        cubeslam::Frame frame(ctx, &extractorLeft, &extractorRight, bf, b, nfeatures + 4 * 8 + 64);
        const int kept = frame.ComputeStereoMatches();           // Frame.cc:118
        printf("stereo %d %zu %d %llx %llx\n", frame.N, mvKeys.size(), kept, fnv(frame.mvuRight.data(), frame.mvuRight.size() * 4), fnv(frame.mvDepth.data(), frame.mvDepth.size() * 4));
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
