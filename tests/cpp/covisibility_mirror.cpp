// covisibility_mirror.cpp -- driver of the C++ mirror cube_slam_amd/host/covisibility.hpp over libcubeslam_hip.so (tests/test_covisibility_host_cpp_gpu.py).  Reads a case
// dumped by tests/covisibility_patterns.py (dump), runs the mirror's function of its kind on the device (or, with "host", through the library's host forms) and writes every
// result as int32 words; for a vote also the connection state UpdateConnections leaves: per key frame the ordered lists, the weights, the parent.
//   usage: covisibility_mirror device|host in.bin out.bin
#include <cstdio>
#include <cstring>
#include <memory>

#include "cube_slam_amd/host/covisibility.hpp"

namespace {
struct Reader {
    std::vector<unsigned char> buf;
    size_t at = 0;
    const unsigned char *take(size_t n) {
        if (at + n > buf.size()) throw std::runtime_error("short input");
        const unsigned char *p = buf.data() + at;
        at += n;
        return p;
    }
    template <class T> std::vector<T> words(size_t n) {
        std::vector<T> v(n);
        const unsigned char *p = take(4 * n);
        if (n) memcpy(v.data(), p, 4 * n);
        return v;
    }
    std::vector<uint8_t> bytes(size_t n) {
        std::vector<uint8_t> v(n);
        const unsigned char *p = take((n + 3) / 4 * 4);
        if (n) memcpy(v.data(), p, n);
        return v;
    }
};
std::vector<int> out;
template <class T> void put(const std::vector<T> &v) { for (const T &x : v) out.push_back((int)x); }
} // namespace

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s device|host in.bin out.bin\n", argv[0]); return 2; }
    try {
        Reader r;
        FILE *f = fopen(argv[2], "rb");
        if (!f) { perror(argv[2]); return 2; }
        unsigned char chunk[65536];
        size_t n;
        while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) r.buf.insert(r.buf.end(), chunk, chunk + n);
        fclose(f);
        const std::vector<int> head = r.words<int>(4);
        const size_t np = (size_t)head[2], n_obs = (size_t)head[3];
        cubeslam::ObsTable t;
        t.n_kf = head[1];
        t.obs_off = r.words<int>(np + 1); t.obs_kf = r.words<int>(n_obs); t.obs_octave = r.words<int>(n_obs); t.obs_stereo = r.bytes(n_obs);
        t.mp_nobs = r.words<int>(np); t.mp_flags = r.bytes(np);
        std::unique_ptr<cubeslam::Context> ctx;
        if (std::string(argv[1]) == "device") ctx.reset(new cubeslam::Context());
        const cubeslam::Covisibility cov(ctx.get());
        if (head[0] == 0) {
            const std::vector<int> h = r.words<int>(4);
            const std::vector<int> queries = r.words<int>((size_t)h[0]);
            cubeslam::SlotLists lists;
            lists.off = r.words<int>((size_t)h[0] + 1); lists.mp = r.words<int>((size_t)h[1]);
            cubeslam::Connections c(t.n_kf);
            const cubeslam::ConnectionVotes v = cov.UpdateConnections(t, queries, lists, c, h[2] != 0, h[3]);
            put(v.cnt_off); put(v.cnt_kf); put(v.cnt_w); put(v.kf_max); put(v.w_max); put(v.ord_off); put(v.ord_kf); put(v.ord_w);
            for (int k = 0; k < t.n_kf; k++) {
                if (c.mConnectedKeyFrameWeights[(size_t)k].empty() && c.mpParent[(size_t)k] < 0) continue; // (most key frames of the seam case have no connection)
                out.push_back(k); out.push_back((int)c.mvpOrderedConnectedKeyFrames[(size_t)k].size());
                put(c.mvpOrderedConnectedKeyFrames[(size_t)k]); put(c.mvOrderedWeights[(size_t)k]);
                out.push_back((int)c.mConnectedKeyFrameWeights[(size_t)k].size());
                for (const auto &kv : c.mConnectedKeyFrameWeights[(size_t)k]) { out.push_back(kv.first); out.push_back(kv.second); }
                out.push_back(c.mpParent[(size_t)k]); out.push_back(c.mbFirstConnection[(size_t)k]);
                put(c.mspChildrens[(size_t)k]);
            }
        } else if (head[0] == 1) {
            const std::vector<int> h = r.words<int>(4);
            const size_t nl = (size_t)h[0], ns = (size_t)h[1];
            const std::vector<int> local = r.words<int>(nl);
            cubeslam::SlotLists lists;
            lists.off = r.words<int>(nl + 1); lists.mp = r.words<int>(ns);
            const std::vector<int> slot_octave = r.words<int>(ns);
            const std::vector<float> slot_depth = r.words<float>(ns), th_depth = r.words<float>(nl);
            const std::vector<uint8_t> kf_flags = r.bytes(nl);
            const cubeslam::KeyFrameCullingResult k = cov.KeyFrameCulling(t, local, lists, slot_octave, slot_depth, th_depth, h[2] != 0, kf_flags, h[3]);
            put(k.verdict); put(k.n_mps); put(k.n_redundant); put(k.mp_nobs); put(k.mp_flags); put(k.alive);
            out.push_back(k.n_rounds);
        } else {
            const std::vector<int> h = r.words<int>(3);
            const std::vector<int> recent = r.words<int>((size_t)h[0]), found = r.words<int>(np), visible = r.words<int>(np), first = r.words<int>(np);
            put(cov.MapPointCulling(t, recent, found, visible, first, h[1], h[2]));
        }
        f = fopen(argv[3], "wb");
        if (!f) { perror(argv[3]); return 2; }
        if (!out.empty()) fwrite(out.data(), sizeof(int), out.size(), f);
        fclose(f);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
