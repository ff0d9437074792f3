// covisibility_driver.cpp -- stand-alone driver of the host walks of covisibility (cube_slam_amd/csrc/covis_walk.h over covis_math.h): plain C++, no HIP and no library, so it
// builds with g++ under -fsanitize=address,undefined (tests/test_covisibility_mirrors.py).  Reads a case dumped by tests/covisibility_patterns.py (dump), runs the walk of its
// kind and writes every output array as int32 words.
//   usage: covisibility_driver in.bin out.bin
#include <cstdint>
#include <cstdio>
#include <vector>

#include "covis_walk.h"

namespace {
struct Reader {
    std::vector<unsigned char> buf;
    size_t at = 0;
    bool ok = true;
    const unsigned char *take(size_t n) {
        if (at + n > buf.size()) { ok = false; at = buf.size(); return nullptr; }
        const unsigned char *p = buf.data() + at;
        at += n;
        return p;
    }
    template <class T> std::vector<T> words(size_t n) { // n elements of 4 bytes each
        std::vector<T> v(n);
        const unsigned char *p = take(4 * n);
        if (p && n) memcpy(v.data(), p, 4 * n);
        return v;
    }
    std::vector<uint8_t> bytes(size_t n) { // n bytes, padded to whole words
        std::vector<uint8_t> v(n);
        const unsigned char *p = take((n + 3) / 4 * 4);
        if (p && n) memcpy(v.data(), p, n);
        return v;
    }
};
struct Writer {
    std::vector<int> out;
    template <class T> void put(const std::vector<T> &v, size_t n) { for (size_t i = 0; i < n; i++) out.push_back((int)v[i]); }
};
} // namespace

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    Reader r;
    if (FILE *f = fopen(argv[1], "rb")) {
        unsigned char chunk[65536];
        size_t n;
        while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) r.buf.insert(r.buf.end(), chunk, chunk + n);
        fclose(f);
    } else { perror(argv[1]); return 2; }
    const std::vector<int> head = r.words<int>(4);
    if (!r.ok || head[1] < 0 || head[2] < 0 || head[3] < 0) { fprintf(stderr, "short or malformed input\n"); return 2; }
    const int kind = head[0];
    const size_t np = (size_t)head[2], n_obs = (size_t)head[3];
    const std::vector<int> obs_off = r.words<int>(np + 1), obs_kf = r.words<int>(n_obs), obs_octave = r.words<int>(n_obs);
    const std::vector<uint8_t> obs_stereo = r.bytes(n_obs);
    const std::vector<int> mp_nobs = r.words<int>(np);
    const std::vector<uint8_t> mp_flags = r.bytes(np);
    const covis_table t{head[1], head[2], obs_off.data(), obs_kf.data(), obs_octave.data(), obs_stereo.data(), mp_nobs.data(), mp_flags.data()};
    Writer w;
    int status = 0;
    if (kind == 0) {
        const std::vector<int> h = r.words<int>(4);
        if (!r.ok || h[0] < 0 || h[1] < 0) { fprintf(stderr, "short input\n"); return 2; }
        const size_t nq = (size_t)h[0];
        const std::vector<int> query = r.words<int>(nq), kf_off = r.words<int>(nq + 1), kf_mp = r.words<int>((size_t)h[1]);
        if (!r.ok) { fprintf(stderr, "short input\n"); return 2; }
        std::vector<int> cnt_off(nq + 1), ord_off(nq + 1), kf_max(nq + 1), w_max(nq + 1), none(1);
        // sized like a caller would: a first call without room, then the sizes it reports
        status = covis_update_host(&t, h[0], query.data(), kf_off.data(), kf_mp.data(), h[2], h[3], 0, cnt_off.data(), none.data(), none.data(), kf_max.data(), w_max.data(),
                                   ord_off.data(), none.data(), none.data());
        const size_t cap = status == -4 ? (size_t)cnt_off[nq] : 0;
        std::vector<int> cnt_kf(cap + 1), cnt_w(cap + 1), ord_kf(cap + 1), ord_w(cap + 1);
        if (status == -4)
            status = covis_update_host(&t, h[0], query.data(), kf_off.data(), kf_mp.data(), h[2], h[3], (int)cap, cnt_off.data(), cnt_kf.data(), cnt_w.data(), kf_max.data(),
                                       w_max.data(), ord_off.data(), ord_kf.data(), ord_w.data());
        if (status == 0) {
            w.put(cnt_off, nq + 1); w.put(cnt_kf, (size_t)cnt_off[nq]); w.put(cnt_w, (size_t)cnt_off[nq]); w.put(kf_max, nq); w.put(w_max, nq);
            w.put(ord_off, nq + 1); w.put(ord_kf, (size_t)ord_off[nq]); w.put(ord_w, (size_t)ord_off[nq]);
        }
    } else if (kind == 1) {
        const std::vector<int> h = r.words<int>(4);
        if (!r.ok || h[0] < 0 || h[1] < 0) { fprintf(stderr, "short input\n"); return 2; }
        const size_t nl = (size_t)h[0], ns = (size_t)h[1];
        const std::vector<int> local = r.words<int>(nl), kf_off = r.words<int>(nl + 1), kf_mp = r.words<int>(ns), slot_octave = r.words<int>(ns);
        const std::vector<float> slot_depth = r.words<float>(ns), th_depth = r.words<float>(nl);
        const std::vector<uint8_t> kf_flags = r.bytes(nl);
        if (!r.ok) { fprintf(stderr, "short input\n"); return 2; }
        std::vector<uint8_t> verdict(nl + 1), flags(np + 1), alive(n_obs + 1);
        std::vector<int> mps(nl + 1), red(nl + 1), nobs(np + 1);
        status = covis_keyframe_culling_host(&t, h[0], local.data(), kf_off.data(), kf_mp.data(), slot_octave.data(), slot_depth.data(), th_depth.data(), h[2], kf_flags.data(), h[3],
                                             verdict.data(), mps.data(), red.data(), nobs.data(), flags.data(), alive.data(), nullptr);
        if (status == 0) { w.put(verdict, nl); w.put(mps, nl); w.put(red, nl); w.put(nobs, np); w.put(flags, np); w.put(alive, n_obs); }
    } else if (kind == 2) {
        const std::vector<int> h = r.words<int>(3);
        if (!r.ok || h[0] < 0) { fprintf(stderr, "short input\n"); return 2; }
        const size_t nr = (size_t)h[0];
        const std::vector<int> recent = r.words<int>(nr), found = r.words<int>(np), visible = r.words<int>(np), first = r.words<int>(np);
        if (!r.ok) { fprintf(stderr, "short input\n"); return 2; }
        std::vector<uint8_t> cases(nr + 1);
        status = covis_mappoint_culling_host(&t, h[0], recent.data(), found.data(), visible.data(), first.data(), h[1], h[2], cases.data());
        if (status == 0) w.put(cases, nr);
    } else { fprintf(stderr, "unknown kind %d\n", kind); return 2; }
    if (status != 0) { fprintf(stderr, "the walk returned %d\n", status); return 3; }
    FILE *f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (!w.out.empty()) fwrite(w.out.data(), sizeof(int), w.out.size(), f);
    fclose(f);
    return 0;
}
