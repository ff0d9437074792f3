// TEST INFRASTRUCTURE: driver of cube_slam_amd/host/initializer.hpp for tests/test_initializer_mirrors.py: cubeslam::Initializer without a context, the g++ build of
// csrc/initializer_math.h (built with -DCUBESLAM_HOST_ONLY it links nothing of the library, and a second time with -fsanitize=address,undefined).  Built without that macro
// and linked against the library (tests/test_initializer_host_cpp_gpu.py) every initializer gets a cubeslam::Context and evaluate_many runs on the device.
//   initializer_mirror <in> <out> [draw]
// <in>: int n; per case int n1, n2, H; float sigma, K[9]; keys1[2 n1], keys2[2 n2]; int vMatches12[n1], sets[8 H].  `draw`: every initializer gets a RandomInt that replays
// the case's sets through ransac_draw<8> instead of the table.  All cases are evaluated in one evaluate_many.
// <out>: per case the table in the order of tests/test_initializer_mirrors.py (table_bytes), then success, candidate, parallax, R21, t21 and, on success, vP3D and
// vbTriangulated.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "cube_slam_amd/host/initializer.hpp"

static FILE *in, *out;
template <class T> static std::vector<T> rd(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
template <class T> static void wr(const T *p, size_t n) { if (n) fwrite(p, sizeof(T), n, out); }

struct Replay { // RandomInt over the wanted indices: the position of each in the Fisher-Yates' vAvailableIndices
    std::vector<int> want, avail;
    size_t pos = 0;
    int N = 0;
    int operator()(int lo, int hi) {
        if (pos % 8 == 0) { avail.resize((size_t)N); for (int i = 0; i < N; i++) avail[i] = i; }
        if (pos >= want.size()) { fprintf(stderr, "RandomInt: past the case's sets\n"); exit(3); }
        const int at = (int)(std::find(avail.begin(), avail.end(), want[pos++]) - avail.begin());
        if (lo != 0 || hi != (int)avail.size() - 1 || at > hi) { fprintf(stderr, "RandomInt: not the Fisher-Yates of :83-98\n"); exit(3); }
        avail[at] = avail.back(); avail.pop_back();
        return at;
    }
};

int main(int argc, char **argv) {
    if (argc < 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    const bool draw = argc > 3 && !strcmp(argv[3], "draw");
    const int n = rd<int>(1)[0];
    cubeslam::Context *ctx = nullptr;
#ifndef CUBESLAM_HOST_ONLY
    cubeslam::Context device(0);
    ctx = &device;
#endif
    std::vector<std::unique_ptr<cubeslam::Initializer>> its;
    for (int s = 0; s < n; s++) {
        const std::vector<int> h = rd<int>(3);
        const std::vector<float> sk = rd<float>(10);
        std::vector<float> keys1 = rd<float>(2 * (size_t)h[0]), keys2 = rd<float>(2 * (size_t)h[1]);
        const std::vector<int> vMatches12 = rd<int>((size_t)h[0]), sets = rd<int>(8 * (size_t)h[2]);
        its.emplace_back(new cubeslam::Initializer(keys1, sk.data() + 1, sk[0], h[2], ctx));
        cubeslam::Initializer &it = *its.back();
        int N = 0;
        for (int m : vMatches12) N += m >= 0;
        if (draw && N >= 8) {
            auto r = std::make_shared<Replay>();
            r->N = N; r->want = sets;
            it.set_random_int([r](int lo, int hi) { return (*r)(lo, hi); });
        } else
            it.set_sets(sets);
        it.prepare(keys2, vMatches12);
    }
    std::vector<cubeslam::Initializer *> all;
    for (auto &p : its) all.push_back(p.get());
    cubeslam::Initializer::evaluate_many(all, ctx); // one call for every frame pair
    for (auto &p : its) {
        const cubeslam::Initializer::Table &t = p->table;
        const int head[5] = {t.model, t.best[0], t.best[1], t.n_inliers, t.n_cand};
        wr(head, 5); wr(t.nGood, 8); wr(t.S, 2); wr(&t.RH, 1); wr(t.cand_Rt, 96); wr(t.cos_parallax, 8);
        wr(t.score.data(), t.score.size()); wr(t.matrix.data(), t.matrix.size()); wr(t.mask.data(), t.mask.size());
        wr(t.good_mask.data(), t.good_mask.size()); wr(t.points.data(), t.points.size());
        const cubeslam::Initializer::Result r = p->result();
        const int res[2] = {(int)r.success, r.candidate};
        wr(res, 2); wr(&r.parallax, 1); wr(r.R21, 9); wr(r.t21, 3);
        if (r.success) {
            wr(r.vP3D.data(), r.vP3D.size());
            std::vector<unsigned char> vb(r.vbTriangulated.begin(), r.vbTriangulated.end());
            wr(vb.data(), vb.size());
        }
    }
    fclose(out);
    return 0;
}
