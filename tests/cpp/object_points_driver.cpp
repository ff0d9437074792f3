// TEST INFRASTRUCTURE: cube_slam_amd/csrc/object_points_math.h as a stand-alone program, so that the text the kernels of object_points.hip run can be built with plain g++ and
// again under -fsanitize=address,undefined (tests/test_object_points_mirrors.py).  It reads one case in the format of tests/object_points_patterns.py dump() and writes the
// outputs one behind the other in the order of TRI_KEYS / OD_KEYS.  The arrays are copied into vectors of their exact size, so that a read past an end is the sanitizer's finding.
//   object_points_driver in.bin out.bin
#include <cstdio>
#include <cstring>
#include <vector>

#include "object_points_math.h"

struct Reader {
    std::vector<unsigned char> buf;
    size_t pos = 0;
    bool ok = true;
    template <class T> std::vector<T> take(size_t n) {
        std::vector<T> v(n);
        if (pos + n * sizeof(T) > buf.size()) { ok = false; return v; }
        if (n) memcpy(v.data(), buf.data() + pos, n * sizeof(T));
        pos += n * sizeof(T);
        return v;
    }
};
struct Writer {
    std::vector<unsigned char> out;
    template <class T> void put(const std::vector<T> &v) { const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data()); out.insert(out.end(), p, p + v.size() * sizeof(T)); }
};

static void run_tri(Reader &r, int n_pairs, int use_truth, Writer &w) {
    const size_t F = (size_t)n_pairs;
    const std::vector<int> first = r.take<int>(F + 1);
    const std::vector<float> Tl = r.take<float>(12 * F), Tn = r.take<float>(12 * F), K4 = r.take<float>(4 * F);
    const std::vector<int> cfl = r.take<int>(F + 1);
    const std::vector<double> pl = r.take<double>(7 * (size_t)(r.ok ? cfl[F] : 0));
    const std::vector<int> cfn = r.take<int>(F + 1);
    const std::vector<double> pn = r.take<double>(7 * (size_t)(r.ok ? cfn[F] : 0));
    std::vector<int> tl, tn;
    if (use_truth) { tl = r.take<int>((size_t)cfl[F]); tn = r.take<int>((size_t)cfn[F]); }
    const size_t P = r.ok ? (size_t)first[F] : 0;
    const std::vector<float> kp1 = r.take<float>(2 * P), kp2 = r.take<float>(2 * P);
    const std::vector<int> ol = r.take<int>(P), on = r.take<int>(P), il = r.take<int>(P);
    const std::vector<float> wp = r.take<float>(3 * P);
    std::vector<uint8_t> status(P);
    std::vector<float> x3D(3 * P), pto(3 * P);
    std::vector<double> dp(3 * P);
    if (r.ok) {
        const DynTables T = {cfl.data(), cfn.data(), pl.data(), pn.data(), use_truth ? tl.data() : nullptr, use_truth ? tn.data() : nullptr};
        for (int f = 0; f < n_pairs; f++) {
            DynCam cam;
            dyn_make_cam(Tl.data() + 12 * (size_t)f, Tn.data() + 12 * (size_t)f, K4.data() + 4 * (size_t)f, &cam);
            for (int i = first[(size_t)f]; i < first[(size_t)f + 1]; i++) {
                const size_t i2 = 2 * (size_t)i, i3 = 3 * (size_t)i;
                dyn_one(cam, f, T, kp1.data() + i2, kp2.data() + i2, ol[(size_t)i], on[(size_t)i], il[(size_t)i], wp.data() + i3, status.data() + i, x3D.data() + i3, pto.data() + i3,
                        dp.data() + i3);
            }
        }
    }
    w.put(status); w.put(x3D); w.put(pto); w.put(dp);
}

static int run_od(Reader &r, int n_frames, int mode, Writer &w) {
    const size_t F = (size_t)n_frames;
    const std::vector<int> first = r.take<int>(F + 1);
    const size_t n = r.ok ? (size_t)first[F] : 0;
    const std::vector<OdKey> keys = r.take<OdKey>(n);
    const std::vector<uint8_t> has_mp = r.take<uint8_t>(n);
    const std::vector<int> oid = r.take<int>(n), cf = r.take<int>(F + 1);
    const std::vector<float> cd = r.take<float>((size_t)(r.ok ? cf[F] : 0)), K4 = r.take<float>(4 * F), bounds = r.take<float>(4 * F), Twc = r.take<float>(12 * F);
    const std::vector<int> df = r.take<int>(F + 1), draws = r.take<int>((size_t)(r.ok ? df[F] : 0));
    if (!r.ok) return 0;
    std::vector<int> n_cand(F), raw(F), max_init(F), cand_first(F + 1, 0), new_first(F + 1, 0), cand, shuf, new_idx;
    std::vector<float> new_x;
    for (int f = 0; f < n_frames; f++) {
        const size_t b0 = (size_t)first[(size_t)f], N = (size_t)first[(size_t)f + 1] - b0;
        // the frame's own slices, each of its exact size
        const std::vector<OdKey> k(keys.begin() + b0, keys.begin() + b0 + N);
        const std::vector<uint8_t> mp(has_mp.begin() + b0, has_mp.begin() + b0 + N);
        const std::vector<int> id(oid.begin() + b0, oid.begin() + b0 + N), dr(draws.begin() + df[(size_t)f], draws.begin() + df[(size_t)f + 1]);
        const std::vector<float> depth(cd.begin() + cf[(size_t)f], cd.begin() + cf[(size_t)f + 1]);
        std::vector<int> c(N), s(N), ni(N);
        std::vector<float> x(3 * N);
        OdFrameOut o;
        od_frame_host(mode, (int)N, k.data(), mp.data(), id.data(), depth.data(), K4.data() + 4 * (size_t)f, bounds.data() + 4 * (size_t)f, Twc.data() + 12 * (size_t)f,
                      mode == OD_FIRST_FRAME ? 0 : (int)dr.size(), dr.data(), &o, c.data(), s.data(), ni.data(), x.data());
        if (o.short_of_draws) return -2;
        n_cand[(size_t)f] = o.n_candidates; raw[(size_t)f] = o.raw_depth_pts; max_init[(size_t)f] = o.max_initialize_pts;
        cand.insert(cand.end(), c.begin(), c.begin() + o.n_candidates); shuf.insert(shuf.end(), s.begin(), s.begin() + o.n_candidates);
        new_idx.insert(new_idx.end(), ni.begin(), ni.begin() + o.n_new); new_x.insert(new_x.end(), x.begin(), x.begin() + 3 * (size_t)o.n_new);
        cand_first[(size_t)f + 1] = (int)cand.size(); new_first[(size_t)f + 1] = (int)new_idx.size();
    }
    w.put(n_cand); w.put(raw); w.put(max_init); w.put(cand_first); w.put(cand); w.put(shuf); w.put(new_first); w.put(new_idx); w.put(new_x);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    Reader r;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        unsigned char chunk[1 << 16];
        size_t n;
        while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) r.buf.insert(r.buf.end(), chunk, chunk + n);
        fclose(f);
    }
    const std::vector<int> head = r.take<int>(3);
    if (!r.ok || head[1] < 0) { fprintf(stderr, "short input\n"); return 2; }
    Writer w;
    int status = 0;
    if (head[0] == 0) run_tri(r, head[1], head[2], w);
    else status = run_od(r, head[1], head[2], w);
    if (!r.ok || r.pos != r.buf.size()) { fprintf(stderr, "the input does not have the size its counts say\n"); return 2; }
    if (status != 0) { fprintf(stderr, "the walk returned %d\n", status); return 3; }
    FILE *f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (!w.out.empty()) fwrite(w.out.data(), 1, w.out.size(), f);
    fclose(f);
    return 0;
}
