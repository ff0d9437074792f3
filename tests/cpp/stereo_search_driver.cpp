// TEST INFRASTRUCTURE: cube_slam_amd/csrc/stereo_search_math.h as a stand-alone program under plain g++ (tests/test_stereo_search_mirrors.py builds it plainly and with
// -fsanitize=address,undefined).  in.bin: int n, then n records of 24 floats (Tcw 3x4, Tlw 3x4), float mb, int mono, and per record m = 4 probes of the two small predicates:
// int direction, int octave, float ur_query, float u_right, float radius.  out.bin per record: float tlc_z, int direction, then per probe int minLevel, int maxLevel, int drops.
#include <cstdio>
#include <cstring>
#include <vector>

#include "stereo_search_math.h"

namespace {
struct Reader {
    std::vector<unsigned char> buf; size_t at = 0; bool ok = true;
    template <class T> T one() { T v{}; if (at + sizeof(T) > buf.size()) { ok = false; return v; } memcpy(&v, buf.data() + at, sizeof(T)); at += sizeof(T); return v; }
};
struct Writer {
    std::vector<unsigned char> buf;
    template <class T> void put(T v) { const unsigned char *p = reinterpret_cast<const unsigned char *>(&v); buf.insert(buf.end(), p, p + sizeof(T)); }
};
constexpr int PROBES = 4;
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
    const int n = r.one<int>();
    if (!r.ok || n < 0) { fprintf(stderr, "short or malformed input\n"); return 2; }
    Writer w;
    for (int i = 0; i < n; i++) {
        float Tcw[12], Tlw[12];
        for (float &v : Tcw) v = r.one<float>();
        for (float &v : Tlw) v = r.one<float>();
        const float mb = r.one<float>();
        const int mono = r.one<int>();
        if (!r.ok) { fprintf(stderr, "short input\n"); return 2; }
        w.put<float>(stereo_search_tlc_z(Tcw, Tlw));
        w.put<int>(stereo_search_direction(Tcw, mono ? nullptr : Tlw, mb, mono)); // (a monocular search has no last pose to read)
        for (int p = 0; p < PROBES; p++) {
            const int d = r.one<int>(), o = r.one<int>();
            const float urq = r.one<float>(), ur = r.one<float>(), rad = r.one<float>();
            if (!r.ok) { fprintf(stderr, "short input\n"); return 2; }
            int lo = -9, hi = -9;
            stereo_search_levels(d, o, lo, hi);
            w.put<int>(lo); w.put<int>(hi); w.put<int>(stereo_search_drops(urq, ur, rad) ? 1 : 0);
        }
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const bool done = fwrite(w.buf.data(), 1, w.buf.size(), f) == w.buf.size();
    fclose(f);
    return done ? 0 : 2;
}
