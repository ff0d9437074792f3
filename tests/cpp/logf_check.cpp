// glibc_logf.h against the host's libm: every STRIDE-th positive normal float (argv[1] = stride, 1 = all), every float within 4 ulp of 1.2f^k, k = -2 .. 10 (the level
// boundaries of MapPoint::PredictScale, as the running float product and as powf give them), and quotients a / b with b in [1, 2) and a = b * 1.2f^k (the ratio
// mfMaxDistance / dist at a boundary, with the rounding of the product and of the quotient)
#include "../../cube_slam_amd/csrc/glibc_logf.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
static long n = 0, bad = 0;
static void one(float x) {
    if (!glibc_logf::in_domain(x)) return;
    n++;
    const float a = logf(x), b = glibc_logf::logf_(x);
    uint32_t ua, ub; memcpy(&ua, &a, 4); memcpy(&ub, &b, 4);
    if (ua != ub) { if (bad < 10) printf("logf(%a) = %a, restated %a\n", x, a, b); bad++; }
}
static void around(float x) {
    uint32_t u; memcpy(&u, &x, 4);
    for (int d = -4; d <= 4; d++) { const uint32_t v = u + (uint32_t)d; float y; memcpy(&y, &v, 4); one(y); }
}
int main(int argc, char **argv) {
    const uint32_t stride = argc > 1 ? (uint32_t)atoi(argv[1]) : 97;
    if (stride < 1) return 2;
    for (uint64_t u = 0x00800000u; u < 0x7f800000u; u += stride) { const uint32_t v = (uint32_t)u; float x; memcpy(&x, &v, 4); one(x); }
    const float edge[] = {1.0f, 0x1p-126f, 0x1.fffffep127f, 0x1.66p-1f, 0x1.66p0f, 0.5f, 2.0f};
    for (float x : edge) around(x);
    float pw[13]; // 1.2f^k, k = -2 .. 10
    for (int k = -2; k <= 10; k++) {
        float p = 1.0f;
        for (int j = 0; j < (k < 0 ? -k : k); j++) p = k < 0 ? p / 1.2f : p * 1.2f;
        pw[k + 2] = p;
        around(p); around(powf(1.2f, (float)k)); around((float)pow(1.2, (double)k));
    }
    uint32_t s = 12345u;
    for (int it = 0; it < 200000; it++) {
        s = s * 1664525u + 1013904223u;
        const uint32_t ub = 0x3f800000u | (s >> 9); // b in [1, 2)
        float b; memcpy(&b, &ub, 4);
        for (int k = 0; k < 13; k++) { const float a = b * pw[k]; one(a / b); }
    }
    printf("%ld values, %ld mismatches\n", n, bad);
    return bad != 0;
}
