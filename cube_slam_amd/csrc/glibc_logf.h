// glibc_logf.h -- logf with the results of glibc >= 2.27 (sysdeps/ieee754/flt-32/e_logf.c: the table-driven double-precision form of the Arm optimized
// routines), for code that runs on the device and has to agree with a host that calls log(float) under `using namespace std` (MapPoint::PredictScale,
// reference orb_object_slam/src/MapPoint.cc:524-533: ceil(log(ratio) / logScaleFactor) -- a level off by one changes the search radius and the level filter).
//
// The device's own logf is not glibc's.  This restatement -- same table, same polynomial, evaluated in the same order in IEEE doubles -- equals glibc 2.35's logf
// on every positive normal float, with or without FMA contraction (tests/cpp/logf_check.cpp walks them against the host's libm: all 2 130 706 432 in the slow
// variant, a strided sample plus the level boundaries 1.2^k by default).
// Domain: positive normal floats.  Zero, subnormals, negatives, inf and NaN are the caller's to keep out (match_project_map drops such a ratio).
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define GL_FN __host__ __device__ inline
#else
#define GL_FN inline
#endif

namespace glibc_logf {
GL_FN bool in_domain(float x) { uint32_t u; memcpy(&u, &x, 4); return u >= 0x00800000u && u < 0x7f800000u; } // a positive normal float
GL_FN void entry(int i, double *invc, double *logc) { // {invc, logc} of __logf_data.tab (a switch: no table in constant memory, usable from host and device)
    switch (i) {
    case 0: *invc = 0x1.661ec79f8f3bep+0; *logc = -0x1.57bf7808caadep-2; break;
    case 1: *invc = 0x1.571ed4aaf883dp+0; *logc = -0x1.2bef0a7c06ddbp-2; break;
    case 2: *invc = 0x1.49539f0f010bp+0; *logc = -0x1.01eae7f513a67p-2; break;
    case 3: *invc = 0x1.3c995b0b80385p+0; *logc = -0x1.b31d8a68224e9p-3; break;
    case 4: *invc = 0x1.30d190c8864a5p+0; *logc = -0x1.6574f0ac07758p-3; break;
    case 5: *invc = 0x1.25e227b0b8eap+0; *logc = -0x1.1aa2bc79c81p-3; break;
    case 6: *invc = 0x1.1bb4a4a1a343fp+0; *logc = -0x1.a4e76ce8c0e5ep-4; break;
    case 7: *invc = 0x1.12358f08ae5bap+0; *logc = -0x1.1973c5a611cccp-4; break;
    case 8: *invc = 0x1.0953f419900a7p+0; *logc = -0x1.252f438e10c1ep-5; break;
    case 9: *invc = 0x1p+0; *logc = 0x0p+0; break;
    case 10: *invc = 0x1.e608cfd9a47acp-1; *logc = 0x1.aa5aa5df25984p-5; break;
    case 11: *invc = 0x1.ca4b31f026aap-1; *logc = 0x1.c5e53aa362eb4p-4; break;
    case 12: *invc = 0x1.b2036576afce6p-1; *logc = 0x1.526e57720db08p-3; break;
    case 13: *invc = 0x1.9c2d163a1aa2dp-1; *logc = 0x1.bc2860d22477p-3; break;
    case 14: *invc = 0x1.886e6037841edp-1; *logc = 0x1.1058bc8a07ee1p-2; break;
    default: *invc = 0x1.767dcf5534862p-1; *logc = 0x1.4043057b6ee09p-2; break;
    }
}
GL_FN float logf_(float x) {
    const double Ln2 = 0x1.62e42fefa39efp-1, A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
    uint32_t ix; memcpy(&ix, &x, 4);
    if (ix == 0x3f800000u) return 0.0f;
    // x = 2^k z, z in [0x1.66p-1, 0x1.66p0) (OFF = 0x3f330000), split into 16 subintervals; log(x) = log1p(z/c - 1) + log(c) + k Ln2
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) % 16u);
    const int k = (int32_t)tmp >> 23;
    const uint32_t iz = ix - (tmp & 0xff800000u);
    float zf; memcpy(&zf, &iz, 4);
    double invc, logc; entry(i, &invc, &logc);
    const double z = (double)zf;
    const double r = z * invc - 1;
    const double y0 = logc + (double)k * Ln2;
    const double r2 = r * r;
    double y = A1 * r + A2;
    y = A0 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}
} // namespace glibc_logf
