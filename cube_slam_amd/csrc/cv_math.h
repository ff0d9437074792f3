// cv_math.h -- the float cv::Mat forms the reference's geometry is written in, as OpenCV evaluates them (the library is built with -ffp-contract=off): a cv::Mat product
// is one gemm per row with double accumulation over k ascending and a single rounding; Mat::dot and cv::norm accumulate in double.  HD: the kernels of match.hip and
// localmap.hip and the CPU drivers under tests/cpp run the same text.
#pragma once
#include <math.h>

#include "hd.h"

#define CVM HD __attribute__((always_inline)) // (the kernels of match.hip had these forced inline before they moved here)

CVM void gemm3(const float *R, const float *p, const float *t, float *o) { // o = R * p + t
    for (int r = 0; r < 3; r++) {
        double sacc = 0;
        for (int k = 0; k < 3; k++) sacc += (double)R[r * 3 + k] * (double)p[k];
        o[r] = (float)(sacc * 1.0 + (double)t[r] * 1.0);
    }
}
CVM double dot3_f64(const float *a, const float *b) { double s = 0; for (int k = 0; k < 3; k++) s += (double)a[k] * (double)b[k]; return s; } // Mat::dot
CVM double norm3_f64(const float *v) { return sqrt(dot3_f64(v, v)); }                                                                          // cv::norm
CVM float norm3(const float *v) { return (float)norm3_f64(v); }                                                                                // const float d = cv::norm(v)
#undef CVM
