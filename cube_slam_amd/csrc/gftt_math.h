// gftt_math.h -- the arithmetic of cv::goodFeaturesToTrack(raw_img, corners, 200, 0.1, 10, good_mask) and of the mask and the new points around it in
// Tracking::CreateNewKeyFrame (reference orb_object_slam/src/Tracking.cc:2263-2331, KeyFrame::UnprojectPixelDepth src/KeyFrame.cc:711-727), one text for the kernels of
// gftt.hip, the library's path without a context and cubeslam::goodFeaturesToTrack / Tracking::CreateNewHarrisFeatures (host/, with or without the library).  OpenCV is
// not part of the reference tree: the definition is the plain C++ (non-SIMD) branches of OpenCV 3.4 featuredetect.cpp, corner.cpp, deriv.cpp, smooth.cpp and
// drawing.cpp as INTEGRATION.md 4e states them (8 bits, one channel, blockSize 3, Sobel aperture 3, minimum eigenvalue).  Every statement is one float operation in
// the written order, or one double accumulation with one rounding.  Built with -ffp-contract=off, as everything that includes this header is.
#pragma once
#include <math.h>
#include <stdint.h>

#include "cv_math.h"
#include "hd.h"
#include "klt_math.h" // klt_reflect101, klt_round

#include <algorithm>
#include <vector>

constexpr int GFTT_MAX_CANDIDATES = 8192; // = CS_GFTT_MAX_CANDIDATES: a frame's keys are sorted in one workgroup's LDS (64 KiB)
constexpr int GFTT_DISC_R = 10;           // MIN_DIST of Tracking.cc:2263, the radius of cv::circle at :2285
constexpr float GFTT_S = (float)(1.0 / (4 * 3 * 255)), GFTT_2S = GFTT_S * 2.f; // the Sobel scale of cornerEigenValsVecs: 1 / (2^(aperture - 1) * blockSize * 255)

// ---- derivatives: Sobel 3 x 3 as the separable row and column filters evaluate it.  p = the pixel, the neighbours at +-1 are its REFLECT_101 neighbours
// (xm / xp, the rows ym / yp): img is the dense or strided image itself.
HD float gftt_row_dx(const uint8_t *row, int xm, int xp) { return (float)((int)row[xp] - (int)row[xm]); }
HD float gftt_row_dy(const uint8_t *row, int x, int xm, int xp) { return (float)row[x] * GFTT_2S + (float)((int)row[xm] + (int)row[xp]) * GFTT_S; }
HD float gftt_dx(float r_up, float r_mid, float r_down) { return (r_up + r_down) * GFTT_S + r_mid * GFTT_2S; }
HD float gftt_dy(float q_up, float q_down) { return q_down - q_up; }
// cov = (Dx Dx, Dx Dy, Dy Dy) at the pixel (x, y) INSIDE the image
HD void gftt_cov(const uint8_t *img, long stride, int w, int h, int x, int y, float *cov) {
    const int xm = klt_reflect101(x - 1, w), xp = klt_reflect101(x + 1, w);
    const uint8_t *up = img + (long)klt_reflect101(y - 1, h) * stride, *mid = img + (long)y * stride, *down = img + (long)klt_reflect101(y + 1, h) * stride;
    const float dx = gftt_dx(gftt_row_dx(up, xm, xp), gftt_row_dx(mid, xm, xp), gftt_row_dx(down, xm, xp));
    const float dy = gftt_dy(gftt_row_dy(up, x, xm, xp), gftt_row_dy(down, x, xm, xp));
    cov[0] = dx * dx; cov[1] = dx * dy; cov[2] = dy * dy;
}
// one row of the unnormalised 3 x 3 box: left to right, in double
HD double gftt_box_row(float l, float m, float r) { return ((double)l + (double)m) + (double)r; }
// ... the three rows top to bottom, one rounding
HD float gftt_box(double top, double mid, double bottom) { return (float)((top + mid) + bottom); }
// calcMinEigenVal on the three box sums
HD float gftt_min_eig(float c0, float c1, float c2) {
    const float a = c0 * 0.5f, b = c1, c = c2 * 0.5f;
    return (a + c) - sqrtf((a - c) * (a - c) + b * b);
}
// an int that orders as the float does (-0 below +0), for the masked maximum; GFTT_NO_MAX: no pixel yet
constexpr int GFTT_NO_MAX = INT32_MIN;
HD int gftt_ordered_int(float v) { union { float f; int32_t i; } u; u.f = v; return u.i >= 0 ? u.i : u.i ^ 0x7fffffff; }
HD float gftt_from_ordered_int(int k) { union { float f; int32_t i; } u; u.i = k >= 0 ? k : k ^ 0x7fffffff; return k == GFTT_NO_MAX ? 0.f : u.f; }
// threshold(eig, eig, maxVal * qualityLevel, 0, THRESH_TOZERO): the product in double, the threshold a float
HD float gftt_threshold(float max_val, double quality_level) { return (float)((double)max_val * quality_level); }
HD float gftt_tozero(float eig, float t) { return eig > t ? eig : 0.f; }
// The sort key of a candidate: descending keys are e' descending and, among equal values, the higher raster index first (greaterThanPtr of 3.4 compares the
// pointers of equal values).  The upper word orders as the float does, negative values included (a candidate's e' is positive; the key does not rely on it).
HD unsigned long long gftt_key(float e, int raster) {
    union { float f; uint32_t u; } v; v.f = e;
    const uint32_t o = v.u & 0x80000000u ? ~v.u : v.u | 0x80000000u;
    return ((unsigned long long)o << 32) | (uint32_t)raster;
}
HD float gftt_key_value(unsigned long long key) {
    const uint32_t o = (uint32_t)(key >> 32);
    union { float f; uint32_t u; } v; v.u = o & 0x80000000u ? o & 0x7fffffffu : ~o;
    return v.f;
}
HD int gftt_key_raster(unsigned long long key) { return (int)(uint32_t)key; }
// the distance test of the greedy walk between two pixels: float differences and products, compared with minDistance^2 (a double) strictly
HD bool gftt_too_close(int x, int y, int ax, int ay, double min_dist2) {
    const float dx = (float)x - (float)ax, dy = (float)y - (float)ay;
    return (double)(dx * dx + dy * dy) < min_dist2;
}

// ---- the filled disc of cv::circle(img, c, 10, 0, -1): the midpoint walk of drawing.cpp's Circle(); hw[k] = the half-width of the rows at |offset| k
struct GfttDisc { int hw[GFTT_DISC_R + 1]; };
constexpr GfttDisc gftt_disc_walk() {
    GfttDisc d{};
    for (int k = 0; k <= GFTT_DISC_R; k++) d.hw[k] = -1;
    int err = 0, dx = GFTT_DISC_R, dy = 0, plus = 1, minus = (GFTT_DISC_R << 1) - 1;
    while (dx >= dy) {
        if (dx > d.hw[dy]) d.hw[dy] = dx; // the spans [cx - dx, cx + dx] on the rows cy -+ dy
        if (dy > d.hw[dx]) d.hw[dx] = dy; // ... and [cx - dy, cx + dy] on the rows cy -+ dx
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
    return d;
}
constexpr GfttDisc GFTT_DISC = gftt_disc_walk();
static_assert(GFTT_DISC.hw[0] == 10 && GFTT_DISC.hw[1] == 9 && GFTT_DISC.hw[4] == 9 && GFTT_DISC.hw[5] == 8 && GFTT_DISC.hw[6] == 8 && GFTT_DISC.hw[7] == 7 && GFTT_DISC.hw[8] == 6 &&
                  GFTT_DISC.hw[9] == 4 && GFTT_DISC.hw[10] == 0, "the walk's half-widths");
HD int gftt_disc_half_width(int k) { // (a table in the instruction stream: a constexpr object is not addressable from a kernel)
    constexpr GfttDisc d = gftt_disc_walk();
    switch (k) {
    case 0: return d.hw[0]; case 1: return d.hw[1]; case 2: return d.hw[2]; case 3: return d.hw[3]; case 4: return d.hw[4]; case 5: return d.hw[5];
    case 6: return d.hw[6]; case 7: return d.hw[7]; case 8: return d.hw[8]; case 9: return d.hw[9]; default: return d.hw[10];
    }
}
constexpr int GFTT_DISC_SIDE = 2 * GFTT_DISC_R + 1, GFTT_DISC_BOX = GFTT_DISC_SIDE * GFTT_DISC_SIDE;
// pixel k of the disc's 21 x 21 box around (cx, cy): true = it is drawn and lies in the image, *idx its raster index
HD bool gftt_disc_pixel(int k, int cx, int cy, int cols, int rows, long *idx) {
    const int oy = k / GFTT_DISC_SIDE - GFTT_DISC_R, ox = k % GFTT_DISC_SIDE - GFTT_DISC_R;
    const int hw = gftt_disc_half_width(oy < 0 ? -oy : oy);
    const long x = (long)cx + ox, y = (long)cy + oy;
    if ((ox < 0 ? -ox : ox) > hw || x < 0 || x >= cols || y < 0 || y >= rows) return false;
    *idx = y * cols + x;
    return true;
}
// good_mask.at<uchar>(Point2f) of Tracking.cc:2283: the index cvRound(y) * cols + cvRound(x), with no bounds test in front of it
HD long gftt_point_index(float x, float y, int cols, int *rx, int *ry) {
    *rx = klt_round(x); *ry = klt_round(y);
    return (long)*ry * cols + *rx;
}
constexpr float GFTT_POINT_LIMIT = 1e9f; // an existing point beyond it is refused: cvRound of it would leave an int
HD bool gftt_point_ok(float v) { return v - v == 0 && v > -GFTT_POINT_LIMIT && v < GFTT_POINT_LIMIT; }

// ---- the new points (Tracking.cc:2308-2331): KeyFrame::UnprojectPixelDepth of a corner at its cuboid's depth.  Twc: the 3 x 4 rows.  Returns x3D_valid.
HD int gftt_unproject(float u, float v, float z, const float *K4, const float *Twc, float *x3D) {
    x3D[0] = x3D[1] = x3D[2] = 0.f;
    if (!(z > 0)) return 0;
    const float invfx = 1.0f / K4[0], invfy = 1.0f / K4[1];
    const float xc[3] = {(u - K4[2]) * z * invfx, (v - K4[3]) * z * invfy, z};
    const float R[9] = {Twc[0], Twc[1], Twc[2], Twc[4], Twc[5], Twc[6], Twc[8], Twc[9], Twc[10]}, t[3] = {Twc[3], Twc[7], Twc[11]};
    gemm3(R, xc, t, x3D); // Twc.rowRange(0, 3).colRange(0, 3) * x3Dc + Twc.rowRange(0, 3).col(3)
    return 1;
}

// ---- host ----
// eig of one image (w, h >= 3) into eig[h * w]
inline void gftt_eig_host(const uint8_t *img, long stride, int w, int h, float *eig) {
    std::vector<float> cov((size_t)3 * w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) gftt_cov(img, stride, w, h, x, y, &cov[3 * ((size_t)y * w + x)]);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float s[3];
            for (int c = 0; c < 3; c++) {
                double rows[3];
                for (int j = -1; j <= 1; j++) { // the border takes cov at the REFLECT_101 coordinate
                    const float *r = &cov[3 * (size_t)klt_reflect101(y + j, h) * w + c];
                    rows[j + 1] = gftt_box_row(r[3 * klt_reflect101(x - 1, w)], r[3 * x], r[3 * klt_reflect101(x + 1, w)]);
                }
                s[c] = gftt_box(rows[0], rows[1], rows[2]);
            }
            eig[(size_t)y * w + x] = gftt_min_eig(s[0], s[1], s[2]);
        }
}
// The greedy walk over sorted keys: a candidate is accepted unless an accepted corner lies nearer than minDistance.  OpenCV looks for that corner in a grid of
// cells of cvRound(minDistance) pixels, in the candidate's cell and the eight around it; two pixels nearer than minDistance are at most cvRound(minDistance) apart in
// x and in y, hence in neighbouring cells, so the walk over every accepted corner gives the same answer.  Returns the corners accepted.
inline int gftt_select_host(const unsigned long long *keys, int n, int w, int max_corners, double min_distance, float *corners, float *quality) {
    const double md2 = min_distance * min_distance;
    std::vector<int> ax, ay;
    for (int i = 0; i < n && (int)ax.size() < max_corners; i++) {
        const int r = gftt_key_raster(keys[i]), x = r % w, y = r / w;
        bool good = true;
        for (size_t k = 0; k < ax.size() && good; k++) good = !gftt_too_close(x, y, ax[k], ay[k], md2);
        if (!good) continue;
        corners[2 * ax.size()] = (float)x; corners[2 * ax.size() + 1] = (float)y;
        if (quality) quality[ax.size()] = gftt_key_value(keys[i]);
        ax.push_back(x); ay.push_back(y);
    }
    return (int)ax.size();
}
// cv::goodFeaturesToTrack of one image.  mask: dense w x h or nullptr.  corners: 2 * max_corners floats, quality: max_corners floats or nullptr.  *count = the corners,
// *n_candidates = the candidates; false = more candidates than GFTT_MAX_CANDIDATES (nothing is selected then).
inline bool gftt_good_features_host(const uint8_t *img, long stride, int w, int h, const uint8_t *mask, int max_corners, double quality_level, double min_distance, float *corners,
                                    float *quality, int *count, int *n_candidates) {
    *count = 0; *n_candidates = 0;
    if (w < 3 || h < 3) return true;
    std::vector<float> eig((size_t)w * h);
    gftt_eig_host(img, stride, w, h, eig.data());
    int mx = GFTT_NO_MAX;
    for (size_t i = 0; i < eig.size(); i++)
        if (!mask || mask[i]) mx = std::max(mx, gftt_ordered_int(eig[i]));
    const float t = gftt_threshold(gftt_from_ordered_int(mx), quality_level);
    std::vector<unsigned long long> keys;
    for (int y = 1; y < h - 1; y++)
        for (int x = 1; x < w - 1; x++) {
            const long i = (long)y * w + x;
            const float e = gftt_tozero(eig[i], t);
            if (e == 0 || (mask && !mask[i])) continue;
            bool is_max = true;
            for (int j = -1; j <= 1; j++)
                for (int k = -1; k <= 1; k++) is_max = is_max && !(gftt_tozero(eig[i + (long)j * w + k], t) > e);
            if (is_max) keys.push_back(gftt_key(e, (int)i));
        }
    *n_candidates = (int)keys.size();
    if (keys.size() > (size_t)GFTT_MAX_CANDIDATES) return false;
    std::sort(keys.begin(), keys.end(), [](unsigned long long a, unsigned long long b) { return a > b; });
    *count = gftt_select_host(keys.data(), (int)keys.size(), w, max_corners, min_distance, corners, quality);
    return true;
}
// Existing points in the order of the walk: observations descending, equal counts by ascending index
inline std::vector<int> gftt_point_order(int n, const int *obs) {
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [obs](int a, int b) { return obs[a] > obs[b]; });
    return order;
}
// Tracking.cc:2265-2287: good = objmask > 0 ? 255 : 0, then the discs around the existing points (pts in the order of the walk).  Returns the points whose index
// lies outside the image.
inline int gftt_build_mask_host(const uint8_t *objmask, int cols, int rows, int n, const float *pts, uint8_t *good) {
    const long total = (long)rows * cols;
    for (long i = 0; i < total; i++) good[i] = objmask[i] > 0 ? 255 : 0;
    int outside = 0;
    for (int i = 0; i < n; i++) {
        int rx, ry;
        const long idx = gftt_point_index(pts[2 * (size_t)i], pts[2 * (size_t)i + 1], cols, &rx, &ry);
        if (idx < 0 || idx >= total) { outside++; continue; }
        if (good[idx] != 255) continue;
        for (int k = 0; k < GFTT_DISC_BOX; k++) {
            long at;
            if (gftt_disc_pixel(k, rx, ry, cols, rows, &at)) good[at] = 0;
        }
    }
    return outside;
}
// Tracking.cc:2308-2331 for the corners of one frame.  false = an object id at or beyond n_cuboids.
inline bool gftt_new_points_host(int n, const float *corners, const uint8_t *objmask, int cols, const float *K4, const float *Twc, int n_cuboids, const float *cuboid_depth,
                                 int *object_id, float *x3D, uint8_t *valid) {
    for (int i = 0; i < n; i++) {
        const int id = (int)objmask[(long)corners[2 * (size_t)i + 1] * cols + (long)corners[2 * (size_t)i]] - 1;
        if (id < 0 || id >= n_cuboids) return false;
        object_id[i] = id;
        valid[i] = (uint8_t)gftt_unproject(corners[2 * (size_t)i], corners[2 * (size_t)i + 1], cuboid_depth[id], K4, Twc, x3D + 3 * (size_t)i);
    }
    return true;
}
// The whole of :2263-2331 for one frame.  exist_pts / exist_obs: the frame's existing points as the caller has them (unsorted).  good: w * h bytes (the mask that was
// built, an output).  Returns 0, 1 for more candidates than the capacity, 2 for an object id beyond the cuboids.
inline int gftt_new_harris_features_host(const uint8_t *img, long stride, int w, int h, const uint8_t *objmask, int n_exist, const float *exist_pts, const int *exist_obs,
                                         const float *K4, const float *Twc, int n_cuboids, const float *cuboid_depth, uint8_t *good, float *new_pts, int *object_id, float *x3D,
                                         uint8_t *valid, int *n_new, int *n_candidates, int *n_mask_outside) {
    const std::vector<int> order = gftt_point_order(n_exist, exist_obs);
    std::vector<float> sorted(2 * (size_t)n_exist);
    for (int i = 0; i < n_exist; i++) { sorted[2 * (size_t)i] = exist_pts[2 * (size_t)order[(size_t)i]]; sorted[2 * (size_t)i + 1] = exist_pts[2 * (size_t)order[(size_t)i] + 1]; }
    *n_mask_outside = gftt_build_mask_host(objmask, w, h, n_exist, sorted.data(), good);
    if (!gftt_good_features_host(img, stride, w, h, good, 200, 0.1, (double)GFTT_DISC_R, new_pts, nullptr, n_new, n_candidates)) return 1;
    return gftt_new_points_host(*n_new, new_pts, objmask, w, K4, Twc, n_cuboids, cuboid_depth, object_id, x3D, valid) ? 0 : 2;
}
