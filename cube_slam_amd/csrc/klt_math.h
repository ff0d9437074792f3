// klt_math.h -- the arithmetic of cv::calcOpticalFlowPyrLK as ORBmatcher::SearchByTrackingHarris / SearchByTracking call it (reference
// orb_object_slam/src/ORBmatcher.cc:1548 / :1620: 8-bit one-channel images, Size(21, 21), maxLevel 3, default criteria / flags / minEigThreshold), one text for the
// kernels of klt.hip, the library's path without a context and cubeslam::ORBmatcher (host/orb_slam_mirrors.hpp, with or without the library).  OpenCV is not part of
// the reference tree: the definition is the plain C++ (non-SIMD) branches of OpenCV 3.x lkpyramid.cpp as INTEGRATION.md states them.  Every statement is one float
// operation in the written order; the 441-term sums are added in window order.  Built with -ffp-contract=off, as everything that includes this header is.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hd.h"

#include <algorithm>
#include <vector>

constexpr int KLT_WIN = 21, KLT_PAD = 21, KLT_HALF = 10, KLT_MAX_LEVELS = 4, KLT_ITERS = 30, KLT_WN = KLT_WIN * KLT_WIN;
constexpr int KLT_W_BITS = 14;

// One frame's levels in one block: level l is (w[l] + 42) x (h[l] + 42) bytes at img_off[l] of the image block (REFLECT_101 pad materialised) and as many
// (Ix, Iy) int16 pairs at der_off[l] (in pairs) of the derivative block (constant 0 pad).
struct KltLayout {
    int n_levels;
    int w[KLT_MAX_LEVELS], h[KLT_MAX_LEVELS];
    long img_off[KLT_MAX_LEVELS], der_off[KLT_MAX_LEVELS];
    long img_frame, der_frame; // bytes / pairs per frame
};
// buildOpticalFlowPyramid's sizes: level l + 1 is ((w + 1) / 2, (h + 1) / 2); building stops at the first level with w <= 21 || h <= 21
inline KltLayout klt_layout(int width, int height) {
    KltLayout L{};
    int w = width, h = height;
    long io = 0;
    for (int l = 0; l < KLT_MAX_LEVELS; l++) {
        if (l > 0 && (w <= KLT_WIN || h <= KLT_WIN)) break;
        L.w[l] = w; L.h[l] = h; L.img_off[l] = io; L.der_off[l] = io;
        io += (long)(w + 2 * KLT_PAD) * (h + 2 * KLT_PAD);
        L.n_levels = l + 1;
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    L.img_frame = io; L.der_frame = io;
    return L;
}

// cv::borderInterpolate(p, n, BORDER_REFLECT_101) for n > 1 and |p| within a few n
HD int klt_reflect101(int p, int n) {
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}
// cv::pyrDown of 8 bits: [1 4 6 4 1]^2 around (2x, 2y), (sum + 128) >> 8.  src: the w x h interior of the level above, `stride` bytes a row.
HD uint8_t klt_pyrdown_pixel(const uint8_t *src, long stride, int w, int h, int x, int y) {
    const int k[5] = {1, 4, 6, 4, 1};
    int sum = 0;
    for (int i = 0; i < 5; i++) {
        const uint8_t *row = src + (long)klt_reflect101(2 * y + i - 2, h) * stride;
        int r = 0;
        for (int j = 0; j < 5; j++) r += k[j] * row[klt_reflect101(2 * x + j - 2, w)];
        sum += k[i] * r;
    }
    return (uint8_t)((sum + 128) >> 8);
}
// calcSharrDeriv at one pixel.  p points at the pixel inside a level whose REFLECT_101 pad is materialised: the neighbours at +-1 are then the reference's own
// edge rule (row -1 is row 1, column w is column w - 2).
HD void klt_scharr_pixel(const uint8_t *p, long stride, short *ix, short *iy) {
    int t0[3], t1[3];
    for (int c = -1; c <= 1; c++) {
        const int r0 = p[c - stride], r1 = p[c], r2 = p[c + stride];
        t0[c + 1] = (r0 + r2) * 3 + r1 * 10;
        t1[c + 1] = r2 - r0;
    }
    *ix = (short)(t0[2] - t0[0]);
    *iy = (short)((t1[2] + t1[0]) * 3 + t1[1] * 10);
}

HD int klt_floor(float v) { return (int)floorf(v); }            // cvFloor
HD int klt_round(float v) { return (int)rintf(v); }             // cvRound: to nearest, ties to even
HD int klt_descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }
// the window of a point whose top-left sample is (ix, iy) lies in the level and its pad: columns ix .. ix + 21 with ix in [-21, cols - 1]
HD bool klt_in_range(int ix, int iy, int cols, int rows) { return !(ix < -KLT_WIN || ix >= cols || iy < -KLT_WIN || iy >= rows); }
struct KltW { int w00, w01, w10, w11; };
HD KltW klt_weights(float a, float b) {
    KltW W;
    W.w00 = klt_round((1.f - a) * (1.f - b) * (float)(1 << KLT_W_BITS));
    W.w01 = klt_round(a * (1.f - b) * (float)(1 << KLT_W_BITS));
    W.w10 = klt_round((1.f - a) * b * (float)(1 << KLT_W_BITS));
    W.w11 = (1 << KLT_W_BITS) - W.w00 - W.w01 - W.w10;
    return W;
}
// one window sample of the image: p = the top-left tap
HD int klt_sample_img(const uint8_t *p, long stride, const KltW &W) {
    return (short)klt_descale(p[0] * W.w00 + p[1] * W.w01 + p[stride] * W.w10 + p[stride + 1] * W.w11, KLT_W_BITS - 5);
}
// ... and of the derivatives: d = the top-left (Ix, Iy) pair, `stride` pairs a row
HD void klt_sample_deriv(const short *d, long stride, const KltW &W, int *ix, int *iy) {
    const short *e = d + 2 * stride;
    *ix = (short)klt_descale(d[0] * W.w00 + d[2] * W.w01 + e[0] * W.w10 + e[2] * W.w11, KLT_W_BITS);
    *iy = (short)klt_descale(d[1] * W.w00 + d[3] * W.w01 + e[1] * W.w10 + e[3] * W.w11, KLT_W_BITS);
}
HD float klt_term(int a, int b) { return (float)(a * b); } // one term of A11 / A12 / A22 / b1 / b2
constexpr float KLT_FLT_SCALE = 1.f / (1 << 20);
// the spatial gradient matrix after its sums: false = the minEig / determinant rejection; otherwise *Dinv = 1.f / D
HD bool klt_gradient_ok(float A11, float A12, float A22, float *Dinv) {
    const float D = A11 * A22 - A12 * A12;
    const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * KLT_WIN * KLT_WIN);
    if ((double)minEig < 1e-4 || D < 1.1920928955078125e-7f) return false;
    *Dinv = 1.f / D;
    return true;
}
HD void klt_step(float A11, float A12, float A22, float Dinv, float b1, float b2, float *dx, float *dy) {
    *dx = (A12 * b2 - A22 * b1) * Dinv;
    *dy = (A12 * b1 - A11 * b2) * Dinv;
}
HD bool klt_eps_stop(float dx, float dy) { return (double)dx * (double)dx + (double)dy * (double)dy <= 0.01 * 0.01; }
HD bool klt_oscillation_stop(float dx, float dy, float pdx, float pdy) { return (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01; }
HD float klt_err(float sum) { return sum * 1.f / (float)(32 * KLT_WIN * KLT_WIN); }

// cv::Mat::at<uchar>(Point2f) of ORBmatcher.cc:1564 behind the bounds test of :1561: the index cvRound(y) * cols + cvRound(x), which is the next row's first pixel
// when x rounds to cols.  -1: the point fails the bounds test.  An index >= rows * cols lies beyond the image (the caller drops the point and counts it).
HD long klt_mask_index(float x, float y, int cols, int rows) {
    if (!(x >= 0 && y >= 0 && x < (float)cols && y < (float)rows)) return -1;
    return (long)klt_round(y) * cols + klt_round(x);
}

// ---- host ----
// Pyramid and derivatives of one frame into the layout's two blocks (img: L.img_frame bytes, der: 2 * L.der_frame shorts).
inline void klt_build_frame_host(const KltLayout &L, const uint8_t *gray, long stride, uint8_t *img, short *der) {
    for (int l = 0; l < L.n_levels; l++) {
        const int w = L.w[l], h = L.h[l];
        const long ps = w + 2 * KLT_PAD;
        uint8_t *lev = img + L.img_off[l];
        const uint8_t *up = l ? img + L.img_off[l - 1] + (long)KLT_PAD * (L.w[l - 1] + 2 * KLT_PAD) + KLT_PAD : nullptr;
        for (int py = 0; py < h + 2 * KLT_PAD; py++)
            for (int px = 0; px < w + 2 * KLT_PAD; px++) {
                const int x = klt_reflect101(px - KLT_PAD, w), y = klt_reflect101(py - KLT_PAD, h);
                lev[py * ps + px] = l ? klt_pyrdown_pixel(up, L.w[l - 1] + 2 * KLT_PAD, L.w[l - 1], L.h[l - 1], x, y) : gray[(long)y * stride + x];
            }
        short *d = der + 2 * L.der_off[l];
        for (int py = 0; py < h + 2 * KLT_PAD; py++)
            for (int px = 0; px < w + 2 * KLT_PAD; px++) {
                short ix = 0, iy = 0;
                if (px >= KLT_PAD && px < w + KLT_PAD && py >= KLT_PAD && py < h + KLT_PAD) klt_scharr_pixel(lev + py * ps + px, ps, &ix, &iy);
                d[2 * (py * ps + px)] = ix; d[2 * (py * ps + px) + 1] = iy;
            }
    }
}
// One point through every level, written as the reference's loop.  prev_img / prev_der / next_img: the frame blocks of klt_build_frame_host.
inline void klt_track_point_host(const KltLayout &L, const uint8_t *prev_img, const short *prev_der, const uint8_t *next_img, float ptx, float pty, float *out_x, float *out_y,
                                 uint8_t *status, float *err) {
    short I[KLT_WN], Ix[KLT_WN], Iy[KLT_WN];
    float nextx = 0, nexty = 0; // nextPts[ptidx]
    *status = 1; *err = 0;
    for (int level = L.n_levels - 1; level >= 0; level--) {
        const int cols = L.w[level], rows = L.h[level];
        const long ps = cols + 2 * KLT_PAD;
        const uint8_t *Ip = prev_img + L.img_off[level], *Jp = next_img + L.img_off[level];
        const short *Dp = prev_der + 2 * L.der_off[level];
        float px = ptx * (float)(1. / (1 << level)), py = pty * (float)(1. / (1 << level));
        float nx, ny;
        if (level == L.n_levels - 1) { nx = px; ny = py; } else { nx = nextx * 2.f; ny = nexty * 2.f; }
        nextx = nx; nexty = ny;
        px -= (float)KLT_HALF; py -= (float)KLT_HALF;
        int ix = klt_floor(px), iy = klt_floor(py);
        if (!klt_in_range(ix, iy, cols, rows)) {
            if (level == 0) { *status = 0; *err = 0; }
            continue;
        }
        KltW W = klt_weights(px - (float)ix, py - (float)iy);
        float A11 = 0, A12 = 0, A22 = 0;
        for (int y = 0; y < KLT_WIN; y++)
            for (int x = 0; x < KLT_WIN; x++) {
                const long o = (long)(iy + KLT_PAD + y) * ps + ix + KLT_PAD + x; // ix + 21 in [0, cols + 20]: columns o .. o + 1 and rows .. + 1 stay inside the padded level
                int gx, gy;
                klt_sample_deriv(Dp + 2 * o, ps, W, &gx, &gy);
                const int k = y * KLT_WIN + x;
                I[k] = (short)klt_sample_img(Ip + o, ps, W); Ix[k] = (short)gx; Iy[k] = (short)gy;
                A11 += klt_term(gx, gx); A12 += klt_term(gx, gy); A22 += klt_term(gy, gy);
            }
        A11 *= KLT_FLT_SCALE; A12 *= KLT_FLT_SCALE; A22 *= KLT_FLT_SCALE;
        float Dinv;
        if (!klt_gradient_ok(A11, A12, A22, &Dinv)) {
            if (level == 0) *status = 0;
            continue;
        }
        nx -= (float)KLT_HALF; ny -= (float)KLT_HALF;
        float pdx = 0, pdy = 0;
        for (int j = 0; j < KLT_ITERS; j++) {
            ix = klt_floor(nx); iy = klt_floor(ny);
            if (!klt_in_range(ix, iy, cols, rows)) {
                if (level == 0) *status = 0;
                break;
            }
            W = klt_weights(nx - (float)ix, ny - (float)iy);
            float b1 = 0, b2 = 0;
            for (int y = 0; y < KLT_WIN; y++)
                for (int x = 0; x < KLT_WIN; x++) {
                    const int k = y * KLT_WIN + x;
                    const int diff = klt_sample_img(Jp + (long)(iy + KLT_PAD + y) * ps + ix + KLT_PAD + x, ps, W) - I[k];
                    b1 += klt_term(diff, Ix[k]); b2 += klt_term(diff, Iy[k]);
                }
            b1 *= KLT_FLT_SCALE; b2 *= KLT_FLT_SCALE;
            float dx, dy;
            klt_step(A11, A12, A22, Dinv, b1, b2, &dx, &dy);
            nx += dx; ny += dy;
            nextx = nx + (float)KLT_HALF; nexty = ny + (float)KLT_HALF;
            if (klt_eps_stop(dx, dy)) break;
            if (j > 0 && klt_oscillation_stop(dx, dy, pdx, pdy)) {
                nextx -= dx * 0.5f; nexty -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
        if (*status && level == 0) {
            const float ex = nextx - (float)KLT_HALF, ey = nexty - (float)KLT_HALF;
            ix = klt_floor(ex); iy = klt_floor(ey);
            if (!klt_in_range(ix, iy, cols, rows)) { *status = 0; continue; }
            W = klt_weights(ex - (float)ix, ey - (float)iy);
            float sum = 0;
            for (int y = 0; y < KLT_WIN; y++)
                for (int x = 0; x < KLT_WIN; x++) {
                    const int diff = klt_sample_img(Jp + (long)(iy + KLT_PAD + y) * ps + ix + KLT_PAD + x, ps, W) - I[y * KLT_WIN + x];
                    sum += fabsf((float)diff);
                }
            *err = klt_err(sum);
        }
    }
    *out_x = nextx; *out_y = nexty;
}
// calcOpticalFlowPyrLK for the pairs of a call on the host.  frames: n_frames images of width x height, rows `stride` bytes apart, frames `frame_stride` bytes apart.
inline void klt_track_host(const uint8_t *frames, int n_frames, int width, int height, long stride, long frame_stride, int n_pairs, const int *pair_prev, const int *pair_next,
                           const int *first, const float *prev_pts, float *next_pts, uint8_t *status, float *err) {
    const KltLayout L = klt_layout(width, height);
    std::vector<std::vector<uint8_t>> img((size_t)n_frames); // a frame's blocks exist once a pair with points names it
    std::vector<std::vector<short>> der((size_t)n_frames);
    for (int p = 0; p < n_pairs; p++) {
        if (first[p + 1] == first[p]) continue;
        for (int f : {pair_prev[p], pair_next[p]})
            if (img[(size_t)f].empty()) {
                img[(size_t)f].resize((size_t)L.img_frame); der[(size_t)f].resize((size_t)L.der_frame * 2);
                klt_build_frame_host(L, frames + (long)f * frame_stride, stride, img[(size_t)f].data(), der[(size_t)f].data());
            }
        for (int i = first[p]; i < first[p + 1]; i++)
            klt_track_point_host(L, img[(size_t)pair_prev[p]].data(), der[(size_t)pair_prev[p]].data(), img[(size_t)pair_next[p]].data(), prev_pts[2 * (size_t)i],
                                 prev_pts[2 * (size_t)i + 1], next_pts + 2 * (size_t)i, next_pts + 2 * (size_t)i + 1, status + i, err + i);
    }
}
// The selection pass of ORBmatcher::SearchByTrackingHarris (ORBmatcher.cc:1556-1576) over one pair's n tracked points.  kept / pts / object_id: room for n entries.
inline int klt_harris_select_host(int n, const float *cur, const uint8_t *status, const uint8_t *mask, int cols, int rows, int *kept, float *pts, int *object_id, int *n_outside) {
    int good = 0, outside = 0;
    for (int i = 0; i < n; i++) {
        if (!status[i]) continue;
        const long idx = klt_mask_index(cur[2 * i], cur[2 * i + 1], cols, rows);
        if (idx < 0) continue;
        if (idx >= (long)rows * cols) { outside++; continue; }
        if (mask[idx] == 0) continue;
        kept[good] = i; pts[2 * good] = cur[2 * i]; pts[2 * good + 1] = cur[2 * i + 1]; object_id[good] = (int)mask[idx] - 1;
        good++;
    }
    *n_outside = outside;
    return good;
}

// ---- ORBmatcher::SearchByTracking (ORBmatcher.cc:1582-1725) behind the optical flow ----
constexpr int KLT_GRID_COLS = 64, KLT_GRID_ROWS = 48, KLT_NCELL = KLT_GRID_COLS * KLT_GRID_ROWS; // Frame.h:32-33
// The current frame's mGrid as the matcher keeps it: the cells in the order c = ix * 48 + iy, a cell's key points in ascending index (push_back order), one record each
struct KltCellRec { float x, y; int id, octave; };
struct KltGridP { int N; float minX, minY, wInv, hInv; };
// Frame::GetCloestFeaturesInArea (Frame.cc:461-523): cells ix outer, iy inner, strict <, so the first candidate wins a tie.  -1 = the reference's N + 1.
HD int klt_closest_feature(const KltGridP &G, const int *cell_start, const KltCellRec *recs, float x, float y, float r, int minLevel, int maxLevel, const uint8_t *keys_static) {
    const int x0 = (int)floorf((x - G.minX - r) * G.wInv) > 0 ? (int)floorf((x - G.minX - r) * G.wInv) : 0;
    if (x0 >= KLT_GRID_COLS) return -1;
    const int cx = (int)ceilf((x - G.minX + r) * G.wInv), x1 = cx < KLT_GRID_COLS - 1 ? cx : KLT_GRID_COLS - 1;
    if (x1 < 0) return -1;
    const int y0 = (int)floorf((y - G.minY - r) * G.hInv) > 0 ? (int)floorf((y - G.minY - r) * G.hInv) : 0;
    if (y0 >= KLT_GRID_ROWS) return -1;
    const int cy = (int)ceilf((y - G.minY + r) * G.hInv), y1 = cy < KLT_GRID_ROWS - 1 ? cy : KLT_GRID_ROWS - 1;
    if (y1 < 0) return -1;
    const bool check = minLevel > 0 || maxLevel >= 0;
    int best = -1;
    float min_dist = -1;
    for (int ix = x0; ix <= x1; ix++)
        for (int iy = y0; iy <= y1; iy++) {
            const int c = ix * KLT_GRID_ROWS + iy; // 0 <= c < KLT_NCELL
            for (int j = cell_start[c]; j < cell_start[c + 1]; j++) {
                const KltCellRec k = recs[j];
                if (keys_static && keys_static[k.id]) continue; // this function is for dynamic points
                if (check && (k.octave < minLevel || (maxLevel >= 0 && k.octave > maxLevel))) continue;
                const float dx = k.x - x, dy = k.y - y;
                if (fabsf(dx) < r && fabsf(dy) < r) {
                    const float d = dx * dx + dy * dy;
                    if (min_dist == -1 || d < min_dist) { min_dist = d; best = k.id; }
                }
            }
        }
    return best;
}
// :1629-1664 for object o: the float sums over the tracked points in index order, the mean and its direction.  An object whose mean flow is zero gets 0 / 0 as
// its direction, which nothing reads: the > 20 guard looks at the norm alone.
HD void klt_object_mean(int n, const uint8_t *status, const int *sel, const int *object_id, const float *cur, const float *last, int o, float *mean3) {
    float sx = 0, sy = 0, norm = 0;
    int cnt = 0;
    for (int i = 0; i < n; i++)
        if (status[i] && object_id[sel[i]] == o) { cnt++; sx += cur[2 * i] - last[2 * i]; sy += cur[2 * i + 1] - last[2 * i + 1]; }
    if (cnt > 0) {
        sx /= (float)cnt; sy /= (float)cnt;
        norm = sqrtf(sx * sx + sy * sy);
        sx /= norm; sy /= norm;
    }
    mean3[0] = sx; mean3[1] = sy; mean3[2] = norm;
}
// :1667-1716 for one tracked point, up to the assignment.  Returns bit 0 kltmatches, bit 1 goodmatches, bit 2 findfeaturematches; *best = the key point it claims
// or -1; a rejected point's current position becomes (0, 0).
HD int klt_tracking_point(bool status, float lx, float ly, float *cx, float *cy, const float *mean3, int octave, float th, const float *scale_factors, const KltGridP &G,
                          const int *cell_start, const KltCellRec *recs, const uint8_t *keys_static, int *best) {
    *best = -1;
    if (!status) { *cx = 0; *cy = 0; return 0; }
    float dx = *cx - lx, dy = *cy - ly;
    const float move = sqrtf(dx * dx + dy * dy);
    dx /= move; dy /= move;
    if (mean3[2] > 20 && move > 20 && (double)(dx * mean3[0] + dy * mean3[1]) < 0.85) { *cx = 0; *cy = 0; return 1; }
    const float radius = th * scale_factors[octave];
    const int b = klt_closest_feature(G, cell_start, recs, *cx, *cy, radius, octave, 2, keys_static);
    if (b < 0 || (keys_static && keys_static[b])) { *cx = 0; *cy = 0; return 3; }
    *best = b;
    return 7;
}

// Frame::AssignFeaturesToGrid (Frame.cc:303-318, PosInGrid :525-535) on the host: xy = pt of mvKeysUn[i] at xy[i * stride_floats], octave likewise in ints
inline KltGridP klt_grid_params(int N, float minX, float maxX, float minY, float maxY) {
    KltGridP G; G.N = N; G.minX = minX; G.minY = minY;
    G.wInv = static_cast<float>(KLT_GRID_COLS) / static_cast<float>(maxX - minX);
    G.hInv = static_cast<float>(KLT_GRID_ROWS) / static_cast<float>(maxY - minY);
    return G;
}
inline void klt_build_grid_host(const KltGridP &G, const float *xy, const int *octave, int stride_floats, std::vector<int> &cell_start, std::vector<KltCellRec> &recs) {
    std::vector<int> cell((size_t)G.N);
    cell_start.assign((size_t)KLT_NCELL + 1, 0);
    for (int i = 0; i < G.N; i++) {
        const int px = (int)roundf((xy[(size_t)i * stride_floats] - G.minX) * G.wInv), py = (int)roundf((xy[(size_t)i * stride_floats + 1] - G.minY) * G.hInv);
        cell[(size_t)i] = (px < 0 || px >= KLT_GRID_COLS || py < 0 || py >= KLT_GRID_ROWS) ? -1 : px * KLT_GRID_ROWS + py;
        if (cell[(size_t)i] >= 0) cell_start[(size_t)cell[(size_t)i] + 1]++;
    }
    for (int c = 0; c < KLT_NCELL; c++) cell_start[(size_t)c + 1] += cell_start[(size_t)c];
    recs.resize((size_t)cell_start[KLT_NCELL]);
    std::vector<int> pos(cell_start.begin(), cell_start.end() - 1);
    for (int i = 0; i < G.N; i++)
        if (cell[(size_t)i] >= 0) recs[(size_t)pos[(size_t)cell[(size_t)i]]++] = KltCellRec{xy[(size_t)i * stride_floats], xy[(size_t)i * stride_floats + 1], i, octave[(size_t)i * stride_floats]};
}
// ORBmatcher::SearchByTracking for one pair on the host.  last_xy / last_octave: pt and octave of LastFrame.mvKeys (stride in floats / ints); cur_*: the current
// frame's mvKeysUn.  sel, klt_last, klt_this: room for n_last entries (2 floats each); train_match: N ints; counters: kltmatches, goodmatches, findfeaturematches,
// uniquematches.  Returns the number of points selected, or -1 for a tracked point whose object id is outside [0, numobject).
inline int klt_search_by_tracking_host(const uint8_t *last_img, const uint8_t *cur_img, int width, int height, long stride, int n_last, const float *last_xy, const int *last_octave,
                                       int last_stride, const uint8_t *eligible, const int *object_id, int numobject, float th, const float *scale_factors, const KltGridP &G,
                                       const float *cur_xy, const int *cur_octave, int cur_stride, const uint8_t *keys_static, const uint8_t *had_map_point, int *train_match, int *sel,
                                       float *klt_last, float *klt_this, int *counters) {
    int n = 0;
    for (int i = 0; i < n_last; i++)
        if (eligible[i] && last_octave[(size_t)i * last_stride] < 3) { sel[n] = i; klt_last[2 * n] = last_xy[(size_t)i * last_stride]; klt_last[2 * n + 1] = last_xy[(size_t)i * last_stride + 1]; n++; }
    for (int k = 0; k < G.N; k++) train_match[k] = -1;
    counters[0] = counters[1] = counters[2] = counters[3] = 0;
    if (n == 0) return 0;
    std::vector<uint8_t> two((size_t)2 * width * height), status((size_t)n);
    std::vector<float> err((size_t)n);
    for (int f = 0; f < 2; f++)
        for (int y = 0; y < height; y++) std::copy((f ? cur_img : last_img) + (long)y * stride, (f ? cur_img : last_img) + (long)y * stride + width, two.begin() + ((size_t)f * height + y) * width);
    const int first[2] = {0, n}, pp[1] = {0}, pn[1] = {1};
    klt_track_host(two.data(), 2, width, height, width, (long)width * height, 1, pp, pn, first, klt_last, klt_this, status.data(), err.data());
    for (int i = 0; i < n; i++)
        if (status[(size_t)i] && (object_id[sel[i]] < 0 || object_id[sel[i]] >= numobject)) return -1;
    std::vector<float> mean(3 * (size_t)(numobject > 0 ? numobject : 1));
    for (int o = 0; o < numobject; o++) klt_object_mean(n, status.data(), sel, object_id, klt_this, klt_last, o, &mean[3 * (size_t)o]);
    std::vector<int> cell_start;
    std::vector<KltCellRec> recs;
    klt_build_grid_host(G, cur_xy, cur_octave, cur_stride, cell_start, recs);
    for (int i = 0; i < n; i++) {
        int best;
        const int bits = klt_tracking_point(status[(size_t)i] != 0, klt_last[2 * i], klt_last[2 * i + 1], klt_this + 2 * i, klt_this + 2 * i + 1,
                                            status[(size_t)i] ? &mean[3 * (size_t)object_id[sel[i]]] : mean.data(), last_octave[(size_t)sel[i] * last_stride], th, scale_factors, G,
                                            cell_start.data(), recs.data(), keys_static, &best);
        counters[0] += bits & 1; counters[1] += (bits >> 1) & 1; counters[2] += (bits >> 2) & 1;
        if (best >= 0) train_match[best] = sel[i]; // sequential: the last i keeps the key point
    }
    for (int k = 0; k < G.N; k++) counters[3] += train_match[k] >= 0 && !(had_map_point && had_map_point[k]); // key points that had no map point when first assigned
    return n;
}
