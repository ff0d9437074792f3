// gftt.hip -- cv::goodFeaturesToTrack and the new-Harris-feature loop of Tracking::CreateNewKeyFrame on MI355X (gfx950).
//
// Replaces reference orb_object_slam/src/Tracking.cc:2263-2331: the mask built from objmask_img with a disc erased around every existing dynamic point, the corner
// detector on raw_img, and KeyFrame::UnprojectPixelDepth (src/KeyFrame.cc:711-727) of every new corner at its cuboid's depth.  The arithmetic is gftt_math.h; the
// definition of the two OpenCV functions is stated in INTEGRATION.md 4e.  The images are level 0 of the frames a cs_klt handle holds (klt.hip), read in place.
//
//   gftt_eig         one workgroup per 32 x 8 tile: pixels + a halo of 2 into LDS once, cov for the tile + a halo of 1 (at the REFLECT_101 coordinate outside the
//                    image), the 3 x 3 box in double, eig out; the masked maximum folds into one word per frame as an int that orders as the float
//   gftt_candidates  one thread per pixel: threshold, 3 x 3 maximum of e', mask; 64-bit keys appended per frame, one atomic per wave
//   gftt_select      one workgroup per frame: bitonic sort of the keys in LDS, then the greedy walk by one wave in batches of 64
//   gftt_mask        one workgroup per frame: good = objmask > 0 ? 255 : 0, then the discs, one existing point after the other
//   gftt_new_points  one thread per corner: object id, depth, unprojection
//
// One stream; every call waits for its results.
#include "common.h"
#include "gftt_math.h"
#include "klt_handle.h"

#include <climits>
#include <cmath>

static_assert(GFTT_MAX_CANDIDATES == CS_GFTT_MAX_CANDIDATES, "the header's constant is the kernels'");

namespace {
// pixel (x, y) of the image in slot s: base[frames[s] * frame_stride + off0 + y * row_stride + x]
struct GfttImg { const uint8_t *base; long frame_stride, off0; int row_stride, w, h; };
constexpr int EG_TX = 32, EG_TY = 8, EG_THREADS = EG_TX * EG_TY;
constexpr int EG_PW = EG_TX + 4, EG_PH = EG_TY + 4, EG_CW = EG_TX + 2, EG_CH = EG_TY + 2;
constexpr int GRID_Y = 65535;

__global__ void __launch_bounds__(256) gftt_init(int n, int *maxword, int *counters) { // counters: ncand, ncorners, outside (3 n) and the error word behind them
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) maxword[i] = GFTT_NO_MAX;
    if (i < 3 * n + 1) counters[i] = 0;
}

__global__ void __launch_bounds__(EG_THREADS) gftt_eig(GfttImg I, const int *__restrict__ frames, int s0, int tiles_x, const uint8_t *__restrict__ masks, float *__restrict__ eig,
                                                      int *maxword) {
    __shared__ uint8_t sP[EG_PH][EG_PW];
    __shared__ float sC[3][EG_CH][EG_CW + 1];
    const int slot = s0 + blockIdx.y, tid = threadIdx.x;
    const int tx0 = (blockIdx.x % tiles_x) * EG_TX, ty0 = (blockIdx.x / tiles_x) * EG_TY; // tx0 < w, ty0 < h
    const uint8_t *img = I.base + (long)frames[slot] * I.frame_stride + I.off0;
    for (int k = tid; k < EG_PW * EG_PH; k += EG_THREADS) { // the positions (tx0 - 2 + i, ty0 - 2 + j); those beyond [-2, w + 1] x [-2, h + 1] are never read
        const int i = k % EG_PW, j = k / EG_PW, x = tx0 - 2 + i, y = ty0 - 2 + j;
        uint8_t v = 0;
        if (x >= -2 && x <= I.w + 1 && y >= -2 && y <= I.h + 1) v = img[(long)klt_reflect101(y, I.h) * I.row_stride + klt_reflect101(x, I.w)]; // inside [0, w) x [0, h)
        sP[j][i] = v;
    }
    __syncthreads();
    for (int k = tid; k < EG_CW * EG_CH; k += EG_THREADS) { // cov at the positions (tx0 - 1 + i, ty0 - 1 + j) of [-1, w] x [-1, h]
        const int i = k % EG_CW, j = k / EG_CW, x = tx0 - 1 + i, y = ty0 - 1 + j;
        float c0 = 0, c1 = 0, c2 = 0;
        if (x >= -1 && x <= I.w && y >= -1 && y <= I.h) {
            // the border takes cov AT the reflected coordinate (xr, yr), a pixel of the image: its row in sP is yr - ty0 + 2 in [1, EG_TY + 2], its column
            // xr - tx0 + 2 in [1, EG_TX + 2] (x = -1 -> 1 with tx0 = 0; x = w -> w - 2 with tx0 < w), so the neighbours at +-1 are staged, reflected where they leave the image
            const int lx = klt_reflect101(x, I.w) - tx0 + 2, ly = klt_reflect101(y, I.h) - ty0 + 2;
            const uint8_t *up = sP[ly - 1], *mid = sP[ly], *down = sP[ly + 1];
            const float dx = gftt_dx(gftt_row_dx(up, lx - 1, lx + 1), gftt_row_dx(mid, lx - 1, lx + 1), gftt_row_dx(down, lx - 1, lx + 1));
            const float dy = gftt_dy(gftt_row_dy(up, lx, lx - 1, lx + 1), gftt_row_dy(down, lx, lx - 1, lx + 1));
            c0 = dx * dx; c1 = dx * dy; c2 = dy * dy;
        }
        sC[0][j][i] = c0; sC[1][j][i] = c1; sC[2][j][i] = c2;
    }
    __syncthreads();
    const int i = tid % EG_TX, j = tid / EG_TX, x = tx0 + i, y = ty0 + j;
    int best = GFTT_NO_MAX;
    if (x < I.w && y < I.h) {
        float s[3];
#pragma unroll
        for (int c = 0; c < 3; c++)
            s[c] = gftt_box(gftt_box_row(sC[c][j][i], sC[c][j][i + 1], sC[c][j][i + 2]), gftt_box_row(sC[c][j + 1][i], sC[c][j + 1][i + 1], sC[c][j + 1][i + 2]),
                            gftt_box_row(sC[c][j + 2][i], sC[c][j + 2][i + 1], sC[c][j + 2][i + 2]));
        const float e = gftt_min_eig(s[0], s[1], s[2]);
        const long at = ((long)slot * I.h + y) * I.w + x;
        eig[at] = e;
        if (!masks || masks[at]) best = gftt_ordered_int(e);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = max(best, __shfl_xor(best, off));
    if ((tid & 63) == 0 && best != GFTT_NO_MAX) atomicMax(&maxword[slot], best);
}

__global__ void __launch_bounds__(256) gftt_candidates(int w, int h, int s0, double quality_level, const uint8_t *__restrict__ masks, const float *__restrict__ eig,
                                                       const int *__restrict__ maxword, unsigned long long *__restrict__ keys, int *ncand) {
    const int slot = s0 + blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int x = p % w, y = p / w;
    const float *e = eig + (long)slot * w * h;
    bool cand = false;
    float v = 0;
    if (y < h - 1 && y >= 1 && x >= 1 && x < w - 1 && (!masks || masks[(long)slot * w * h + p])) { // the 3 x 3 neighbourhood lies in the image
        const float t = gftt_threshold(gftt_from_ordered_int(maxword[slot]), quality_level);
        v = gftt_tozero(e[p], t);
        cand = v != 0;
        for (int j = -1; j <= 1; j++)
            for (int k = -1; k <= 1; k++) cand = cand && !(gftt_tozero(e[p + j * w + k], t) > v);
    }
    const unsigned long long b = __ballot(cand);
    if (!b) return;
    int base = 0;
    if (lane == __ffsll((long long)b) - 1) base = atomicAdd(&ncand[slot], __popcll(b));
    base = __shfl(base, __ffsll((long long)b) - 1);
    const int pos = base + wave_rank(b, lane);
    if (cand && pos < GFTT_MAX_CANDIDATES) keys[(long)slot * GFTT_MAX_CANDIDATES + pos] = gftt_key(v, p); // (the count goes on beyond the capacity; the call then fails)
}

constexpr int SL_THREADS = 1024;
// Sort and greedy walk of one frame.  The walk is sequential in meaning: candidate i, in key order, is accepted unless an ACCEPTED corner lies nearer than
// minDistance.  Wave 0 takes 64 candidates at a time.  Each lane first tests its candidate against the corners accepted before the batch.  Then, while lanes are
// pending: the lowest pending lane i has passed the corners accepted before the batch and every accepted lower lane (a pending lane is struck out as soon as a lane
// below it is accepted too near), and every lane below i is decided, so the sequential walk, arriving at i, has accepted exactly those corners and accepts i; i's
// position goes to the lanes above it, which strike themselves out when too near.  The walk stops with the accepted count at max_corners, as the sequential one does
// behind its push_back.  The accepted positions overwrite the head of the key array: never more corners than candidates walked, and a batch sits in registers before
// any of its lanes is written.  (OpenCV's grid of cvRound(minDistance) cells only shortens the search: gftt_math.h, gftt_select_host.)
__global__ void __launch_bounds__(SL_THREADS) gftt_select(int w, int max_corners, int cap_corners, double min_dist2, const unsigned long long *__restrict__ keys, const int *__restrict__ ncand,
                                                          float *__restrict__ corners, float *__restrict__ quality, int *__restrict__ ncorners) {
    __shared__ unsigned long long sK[GFTT_MAX_CANDIDATES];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int n = ncand[slot];
    if (n > GFTT_MAX_CANDIDATES || n == 0) { if (tid == 0) ncorners[slot] = 0; return; }
    int m = 64;
    while (m < n) m <<= 1; // <= GFTT_MAX_CANDIDATES
    for (int i = tid; i < m; i += SL_THREADS) sK[i] = i < n ? keys[(long)slot * GFTT_MAX_CANDIDATES + i] : 0ull; // (0 is below every key: a key's upper word is not 0)
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += SL_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const unsigned long long a = sK[i], b = sK[o];
                    if ((i & k) == 0 ? a < b : a > b) { sK[i] = b; sK[o] = a; } // descending
                }
            }
            __syncthreads();
        }
    if (tid >= 64) return;
    const int lane = tid;
    int na = 0; // the same in every lane
    for (int b0 = 0; b0 < n && na < max_corners; b0 += 64) {
        const bool live = b0 + lane < n;
        const unsigned long long key = sK[min(b0 + lane, n - 1)];
        const int r = gftt_key_raster(key), x = r % w, y = r / w;
        bool ok = live;
        for (int k = 0; k < na && __any(ok); k++) {
            const unsigned long long a = sK[k]; // an accepted corner: y above x
            ok = ok && !gftt_too_close(x, y, (int)(uint32_t)a, (int)(a >> 32), min_dist2);
        }
        unsigned long long pending = __ballot(ok), accepted = 0;
        int total = na;
        while (pending && total < max_corners) {
            const int i = __ffsll((long long)pending) - 1;
            accepted |= 1ull << i; total++;
            const int ax = __shfl(x, i), ay = __shfl(y, i);
            const unsigned long long struck = __ballot(lane > i && gftt_too_close(x, y, ax, ay, min_dist2));
            pending &= ~struck & ~(1ull << i);
        }
        if ((accepted >> lane) & 1) {
            const int at = na + wave_rank(accepted, lane); // < total <= min(max_corners, n) <= cap_corners, and <= b0 + lane
            sK[at] = ((unsigned long long)(uint32_t)y << 32) | (uint32_t)x;
            const long o = (long)slot * cap_corners + at;
            corners[2 * o] = (float)x; corners[2 * o + 1] = (float)y; quality[o] = gftt_key_value(key);
        }
        na = total;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    if (lane == 0) ncorners[slot] = na;
}

constexpr int MK_THREADS = 256;
// Tracking.cc:2265-2287 for slot blockIdx.x.  The walk over the existing points (already in its order) is sequential in meaning -- a point whose pixel an earlier
// disc erased draws nothing -- and it is run so: one point after the other, every thread reads the point's pixel, a barrier, the threads draw the disc's 441-pixel box
// together, a barrier.
__global__ void __launch_bounds__(MK_THREADS) gftt_mask(int cols, int rows, const uint8_t *__restrict__ objmask, const int *__restrict__ first, const float *__restrict__ pts, uint8_t *good,
                                                        int *outside) {
    const int slot = blockIdx.x, tid = threadIdx.x;
    const long total = (long)rows * cols;
    const uint8_t *om = objmask + slot * total;
    uint8_t *g = good + slot * total;
    for (long i = tid; i < total; i += MK_THREADS) g[i] = om[i] > 0 ? 255 : 0;
    __syncthreads();
    int out = 0;
    for (int p = first[slot]; p < first[slot + 1]; p++) {
        int rx, ry;
        const long idx = gftt_point_index(pts[2 * (long)p], pts[2 * (long)p + 1], cols, &rx, &ry);
        if (idx < 0 || idx >= total) { out++; continue; } // (the same in every thread)
        const bool draw = g[idx] == 255;                  // 0 <= idx < total
        __syncthreads();
        if (draw)
            for (int k = tid; k < GFTT_DISC_BOX; k += MK_THREADS) {
                long at;
                if (gftt_disc_pixel(k, rx, ry, cols, rows, &at)) g[at] = 0; // 0 <= at < total: the pixel lies in the image
            }
        __syncthreads();
    }
    if (tid == 0) outside[slot] = out;
}

struct NewP { float K4[4]; int cols, rows, cap_corners; };
__global__ void __launch_bounds__(64) gftt_new_points(NewP P, const float *__restrict__ corners, const int *__restrict__ ncorners, const uint8_t *__restrict__ objmask,
                                                      const float *__restrict__ Twc, const int *__restrict__ cub_first, const float *__restrict__ cuboid_depth, int *__restrict__ object_id,
                                                      float *__restrict__ x3D, uint8_t *__restrict__ valid, int *bad_id) {
    const int slot = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    if (k >= ncorners[slot]) return;
    const long o = (long)slot * P.cap_corners + k;
    const float u = corners[2 * o], v = corners[2 * o + 1];
    const int id = (int)objmask[((long)slot * P.rows + (long)v) * P.cols + (long)u] - 1; // a corner is a pixel of the image
    float X[3] = {0, 0, 0};
    int ok = 0;
    if (id < 0 || id >= cub_first[slot + 1] - cub_first[slot]) atomicOr(bad_id, 1);
    else ok = gftt_unproject(u, v, cuboid_depth[cub_first[slot] + id], P.K4, Twc + 12 * (long)slot, X);
    object_id[o] = id; x3D[3 * o] = X[0]; x3D[3 * o + 1] = X[1]; x3D[3 * o + 2] = X[2]; valid[o] = (uint8_t)ok;
}

int fail(cs_ctx *ctx, const char *fn, const char *what, int status) {
    if (ctx) ctx->err = std::string(fn) + ": " + what;
    return status;
}
const char *detect_check(int n, int max_corners, double quality_level, double min_distance, const void *corners, const void *counts, const void *n_candidates) {
    if (n < 1 || !corners || !counts || !n_candidates) return "a null argument or no frame";
    if (max_corners < 1) return "max_corners < 1";
    if (!(min_distance >= 1) || !std::isfinite(min_distance)) return "min_distance < 1";
    if (!(quality_level > 0 && quality_level <= 1)) return "quality_level outside (0, 1]";
    return nullptr;
}
// the int block of a call: frames, maxword, ncand, ncorners, outside (n each), the error word
struct Ints { int *frames, *maxword, *ncand, *ncorners, *outside, *bad; };
int ints_of(cs_ctx *ctx, cs_owner &own, GfttBufs &B, int n, const int *frames, Ints *o) {
    CS_TRY(B.ints.grow(ctx, own, 5 * (size_t)n + 1));
    int *p = B.ints.p;
    *o = Ints{p, p + n, p + 2 * (size_t)n, p + 3 * (size_t)n, p + 4 * (size_t)n, p + 5 * (size_t)n};
    CS_TRY(cs_h2d(ctx, o->frames, frames, (size_t)n));
    CS_LAUNCH(ctx, "gftt_init", gftt_init, dim3((3 * n + 1 + 255) / 256), dim3(256), 0, n, o->maxword, o->ncand);
    return CS_OK;
}
int cap_of(int max_corners) { return std::min(max_corners, GFTT_MAX_CANDIDATES); } // a frame has no more corners than candidates
// eig, candidates and selection of n slots; d_masks: n dense images on the device or nullptr.  Results in B.corners / B.quality (cap_of(max_corners) per slot) and I.ncorners.
int detect(cs_ctx *ctx, cs_owner &own, GfttBufs &B, const GfttImg &I, int n, const Ints &T, const uint8_t *d_masks, int max_corners, double quality_level, double min_distance) {
    const size_t px = (size_t)I.w * I.h;
    const int cap = cap_of(max_corners);
    CS_TRY(B.eig.grow(ctx, own, px * n));
    CS_TRY(B.keys.grow(ctx, own, (size_t)GFTT_MAX_CANDIDATES * n));
    CS_TRY(B.corners.grow(ctx, own, 2 * (size_t)cap * n));
    CS_TRY(B.quality.grow(ctx, own, (size_t)cap * n));
    const int tiles_x = (I.w + EG_TX - 1) / EG_TX, tiles_y = (I.h + EG_TY - 1) / EG_TY;
    for (int s0 = 0; s0 < n; s0 += GRID_Y) { // (a grid's y extent ends at 65 535)
        const int ny = std::min(GRID_Y, n - s0);
        CS_LAUNCH(ctx, "gftt_eig", gftt_eig, dim3(tiles_x * tiles_y, ny), dim3(EG_THREADS), 0, I, T.frames, s0, tiles_x, d_masks, B.eig.p, T.maxword);
    }
    for (int s0 = 0; s0 < n; s0 += GRID_Y) {
        const int ny = std::min(GRID_Y, n - s0);
        CS_LAUNCH(ctx, "gftt_candidates", gftt_candidates, dim3((unsigned)((px + 255) / 256), ny), dim3(256), 0, I.w, I.h, s0, quality_level, d_masks, B.eig.p, T.maxword, B.keys.p,
                  T.ncand);
    }
    CS_LAUNCH(ctx, "gftt_select", gftt_select, dim3(n), dim3(SL_THREADS), 0, I.w, max_corners, cap, min_distance * min_distance, B.keys.p, T.ncand, B.corners.p, B.quality.p, T.ncorners);
    CS_HIP(ctx, hipGetLastError());
    return CS_OK;
}
// the corners of the slots from the device to the caller's arrays (max_corners per slot); CS_ERR_CAPACITY for a frame with too many candidates
int read_corners(cs_ctx *ctx, const char *fn, GfttBufs &B, const Ints &T, int n, int max_corners, float *corners, float *quality, int *counts, int *n_candidates) {
    const int cap = cap_of(max_corners);
    std::vector<float> c(2 * (size_t)cap * n), q((size_t)cap * n);
    CS_TRY(cs_d2h(ctx, n_candidates, T.ncand, (size_t)n));
    CS_TRY(cs_d2h(ctx, counts, T.ncorners, (size_t)n));
    CS_TRY(cs_d2h(ctx, c.data(), B.corners.p, c.size()));
    CS_TRY(cs_d2h(ctx, q.data(), B.quality.p, q.size()));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < n; s++)
        if (n_candidates[s] > GFTT_MAX_CANDIDATES) {
            for (int k = 0; k < n; k++) counts[k] = 0;
            return fail(ctx, fn, "a frame has more candidates than CS_GFTT_MAX_CANDIDATES", CS_ERR_CAPACITY);
        }
    for (int s = 0; s < n; s++) {
        std::copy(c.begin() + 2 * (size_t)cap * s, c.begin() + 2 * ((size_t)cap * s + counts[s]), corners + 2 * (size_t)max_corners * s);
        if (quality) std::copy(q.begin() + (size_t)cap * s, q.begin() + (size_t)cap * s + counts[s], quality + (size_t)max_corners * s);
    }
    return CS_OK;
}
GfttImg resident(const cs_klt *h) { // level 0 inside its 21-pixel pad
    const int ps = h->W + 2 * KLT_PAD;
    return GfttImg{h->d_img, h->L.img_frame, h->L.img_off[0] + (long)KLT_PAD * ps + KLT_PAD, ps, h->W, h->H};
}
const char *frames_check(const cs_klt *h, int n, const int *frames) {
    if (h->n_frames < 1) return "no frames are set";
    if (n < 1 || !frames) return "a null argument or no frame";
    for (int s = 0; s < n; s++)
        if (frames[s] < 0 || frames[s] >= h->n_frames) return "a frame that is not set";
    return nullptr;
}
int good_features_device(cs_ctx *ctx, const char *fn, cs_owner &own, GfttBufs &B, const GfttImg &I, int n, const int *frames, const uint8_t *masks, int max_corners,
                         double quality_level, double min_distance, float *corners, float *quality, int *counts, int *n_candidates) {
    Ints T;
    CS_TRY(ints_of(ctx, own, B, n, frames, &T));
    const size_t px = (size_t)I.w * I.h;
    if (masks) {
        CS_TRY(B.masks.grow(ctx, own, px * n));
        CS_TRY(cs_h2d(ctx, B.masks.p, masks, px * n));
    }
    CS_TRY(detect(ctx, own, B, I, n, T, masks ? B.masks.p : nullptr, max_corners, quality_level, min_distance));
    return read_corners(ctx, fn, B, T, n, max_corners, corners, quality, counts, n_candidates);
}
// what is wrong with the lists of cs_track_new_harris_features, or nullptr
const char *harris_check(int n, const uint8_t *objmasks, const int *exist_first, const float *exist_pts, const int *exist_obs, const float *K4, const float *Twc, const int *cub_first,
                         const float *cuboid_depth, const void *new_first, const void *new_pts, const void *new_object_id, const void *new_x3D, const void *x3D_valid) {
    if (n < 1 || !objmasks || !K4 || !Twc || !new_first || !new_pts || !new_object_id || !new_x3D || !x3D_valid) return "a null argument or no frame";
    if (!cs_offsets_ok(exist_first, n, exist_pts) || (exist_first[n] > 0 && !exist_obs)) return "exist_first does not start at 0, decreases, or points are missing";
    if (!cs_offsets_ok(cub_first, n, cuboid_depth)) return "cub_first does not start at 0, decreases, or depths are missing";
    for (long i = 0; i < 2 * (long)exist_first[n]; i++)
        if (!gftt_point_ok(exist_pts[i])) return "an existing point that is not finite (or beyond 1e9)";
    return nullptr;
}
// the existing points of every frame in the order of the walk
std::vector<float> sorted_points(int n, const int *exist_first, const float *exist_pts, const int *exist_obs) {
    std::vector<float> s(2 * (size_t)exist_first[n] + 2);
    for (int f = 0; f < n; f++) {
        const int b0 = exist_first[f];
        const std::vector<int> order = gftt_point_order(exist_first[f + 1] - b0, exist_obs + b0);
        for (size_t i = 0; i < order.size(); i++) { s[2 * (b0 + i)] = exist_pts[2 * ((size_t)b0 + order[i])]; s[2 * (b0 + i) + 1] = exist_pts[2 * ((size_t)b0 + order[i]) + 1]; }
    }
    return s;
}
constexpr int NH_CORNERS = 200; // max_new_pts of Tracking.cc:2290
int new_harris_device(cs_ctx *ctx, const char *fn, cs_owner &own, GfttBufs &B, const GfttImg &I, int n, const int *frames, const uint8_t *objmasks, const int *exist_first,
                      const float *exist_pts, const int *exist_obs, const float *K4, const float *Twc, const int *cub_first, const float *cuboid_depth, int *new_first, float *new_pts,
                      int *new_object_id, float *new_x3D, uint8_t *x3D_valid, int *n_mask_outside, uint8_t *good_masks, int *n_candidates) {
    Ints T;
    CS_TRY(ints_of(ctx, own, B, n, frames, &T));
    const size_t px = (size_t)I.w * I.h;
    const std::vector<float> sorted = sorted_points(n, exist_first, exist_pts, exist_obs);
    cs_scratch sc(ctx); // the lists of this call
    int *d_first = nullptr, *d_cub = nullptr, *d_id = nullptr;
    float *d_Twc = nullptr, *d_depth = nullptr, *d_x3D = nullptr;
    uint8_t *d_valid = nullptr;
    const float none = 0;
    CS_TRY(B.masks.grow(ctx, own, px * n));
    CS_TRY(B.good.grow(ctx, own, px * n));
    CS_TRY(B.pts.grow(ctx, own, sorted.size()));
    CS_TRY(cs_h2d(ctx, B.masks.p, objmasks, px * n));
    CS_TRY(cs_h2d(ctx, B.pts.p, sorted.data(), sorted.size()));
    CS_TRY(sc.upload(ctx, &d_first, exist_first, (size_t)n + 1));
    CS_TRY(sc.upload(ctx, &d_cub, cub_first, (size_t)n + 1));
    CS_TRY(sc.upload(ctx, &d_Twc, Twc, 12 * (size_t)n));
    CS_TRY(sc.upload(ctx, &d_depth, cub_first[n] ? cuboid_depth : &none, (size_t)std::max(cub_first[n], 1)));
    CS_TRY(sc.alloc(ctx, &d_id, (size_t)NH_CORNERS * n));
    CS_TRY(sc.alloc(ctx, &d_x3D, 3 * (size_t)NH_CORNERS * n));
    CS_TRY(sc.alloc(ctx, &d_valid, (size_t)NH_CORNERS * n));
    CS_LAUNCH(ctx, "gftt_mask", gftt_mask, dim3(n), dim3(MK_THREADS), 0, I.w, I.h, B.masks.p, d_first, B.pts.p, B.good.p, T.outside);
    CS_TRY(detect(ctx, own, B, I, n, T, B.good.p, NH_CORNERS, 0.1, (double)GFTT_DISC_R));
    NewP P{{K4[0], K4[1], K4[2], K4[3]}, I.w, I.h, NH_CORNERS};
    CS_LAUNCH(ctx, "gftt_new_points", gftt_new_points, dim3((NH_CORNERS + 63) / 64, n), dim3(64), 0, P, B.corners.p, T.ncorners, B.masks.p, d_Twc, d_cub, d_depth, d_id, d_x3D, d_valid, T.bad);
    CS_HIP(ctx, hipGetLastError());
    std::vector<float> c(2 * (size_t)NH_CORNERS * n), X(3 * (size_t)NH_CORNERS * n);
    std::vector<int> id((size_t)NH_CORNERS * n), counts((size_t)n), ncand((size_t)n), outside((size_t)n);
    std::vector<uint8_t> valid((size_t)NH_CORNERS * n);
    int bad = 0;
    CS_TRY(cs_d2h(ctx, counts.data(), T.ncorners, (size_t)n));
    CS_TRY(cs_d2h(ctx, ncand.data(), T.ncand, (size_t)n));
    CS_TRY(cs_d2h(ctx, outside.data(), T.outside, (size_t)n));
    CS_TRY(cs_d2h(ctx, &bad, T.bad, (size_t)1));
    CS_TRY(cs_d2h(ctx, c.data(), B.corners.p, c.size()));
    CS_TRY(cs_d2h(ctx, X.data(), d_x3D, X.size()));
    CS_TRY(cs_d2h(ctx, id.data(), d_id, id.size()));
    CS_TRY(cs_d2h(ctx, valid.data(), d_valid, valid.size()));
    if (good_masks) CS_TRY(cs_d2h(ctx, good_masks, B.good.p, px * n));
    CS_TRY(sc.drain());
    new_first[0] = 0;
    for (int s = 0; s < n; s++) {
        new_first[s + 1] = 0;
        if (n_candidates) n_candidates[s] = ncand[(size_t)s];
        if (n_mask_outside) n_mask_outside[s] = outside[(size_t)s];
    }
    for (int s = 0; s < n; s++)
        if (ncand[(size_t)s] > GFTT_MAX_CANDIDATES) return fail(ctx, fn, "a frame has more candidates than CS_GFTT_MAX_CANDIDATES", CS_ERR_CAPACITY);
    if (bad) return fail(ctx, fn, "a corner's object id is at or beyond its frame's cuboid count", CS_ERR_BAD_ARG);
    for (int s = 0; s < n; s++) {
        const size_t from = (size_t)NH_CORNERS * s, to = (size_t)new_first[s], k = (size_t)counts[(size_t)s];
        std::copy(c.begin() + 2 * from, c.begin() + 2 * (from + k), new_pts + 2 * to);
        std::copy(X.begin() + 3 * from, X.begin() + 3 * (from + k), new_x3D + 3 * to);
        std::copy(id.begin() + from, id.begin() + from + k, new_object_id + to);
        std::copy(valid.begin() + from, valid.begin() + from + k, x3D_valid + to);
        new_first[s + 1] = (int)(to + k);
    }
    return CS_OK;
}
int host_images_check(const uint8_t *gray, int n, int width, int height, long stride) {
    return gray && n >= 1 && width >= 1 && height >= 1 && stride >= width && (long)width * height <= INT_MAX ? CS_OK : CS_ERR_BAD_ARG;
}
} // namespace

extern "C" {

int cs_klt_good_features(cs_ctx *ctx, cs_klt *h, int n, const int *frames, const uint8_t *masks, int max_corners, double quality_level, double min_distance, float *corners,
                         float *quality, int *counts, int *n_candidates) {
    if (!ctx || !h) return CS_ERR_BAD_ARG;
    if (const char *what = frames_check(h, n, frames)) return fail(ctx, "cs_klt_good_features", what, CS_ERR_BAD_ARG);
    if (const char *what = detect_check(n, max_corners, quality_level, min_distance, corners, counts, n_candidates)) return fail(ctx, "cs_klt_good_features", what, CS_ERR_BAD_ARG);
    CS_HIP(ctx, hipSetDevice(ctx->device));
    return good_features_device(ctx, "cs_klt_good_features", h->own, h->gftt, resident(h), n, frames, masks, max_corners, quality_level, min_distance, corners, quality, counts,
                                n_candidates);
}

int cs_good_features_images(cs_ctx *ctx, const uint8_t *gray, int n, int width, int height, long stride_bytes, const uint8_t *masks, int max_corners, double quality_level,
                            double min_distance, float *corners, float *quality, int *counts, int *n_candidates) {
    if (!ctx) return CS_ERR_BAD_ARG;
    if (host_images_check(gray, n, width, height, stride_bytes) != CS_OK) return fail(ctx, "cs_good_features_images", "no image, or rows that overlap", CS_ERR_BAD_ARG);
    if (const char *what = detect_check(n, max_corners, quality_level, min_distance, corners, counts, n_candidates)) return fail(ctx, "cs_good_features_images", what, CS_ERR_BAD_ARG);
    for (int s = 0; s < n; s++) counts[s] = n_candidates[s] = 0;
    if (width < 3 || height < 3) return CS_OK; // no pixel has a 3 x 3 neighbourhood
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    GfttBufs B;
    uint8_t *d_gray = nullptr;
    CS_TRY(sc.alloc(ctx, &d_gray, (size_t)width * height * n));
    CS_HIP(ctx, hipMemcpy2DAsync(d_gray, (size_t)width, gray, (size_t)stride_bytes, (size_t)width, (size_t)height * n, hipMemcpyHostToDevice, ctx->stream));
    std::vector<int> frames((size_t)n);
    for (int s = 0; s < n; s++) frames[(size_t)s] = s;
    return good_features_device(ctx, "cs_good_features_images", sc, B, GfttImg{d_gray, (long)width * height, 0, width, width, height}, n, frames.data(), masks, max_corners,
                                quality_level, min_distance, corners, quality, counts, n_candidates);
}

int cs_klt_good_features_host(const uint8_t *gray, int n, int width, int height, long stride_bytes, const uint8_t *masks, int max_corners, double quality_level, double min_distance,
                              float *corners, float *quality, int *counts, int *n_candidates) {
    if (host_images_check(gray, n, width, height, stride_bytes) != CS_OK || detect_check(n, max_corners, quality_level, min_distance, corners, counts, n_candidates)) return CS_ERR_BAD_ARG;
    const size_t px = (size_t)width * height;
    const int cap = cap_of(max_corners);
    bool fits = true;
#pragma omp parallel for schedule(dynamic) reduction(&& : fits)
    for (int s = 0; s < n; s++) {
        std::vector<float> c(2 * (size_t)cap), q((size_t)cap);
        const bool ok = gftt_good_features_host(gray + (long)s * height * stride_bytes, stride_bytes, width, height, masks ? masks + px * s : nullptr, cap, quality_level, min_distance,
                                                c.data(), q.data(), counts + s, n_candidates + s);
        fits = fits && ok;
        std::copy(c.begin(), c.begin() + 2 * (size_t)counts[s], corners + 2 * (size_t)max_corners * s);
        if (quality) std::copy(q.begin(), q.begin() + counts[s], quality + (size_t)max_corners * s);
    }
    if (!fits) {
        for (int s = 0; s < n; s++) counts[s] = 0;
        return CS_ERR_CAPACITY;
    }
    return CS_OK;
}

int cs_track_new_harris_features(cs_ctx *ctx, cs_klt *h, int n, const int *frames, const uint8_t *objmasks, const int *exist_first, const float *exist_pts, const int *exist_obs,
                                 const float *K4, const float *Twc, const int *cub_first, const float *cuboid_depth, int *new_first, float *new_pts, int *new_object_id, float *new_x3D,
                                 uint8_t *x3D_valid, int *n_mask_outside, uint8_t *good_masks, int *n_candidates) {
    if (!ctx || !h) return CS_ERR_BAD_ARG;
    if (const char *what = frames_check(h, n, frames)) return fail(ctx, "cs_track_new_harris_features", what, CS_ERR_BAD_ARG);
    if (const char *what = harris_check(n, objmasks, exist_first, exist_pts, exist_obs, K4, Twc, cub_first, cuboid_depth, new_first, new_pts, new_object_id, new_x3D, x3D_valid))
        return fail(ctx, "cs_track_new_harris_features", what, CS_ERR_BAD_ARG);
    CS_HIP(ctx, hipSetDevice(ctx->device));
    return new_harris_device(ctx, "cs_track_new_harris_features", h->own, h->gftt, resident(h), n, frames, objmasks, exist_first, exist_pts, exist_obs, K4, Twc, cub_first, cuboid_depth,
                             new_first, new_pts, new_object_id, new_x3D, x3D_valid, n_mask_outside, good_masks, n_candidates);
}

int cs_track_new_harris_features_host(const uint8_t *gray, int n, int width, int height, long stride_bytes, const uint8_t *objmasks, const int *exist_first, const float *exist_pts,
                                      const int *exist_obs, const float *K4, const float *Twc, const int *cub_first, const float *cuboid_depth, int *new_first, float *new_pts,
                                      int *new_object_id, float *new_x3D, uint8_t *x3D_valid, int *n_mask_outside, uint8_t *good_masks, int *n_candidates) {
    if (host_images_check(gray, n, width, height, stride_bytes) != CS_OK ||
        harris_check(n, objmasks, exist_first, exist_pts, exist_obs, K4, Twc, cub_first, cuboid_depth, new_first, new_pts, new_object_id, new_x3D, x3D_valid))
        return CS_ERR_BAD_ARG;
    const size_t px = (size_t)width * height;
    std::vector<float> c(2 * (size_t)NH_CORNERS * n), X(3 * (size_t)NH_CORNERS * n);
    std::vector<int> id((size_t)NH_CORNERS * n), counts((size_t)n, 0), ncand((size_t)n, 0), outside((size_t)n, 0), rc((size_t)n, 0);
    std::vector<uint8_t> valid((size_t)NH_CORNERS * n), good(good_masks ? 0 : px * n);
    uint8_t *g = good_masks ? good_masks : good.data();
#pragma omp parallel for schedule(dynamic)
    for (int s = 0; s < n; s++) {
        const size_t o = (size_t)NH_CORNERS * s;
        rc[(size_t)s] = gftt_new_harris_features_host(gray + (long)s * height * stride_bytes, stride_bytes, width, height, objmasks + px * s, exist_first[s + 1] - exist_first[s],
                                                      exist_pts + 2 * (size_t)exist_first[s], exist_obs + exist_first[s], K4, Twc + 12 * (size_t)s, cub_first[s + 1] - cub_first[s],
                                                      cuboid_depth + cub_first[s], g + px * s, &c[2 * o], &id[o], &X[3 * o], &valid[o], &counts[(size_t)s], &ncand[(size_t)s],
                                                      &outside[(size_t)s]);
    }
    new_first[0] = 0;
    for (int s = 0; s < n; s++) {
        new_first[s + 1] = 0;
        if (n_candidates) n_candidates[s] = ncand[(size_t)s];
        if (n_mask_outside) n_mask_outside[s] = outside[(size_t)s];
    }
    for (int s = 0; s < n; s++) if (rc[(size_t)s] == 1) return CS_ERR_CAPACITY;
    for (int s = 0; s < n; s++) if (rc[(size_t)s] == 2) return CS_ERR_BAD_ARG;
    for (int s = 0; s < n; s++) {
        const size_t from = (size_t)NH_CORNERS * s, to = (size_t)new_first[s], k = (size_t)counts[(size_t)s];
        std::copy(c.begin() + 2 * from, c.begin() + 2 * (from + k), new_pts + 2 * to);
        std::copy(X.begin() + 3 * from, X.begin() + 3 * (from + k), new_x3D + 3 * to);
        std::copy(id.begin() + from, id.begin() + from + k, new_object_id + to);
        std::copy(valid.begin() + from, valid.begin() + from + k, x3D_valid + to);
        new_first[s + 1] = (int)(to + k);
    }
    return CS_OK;
}

} // extern "C"
