// klt.hip -- cv::calcOpticalFlowPyrLK of ORBmatcher::SearchByTrackingHarris / SearchByTracking on MI355X (gfx950).
//
// Replaces the two optical-flow calls of the dynamic mode (reference orb_object_slam/src/ORBmatcher.cc:1548 and :1620) and the selection pass of
// SearchByTrackingHarris (:1556-1576) and everything of SearchByTracking around its call (:1591-1716).  The arithmetic is klt_math.h; the definition of the OpenCV function is stated in INTEGRATION.md.
//
//   klt_level          one thread per PADDED pixel of one level of every frame: level 0 copies the image, level l + 1 is pyrDown of level l, both at the
//                      REFLECT_101 image of the padded coordinate, so the 21-pixel pad is materialised by the same launch
//   klt_scharr         one thread per padded pixel: calcSharrDeriv inside (its +-1 neighbours are the pad's own reflection), constant 0 in the pad
//   klt_track          16 lanes per point, 4 points per 64-thread workgroup: the lanes sample the 21 x 21 window into LDS (I, Ix, Iy as shorts, resident across
//                      the iterations; the terms of b1 / b2 as floats), then one lane per sum adds its 441 terms in window order
//   klt_harris_select  one workgroup per pair: bounds test, mask lookup, ordered compaction
//   klt_tracking_select / klt_tracking_assign   ORBmatcher::SearchByTracking (:1582-1725) around klt_track for one pair, on a matcher's resident grid: the
//                      octave < 3 selection, then per-object mean flow, direction test, Frame::GetCloestFeaturesInArea and the assignment in one workgroup
//
// One stream; cs_klt_set_frames waits for its upload (the caller's images are free when it returns), the track calls wait for their results.
#include "common.h"
#include "klt_handle.h"
#include "klt_math.h"

#include <climits>
#include <cmath>
#include <new>
#include <vector>

namespace {
constexpr int TK_LANES = 16, TK_THREADS = 64, TK_PTS = TK_THREADS / TK_LANES;
constexpr int TK_ROW = 444; // 441 terms, rows 16 bytes apart
static_assert(TK_THREADS == 64, "klt_track's loop conditions are wave votes: the workgroup is one wave");

struct LevelP { int l, w, h, pw, ph, uw, uh, f0; long off, up_off, frame, gray_frame; }; // a launch takes the frames f0 + blockIdx.y
constexpr int KLT_GRID_Y = 65535;

__global__ void __launch_bounds__(256) klt_level(LevelP P, const uint8_t *__restrict__ gray, uint8_t *img) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.pw * P.ph) return;
    const int px = i % P.pw, py = i / P.pw;
    const int x = klt_reflect101(px - KLT_PAD, P.w), y = klt_reflect101(py - KLT_PAD, P.h); // inside [0, w) x [0, h): w, h > 21
    const long f = P.f0 + (long)blockIdx.y;
    uint8_t *frame = img + f * P.frame;
    uint8_t v;
    if (P.l == 0) v = gray[f * P.gray_frame + (long)y * P.w + x];
    else v = klt_pyrdown_pixel(frame + P.up_off + (long)KLT_PAD * (P.uw + 2 * KLT_PAD) + KLT_PAD, P.uw + 2 * KLT_PAD, P.uw, P.uh, x, y); // (reads the interior of the level above only)
    frame[P.off + i] = v;
}

__global__ void __launch_bounds__(256) klt_scharr(LevelP P, const uint8_t *__restrict__ img, short *__restrict__ der) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.pw * P.ph) return;
    const int px = i % P.pw, py = i / P.pw;
    short ix = 0, iy = 0;
    if (px >= KLT_PAD && px < P.w + KLT_PAD && py >= KLT_PAD && py < P.h + KLT_PAD) // the neighbours at +-1 lie in the level or in the first ring of its pad
        klt_scharr_pixel(img + (P.f0 + (long)blockIdx.y) * P.frame + P.off + i, P.pw, &ix, &iy);
    short *o = der + 2 * ((P.f0 + (long)blockIdx.y) * P.frame + P.off + i);
    o[0] = ix; o[1] = iy;
}

// first[p] <= i < first[p + 1]; empty pairs are stepped over
__device__ __forceinline__ int pair_of(const int *__restrict__ first, int n_pairs, int i) {
    int lo = 0, hi = n_pairs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

struct TrackP { KltLayout L; int n_pairs, total; };

// the 441 terms of one sum, added in window order by the calling lane
__device__ __forceinline__ float chain_sum(const float *t) {
    float s = 0;
#pragma unroll 7
    for (int k = 0; k < KLT_WN; k++) s += t[k];
    return s;
}

__global__ void __launch_bounds__(TK_THREADS) klt_track(TrackP P, const int *__restrict__ first, const int *__restrict__ pair_prev, const int *__restrict__ pair_next,
                                                       const uint8_t *__restrict__ img, const short *__restrict__ der, const float *__restrict__ prev_pts,
                                                       float *__restrict__ next_pts, uint8_t *__restrict__ status, float *__restrict__ err) {
    __shared__ short sI[TK_PTS][TK_ROW], sIx[TK_PTS][TK_ROW], sIy[TK_PTS][TK_ROW];
    __shared__ __attribute__((aligned(16))) float sB1[TK_PTS][TK_ROW], sB2[TK_PTS][TK_ROW];
    __shared__ float sR[TK_PTS][4];
    const int g = threadIdx.x / TK_LANES, lane = threadIdx.x % TK_LANES;
    const int p = blockIdx.x * TK_PTS + g;
    const bool live = p < P.total;
    float ptx = 0, pty = 0;
    const uint8_t *Ifr = img, *Jfr = img;
    const short *Dfr = der;
    if (live) {
        const int pr = pair_of(first, P.n_pairs, p);
        ptx = prev_pts[2 * (size_t)p]; pty = prev_pts[2 * (size_t)p + 1];
        Ifr = img + (long)pair_prev[pr] * P.L.img_frame; Jfr = img + (long)pair_next[pr] * P.L.img_frame;
        Dfr = der + 2 * (long)pair_prev[pr] * P.L.der_frame;
    }
    short *I = sI[g], *Ix = sIx[g], *Iy = sIy[g];
    float *B1 = sB1[g], *B2 = sB2[g], *R = sR[g];
    float nextx = 0, nexty = 0, er = 0; // nextPts[ptidx], err[ptidx]
    bool st = true;                     // status[ptidx]
    for (int level = P.L.n_levels - 1; level >= 0; level--) {
        const int cols = P.L.w[level], rows = P.L.h[level];
        const long ps = cols + 2 * KLT_PAD;
        const uint8_t *Ip = Ifr + P.L.img_off[level], *Jp = Jfr + P.L.img_off[level];
        const short *Dp = Dfr + 2 * P.L.der_off[level];
        float px = ptx * (float)(1. / (1 << level)), py = pty * (float)(1. / (1 << level));
        float nx, ny;
        if (level == P.L.n_levels - 1) { nx = px; ny = py; } else { nx = nextx * 2.f; ny = nexty * 2.f; }
        nextx = nx; nexty = ny;
        px -= (float)KLT_HALF; py -= (float)KLT_HALF;
        int ix = klt_floor(px), iy = klt_floor(py);
        bool act = live; // this point goes on at this level
        if (act && !klt_in_range(ix, iy, cols, rows)) {
            if (level == 0) { st = false; er = 0; }
            act = false;
        }
        if (act) {
            const KltW W = klt_weights(px - (float)ix, py - (float)iy);
            // ix in [-21, cols - 1]: the padded column ix + 21 + x + 1 <= cols + 41 < ps, and the same for the rows: the window lies in the level and its pad
            const long o0 = (long)(iy + KLT_PAD) * ps + ix + KLT_PAD;
            for (int k = lane; k < KLT_WN; k += TK_LANES) {
                const long o = o0 + (k / KLT_WIN) * ps + k % KLT_WIN;
                int gx, gy;
                klt_sample_deriv(Dp + 2 * o, ps, W, &gx, &gy);
                I[k] = (short)klt_sample_img(Ip + o, ps, W); Ix[k] = (short)gx; Iy[k] = (short)gy;
            }
        }
        __syncthreads();
        if (act && lane < 3) { // A11, A12, A22: one lane each, in window order
            const short *a = lane < 2 ? Ix : Iy, *b = lane == 0 ? Ix : Iy;
            float s = 0;
#pragma unroll 7
            for (int k = 0; k < KLT_WN; k++) s += klt_term(a[k], b[k]);
            R[lane] = s * KLT_FLT_SCALE;
        }
        __syncthreads();
        float A11 = 0, A12 = 0, A22 = 0, Dinv = 0;
        if (act) {
            A11 = R[0]; A12 = R[1]; A22 = R[2];
            if (!klt_gradient_ok(A11, A12, A22, &Dinv)) {
                if (level == 0) st = false;
                act = false;
            }
        }
        nx -= (float)KLT_HALF; ny -= (float)KLT_HALF;
        bool iter = act;
        float pdx = 0, pdy = 0;
        for (int j = 0; j < KLT_ITERS; j++) {
            if (!__any(iter)) break; // the same for the whole workgroup (one wave)
            if (iter) {
                ix = klt_floor(nx); iy = klt_floor(ny);
                if (!klt_in_range(ix, iy, cols, rows)) {
                    if (level == 0) st = false;
                    iter = false;
                }
            }
            if (iter) {
                const KltW W = klt_weights(nx - (float)ix, ny - (float)iy);
                const long o0 = (long)(iy + KLT_PAD) * ps + ix + KLT_PAD; // the same bound as above
                for (int k = lane; k < KLT_WN; k += TK_LANES) {
                    const int diff = klt_sample_img(Jp + o0 + (k / KLT_WIN) * ps + k % KLT_WIN, ps, W) - I[k];
                    B1[k] = klt_term(diff, Ix[k]); B2[k] = klt_term(diff, Iy[k]);
                }
            }
            __syncthreads();
            if (iter && lane < 2) R[lane] = chain_sum(lane ? B2 : B1) * KLT_FLT_SCALE;
            __syncthreads();
            if (iter) {
                float dx, dy;
                klt_step(A11, A12, A22, Dinv, R[0], R[1], &dx, &dy);
                nx += dx; ny += dy;
                nextx = nx + (float)KLT_HALF; nexty = ny + (float)KLT_HALF;
                if (klt_eps_stop(dx, dy)) iter = false;
                else if (j > 0 && klt_oscillation_stop(dx, dy, pdx, pdy)) {
                    nextx -= dx * 0.5f; nexty -= dy * 0.5f;
                    iter = false;
                }
                pdx = dx; pdy = dy;
            }
        }
        bool e = act && st && level == 0;
        if (e) {
            const float ex = nextx - (float)KLT_HALF, ey = nexty - (float)KLT_HALF;
            ix = klt_floor(ex); iy = klt_floor(ey);
            if (!klt_in_range(ix, iy, cols, rows)) { st = false; e = false; }
            else {
                const KltW W = klt_weights(ex - (float)ix, ey - (float)iy);
                const long o0 = (long)(iy + KLT_PAD) * ps + ix + KLT_PAD; // the same bound as above
                for (int k = lane; k < KLT_WN; k += TK_LANES) B1[k] = fabsf((float)(klt_sample_img(Jp + o0 + (k / KLT_WIN) * ps + k % KLT_WIN, ps, W) - I[k]));
            }
        }
        __syncthreads();
        if (e && lane == 0) R[3] = chain_sum(B1);
        __syncthreads();
        if (e) er = klt_err(R[3]);
    }
    if (live && lane == 0) {
        next_pts[2 * (size_t)p] = nextx; next_pts[2 * (size_t)p + 1] = nexty;
        status[p] = st ? 1 : 0; err[p] = er;
    }
}

constexpr int HS_THREADS = 256, HS_WAVES = HS_THREADS / 64;
// ORBmatcher.cc:1556-1576 for pair blockIdx.x: the survivors in index order at the pair's own slots (first[p] ...), counts[2 p] = goodmatches, [2 p + 1] = lookups
// beyond the mask
__global__ void __launch_bounds__(HS_THREADS) klt_harris_select(const int *__restrict__ first, const float *__restrict__ cur, const uint8_t *__restrict__ status,
                                                                 const uint8_t *__restrict__ masks, int cols, int rows, int *__restrict__ kept, float *__restrict__ kept_pts,
                                                                 int *__restrict__ object_id, int *__restrict__ counts) {
    __shared__ int s_wave[HS_WAVES], s_wout[HS_WAVES]; // per wave: the points kept and the lookups beyond the mask of the current pass
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b0 = first[p], n = first[p + 1] - b0;
    const uint8_t *mask = masks + (long)p * rows * cols;
    int good = 0, beyond = 0; // the same in every thread
    for (int start = 0; start < n; start += HS_THREADS) {
        const int i = start + tid;
        bool keep = false, outside = false;
        int id = 0;
        float x = 0, y = 0;
        if (i < n && status[b0 + i]) {
            x = cur[2 * (size_t)(b0 + i)]; y = cur[2 * (size_t)(b0 + i) + 1];
            const long idx = klt_mask_index(x, y, cols, rows);
            if (idx >= (long)rows * cols) outside = true;
            else if (idx >= 0) { id = mask[idx]; keep = id != 0; } // 0 <= idx < rows * cols: inside this pair's mask
        }
        // block_rank (common.h) written out: the count of `outside` rides on its two barriers
        const unsigned long long b = __ballot(keep), bo = __ballot(outside);
        if (lane == 0) { s_wave[wave] = __popcll(b); s_wout[wave] = __popcll(bo); }
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < HS_WAVES; w++) { const int v = s_wave[w]; before += w < wave ? v : 0; all += v; beyond += s_wout[w]; }
        __syncthreads();
        if (keep) {
            const int pos = b0 + good + before + wave_rank(b, lane); // < b0 + n
            kept[pos] = i; kept_pts[2 * (size_t)pos] = x; kept_pts[2 * (size_t)pos + 1] = y; object_id[pos] = id - 1;
        }
        good += all;
    }
    if (tid == 0) { counts[2 * p] = good; counts[2 * p + 1] = beyond; }
}

constexpr int TS_THREADS = 256, TS_WAVES = TS_THREADS / 64; // one workgroup walks a frame's few hundred to few thousand points in passes of 256
// ORBmatcher.cc:1591-1603: the last frame's key points that are tracked, in index order.  One workgroup.  counts[0] = their number.
__global__ void __launch_bounds__(TS_THREADS) klt_tracking_select(int n_last, const cs_keypoint *__restrict__ last_keys, const uint8_t *__restrict__ eligible, int *__restrict__ sel,
                                                                  float *__restrict__ pts, int *__restrict__ counts) {
    __shared__ int s_wave[TS_WAVES];
    const int tid = threadIdx.x;
    int n = 0;
    for (int start = 0; start < n_last; start += TS_THREADS) {
        const int i = start + tid;
        const bool keep = i < n_last && eligible[i] && last_keys[i].octave < 3;
        int all;
        const int rank = block_rank<TS_WAVES>(keep, s_wave, &all);
        if (keep) {
            const int pos = n + rank; // < n_last
            sel[pos] = i; pts[2 * pos] = last_keys[i].x; pts[2 * pos + 1] = last_keys[i].y;
        }
        n += all;
    }
    if (tid == 0) counts[0] = n;
}

struct AssignP { KltGridP G; int n, numobject; float th; };
// ORBmatcher.cc:1629-1716 behind the optical flow.  One workgroup: a thread per object adds its flows in index order, a thread per point runs the direction test and
// Frame::GetCloestFeaturesInArea; the sequential assignment (the last i keeps a key point) is an atomic maximum over the points' indices, which ascend with i.
// counts[1 .. 4] = kltmatches, goodmatches, findfeaturematches, uniquematches; counts[5] = 1: a tracked point's object id is outside [0, numobject).
__global__ void __launch_bounds__(TS_THREADS) klt_tracking_assign(AssignP P, const int *__restrict__ cell_start, const KltCellRec *__restrict__ recs, const cs_keypoint *__restrict__ last_keys,
                                                                  const int *__restrict__ object_id, const int *__restrict__ sel, const float *__restrict__ last_pts, float *cur_pts,
                                                                  const uint8_t *__restrict__ status, const float *__restrict__ scale_factors, const uint8_t *__restrict__ keys_static,
                                                                  const uint8_t *__restrict__ had_map_point, float *mean, int *train_match, int *counts) {
    __shared__ int s_cnt[4], s_bad;
    const int tid = threadIdx.x;
    if (tid < 4) s_cnt[tid] = 0;
    if (tid == 0) s_bad = 0;
    for (int k = tid; k < P.G.N; k += TS_THREADS) train_match[k] = -1;
    __syncthreads();
    for (int i = tid; i < P.n; i += TS_THREADS)
        if (status[i] && (object_id[sel[i]] < 0 || object_id[sel[i]] >= P.numobject)) s_bad = 1;
    __syncthreads();
    if (s_bad) { if (tid == 0) counts[5] = 1; return; }
    for (int o = tid; o < P.numobject; o += TS_THREADS) klt_object_mean(P.n, status, sel, object_id, cur_pts, last_pts, o, mean + 3 * (size_t)o);
    __syncthreads();
    for (int i = tid; i < P.n; i += TS_THREADS) {
        int best;
        float cx = cur_pts[2 * i], cy = cur_pts[2 * i + 1];
        const int li = sel[i];
        const int bits = klt_tracking_point(status[i] != 0, last_pts[2 * i], last_pts[2 * i + 1], &cx, &cy, status[i] ? mean + 3 * (size_t)object_id[li] : mean, last_keys[li].octave, P.th,
                                            scale_factors, P.G, cell_start, recs, keys_static, &best);
        cur_pts[2 * i] = cx; cur_pts[2 * i + 1] = cy;
        if (bits & 1) atomicAdd(&s_cnt[0], 1);
        if (bits & 2) atomicAdd(&s_cnt[1], 1);
        if (bits & 4) atomicAdd(&s_cnt[2], 1);
        if (best >= 0) atomicMax(&train_match[best], li); // 0 <= best < N: an id of the matcher's grid
    }
    __syncthreads();
    int unique = 0;
    for (int k = tid; k < P.G.N; k += TS_THREADS) unique += train_match[k] >= 0 && !(had_map_point && had_map_point[k]);
    if (unique) atomicAdd(&s_cnt[3], unique);
    __syncthreads();
    if (tid < 4) counts[1 + tid] = s_cnt[tid];
    if (tid == 0) counts[5] = 0;
}
} // namespace

namespace {
// nullptr, or what is wrong with the pairs and points of a call
const char *track_check(int n_frames, int n_pairs, const int *pair_prev, const int *pair_next, const int *first, const float *prev_pts, bool outputs) {
    if (n_pairs < 1 || !pair_prev || !pair_next || !first) return "a null argument or no pair";
    if (first[0] != 0) return "first[0] is not 0";
    for (int p = 0; p < n_pairs; p++) {
        if (first[p + 1] < first[p]) return "first decreases";
        if (pair_prev[p] < 0 || pair_prev[p] >= n_frames || pair_next[p] < 0 || pair_next[p] >= n_frames) return "a pair names a frame that is not set";
    }
    if (first[n_pairs] > 0 && (!prev_pts || !outputs)) return "points without prev_pts or an output array";
    for (long i = 0; i < 2 * (long)first[n_pairs]; i++)
        if (!std::isfinite(prev_pts[i])) return "a point that is not finite";
    return nullptr;
}
int image_check(const void *gray, int n_frames, int width, int height, long stride) {
    return gray && n_frames >= 1 && width > KLT_WIN && height > KLT_WIN && stride >= width ? CS_OK : CS_ERR_BAD_ARG; // (a level 0 of 21 or less has no window in it)
}
// the tracker over the handle's frames; the results stay in d_next / d_status / d_err
int track_device(cs_ctx *ctx, cs_klt *h, cs_scratch &sc, int n_pairs, const int *pair_prev, const int *pair_next, const int *first, const float *prev_pts, int **d_first_out) {
    const int total = first[n_pairs];
    int *d_first = nullptr, *d_pp = nullptr, *d_pn = nullptr;
    CS_TRY(sc.upload(ctx, &d_first, first, (size_t)n_pairs + 1));
    CS_TRY(sc.upload(ctx, &d_pp, pair_prev, (size_t)n_pairs));
    CS_TRY(sc.upload(ctx, &d_pn, pair_next, (size_t)n_pairs));
    CS_TRY(cs_h2d(ctx, h->d_prev, prev_pts, 2 * (size_t)total));
    if (total > 0) {
        TrackP P{h->L, n_pairs, total};
        CS_LAUNCH(ctx, "klt_track", klt_track, dim3((total + TK_PTS - 1) / TK_PTS), dim3(TK_THREADS), 0, P, d_first, d_pp, d_pn, h->d_img, h->d_der, h->d_prev, h->d_next,
                  h->d_status, h->d_err);
    }
    CS_HIP(ctx, hipGetLastError());
    *d_first_out = d_first;
    return CS_OK;
}
int fail(cs_ctx *ctx, const char *fn, const char *what, int status) {
    if (ctx) ctx->err = std::string(fn) + ": " + what;
    return status;
}
// kept / kept_pts / object_id of the pairs one behind the other, from the pairs' own slots
void pack_kept(int n_pairs, const int *first, const int *counts, const int *s_kept, const float *s_pts, const int *s_id, int *kept_first, int *kept, float *kept_pts,
               int *object_id, int *goodmatches, int *n_mask_outside) {
    kept_first[0] = 0;
    for (int p = 0; p < n_pairs; p++) {
        const int n = counts[2 * p], to = kept_first[p], from = first[p];
        std::copy(s_kept + from, s_kept + from + n, kept + to);
        std::copy(s_pts + 2 * (size_t)from, s_pts + 2 * ((size_t)from + n), kept_pts + 2 * (size_t)to);
        std::copy(s_id + from, s_id + from + n, object_id + to);
        goodmatches[p] = n; kept_first[p + 1] = to + n;
        if (n_mask_outside) n_mask_outside[p] = counts[2 * p + 1];
    }
}
} // namespace

extern "C" {

void cs_klt_destroy(cs_ctx *ctx, cs_klt *h) {
    if (!h) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    h->own.free_all(ctx);
    delete h;
}

int cs_klt_create(cs_ctx *ctx, int max_frames, int max_width, int max_height, int max_points, cs_klt **out) {
    if (!ctx || !out || max_frames < 1 || max_width <= KLT_WIN || max_height <= KLT_WIN || max_points < 1) return CS_ERR_BAD_ARG;
    *out = nullptr;
    const KltLayout L = klt_layout(max_width, max_height);
    if (L.img_frame > INT_MAX) return CS_ERR_BAD_ARG; // (a level is indexed with ints)
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_klt *h = new (std::nothrow) cs_klt();
    if (!h) return CS_ERR_NOMEM;
    h->max_frames = max_frames; h->max_w = max_width; h->max_h = max_height; h->max_points = max_points;
    cs_owner &o = h->own;
    const size_t n = (size_t)max_points;
    if (o.alloc(ctx, &h->d_gray, (size_t)max_width * max_height * max_frames) != CS_OK || o.alloc(ctx, &h->d_img, (size_t)L.img_frame * max_frames) != CS_OK ||
        o.alloc(ctx, &h->d_der, (size_t)L.der_frame * 2 * max_frames) != CS_OK || o.alloc(ctx, &h->d_prev, 2 * n) != CS_OK || o.alloc(ctx, &h->d_next, 2 * n) != CS_OK ||
        o.alloc(ctx, &h->d_status, n) != CS_OK || o.alloc(ctx, &h->d_err, n) != CS_OK) {
        (void)hipGetLastError();
        ctx->err = "cs_klt_create: out of device memory";
        cs_klt_destroy(ctx, h);
        return CS_ERR_NOMEM;
    }
    *out = h;
    return CS_OK;
}

int cs_klt_set_frames(cs_ctx *ctx, cs_klt *h, int n_frames, int width, int height, const uint8_t *gray, long stride_bytes) {
    if (!ctx || !h) return CS_ERR_BAD_ARG;
    if (image_check(gray, n_frames, width, height, stride_bytes) != CS_OK) return fail(ctx, "cs_klt_set_frames", "no image, an image of 21 pixels or less a side, or rows that overlap", CS_ERR_BAD_ARG);
    if (n_frames > h->max_frames || width > h->max_w || height > h->max_h) return fail(ctx, "cs_klt_set_frames", "more frames or a larger image than the handle was created for", CS_ERR_CAPACITY);
    CS_HIP(ctx, hipSetDevice(ctx->device));
    h->n_frames = 0; // the upload overwrites the frames the handle had: it holds none until the new ones are complete
    CS_HIP(ctx, hipMemcpy2DAsync(h->d_gray, (size_t)width, gray, (size_t)stride_bytes, (size_t)width, (size_t)height * n_frames, hipMemcpyHostToDevice, ctx->stream));
    const KltLayout L = klt_layout(width, height);
    for (int l = 0; l < L.n_levels; l++) {
        LevelP P{};
        P.l = l; P.w = L.w[l]; P.h = L.h[l]; P.pw = P.w + 2 * KLT_PAD; P.ph = P.h + 2 * KLT_PAD; P.off = L.img_off[l]; P.frame = L.img_frame; P.gray_frame = (long)width * height;
        if (l) { P.uw = L.w[l - 1]; P.uh = L.h[l - 1]; P.up_off = L.img_off[l - 1]; }
        for (int f0 = 0; f0 < n_frames; f0 += KLT_GRID_Y) { // (a grid's y extent ends at 65 535)
            P.f0 = f0;
            const dim3 grid((P.pw * P.ph + 255) / 256, std::min(KLT_GRID_Y, n_frames - f0));
            CS_LAUNCH(ctx, "klt_level", klt_level, grid, dim3(256), 0, P, h->d_gray, h->d_img);
            CS_LAUNCH(ctx, "klt_scharr", klt_scharr, grid, dim3(256), 0, P, h->d_img, h->d_der);
        }
    }
    CS_HIP(ctx, hipGetLastError());
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the caller's images are free when the call returns
    h->L = L; h->W = width; h->H = height; h->n_frames = n_frames; // ... and only now does the handle describe them
    return CS_OK;
}

int cs_klt_levels(const cs_klt *h) { return h && h->n_frames > 0 ? h->L.n_levels : 0; }

int cs_klt_read_level(cs_ctx *ctx, cs_klt *h, int frame, int level, uint8_t *image, int16_t *deriv) {
    if (!ctx || !h || frame < 0 || frame >= h->n_frames || level < 0 || level >= h->L.n_levels) return CS_ERR_BAD_ARG;
    const size_t n = (size_t)(h->L.w[level] + 2 * KLT_PAD) * (h->L.h[level] + 2 * KLT_PAD);
    CS_HIP(ctx, hipSetDevice(ctx->device));
    if (image) CS_TRY(cs_d2h(ctx, image, h->d_img + (size_t)frame * h->L.img_frame + h->L.img_off[level], n));
    if (deriv) CS_TRY(cs_d2h(ctx, deriv, (int16_t *)h->d_der + 2 * ((size_t)frame * h->L.der_frame + h->L.der_off[level]), 2 * n));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_klt_track(cs_ctx *ctx, cs_klt *h, int n_pairs, const int *pair_prev, const int *pair_next, const int *first, const float *prev_pts, float *next_pts, uint8_t *status,
                 float *err) {
    if (!ctx || !h) return CS_ERR_BAD_ARG;
    if (h->n_frames < 1) return fail(ctx, "cs_klt_track", "no frames are set", CS_ERR_BAD_ARG);
    if (const char *what = track_check(h->n_frames, n_pairs, pair_prev, pair_next, first, prev_pts, next_pts && status && err)) return fail(ctx, "cs_klt_track", what, CS_ERR_BAD_ARG);
    const size_t total = (size_t)first[n_pairs];
    if (total > (size_t)h->max_points) return fail(ctx, "cs_klt_track", "more points than the handle was created for", CS_ERR_CAPACITY);
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    int *d_first = nullptr;
    CS_TRY(track_device(ctx, h, sc, n_pairs, pair_prev, pair_next, first, prev_pts, &d_first));
    CS_TRY(cs_d2h(ctx, next_pts, h->d_next, 2 * total));
    CS_TRY(cs_d2h(ctx, status, h->d_status, total));
    CS_TRY(cs_d2h(ctx, err, h->d_err, total));
    return sc.drain();
}

int cs_klt_track_host(const uint8_t *gray, int n_frames, int width, int height, long stride_bytes, int n_pairs, const int *pair_prev, const int *pair_next, const int *first,
                      const float *prev_pts, float *next_pts, uint8_t *status, float *err) {
    if (image_check(gray, n_frames, width, height, stride_bytes) != CS_OK || klt_layout(width, height).img_frame > INT_MAX) return CS_ERR_BAD_ARG;
    if (track_check(n_frames, n_pairs, pair_prev, pair_next, first, prev_pts, next_pts && status && err)) return CS_ERR_BAD_ARG;
    klt_track_host(gray, n_frames, width, height, stride_bytes, stride_bytes * height, n_pairs, pair_prev, pair_next, first, prev_pts, next_pts, status, err);
    return CS_OK;
}

int cs_match_by_tracking_harris(cs_ctx *ctx, cs_klt *h, int n_pairs, const int *pair_prev, const int *pair_next, const int *first, const float *last_pts, const uint8_t *masks,
                                float *this_pts, uint8_t *status, float *err, int *kept_first, int *kept, float *kept_pts, int *object_id, int *goodmatches,
                                int *n_mask_outside) {
    if (!ctx || !h) return CS_ERR_BAD_ARG;
    if (h->n_frames < 1) return fail(ctx, "cs_match_by_tracking_harris", "no frames are set", CS_ERR_BAD_ARG);
    if (const char *what = track_check(h->n_frames, n_pairs, pair_prev, pair_next, first, last_pts, this_pts && status && err && kept && kept_pts && object_id))
        return fail(ctx, "cs_match_by_tracking_harris", what, CS_ERR_BAD_ARG);
    if (!masks || !kept_first || !goodmatches) return fail(ctx, "cs_match_by_tracking_harris", "a null argument", CS_ERR_BAD_ARG);
    const size_t total = (size_t)first[n_pairs];
    if (total > (size_t)h->max_points) return fail(ctx, "cs_match_by_tracking_harris", "more points than the handle was created for", CS_ERR_CAPACITY);
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    int *d_first = nullptr, *d_kept = nullptr, *d_id = nullptr, *d_counts = nullptr;
    float *d_kpts = nullptr;
    uint8_t *d_masks = nullptr;
    CS_TRY(sc.upload(ctx, &d_masks, masks, (size_t)n_pairs * h->W * h->H));
    CS_TRY(track_device(ctx, h, sc, n_pairs, pair_prev, pair_next, first, last_pts, &d_first));
    CS_TRY(sc.alloc(ctx, &d_kept, total));
    CS_TRY(sc.alloc(ctx, &d_id, total));
    CS_TRY(sc.alloc(ctx, &d_kpts, 2 * total));
    CS_TRY(sc.alloc(ctx, &d_counts, 2 * (size_t)n_pairs));
    CS_LAUNCH(ctx, "klt_harris_select", klt_harris_select, dim3(n_pairs), dim3(HS_THREADS), 0, d_first, h->d_next, h->d_status, d_masks, h->W, h->H, d_kept, d_kpts, d_id, d_counts);
    CS_HIP(ctx, hipGetLastError());
    std::vector<int> counts(2 * (size_t)n_pairs), s_kept(total), s_id(total);
    std::vector<float> s_pts(2 * total);
    CS_TRY(cs_d2h(ctx, this_pts, h->d_next, 2 * total));
    CS_TRY(cs_d2h(ctx, status, h->d_status, total));
    CS_TRY(cs_d2h(ctx, err, h->d_err, total));
    CS_TRY(cs_d2h(ctx, counts.data(), d_counts, counts.size()));
    CS_TRY(cs_d2h(ctx, s_kept.data(), d_kept, total));
    CS_TRY(cs_d2h(ctx, s_id.data(), d_id, total));
    CS_TRY(cs_d2h(ctx, s_pts.data(), d_kpts, 2 * total));
    CS_TRY(sc.drain());
    pack_kept(n_pairs, first, counts.data(), s_kept.data(), s_pts.data(), s_id.data(), kept_first, kept, kept_pts, object_id, goodmatches, n_mask_outside);
    return CS_OK;
}

int cs_match_by_tracking(cs_ctx *ctx, cs_matcher *m, cs_klt *h, int last_frame, int current_frame, int n_last, const cs_keypoint *last_keys, const uint8_t *eligible,
                         const int *object_id, int numobject, float th, const float *scale_factors, int n_levels, const uint8_t *keys_static, const uint8_t *had_map_point,
                         int *train_match, int *n_tracked, int *sel, float *klt_last, float *klt_this, int *counters) {
    if (!ctx || !m || !h) return CS_ERR_BAD_ARG;
    cs_matcher_grid_view V;
    CS_TRY(cs_matcher_device_grid(m, &V));
    if (h->n_frames < 1 || last_frame < 0 || last_frame >= h->n_frames || current_frame < 0 || current_frame >= h->n_frames)
        return fail(ctx, "cs_match_by_tracking", "a frame that is not set", CS_ERR_BAD_ARG);
    if (n_last < 0 || numobject < 0 || n_levels < 3 || !scale_factors || !train_match || !n_tracked || !counters || (n_last > 0 && (!last_keys || !eligible || !object_id || !sel || !klt_last || !klt_this)))
        return fail(ctx, "cs_match_by_tracking", "a null argument, or fewer than three scale factors", CS_ERR_BAD_ARG);
    for (int i = 0; i < n_last; i++)
        if (eligible[i] && last_keys[i].octave < 3 && (last_keys[i].octave < 0 || !std::isfinite(last_keys[i].x) || !std::isfinite(last_keys[i].y)))
            return fail(ctx, "cs_match_by_tracking", "a key point that is not finite or has a negative octave", CS_ERR_BAD_ARG);
    CS_HIP(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k < V.N; k++) train_match[k] = -1;
    counters[0] = counters[1] = counters[2] = counters[3] = 0;
    *n_tracked = 0;
    if (n_last == 0) return CS_OK;
    cs_scratch sc(ctx);
    cs_keypoint *d_keys = nullptr;
    uint8_t *d_elig = nullptr, *d_static = nullptr, *d_had = nullptr;
    int *d_obj = nullptr, *d_sel = nullptr, *d_counts = nullptr, *d_tm = nullptr, *d_first = nullptr;
    float *d_sf = nullptr, *d_mean = nullptr, *d_last = nullptr;
    CS_TRY(sc.upload(ctx, &d_keys, last_keys, (size_t)n_last));
    CS_TRY(sc.upload(ctx, &d_elig, eligible, (size_t)n_last));
    CS_TRY(sc.upload(ctx, &d_obj, object_id, (size_t)n_last));
    CS_TRY(sc.upload(ctx, &d_sf, scale_factors, (size_t)n_levels));
    if (keys_static) CS_TRY(sc.upload(ctx, &d_static, keys_static, (size_t)V.N));
    if (had_map_point) CS_TRY(sc.upload(ctx, &d_had, had_map_point, (size_t)V.N));
    CS_TRY(sc.alloc(ctx, &d_sel, (size_t)n_last));
    CS_TRY(sc.alloc(ctx, &d_last, 2 * (size_t)n_last));
    CS_TRY(sc.alloc(ctx, &d_counts, (size_t)8));
    CS_TRY(sc.alloc(ctx, &d_tm, (size_t)V.N));
    CS_TRY(sc.alloc(ctx, &d_mean, 3 * (size_t)(numobject > 0 ? numobject : 1)));
    CS_LAUNCH(ctx, "klt_tracking_select", klt_tracking_select, dim3(1), dim3(TS_THREADS), 0, n_last, d_keys, d_elig, d_sel, d_last, d_counts);
    CS_HIP(ctx, hipGetLastError());
    int n = 0;
    CS_TRY(cs_d2h(ctx, &n, d_counts, 1));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the launch below is sized by the count
    *n_tracked = n;
    if (n == 0) return CS_OK;
    if (n > h->max_points) return fail(ctx, "cs_match_by_tracking", "more tracked points than the KLT handle was created for", CS_ERR_CAPACITY);
    const int first[2] = {0, n};
    int *d_pp = nullptr, *d_pn = nullptr;
    CS_TRY(sc.upload(ctx, &d_first, first, (size_t)2));
    CS_TRY(sc.upload(ctx, &d_pp, &last_frame, (size_t)1));
    CS_TRY(sc.upload(ctx, &d_pn, &current_frame, (size_t)1));
    TrackP P{h->L, 1, n};
    CS_LAUNCH(ctx, "klt_track", klt_track, dim3((n + TK_PTS - 1) / TK_PTS), dim3(TK_THREADS), 0, P, d_first, d_pp, d_pn, h->d_img, h->d_der, d_last, h->d_next, h->d_status, h->d_err);
    AssignP A{KltGridP{V.N, V.minX, V.minY, V.wInv, V.hInv}, n, numobject, th};
    CS_LAUNCH(ctx, "klt_tracking_assign", klt_tracking_assign, dim3(1), dim3(TS_THREADS), 0, A, V.d_cell_start, (const KltCellRec *)V.d_cell_recs, d_keys, d_obj, d_sel, d_last, h->d_next,
              h->d_status, d_sf, d_static, d_had, d_mean, d_tm, d_counts);
    CS_HIP(ctx, hipGetLastError());
    int counts[8] = {0};
    CS_TRY(cs_d2h(ctx, counts, d_counts, 6));
    CS_TRY(cs_d2h(ctx, sel, d_sel, (size_t)n));
    CS_TRY(cs_d2h(ctx, klt_last, d_last, 2 * (size_t)n));
    CS_TRY(cs_d2h(ctx, klt_this, h->d_next, 2 * (size_t)n));
    CS_TRY(cs_d2h(ctx, train_match, d_tm, (size_t)V.N));
    CS_TRY(sc.drain());
    if (counts[5]) {
        for (int k = 0; k < V.N; k++) train_match[k] = -1;
        return fail(ctx, "cs_match_by_tracking", "a tracked point's object id is outside [0, numobject)", CS_ERR_BAD_ARG);
    }
    for (int c = 0; c < 4; c++) counters[c] = counts[1 + c];
    return CS_OK;
}

int cs_match_by_tracking_host(const uint8_t *last_gray, const uint8_t *current_gray, int width, int height, long stride_bytes, int n_last, const cs_keypoint *last_keys,
                              const uint8_t *eligible, const int *object_id, int numobject, float th, const float *scale_factors, int n_levels, const cs_keypoint *keysUn, int N,
                              float minX, float maxX, float minY, float maxY, const uint8_t *keys_static, const uint8_t *had_map_point, int *train_match, int *n_tracked, int *sel,
                              float *klt_last, float *klt_this, int *counters) {
    if (image_check(last_gray, 1, width, height, stride_bytes) != CS_OK || !current_gray || n_last < 0 || N < 0 || numobject < 0 || n_levels < 3 || !scale_factors || !train_match ||
        !n_tracked || !counters || !(maxX > minX) || !(maxY > minY) || (N > 0 && !keysUn) || (n_last > 0 && (!last_keys || !eligible || !object_id || !sel || !klt_last || !klt_this)))
        return CS_ERR_BAD_ARG;
    for (int i = 0; i < n_last; i++)
        if (eligible[i] && last_keys[i].octave < 3 && (last_keys[i].octave < 0 || !std::isfinite(last_keys[i].x) || !std::isfinite(last_keys[i].y))) return CS_ERR_BAD_ARG;
    static_assert(sizeof(cs_keypoint) == 7 * sizeof(float), "pt is the first two floats of a 28-byte record");
    const cs_keypoint none{};
    const cs_keypoint *lk = n_last ? last_keys : &none, *ck = N ? keysUn : &none;
    const int n = klt_search_by_tracking_host(last_gray, current_gray, width, height, stride_bytes, n_last, &lk->x, &lk->octave, 7, eligible, object_id, numobject, th, scale_factors,
                                              klt_grid_params(N, minX, maxX, minY, maxY), &ck->x, &ck->octave, 7, keys_static, had_map_point, train_match, sel, klt_last, klt_this, counters);
    if (n < 0) return CS_ERR_BAD_ARG;
    *n_tracked = n;
    return CS_OK;
}

int cs_match_by_tracking_harris_host(const uint8_t *gray, int n_frames, int width, int height, long stride_bytes, int n_pairs, const int *pair_prev, const int *pair_next,
                                     const int *first, const float *last_pts, const uint8_t *masks, float *this_pts, uint8_t *status, float *err, int *kept_first, int *kept,
                                     float *kept_pts, int *object_id, int *goodmatches, int *n_mask_outside) {
    if (!masks || !kept_first || !goodmatches || !kept || !kept_pts || !object_id) return CS_ERR_BAD_ARG;
    CS_TRY(cs_klt_track_host(gray, n_frames, width, height, stride_bytes, n_pairs, pair_prev, pair_next, first, last_pts, this_pts, status, err));
    kept_first[0] = 0;
    for (int p = 0; p < n_pairs; p++) {
        const int b0 = first[p], to = kept_first[p];
        int outside = 0;
        const int good = klt_harris_select_host(first[p + 1] - b0, this_pts + 2 * (size_t)b0, status + b0, masks + (size_t)p * width * height, width, height, kept + to,
                                                kept_pts + 2 * (size_t)to, object_id + to, &outside);
        goodmatches[p] = good; kept_first[p + 1] = to + good;
        if (n_mask_outside) n_mask_outside[p] = outside;
    }
    return CS_OK;
}

} // extern "C"
