// stereo.hip -- ORB_SLAM2::Frame::ComputeStereoMatches on MI355X (gfx950).
//
// Replaces Frame::ComputeStereoMatches (reference orb_object_slam/src/Frame.cc:611-783, called at :118 right after the two ORB
// extractions) for a batch of rectified stereo pairs.  Everything it reads is resident after cs_orb_run: the key points and
// descriptors of both images (cs_orb_device_frame) and both pyramids (cs_orb_device_pyramid).  Results (mvuRight, mvDepth) stay
// on the device, packed in the order of the left frames' key points, until cs_stereo_read*.
//
//   stereo_prep    per right key point: the rows of the reference's table it would be entered in (:625-636, floor(y - r) .. ceil(y + r),
//                  r = 2 * mvScaleFactors[octave]) with x and octave as one 16-byte record; per pair the first right key point of every level
//   stereo_match   sixteen lanes per left key point stride over the right records of its pair's levels levelL - 1 .. levelL + 1: row, octave (:676) and
//                  minU <= x <= maxU (:659-663, :681) tests, 256-bit Hamming distance (4 x popcount(u64)) for the survivors, minimum
//                  of (dist << 32 | iR) = the reference's strict `<` over increasing iR (:686); below TH_HIGH or no match
//   stereo_sad     one wave per left key point with a match: the 11 x 11 left patch and the 11 x 21 right strip of the LEFT key point's
//                  level in LDS, 121 (shift, row) partial sums in integers (every sum <= 121 * 510, equal to the reference's float /
//                  cv::norm sums), then one lane runs :737-765 in float in the written operation order (no FMA contraction: the
//                  Makefile's -ffp-contract=off; `/` is the correctly rounded IEEE division, hipcc's default)
//   stereo_cut     one workgroup per pair: the order statistic n/2 of the accepted SAD values (:769-771, sort + [size/2]) by a two-level
//                  256-bin histogram in LDS, thDist = 1.5f * 1.4f * median, reset of every match at or above it (:773-782), count
//
// One stream, no host round trip and no synchronisation between the passes.
//
// What the reference leaves undefined is guarded and ends as "unmatched" (-1 / -1): a left key point whose (int)y is outside
// [0, rows) (the reference indexes vRowIndices with it), a right key point whose row span leaves [0, rows) or whose octave is
// not a level (it takes no part), an 11 x 11 patch or 11 x 21 strip that leaves the level image (an OpenCV exception in the
// reference), and n == 0 accepted matches (the reference indexes an empty vector).  None of these occurs for key points that
// come from the extractor: they lie >= 19 level pixels from every border, and a right key point at most one level away
// is >= 15 level pixels in.
#include "common.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <new>
#include <vector>

namespace {
constexpr int TH_HIGH = 100;     // ORBmatcher.cc:42
constexpr int SW = 5, SL = 5;    // w, L of Frame.cc:706, :714
constexpr int PATCH = 2 * SW + 1, STRIP = 2 * (SW + SL) + 1, NSHIFT = 2 * SL + 1;
constexpr int GROUP = 16;        // lanes per left key point in stereo_match

struct StereoP {
    int nlevels, rows;           // rows = mvImagePyramid[0].rows
    long off[CS_ORB_MAX_LEVELS];
    int w[CS_ORB_MAX_LEVELS], h[CS_ORB_MAX_LEVELS];
    float scale[CS_ORB_MAX_LEVELS], inv_scale[CS_ORB_MAX_LEVELS];
    float bf, maxD;              // mbf, mbf / mb
};
struct PairRec { int l0, nl, r0, nr; }; // first key point and count of the pair's left / right frame, relative to the call's first left / right frame
struct RightRec { float x; int ylo, yhi, octave; };

// Also the first right key point of every level (lvl[pair][l], lvl[pair][nlevels] = Nr): the extractor emits a frame's key points level-major
// (ORBextractor.cc:1065-1098), so the octaves levelL - 1 .. levelL + 1 of :676 are one contiguous range and stereo_match walks only that.
__global__ void __launch_bounds__(256) stereo_prep(StereoP P, const PairRec *__restrict__ pairs, const cs_keypoint *__restrict__ kpsR, RightRec *__restrict__ rec,
                                                   int *__restrict__ lvl) {
    const PairRec pr = pairs[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    int *lv = lvl + (size_t)blockIdx.y * (CS_ORB_MAX_LEVELS + 1);
    if (pr.nr == 0 && j <= P.nlevels) lv[j] = 0;
    if (j >= pr.nr) return;
    const int i = pr.r0 + j;
    const float x = kpsR[i].x, y = kpsR[i].y;
    const int oct = kpsR[i].octave;
    RightRec r{x, 1, 0, oct}; // an empty row span: takes no part
    if (oct >= 0 && oct < P.nlevels) {
        const float rad = 2.0f * P.scale[oct];
        const int maxr = (int)ceilf(y + rad), minr = (int)floorf(y - rad);
        if (minr >= 0 && maxr < P.rows) { r.ylo = minr; r.yhi = maxr; }
    }
    rec[i] = r;
    const int here = min(max(oct, 0), P.nlevels - 1), before = j == 0 ? -1 : min(max(kpsR[i - 1].octave, 0), P.nlevels - 1);
    for (int l = before + 1; l <= here; l++) lv[l] = j;
    if (j == pr.nr - 1) for (int l = here + 1; l <= P.nlevels; l++) lv[l] = pr.nr;
}

__global__ void __launch_bounds__(256) stereo_match(StereoP P, const PairRec *__restrict__ pairs, const cs_keypoint *__restrict__ kpsL,
                                                    const unsigned long long *__restrict__ descL, const RightRec *__restrict__ rec,
                                                    const unsigned long long *__restrict__ descR, const int *__restrict__ lvl, int *__restrict__ best) {
    const PairRec pr = pairs[blockIdx.y];
    const int iL = blockIdx.x * (256 / GROUP) + (threadIdx.x / GROUP), sub = threadIdx.x % GROUP;
    const bool live = iL < pr.nl;
    const int o = pr.l0 + (live ? iL : 0);
    int j0 = 0, nr = 0, vL = 0, lv = 0;
    float minU = 0, maxU = 0;
    unsigned long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    if (live && pr.nl > 0) {
        const float uL = kpsL[o].x, fv = kpsL[o].y;
        lv = kpsL[o].octave;
        minU = uL - P.maxD; maxU = uL + 3.0f; // uL - minD, minD = -3
        vL = (fv >= 0.0f && fv < (float)P.rows) ? (int)fv : -1;
        if (vL >= 0 && !(maxU < 0) && lv >= 0 && lv < P.nlevels) { // the right key points of levels lv - 1 .. lv + 1
            const int *ls = lvl + (size_t)blockIdx.y * (CS_ORB_MAX_LEVELS + 1);
            j0 = max(ls[max(lv - 1, 0)], 0); nr = min(ls[min(lv + 1, P.nlevels - 1) + 1], pr.nr); // clamped: key points that are not level-major must not lead outside the pair
        }
        const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(descL + (size_t)o * 4), b = *reinterpret_cast<const ulonglong2 *>(descL + (size_t)o * 4 + 2);
        d0 = a.x; d1 = a.y; d2 = b.x; d3 = b.y;
    }
    unsigned long long key = ((unsigned long long)TH_HIGH << 32) | 0xffffffffull;
    for (int j = j0 + sub; j < nr; j += GROUP) {
        const int4 q = *reinterpret_cast<const int4 *>(rec + pr.r0 + j);
        const float uR = __int_as_float(q.x);
        if (q.y <= vL && vL <= q.z && q.w >= lv - 1 && q.w <= lv + 1 && uR >= minU && uR <= maxU) {
            const unsigned long long *e = descR + (size_t)(pr.r0 + j) * 4;
            const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(e), b = *reinterpret_cast<const ulonglong2 *>(e + 2);
            const unsigned long long ab[4] = {a.x, a.y, b.x, b.y};
            const int dist = hamming256(ab, d0, d1, d2, d3);
            const unsigned long long k = ((unsigned long long)dist << 32) | (unsigned)j;
            key = k < key ? k : key;
        }
    }
    for (int m = GROUP / 2; m >= 1; m >>= 1) {
        const unsigned long long other = __shfl_xor(key, m, GROUP);
        key = other < key ? other : key;
    }
    if (live && sub == 0) best[o] = (int)(key >> 32) < TH_HIGH ? (int)(key & 0xffffffffu) : -1;
}

__global__ void __launch_bounds__(64) stereo_sad(StereoP P, const PairRec *__restrict__ pairs, const cs_keypoint *__restrict__ kpsL, const cs_keypoint *__restrict__ kpsR,
                                                 const int *__restrict__ best, const uint8_t *__restrict__ pyrL, const uint8_t *__restrict__ pyrR, long frame_strideL,
                                                 long frame_strideR, float *__restrict__ u_right, float *__restrict__ depth, int *__restrict__ sad) {
    __shared__ int sLeft[PATCH * PATCH], sRight[PATCH * STRIP], sPart[NSHIFT * PATCH], sDist[NSHIFT];
    const int p = blockIdx.y, lane = threadIdx.x;
    const PairRec pr = pairs[p];
    if ((int)blockIdx.x >= pr.nl) return; // the whole workgroup (one wave) leaves
    const int o = pr.l0 + blockIdx.x;
    const int bR = best[o];
    float out_u = -1.0f, out_d = -1.0f;
    int out_s = -1;
    const int lv = kpsL[o].octave;
    if (bR >= 0 && lv >= 0 && lv < P.nlevels) {
        const float uL = kpsL[o].x, vL = kpsL[o].y, uR0 = kpsR[pr.r0 + bR].x;
        const float s = P.inv_scale[lv];
        const int su = (int)roundf(uL * s), sv = (int)roundf(vL * s), sr = (int)roundf(uR0 * s); // scaleduL, scaledvL, scaleduR0 (:699-701)
        const int w = P.w[lv], h = P.h[lv];
        // :716-719 (iniu = scaleduR0 + L - w, endu = scaleduR0 + L + w + 1) and the reads the reference leaves to cv::Mat's range checks
        const bool inside = sv - SW >= 0 && sv + SW < h && su - SW >= 0 && su + SW < w && sr - SW - SL >= 0 && sr + SL + SW < w;
        if (inside && !(sr + SL - SW < 0 || sr + SL + SW + 1 >= w)) {
            const uint8_t *imL = pyrL + (long)p * frame_strideL + P.off[lv] + (long)(sv - SW) * w + (su - SW);
            const uint8_t *imR = pyrR + (long)p * frame_strideR + P.off[lv] + (long)(sv - SW) * w + (sr - SW - SL);
            for (int t = lane; t < PATCH * PATCH; t += 64) sLeft[t] = imL[(t / PATCH) * w + t % PATCH];
            for (int t = lane; t < PATCH * STRIP; t += 64) sRight[t] = imR[(t / STRIP) * w + t % STRIP];
            __syncthreads();
            const int cL = sLeft[SW * PATCH + SW];
            for (int t = lane; t < NSHIFT * PATCH; t += 64) {
                const int shift = t / PATCH, row = t % PATCH;
                const int cR = sRight[SW * STRIP + shift + SW];
                int acc = 0;
#pragma unroll
                for (int c = 0; c < PATCH; c++) acc += abs((sLeft[row * PATCH + c] - cL) - (sRight[row * STRIP + shift + c] - cR));
                sPart[t] = acc;
            }
            __syncthreads();
            if (lane < NSHIFT) {
                int acc = 0;
                for (int r = 0; r < PATCH; r++) acc += sPart[lane * PATCH + r];
                sDist[lane] = acc;
            }
            __syncthreads();
            if (lane == 0) {
                int bestDist = INT_MAX, bestincR = 0;
                for (int i = 0; i < NSHIFT; i++)
                    if (sDist[i] < bestDist) { bestDist = sDist[i]; bestincR = i - SL; }
                if (bestincR != -SL && bestincR != SL) {
                    const float dist1 = (float)sDist[SL + bestincR - 1], dist2 = (float)sDist[SL + bestincR], dist3 = (float)sDist[SL + bestincR + 1];
                    const float deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2)); // :745
                    // The test of :748 is kept as written but cannot fail: dist2 is the strict first minimum of integers, so dist1 > dist2 and dist3 >= dist2, the
                    // denominator is >= 2 and |dist1 - dist3| <= dist1 + dist3 - 2 * dist2 (all exact in float, below 2^24): |deltaR| <= 0.5, never NaN or inf.
                    if (!(deltaR < -1 || deltaR > 1)) {
                        float bestuR = P.scale[lv] * ((float)sr + (float)bestincR + deltaR);
                        float disparity = uL - bestuR;
                        if (disparity >= 0 && disparity < P.maxD) {
                            if (disparity <= 0) { disparity = 0.01; bestuR = uL - 0.01; } // double literals, as written at :759-760
                            out_d = P.bf / disparity; out_u = bestuR; out_s = bestDist;
                        }
                    }
                }
            }
        }
    }
    if (lane == 0) { u_right[o] = out_u; depth[o] = out_d; sad[o] = out_s; }
}

__global__ void __launch_bounds__(256) stereo_cut(const PairRec *__restrict__ pairs, const int *__restrict__ sad, float *__restrict__ u_right, float *__restrict__ depth,
                                                  int *__restrict__ n_matched) {
    __shared__ int hist[256];
    __shared__ int s_bin, s_rank, s_med, s_kept;
    const PairRec pr = pairs[blockIdx.x];
    const int tid = threadIdx.x;
    const int *sd = sad + pr.l0;
    hist[tid] = 0;
    if (tid == 0) s_kept = 0;
    __syncthreads();
    for (int i = tid; i < pr.nl; i += 256) { const int s = sd[i]; if (s >= 0) atomicAdd(&hist[(s >> 8) & 255], 1); } // SAD <= 121 * 510 < 2^16
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int b = 0; b < 256; b++) n += hist[b];
        s_bin = -1; s_rank = 0;
        if (n > 0) {
            int k = n / 2, cum = 0, b = 0;
            while (cum + hist[b] <= k) cum += hist[b++];
            s_bin = b; s_rank = k - cum;
        }
    }
    __syncthreads();
    const int bin = s_bin;
    if (bin < 0) { if (tid == 0) n_matched[blockIdx.x] = 0; return; }
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < pr.nl; i += 256) { const int s = sd[i]; if (s >= 0 && ((s >> 8) & 255) == bin) atomicAdd(&hist[s & 255], 1); }
    __syncthreads();
    if (tid == 0) {
        int cum = 0, b = 0;
        while (cum + hist[b] <= s_rank) cum += hist[b++];
        s_med = (bin << 8) | b;
    }
    __syncthreads();
    const float median = (float)s_med;
    const float thDist = 1.5f * 1.4f * median;
    int kept = 0;
    for (int i = tid; i < pr.nl; i += 256) {
        const int s = sd[i];
        if (s < 0) continue;
        if ((float)s < thDist) kept++;
        else { u_right[pr.l0 + i] = -1.0f; depth[pr.l0 + i] = -1.0f; }
    }
    if (kept) atomicAdd(&s_kept, kept);
    __syncthreads();
    if (tid == 0) n_matched[blockIdx.x] = s_kept;
}
} // namespace

struct cs_stereo {
    int cap = 0, max_pairs = 0;
    cs_owner own;
    // device
    float *d_u_right = nullptr, *d_depth = nullptr;
    int *d_sad = nullptr, *d_best = nullptr, *d_n_matched = nullptr, *d_lvl = nullptr;
    RightRec *d_rec = nullptr;
    PairRec *d_pairs = nullptr;
    cs_keypoint *d_keys_l = nullptr, *d_keys_r = nullptr; // key points and descriptors of cs_stereo_match_from_keys, cap * max_pairs each, allocated by its first call
    unsigned long long *d_desc_l = nullptr, *d_desc_r = nullptr; // (cs_stereo_match_from_orb reads the extractors')
    // host: the last call
    int n_pairs = 0;
    std::vector<PairRec> pairs;
};

namespace {
constexpr float MAX_COORD = 16777216.0f; // 2^24

// The two extractors' resident pyramids, and the geometry checks both entries share.
int pyramids(cs_ctx *ctx, const char *who, const cs_orb *left, int left_first, const cs_orb *right, int right_first, int n_pairs, cs_orb_pyramid_view *VL, cs_orb_pyramid_view *VR) {
    if (cs_orb_device_pyramid(left, VL) != CS_OK || cs_orb_device_pyramid(right, VR) != CS_OK) return CS_ERR_BAD_ARG;
    if (left_first + n_pairs > VL->n_frames || right_first + n_pairs > VR->n_frames) { ctx->err = std::string(who) + ": pairs outside the extractor's last run"; return CS_ERR_BAD_ARG; }
    if (VL->W != VR->W || VL->H != VR->H || VL->nlevels != VR->nlevels || VL->scale_factor != VR->scale_factor) {
        ctx->err = std::string(who) + ": the extractors differ in image size, nlevels or scaleFactor";
        return CS_ERR_BAD_ARG;
    }
    const cs_keypoint *k = nullptr;
    const unsigned long long *d = nullptr;
    int n = 0;
    if (cs_orb_device_frame(left, left_first + n_pairs - 1, &k, &d, &n) != CS_OK || cs_orb_device_frame(right, right_first + n_pairs - 1, &k, &d, &n) != CS_OK) return CS_ERR_BAD_ARG; // no run yet
    return CS_OK;
}

// The four passes over s->pairs (set by the caller), for both entries: kL0 / dL0 / kR0 / dR0 = the device arrays that PairRec::l0 / r0 count from.
int associate(cs_ctx *ctx, cs_stereo *s, const cs_orb_pyramid_view &VL, int left_first, const cs_orb_pyramid_view &VR, int right_first, const cs_keypoint *kL0,
              const unsigned long long *dL0, const cs_keypoint *kR0, const unsigned long long *dR0, float bf, float b) {
    const int n_pairs = s->n_pairs;
    int max_nl = 0, max_nr = 0;
    for (const PairRec &pr : s->pairs) { max_nl = std::max(max_nl, pr.nl); max_nr = std::max(max_nr, pr.nr); }
    StereoP P{};
    P.nlevels = VL.nlevels; P.rows = VL.H; P.bf = bf; P.maxD = bf / b;
    for (int l = 0; l < VL.nlevels; l++) { P.off[l] = VL.off[l]; P.w[l] = VL.w[l]; P.h[l] = VL.h[l]; P.scale[l] = VL.scale[l]; P.inv_scale[l] = VL.inv_scale[l]; }
    int r = cs_h2d(ctx, s->d_pairs, s->pairs.data(), (size_t)n_pairs); if (r) return r;
    CS_LAUNCH(ctx, "stereo_prep", stereo_prep, dim3(std::max((max_nr + 255) / 256, 1), n_pairs), dim3(256), 0, P, s->d_pairs, kR0, s->d_rec, s->d_lvl);
    if (max_nl > 0) {
        CS_LAUNCH(ctx, "stereo_match", stereo_match, dim3((max_nl + 256 / GROUP - 1) / (256 / GROUP), n_pairs), dim3(256), 0, P, s->d_pairs, kL0, dL0, s->d_rec, dR0, s->d_lvl, s->d_best);
        CS_LAUNCH(ctx, "stereo_sad", stereo_sad, dim3(max_nl, n_pairs), dim3(64), 0, P, s->d_pairs, kL0, kR0, s->d_best, VL.d_pyr + (long)left_first * VL.frame_stride,
                  VR.d_pyr + (long)right_first * VR.frame_stride, VL.frame_stride, VR.frame_stride, s->d_u_right, s->d_depth, s->d_sad);
    }
    CS_LAUNCH(ctx, "stereo_cut", stereo_cut, dim3(n_pairs), dim3(256), 0, s->d_pairs, s->d_sad, s->d_u_right, s->d_depth, s->d_n_matched);
    CS_HIP(ctx, hipGetLastError());
    return CS_OK;
}
} // namespace

extern "C" {

void cs_stereo_destroy(cs_ctx *ctx, cs_stereo *s) {
    if (!s) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    s->own.free_all(ctx);
    delete s;
}

int cs_stereo_create(cs_ctx *ctx, int max_keypoints_per_frame, int max_pairs, cs_stereo **out) {
    if (!ctx || !out || max_keypoints_per_frame < 1 || max_pairs < 1 || max_pairs > 65535 || (long)max_keypoints_per_frame * max_pairs > INT_MAX) return CS_ERR_BAD_ARG;
    *out = nullptr;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_stereo *s = new (std::nothrow) cs_stereo();
    if (!s) return CS_ERR_NOMEM;
    s->cap = max_keypoints_per_frame; s->max_pairs = max_pairs;
    const size_t n = (size_t)max_keypoints_per_frame * max_pairs;
    int r = CS_OK;
    cs_owner &o = s->own;
    if (o.alloc(ctx, &s->d_u_right, n) != CS_OK || o.alloc(ctx, &s->d_depth, n) != CS_OK || o.alloc(ctx, &s->d_sad, n) != CS_OK || o.alloc(ctx, &s->d_best, n) != CS_OK ||
        o.alloc(ctx, &s->d_rec, n) != CS_OK || o.alloc(ctx, &s->d_n_matched, (size_t)max_pairs) != CS_OK || o.alloc(ctx, &s->d_pairs, (size_t)max_pairs) != CS_OK ||
        o.alloc(ctx, &s->d_lvl, (size_t)max_pairs * (CS_ORB_MAX_LEVELS + 1)) != CS_OK) { // this call reports a failed allocation as CS_ERR_NOMEM with its own message
        (void)hipGetLastError();
        ctx->err = "cs_stereo_create: out of device memory";
        r = CS_ERR_NOMEM;
    }
    if (r != CS_OK) { cs_stereo_destroy(ctx, s); return r; }
    *out = s;
    return CS_OK;
}

int cs_stereo_match_from_orb(cs_ctx *ctx, cs_stereo *s, const cs_orb *left, int left_first, const cs_orb *right, int right_first, int n_pairs, float bf, float b) {
    if (!ctx || !s || !left || !right || n_pairs < 1 || n_pairs > s->max_pairs || left_first < 0 || right_first < 0 || !(bf > 0.0f) || !(b > 0.0f)) return CS_ERR_BAD_ARG;
    cs_orb_pyramid_view VL, VR;
    CS_TRY(pyramids(ctx, "cs_stereo_match_from_orb", left, left_first, right, right_first, n_pairs, &VL, &VR));
    const cs_keypoint *kL0 = nullptr, *kR0 = nullptr, *k = nullptr;
    const unsigned long long *dL0 = nullptr, *dR0 = nullptr, *d = nullptr;
    int n = 0;
    std::vector<PairRec> pairs((size_t)n_pairs); // the handle keeps its last call until this one is known to be good
    for (int p = 0; p < n_pairs; p++) {
        PairRec &pr = pairs[(size_t)p];
        if (cs_orb_device_frame(left, left_first + p, &k, &d, &n) != CS_OK) return CS_ERR_BAD_ARG; // no run yet
        if (p == 0) { kL0 = k; dL0 = d; }
        pr.l0 = (int)(k - kL0); pr.nl = n;
        if (cs_orb_device_frame(right, right_first + p, &k, &d, &n) != CS_OK) return CS_ERR_BAD_ARG;
        if (p == 0) { kR0 = k; dR0 = d; }
        pr.r0 = (int)(k - kR0); pr.nr = n;
        if (pr.nl > s->cap || pr.nr > s->cap) { ctx->err = "cs_stereo_match_from_orb: a frame has more key points than the handle was created for"; return CS_ERR_CAPACITY; }
    }
    s->pairs.swap(pairs);
    s->n_pairs = n_pairs;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    return associate(ctx, s, VL, left_first, VR, right_first, kL0, dL0, kR0, dR0, bf, b);
}

int cs_stereo_match_from_keys(cs_ctx *ctx, cs_stereo *s, const cs_orb *left, int left_first, const cs_orb *right, int right_first, int n_pairs, const int *firstL,
                              const cs_keypoint *keysL, const uint8_t *descL, const int *firstR, const cs_keypoint *keysR, const uint8_t *descR, float bf, float b) {
    if (!ctx || !s || !left || !right || n_pairs < 1 || n_pairs > s->max_pairs || left_first < 0 || right_first < 0 || !(bf > 0.0f) || !(b > 0.0f)) return CS_ERR_BAD_ARG;
    if (!cs_offsets_ok(firstL, n_pairs, keysL) || !cs_offsets_ok(firstR, n_pairs, keysR) || (firstL[n_pairs] > 0 && !descL) || (firstR[n_pairs] > 0 && !descR)) return CS_ERR_BAD_ARG;
    cs_orb_pyramid_view VL, VR;
    CS_TRY(pyramids(ctx, "cs_stereo_match_from_keys", left, left_first, right, right_first, n_pairs, &VL, &VR));
    std::vector<PairRec> pairs((size_t)n_pairs); // the handle keeps its last call until this one is known to be good
    for (int p = 0; p < n_pairs; p++) {
        PairRec &pr = pairs[(size_t)p];
        pr.l0 = firstL[p]; pr.nl = firstL[p + 1] - firstL[p];
        pr.r0 = firstR[p]; pr.nr = firstR[p + 1] - firstR[p];
        if (pr.nl > s->cap || pr.nr > s->cap) { ctx->err = "cs_stereo_match_from_keys: a frame has more key points than the handle was created for"; return CS_ERR_CAPACITY; }
        for (int j = 1; j < pr.nr; j++)
            if (keysR[pr.r0 + j].octave < keysR[pr.r0 + j - 1].octave) { ctx->err = "cs_stereo_match_from_keys: a right frame's key points are not in level-major order (an octave decreases)"; return CS_ERR_BAD_ARG; }
    }
    // the level coordinates the kernels round to int stay far inside its range
    auto plain = [](const cs_keypoint *k, int n) { for (int i = 0; i < n; i++) if (!(std::fabs(k[i].x) <= MAX_COORD && std::fabs(k[i].y) <= MAX_COORD)) return false; return true; };
    if (!plain(keysL, firstL[n_pairs]) || !plain(keysR, firstR[n_pairs])) { ctx->err = "cs_stereo_match_from_keys: a key point's coordinate is not finite or above 2^24 in magnitude"; return CS_ERR_BAD_ARG; }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->d_keys_l) { // the first call through this entry
        const size_t n = (size_t)s->cap * s->max_pairs;
        cs_owner o;
        if (o.alloc(ctx, &s->d_keys_l, n) != CS_OK || o.alloc(ctx, &s->d_keys_r, n) != CS_OK || o.alloc(ctx, &s->d_desc_l, n * 4) != CS_OK || o.alloc(ctx, &s->d_desc_r, n * 4) != CS_OK) {
            (void)hipGetLastError();
            o.free_all(ctx);
            s->d_keys_l = s->d_keys_r = nullptr; s->d_desc_l = s->d_desc_r = nullptr;
            ctx->err = "cs_stereo_match_from_keys: out of device memory";
            return CS_ERR_NOMEM;
        }
        s->own.adopt(o);
    }
    s->pairs.swap(pairs);
    s->n_pairs = n_pairs;
    CS_TRY(cs_h2d(ctx, s->d_keys_l, keysL, (size_t)firstL[n_pairs]));
    CS_TRY(cs_h2d(ctx, s->d_keys_r, keysR, (size_t)firstR[n_pairs]));
    CS_TRY(cs_h2d(ctx, reinterpret_cast<uint8_t *>(s->d_desc_l), descL, (size_t)firstL[n_pairs] * 32));
    CS_TRY(cs_h2d(ctx, reinterpret_cast<uint8_t *>(s->d_desc_r), descR, (size_t)firstR[n_pairs] * 32));
    CS_TRY(associate(ctx, s, VL, left_first, VR, right_first, s->d_keys_l, s->d_desc_l, s->d_keys_r, s->d_desc_r, bf, b));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the caller's arrays are free when the call returns
    return CS_OK;
}

int cs_stereo_read(cs_ctx *ctx, cs_stereo *s, float *u_right, float *depth, int cap_per_frame, int *counts, int *n_matched) {
    if (!ctx || !s || !u_right || !depth || !counts || !n_matched || cap_per_frame < 1 || s->n_pairs < 1) return CS_ERR_BAD_ARG;
    for (int p = 0; p < s->n_pairs; p++)
        if (s->pairs[(size_t)p].nl > cap_per_frame) return CS_ERR_CAPACITY;
    for (int p = 0; p < s->n_pairs; p++) {
        const PairRec &pr = s->pairs[(size_t)p];
        counts[p] = pr.nl;
        int r = cs_d2h(ctx, u_right + (size_t)p * cap_per_frame, s->d_u_right + pr.l0, (size_t)pr.nl); if (r) return r;
        r = cs_d2h(ctx, depth + (size_t)p * cap_per_frame, s->d_depth + pr.l0, (size_t)pr.nl); if (r) return r;
    }
    int r = cs_d2h(ctx, n_matched, s->d_n_matched, (size_t)s->n_pairs); if (r) return r;
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_stereo_read_packed(cs_ctx *ctx, cs_stereo *s, float *u_right, float *depth, long cap_total, int *first, long *total, int *n_matched) {
    if (!ctx || !s || !first || !total || s->n_pairs < 1) return CS_ERR_BAD_ARG;
    const PairRec &last = s->pairs[(size_t)s->n_pairs - 1];
    const long n = (long)last.l0 + last.nl;
    *total = n;
    for (int p = 0; p < s->n_pairs; p++) first[p] = s->pairs[(size_t)p].l0;
    first[s->n_pairs] = (int)n;
    if (!u_right || !depth) return CS_OK; // size query
    if (n > cap_total) return CS_ERR_CAPACITY;
    int r = cs_d2h(ctx, u_right, s->d_u_right, (size_t)n); if (r) return r;
    r = cs_d2h(ctx, depth, s->d_depth, (size_t)n); if (r) return r;
    if (n_matched) { r = cs_d2h(ctx, n_matched, s->d_n_matched, (size_t)s->n_pairs); if (r) return r; }
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_stereo_device_pair(const cs_stereo *s, int pair, const float **d_u_right, const float **d_depth, int *n) {
    if (!s || !d_u_right || !d_depth || !n || pair < 0 || pair >= s->n_pairs) return CS_ERR_BAD_ARG;
    const PairRec &pr = s->pairs[(size_t)pair];
    *d_u_right = s->d_u_right + pr.l0; *d_depth = s->d_depth + pr.l0; *n = pr.nl;
    return CS_OK;
}

} // extern "C"
