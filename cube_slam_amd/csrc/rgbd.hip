// rgbd.hip -- ORB_SLAM2::Frame::ComputeStereoFromRGBD and Tracking's close-point rule on MI355X (gfx950).
//
// Replaces Frame::ComputeStereoFromRGBD (reference orb_object_slam/src/Frame.cc:785-806, called at :173 of the RGB-D constructor) with the conversion of
// Tracking::GrabImageRGBD (src/Tracking.cc:388) folded into the one sample it reads, and the creation of map points from measured depth in
// Tracking::StereoInitialization (:783-850), UpdateLastFrame (:1207-1274) and CreateNewKeyFrame (:2067-2130).  The arithmetic is rgbd_math.h.
//
//   rgbd_gather        one thread per key point of the whole batch: Frame::UndistortKeyPoints (frame_math.h) or the caller's mvKeysUn, the raw depth sample under
//                      the distorted key point, its conversion, mvDepth / mvuRight; the per-frame counts by one vector atomic per wave and frame
//   rgbd_close_points  one workgroup per frame: ordered compaction of the z > 0 key points into 64-bit keys (bits of z) << 32 | index in LDS, a bitonic network over
//                      the next power of two (padded with all-ones keys), the walked prefix in closed form (rgbd_walked), ordered compaction of its need_new
//                      entries, Frame::UnprojectStereo of those
//
// The depth image is never converted as a whole: 640 x 480 samples against the ~1 000 that are read.  One stream, nothing waits before the read functions.
#include "common.h"
#include "frame_math.h"
#include "rgbd_math.h"

#include <climits>
#include <new>
#include <vector>

static_assert(RGBD_DEPTH_U16 == CS_DEPTH_U16 && RGBD_DEPTH_F32 == CS_DEPTH_F32 && RGBD_CLOSE_NEAREST == CS_CLOSE_POINTS_NEAREST && RGBD_CLOSE_ALL == CS_CLOSE_POINTS_ALL,
              "rgbd_math.h and the C header name the same values");

namespace {
constexpr int CP_THREADS = 1024, CP_WAVES = CP_THREADS / 64;
constexpr int CP_MAX = CS_RGBD_MAX_KEYPOINTS; // keys in LDS
static_assert((CP_MAX & (CP_MAX - 1)) == 0 && CP_MAX >= CP_THREADS, "the bitonic network runs over a power of two");

struct GatherP {
    UndP U;
    int W, H, type, n_frames, total;
    long pitch, frame_bytes; // of the raw depth image
    float bf, factor;
};

// first[f] <= i < first[f + 1]; empty frames are stepped over
__device__ __forceinline__ int frame_of(const int *__restrict__ first, int n_frames, int i) {
    int lo = 0, hi = n_frames; // first[lo] <= i < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// have_un: keysUn already holds the caller's mvKeysUn (cs_rgbd_from_keys); otherwise Frame::UndistortKeyPoints writes it here (cs_rgbd_from_orb)
__global__ void __launch_bounds__(256) rgbd_gather(GatherP P, const int *__restrict__ first, const cs_keypoint *__restrict__ keys, int have_un, const uint8_t *__restrict__ image,
                                                   cs_keypoint *keysUn, float *__restrict__ u_right, float *__restrict__ depth, int *__restrict__ n_with_depth,
                                                   int *__restrict__ n_outside) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < P.total;
    int f = -1;
    bool has = false, outside = false;
    if (live) {
        f = frame_of(first, P.n_frames, i);
        const float x = keys[i].x, y = keys[i].y;
        float xu, yu;
        if (have_un) xu = keysUn[i].x;
        else {
            undistort_point(P.U, x, y, xu, yu);
            cs_keypoint ku = keys[i];
            ku.x = xu; ku.y = yu;
            keysUn[i] = ku;
        }
        int col, row;
        float d = -1.0f;
        if (rgbd_sample_index(x, y, P.W, P.H, &col, &row)) d = rgbd_sample(image + (long)f * P.frame_bytes, P.type, P.pitch, col, row, P.factor);
        else outside = true;
        float ur, dep;
        has = rgbd_associate(d, xu, P.bf, &ur, &dep);
        u_right[i] = ur; depth[i] = dep;
    }
    // a wave covers one frame, or a few at a seam: one atomic per frame present
    const int lane = lane_id();
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int f0 = __shfl(f, leader);
        const bool mine = live && f == f0;
        const unsigned long long same = __ballot(mine), bd = __ballot(mine && has), bo = __ballot(mine && outside);
        if (lane == leader) {
            if (bd) atomicAdd(&n_with_depth[f0], __popcll(bd));
            if (bo) atomicAdd(&n_outside[f0], __popcll(bo));
        }
        todo &= ~same;
    }
}

struct CloseP { float cx, cy, invfx, invfy, th; int mode; };

// counts: n_valid, n_walked, n_new per frame.  order / new_idx / new_x3D: frame f's entries from first[f] (3 * first[f]) on.
// (8 waves per SIMD: two workgroups fit a compute unit by LDS, 2 x 64 KB of 160, and at 64 registers or fewer they fit by registers too.)
__global__ void __launch_bounds__(CP_THREADS, 8) rgbd_close_points(CloseP P, const int *__restrict__ first, const float *__restrict__ depth, const cs_keypoint *__restrict__ keysUn,
                                                               const uint8_t *__restrict__ need_new, const float *__restrict__ Tcw, int *__restrict__ order,
                                                               int *__restrict__ new_idx, float *__restrict__ new_x3D, int *__restrict__ counts) {
    __shared__ unsigned long long s_key[CP_MAX];
    __shared__ int s_wave[CP_WAVES];
    __shared__ int s_close;
    __shared__ float s_Rwc[9], s_Ow[3];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int b0 = first[f], n = min(first[f + 1] - b0, CP_MAX); // (the host has checked n <= CP_MAX)
    if (tid == 0) { s_close = 0; rgbd_pose_matrices(Tcw + 12 * (size_t)f, s_Rwc, s_Ow); }
    __syncthreads();
    // vDepthIdx in push_back order; c = the entries that are not beyond the threshold
    int n_valid = 0, close = 0;
    for (int start = 0; start < n; start += CP_THREADS) {
        const int i = start + tid;
        const float z = i < n ? depth[b0 + i] : -1.0f;
        const bool valid = z > 0;
        int tot;
        const int pos = block_rank<CP_WAVES>(valid, s_wave, &tot);
        if (valid) {
            s_key[n_valid + pos] = P.mode == RGBD_CLOSE_ALL ? (unsigned long long)(uint32_t)i : rgbd_sort_key(z, i);
            close += !(z > P.th);
        }
        n_valid += tot;
    }
    if (close) atomicAdd(&s_close, close);
    int n_walked = n_valid;
    if (P.mode != RGBD_CLOSE_ALL) {
        int pow2 = 1;
        while (pow2 < n_valid) pow2 <<= 1;
        for (int t = n_valid + tid; t < pow2; t += CP_THREADS) s_key[t] = ~0ull;
        __syncthreads();
        for (int k = 2; k <= pow2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (pow2 >> 1); t += CP_THREADS) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j; // bit j of lo is clear
                    const unsigned long long a = s_key[lo], b = s_key[hi];
                    if ((a > b) == ((lo & k) == 0)) { s_key[lo] = b; s_key[hi] = a; }
                }
                __syncthreads();
            }
        }
        n_walked = rgbd_walked(n_valid, s_close);
    } else {
        __syncthreads();
    }
    for (int t = tid; t < n_valid; t += CP_THREADS) order[b0 + t] = (int)(uint32_t)s_key[t];
    // the created points of the walked prefix, in the order of the walk
    int n_new = 0;
    for (int start = 0; start < n_walked; start += CP_THREADS) {
        const int t = start + tid;
        const int i = t < n_walked ? (int)(uint32_t)s_key[t] : 0;
        const bool create = t < n_walked && (P.mode == RGBD_CLOSE_ALL || need_new[b0 + i] != 0);
        int tot;
        const int pos = n_new + block_rank<CP_WAVES>(create, s_wave, &tot);
        if (create) {
            const cs_keypoint ku = keysUn[b0 + i];
            float x3D[3];
            rgbd_unproject(ku.x, ku.y, depth[b0 + i], P.cx, P.cy, P.invfx, P.invfy, s_Rwc, s_Ow, x3D);
            new_idx[b0 + pos] = i;
            float *o = new_x3D + 3 * (size_t)(b0 + pos);
            o[0] = x3D[0]; o[1] = x3D[1]; o[2] = x3D[2];
        }
        n_new += tot;
    }
    if (tid == 0) { counts[3 * f] = n_valid; counts[3 * f + 1] = n_walked; counts[3 * f + 2] = n_new; }
}

// The launch and the hand-back of the close-point pass over device arrays: d_first (n_frames + 1), d_depth, d_keysUn hold `total` key points.
int close_points_device(cs_ctx *ctx, int n_frames, const int *first, const int *d_first, const float *d_depth, const cs_keypoint *d_keysUn, const uint8_t *need_new,
                        const float *Tcw, const float *K4, float th_depth, int mode, int *n_valid, int *order, int *n_walked, int *new_first, int *new_idx, float *new_x3D) {
    const size_t total = (size_t)first[n_frames];
    cs_scratch sc(ctx);
    uint8_t *d_need = nullptr;
    float *d_Tcw = nullptr, *d_x3D = nullptr;
    int *d_order = nullptr, *d_new = nullptr, *d_counts = nullptr;
    if (mode != CS_CLOSE_POINTS_ALL) CS_TRY(sc.upload(ctx, &d_need, need_new, total));
    CS_TRY(sc.upload(ctx, &d_Tcw, Tcw, (size_t)n_frames * 12));
    CS_TRY(sc.alloc(ctx, &d_order, total));
    CS_TRY(sc.alloc(ctx, &d_new, total));
    CS_TRY(sc.alloc(ctx, &d_x3D, total * 3));
    CS_TRY(sc.alloc(ctx, &d_counts, (size_t)n_frames * 3));
    CloseP P{K4[2], K4[3], 1.0f / K4[0], 1.0f / K4[1], th_depth, mode};
    CS_LAUNCH(ctx, "rgbd_close_points", rgbd_close_points, dim3(n_frames), dim3(CP_THREADS), 0, P, d_first, d_depth, d_keysUn, d_need, d_Tcw, d_order, d_new, d_x3D, d_counts);
    CS_HIP(ctx, hipGetLastError());
    std::vector<int> counts((size_t)n_frames * 3), h_new(total);
    std::vector<float> h_x3D(total * 3);
    CS_TRY(cs_d2h(ctx, counts.data(), d_counts, counts.size()));
    CS_TRY(cs_d2h(ctx, order, d_order, total));
    CS_TRY(cs_d2h(ctx, h_new.data(), d_new, total));
    CS_TRY(cs_d2h(ctx, h_x3D.data(), d_x3D, total * 3));
    CS_TRY(sc.drain());
    new_first[0] = 0;
    for (int f = 0; f < n_frames; f++) { // the created points of the frames one behind the other; order keeps the frames' own slots
        const int nn = counts[3 * (size_t)f + 2], to = new_first[f];
        n_valid[f] = counts[3 * (size_t)f]; n_walked[f] = counts[3 * (size_t)f + 1];
        std::copy(h_new.begin() + first[f], h_new.begin() + first[f] + nn, new_idx + to);
        std::copy(h_x3D.begin() + 3 * (size_t)first[f], h_x3D.begin() + 3 * ((size_t)first[f] + nn), new_x3D + 3 * (size_t)to);
        new_first[f + 1] = to + nn;
    }
    return CS_OK;
}

// nullptr, or what is wrong with the frames of a close-point call
const char *close_points_check(int n_frames, const int *first, const void *depth, const void *keysUn, const void *need_new, const float *Tcw, const float *K4, int mode,
                               bool outputs, int *status) {
    *status = CS_ERR_BAD_ARG;
    if (n_frames < 1 || !first || !Tcw || !K4 || !outputs) return "a null argument or no frame";
    if (mode != CS_CLOSE_POINTS_NEAREST && mode != CS_CLOSE_POINTS_ALL) return "mode is neither CS_CLOSE_POINTS_NEAREST nor CS_CLOSE_POINTS_ALL";
    if (first[0] != 0) return "first[0] is not 0";
    for (int f = 0; f < n_frames; f++) {
        if (first[f + 1] < first[f]) return "first decreases";
        if (first[f + 1] - first[f] > CS_RGBD_MAX_KEYPOINTS) { *status = CS_ERR_CAPACITY; return "a frame has more than CS_RGBD_MAX_KEYPOINTS key points"; }
    }
    if (first[n_frames] > 0 && (!depth || !keysUn || (mode == CS_CLOSE_POINTS_NEAREST && !need_new))) return "key points without depth, keysUn or need_new";
    return nullptr;
}
} // namespace

struct cs_rgbd {
    int W = 0, H = 0, cap = 0, max_frames = 0;
    cs_owner own;
    // device
    uint8_t *d_image = nullptr; // max_frames raw images, rows of W * 4 bytes reserved (U16 uses half of each)
    cs_keypoint *d_keys = nullptr, *d_keys_un = nullptr; // d_keys: mvKeys of cs_rgbd_from_keys (cs_rgbd_from_orb reads the extractor's)
    float *d_u_right = nullptr, *d_depth = nullptr;
    int *d_first = nullptr, *d_counts = nullptr; // n_with_depth[max_frames], n_outside[max_frames]
    // host: the depth batch and the last cs_rgbd_from_*
    int type = -1, n_images = 0, n_frames = 0;
    std::vector<int> first;
    long pitch() const { return (long)W * (type == CS_DEPTH_U16 ? 2 : 4); }
};

namespace {
int gather(cs_ctx *ctx, cs_rgbd *h, const cs_keypoint *d_keys, int have_un, const UndP &U, float bf, float factor) {
    const int total = h->first[(size_t)h->n_frames];
    CS_TRY(cs_h2d(ctx, h->d_first, h->first.data(), (size_t)h->n_frames + 1));
    CS_HIP(ctx, hipMemsetAsync(h->d_counts, 0, sizeof(int) * 2 * (size_t)h->max_frames, ctx->stream));
    if (total > 0) {
        GatherP P{};
        P.U = U; P.W = h->W; P.H = h->H; P.type = h->type; P.n_frames = h->n_frames; P.total = total;
        P.pitch = h->pitch(); P.frame_bytes = P.pitch * h->H; P.bf = bf; P.factor = factor;
        CS_LAUNCH(ctx, "rgbd_gather", rgbd_gather, dim3((total + 255) / 256), dim3(256), 0, P, h->d_first, d_keys, have_un, h->d_image, h->d_keys_un, h->d_u_right, h->d_depth,
                  h->d_counts, h->d_counts + h->max_frames);
    }
    CS_HIP(ctx, hipGetLastError());
    return CS_OK;
}
int set_type(cs_ctx *ctx, cs_rgbd *h, int type, int n_frames, const void *p) {
    if (!ctx || !h || !p || (type != CS_DEPTH_U16 && type != CS_DEPTH_F32) || n_frames < 1 || n_frames > h->max_frames) return CS_ERR_BAD_ARG;
    return CS_OK;
}
} // namespace

extern "C" {

void cs_rgbd_destroy(cs_ctx *ctx, cs_rgbd *h) {
    if (!h) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    h->own.free_all(ctx);
    delete h;
}

int cs_rgbd_create(cs_ctx *ctx, int width, int height, int max_keypoints_per_frame, int max_frames, cs_rgbd **out) {
    if (!ctx || !out || width < 1 || height < 1 || max_keypoints_per_frame < 1 || max_frames < 1 || (long)max_keypoints_per_frame * max_frames > INT_MAX) return CS_ERR_BAD_ARG;
    *out = nullptr;
    if (max_keypoints_per_frame > CS_RGBD_MAX_KEYPOINTS) { ctx->err = "cs_rgbd_create: max_keypoints_per_frame above CS_RGBD_MAX_KEYPOINTS"; return CS_ERR_BAD_ARG; }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_rgbd *h = new (std::nothrow) cs_rgbd();
    if (!h) return CS_ERR_NOMEM;
    h->W = width; h->H = height; h->cap = max_keypoints_per_frame; h->max_frames = max_frames;
    const size_t n = (size_t)max_keypoints_per_frame * max_frames;
    cs_owner &o = h->own;
    if (o.alloc(ctx, &h->d_image, (size_t)width * height * 4 * max_frames) != CS_OK || o.alloc(ctx, &h->d_keys_un, n) != CS_OK ||
        o.alloc(ctx, &h->d_keys, n) != CS_OK || o.alloc(ctx, &h->d_u_right, n) != CS_OK || o.alloc(ctx, &h->d_depth, n) != CS_OK ||
        o.alloc(ctx, &h->d_first, (size_t)max_frames + 1) != CS_OK || o.alloc(ctx, &h->d_counts, (size_t)max_frames * 2) != CS_OK) {
        (void)hipGetLastError();
        ctx->err = "cs_rgbd_create: out of device memory";
        cs_rgbd_destroy(ctx, h);
        return CS_ERR_NOMEM;
    }
    *out = h;
    return CS_OK;
}

int cs_rgbd_upload_depth(cs_ctx *ctx, cs_rgbd *h, const void *depth, int type, int n_frames, long stride_bytes) {
    CS_TRY(set_type(ctx, h, type, n_frames, depth));
    const long row = (long)h->W * (type == CS_DEPTH_U16 ? 2 : 4);
    if (stride_bytes < row) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    CS_HIP(ctx, hipMemcpy2DAsync(h->d_image, (size_t)row, depth, (size_t)stride_bytes, (size_t)row, (size_t)h->H * n_frames, hipMemcpyHostToDevice, ctx->stream));
    h->type = type; h->n_images = n_frames;
    return CS_OK;
}

int cs_rgbd_set_depth_device(cs_ctx *ctx, cs_rgbd *h, const void *d_depth, int type, int n_frames) {
    CS_TRY(set_type(ctx, h, type, n_frames, d_depth));
    const size_t row = (size_t)h->W * (type == CS_DEPTH_U16 ? 2 : 4);
    CS_HIP(ctx, hipSetDevice(ctx->device));
    CS_HIP(ctx, hipMemcpyAsync(h->d_image, d_depth, row * h->H * n_frames, hipMemcpyDeviceToDevice, ctx->stream));
    h->type = type; h->n_images = n_frames;
    return CS_OK;
}

int cs_rgbd_from_orb(cs_ctx *ctx, cs_rgbd *h, const cs_orb *orb, int first_frame, int n_frames, const float *K4, const float *dist5, float bf, float depth_map_factor) {
    if (!ctx || !h || !orb || !K4 || first_frame < 0 || n_frames < 1 || !(bf > 0.0f)) return CS_ERR_BAD_ARG;
    if (n_frames > h->max_frames || n_frames > h->n_images) { ctx->err = "cs_rgbd_from_orb: more frames than the handle holds depth images for"; return CS_ERR_BAD_ARG; }
    cs_orb_pyramid_view V;
    if (cs_orb_device_pyramid(orb, &V) != CS_OK) return CS_ERR_BAD_ARG;
    if (first_frame + n_frames > V.n_frames) { ctx->err = "cs_rgbd_from_orb: frames outside the extractor's last run"; return CS_ERR_BAD_ARG; }
    if (V.W != h->W || V.H != h->H) { ctx->err = "cs_rgbd_from_orb: the extractor's image size differs from the depth images'"; return CS_ERR_BAD_ARG; }
    std::vector<int> first((size_t)n_frames + 1, 0); // the handle keeps its last call until this one is known to be good
    const cs_keypoint *k0 = nullptr, *k = nullptr;
    const unsigned long long *d = nullptr;
    for (int f = 0; f < n_frames; f++) {
        int n = 0;
        if (cs_orb_device_frame(orb, first_frame + f, &k, &d, &n) != CS_OK) return CS_ERR_BAD_ARG; // no run yet
        if (f == 0) k0 = k;
        if (n > h->cap) { ctx->err = "cs_rgbd_from_orb: a frame has more key points than the handle was created for"; return CS_ERR_CAPACITY; }
        if ((int)(k - k0) != first[(size_t)f]) { ctx->err = "cs_rgbd_from_orb: the extractor's frames are not one behind the other"; return CS_ERR_BAD_ARG; }
        first[(size_t)f + 1] = first[(size_t)f] + n;
    }
    h->first.swap(first); h->n_frames = n_frames;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    return gather(ctx, h, k0, 0, make_undp(K4, dist5), bf, depth_map_factor);
}

int cs_rgbd_from_keys(cs_ctx *ctx, cs_rgbd *h, int n_frames, const int *first, const cs_keypoint *keys, const cs_keypoint *keysUn, float bf, float depth_map_factor) {
    if (!ctx || !h || !first || n_frames < 1 || !(bf > 0.0f) || first[0] != 0) return CS_ERR_BAD_ARG;
    if (n_frames > h->max_frames || n_frames > h->n_images) { ctx->err = "cs_rgbd_from_keys: more frames than the handle holds depth images for"; return CS_ERR_BAD_ARG; }
    for (int f = 0; f < n_frames; f++) {
        if (first[f + 1] < first[f]) return CS_ERR_BAD_ARG;
        if (first[f + 1] - first[f] > h->cap) { ctx->err = "cs_rgbd_from_keys: a frame has more key points than the handle was created for"; return CS_ERR_CAPACITY; }
    }
    if (first[n_frames] > 0 && (!keys || !keysUn)) return CS_ERR_BAD_ARG;
    h->first.assign(first, first + n_frames + 1); h->n_frames = n_frames;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    CS_TRY(cs_h2d(ctx, h->d_keys, keys, (size_t)first[n_frames]));
    CS_TRY(cs_h2d(ctx, h->d_keys_un, keysUn, (size_t)first[n_frames]));
    UndP U{}; U.identity = 1;
    CS_TRY(gather(ctx, h, h->d_keys, 1, U, bf, depth_map_factor));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the caller's arrays are free when the call returns
    return CS_OK;
}

int cs_rgbd_read(cs_ctx *ctx, cs_rgbd *h, float *u_right, float *depth, int cap_per_frame, int *counts, int *n_with_depth, int *n_outside) {
    if (!ctx || !h || !u_right || !depth || !counts || !n_with_depth || cap_per_frame < 1 || h->n_frames < 1) return CS_ERR_BAD_ARG;
    for (int f = 0; f < h->n_frames; f++)
        if (h->first[(size_t)f + 1] - h->first[(size_t)f] > cap_per_frame) return CS_ERR_CAPACITY;
    for (int f = 0; f < h->n_frames; f++) {
        const int b0 = h->first[(size_t)f], n = h->first[(size_t)f + 1] - b0;
        counts[f] = n;
        CS_TRY(cs_d2h(ctx, u_right + (size_t)f * cap_per_frame, h->d_u_right + b0, (size_t)n));
        CS_TRY(cs_d2h(ctx, depth + (size_t)f * cap_per_frame, h->d_depth + b0, (size_t)n));
    }
    CS_TRY(cs_d2h(ctx, n_with_depth, h->d_counts, (size_t)h->n_frames));
    if (n_outside) CS_TRY(cs_d2h(ctx, n_outside, h->d_counts + h->max_frames, (size_t)h->n_frames));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_rgbd_read_packed(cs_ctx *ctx, cs_rgbd *h, float *u_right, float *depth, long cap_total, int *first, long *total, int *n_with_depth, int *n_outside) {
    if (!ctx || !h || !first || !total || h->n_frames < 1) return CS_ERR_BAD_ARG;
    const long n = h->first[(size_t)h->n_frames];
    *total = n;
    for (int f = 0; f <= h->n_frames; f++) first[f] = h->first[(size_t)f];
    if (!u_right || !depth) return CS_OK; // size query
    if (n > cap_total) return CS_ERR_CAPACITY;
    CS_TRY(cs_d2h(ctx, u_right, h->d_u_right, (size_t)n));
    CS_TRY(cs_d2h(ctx, depth, h->d_depth, (size_t)n));
    if (n_with_depth) CS_TRY(cs_d2h(ctx, n_with_depth, h->d_counts, (size_t)h->n_frames));
    if (n_outside) CS_TRY(cs_d2h(ctx, n_outside, h->d_counts + h->max_frames, (size_t)h->n_frames));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_rgbd_read_keys_un(cs_ctx *ctx, cs_rgbd *h, cs_keypoint *keysUn, long cap_total) {
    if (!ctx || !h || !keysUn || h->n_frames < 1) return CS_ERR_BAD_ARG;
    const long n = h->first[(size_t)h->n_frames];
    if (n > cap_total) return CS_ERR_CAPACITY;
    CS_TRY(cs_d2h(ctx, keysUn, h->d_keys_un, (size_t)n));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_rgbd_device_frame(const cs_rgbd *h, int frame, const float **d_u_right, const float **d_depth, const cs_keypoint **d_keysUn, int *n) {
    if (!h || !d_u_right || !d_depth || !n || frame < 0 || frame >= h->n_frames) return CS_ERR_BAD_ARG;
    const int b0 = h->first[(size_t)frame];
    *d_u_right = h->d_u_right + b0; *d_depth = h->d_depth + b0; *n = h->first[(size_t)frame + 1] - b0;
    if (d_keysUn) *d_keysUn = h->d_keys_un + b0;
    return CS_OK;
}

int cs_rgbd_host_from_keys(const void *depth, int type, int width, int height, long stride_bytes, int n, const cs_keypoint *keys, const cs_keypoint *keysUn, float bf,
                           float depth_map_factor, float *u_right, float *depth_out, int *n_with_depth, int *n_outside) {
    if (!depth || (type != CS_DEPTH_U16 && type != CS_DEPTH_F32) || width < 1 || height < 1 || stride_bytes < (long)width * (type == CS_DEPTH_U16 ? 2 : 4) || n < 0 ||
        (n > 0 && (!keys || !keysUn || !u_right || !depth_out)) || !n_with_depth || !n_outside || !(bf > 0.0f))
        return CS_ERR_BAD_ARG;
    static_assert(sizeof(cs_keypoint) == 7 * sizeof(float), "pt is the first two floats of a 28-byte record");
    rgbd_frame_host(depth, type, width, height, stride_bytes, n, &keys->x, &keysUn->x, 7, bf, depth_map_factor, u_right, depth_out, n_with_depth, n_outside);
    return CS_OK;
}

int cs_close_points(cs_ctx *ctx, int n_frames, const int *first, const float *depth, const cs_keypoint *keysUn, const uint8_t *need_new, const float *Tcw, const float *K4,
                    float th_depth, int mode, int *n_valid, int *order, int *n_walked, int *new_first, int *new_idx, float *new_x3D) {
    int status = CS_OK;
    if (const char *what = close_points_check(n_frames, first, depth, keysUn, need_new, Tcw, K4, mode, n_valid && order && n_walked && new_first && new_idx && new_x3D, &status)) {
        if (ctx) ctx->err = std::string("cs_close_points: ") + what;
        return status;
    }
    if (!ctx) { // the same statement on the host
        new_first[0] = 0;
        for (int f = 0; f < n_frames; f++) {
            const int b0 = first[f], to = new_first[f];
            int nn = 0;
            rgbd_close_points_host(first[f + 1] - b0, depth + b0, keysUn ? &keysUn[b0].x : nullptr, 7, need_new ? need_new + b0 : nullptr, Tcw + 12 * (size_t)f, K4, th_depth, mode,
                                   n_valid + f, order + b0, n_walked + f, &nn, new_idx + to, new_x3D + 3 * (size_t)to);
            new_first[f + 1] = to + nn;
        }
        return CS_OK;
    }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t total = (size_t)first[n_frames];
    cs_scratch sc(ctx);
    int *d_first = nullptr;
    float *d_depth = nullptr;
    cs_keypoint *d_keysUn = nullptr;
    CS_TRY(sc.upload(ctx, &d_first, first, (size_t)n_frames + 1));
    CS_TRY(sc.upload(ctx, &d_depth, depth, total));
    CS_TRY(sc.upload(ctx, &d_keysUn, keysUn, total));
    return close_points_device(ctx, n_frames, first, d_first, d_depth, d_keysUn, need_new, Tcw, K4, th_depth, mode, n_valid, order, n_walked, new_first, new_idx, new_x3D);
}

int cs_rgbd_close_points(cs_ctx *ctx, cs_rgbd *h, const uint8_t *need_new, const float *Tcw, const float *K4, float th_depth, int mode, int *n_valid, int *order,
                         int *n_walked, int *new_first, int *new_idx, float *new_x3D) {
    if (!ctx || !h || h->n_frames < 1) return CS_ERR_BAD_ARG;
    int status = CS_OK;
    if (const char *what = close_points_check(h->n_frames, h->first.data(), h->d_depth, h->d_keys_un, need_new, Tcw, K4, mode,
                                              n_valid && order && n_walked && new_first && new_idx && new_x3D, &status)) {
        ctx->err = std::string("cs_rgbd_close_points: ") + what;
        return status;
    }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    return close_points_device(ctx, h->n_frames, h->first.data(), h->d_first, h->d_depth, h->d_keys_un, need_new, Tcw, K4, th_depth, mode, n_valid, order, n_walked, new_first,
                               new_idx, new_x3D);
}

} // extern "C"
