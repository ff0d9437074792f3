// tracklocal.hip -- Tracking::UpdateLocalPoints and UpdateLocalKeyFrames (reference orb_object_slam/src/Tracking.cc:2740-2764, :2766-2874) on MI355X (gfx950).
//
// UpdateLocalPoints pushes, over the concatenated map-point lists of the local key frames, every point that is not bad (nor dynamic) at its FIRST occurrence
// (mnTrackReferenceForFrame marks it).  That order is the query order of the search that follows, whose claims depend on it.  On the device:
//   tracklocal_first   per entry: atomicMin of its position into first[point] -- a minimum is the same whatever order the atomics arrive in
//   tracklocal_count   per workgroup of TL_TILE entries: how many are the first occurrence of their point
//   tracklocal_bases   exclusive scan of the workgroup counts (one workgroup, TL_TILE counts per round, a carry between rounds) and the total
//   tracklocal_emit    the flags again, an exclusive scan inside the workgroup, and the store at base + rank: an order-preserving compaction
// The result is integers and fully determined.  UpdateLocalKeyFrames stays on the host (track_local_walk.h): a walk over at most a few hundred key frames.
#include "common.h"
#include "track_local_walk.h"

#include <climits>

namespace {
constexpr int TL_PER = 4, TL_TILE = 256 * TL_PER;
constexpr int TL_NONE = 0x7f7f7f7f; // what hipMemset(0x7f) leaves: above every position

__global__ void __launch_bounds__(256) tracklocal_first(int total, const int *kf_mp, int n_points, const uint8_t *skip, int *first, int *err) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int id = kf_mp[e];
    if (id < 0) return; // !pMP (:2751)
    if (id >= n_points) { *err = 1; return; }
    if (!skip[id]) atomicMin(&first[id], e);
}

// entry e is the first occurrence of a pushed point
__device__ __forceinline__ bool tl_is_first(int e, int total, const int *kf_mp, int n_points, const int *first) {
    if (e >= total) return false;
    const int id = kf_mp[e];
    return id >= 0 && id < n_points && first[id] == e;
}

__global__ void __launch_bounds__(256) tracklocal_count(int total, const int *kf_mp, int n_points, const int *first, int *tile_count) {
    __shared__ int s_w[4];
    const int e0 = blockIdx.x * TL_TILE + threadIdx.x * TL_PER; // (total < TL_NONE and the grid covers it: no overflow)
    int c = 0;
    for (int k = 0; k < TL_PER; k++) c += tl_is_first(e0 + k, total, kf_mp, n_points, first);
    int sum;
    block_excl_scan<4>(c, s_w, &sum);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(256) tracklocal_bases(int n_tiles, const int *tile_count, int *tile_base, int *n_out) {
    __shared__ int s_w[4];
    int carry = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += TL_TILE) {
        const int t = t0 + threadIdx.x * TL_PER;
        int c[TL_PER], mine = 0;
        for (int k = 0; k < TL_PER; k++) { c[k] = t + k < n_tiles ? tile_count[t + k] : 0; mine += c[k]; }
        int sum;
        int run = carry + block_excl_scan<4>(mine, s_w, &sum);
        for (int k = 0; k < TL_PER; k++) { if (t + k < n_tiles) tile_base[t + k] = run; run += c[k]; }
        carry += sum;
    }
    if (threadIdx.x == 0) *n_out = carry;
}

__global__ void __launch_bounds__(256) tracklocal_emit(int total, const int *kf_mp, int n_points, const int *first, const int *tile_base, int *out) {
    __shared__ int s_w[4];
    const int e0 = blockIdx.x * TL_TILE + threadIdx.x * TL_PER;
    bool f[TL_PER];
    int c = 0;
    for (int k = 0; k < TL_PER; k++) { f[k] = tl_is_first(e0 + k, total, kf_mp, n_points, first); c += f[k]; }
    int sum;
    int o = tile_base[blockIdx.x] + block_excl_scan<4>(c, s_w, &sum); // (o + c <= the number of distinct pushed points <= the capacity of out)
    for (int k = 0; k < TL_PER; k++) if (f[k]) out[o++] = kf_mp[e0 + k];
}
} // namespace

extern "C" {

int cs_track_local_points(cs_ctx *ctx, int n_kf, const int *kf_off, const int *kf_mp, int n_points, const uint8_t *skip, int *local_points, int *n_local) {
    if (!ctx || n_kf < 0 || n_points < 0 || !n_local || !cs_offsets_ok(kf_off, n_kf, kf_mp) || (n_points && !skip)) return CS_ERR_BAD_ARG;
    *n_local = 0;
    const int total = kf_off[n_kf];
    if (total >= TL_NONE - TL_TILE) return CS_ERR_CAPACITY;
    if (total == 0 || n_points == 0) { // (an entry that is not -1 would be outside an empty table)
        for (int e = 0; e < total; e++) if (kf_mp[e] >= 0) return CS_ERR_BAD_ARG;
        return CS_OK;
    }
    if (!local_points) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const int n_tiles = (total + TL_TILE - 1) / TL_TILE, cap = std::min(total, n_points);
    std::vector<int> res((size_t)cap);
    int tail[2] = {0, 0}; // n_out, err
    cs_scratch sc(ctx); // (after the host arrays: it waits for the copies out of and into them before they go)
    int *d_mp = nullptr, *d_first = nullptr, *d_cnt = nullptr, *d_base = nullptr, *d_out = nullptr, *d_tail = nullptr; uint8_t *d_skip = nullptr;
    CS_TRY(sc.alloc(ctx, &d_mp, (size_t)total)); CS_TRY(sc.alloc(ctx, &d_first, (size_t)n_points)); CS_TRY(sc.alloc(ctx, &d_cnt, (size_t)n_tiles)); CS_TRY(sc.alloc(ctx, &d_base, (size_t)n_tiles));
    CS_TRY(sc.alloc(ctx, &d_out, (size_t)cap)); CS_TRY(sc.alloc(ctx, &d_tail, (size_t)2)); CS_TRY(sc.alloc(ctx, &d_skip, (size_t)n_points));
    CS_TRY(cs_h2d(ctx, d_mp, kf_mp, (size_t)total)); CS_TRY(cs_h2d(ctx, d_skip, skip, (size_t)n_points));
    CS_HIP(ctx, hipMemsetAsync(d_first, 0x7f, sizeof(int) * (size_t)n_points, ctx->stream));
    CS_HIP(ctx, hipMemsetAsync(d_tail, 0, 2 * sizeof(int), ctx->stream));
    CS_LAUNCH(ctx, "tracklocal_first", tracklocal_first, dim3((total + 255) / 256), dim3(256), 0, total, d_mp, n_points, d_skip, d_first, d_tail + 1);
    CS_LAUNCH(ctx, "tracklocal_count", tracklocal_count, dim3(n_tiles), dim3(256), 0, total, d_mp, n_points, d_first, d_cnt);
    CS_LAUNCH(ctx, "tracklocal_bases", tracklocal_bases, dim3(1), dim3(256), 0, n_tiles, d_cnt, d_base, d_tail);
    CS_LAUNCH(ctx, "tracklocal_emit", tracklocal_emit, dim3(n_tiles), dim3(256), 0, total, d_mp, n_points, d_first, d_base, d_out);
    CS_TRY(cs_d2h(ctx, tail, d_tail, 2));
    CS_TRY(cs_d2h(ctx, res.data(), d_out, (size_t)cap));
    CS_TRY(sc.drain());
    if (tail[1]) { ctx->err = "cs_track_local_points: a map-point index outside the point table"; return CS_ERR_BAD_ARG; }
    if (tail[0] < 0 || tail[0] > cap) { ctx->err = "cs_track_local_points: count out of range"; return CS_ERR_HIP; }
    memcpy(local_points, res.data(), sizeof(int) * (size_t)tail[0]);
    *n_local = tail[0];
    return CS_OK;
}

int cs_track_local_keyframes(int n_frame, const int *frame_mp, int n_points, const uint8_t *mp_skip, const int *obs_off, const int *obs_kf, int n_kf, const uint8_t *kf_bad,
                             const int *cov_off, const int *cov_kf, const int *child_off, const int *child_kf, const int *parent, int *local_kf, int *n_local, int *kf_max) {
    if (n_frame < 0 || n_points < 0 || n_kf < 0 || (n_frame && !frame_mp) || (n_points && !mp_skip) || !cs_offsets_ok(obs_off, n_points, obs_kf) || !cs_offsets_ok(cov_off, n_kf, cov_kf) ||
        !cs_offsets_ok(child_off, n_kf, child_kf) || (n_kf && (!kf_bad || !parent || !local_kf)) || !n_local || !kf_max)
        return CS_ERR_BAD_ARG;
    const int n = track_local_keyframes(n_frame, frame_mp, n_points, mp_skip, obs_off, obs_kf, n_kf, kf_bad, cov_off, cov_kf, child_off, child_kf, parent, local_kf, kf_max);
    if (n == -2) return CS_ERR_BAD_ARG;
    *n_local = n;
    return CS_OK;
}

} // extern "C"
