// localmap.hip -- the middle of the local-mapping thread's key-frame cycle on the device: the triangulation loop of LocalMapping::CreateNewMapPoints
// (LocalMapping.cc:319-570) and MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (MapPoint.cc:381-446, :469-510) for many points in one call.
//
//   lm_triangulate   one thread per matched pair of all neighbours: triangulate_pair (triangulate_math.h, :410-549) -> x3D, status
//   lm_claim         one thread per key point idx1 of the current key frame: the first neighbour in order whose pair was accepted creates the point, the later
//                    pairs of idx1 become TRI_CLAIMED (the reference's search would have skipped idx1 from there on, ORBmatcher.cc:721-725)
//   mp_distinctive   one wave per map point: lane i holds row i of the distance matrix (N <= 64: in LDS, each lane its own column of the transposed tile; above: row blocks of
//                    64 that recompute the distances), finds the row's k-th smallest by counting (distances lie in 0..256: a bisection over the value), then the first
//                    row with the smallest such value wins
//   mp_normal_depth  one thread per map point: mappoint_normal_depth (triangulate_math.h)
//
// The entry points take host pointers, check every index on the host before anything is launched, and wait once.
#include "common.h"
#include "triangulate_math.h"

struct LmFrameD { TriCam cam; int key_base, lvl_base; };
struct LmKey { float ux, uy, kx, ky, ur, depth; int octave; };
struct LmPair { int neigh, idx1, idx2; };

__global__ void __launch_bounds__(256) lm_triangulate(int n_pairs, const LmPair *pairs, const LmFrameD *frames, const LmKey *keys, const float2 *levels /* sigma2, scale */,
                                                     float ratioFactor, float *x3D, uint8_t *status) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    const LmPair pr = pairs[p];
    const LmFrameD &F1 = frames[0], &F2 = frames[1 + pr.neigh];
    const LmKey k1 = keys[F1.key_base + pr.idx1], k2 = keys[F2.key_base + pr.idx2];
    const float2 l1 = levels[F1.lvl_base + k1.octave], l2 = levels[F2.lvl_base + k2.octave];
    const TriObs o1 = {k1.ux, k1.uy, k1.kx, k1.ky, k1.ur, k1.depth, l1.x, l1.y}, o2 = {k2.ux, k2.uy, k2.kx, k2.ky, k2.ur, k2.depth, l2.x, l2.y};
    float x[3];
    status[p] = (uint8_t)triangulate_pair(F1.cam, o1, F2.cam, o2, ratioFactor, x);
    x3D[3 * (size_t)p] = x[0]; x3D[3 * (size_t)p + 1] = x[1]; x3D[3 * (size_t)p + 2] = x[2];
}

__global__ void __launch_bounds__(256) lm_claim(int N1, int n_neigh, const int *pair_of /* n_neigh x N1: pair of (neighbour, idx1) or -1 */, uint8_t *status, int *new_pair_of_idx1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N1) return;
    int winner = -1;
    for (int n = 0; n < n_neigh; n++) {
        const int p = pair_of[(size_t)n * N1 + i];
        if (p < 0) continue;
        if (winner >= 0) status[p] = TRI_CLAIMED;
        else if (status[p] == TRI_CREATED) winner = p;
    }
    new_pair_of_idx1[i] = winner;
}

// ---- ComputeDistinctiveDescriptors
// the smallest value v of 0..256 with at least `need` of the row's N distances <= v, i.e. sorted[need - 1]
template <class Count> __device__ __forceinline__ int kth_by_counting(int need, Count count_le) {
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (count_le(mid) >= need) hi = mid; else lo = mid + 1;
    }
    return lo;
}
constexpr int MP_WAVES = 4; // points per 256-thread workgroup
__global__ void __launch_bounds__(256) mp_distinctive(int n_points, const int *obs_off, const unsigned long long *desc, int *best) {
    __shared__ unsigned short s_d[MP_WAVES][64 * 64]; // [j * 64 + lane]: lane i reads and writes its own column only, so the waves need no barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pt = blockIdx.x * MP_WAVES + wave;
    if (pt >= n_points) return;
    const int o0 = obs_off[pt], N = obs_off[pt + 1] - o0;
    if (N <= 0) { if (lane == 0) best[pt] = -1; return; }
    const unsigned long long *D = desc + 4 * (size_t)o0;
    const int need = (int)(0.5 * (N - 1)) + 1;
    int key = 0x7fffffff; // (median << 20) | row: the minimum is the first row with the smallest median
    if (N <= 64) {
        if (lane < N) {
            const unsigned long long a[4] = {D[4 * lane], D[4 * lane + 1], D[4 * lane + 2], D[4 * lane + 3]};
            unsigned short *col = &s_d[wave][lane];
            for (int j = 0; j < N; j++) col[j * 64] = (unsigned short)hamming256(a, D[4 * j], D[4 * j + 1], D[4 * j + 2], D[4 * j + 3]);
            const int med = kth_by_counting(need, [&](int v) { int c = 0; for (int j = 0; j < N; j++) c += col[j * 64] <= v; return c; });
            key = (med << 20) | lane;
        }
    } else {
        for (int row = lane; row < N; row += 64) { // (N < 2^20 rows: checked by the entry point)
            const unsigned long long a[4] = {D[4 * (size_t)row], D[4 * (size_t)row + 1], D[4 * (size_t)row + 2], D[4 * (size_t)row + 3]};
            const int med = kth_by_counting(need, [&](int v) {
                int c = 0;
                for (int j = 0; j < N; j++) c += hamming256(a, D[4 * (size_t)j], D[4 * (size_t)j + 1], D[4 * (size_t)j + 2], D[4 * (size_t)j + 3]) <= v;
                return c;
            });
            key = min(key, (med << 20) | row);
        }
    }
    for (int off = 32; off > 0; off >>= 1) key = min(key, __shfl_xor(key, off));
    if (lane == 0) best[pt] = key & 0xfffff;
}

// ---- UpdateNormalAndDepth
__global__ void __launch_bounds__(256) mp_normal_depth(int n_points, const float *world_pos, const int *obs_off, const int *obs_kf, const float *kf_Ow, const int *ref_kf,
                                                      const int *ref_octave, const float *scale_factors, int n_levels, float *normal, float *min_distance, float *max_distance,
                                                      uint8_t *updated) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const int o0 = obs_off[i], n = obs_off[i + 1] - o0;
    updated[i] = n > 0;
    if (n <= 0) return;
    const float pos[3] = {world_pos[3 * (size_t)i], world_pos[3 * (size_t)i + 1], world_pos[3 * (size_t)i + 2]};
    float nv[3], mind, maxd;
    mappoint_normal_depth(pos, obs_kf + o0, n, kf_Ow, ref_kf[i], scale_factors[ref_octave[i]], scale_factors[n_levels - 1], nv, &mind, &maxd);
    normal[3 * (size_t)i] = nv[0]; normal[3 * (size_t)i + 1] = nv[1]; normal[3 * (size_t)i + 2] = nv[2];
    min_distance[i] = mind; max_distance[i] = maxd;
}

static int lm_bad(cs_ctx *ctx, const char *fn, const char *what, long a = -1, long b = -1) {
    char buf[256];
    if (a >= 0 && b >= 0) snprintf(buf, sizeof buf, "%s: %s (%ld, %ld)", fn, what, a, b);
    else if (a >= 0) snprintf(buf, sizeof buf, "%s: %s (%ld)", fn, what, a);
    else snprintf(buf, sizeof buf, "%s: %s", fn, what);
    ctx->err = buf;
    return CS_ERR_BAD_ARG;
}
static bool lm_frame_ok(const cs_lm_frame &f) {
    return f.N >= 0 && f.n_levels >= 1 && f.scale_factors && f.level_sigma2 && (f.N == 0 || (f.keysUn && f.keys_xy && f.u_right && f.depth));
}

extern "C" {

int cs_create_new_map_points(cs_ctx *ctx, const cs_lm_frame *kf, const cs_lm_frame *neighbours, int n_neigh, const int *matches12, int pair_cap, int *pair_off, int *pair_idx1,
                             int *pair_idx2, float *x3D, uint8_t *status, int *new_pair_of_idx1, int *nnew) {
    static const char *fn = "cs_create_new_map_points";
    if (!ctx) return CS_ERR_BAD_ARG;
    if (!kf || !pair_off || !nnew || pair_cap < 0 || (pair_cap && (!pair_idx1 || !pair_idx2 || !x3D || !status))) return lm_bad(ctx, fn, "NULL argument");
    if (n_neigh < 0 || n_neigh > CS_LM_MAX_NEIGHBOURS) return lm_bad(ctx, fn, "n_neigh outside 0..32", n_neigh);
    if (!lm_frame_ok(*kf)) return lm_bad(ctx, fn, "the current key frame has a NULL array, N < 0 or n_levels < 1");
    const int N1 = kf->N;
    if (n_neigh && (!neighbours || (N1 && !matches12))) return lm_bad(ctx, fn, "NULL argument");
    if (N1 && !new_pair_of_idx1) return lm_bad(ctx, fn, "NULL argument");
    for (int n = 0; n < n_neigh; n++) if (!lm_frame_ok(neighbours[n])) return lm_bad(ctx, fn, "a neighbour has a NULL array, N < 0 or n_levels < 1", n);
    // every index a kernel will use: the pairs' key points and the octaves of every key point a pair names
    std::vector<LmPair> pairs;
    std::vector<int> off((size_t)n_neigh + 1, 0), pair_of((size_t)n_neigh * N1, -1);
    for (int n = 0; n < n_neigh; n++) {
        const cs_lm_frame &f2 = neighbours[n];
        for (int i = 0; i < N1; i++) {
            const int j = matches12[(size_t)n * N1 + i];
            if (j == -1) continue;
            if (j < 0 || j >= f2.N) return lm_bad(ctx, fn, "a matches12 entry is outside -1..N2 - 1 (neighbour, idx1)", n, i);
            if (kf->keysUn[i].octave < 0 || kf->keysUn[i].octave >= kf->n_levels) return lm_bad(ctx, fn, "octave of a key point of the current key frame outside 0..n_levels - 1", i);
            if (f2.keysUn[j].octave < 0 || f2.keysUn[j].octave >= f2.n_levels) return lm_bad(ctx, fn, "octave of a key point of a neighbour outside 0..n_levels - 1 (neighbour, idx2)", n, j);
            pair_of[(size_t)n * N1 + i] = (int)pairs.size();
            pairs.push_back(LmPair{n, i, j});
        }
        off[n + 1] = (int)pairs.size();
    }
    const int P = (int)pairs.size();
    memcpy(pair_off, off.data(), sizeof(int) * off.size());
    if (P > pair_cap) { ctx->err = std::string(fn) + ": more pairs than pair_cap"; return CS_ERR_CAPACITY; }
    *nnew = 0;
    for (int i = 0; i < N1; i++) new_pair_of_idx1[i] = -1;
    for (int p = 0; p < P; p++) { pair_idx1[p] = pairs[p].idx1; pair_idx2[p] = pairs[p].idx2; }
    if (P == 0) return CS_OK;
    CS_HIP(ctx, hipSetDevice(ctx->device));

    // the frames as the kernels read them: one table of cameras, the key points and level tables of all frames behind each other
    std::vector<LmFrameD> frames((size_t)n_neigh + 1);
    std::vector<LmKey> keys;
    std::vector<float2> levels;
    for (int f = 0; f <= n_neigh; f++) {
        const cs_lm_frame &F = f ? neighbours[f - 1] : *kf;
        tri_make_cam(F.Rcw, F.tcw, F.Ow, F.fx, F.fy, F.cx, F.cy, F.invfx, F.invfy, F.mbf, F.mb, &frames[f].cam);
        frames[f].key_base = (int)keys.size(); frames[f].lvl_base = (int)levels.size();
        for (int i = 0; i < F.N; i++) keys.push_back(LmKey{F.keysUn[i].x, F.keysUn[i].y, F.keys_xy[2 * i], F.keys_xy[2 * i + 1], F.u_right[i], F.depth[i], F.keysUn[i].octave});
        for (int l = 0; l < F.n_levels; l++) levels.push_back(make_float2(F.level_sigma2[l], F.scale_factors[l]));
    }
    const float ratioFactor = 1.5f * kf->scale_factor;
    std::vector<int> h_new((size_t)N1);
    cs_scratch sc(ctx); // (after the host arrays: it waits for the copies out of and into them before they go)
    LmPair *d_pairs = nullptr; LmFrameD *d_frames = nullptr; LmKey *d_keys = nullptr; float2 *d_levels = nullptr; int *d_pair_of = nullptr, *d_new = nullptr; float *d_x = nullptr;
    uint8_t *d_st = nullptr;
    CS_TRY(sc.upload(ctx, &d_pairs, pairs.data(), pairs.size())); CS_TRY(sc.upload(ctx, &d_frames, frames.data(), frames.size()));
    CS_TRY(sc.upload(ctx, &d_keys, keys.data(), keys.size())); CS_TRY(sc.upload(ctx, &d_levels, levels.data(), levels.size()));
    CS_TRY(sc.upload(ctx, &d_pair_of, pair_of.data(), pair_of.size()));
    CS_TRY(sc.alloc(ctx, &d_new, (size_t)N1)); CS_TRY(sc.alloc(ctx, &d_x, 3 * (size_t)P)); CS_TRY(sc.alloc(ctx, &d_st, (size_t)P));
    CS_LAUNCH(ctx, "lm_triangulate", lm_triangulate, dim3((P + 255) / 256), dim3(256), 0, P, d_pairs, d_frames, d_keys, d_levels, ratioFactor, d_x, d_st);
    CS_LAUNCH(ctx, "lm_claim", lm_claim, dim3((N1 + 255) / 256), dim3(256), 0, N1, n_neigh, d_pair_of, d_st, d_new);
    CS_TRY(cs_d2h(ctx, x3D, d_x, 3 * (size_t)P)); CS_TRY(cs_d2h(ctx, status, d_st, (size_t)P)); CS_TRY(cs_d2h(ctx, h_new.data(), d_new, (size_t)N1));
    CS_TRY(sc.drain());
    int cnt = 0;
    for (int i = 0; i < N1; i++) { new_pair_of_idx1[i] = h_new[i]; cnt += h_new[i] >= 0; }
    *nnew = cnt;
    return CS_OK;
}

int cs_mappoint_distinctive_descriptors(cs_ctx *ctx, int n_points, const int *obs_off, const uint8_t *desc, int *best) {
    static const char *fn = "cs_mappoint_distinctive_descriptors";
    if (!ctx) return CS_ERR_BAD_ARG;
    if (n_points < 0 || (n_points && !best)) return lm_bad(ctx, fn, "NULL argument or n_points < 0");
    if (n_points == 0) return CS_OK;
    if (!cs_offsets_ok(obs_off, n_points, desc)) return lm_bad(ctx, fn, "obs_off does not start at 0, decreases, or desc is NULL");
    for (int p = 0; p < n_points; p++) if (obs_off[p + 1] - obs_off[p] >= (1 << 20)) return lm_bad(ctx, fn, "a point with 2^20 observations or more", p);
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    int *d_off = nullptr, *d_best = nullptr; unsigned long long *d_desc = nullptr;
    CS_TRY(sc.upload(ctx, &d_off, obs_off, (size_t)n_points + 1));
    CS_TRY(sc.alloc(ctx, &d_desc, 4 * (size_t)obs_off[n_points])); CS_TRY(cs_h2d(ctx, (uint8_t *)d_desc, desc, 32 * (size_t)obs_off[n_points]));
    CS_TRY(sc.alloc(ctx, &d_best, (size_t)n_points));
    CS_LAUNCH(ctx, "mp_distinctive", mp_distinctive, dim3((n_points + MP_WAVES - 1) / MP_WAVES), dim3(256), 0, n_points, d_off, d_desc, d_best);
    CS_TRY(cs_d2h(ctx, best, d_best, (size_t)n_points));
    return sc.drain();
}

int cs_mappoint_update_normal_and_depth(cs_ctx *ctx, int n_points, const float *world_pos, const int *obs_off, const int *obs_kf, int n_kf, const float *kf_Ow,
                                        const int *ref_kf, const int *ref_octave, const float *scale_factors, int n_levels, float *normal, float *min_distance,
                                        float *max_distance, uint8_t *updated) {
    static const char *fn = "cs_mappoint_update_normal_and_depth";
    if (!ctx) return CS_ERR_BAD_ARG;
    if (n_points < 0 || n_kf < 0 || n_levels < 1 || !scale_factors || (n_kf && !kf_Ow)) return lm_bad(ctx, fn, "NULL argument, a negative size or n_levels < 1");
    if (n_points == 0) return CS_OK;
    if (!world_pos || !ref_kf || !ref_octave || !normal || !min_distance || !max_distance || !updated) return lm_bad(ctx, fn, "NULL argument");
    if (!cs_offsets_ok(obs_off, n_points, obs_kf)) return lm_bad(ctx, fn, "obs_off does not start at 0, decreases, or obs_kf is NULL");
    for (int p = 0; p < n_points; p++) {
        if (obs_off[p + 1] == obs_off[p]) continue; // an empty run reads neither its key frame nor its octave
        for (int o = obs_off[p]; o < obs_off[p + 1]; o++) if (obs_kf[o] < 0 || obs_kf[o] >= n_kf) return lm_bad(ctx, fn, "an observation's key frame outside 0..n_kf - 1 (point, observation)", p, o);
        if (ref_kf[p] < 0 || ref_kf[p] >= n_kf) return lm_bad(ctx, fn, "a reference key frame outside 0..n_kf - 1", p);
        if (ref_octave[p] < 0 || ref_octave[p] >= n_levels) return lm_bad(ctx, fn, "a reference octave outside 0..n_levels - 1", p);
    }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    float *d_pos = nullptr, *d_Ow = nullptr, *d_sf = nullptr, *d_out = nullptr; int *d_off = nullptr, *d_obs = nullptr, *d_rk = nullptr, *d_ro = nullptr; uint8_t *d_up = nullptr;
    const size_t n = (size_t)n_points;
    CS_TRY(sc.upload(ctx, &d_pos, world_pos, 3 * n)); CS_TRY(sc.upload(ctx, &d_off, obs_off, n + 1)); CS_TRY(sc.upload(ctx, &d_obs, obs_kf, (size_t)obs_off[n_points]));
    CS_TRY(sc.upload(ctx, &d_Ow, kf_Ow, 3 * (size_t)n_kf)); CS_TRY(sc.upload(ctx, &d_rk, ref_kf, n)); CS_TRY(sc.upload(ctx, &d_ro, ref_octave, n));
    CS_TRY(sc.upload(ctx, &d_sf, scale_factors, (size_t)n_levels));
    CS_TRY(sc.alloc(ctx, &d_out, 5 * n)); CS_TRY(sc.alloc(ctx, &d_up, n));
    CS_LAUNCH(ctx, "mp_normal_depth", mp_normal_depth, dim3((n_points + 255) / 256), dim3(256), 0, n_points, d_pos, d_off, d_obs, d_Ow, d_rk, d_ro, d_sf, n_levels, d_out, d_out + 3 * n,
              d_out + 4 * n, d_up);
    std::vector<float> h_out(5 * n);
    CS_TRY(cs_d2h(ctx, h_out.data(), d_out, 5 * n)); CS_TRY(cs_d2h(ctx, updated, d_up, n));
    CS_TRY(sc.drain());
    for (size_t p = 0; p < n; p++) { // an empty run keeps the caller's values
        if (!updated[p]) continue;
        for (int k = 0; k < 3; k++) normal[3 * p + k] = h_out[3 * p + k];
        min_distance[p] = h_out[3 * n + p]; max_distance[p] = h_out[4 * n + p];
    }
    return CS_OK;
}

} // extern "C"
