// object_points.hip -- point coordinates out of cuboids (include/cubeslam_hip/object_points.h): the dynamic-point triangulation of Tracking::CreateNewKeyFrame
// (Tracking.cc:2144-2244) and the object-depth initialisation (Tracking.cc:876-898, :2339-2424, LocalMapping.cc:574-652), many key frames per call.
//
//   dyn_triangulate   one thread per point, 256 per block: dyn_triangulate_point (object_points_math.h); cameras and cuboid rows through the point's pair index.  No LDS,
//                     no atomics.  The f64 Jacobi is the cost, as in lm_triangulate.
//   od_frame          one 256-thread workgroup per frame.  Tracking mode: the owner of a grid cell is the first qualifying index the sequential loop meets, i.e. the
//                     smallest one: atomicMin into a 64 x 48 table of ints in LDS (12 KB).  Candidates are compacted in index order (ballot + wave totals), the draws and
//                     the walk run in lane 0 over the frame's slice in global memory (at most `candidates` steps), the unprojection runs over all lanes.
//
// The entry points take host pointers, check every index on the host before anything is launched, and wait once.  ctx == NULL: the same header on the host.
#include "common.h"
#include "object_points_math.h"
#include "../../include/cubeslam_hip/object_points.h"

static_assert(CS_DYN_TRIANGULATED == DYN_TRIANGULATED && CS_DYN_NO_OBSERVATION == DYN_NO_OBSERVATION && CS_DYN_TRACKLET == DYN_TRACKLET && CS_DYN_W_ZERO == DYN_W_ZERO &&
              CS_DYN_TOO_FAR == DYN_TOO_FAR, "the header's status bytes are the math header's");
static_assert(sizeof(OdKey) == sizeof(cs_keypoint) && offsetof(OdKey, octave) == offsetof(cs_keypoint, octave), "OdKey is cs_keypoint");
static_assert(CS_OBJECT_DEPTH_FIRST_FRAME == OD_FIRST_FRAME && CS_OBJECT_DEPTH_TRACKING == OD_TRACKING && CS_OBJECT_DEPTH_LOCAL_MAPPING == OD_LOCAL_MAPPING, "modes");

__global__ void __launch_bounds__(256) dyn_triangulate(int n_points, const int *pair_of, const DynCam *cams, DynTables T, const float *kp1, const float *kp2, const int *obj_last,
                                                      const int *obj_now, const int *idx_last, const float *world_pos, uint8_t *status, float *x3D, float *pto, double *dp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const int f = pair_of[i];
    const size_t i2 = 2 * (size_t)i, i3 = 3 * (size_t)i;
    dyn_one(cams[f], f, T, kp1 + i2, kp2 + i2, obj_last[i], obj_now[i], idx_last[i], world_pos + i3, status + i, x3D + i3, pto + i3, dp + i3);
}

// ---- object depth
// the frame's key points that satisfy pred, in index order: emit(position, index) -> their number (every thread gets it).  256 threads.  What emit stored is
// readable by the whole workgroup behind the call.
template <class Pred, class Emit> __device__ __forceinline__ int od_compact(int N, int *s_wave, Pred pred, Emit emit) {
    int running = 0;
    for (int base = 0; base < N; base += 256) {
        const int i = base + threadIdx.x;
        const bool flag = i < N && pred(i);
        int total;
        const int rank = block_rank<4>(flag, s_wave, &total);
        if (flag) emit(running + rank, i);
        running += total;
    }
    __syncthreads();
    return running;
}

__global__ void __launch_bounds__(256) od_frame(int mode, const int *first, const cs_keypoint *keys_all, const uint8_t *has_mp_all, const int *object_id_all, const int *cub_first,
                                               const float *cuboid_depth, const float *K4, const float *bounds, const float *Twc, const int *draw_first, const int *draws,
                                               OdFrameOut *out, int *candidates_all, int *shuffled_all, int *new_idx_all, float *new_x3D_all) {
    __shared__ int s_cell[OD_NCELL];
    __shared__ int s_wave[4];
    __shared__ int s_raw, s_new;
    const int f = blockIdx.x, tid = threadIdx.x, b0 = first[f], N = first[f + 1] - b0;
    const cs_keypoint *keys = keys_all + b0;
    const uint8_t *has_mp = has_mp_all ? has_mp_all + b0 : nullptr;
    const int *object_id = object_id_all + b0;
    const float *cub_depth = cuboid_depth + cub_first[f];
    int *candidates = candidates_all + b0, *shuffled = shuffled_all + b0, *new_idx = new_idx_all + b0;
    float *new_x3D = new_x3D_all + 3 * (size_t)b0;
    OdGrid G = {0.f, 0.f, 0.f, 0.f};
    if (mode == OD_TRACKING) {
        G = od_make_grid(bounds + 4 * (size_t)f);
        for (int c = tid; c < OD_NCELL; c += 256) s_cell[c] = 0x7fffffff;
    }
    if (tid == 0) { s_raw = 0; s_new = 0; }
    __syncthreads();
    if (mode != OD_FIRST_FRAME) {
        int raw = 0;
        for (int i = tid; i < N; i += 256) {
            const int mp = has_mp[i];
            raw += mp != 0;
            if (mode == OD_TRACKING && od_qualifies(mode, mp, object_id[i], keys[i].octave)) {
                const int c = od_cell(G, keys[i].x, keys[i].y);
                if (c >= 0) atomicMin(&s_cell[c], i);
            }
        }
        for (int off = 32; off > 0; off >>= 1) raw += __shfl_xor(raw, off);
        if ((tid & 63) == 0) atomicAdd(&s_raw, raw);
        __syncthreads();
    }
    const int n_cand = od_compact(N, s_wave,
        [&](int i) {
            if (!od_qualifies(mode, has_mp ? has_mp[i] : 0, object_id[i], keys[i].octave)) return false;
            if (mode != OD_TRACKING) return true;
            const int c = od_cell(G, keys[i].x, keys[i].y);
            return c >= 0 && s_cell[c] == i;
        },
        [&](int pos, int i) { candidates[pos] = i; shuffled[pos] = i; });
    int n_new;
    if (mode == OD_FIRST_FRAME) { // no draws: the points are the candidates with a cuboid in front of the camera, in index order
        n_new = od_compact(n_cand, s_wave, [&](int j) { return cub_depth[object_id[candidates[j]]] > 0; }, [&](int pos, int j) { new_idx[pos] = candidates[j]; });
        if (tid == 0) out[f] = OdFrameOut{n_cand, 0, n_cand, n_new, 0};
    } else {
        if (tid == 0) {
            const int raw = s_raw, max_init = od_max_initialize(mode, N, raw, n_cand), have = draw_first[f + 1] - draw_first[f];
            int nn = 0, lacking = 0;
            if (max_init > have) lacking = 1;
            else if (max_init > 0) nn = od_shuffle_walk(shuffled, n_cand, max_init, max_init, draws + draw_first[f], object_id, cub_depth, new_idx);
            out[f] = OdFrameOut{n_cand, raw, max_init, nn, lacking};
            s_new = nn;
        }
        __syncthreads();
        n_new = s_new;
    }
    __syncthreads(); // new_idx of lane 0 (or of the compaction) is read by every lane below
    for (int j = tid; j < n_new; j += 256) {
        const int i = new_idx[j];
        float x[3];
        od_unproject(keys[i].x, keys[i].y, cub_depth[object_id[i]], K4 + 4 * (size_t)f, Twc + 12 * (size_t)f, x);
        new_x3D[3 * (size_t)j] = x[0]; new_x3D[3 * (size_t)j + 1] = x[1]; new_x3D[3 * (size_t)j + 2] = x[2];
    }
}

static int op_bad(cs_ctx *ctx, const char *fn, const char *what, long a = -1, long b = -1) {
    if (!ctx) return CS_ERR_BAD_ARG;
    char buf[256];
    if (a >= 0 && b >= 0) snprintf(buf, sizeof buf, "%s: %s (%ld, %ld)", fn, what, a, b);
    else if (a >= 0) snprintf(buf, sizeof buf, "%s: %s (%ld)", fn, what, a);
    else snprintf(buf, sizeof buf, "%s: %s", fn, what);
    ctx->err = buf;
    return CS_ERR_BAD_ARG;
}
static bool op_offsets_ok(const int *off, int n) {
    if (!off || off[0] != 0) return false;
    for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
    return true;
}

extern "C" {

int cs_object_points_version(void) { return CS_OBJECT_POINTS_VERSION; }

int cs_triangulate_dynamic_points(cs_ctx *ctx, int n_pairs, const int *first, const float *Tcw_last, const float *Tcw_now, const float *K4, const int *cub_first_last,
                                  const double *cub_pose_last, const int *cub_first_now, const double *cub_pose_now, const int *tracklet_last, const int *tracklet_now,
                                  const float *kp1, const float *kp2, const int *obj_last, const int *obj_now, const int *idx_last, const float *world_pos, uint8_t *status,
                                  float *x3D, float *pos_to_obj, double *dpoints) {
    static const char *fn = "cs_triangulate_dynamic_points";
    if (n_pairs < 0) return op_bad(ctx, fn, "n_pairs < 0");
    if (n_pairs == 0) return CS_OK;
    if (!op_offsets_ok(first, n_pairs)) return op_bad(ctx, fn, "first is NULL, does not start at 0 or decreases");
    if (!op_offsets_ok(cub_first_last, n_pairs) || !op_offsets_ok(cub_first_now, n_pairs)) return op_bad(ctx, fn, "a cuboid offset table is NULL, does not start at 0 or decreases");
    if (!Tcw_last || !Tcw_now || !K4) return op_bad(ctx, fn, "NULL argument");
    if ((tracklet_last == nullptr) != (tracklet_now == nullptr)) return op_bad(ctx, fn, "one tracklet table without the other");
    const int P = first[n_pairs];
    if (P == 0) return CS_OK;
    if (!kp1 || !kp2 || !obj_last || !obj_now || !idx_last || !world_pos || !status || !x3D || !pos_to_obj || !dpoints) return op_bad(ctx, fn, "NULL argument");
    const int n_last = cub_first_last[n_pairs], n_now = cub_first_now[n_pairs];
    std::vector<int> pair_of((size_t)P);
    for (int f = 0; f < n_pairs; f++) {
        const int nl = cub_first_last[f + 1] - cub_first_last[f], nn = cub_first_now[f + 1] - cub_first_now[f];
        for (int i = first[f]; i < first[f + 1]; i++) {
            pair_of[(size_t)i] = f;
            if (idx_last[i] < -1) return op_bad(ctx, fn, "idx_last < -1 (point)", i);
            if (!std::isfinite(kp1[2 * (size_t)i]) || !std::isfinite(kp1[2 * (size_t)i + 1]) || !std::isfinite(kp2[2 * (size_t)i]) || !std::isfinite(kp2[2 * (size_t)i + 1]))
                return op_bad(ctx, fn, "a key point that is not finite (point)", i);
            if (idx_last[i] == -1) continue;
            if (obj_last[i] < 0 || obj_last[i] >= nl) return op_bad(ctx, fn, "an object row outside the last key frame's table (pair, point)", f, i);
            if (obj_now[i] < 0 || obj_now[i] >= nn) return op_bad(ctx, fn, "an object row outside the current key frame's table (pair, point)", f, i);
        }
    }
    if ((n_last && !cub_pose_last) || (n_now && !cub_pose_now)) return op_bad(ctx, fn, "NULL argument");
    std::vector<DynCam> cams((size_t)n_pairs);
    for (int f = 0; f < n_pairs; f++) dyn_make_cam(Tcw_last + 12 * (size_t)f, Tcw_now + 12 * (size_t)f, K4 + 4 * (size_t)f, &cams[(size_t)f]);
    if (!ctx) { // the same statement on the host
        const DynTables T = {cub_first_last, cub_first_now, cub_pose_last, cub_pose_now, tracklet_last, tracklet_now};
        for (int i = 0; i < P; i++) {
            const size_t i2 = 2 * (size_t)i, i3 = 3 * (size_t)i;
            const int f = pair_of[(size_t)i];
            dyn_one(cams[(size_t)f], f, T, kp1 + i2, kp2 + i2, obj_last[i], obj_now[i], idx_last[i], world_pos + i3, status + i, x3D + i3, pos_to_obj + i3, dpoints + i3);
        }
        return CS_OK;
    }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    const size_t n = (size_t)P;
    int *d_pair = nullptr, *d_cfl = nullptr, *d_cfn = nullptr, *d_tl = nullptr, *d_tn = nullptr, *d_ol = nullptr, *d_on = nullptr, *d_il = nullptr;
    DynCam *d_cams = nullptr; double *d_pl = nullptr, *d_pn = nullptr, *d_dp = nullptr; float *d_k1 = nullptr, *d_k2 = nullptr, *d_wp = nullptr, *d_x = nullptr, *d_o = nullptr;
    uint8_t *d_st = nullptr;
    CS_TRY(sc.upload(ctx, &d_pair, pair_of.data(), n)); CS_TRY(sc.upload(ctx, &d_cams, cams.data(), cams.size()));
    CS_TRY(sc.upload(ctx, &d_cfl, cub_first_last, (size_t)n_pairs + 1)); CS_TRY(sc.upload(ctx, &d_cfn, cub_first_now, (size_t)n_pairs + 1));
    CS_TRY(sc.upload(ctx, &d_pl, cub_pose_last, 7 * (size_t)n_last)); CS_TRY(sc.upload(ctx, &d_pn, cub_pose_now, 7 * (size_t)n_now));
    if (tracklet_last) { CS_TRY(sc.upload(ctx, &d_tl, tracklet_last, (size_t)n_last)); CS_TRY(sc.upload(ctx, &d_tn, tracklet_now, (size_t)n_now)); }
    CS_TRY(sc.upload(ctx, &d_k1, kp1, 2 * n)); CS_TRY(sc.upload(ctx, &d_k2, kp2, 2 * n)); CS_TRY(sc.upload(ctx, &d_ol, obj_last, n)); CS_TRY(sc.upload(ctx, &d_on, obj_now, n));
    CS_TRY(sc.upload(ctx, &d_il, idx_last, n)); CS_TRY(sc.upload(ctx, &d_wp, world_pos, 3 * n));
    CS_TRY(sc.alloc(ctx, &d_st, n)); CS_TRY(sc.alloc(ctx, &d_x, 3 * n)); CS_TRY(sc.alloc(ctx, &d_o, 3 * n)); CS_TRY(sc.alloc(ctx, &d_dp, 3 * n));
    const DynTables T = {d_cfl, d_cfn, d_pl, d_pn, d_tl, d_tn};
    CS_LAUNCH(ctx, "dyn_triangulate", dyn_triangulate, dim3((P + 255) / 256), dim3(256), 0, P, d_pair, d_cams, T, d_k1, d_k2, d_ol, d_on, d_il, d_wp, d_st, d_x, d_o, d_dp);
    CS_TRY(cs_d2h(ctx, status, d_st, n)); CS_TRY(cs_d2h(ctx, x3D, d_x, 3 * n)); CS_TRY(cs_d2h(ctx, pos_to_obj, d_o, 3 * n)); CS_TRY(cs_d2h(ctx, dpoints, d_dp, 3 * n));
    return sc.drain();
}

int cs_object_depth_points(cs_ctx *ctx, int mode, int n_frames, const int *first, const cs_keypoint *keys, const uint8_t *has_map_point, const int *object_id,
                           const int *cub_first, const float *cuboid_depth, const float *K4, const float *bounds, const float *Twc, const int *draw_first, const int *draws,
                           int *n_candidates, int *raw_depth_pts, int *max_initialize_pts, int *cand_first, int *candidates, int *shuffled, int *new_first, int *new_idx,
                           float *new_x3D) {
    static const char *fn = "cs_object_depth_points";
    if (mode != OD_FIRST_FRAME && mode != OD_TRACKING && mode != OD_LOCAL_MAPPING) return op_bad(ctx, fn, "unknown mode", mode);
    if (n_frames < 0) return op_bad(ctx, fn, "n_frames < 0");
    if (n_frames == 0) return CS_OK;
    if (!op_offsets_ok(first, n_frames)) return op_bad(ctx, fn, "first is NULL, does not start at 0 or decreases");
    if (!op_offsets_ok(cub_first, n_frames)) return op_bad(ctx, fn, "cub_first is NULL, does not start at 0 or decreases");
    if (mode != OD_FIRST_FRAME && !op_offsets_ok(draw_first, n_frames)) return op_bad(ctx, fn, "draw_first is NULL, does not start at 0 or decreases");
    if (!K4 || !Twc || !n_candidates || !raw_depth_pts || !max_initialize_pts || !cand_first || !new_first || (mode == OD_TRACKING && !bounds)) return op_bad(ctx, fn, "NULL argument");
    const int total = first[n_frames], n_cub = cub_first[n_frames], n_draws = mode == OD_FIRST_FRAME ? 0 : draw_first[n_frames];
    if (total && (!keys || !object_id || (mode != OD_FIRST_FRAME && !has_map_point) || !candidates || !shuffled || !new_idx || !new_x3D)) return op_bad(ctx, fn, "NULL argument");
    if ((n_cub && !cuboid_depth) || (n_draws && !draws)) return op_bad(ctx, fn, "NULL argument");
    for (int f = 0; f < n_frames; f++) {
        if (first[f + 1] - first[f] > CS_RGBD_MAX_KEYPOINTS) return op_bad(ctx, fn, "a frame with more than CS_RGBD_MAX_KEYPOINTS key points (frame)", f);
        const int nc = cub_first[f + 1] - cub_first[f];
        for (int i = first[f]; i < first[f + 1]; i++) if (object_id[i] >= nc) return op_bad(ctx, fn, "an object id at or beyond the frame's cuboid count (frame, key point)", f, i - first[f]);
    }
    for (int d = 0; d < n_draws; d++) if (draws[d] < 0) return op_bad(ctx, fn, "a negative draw", d);
    if (mode == OD_TRACKING)
        for (int f = 0; f < n_frames; f++) {
            const float *b = bounds + 4 * (size_t)f;
            for (int k = 0; k < 4; k++) if (!(std::fabs(b[k]) < 1e9f)) return op_bad(ctx, fn, "image bounds that are not finite or beyond 1e9 (frame)", f);
            if (!(b[1] > b[0]) || !(b[3] > b[2])) return op_bad(ctx, fn, "image bounds with mnMaxX <= mnMinX or mnMaxY <= mnMinY (frame)", f);
        }
    const size_t n = (size_t)total, F = (size_t)n_frames;
    static const int no_draws[1] = {0};
    std::vector<int> zero_first;
    if (mode == OD_FIRST_FRAME) { zero_first.assign(F + 1, 0); draw_first = zero_first.data(); draws = no_draws; }
    std::vector<OdFrameOut> out(F);
    std::vector<int> h_cand(n), h_shuf(n), h_new(n);
    std::vector<float> h_x(3 * n);
    if (!ctx) {
        for (int f = 0; f < n_frames; f++) {
            const int b0 = first[f];
            od_frame_host(mode, first[f + 1] - b0, reinterpret_cast<const OdKey *>(keys) + b0, has_map_point ? has_map_point + b0 : nullptr, object_id + b0, cuboid_depth + cub_first[f], K4 + 4 * (size_t)f,
                          bounds ? bounds + 4 * (size_t)f : nullptr, Twc + 12 * (size_t)f, draw_first[f + 1] - draw_first[f], draws + draw_first[f], &out[(size_t)f],
                          h_cand.data() + b0, h_shuf.data() + b0, h_new.data() + b0, h_x.data() + 3 * (size_t)b0);
        }
    } else {
        CS_HIP(ctx, hipSetDevice(ctx->device));
        cs_scratch sc(ctx);
        int *d_first = nullptr, *d_oid = nullptr, *d_cf = nullptr, *d_df = nullptr, *d_draws = nullptr, *d_cand = nullptr, *d_shuf = nullptr, *d_new = nullptr;
        cs_keypoint *d_keys = nullptr; uint8_t *d_mp = nullptr; float *d_cd = nullptr, *d_K = nullptr, *d_b = nullptr, *d_T = nullptr, *d_x = nullptr; OdFrameOut *d_out = nullptr;
        CS_TRY(sc.upload(ctx, &d_first, first, F + 1)); CS_TRY(sc.upload(ctx, &d_keys, keys, n)); CS_TRY(sc.upload(ctx, &d_oid, object_id, n));
        if (has_map_point) CS_TRY(sc.upload(ctx, &d_mp, has_map_point, n));
        CS_TRY(sc.upload(ctx, &d_cf, cub_first, F + 1)); CS_TRY(sc.upload(ctx, &d_cd, cuboid_depth, (size_t)n_cub)); CS_TRY(sc.upload(ctx, &d_K, K4, 4 * F));
        if (mode == OD_TRACKING) CS_TRY(sc.upload(ctx, &d_b, bounds, 4 * F));
        CS_TRY(sc.upload(ctx, &d_T, Twc, 12 * F)); CS_TRY(sc.upload(ctx, &d_df, draw_first, F + 1)); CS_TRY(sc.upload(ctx, &d_draws, draws, (size_t)n_draws));
        CS_TRY(sc.alloc(ctx, &d_out, F)); CS_TRY(sc.alloc(ctx, &d_cand, n)); CS_TRY(sc.alloc(ctx, &d_shuf, n)); CS_TRY(sc.alloc(ctx, &d_new, n)); CS_TRY(sc.alloc(ctx, &d_x, 3 * n));
        CS_LAUNCH(ctx, "od_frame", od_frame, dim3(n_frames), dim3(256), 0, mode, d_first, d_keys, d_mp, d_oid, d_cf, d_cd, d_K, d_b, d_T, d_df, d_draws, d_out, d_cand, d_shuf, d_new, d_x);
        CS_TRY(cs_d2h(ctx, out.data(), d_out, F)); CS_TRY(cs_d2h(ctx, h_cand.data(), d_cand, n)); CS_TRY(cs_d2h(ctx, h_shuf.data(), d_shuf, n));
        CS_TRY(cs_d2h(ctx, h_new.data(), d_new, n)); CS_TRY(cs_d2h(ctx, h_x.data(), d_x, 3 * n));
        CS_TRY(sc.drain());
    }
    for (int f = 0; f < n_frames; f++) if (out[(size_t)f].short_of_draws) return op_bad(ctx, fn, "fewer draws than max_initialize_pts (frame, max_initialize_pts)", f, out[(size_t)f].max_initialize_pts);
    // the frames' slices, one behind the other
    cand_first[0] = 0; new_first[0] = 0;
    for (int f = 0; f < n_frames; f++) {
        const OdFrameOut &o = out[(size_t)f];
        const int b0 = first[f], c0 = cand_first[f], n0 = new_first[f];
        n_candidates[f] = o.n_candidates; raw_depth_pts[f] = o.raw_depth_pts; max_initialize_pts[f] = o.max_initialize_pts;
        for (int j = 0; j < o.n_candidates; j++) { candidates[c0 + j] = h_cand[(size_t)b0 + j]; shuffled[c0 + j] = h_shuf[(size_t)b0 + j]; }
        for (int j = 0; j < o.n_new; j++) { new_idx[n0 + j] = h_new[(size_t)b0 + j]; for (int k = 0; k < 3; k++) new_x3D[3 * (size_t)(n0 + j) + k] = h_x[3 * ((size_t)b0 + j) + k]; }
        cand_first[f + 1] = c0 + o.n_candidates; new_first[f + 1] = n0 + o.n_new;
    }
    return CS_OK;
}

} // extern "C"
