// covisibility.hip -- KeyFrame::UpdateConnections (KeyFrame.cc:345-437), LocalMapping::KeyFrameCulling (LocalMapping.cc:833-902, with KeyFrame::SetBadFlag :511-529 and
// MapPoint::EraseObservation, MapPoint.cc:178-205) and LocalMapping::MapPointCulling (LocalMapping.cc:249-302) on MI355X (gfx950).  The C-ABI is
// include/cubeslam_hip/covisibility.h; predicates and arithmetic are covis_math.h, shared with the host forms (covis_walk.h).
//
// The vote, one workgroup per query key frame:
//   covis_vote<false>  counters of COVIS_COUNTER_TILE key-frame indices in LDS; the threads walk the observation runs of the query's slots and add with LDS atomics (one add for
//                      the wave where all its active lanes hit the same counter); n_kf above the tile takes several sweeps over the slots.  Behind each sweep the non-zero
//                      counters are counted; out: per query the number of counters, of counters >= th, and (w_max, kf_max)
//   covis_offsets      exclusive scans of both numbers over the queries (one workgroup): cnt_off, ord_off.  The host reads cnt_off and stops here when conn_cap is too small
//   covis_vote<true>   the vote again, now with an ordered compaction of the non-zero counters behind each sweep (a scan inside the workgroup, a carry between sweeps), then the
//                      ordered list by rank counting: an entry's place is the number of entries that stand in front of it (covis_ordered_before), so nothing depends on the
//                      order in which anything ran.  An integer sum does not depend on the order of its atomics either.
// The culling is a sequence (an erased key frame changes what every later one counts), run in rounds:
//   covis_cull_eval    one workgroup per remaining key frame of the list, threads over its slots, each walking one observation run on the current state; atomicMin finds the
//                      first key frame that erases.  Every verdict up to and including that one is final, because no state changed in front of it.
//   covis_cull_erase   that key frame's EraseObservation calls, threads over its slots.  The alive byte is cleared with an atomic AND on its word, and only the thread that saw
//                      it set goes on, so a point held in two slots is erased once.
//   The next round starts behind it: rounds = erasing key frames + 1, and the common cycle, where nothing is culled, is one parallel pass.
//   covis_mp_cases     MapPointCulling: one thread per entry of the recent list.
#include "common.h"
#include "../../include/cubeslam_hip/covisibility.h"
#include "covis_walk.h"

#include <climits>
#include <cstddef>

namespace {
constexpr int CV_BLOCK = 256, CV_PER = COVIS_COUNTER_TILE / CV_BLOCK;
static_assert(COVIS_COUNTER_TILE % CV_BLOCK == 0, "the compaction gives every thread the same number of counters");

struct covis_dtable { // cs_obs_table on the device
    int n_kf, n_points;
    const int *obs_off, *obs_kf, *obs_octave;
    const uint8_t *obs_stereo;
};

constexpr int CV_WAVES = CV_BLOCK / 64;
__device__ __forceinline__ int cv_sum256(int v, int *s_w) { int total; block_excl_scan<CV_WAVES>(v, s_w, &total); return total; }

template <bool EMIT>
__global__ void __launch_bounds__(CV_BLOCK) covis_vote(covis_dtable t, const uint8_t *mp_flags, const int *query_kf, const int *kf_off, const int *kf_mp, int skip_dynamic, int th,
                                                       int *n_cnt, int *n_ge, int *kf_max, int *w_max, const int *cnt_off, int *cnt_kf, int *cnt_w, const int *ord_off, int *ord_kf,
                                                       int *ord_w) {
    __shared__ int s_cnt[COVIS_COUNTER_TILE];
    __shared__ int s_w[4];
    __shared__ unsigned long long s_key[4];
    const int q = blockIdx.x, self = query_kf[q], s_begin = kf_off[q], s_end = kf_off[q + 1];
    const int lane = threadIdx.x & 63;
    int carry = 0, ge = 0;
    unsigned long long best = 0; // (a counter that exists has w >= 1: its key is above 0)
    for (int lo = 0; lo < t.n_kf; lo += COVIS_COUNTER_TILE) {
        for (int k = threadIdx.x; k < COVIS_COUNTER_TILE; k += CV_BLOCK) s_cnt[k] = 0;
        __syncthreads();
        for (int s0 = s_begin; s0 < s_end; s0 += CV_BLOCK) { // (wave-uniform: the ballots below see whole waves)
            const int s = s0 + threadIdx.x;
            int b = 0, e = 0;
            if (s < s_end) {
                const int p = kf_mp[s];
                if (!covis_vote_skips(p, mp_flags, skip_dynamic)) { b = t.obs_off[p]; e = t.obs_off[p + 1]; }
            }
            for (int j = 0; __any(b + j < e); j++) {
                int k = -1;
                if (b + j < e) { k = t.obs_kf[b + j] - lo; if (k + lo == self || k < 0 || k >= COVIS_COUNTER_TILE) k = -1; }
                const unsigned long long hit = __ballot(k >= 0);
                if (!hit) continue;
                const int lead = __ffsll((long long)hit) - 1, k0 = __shfl(k, lead);
                if (__ballot(k == k0) == hit) { // every voting lane on one counter: one add for the wave
                    if (lane == lead) atomicAdd(&s_cnt[k0], __popcll(hit));
                } else if (k >= 0) atomicAdd(&s_cnt[k], 1);
            }
        }
        __syncthreads();
        // this thread's CV_PER consecutive counters, ascending
        const int k0 = threadIdx.x * CV_PER;
        int mine = 0;
        for (int k = 0; k < CV_PER; k++) {
            const int w = s_cnt[k0 + k];
            if (!w) continue;
            mine++;
            ge += w >= th;
            const unsigned long long key = covis_max_key(w, lo + k0 + k);
            if (key > best) best = key;
        }
        int total;
        int o = block_excl_scan<CV_WAVES>(mine, s_w, &total);
        if (EMIT) {
            o += cnt_off[q] + carry;
            for (int k = 0; k < CV_PER; k++) { const int w = s_cnt[k0 + k]; if (w) { cnt_kf[o] = lo + k0 + k; cnt_w[o] = w; o++; } }
        }
        carry += total;
        __syncthreads(); // s_cnt is zeroed again at the top
    }
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(best, off); if (o > best) best = o; }
    if (lane == 0) s_key[threadIdx.x >> 6] = best;
    ge = cv_sum256(ge, s_w); // (its barriers stand between the store of s_key and the loads)
    for (int k = 0; k < 4; k++) if (s_key[k] > best) best = s_key[k];
    if (!EMIT) {
        if (threadIdx.x == 0) {
            n_cnt[q] = carry;
            n_ge[q] = carry == 0 ? 0 : (ge ? ge : 1); // the length of the ordered list: the fallback pair when nothing reaches th
            kf_max[q] = carry ? covis_key_kf(best) : -1;
            w_max[q] = carry ? covis_key_w(best) : 0;
        }
        return;
    }
    if (carry == 0) return;
    const int c0 = cnt_off[q], o0 = ord_off[q];
    if (ge == 0) { // vPairs.empty() :405
        if (threadIdx.x == 0) { ord_kf[o0] = covis_key_kf(best); ord_w[o0] = covis_key_w(best); }
        return;
    }
    __syncthreads(); // the workgroup's own stores to cnt_kf / cnt_w are read back below
    for (int i = threadIdx.x; i < carry; i += CV_BLOCK) {
        const int w = cnt_w[c0 + i], kf = cnt_kf[c0 + i];
        if (w < th) continue;
        int rank = 0;
        for (int j = 0; j < carry; j++) { const int wj = cnt_w[c0 + j]; rank += wj >= th && covis_ordered_before(wj, cnt_kf[c0 + j], w, kf); }
        ord_kf[o0 + rank] = kf; ord_w[o0 + rank] = w; // (rank < ge = ord_off[q + 1] - o0: the key-frame indices of a run differ, so the ranks are a permutation)
    }
}

// exclusive scans of a[n] and b[n] into a_off[n + 1], b_off[n + 1]; one workgroup
__global__ void __launch_bounds__(CV_BLOCK) covis_offsets(int n, const int *a, const int *b, int *a_off, int *b_off) {
    __shared__ int s_w[4];
    int ca = 0, cb = 0;
    for (int i0 = 0; i0 < n; i0 += CV_BLOCK) {
        const int i = i0 + threadIdx.x;
        const int va = i < n ? a[i] : 0, vb = i < n ? b[i] : 0;
        int ta, tb;
        const int ea = block_excl_scan<CV_WAVES>(va, s_w, &ta), eb = block_excl_scan<CV_WAVES>(vb, s_w, &tb);
        if (i < n) { a_off[i] = ca + ea; b_off[i] = cb + eb; }
        ca += ta; cb += tb;
    }
    if (threadIdx.x == 0) { a_off[n] = ca; b_off[n] = cb; }
}

// alive[e] = 1 for the entries of points that are not bad on entry
__global__ void __launch_bounds__(CV_BLOCK) covis_cull_init(int n_points, const int *obs_off, const uint8_t *flags, uint8_t *alive) {
    const int p = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (p >= n_points) return;
    const uint8_t a = !(flags[p] & COVIS_MP_BAD);
    for (int e = obs_off[p]; e < obs_off[p + 1]; e++) alive[e] = a;
}

__global__ void __launch_bounds__(CV_BLOCK) covis_cull_eval(covis_dtable t, int start, const int *local_kf, const int *kf_off, const int *kf_mp, const int *slot_octave,
                                                            const float *slot_depth, const float *kf_th_depth, int monocular, const uint8_t *kf_flags, int th_obs, const int *nobs,
                                                            const uint8_t *flags, const uint8_t *alive, uint8_t *verdict, int *n_mps, int *n_redundant, int *first_erase) {
    __shared__ int s_w[4];
    const int i = start + blockIdx.x, kf = local_kf[i];
    const uint8_t kflags = kf_flags[i];
    int mps = 0, red = 0;
    if (!(kflags & COVIS_KF_ID0)) { // (uniform over the workgroup)
        const float th_depth = kf_th_depth[i];
        for (int s = kf_off[i] + threadIdx.x; s < kf_off[i + 1]; s += CV_BLOCK) {
            const int p = kf_mp[s];
            if (covis_cull_skips(p, flags, monocular, slot_depth[s], th_depth)) continue;
            mps++;
            red += covis_cull_redundant(p, kf, slot_octave[s], th_obs, nobs, t.obs_off, t.obs_kf, t.obs_octave, alive);
        }
    }
    mps = cv_sum256(mps, s_w);
    red = cv_sum256(red, s_w);
    if (threadIdx.x == 0) {
        const uint8_t v = covis_cull_verdict(red, mps, kflags);
        verdict[i] = v; n_mps[i] = mps; n_redundant[i] = red;
        if (v == COVIS_CULLED) atomicMin(first_erase, i);
    }
}

// clears byte e of `bytes` and returns what it held: an atomic AND on the byte's word (the block is a device allocation, so the word is inside it)
__device__ __forceinline__ uint8_t cv_clear_byte(uint8_t *bytes, int e) {
    unsigned *word = reinterpret_cast<unsigned *>(bytes) + (e >> 2);
    const int shift = (e & 3) * 8;
    return (uint8_t)((atomicAnd(word, ~(0xffu << shift)) >> shift) & 0xffu);
}

__global__ void __launch_bounds__(CV_BLOCK) covis_cull_erase(covis_dtable t, int kf, int s_begin, int s_end, const int *kf_mp, int *nobs, uint8_t *flags, uint8_t *alive) {
    const int s = s_begin + blockIdx.x * CV_BLOCK + threadIdx.x;
    if (s >= s_end) return;
    const int p = kf_mp[s];
    if (p < 0) return;
    const int e = covis_find_entry(p, kf, t.obs_off, t.obs_kf);
    if (e < 0 || !cv_clear_byte(alive, e)) return; // no entry, dead already, or another slot of the same point was here first
    // the one thread that erases p's entry: nobody else writes nobs[p] or flags[p] in this launch
    const int n = nobs[p] - covis_erase_step(t.obs_stereo[e]);
    nobs[p] = n;
    if (covis_erase_turns_bad(n)) {
        flags[p] |= COVIS_MP_BAD;
        for (int k = t.obs_off[p]; k < t.obs_off[p + 1]; k++) cv_clear_byte(alive, k);
    }
}

__global__ void __launch_bounds__(CV_BLOCK) covis_mp_cases(int n_recent, const int *recent, const uint8_t *flags, const int *found, const int *visible, const int *nobs,
                                                           const int *first_kf_id, int current_kf_id, int th_obs, uint8_t *cases) {
    const int i = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (i >= n_recent) return;
    const int p = recent[i];
    cases[i] = covis_mappoint_case(flags[p], found[p], visible[p], nobs[p], first_kf_id[p], current_kf_id, th_obs);
}

const covis_table *as_walk(const cs_obs_table *t) { return reinterpret_cast<const covis_table *>(t); }
static_assert(sizeof(covis_table) == sizeof(cs_obs_table) && offsetof(covis_table, mp_flags) == offsetof(cs_obs_table, mp_flags), "covis_walk.h restates cs_obs_table");

// the observation runs on the device; the vote reads the key frames only (levels = false: obs_octave and obs_stereo stay NULL)
int upload_table(cs_ctx *ctx, cs_scratch &sc, const cs_obs_table *t, bool levels, covis_dtable *d) {
    const size_t n_obs = (size_t)t->obs_off[t->n_points];
    int *off = nullptr, *kf = nullptr, *oct = nullptr; uint8_t *st = nullptr;
    CS_TRY(sc.upload(ctx, &off, t->obs_off, (size_t)t->n_points + 1)); CS_TRY(sc.upload(ctx, &kf, t->obs_kf, n_obs));
    if (levels) { CS_TRY(sc.upload(ctx, &oct, t->obs_octave, n_obs)); CS_TRY(sc.upload(ctx, &st, t->obs_stereo, n_obs)); }
    *d = covis_dtable{t->n_kf, t->n_points, off, kf, oct, st};
    return CS_OK;
}
} // namespace

extern "C" {

int cs_covisibility_version(void) { return CS_COVISIBILITY_VERSION; }

int cs_covisibility_update_host(const cs_obs_table *table, int n_query, const int *query_kf, const int *kf_off, const int *kf_mp, int skip_dynamic, int th, int conn_cap,
                                int *cnt_off, int *cnt_kf, int *cnt_w, int *kf_max, int *w_max, int *ord_off, int *ord_kf, int *ord_w) {
    return covis_update_host(as_walk(table), n_query, query_kf, kf_off, kf_mp, skip_dynamic, th, conn_cap, cnt_off, cnt_kf, cnt_w, kf_max, w_max, ord_off, ord_kf, ord_w);
}

int cs_covisibility_update(cs_ctx *ctx, const cs_obs_table *table, int n_query, const int *query_kf, const int *kf_off, const int *kf_mp, int skip_dynamic, int th, int conn_cap,
                           int *cnt_off, int *cnt_kf, int *cnt_w, int *kf_max, int *w_max, int *ord_off, int *ord_kf, int *ord_w) {
    const covis_table *t = as_walk(table);
    if (!ctx || !covis_table_ok(t) || !covis_lists_ok(t, n_query, query_kf, kf_off, kf_mp) || conn_cap < 0 || !cnt_off || !ord_off || (n_query && (!kf_max || !w_max)) ||
        (conn_cap && (!cnt_kf || !cnt_w || !ord_kf || !ord_w)))
        return CS_ERR_BAD_ARG;
    cnt_off[0] = 0; ord_off[0] = 0;
    if (n_query == 0) return CS_OK;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)n_query, n_slots = (size_t)kf_off[n_query];
    cs_scratch sc(ctx);
    covis_dtable d;
    CS_TRY(upload_table(ctx, sc, table, false, &d));
    uint8_t *d_flags = nullptr;
    int *d_query = nullptr, *d_kf_off = nullptr, *d_kf_mp = nullptr, *d_n_cnt = nullptr, *d_n_ge = nullptr, *d_kf_max = nullptr, *d_w_max = nullptr, *d_cnt_off = nullptr,
        *d_ord_off = nullptr, *d_cnt_kf = nullptr, *d_cnt_w = nullptr, *d_ord_kf = nullptr, *d_ord_w = nullptr;
    CS_TRY(sc.upload(ctx, &d_flags, table->mp_flags, (size_t)table->n_points));
    CS_TRY(sc.upload(ctx, &d_query, query_kf, nq)); CS_TRY(sc.upload(ctx, &d_kf_off, kf_off, nq + 1)); CS_TRY(sc.upload(ctx, &d_kf_mp, kf_mp, n_slots));
    CS_TRY(sc.alloc(ctx, &d_n_cnt, nq)); CS_TRY(sc.alloc(ctx, &d_n_ge, nq)); CS_TRY(sc.alloc(ctx, &d_kf_max, nq)); CS_TRY(sc.alloc(ctx, &d_w_max, nq));
    CS_TRY(sc.alloc(ctx, &d_cnt_off, nq + 1)); CS_TRY(sc.alloc(ctx, &d_ord_off, nq + 1));
    CS_LAUNCH(ctx, "covis_vote_count", covis_vote<false>, dim3(n_query), dim3(CV_BLOCK), 0, d, d_flags, d_query, d_kf_off, d_kf_mp, skip_dynamic, th, d_n_cnt, d_n_ge, d_kf_max,
              d_w_max, (const int *)nullptr, (int *)nullptr, (int *)nullptr, (const int *)nullptr, (int *)nullptr, (int *)nullptr);
    CS_LAUNCH(ctx, "covis_offsets", covis_offsets, dim3(1), dim3(CV_BLOCK), 0, n_query, d_n_cnt, d_n_ge, d_cnt_off, d_ord_off);
    std::vector<int> h_cnt_off(nq + 1), h_ord_off(nq + 1);
    CS_TRY(cs_d2h(ctx, h_cnt_off.data(), d_cnt_off, nq + 1)); CS_TRY(cs_d2h(ctx, h_ord_off.data(), d_ord_off, nq + 1));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // (a sum of at most n_query * n_kf counters: beyond INT_MAX the scan has wrapped, which shows as a decrease)
    for (size_t q = 0; q < nq; q++) if (h_cnt_off[q + 1] < h_cnt_off[q] || h_ord_off[q + 1] < h_ord_off[q]) { ctx->err = "cs_covisibility_update: more than INT_MAX counters"; return CS_ERR_CAPACITY; }
    memcpy(cnt_off, h_cnt_off.data(), sizeof(int) * (nq + 1));
    const size_t n_cnt = (size_t)h_cnt_off[nq], n_ord = (size_t)h_ord_off[nq];
    if (n_cnt > (size_t)conn_cap) { ctx->err = "cs_covisibility_update: the counters need more than conn_cap entries (cnt_off holds the sizes)"; return CS_ERR_CAPACITY; }
    if (n_ord > n_cnt || h_cnt_off[0] != 0 || h_ord_off[0] != 0) { ctx->err = "cs_covisibility_update: offsets out of range"; return CS_ERR_HIP; }
    CS_TRY(sc.alloc(ctx, &d_cnt_kf, n_cnt)); CS_TRY(sc.alloc(ctx, &d_cnt_w, n_cnt)); CS_TRY(sc.alloc(ctx, &d_ord_kf, n_ord)); CS_TRY(sc.alloc(ctx, &d_ord_w, n_ord));
    CS_LAUNCH(ctx, "covis_vote_emit", covis_vote<true>, dim3(n_query), dim3(CV_BLOCK), 0, d, d_flags, d_query, d_kf_off, d_kf_mp, skip_dynamic, th, (int *)nullptr, (int *)nullptr,
              (int *)nullptr, (int *)nullptr, (const int *)d_cnt_off, d_cnt_kf, d_cnt_w, (const int *)d_ord_off, d_ord_kf, d_ord_w);
    std::vector<int> h_cnt_kf(n_cnt), h_cnt_w(n_cnt), h_ord_kf(n_ord), h_ord_w(n_ord), h_kf_max(nq), h_w_max(nq);
    CS_TRY(cs_d2h(ctx, h_cnt_kf.data(), d_cnt_kf, n_cnt)); CS_TRY(cs_d2h(ctx, h_cnt_w.data(), d_cnt_w, n_cnt));
    CS_TRY(cs_d2h(ctx, h_ord_kf.data(), d_ord_kf, n_ord)); CS_TRY(cs_d2h(ctx, h_ord_w.data(), d_ord_w, n_ord));
    CS_TRY(cs_d2h(ctx, h_kf_max.data(), d_kf_max, nq)); CS_TRY(cs_d2h(ctx, h_w_max.data(), d_w_max, nq));
    CS_TRY(sc.drain());
    memcpy(ord_off, h_ord_off.data(), sizeof(int) * (nq + 1));
    memcpy(kf_max, h_kf_max.data(), sizeof(int) * nq); memcpy(w_max, h_w_max.data(), sizeof(int) * nq);
    if (n_cnt) { memcpy(cnt_kf, h_cnt_kf.data(), sizeof(int) * n_cnt); memcpy(cnt_w, h_cnt_w.data(), sizeof(int) * n_cnt); }
    if (n_ord) { memcpy(ord_kf, h_ord_kf.data(), sizeof(int) * n_ord); memcpy(ord_w, h_ord_w.data(), sizeof(int) * n_ord); }
    return CS_OK;
}

int cs_keyframe_culling_host(const cs_obs_table *table, int n_local, const int *local_kf, const int *kf_off, const int *kf_mp, const int *slot_octave, const float *slot_depth,
                             const float *kf_th_depth, int monocular, const uint8_t *kf_flags, int th_obs, uint8_t *verdict, int *n_mps, int *n_redundant, int *out_nobs,
                             uint8_t *out_flags, uint8_t *out_alive, int *n_rounds) {
    return covis_keyframe_culling_host(as_walk(table), n_local, local_kf, kf_off, kf_mp, slot_octave, slot_depth, kf_th_depth, monocular, kf_flags, th_obs, verdict, n_mps,
                                       n_redundant, out_nobs, out_flags, out_alive, n_rounds);
}

int cs_keyframe_culling(cs_ctx *ctx, const cs_obs_table *table, int n_local, const int *local_kf, const int *kf_off, const int *kf_mp, const int *slot_octave, const float *slot_depth,
                        const float *kf_th_depth, int monocular, const uint8_t *kf_flags, int th_obs, uint8_t *verdict, int *n_mps, int *n_redundant, int *out_nobs,
                        uint8_t *out_flags, uint8_t *out_alive, int *n_rounds) {
    const covis_table *t = as_walk(table);
    if (!ctx || !covis_culling_args_ok(t, n_local, local_kf, kf_off, kf_mp, slot_octave, slot_depth, kf_th_depth, kf_flags, verdict, n_mps, n_redundant, out_nobs, out_flags, out_alive))
        return CS_ERR_BAD_ARG;
    if (n_rounds) *n_rounds = 0;
    if (n_local == 0) { covis_culling_init(t, out_nobs, out_flags, out_alive); return CS_OK; }
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nl = (size_t)n_local, n_slots = (size_t)kf_off[n_local], np = (size_t)table->n_points, n_obs = (size_t)table->obs_off[table->n_points];
    std::vector<uint8_t> h_verdict(nl), h_flags(np), h_alive(n_obs);
    std::vector<int> h_mps(nl), h_red(nl), h_nobs(np);
    int first = 0;
    cs_scratch sc(ctx);
    covis_dtable d;
    CS_TRY(upload_table(ctx, sc, table, true, &d));
    int *d_local = nullptr, *d_kf_off = nullptr, *d_kf_mp = nullptr, *d_oct = nullptr, *d_nobs = nullptr, *d_mps = nullptr, *d_red = nullptr, *d_first = nullptr;
    float *d_depth = nullptr, *d_th = nullptr;
    uint8_t *d_kflags = nullptr, *d_flags = nullptr, *d_alive = nullptr, *d_verdict = nullptr;
    CS_TRY(sc.upload(ctx, &d_local, local_kf, nl)); CS_TRY(sc.upload(ctx, &d_kf_off, kf_off, nl + 1)); CS_TRY(sc.upload(ctx, &d_kf_mp, kf_mp, n_slots));
    CS_TRY(sc.upload(ctx, &d_oct, slot_octave, n_slots)); CS_TRY(sc.upload(ctx, &d_depth, slot_depth, n_slots)); CS_TRY(sc.upload(ctx, &d_th, kf_th_depth, nl));
    CS_TRY(sc.upload(ctx, &d_kflags, kf_flags, nl)); CS_TRY(sc.upload(ctx, &d_nobs, table->mp_nobs, np)); CS_TRY(sc.upload(ctx, &d_flags, table->mp_flags, np));
    CS_TRY(sc.alloc(ctx, &d_alive, n_obs + 4)); // (whole words for cv_clear_byte)
    CS_TRY(sc.alloc(ctx, &d_verdict, nl)); CS_TRY(sc.alloc(ctx, &d_mps, nl)); CS_TRY(sc.alloc(ctx, &d_red, nl)); CS_TRY(sc.alloc(ctx, &d_first, (size_t)1));
    if (np) CS_LAUNCH(ctx, "covis_cull_init", covis_cull_init, dim3((unsigned)((np + CV_BLOCK - 1) / CV_BLOCK)), dim3(CV_BLOCK), 0, table->n_points, d.obs_off, d_flags, d_alive);
    int rounds = 0;
    for (int start = 0; start < n_local; start = first + 1) {
        CS_HIP(ctx, hipMemsetAsync(d_first, 0x7f, sizeof(int), ctx->stream)); // above every position of the list
        CS_LAUNCH(ctx, "covis_cull_eval", covis_cull_eval, dim3(n_local - start), dim3(CV_BLOCK), 0, d, start, d_local, d_kf_off, d_kf_mp, d_oct, d_depth, d_th, monocular, d_kflags,
                  th_obs, d_nobs, d_flags, d_alive, d_verdict, d_mps, d_red, d_first);
        CS_TRY(cs_d2h(ctx, &first, d_first, 1));
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        rounds++;
        if (first >= n_local) break; // nobody erases: every verdict is final
        if (first < start) { ctx->err = "cs_keyframe_culling: position out of range"; return CS_ERR_HIP; }
        const int s_begin = kf_off[first], s_end = kf_off[first + 1];
        if (s_end > s_begin)
            CS_LAUNCH(ctx, "covis_cull_erase", covis_cull_erase, dim3((s_end - s_begin + CV_BLOCK - 1) / CV_BLOCK), dim3(CV_BLOCK), 0, d, local_kf[first], s_begin, s_end, d_kf_mp,
                      d_nobs, d_flags, d_alive);
    }
    CS_TRY(cs_d2h(ctx, h_verdict.data(), d_verdict, nl)); CS_TRY(cs_d2h(ctx, h_mps.data(), d_mps, nl)); CS_TRY(cs_d2h(ctx, h_red.data(), d_red, nl));
    CS_TRY(cs_d2h(ctx, h_nobs.data(), d_nobs, np)); CS_TRY(cs_d2h(ctx, h_flags.data(), d_flags, np)); CS_TRY(cs_d2h(ctx, h_alive.data(), d_alive, n_obs));
    CS_TRY(sc.drain());
    memcpy(verdict, h_verdict.data(), nl); memcpy(n_mps, h_mps.data(), sizeof(int) * nl); memcpy(n_redundant, h_red.data(), sizeof(int) * nl);
    if (np) { memcpy(out_nobs, h_nobs.data(), sizeof(int) * np); memcpy(out_flags, h_flags.data(), np); }
    if (n_obs) memcpy(out_alive, h_alive.data(), n_obs);
    if (n_rounds) *n_rounds = rounds;
    return CS_OK;
}

int cs_mappoint_culling_host(const cs_obs_table *table, int n_recent, const int *recent, const int *mp_found, const int *mp_visible, const int *mp_first_kf_id,
                             int current_kf_id, int th_obs, uint8_t *cases) {
    return covis_mappoint_culling_host(as_walk(table), n_recent, recent, mp_found, mp_visible, mp_first_kf_id, current_kf_id, th_obs, cases);
}

int cs_mappoint_culling(cs_ctx *ctx, const cs_obs_table *table, int n_recent, const int *recent, const int *mp_found, const int *mp_visible, const int *mp_first_kf_id,
                        int current_kf_id, int th_obs, uint8_t *cases) {
    const covis_table *t = as_walk(table);
    if (!ctx || !covis_mappoint_args_ok(t, n_recent, recent, mp_found, mp_visible, mp_first_kf_id, cases)) return CS_ERR_BAD_ARG;
    if (n_recent == 0) return CS_OK;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nr = (size_t)n_recent, np = (size_t)table->n_points;
    std::vector<uint8_t> h_cases(nr);
    cs_scratch sc(ctx);
    int *d_recent = nullptr, *d_found = nullptr, *d_visible = nullptr, *d_first = nullptr, *d_nobs = nullptr;
    uint8_t *d_flags = nullptr, *d_cases = nullptr;
    CS_TRY(sc.upload(ctx, &d_recent, recent, nr)); CS_TRY(sc.upload(ctx, &d_found, mp_found, np)); CS_TRY(sc.upload(ctx, &d_visible, mp_visible, np));
    CS_TRY(sc.upload(ctx, &d_first, mp_first_kf_id, np)); CS_TRY(sc.upload(ctx, &d_nobs, table->mp_nobs, np)); CS_TRY(sc.upload(ctx, &d_flags, table->mp_flags, np));
    CS_TRY(sc.alloc(ctx, &d_cases, nr));
    CS_LAUNCH(ctx, "covis_mp_cases", covis_mp_cases, dim3((unsigned)((nr + CV_BLOCK - 1) / CV_BLOCK)), dim3(CV_BLOCK), 0, n_recent, d_recent, d_flags, d_found, d_visible, d_nobs,
              d_first, current_kf_id, th_obs, d_cases);
    CS_TRY(cs_d2h(ctx, h_cases.data(), d_cases, nr));
    CS_TRY(sc.drain());
    memcpy(cases, h_cases.data(), nr);
    return CS_OK;
}

} // extern "C"
