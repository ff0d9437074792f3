// covis_walk.h -- the argument checks and the host forms of covisibility.hip: the reference's loops as sequences over the tables, with the predicates of covis_math.h.
// Plain C++ (no HIP, no library header): tests/cpp/covisibility_driver.cpp compiles it with g++ under the sanitizers.  Return values: 0 ok, -2 bad argument, -4 capacity
// (CS_OK, CS_ERR_BAD_ARG, CS_ERR_CAPACITY).
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "covis_math.h"

struct covis_table { // cs_obs_table, field by field
    int n_kf, n_points;
    const int *obs_off, *obs_kf, *obs_octave;
    const uint8_t *obs_stereo;
    const int *mp_nobs;
    const uint8_t *mp_flags;
};

inline bool covis_offsets_ok(const int *off, int n) {
    if (!off || off[0] != 0) return false;
    for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
    return true;
}
// the point side only (what cs_mappoint_culling reads)
inline bool covis_points_ok(const covis_table *t) { return t && t->n_kf >= 0 && t->n_points >= 0 && (t->n_points == 0 || (t->mp_nobs && t->mp_flags)); }
// the whole table: offsets, every key-frame index inside the key-frame table, every run strictly ascending
inline bool covis_table_ok(const covis_table *t) {
    if (!covis_points_ok(t) || !covis_offsets_ok(t->obs_off, t->n_points)) return false;
    const int n = t->obs_off[t->n_points];
    if (n && (!t->obs_kf || !t->obs_octave || !t->obs_stereo)) return false;
    for (int p = 0; p < t->n_points; p++)
        for (int e = t->obs_off[p]; e < t->obs_off[p + 1]; e++) {
            if (t->obs_kf[e] < 0 || t->obs_kf[e] >= t->n_kf) return false;
            if (e > t->obs_off[p] && t->obs_kf[e] <= t->obs_kf[e - 1]) return false;
        }
    return true;
}
// n lists of map-point slots: kf[i] inside the key-frame table, every slot -1 or inside the point table
inline bool covis_lists_ok(const covis_table *t, int n, const int *kf, const int *kf_off, const int *kf_mp) {
    if (n < 0 || (n && !kf) || !covis_offsets_ok(kf_off, n) || (kf_off[n] && !kf_mp)) return false;
    for (int i = 0; i < n; i++) if (kf[i] < 0 || kf[i] >= t->n_kf) return false;
    for (int s = 0; s < kf_off[n]; s++) if (kf_mp[s] < -1 || kf_mp[s] >= t->n_points) return false;
    return true;
}

// ---- KeyFrame::UpdateConnections ---------------------------------------------------------------------------------------------------------------------------------------------
inline int covis_update_host(const covis_table *t, int n_query, const int *query_kf, const int *kf_off, const int *kf_mp, int skip_dynamic, int th, int conn_cap, int *cnt_off,
                             int *cnt_kf, int *cnt_w, int *kf_max, int *w_max, int *ord_off, int *ord_kf, int *ord_w) {
    if (!covis_table_ok(t) || !covis_lists_ok(t, n_query, query_kf, kf_off, kf_mp) || conn_cap < 0 || !cnt_off || !ord_off || (n_query && (!kf_max || !w_max)) ||
        (conn_cap && (!cnt_kf || !cnt_w || !ord_kf || !ord_w)))
        return -2;
    std::vector<int> counter((size_t)t->n_kf, 0), all_kf, all_w;
    cnt_off[0] = 0;
    bool fits = true;
    for (int q = 0; q < n_query; q++) {
        std::fill(counter.begin(), counter.end(), 0);
        for (int s = kf_off[q]; s < kf_off[q + 1]; s++) {
            const int p = kf_mp[s];
            if (covis_vote_skips(p, t->mp_flags, skip_dynamic)) continue;
            for (int e = t->obs_off[p]; e < t->obs_off[p + 1]; e++)
                if (t->obs_kf[e] != query_kf[q]) counter[(size_t)t->obs_kf[e]]++;
        }
        int n = 0;
        for (int k = 0; k < t->n_kf; k++) if (counter[(size_t)k]) { all_kf.push_back(k); all_w.push_back(counter[(size_t)k]); n++; }
        if ((long long)cnt_off[q] + n > 0x7fffffffLL) return -4;
        cnt_off[q + 1] = cnt_off[q] + n;
        fits = fits && cnt_off[q + 1] <= conn_cap;
    }
    if (!fits) return -4;
    ord_off[0] = 0;
    for (int q = 0; q < n_query; q++) {
        unsigned long long best = 0;
        bool any = false;
        int o = ord_off[q];
        for (int i = cnt_off[q]; i < cnt_off[q + 1]; i++) {
            cnt_kf[i] = all_kf[(size_t)i]; cnt_w[i] = all_w[(size_t)i];
            const unsigned long long key = covis_max_key(cnt_w[i], cnt_kf[i]);
            if (!any || key > best) { best = key; any = true; }
            if (cnt_w[i] >= th) { ord_kf[o] = cnt_kf[i]; ord_w[o] = cnt_w[i]; o++; }
        }
        kf_max[q] = any ? covis_key_kf(best) : -1;
        w_max[q] = any ? covis_key_w(best) : 0;
        if (any && o == ord_off[q]) { ord_kf[o] = kf_max[q]; ord_w[o] = w_max[q]; o++; }
        // the order by the same comparison the device ranks with (insertion: the lists are short)
        for (int i = ord_off[q] + 1; i < o; i++) {
            const int w = ord_w[i], k = ord_kf[i];
            int j = i;
            for (; j > ord_off[q] && covis_ordered_before(w, k, ord_w[j - 1], ord_kf[j - 1]); j--) { ord_w[j] = ord_w[j - 1]; ord_kf[j] = ord_kf[j - 1]; }
            ord_w[j] = w; ord_kf[j] = k;
        }
        ord_off[q + 1] = o;
    }
    return 0;
}

// ---- LocalMapping::KeyFrameCulling -------------------------------------------------------------------------------------------------------------------------------------------
inline bool covis_culling_args_ok(const covis_table *t, int n_local, const int *local_kf, const int *kf_off, const int *kf_mp, const int *slot_octave, const float *slot_depth,
                                  const float *kf_th_depth, const uint8_t *kf_flags, const uint8_t *verdict, const int *n_mps, const int *n_redundant, const int *out_nobs,
                                  const uint8_t *out_flags, const uint8_t *out_alive) {
    if (!covis_table_ok(t) || !covis_lists_ok(t, n_local, local_kf, kf_off, kf_mp)) return false;
    if (kf_off[n_local] && (!slot_octave || !slot_depth)) return false;
    if (n_local && (!kf_th_depth || !kf_flags || !verdict || !n_mps || !n_redundant)) return false;
    if (t->n_points && (!out_nobs || !out_flags)) return false;
    return !(t->obs_off[t->n_points] && !out_alive);
}
// the state the loop starts on
inline void covis_culling_init(const covis_table *t, int *nobs, uint8_t *flags, uint8_t *alive) {
    if (t->n_points) { memcpy(nobs, t->mp_nobs, sizeof(int) * (size_t)t->n_points); memcpy(flags, t->mp_flags, (size_t)t->n_points); }
    for (int p = 0; p < t->n_points; p++)
        for (int e = t->obs_off[p]; e < t->obs_off[p + 1]; e++) alive[e] = !(t->mp_flags[p] & COVIS_MP_BAD);
}
inline int covis_keyframe_culling_host(const covis_table *t, int n_local, const int *local_kf, const int *kf_off, const int *kf_mp, const int *slot_octave,
                                       const float *slot_depth, const float *kf_th_depth, int monocular, const uint8_t *kf_flags, int th_obs, uint8_t *verdict, int *n_mps,
                                       int *n_redundant, int *out_nobs, uint8_t *out_flags, uint8_t *out_alive, int *n_rounds) {
    if (!covis_culling_args_ok(t, n_local, local_kf, kf_off, kf_mp, slot_octave, slot_depth, kf_th_depth, kf_flags, verdict, n_mps, n_redundant, out_nobs, out_flags, out_alive))
        return -2;
    covis_culling_init(t, out_nobs, out_flags, out_alive);
    for (int i = 0; i < n_local; i++) {
        const int kf = local_kf[i];
        int mps = 0, red = 0;
        if (!(kf_flags[i] & COVIS_KF_ID0))
            for (int s = kf_off[i]; s < kf_off[i + 1]; s++) {
                const int p = kf_mp[s];
                if (covis_cull_skips(p, out_flags, monocular, slot_depth[s], kf_th_depth[i])) continue;
                mps++;
                red += covis_cull_redundant(p, kf, slot_octave[s], th_obs, out_nobs, t->obs_off, t->obs_kf, t->obs_octave, out_alive);
            }
        verdict[i] = covis_cull_verdict(red, mps, kf_flags[i]);
        n_mps[i] = mps; n_redundant[i] = red;
        if (verdict[i] != COVIS_CULLED) continue;
        for (int s = kf_off[i]; s < kf_off[i + 1]; s++) { // KeyFrame::SetBadFlag :526-528
            const int p = kf_mp[s];
            if (p < 0) continue;
            const int e = covis_find_entry(p, kf, t->obs_off, t->obs_kf);
            if (e < 0 || !out_alive[e]) continue; // mObservations.count(pKF) == 0
            out_alive[e] = 0;
            out_nobs[p] -= covis_erase_step(t->obs_stereo[e]);
            if (covis_erase_turns_bad(out_nobs[p])) {
                out_flags[p] |= COVIS_MP_BAD;
                for (int k = t->obs_off[p]; k < t->obs_off[p + 1]; k++) out_alive[k] = 0;
            }
        }
    }
    if (n_rounds) *n_rounds = 1;
    return 0;
}

// ---- LocalMapping::MapPointCulling -------------------------------------------------------------------------------------------------------------------------------------------
inline bool covis_mappoint_args_ok(const covis_table *t, int n_recent, const int *recent, const int *mp_found, const int *mp_visible, const int *mp_first_kf_id,
                                   const uint8_t *cases) {
    if (!covis_points_ok(t) || n_recent < 0) return false;
    if (n_recent && (!recent || !mp_found || !mp_visible || !mp_first_kf_id || !cases)) return false;
    for (int i = 0; i < n_recent; i++) if (recent[i] < 0 || recent[i] >= t->n_points) return false;
    return true;
}
inline int covis_mappoint_culling_host(const covis_table *t, int n_recent, const int *recent, const int *mp_found, const int *mp_visible, const int *mp_first_kf_id,
                                       int current_kf_id, int th_obs, uint8_t *cases) {
    if (!covis_mappoint_args_ok(t, n_recent, recent, mp_found, mp_visible, mp_first_kf_id, cases)) return -2;
    for (int i = 0; i < n_recent; i++) {
        const int p = recent[i];
        cases[i] = covis_mappoint_case(t->mp_flags[p], mp_found[p], mp_visible[p], t->mp_nobs[p], mp_first_kf_id[p], current_kf_id, th_obs);
    }
    return 0;
}
