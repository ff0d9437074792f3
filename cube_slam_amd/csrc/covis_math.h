// covis_math.h -- the predicates and the arithmetic of KeyFrame::UpdateConnections (KeyFrame.cc:345-437), LocalMapping::KeyFrameCulling (LocalMapping.cc:833-902) with
// MapPoint::EraseObservation (MapPoint.cc:178-205), and LocalMapping::MapPointCulling (LocalMapping.cc:249-302): one text for the kernels of covisibility.hip and for the host
// forms (covis_walk.h).  Plain C++ under g++ (tests/cpp/covisibility_driver.cpp).
#pragma once
#include <cstdint>

#include "hd.h"

constexpr int COVIS_COUNTER_TILE = 4096; // key-frame indices whose counters one sweep of the vote holds in LDS (16 KiB); n_kf above it takes several sweeps
constexpr uint8_t COVIS_MP_BAD = 1, COVIS_MP_DYNAMIC = 2;    // mp_flags
constexpr uint8_t COVIS_KF_ID0 = 1, COVIS_KF_NOT_ERASE = 2;  // kf_flags
enum : uint8_t { COVIS_KEPT = 0, COVIS_CULLED = 1, COVIS_TO_BE_ERASED = 2, COVIS_SKIPPED = 3 };

// UpdateConnections :363-370: the slot's point does not vote
HD bool covis_vote_skips(int point, const uint8_t *mp_flags, int skip_dynamic) {
    if (point < 0) return true;
    const uint8_t f = mp_flags[point];
    return (f & COVIS_MP_BAD) || (skip_dynamic && (f & COVIS_MP_DYNAMIC));
}
// :395 over an ascending walk: (w, kf) replaces the best so far only with a strictly larger count.  As one key whose maximum is the answer: count first, then the LOWER index
HD unsigned long long covis_max_key(int w, int kf) { return ((unsigned long long)(unsigned)w << 32) | (unsigned)(0x7fffffff - kf); }
HD int covis_key_w(unsigned long long key) { return (int)(key >> 32); }
HD int covis_key_kf(unsigned long long key) { return 0x7fffffff - (int)(key & 0xffffffffu); }
// mvpOrderedConnectedKeyFrames: sort ascending on (weight, pointer), then push_front -- a stands in front of b
HD bool covis_ordered_before(int wa, int kfa, int wb, int kfb) { return wa > wb || (wa == wb && kfa > kfb); }

// KeyFrameCulling :857-868: the slot does not count into nMPs (bad, far or invalid depth of a stereo / RGB-D key frame, dynamic)
HD bool covis_cull_skips(int point, const uint8_t *flags, int monocular, float depth, float th_depth) {
    if (point < 0) return true;
    if (flags[point] & COVIS_MP_BAD) return true;
    if (!monocular && (depth > th_depth || depth < 0)) return true;
    return (flags[point] & COVIS_MP_DYNAMIC) != 0;
}
// :871-894 for a slot that counts: nObs > thObs and at least thObs alive observations of other key frames at the same or a finer scale (+1).  The reference's early break
// does not change the comparison.
HD bool covis_cull_redundant(int point, int kf, int slot_octave, int th_obs, const int *nobs, const int *obs_off, const int *obs_kf, const int *obs_octave, const uint8_t *alive) {
    if (!(nobs[point] > th_obs)) return false;
    int n = 0;
    for (int e = obs_off[point]; e < obs_off[point + 1]; e++)
        if (alive[e] && obs_kf[e] != kf && obs_octave[e] <= slot_octave + 1) n++;
    return n >= th_obs;
}
// :898 with the two early ways out of KeyFrame::SetBadFlag (:513-521)
HD uint8_t covis_cull_verdict(int n_redundant, int n_mps, uint8_t kf_flags) {
    if (kf_flags & COVIS_KF_ID0) return COVIS_SKIPPED;
    if (!((double)n_redundant > 0.9 * (double)n_mps)) return COVIS_KEPT;
    return (kf_flags & COVIS_KF_NOT_ERASE) ? COVIS_TO_BE_ERASED : COVIS_CULLED;
}
// the entry of `kf` in the point's run, -1 none (the run is strictly ascending)
HD int covis_find_entry(int point, int kf, const int *obs_off, const int *obs_kf) {
    int lo = obs_off[point], hi = obs_off[point + 1];
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (obs_kf[mid] < kf) lo = mid + 1; else hi = mid;
    }
    return lo < obs_off[point + 1] && obs_kf[lo] == kf ? lo : -1;
}
// EraseObservation :186-189
HD int covis_erase_step(uint8_t stereo) { return stereo ? 2 : 1; }
HD bool covis_erase_turns_bad(int nobs) { return nobs <= 2; } // :197

// MapPointCulling :275-299
HD uint8_t covis_mappoint_case(uint8_t flags, int found, int visible, int nobs, int first_kf_id, int current_kf_id, int th_obs) {
    if (flags & (COVIS_MP_BAD | COVIS_MP_DYNAMIC)) return 1;
    if ((float)found / (float)visible < 0.25f) return 2; // GetFoundRatio: static_cast<float>(mnFound) / mnVisible
    if (current_kf_id - first_kf_id >= 2 && nobs <= th_obs) return 3;
    if (current_kf_id - first_kf_id >= 3) return 4;
    return 0;
}
