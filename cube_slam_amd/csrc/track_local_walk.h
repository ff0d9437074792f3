// track_local_walk.h -- Tracking::UpdateLocalKeyFrames (orb_object_slam/src/Tracking.cc:2766-2874) over flat arrays: the votes of the frame's map points for the key frames that
// observe them and the expansion loop with its quirks.  Host only, no arithmetic; one place for cs_track_local_keyframes (tracklocal.hip) and for cubeslam::Tracking with or
// without the library (host/tracking.hpp).
//
// The reference counts the votes in a std::map<KeyFrame *, int> and walks it in pointer order, which a run does not reproduce.  That order is DEFINED here as ascending index in
// the caller's key-frame table; the children of a key frame (a std::set<KeyFrame *>) are walked in the order the caller lists them, which the same definition makes ascending.
#pragma once
#include <cstdint>
#include <vector>

// frame_mp[n_frame]: the frame's map point per key point, an index into the point table or -1.  mp_skip[n_points]: isBad, or is_dynamic under whether_dynamic_object (:2775-2778;
// setting a bad point's slot to NULL, :2785, stays with the caller).  obs_off / obs_kf: per point the key frames of GetObservations().  kf_bad[n_kf] = isBad.  cov_off / cov_kf:
// per key frame its covisible key frames by descending weight (mvpOrderedConnectedKeyFrames); the first ten are GetBestCovisibilityKeyFrames(10).  child_off / child_kf: GetChilds().
// parent[n_kf]: GetParent() or -1.
// Returns the number of local key frames written to local_kf (room for n_kf), -1 when no key frame received a vote (the reference returns at :2790-2791 and the caller keeps its
// lists), -2 for an index outside its table.  *kf_max: pKFmax or -1 (:2869: the reference key frame changes only when it is set).
inline int track_local_keyframes(int n_frame, const int *frame_mp, int n_points, const uint8_t *mp_skip, const int *obs_off, const int *obs_kf, int n_kf, const uint8_t *kf_bad,
                                 const int *cov_off, const int *cov_kf, const int *child_off, const int *child_kf, const int *parent, int *local_kf, int *kf_max) {
    *kf_max = -1;
    std::vector<int> counter((size_t)n_kf, 0); // keyframeCounter: an entry exists where the count is positive
    int n_voters = 0;
    for (int i = 0; i < n_frame; i++) { // :2770-2788
        const int mp = frame_mp[i];
        if (mp < 0) continue;
        if (mp >= n_points) return -2;
        if (mp_skip[mp]) continue;
        for (int o = obs_off[mp]; o < obs_off[mp + 1]; o++) {
            const int kf = obs_kf[o];
            if (kf < 0 || kf >= n_kf) return -2;
            if (counter[kf]++ == 0) n_voters++;
        }
    }
    if (n_voters == 0) return -1; // :2790
    int max = 0, n = 0;
    std::vector<char> mark((size_t)n_kf, 0); // mnTrackReferenceForFrame == mCurrentFrame.mnId
    for (int kf = 0; kf < n_kf; kf++) { // :2800-2815, the map's order
        if (counter[kf] == 0) continue;
        if (kf_bad[kf]) continue;
        if (counter[kf] > max) { max = counter[kf]; *kf_max = kf; } // the first strict maximum
        local_kf[n++] = kf;
        mark[kf] = 1;
    }
    const int n_end = n; // :2818: the end iterator is taken before the pushes -- only the voters are walked
    for (int it = 0; it < n_end; it++) {
        if (n > 80) break; // :2821
        const int kf = local_kf[it];
        const int c_end = cov_off[kf] + 10 < cov_off[kf + 1] ? cov_off[kf] + 10 : cov_off[kf + 1];
        for (int c = cov_off[kf]; c < c_end; c++) { // :2826-2840: at most one neighbour
            const int nb = cov_kf[c];
            if (nb < 0 || nb >= n_kf) return -2;
            if (!kf_bad[nb] && !mark[nb]) { local_kf[n++] = nb; mark[nb] = 1; break; }
        }
        for (int c = child_off[kf]; c < child_off[kf + 1]; c++) { // :2842-2855: at most one child
            const int ch = child_kf[c];
            if (ch < 0 || ch >= n_kf) return -2;
            if (!kf_bad[ch] && !mark[ch]) { local_kf[n++] = ch; mark[ch] = 1; break; }
        }
        const int pa = parent[kf]; // :2857-2866: isBad is not asked, and the break leaves the OUTER loop -- the first new parent ends the expansion
        if (pa >= n_kf) return -2;
        if (pa >= 0 && !mark[pa]) { local_kf[n++] = pa; mark[pa] = 1; break; }
    }
    return n;
}
