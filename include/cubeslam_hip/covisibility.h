/* cubeslam_hip/covisibility.h -- extension of cubeslam_hip.h: the graph work at both ends of LocalMapping::RunMappingIteration (LocalMapping.cc:79-149).
 *   cs_covisibility_update   KeyFrame::UpdateConnections (KeyFrame.cc:345-437) for a batch of key frames
 *   cs_keyframe_culling      LocalMapping::KeyFrameCulling (LocalMapping.cc:833-902) with the MapPoint::EraseObservation chain of every culled key frame
 *   cs_mappoint_culling      LocalMapping::MapPointCulling (LocalMapping.cc:249-302)
 * Each has a host form with the same arguments and no context (..._host), built from the same predicates (csrc/covis_math.h): one key frame's vote is
 * launch-latency-sized and the caller may choose.  Everything is integers; both forms give the same bytes.
 * The main header is unchanged by this file: CS_VERSION and the ABI of its functions stay, this header has a version of its own. */
#ifndef CUBESLAM_HIP_COVISIBILITY_H
#define CUBESLAM_HIP_COVISIBILITY_H

#include "../cubeslam_hip.h"

#define CS_COVISIBILITY_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

/* The observation side of the map, in the caller's memory.  Point p's mObservations are the entries obs_off[p] .. obs_off[p + 1]: obs_kf strictly ascending (the
 * reference's std::map<KeyFrame *, size_t> pointer order is defined as ascending index in the key-frame table, as for cs_track_local_keyframes), obs_octave =
 * pKFi->mvKeysUn[idx].octave and obs_stereo = pKFi->mvuRight[idx] >= 0 for the observation's own idx.  mp_nobs = MapPoint::nObs as the reference holds it: an input, not
 * derived from the runs (AddObservation and EraseObservation count a stereo observation differently under use_dynamic_klt_features, MapPoint.cc:144-152 against :186-189).
 * mp_flags: bit 0 isBad, bit 1 is_dynamic. */
typedef struct cs_obs_table {
    int n_kf, n_points;
    const int *obs_off;         /* [n_points + 1] */
    const int *obs_kf;          /* [obs_off[n_points]] */
    const int *obs_octave;      /* [obs_off[n_points]] */
    const uint8_t *obs_stereo;  /* [obs_off[n_points]] */
    const int *mp_nobs;         /* [n_points] */
    const uint8_t *mp_flags;    /* [n_points] */
} cs_obs_table;
#define CS_MP_BAD 1
#define CS_MP_DYNAMIC 2

/* CS_COVISIBILITY_VERSION of the library that is loaded */
int cs_covisibility_version(void);

/* KeyFrame::UpdateConnections for n_query key frames.  query_kf[q]: the key frame's index; kf_off[n_query + 1] / kf_mp: its GetMapPointMatches() as indices into the point table,
 * -1 no point.  Per query, every slot whose point is not skipped (-1, bad, dynamic when skip_dynamic = whether_dynamic_object) adds one to KFcounter[obs_kf] for every entry of the
 * point with obs_kf != query_kf[q]; a point held in two slots votes twice, as in the reference's walk over vpMP.  th = 15 in the reference.
 *   cnt_off[n_query + 1] / cnt_kf / cnt_w   KFcounter, ascending index
 *   kf_max[q] / w_max[q]                    pKFmax / nmax: the lowest index among the largest counts (:395 is a strict > over an ascending walk); -1 / 0: the counter is empty,
 *                                           the reference returns at :382 and the caller keeps its lists
 *   ord_off[n_query + 1] / ord_kf / ord_w   mvpOrderedConnectedKeyFrames / mvOrderedWeights: the pairs with weight >= th, or the pair (w_max, kf_max) when there is none; weight
 *                                           descending, ties by index descending (sort ascending on (weight, pointer), then push_front).  The same entries are the
 *                                           AddConnection(this, w) calls the reference makes on the other key frames.
 * cnt_kf, cnt_w, ord_kf, ord_w have room for conn_cap entries.  CS_ERR_CAPACITY: the counters need more; cnt_off is written all the same (the caller sizes its buffers with it),
 * nothing else is.  CS_ERR_BAD_ARG: a NULL, an index outside its table, offsets that decrease, a run that is not strictly ascending.  A query depends on the table alone, so the
 * batch is exact; no result depends on the order in which the device runs anything. */
int cs_covisibility_update(cs_ctx *ctx, const cs_obs_table *table, int n_query, const int *query_kf, const int *kf_off, const int *kf_mp, int skip_dynamic, int th, int conn_cap,
                           int *cnt_off, int *cnt_kf, int *cnt_w, int *kf_max, int *w_max, int *ord_off, int *ord_kf, int *ord_w);
int cs_covisibility_update_host(const cs_obs_table *table, int n_query, const int *query_kf, const int *kf_off, const int *kf_mp, int skip_dynamic, int th, int conn_cap,
                                int *cnt_off, int *cnt_kf, int *cnt_w, int *kf_max, int *w_max, int *ord_off, int *ord_kf, int *ord_w);

/* LocalMapping::KeyFrameCulling: the loop :841-901 over local_kf[n_local] (vpLocalKeyFrames as key-frame indices), exactly as a sequence.  kf_off[n_local + 1] / kf_mp: the
 * GetMapPointMatches() of each; slot_octave / slot_depth (per entry of kf_mp) = mvKeysUn[i].octave / mvDepth[i]; kf_th_depth[n_local] = mThDepth; monocular = mbMonocular;
 * kf_flags[n_local]: bit 0 mnId == 0, bit 1 mbNotErase; th_obs = 3 in the reference.
 * A slot counts into nMPs unless it is -1, its point is bad or dynamic, or (not monocular and depth > th or depth < 0).  It counts into nRedundant when nObs > th_obs and at least
 * th_obs alive observations of OTHER key frames have obs_octave <= slot_octave + 1.  The key frame goes when (double)nRedundant > 0.9 * (double)nMPs.
 *   verdict[n_local]   0 kept; 1 culled and erased; 2 over the threshold but mbNotErase (mbToBeErased only, no state changes, KeyFrame.cc:517-521); 3 mnId == 0, skipped
 *   n_mps / n_redundant [n_local]   the two counts as the key frame's turn found them (0 for verdict 3)
 * On verdict 1 (KeyFrame::SetBadFlag :511-529 -> MapPoint::EraseObservation, MapPoint.cc:178-205) every slot's point >= 0 loses its alive entry of this key frame, once:
 * nObs -= obs_stereo ? 2 : 1, and with nObs <= 2 the point turns bad and all its entries die (MapPoint::SetBadFlag).  Later key frames of the list count on that state.
 *   out_nobs[n_points], out_flags[n_points], out_alive[obs_off[n_points]]   the final nObs, point flags and one alive byte per observation entry.  The caller's tables are inputs
 *   and are not written.  The entries of a point that is bad on entry are not alive (its mObservations are empty in the reference).
 *   *n_rounds (nullable)   evaluation passes the device form took: culled key frames + 1, less one when the last of the list is culled (the host form reports 1).
 * With the caller stay the new mpRefKF of a point (its lowest alive index) and the connection and spanning-tree repair of KeyFrame::SetBadFlag :524-604. */
int cs_keyframe_culling(cs_ctx *ctx, const cs_obs_table *table, int n_local, const int *local_kf, const int *kf_off, const int *kf_mp, const int *slot_octave, const float *slot_depth,
                        const float *kf_th_depth, int monocular, const uint8_t *kf_flags, int th_obs, uint8_t *verdict, int *n_mps, int *n_redundant, int *out_nobs,
                        uint8_t *out_flags, uint8_t *out_alive, int *n_rounds);
int cs_keyframe_culling_host(const cs_obs_table *table, int n_local, const int *local_kf, const int *kf_off, const int *kf_mp, const int *slot_octave, const float *slot_depth,
                             const float *kf_th_depth, int monocular, const uint8_t *kf_flags, int th_obs, uint8_t *verdict, int *n_mps, int *n_redundant, int *out_nobs,
                             uint8_t *out_flags, uint8_t *out_alive, int *n_rounds);

/* LocalMapping::MapPointCulling :272-301 for mlpRecentAddedMapPoints = recent[n_recent] (indices into the point table; of the table only n_points, mp_nobs and mp_flags are read).
 * mp_found / mp_visible / mp_first_kf_id [n_points] = mnFound / mnVisible / mnFirstKFid; current_kf_id = mpCurrentKeyFrame->mnId; th_obs = cnThObs.
 * cases[n_recent]: 0 stays; 1 bad or dynamic (leaves the list); 2 float(found) / visible < 0.25f (SetBadFlag, leaves; computed in float, so visible == 0 gives inf or NaN and is
 * not case 2); 3 (current - first) >= 2 && nObs <= th_obs (SetBadFlag, leaves); 4 (current - first) >= 3 (leaves).  The first that applies wins; entries are independent. */
int cs_mappoint_culling(cs_ctx *ctx, const cs_obs_table *table, int n_recent, const int *recent, const int *mp_found, const int *mp_visible, const int *mp_first_kf_id,
                        int current_kf_id, int th_obs, uint8_t *cases);
int cs_mappoint_culling_host(const cs_obs_table *table, int n_recent, const int *recent, const int *mp_found, const int *mp_visible, const int *mp_first_kf_id,
                             int current_kf_id, int th_obs, uint8_t *cases);

#ifdef __cplusplus
}
#endif
#endif
