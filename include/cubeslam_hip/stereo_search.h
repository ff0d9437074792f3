/* cubeslam_hip/stereo_search.h -- extension of cubeslam_hip.h: the stereo / RGB-D branches of both ORBmatcher::SearchByProjection overloads that track a frame.
 *   cs_matcher_set_u_right                 CurrentFrame.mvuRight for the searches below
 *   cs_match_by_projection_frame_stereo    SearchByProjection(CurrentFrame, LastFrame, th, bMono = false) (ORBmatcher.cc:1373-1522), one pair
 *   cs_match_by_projection_stream_stereo   the same for every pair of a window the extractor holds in HBM
 *   cs_match_local_map_stereo              SearchByProjection(F, vpMapPoints, th) (:50-142) with the mvuRight test of :104-109
 *   cs_match_local_map_frustum_stereo      Tracking::SearchLocalPoints in one call, with that test
 * Each takes the arguments of the entry of cubeslam_hip.h it is named after, which stays the monocular search (mvuRight < 0), and more behind them.  What the stereo branch adds:
 *   direction (:1383-1394)   twc = -Rcw.t() * tcw, tlc = Rlw * twc + tlw; forward when tlc.z > mb, backward when -tlc.z > mb, both strict float comparisons.  A cv::Mat product is
 *                            one gemm per row, accumulated in double with k ascending and rounded once: twc[r] = (float)(-sum_k Rcw[k][r] tcw[k]),
 *                            tlc.z = (float)(sum_k Rlw[2][k] twc[k] + tlw[2]).
 *   level window (:1433-1438) of a last-frame key point of level o: forward (o, -1) -- with o == 0 no level check at all (Frame.cc:404-459, bCheckLevels) --, backward (0, o),
 *                            otherwise (o - 1, o + 1).
 *   the mvuRight test        (:1459-1465) ur = u - mbf * invzc in float; a candidate i2 with mvuRight[i2] > 0 and fabs(ur - mvuRight[i2]) > radius is dropped.  (:104-109) the same with
 *                            ur = mTrackProjXR and radius = r * mvScaleFactors[nPredictedLevel], the float the window was opened with.  The comparison with 0 is strict: a right
 *                            coordinate of exactly 0 is not tested (Fuse tests >= 0).
 * The test runs where the candidates are enumerated, ahead of their Hamming distances; cs_matcher_last_counts / cs_match_stream_last_counts after one of these searches count the
 * candidates AFTER the test.
 * The main header is unchanged by this file: CS_VERSION and the ABI of its functions stay, this header has a version of its own. */
#ifndef CUBESLAM_HIP_STEREO_SEARCH_H
#define CUBESLAM_HIP_STEREO_SEARCH_H

#include "../cubeslam_hip.h"

#define CS_STEREO_SEARCH_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

/* CS_STEREO_SEARCH_VERSION of the library that is loaded */
int cs_stereo_search_version(void);

/* CurrentFrame.mvuRight (Frame.h: -1 for a key point without a right coordinate) for the frame the matcher holds; n must be that frame's N, otherwise CS_ERR_BAD_ARG (also
 * for a matcher without a frame).  on_device != 0: u_right is a device pointer, such as cs_stereo_device_pair and cs_rgbd_device_frame hand out; it is copied device to device by
 * work queued on the context's stream, without a host round trip and without a wait, and must stay valid until the next call that waits for that stream (every search does, and
 * cs_sync).  A host pointer is read before the call returns.  Any later cs_matcher_set_frame* detaches it. */
int cs_matcher_set_u_right(cs_ctx *ctx, cs_matcher *m, const float *u_right, int n, int on_device);

/* ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1373-1522): cs_match_by_projection_frame's arguments, then Tlw = LastFrame.mTcw (3x4 row-major),
 * bf = CurrentFrame.mbf, mb = CurrentFrame.mb, mono = bMono.  *direction (nullable): 0 neither, 1 forward, 2 backward (:1393-1394).
 * mono != 0: needs no u_right and no Tlw, and is cs_match_by_projection_frame byte for byte (a monocular frame has no right coordinates).  mono == 0 without u_right set:
 * CS_ERR_BAD_ARG.  NULL or out-of-range arguments: CS_ERR_BAD_ARG before anything is queued; CS_ERR_CAPACITY (the candidate arena) leaves the matcher usable. */
int cs_match_by_projection_frame_stereo(cs_ctx *ctx, cs_matcher *m, int n_last, const float *world_pos, const uint8_t *valid, const uint8_t *blocks, const uint8_t *mp_desc,
                                        const int *last_octave, const float *last_angle, const float *Tcw, float fx, float fy, float cx, float cy, const float *scale_factors,
                                        int n_levels, float th, int check_orientation, const uint8_t *train_blocked /* nullable */, int *train_match, int *nmatches, const float *Tlw,
                                        float bf, float mb, int mono, int *direction /* nullable */);

/* The same search (:1373-1522) for the pairs (f0 + p, f0 + p + 1) of a window: cs_match_by_projection_stream's arguments, then Tlw (12 floats per pair: the last frame's pose),
 * u_right (mvuRight packed over the current frames f0 + 1 .. f0 + n_pairs, n_train values, in train_match's order; a device pointer with u_right_on_device != 0, under
 * cs_matcher_set_u_right's rule), bf, mb, mono.  Each pair takes its own direction: direction[n_pairs], nullable.  Results equal the per-frame calls'.  mono != 0 is
 * cs_match_by_projection_stream byte for byte. */
int cs_match_by_projection_stream_stereo(cs_ctx *ctx, cs_match_stream *m, const cs_orb *orb, int f0, int n_pairs, const float *K4, const float *dist5 /* nullable */, float minX,
                                         float maxX, float minY, float maxY, int n_queries, int n_train, const float *world_pos, const uint8_t *valid, const uint8_t *blocks,
                                         const uint8_t *mp_desc /* nullable */, const float *Tcw, float fx, float fy, float cx, float cy, const float *scale_factors, int n_levels,
                                         float th, int check_orientation, int *train_match, int *nmatches, const float *Tlw, const float *u_right, int u_right_on_device, float bf,
                                         float mb, int mono, int *direction /* [n_pairs], nullable */);

/* ORBmatcher::SearchByProjection(F, vpMapPoints, th) (:50-142) with the test of :104-109: cs_match_local_map's arguments, then proj_xr = mTrackProjXR per map point.  Needs u_right
 * set (CS_ERR_BAD_ARG otherwise). */
int cs_match_local_map_stereo(cs_ctx *ctx, cs_matcher *m, int n_mp, const float *proj_xy, const float *view_cos, const int *pred_level, const uint8_t *in_view, const uint8_t *blocks,
                              const uint8_t *mp_desc, const float *scale_factors, int n_levels, float th, float nnratio, const uint8_t *train_blocked /* nullable */, int *train_match,
                              int *nmatches, const float *proj_xr);

/* Tracking::SearchLocalPoints (Tracking.cc:2673-2728) with the test of ORBmatcher.cc:104-109: exactly cs_match_local_map_frustum's arguments.  The uR = u - bf * invz that
 * Frame::isInFrustum leaves on a point (Frame.cc:396, returned in proj) is what the test compares.  Needs u_right set (CS_ERR_BAD_ARG otherwise). */
int cs_match_local_map_frustum_stereo(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal,
                                      const float *min_distance, const float *max_distance, const uint8_t *skip, const uint8_t *blocks, const uint8_t *mp_desc,
                                      const uint8_t *train_blocked /* nullable */, float fx, float fy, float cx, float cy, float bf, float log_scale_factor, const float *scale_factors,
                                      int n_levels, float viewing_cos_limit, float th, float nnratio, int *train_match, int *nmatches, int *n_to_match,
                                      int *n_level_outside /* nullable */, uint8_t *in_view, float *proj /* nullable */, int *pred_level /* nullable */, float *view_cos /* nullable */);

#ifdef __cplusplus
}
#endif
#endif
