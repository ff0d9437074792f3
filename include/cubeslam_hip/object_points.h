/* cubeslam_hip/object_points.h -- extension of cubeslam_hip.h: the two ways the reference makes point coordinates out of cuboids.
 *   cs_triangulate_dynamic_points   the triangulation of every not-yet-triangulated dynamic point against the last key frame with the object's own motion folded into the
 *                                   second camera (Tracking::CreateNewKeyFrame, orb_object_slam/src/Tracking.cc:2144-2244): x3D and MapPoint::PosToObj, the dpoints of cs_ba_dyn_*
 *   cs_object_depth_points          the object-depth initialisation: Tracking::MonoObjDepthInitialization (Tracking.cc:876-898), the grid-gated branch of CreateNewKeyFrame
 *                                   (:2339-2424) and the tail of LocalMapping::CreateNewMapPoints (LocalMapping.cc:574-652)
 * Both take host pointers, many key frames per call, and wait once.  ctx == NULL runs the same statements (csrc/object_points_math.h) on the host: the comparison side.
 * The main header is unchanged by this file: CS_VERSION and the ABI of its functions stay, this header has a version of its own. */
#ifndef CUBESLAM_HIP_OBJECT_POINTS_H
#define CUBESLAM_HIP_OBJECT_POINTS_H

#include "../cubeslam_hip.h"

#define CS_OBJECT_POINTS_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

/* CS_OBJECT_POINTS_VERSION of the library that is loaded */
int cs_object_points_version(void);

/* status byte of a dynamic point: 0 triangulated, otherwise the first test that failed, in the reference's order */
#define CS_DYN_TRIANGULATED 0
#define CS_DYN_NO_OBSERVATION 1 /* :2167 pixelindLastKf == -1 */
#define CS_DYN_TRACKLET 2       /* :2191 truth_tracklet_id of the two objects differs */
#define CS_DYN_W_ZERO 3         /* :2228 */
#define CS_DYN_TOO_FAR 4        /* :2235 farther than 5 from the point's current position */

/* Tracking.cc:2158-2243 for n_pairs key-frame pairs (last key frame, current key frame); pair f has the points first[f] .. first[f + 1].
 * Per pair: Tcw_last / Tcw_now = 12 floats each (rows of [Rcw | tcw] of mpLastKeyFrame->GetPose() / mpCurrentKeyFrame->GetPose()), K4 = fx fy cx cy of the current key
 * frame (4 floats per pair), and two cuboid tables of 7 doubles a row (t, qx qy qz qw): cub_pose_last[cub_first_last[f] + row] = the pose the caller resolved at
 * :2178-2181 (allDynamicPoses[mpLastKeyFrame].first or GetWorldPos()) for local_cuboids[row] of the last key frame, cub_pose_now[cub_first_now[f] + row] = GetWorldPos() of
 * local_cuboids[row] of the current one.  tracklet_last / tracklet_now: truth_tracklet_id per row of the two tables; both NULL = use_truth_trackid is false.
 * Per point: kp1 / kp2 = pt of the key point in the last / current key frame (2 floats; mvKeysHarris or mvKeysUn, the caller's use_dynamic_klt_features), obj_last /
 * obj_now = the object's row in its pair's tables, idx_last = pixelindLastKf (-1: no observation; the rows of such a point are not read), world_pos = GetWorldPosVec().
 * Outputs per point: status, x3D (3 floats), pos_to_obj (3 floats, PosToObj as the reference stores it) and dpoints (the same 3 values as doubles, the layout
 * cs_ba_dyn_problem reads); zeros where the status is not 0.
 * Stated definitions: cv::SVD::compute is the fixed-order Jacobi of cs_create_new_map_points and x3D / w is float(x_k * (1.0 / w)); the norm of
 * :2235 is sqrt(d0 * d0 + (d1 * d1 + d2 * d2)) in float.
 * CS_ERR_BAD_ARG, nothing launched and nothing written: a NULL argument, offsets that do not start at 0 or that decrease, one tracklet table without the other, an object
 * row outside its pair's table (of a point with idx_last != -1), idx_last < -1, a key point that is not finite. */
int cs_triangulate_dynamic_points(cs_ctx *ctx, int n_pairs, const int *first, const float *Tcw_last, const float *Tcw_now, const float *K4, const int *cub_first_last,
                                  const double *cub_pose_last, const int *cub_first_now, const double *cub_pose_now, const int *tracklet_last, const int *tracklet_now,
                                  const float *kp1, const float *kp2, const int *obj_last, const int *obj_now, const int *idx_last, const float *world_pos, uint8_t *status,
                                  float *x3D, float *pos_to_obj, double *dpoints);

#define CS_OBJECT_DEPTH_FIRST_FRAME 0   /* Tracking.cc:876-898, Frame::UnprojectDepth: keys = mvKeysUn */
#define CS_OBJECT_DEPTH_TRACKING 1      /* Tracking.cc:2339-2424, KeyFrame::UnprojectDepth: keys = mvKeys */
#define CS_OBJECT_DEPTH_LOCAL_MAPPING 2 /* LocalMapping.cc:574-652, KeyFrame::UnprojectDepth: keys = mvKeys */

/* The object-depth initialisation for n_frames key frames; frame f has the key points first[f] .. first[f + 1] (at most CS_RGBD_MAX_KEYPOINTS).
 * Per key point: keys, has_map_point = the reference's pMP != NULL (NULL in the first-frame mode, which does not read it), object_id = keypoint_associate_objectID.
 * Per frame: cuboid_depth[cub_first[f] + id] = (float)local_cuboids[id]->cube_meas.translation()[2]; K4 = fx fy cx cy (4 floats per frame); bounds = mnMinX mnMaxX mnMinY
 * mnMaxY (4 floats per frame, cs_frame_image_bounds; read by the tracking mode only, NULL elsewhere; KeyFrame::PosInGrid subtracts KeyFrame's `const int` mnMinX / mnMinY, i.e.
 * the truncated values, and multiplies by Frame's mfGridElementWidthInv / HeightInv, which come from the floats); Twc = 12 floats (rows of [Rwc | Ow]); draws[draw_first[f] ..
 * draw_first[f + 1]] = the values the caller's rand() returned, in call order (each >= 0; the first-frame mode takes none and both may be NULL there).
 *   first frame     every key point with object_id > -1 is a candidate, in index order; the points are those whose cuboid depth is > 0.  raw_depth_pts = 0 and
 *                   max_initialize_pts = n_candidates.
 *   tracking        candidates = has_object_depth_pixel_inds under the gridsHasMappt gate: the first index per cell that has no map point, lies inside the grid, has an object
 *                   and octave < 3.  raw_depth_pts = key points with a map point.  max_initialize_pts = min(min(int(total * 0.30) - int(raw), candidates), 80) in the
 *                   reference's double and int arithmetic, or -1 when raw / total < 0.30 is false (nothing is drawn or created then).  random_unique2 consumes exactly
 *                   max_initialize_pts draws as draw % left; the walk of :2390-2420 goes on past max_initialize_pts into the unshuffled remainder while cuboids of
 *                   depth <= 0 are skipped.
 *   local mapping   the same without the grid gate, the octave test and the 80.
 * Outputs per frame: n_candidates, raw_depth_pts, max_initialize_pts; candidates / shuffled at cand_first[f] .. cand_first[f + 1] (the list before and after the draws;
 * room for first[n_frames] ints each); new_idx at new_first[f] .. new_first[f + 1] in creation order (the order of MapPoint::mnId and of mlpRecentAddedMapPoints) with
 * new_x3D (3 floats; room for first[n_frames] entries).
 * CS_ERR_BAD_ARG, nothing written: a NULL argument, an unknown mode, offsets that do not start at 0 or that decrease, a frame with more than CS_RGBD_MAX_KEYPOINTS key
 * points, an object id at or beyond the frame's cuboid count (the reference indexes local_cuboids out of bounds), a negative draw, fewer draws than max_initialize_pts
 * for a frame, image bounds (tracking mode) that are not finite, beyond 1e9 or empty. */
int cs_object_depth_points(cs_ctx *ctx, int mode, int n_frames, const int *first, const cs_keypoint *keys, const uint8_t *has_map_point, const int *object_id,
                           const int *cub_first, const float *cuboid_depth, const float *K4, const float *bounds, const float *Twc, const int *draw_first, const int *draws,
                           int *n_candidates, int *raw_depth_pts, int *max_initialize_pts, int *cand_first, int *candidates, int *shuffled, int *new_first, int *new_idx,
                           float *new_x3D);

#ifdef __cplusplus
}
#endif
#endif
