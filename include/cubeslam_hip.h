/*
 * cubeslam_hip.h -- C-ABI of libcubeslam_hip.so: MI355X (gfx950) kernels for CubeSLAM's per-frame hot path.
 *
 * Plain C, POD pointers and sizes only.  Every entry point cites the reference (shichaoy/cube_slam) interface
 * it replaces.  All functions return 0 (CS_OK) or a negative cs_status; they never throw and never fall back to
 * a CPU path: without a usable HIP device cs_create() fails with CS_ERR_NO_DEVICE.
 *
 * Threading: one cs_ctx per host thread / HIP stream (the reference objects are not re-entrant either:
 * detect_3d_cuboid.h:55-57 keeps cam_pose state, ORBextractor.h:85 keeps the pyramid).
 */
#ifndef CUBESLAM_HIP_H
#define CUBESLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CS_VERSION 108 /* 108: cs_stereo_* (Frame::ComputeStereoMatches on the extractor's resident buffers); 107: cs_match_by_projection_stream takes n_queries / n_train, cs_cuboid_batch_set_scene, the matchers' claim passes run on the device; 106: cs_cuboid_batch_n_frames, cs_frontend_queues, cs_match_by_projection_stream, cs_frontend_stream_*, cs_*_set_frames_device, cs_orb_read_packed; 105: cs_frontend_set_backlog; 104: cs_frontend_set_cuboid_ctx; 103: cs_lsd_read_filter_lines takes the caller's frame count, cs_frontend_set_chain; 102: cs_cuboid_batch_set_lines, cs_cuboid_batch_set_shared_gpu, cs_lsd_read_filter_lines; 101: cs_ba_set_stop_flag_bool / cs_ba_dyn_set_stop_flag_bool; cs_match_by_projection_frame takes train_blocked */

typedef enum cs_status {
    CS_OK = 0,
    CS_ERR_NO_DEVICE = -1,   /* no HIP device / runtime error at create */
    CS_ERR_BAD_ARG = -2,     /* null pointer, negative size, ROI outside image (cv::Rect assert in the reference) */
    CS_ERR_HIP = -3,         /* a HIP runtime call failed; see cs_last_error() */
    CS_ERR_CAPACITY = -4,    /* an internal fixed capacity was exceeded (e.g. > CS_MAX_ROI_LINES lines in one box) */
    CS_ERR_NOMEM = -5
} cs_status;

typedef struct cs_ctx cs_ctx;

/* Creates a context bound to HIP device `device_id` with its own stream. */
int cs_create(int device_id, cs_ctx **out);
/* Same with a stream priority: > 0 highest, < 0 lowest, 0 default.  The batch front-end runs ORB + cuboid (what the tracking thread waits
 * for) on a high-priority stream and the line detectors' device phases, which overlap their own host stage, on low-priority ones. */
int cs_create_with_priority(int device_id, int priority, cs_ctx **out);
void cs_destroy(cs_ctx *ctx);
const char *cs_last_error(const cs_ctx *ctx);

/* RCCL over xGMI inside the library (one process per GPU).  Rank 0 calls cs_comm_unique_id and hands the 128 bytes to the other ranks by
 * any out-of-band means (MPI, a socket, torch.distributed, a file); every rank then calls cs_comm_init on its context.  A sharded cs_ba
 * (world > 1) without a cs_ba_set_allreduce callback all-reduces the reduced camera system with ncclAllReduce(ncclDouble, ncclSum) on the
 * context's own stream: one fused buffer [36 * slots | 6 * P] per LM trial, no host synchronisation around it.  librccl.so is opened at
 * cs_comm_init (not a link-time dependency). */
#define CS_COMM_ID_BYTES 128
int cs_comm_unique_id(void *id128);
int cs_comm_init(cs_ctx *ctx, int rank, int world, const void *id128);
void cs_comm_destroy(cs_ctx *ctx);
/* ncclAllReduce(ncclDouble, ncclSum) in place over n doubles of device memory, enqueued on the context's stream (no synchronisation). */
int cs_comm_allreduce_f64(cs_ctx *ctx, double *device_buf, long n);
int cs_version(void);
/* Blocks until all work queued on the context's stream is done. */
int cs_sync(cs_ctx *ctx);
/* CPU threads the host stages use (affinity mask capped by the cgroup CPU quota; env CUBESLAM_HOST_THREADS overrides) */
int cs_host_thread_count(void);

/* Per-kernel hipEvent timing on the context's stream (replaces ca::Profiler::tictoc,
 * dependency/tictoc_profiler/src/profiler.cpp:40-67).  Disabled by default. */
int cs_timing_enable(cs_ctx *ctx, int on);
int cs_timing_reset(cs_ctx *ctx);
/* total milliseconds and launch count recorded for kernel `name` since the last reset; unknown name -> 0,0 */
int cs_timing_get(cs_ctx *ctx, const char *name, double *total_ms, long *count);

/* ===================================================================== detect_3d_cuboid
 * Replaces detect_3d_cuboid::detect_cuboid (detect_3d_cuboid/include/detect_3d_cuboid/detect_3d_cuboid.h:62-63,
 * detect_3d_cuboid/src/box_proposal_detail.cpp:56-557) and everything it calls in object_3d_util.cpp. */

#define CS_MAX_ROI_LINES 1024

typedef struct cs_cuboid_opts {          /* public members of class detect_3d_cuboid, detect_3d_cuboid.h:65-79 */
    int consider_config_1;
    int consider_config_2;
    int whether_sample_cam_roll_pitch;
    int whether_sample_bbox_height;
    int max_cuboid_num;
    double nominal_skew_ratio;
    double max_cut_skew;
    /* extensions; the defaults reproduce the constants hard-coded at box_proposal_detail.cpp:126-128,197 */
    double yaw_range_deg;                /* 45 */
    double yaw_step_deg;                 /* 6  */
    int canny_low;                       /* 80 */
    int canny_high;                      /* 200 */
} cs_cuboid_opts;

typedef struct cs_cuboid {               /* class cuboid, detect_3d_cuboid.h:15-36 */
    double pos[3];
    double scale[3];
    double rotY;
    double box_config_type[2];
    int32_t box_corners_2d[16];          /* 2x8 row-major */
    double box_corners_3d_world[24];     /* 3x8 row-major */
    double rect_detect_2d[4];
    double edge_distance_error;
    double edge_angle_error;
    double normalized_error;
    double skew_ratio;
    double down_expand_height;
    double camera_roll_delta;
    double camera_pitch_delta;
} cs_cuboid;

void cs_cuboid_default_opts(cs_cuboid_opts *opts);

/*
 * One frame, host buffers in / host buffers out (the drop-in call; H2D + kernels + D2H).
 *   img      : height x width x channels u8, row stride `stride` bytes; channels 1 (gray) or 3 (BGR, converted like
 *              cv::cvtColor(CV_BGR2GRAY), box_proposal_detail.cpp:62-66)
 *   K        : 3x3 row-major calibration (set_calibration, box_proposal_detail.cpp:36-40)
 *   Twc      : 4x4 row-major camera-to-world (transToWolrd)
 *   boxes    : n_boxes x 5  [x y w h prob], 0-based (obj_bbox_coors)
 *   lines    : n_lines x 4  [x1 y1 x2 y2] (all_lines_raw; copied, like the by-value MatrixXd of the reference)
 *   out      : n_boxes * max_cuboid_num records; box b's cuboids are out[b*max_cuboid_num + i], i < counts[b],
 *              sorted by combined score (ObjectSet order, box_proposal_detail.cpp:517-536)
 * With whether_sample_cam_roll_pitch and more than one box the boxes are taken one after the other, like the reference's loop
 * over objects: box b + 1 reads the camera yaw that box b left in cam_pose (box_proposal_detail.cpp:126 after :233-239 /
 * :481-487) -- the configuration of object_slam/src/main_obj.cpp:442.  A cs_cuboid_batch starts every box from the raw pose.
 */
int cs_cuboid_detect(cs_ctx *ctx, const uint8_t *img, int width, int height, int channels, int stride,
                     const double *K, const double *Twc, const double *boxes, int n_boxes,
                     const double *lines, int n_lines, const cs_cuboid_opts *opts,
                     cs_cuboid *out, int *counts);

/*
 * Batched, device-resident form (BASELINE config 4: many frames x boxes).  create() uploads everything to HBM and
 * plans the arenas; run() only launches kernels on the context's stream (asynchronous); read() synchronises and
 * copies results back.  All frames share width/height/K/opts.
 *   gray        : n_frames x height x width u8, densely packed
 *   Twc         : n_frames x 16
 *   box_offsets : n_frames+1 prefix offsets into `boxes` (rows)
 *   line_offsets: n_frames+1 prefix offsets into `lines` (rows)
 */
typedef struct cs_cuboid_batch cs_cuboid_batch;
int cs_cuboid_batch_create(cs_ctx *ctx, int n_frames, int width, int height, const uint8_t *gray,
                           const double *K, const double *Twc, const int *box_offsets, const double *boxes,
                           const int *line_offsets, const double *lines, const cs_cuboid_opts *opts,
                           cs_cuboid_batch **out);
int cs_cuboid_batch_run(cs_ctx *ctx, cs_cuboid_batch *b);
/* New edge lists (line_offsets[n_frames + 1], lines m x 4 as in cs_cuboid_batch_create) for the frames of an existing batch: the hand-over of the
 * chain detect_filter_lines -> detect_cuboid (main_obj.cpp:428-449) when frames and boxes stay resident. */
int cs_cuboid_batch_set_lines(cs_ctx *ctx, cs_cuboid_batch *b, const int *line_offsets, const double *lines);
/* frames the batch was created with (line_offsets of cs_cuboid_batch_set_lines holds one more entry); -1 for NULL */
int cs_cuboid_batch_n_frames(const cs_cuboid_batch *b);
/* Other 2-D boxes, camera poses and (line_offsets non-NULL) edge lists for the frames of an existing batch -- the arguments every call of detect_cuboid brings with its
 * pixels (detect_3d_cuboid.h:62-63).  Same frame count, image size and options; layouts as in cs_cuboid_batch_create.  The plan of the sweep (ROIs, top samples, arena
 * slices: box_proposal_detail.cpp:107-161) is rebuilt for them on the host (a function of boxes and poses alone) and uploaded from pinned staging on the context's stream
 * behind the run that still reads the old one; the call waits only when an arena has to grow.  A box whose ROI leaves the image, offsets that do not start at 0 or
 * that decrease, rows that are NULL where the offsets count some: CS_ERR_BAD_ARG; after that or a failed allocation the batch stays as it was.
 * Results (cs_cuboid_batch_read) then hold box_offsets[n_frames] boxes. */
int cs_cuboid_batch_set_scene(cs_ctx *ctx, cs_cuboid_batch *b, const double *Twc, const int *box_offsets, const double *boxes, const int *line_offsets, const double *lines);
int cs_cuboid_batch_n_boxes(const cs_cuboid_batch *b);
/* shared != 0: long-running kernels of other streams hold most CUs while this batch runs (cs_frontend's alternating runner does this itself): the edge-scoring
 * kernel takes the launch shape that fits beside them.  A speed hint only. */
int cs_cuboid_batch_set_shared_gpu(cs_cuboid_batch *b, int shared);
/* out: total_boxes * max_cuboid_num, counts: total_boxes */
int cs_cuboid_batch_read(cs_ctx *ctx, cs_cuboid_batch *b, cs_cuboid *out, int *counts);
void cs_cuboid_batch_destroy(cs_ctx *ctx, cs_cuboid_batch *b);

/* Workload facts for roofline accounting (valid after run + sync): number of (box, height-sample) units, total ROI
 * pixels A, total enumerated hypotheses, total valid proposals. */
int cs_cuboid_batch_stats(cs_ctx *ctx, cs_cuboid_batch *b, long *n_units, long *roi_pixels, long *n_hypotheses,
                          long *n_valid);
/* The same facts split by scoring kernel (valid after run + sync).  out[0..2] = units, ROI pixels, valid proposals scored by
 * cuboid_sweep_score (the unit's 16-bit chamfer code map fits one CU's LDS); out[3..5] = the same for cuboid_sweep_score_big (larger
 * ROIs, or a pixel farther than 244 px from every edge), which gathers from the float map. */
int cs_cuboid_batch_score_stats(cs_ctx *ctx, cs_cuboid_batch *b, long out[6]);

/* Introspection for parity tests (after run).  unit = index over (frame, box, height-sample) in that order.
 *   dims    : [roi_x, roi_y, roi_w, roi_h, n_hyp_capacity, n_valid, n_merged_lines, n_yaw, frame, box, height_sample, n_height_samples]
 *   edges   : roi_w*roi_h u8 Canny output (0/255), may be NULL
 *   dist    : roi_w*roi_h f32 distance map, may be NULL
 *   rows    : n_valid x 25 doubles in the reference's row layout
 *             [cfg, vp1pos, yaw, top_id, dist/diag, angle, hExp, roll, pitch, x0..x7, y0..y7], may be NULL (cap rows_cap)
 *   merged  : n_merged_lines x 4 doubles, may be NULL (cap merged_cap rows)
 */
int cs_cuboid_batch_unit(cs_ctx *ctx, cs_cuboid_batch *b, int unit, int dims[12], uint8_t *edges, float *dist,
                         double *rows, long rows_cap, double *merged, long merged_cap);

/* ===================================================================== ORBextractor
 * Replaces ORB_SLAM2::ORBextractor (orb_object_slam/include/ORBextractor.h:46-117, src/ORBextractor.cc):
 * constructor tables (:412-471), ComputePyramid (:1101-1125), ComputeKeyPointsOctTree (:766-853), IC_Angle (:74-101),
 * 7x7 Gaussian blur + steered rBRIEF (:104-150,:1069-1098).  FAST scores / cell NMS / orientation / blur / descriptors
 * run on the GPU; the order-dependent quadtree selection (DistributeOctTree :540-763) runs on the host between the two
 * GPU phases. */
typedef struct cs_keypoint {             /* cv::KeyPoint layout, 28 bytes */
    float x, y;                          /* pt */
    float size;
    float angle;                         /* degrees, cv::fastAtan2 */
    float response;                      /* FAST corner score */
    int32_t octave;
    int32_t class_id;                    /* -1 */
} cs_keypoint;

typedef struct cs_orb cs_orb;
/* ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) for images of width x height; up to max_frames
 * frames are processed per call (device buffers are sized once). */
int cs_orb_create(cs_ctx *ctx, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                  int width, int height, int max_frames, cs_orb **out);
void cs_orb_destroy(cs_ctx *ctx, cs_orb *e);
/* GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares (ORBextractor.h:63-83);
 * which = 0..3, out has nlevels floats.  which = 4: mnFeaturesPerLevel as ints (out reinterpreted as int32). */
int cs_orb_get_table(const cs_orb *e, int which, void *out);
/* ORBextractor::operator() for n_frames gray images (host, row stride `stride`).  Per frame f: counts[f] keypoints at
 * kps[f*cap_per_frame ...] and descriptors at desc[(f*cap_per_frame + i)*32], level-major order (:1065-1098).
 * Returns CS_ERR_CAPACITY if a frame yields more than cap_per_frame keypoints. */
int cs_orb_extract(cs_ctx *ctx, cs_orb *e, const uint8_t *gray, int n_frames, int stride,
                   cs_keypoint *kps, uint8_t *desc, int cap_per_frame, int *counts);
/* Device-resident form: upload once, run() = both GPU phases + host quadtree, read() = D2H of the results. */
int cs_orb_upload(cs_ctx *ctx, cs_orb *e, const uint8_t *gray, int n_frames, int stride);
int cs_orb_run(cs_ctx *ctx, cs_orb *e);
int cs_orb_read(cs_ctx *ctx, cs_orb *e, cs_keypoint *kps, uint8_t *desc, int cap_per_frame, int *counts);
/* The same results packed: every frame's key points / descriptors one frame behind the other, frame f = first[f] .. first[f + 1] (n_frames + 1 entries), two copies
 * for the whole batch.  kps / desc NULL: only *total and first are filled (size query); CS_ERR_CAPACITY when cap_total < *total. */
int cs_orb_read_packed(cs_ctx *ctx, cs_orb *e, cs_keypoint *kps, uint8_t *desc, long cap_total, int *first, long *total);
/* Introspection for parity tests (after run): pyramid level (mvImagePyramid, ORBextractor.h:85) or its blurred copy;
 * the FAST keypoints handed to DistributeOctTree (x, y, response; cell-major order). */
int cs_orb_get_level(cs_ctx *ctx, cs_orb *e, int frame, int level, int blurred, uint8_t *out, int *w, int *h);
int cs_orb_get_candidates(cs_ctx *ctx, cs_orb *e, int frame, int level, float *xyr, int cap, int *n);

/* ===================================================================== Stereo association
 * Replaces ORB_SLAM2::Frame::ComputeStereoMatches (orb_object_slam/src/Frame.cc:611-783, called at :118 after the two extractions of the stereo
 * constructor, :106-110): fills mvuRight / mvDepth for rectified stereo pairs from what cs_orb_run left on the device (key points, descriptors and
 * mvImagePyramid of both extractors), bit-identical to the reference's arithmetic.  GPU: row / octave / disparity-range tests and 256-bit Hamming
 * distances (:639-692), the 11 x 11 SAD search over 11 shifts at the left key point's level with the parabola fit (:696-765), the median cut (:769-782).
 * What is undefined in the reference (a row index outside the image, a patch that leaves its level, zero accepted matches) is guarded and ends as
 * unmatched; it cannot occur for key points that come from the extractor. */
typedef struct cs_stereo cs_stereo;
/* Room for max_pairs pairs of at most max_keypoints_per_frame key points per image (left and right). */
int cs_stereo_create(cs_ctx *ctx, int max_keypoints_per_frame, int max_pairs, cs_stereo **out);
void cs_stereo_destroy(cs_ctx *ctx, cs_stereo *s);
/* Frame::ComputeStereoMatches (Frame.cc:611-783) for n_pairs pairs: pair p = frame left_first + p of `left`'s last cs_orb_run against frame
 * right_first + p of `right`'s.  left == right is allowed (one extractor run over 2F images, left_first = 0, right_first = F).  Both extractors
 * must agree in image size, nlevels and scaleFactor (CS_ERR_BAD_ARG otherwise, as for n_pairs outside either run or above max_pairs, bf <= 0, b <= 0);
 * CS_ERR_CAPACITY when a frame has more key points than the handle was created for.  bf = mbf, b = mb (minZ = mb, maxD = mbf / mb, :639-641): the
 * reference's stereo constructor sets mb = mbf / fx at Frame.cc:141, after the call at :118, so the caller passes the value it means.  Queues the
 * kernels on the context's stream and returns; the results stay on the device. */
int cs_stereo_match_from_orb(cs_ctx *ctx, cs_stereo *s, const cs_orb *left, int left_first, const cs_orb *right, int right_first, int n_pairs, float bf, float b);
/* The same over host arrays, for a caller whose key points and descriptors come from elsewhere (the CPU extractor, a replayed log): pair p's left key points are
 * keysL[firstL[p] .. firstL[p + 1]) with 32-byte descriptors descL (likewise firstR / keysR / descR; n_pairs + 1 offsets each, starting at 0 and not decreasing).
 * The extractors supply only the resident pyramids and scale tables (cs_orb_device_pyramid): they must have run on the frames named, and the geometry checks are
 * those of cs_stereo_match_from_orb.  A right frame's key points must be in level-major order, as ORBextractor::operator() emits them (its octaves never decrease
 * within the frame): the device finds a level's right key points as one contiguous range.  CS_ERR_BAD_ARG: a NULL array that is needed, offsets that do not start
 * at 0 or decrease, a right frame whose octaves decrease, a coordinate that is not finite or above 2^24 in magnitude; CS_ERR_CAPACITY: a frame with more key
 * points than the handle was created for.  A refused call leaves the previous result readable.  The key points go into device blocks the handle allocates on the
 * first call through this entry; the same kernels run; the call waits for its uploads, so the arrays are the caller's again when it returns. */
int cs_stereo_match_from_keys(cs_ctx *ctx, cs_stereo *s, const cs_orb *left, int left_first, const cs_orb *right, int right_first, int n_pairs, const int *firstL,
                              const cs_keypoint *keysL, const uint8_t *descL, const int *firstR, const cs_keypoint *keysR, const uint8_t *descR, float bf, float b);
/* mvuRight / mvDepth of the last call: pair p's counts[p] values at u_right[p * cap_per_frame ...] / depth[...], -1 where unmatched (:613-614);
 * n_matched[p] = matches left after the cut.  CS_ERR_CAPACITY (nothing copied) when a pair has more than cap_per_frame left key points. */
int cs_stereo_read(cs_ctx *ctx, cs_stereo *s, float *u_right, float *depth, int cap_per_frame, int *counts, int *n_matched);
/* The same packed like cs_orb_read_packed: pair p = first[p] .. first[p + 1] (n_pairs + 1 entries), two copies for the whole batch.  u_right / depth NULL:
 * only *total and first are filled (size query); CS_ERR_CAPACITY when cap_total < *total.  n_matched may be NULL. */
int cs_stereo_read_packed(cs_ctx *ctx, cs_stereo *s, float *u_right, float *depth, long cap_total, int *first, long *total, int *n_matched);
/* Device pointers of pair `pair`'s mvuRight / mvDepth (*n floats each, valid until the next call on this handle) for a caller that feeds
 * cs_match_fuse / cs_pose_optimization next; work queued on the context's stream after the call sees the results. */
int cs_stereo_device_pair(const cs_stereo *s, int pair, const float **d_u_right, const float **d_depth, int *n);

/* ===================================================================== RGB-D association and close-point creation
 * Replaces ORB_SLAM2::Frame::ComputeStereoFromRGBD (orb_object_slam/src/Frame.cc:785-806, called at :173 of the RGB-D constructor, :146-199) together with the
 * one use of the converted depth image (Tracking::GrabImageRGBD, src/Tracking.cc:366-404, convertTo(CV_32F, mDepthMapFactor) at :388), and the rule by which
 * Tracking creates map points from measured depth for both depth sensors: StereoInitialization (:783-850), UpdateLastFrame (:1207-1274) and the stereo / RGB-D
 * block of CreateNewKeyFrame (:2067-2130), all over Frame::UnprojectStereo (Frame.cc:808-822) and Frame::UpdatePoseMatrices (:334-344).
 * The depth image stays raw on the device: only the samples under the key points are read and converted, d = (float)raw * depth_map_factor (one float multiply,
 * what cv::Mat::convertTo gives for that sample; depth_map_factor == 1 is the exact copy).  Sample: row (int)kp.pt.y, column (int)kp.pt.x of the DISTORTED key
 * point (truncation toward zero).  d > 0 (NaN is not, +inf is): mvDepth = d, mvuRight = kpU.pt.x - mbf / d; -1 / -1 otherwise.  A sample outside the image or a NaN
 * coordinate reads beyond the Mat in the reference; here the key point ends unmatched and is counted in n_outside.  It cannot occur for key points that come from
 * the extractor: they lie >= 19 pixels from every border. */
#define CS_DEPTH_U16 0                   /* CV_16UC1, the sensor's raw units */
#define CS_DEPTH_F32 1                   /* CV_32FC1 */
#define CS_RGBD_MAX_KEYPOINTS 8192       /* per frame: what the close-point kernel sorts in one compute unit's LDS (8 192 64-bit keys = 64 KB) */
#define CS_CLOSE_POINTS_NEAREST 0        /* the sorted walk of Tracking.cc:1221-1273 / :2075-2128 */
#define CS_CLOSE_POINTS_ALL 1            /* StereoInitialization (:804-819): every z > 0 in index order, need_new ignored */
typedef struct cs_rgbd cs_rgbd;
/* Room for max_frames depth images of width x height and at most max_keypoints_per_frame key points per frame (CS_ERR_BAD_ARG above CS_RGBD_MAX_KEYPOINTS). */
int cs_rgbd_create(cs_ctx *ctx, int width, int height, int max_keypoints_per_frame, int max_frames, cs_rgbd **out);
void cs_rgbd_destroy(cs_ctx *ctx, cs_rgbd *h);
/* n_frames depth images (host, rows stride_bytes apart, frames height * stride_bytes apart), type CS_DEPTH_U16 / CS_DEPTH_F32, stored as they are. */
int cs_rgbd_upload_depth(cs_ctx *ctx, cs_rgbd *h, const void *depth, int type, int n_frames, long stride_bytes);
/* The same for a batch already in device memory, frames one behind the other with dense rows (a copy on the context's stream, nothing waits; cs_orb_set_frames_device). */
int cs_rgbd_set_depth_device(cs_ctx *ctx, cs_rgbd *h, const void *d_depth, int type, int n_frames);
/* Frame::ComputeStereoFromRGBD for frames first_frame .. first_frame + n_frames - 1 of the extractor's last cs_orb_run against depth images 0 .. n_frames - 1 of the
 * handle: Frame::UndistortKeyPoints (K4 = fx fy cx cy, dist5 = k1 k2 p1 p2 k3 or NULL, as cs_matcher_set_frame_from_orb) and the association, from the extractor's
 * device key points.  CS_ERR_BAD_ARG: frames outside the run, more than the handle holds or than depth images were given, an extractor of another image size, a
 * NULL K4, bf <= 0; CS_ERR_CAPACITY: a frame with more key points than the handle was created for.  Queued on the context's stream; the results stay on the device. */
int cs_rgbd_from_orb(cs_ctx *ctx, cs_rgbd *h, const cs_orb *orb, int first_frame, int n_frames, const float *K4, const float *dist5, float bf, float depth_map_factor);
/* The same over host arrays, for a caller that owns mvKeys / mvKeysUn: frame f = first[f] .. first[f + 1] (n_frames + 1 entries) of keys / keysUn.  The call waits
 * for its uploads, so both arrays are the caller's again when it returns; the results stay on the device. */
int cs_rgbd_from_keys(cs_ctx *ctx, cs_rgbd *h, int n_frames, const int *first, const cs_keypoint *keys, const cs_keypoint *keysUn, float bf, float depth_map_factor);
/* mvuRight / mvDepth of the last cs_rgbd_from_*: frame f's counts[f] values at u_right[f * cap_per_frame ...] / depth[...], -1 where there is no depth;
 * n_with_depth[f] = key points with depth, n_outside[f] (may be NULL) = key points whose sample lies outside the image.  CS_ERR_CAPACITY (nothing copied) when a
 * frame has more than cap_per_frame key points. */
int cs_rgbd_read(cs_ctx *ctx, cs_rgbd *h, float *u_right, float *depth, int cap_per_frame, int *counts, int *n_with_depth, int *n_outside);
/* The same packed like cs_stereo_read_packed: frame f = first[f] .. first[f + 1].  u_right / depth NULL: only *total and first are filled; CS_ERR_CAPACITY (nothing
 * copied) when cap_total < *total.  n_with_depth / n_outside may be NULL. */
int cs_rgbd_read_packed(cs_ctx *ctx, cs_rgbd *h, float *u_right, float *depth, long cap_total, int *first, long *total, int *n_with_depth, int *n_outside);
/* mvKeysUn of the last cs_rgbd_from_*, packed in the same order (cap_total records; CS_ERR_CAPACITY with nothing copied when there are more). */
int cs_rgbd_read_keys_un(cs_ctx *ctx, cs_rgbd *h, cs_keypoint *keysUn, long cap_total);
/* Device pointers of frame `frame`'s mvuRight / mvDepth (*n floats each) and, d_keysUn non-NULL, mvKeysUn; valid until the next call on this handle.  Work queued
 * on the context's stream after the call sees the results. */
int cs_rgbd_device_frame(const cs_rgbd *h, int frame, const float **d_u_right, const float **d_depth, const cs_keypoint **d_keysUn, int *n);
/* Frame::ComputeStereoFromRGBD of one frame on the host, the same text as the kernel (the comparison side of tests and benchmarks; no context, no device). */
int cs_rgbd_host_from_keys(const void *depth, int type, int width, int height, long stride_bytes, int n, const cs_keypoint *keys, const cs_keypoint *keysUn, float bf,
                           float depth_map_factor, float *u_right, float *depth_out, int *n_with_depth, int *n_outside);

/* The close-point rule for n_frames frames (frame f = first[f] .. first[f + 1] of depth / keysUn / need_new; at most CS_RGBD_MAX_KEYPOINTS per frame, CS_ERR_CAPACITY
 * above).  depth = mvDepth from any source (cs_stereo_read, cs_rgbd_read), keysUn = mvKeysUn, need_new[i] = the caller's `!pMP || pMP->Observations() < 1` (may be
 * NULL with CS_CLOSE_POINTS_ALL), Tcw = 12 floats per frame (rows of [Rcw | tcw]), K4 = fx fy cx cy, th_depth = mThDepth.  Per frame f:
 *   n_valid[f]   key points with z > 0
 *   order        their indices in the frame, sorted by (z, index) = sort(vDepthIdx) (CS_CLOSE_POINTS_ALL: in index order), at order[first[f] ...]
 *   n_walked[f]  the reference's nPoints when its loop ends: the entries of `order` that were looked at
 *   new_first    n_frames + 1 offsets into new_idx / new_x3D
 *   new_idx      the key points a point is created for, in creation order (the order of MapPoint::mnId and of mlpTemporalPoints)
 *   new_x3D      Frame::UnprojectStereo of each, 3 floats
 * order, new_idx: room for first[n_frames] ints, new_x3D for 3 * first[n_frames] floats.  ctx == NULL: the same statement on the host (the comparison side).
 * The test mCurrentFrame.N > 500 of Tracking.cc:786 and everything done with `new MapPoint` stay the caller's. */
int cs_close_points(cs_ctx *ctx, int n_frames, const int *first, const float *depth, const cs_keypoint *keysUn, const uint8_t *need_new, const float *Tcw, const float *K4,
                    float th_depth, int mode, int *n_valid, int *order, int *n_walked, int *new_first, int *new_idx, float *new_x3D);
/* The same on what the last cs_rgbd_from_* left on the device (frames and order of that call; mvDepth and mvKeysUn are not copied). */
int cs_rgbd_close_points(cs_ctx *ctx, cs_rgbd *h, const uint8_t *need_new, const float *Tcw, const float *K4, float th_depth, int mode, int *n_valid, int *order,
                         int *n_walked, int *new_first, int *new_idx, float *new_x3D);

/* ===================================================================== dynamic-object KLT
 * Replaces cv::calcOpticalFlowPyrLK(LastFrame.raw_img, CurrentFrame.raw_img, lastobjpts, currobjpts, status, err, cv::Size(21, 21), 3) of
 * ORBmatcher::SearchByTrackingHarris (orb_object_slam/src/ORBmatcher.cc:1548) and ORBmatcher::SearchByTracking (:1620), for many frame pairs in one call, and the
 * selection pass of SearchByTrackingHarris (:1556-1579).  OpenCV is not part of the reference tree: the function is a stated definition (the plain
 * C++ branches of OpenCV 3.x lkpyramid.cpp), and every result equals that statement bit for bit.
 * GPU: pyramid and Scharr derivatives of every frame once, levels resident with their 21-pixel pads; all points of all pairs in one launch.
 * A handle holds at most max_frames 8-bit images of at most max_width x max_height and tracks at most max_points points per call. */
typedef struct cs_klt cs_klt;
int cs_klt_create(cs_ctx *ctx, int max_frames, int max_width, int max_height, int max_points, cs_klt **out);
void cs_klt_destroy(cs_ctx *ctx, cs_klt *h);
/* buildOpticalFlowPyramid and calcSharrDeriv for n_frames images of width x height (both > 21; rows stride_bytes apart, frame f at gray + f * height * stride_bytes).
 * A later call may bring fewer frames or another size within the capacity (CS_ERR_CAPACITY beyond it; the handle keeps its frames then).  A call that fails with
 * CS_ERR_HIP leaves the handle without frames. */
int cs_klt_set_frames(cs_ctx *ctx, cs_klt *h, int n_frames, int width, int height, const uint8_t *gray, long stride_bytes);
/* The levels the pyramids hold: 4, or fewer where building stopped at the first level of 21 pixels or less a side (0: no frames are set). */
int cs_klt_levels(const cs_klt *h);
/* One resident level as the tracker reads it, for inspection: (w + 42) x (h + 42) bytes with the REFLECT_101 pad, and as many (Ix, Iy) int16 pairs with the
 * constant pad; either pointer may be NULL. */
int cs_klt_read_level(cs_ctx *ctx, cs_klt *h, int frame, int level, uint8_t *image, int16_t *deriv);
/* The calcOpticalFlowPyrLK call of :1548 / :1620 for n_pairs pairs: pair p tracks the points first[p] .. first[p + 1] (x, y floats in prev_pts) from frame
 * pair_prev[p] to frame pair_next[p] of the last cs_klt_set_frames.  A frame may be `next` of one pair and `prev` of another; an empty pair is legal.
 * next_pts (2 floats), status and err per point as the OpenCV function returns them.  Points that are not finite: CS_ERR_BAD_ARG. */
int cs_klt_track(cs_ctx *ctx, cs_klt *h, int n_pairs, const int *pair_prev, const int *pair_next, const int *first, const float *prev_pts, float *next_pts, uint8_t *status,
                 float *err);
/* The same statement on the host, without a context, over the images themselves (the comparison side). */
int cs_klt_track_host(const uint8_t *gray, int n_frames, int width, int height, long stride_bytes, int n_pairs, const int *pair_prev, const int *pair_next, const int *first,
                      const float *prev_pts, float *next_pts, uint8_t *status, float *err);
/* ORBmatcher::SearchByTrackingHarris (ORBmatcher.cc:1524-1580) for n_pairs pairs.  last_pts = pt of LastFrame.mvKeysHarris (= featuresklt_lastframe), masks = the
 * pairs' CurrentFrame.objmask_img, n_pairs dense images of the frames' size.  Outputs: this_pts / status / err = featuresklt_thisframe and the tracker's flags for
 * every point; per pair p the survivors in index order at kept_first[p] .. kept_first[p + 1]: kept = the index within the pair (of LastFrame.mvpMapPointsHarris),
 * kept_pts = the new mvKeysHarris, object_id = maskval - 1; goodmatches[p].  The mask is read as cv::Mat::at<uchar>(Point2f) reads it, at
 * data[cvRound(y) * cols + cvRound(x)], which is the next row's first pixel when x rounds to cols.  DEVIATION: where that index is >= rows * cols the reference
 * reads beyond the image; here the point is dropped and counted in n_mask_outside[p] (may be NULL).  kept, object_id: room for first[n_pairs] ints. */
int cs_match_by_tracking_harris(cs_ctx *ctx, cs_klt *h, int n_pairs, const int *pair_prev, const int *pair_next, const int *first, const float *last_pts, const uint8_t *masks,
                                float *this_pts, uint8_t *status, float *err, int *kept_first, int *kept, float *kept_pts, int *object_id, int *goodmatches,
                                int *n_mask_outside);
int cs_match_by_tracking_harris_host(const uint8_t *gray, int n_frames, int width, int height, long stride_bytes, int n_pairs, const int *pair_prev, const int *pair_next,
                                     const int *first, const float *last_pts, const uint8_t *masks, float *this_pts, uint8_t *status, float *err, int *kept_first, int *kept,
                                     float *kept_pts, int *object_id, int *goodmatches, int *n_mask_outside);
/* (cs_match_by_tracking, ORBmatcher::SearchByTracking over the same tracker, is declared behind cs_matcher below.) */

/* ----- new dynamic-object points: cv::goodFeaturesToTrack and the new-feature loop of Tracking::CreateNewKeyFrame (orb_object_slam/src/Tracking.cc:2258-2337)
 * cv::goodFeaturesToTrack(raw_img, corners, 200, 0.1, MIN_DIST, good_mask) of Tracking.cc:2292 for n frames a KLT handle holds: frames[s] = an index of the last
 * cs_klt_set_frames (level 0 of the pyramid is raw_img and is read in place), masks = n dense images of the frames' size or NULL (every pixel counts).  8 bits, one
 * channel, blockSize 3, Sobel aperture 3, minimum eigenvalue; useHarrisDetector is not built.  Like cs_klt_track the function is a stated definition (INTEGRATION.md 4e,
 * the plain C++ branches of OpenCV 3.4), and every result equals that statement bit for bit.
 * corners: room for n * max_corners points (x, y floats), frame s at corners + 2 * max_corners * s in the order of acceptance; quality (may be NULL): the thresholded
 * eigenvalue of each corner, likewise; counts[s] = the corners of frame s, n_candidates[s] = its local maxima above the threshold inside the mask.
 * CS_ERR_BAD_ARG: max_corners < 1; min_distance < 1 (or not finite); quality_level outside (0, 1]; a frame index that is not set; a null argument.
 * CS_ERR_CAPACITY: a frame with more than CS_GFTT_MAX_CANDIDATES candidates (n_candidates is filled, counts are 0).  The handle stays usable after either. */
#define CS_GFTT_MAX_CANDIDATES 8192
int cs_klt_good_features(cs_ctx *ctx, cs_klt *h, int n, const int *frames, const uint8_t *masks, int max_corners, double quality_level, double min_distance, float *corners,
                         float *quality, int *counts, int *n_candidates);
/* The same on the device for n images the caller passes (width x height, rows stride_bytes apart, image s at gray + s * height * stride_bytes), of any size: an
 * image with width < 3 or height < 3 has no corner. */
int cs_good_features_images(cs_ctx *ctx, const uint8_t *gray, int n, int width, int height, long stride_bytes, const uint8_t *masks, int max_corners, double quality_level,
                            double min_distance, float *corners, float *quality, int *counts, int *n_candidates);
/* The same statement on the host, without a context (the comparison side). */
int cs_klt_good_features_host(const uint8_t *gray, int n, int width, int height, long stride_bytes, const uint8_t *masks, int max_corners, double quality_level, double min_distance,
                              float *corners, float *quality, int *counts, int *n_candidates);
/* Tracking.cc:2263-2331 for n resident frames with the reference's constants (MIN_DIST = 10, 200 corners, quality 0.1): good_mask from objmasks (n dense objmask_img,
 * 0 background, > 0 object id + 1) with the disc of cv::circle(good_mask, pt, 10, 0, -1) erased around the existing points, goodFeaturesToTrack on it, and
 * KeyFrame::UnprojectPixelDepth (src/KeyFrame.cc:711-727) of every new corner at its cuboid's depth.
 * Frame s has the existing points exist_first[s] .. exist_first[s + 1]: exist_pts = mvKeysHarris[i].pt and exist_obs = pMP->Observations() of the points with
 * `pMP && pMP->is_dynamic` (:2270-2277).  They are walked by observations descending, equal counts by ascending index (the reference's std::sort leaves ties open).
 * K4 = fx, fy, cx, cy; Twc = 12 floats per frame (the 3 x 4 rows of the key frame's Twc); cuboid_depth[cub_first[s] + id] = (float)local_cuboids[id]->cube_meas.translation()[2].
 * Outputs, frame s at new_first[s] .. new_first[s + 1] (room for 200 n entries): new_pts = the corners, new_object_id = maskval - 1, new_x3D (3 floats) and x3D_valid
 * (0 where the depth is not > 0: the reference returns an empty Mat, here the position is zeros).  n_mask_outside[s] (may be NULL): DEVIATION, existing points whose
 * index cvRound(y) * cols + cvRound(x) is outside [0, rows * cols), where the reference reads beyond the image; they are skipped.  good_masks (may be NULL): the n masks
 * that were built, for inspection.  n_candidates (may be NULL): as above.
 * CS_ERR_BAD_ARG: an existing point that is not finite (or beyond 1e9 in magnitude); a frame index that is not set; offsets that do not start at 0 or decrease; a null
 * argument; a corner whose object id is at or beyond its frame's cuboid count (the reference indexes local_cuboids out of bounds).  CS_ERR_CAPACITY: as above. */
int cs_track_new_harris_features(cs_ctx *ctx, cs_klt *h, int n, const int *frames, const uint8_t *objmasks, const int *exist_first, const float *exist_pts, const int *exist_obs,
                                 const float *K4, const float *Twc, const int *cub_first, const float *cuboid_depth, int *new_first, float *new_pts, int *new_object_id, float *new_x3D,
                                 uint8_t *x3D_valid, int *n_mask_outside, uint8_t *good_masks, int *n_candidates);
int cs_track_new_harris_features_host(const uint8_t *gray, int n, int width, int height, long stride_bytes, const uint8_t *objmasks, const int *exist_first, const float *exist_pts,
                                      const int *exist_obs, const float *K4, const float *Twc, const int *cub_first, const float *cuboid_depth, int *new_first, float *new_pts,
                                      int *new_object_id, float *new_x3D, uint8_t *x3D_valid, int *n_mask_outside, uint8_t *good_masks, int *n_candidates);

/* ===================================================================== ORBmatcher
 * Replaces the Hamming searches of ORB_SLAM2::ORBmatcher (orb_object_slam/include/ORBmatcher.h:43-89, src/ORBmatcher.cc)
 * and the Frame grid they use (src/Frame.cc:303-318 AssignFeaturesToGrid, :404-459 GetFeaturesInArea, :525-535 PosInGrid).
 * GPU: 64x48 grid build, projection, per-query candidate lists (grid order) with 256-bit Hamming distances.
 * Host: the order-dependent greedy claim / ratio / rotation-histogram pass over those lists (sequential in the reference).
 * Monocular paths (mvuRight < 0). */
typedef struct cs_matcher cs_matcher;
int cs_matcher_create(cs_ctx *ctx, int max_keypoints, int max_queries, long max_candidates, cs_matcher **out);
void cs_matcher_destroy(cs_ctx *ctx, cs_matcher *m);
/* The frame searched in (CurrentFrame / F / F2): mvKeysUn, mDescriptors, mnMinX..mnMaxY. */
int cs_matcher_set_frame(cs_ctx *ctx, cs_matcher *m, const cs_keypoint *keysUn, const uint8_t *desc, int N,
                         float minX, float maxX, float minY, float maxY);
/* Frame post-processing without a host round trip: the keypoints and descriptors of frame `frame` of the last
 * cs_orb_run stay in HBM; Frame::UndistortKeyPoints (Frame.cc:546-576: copy when dist[0] == 0, else cv::undistortPoints(K, dist, P = K),
 * classic five-iteration form) and Frame::AssignFeaturesToGrid (:303-318) run on the device and the matcher is ready for the searches.
 * K4 = fx fy cx cy, dist5 = k1 k2 p1 p2 k3 (NULL = none); bounds from cs_frame_image_bounds.  keysUn_out (nullable, room for the
 * frame's keypoints) receives mvKeysUn; with NULL nothing is copied back and the call does not wait for the device (every search reads what it needs of a train key point
 * from the device copy; only cs_match_for_initialization, which updates vbPrevMatched on the host, needs a frame set WITH the copy). */
int cs_matcher_set_frame_from_orb(cs_ctx *ctx, cs_matcher *m, const cs_orb *orb, int frame, const float *K4, const float *dist5, float minX, float maxX, float minY,
                                  float maxY, cs_keypoint *keysUn_out, int *n_out);
/* Frame::ComputeImageBounds (Frame.cc:578-609): bounds = mnMinX, mnMaxX, mnMinY, mnMaxY of the undistorted image corners. */
int cs_frame_image_bounds(int cols, int rows, const float *K4, const float *dist5, float *bounds);
/* Workload facts of the last search on this matcher (queries, candidates the search windows enumerated), for roofline accounting. */
int cs_matcher_last_counts(const cs_matcher *m, int *queries, long *candidates);
/* Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) on the frame set above; *n = count (may exceed cap). */
int cs_matcher_features_in_area(cs_ctx *ctx, cs_matcher *m, float x, float y, float r, int minLevel, int maxLevel,
                                int *out, int cap, int *n);
/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono=true) (ORBmatcher.cc:1373-1522).
 * Per last-frame keypoint i: valid[i] (map point present, not outlier/dynamic), world_pos (float xyz), blocks[i] (map point
 * has Observations() > 0), the map point descriptor, LastFrame.mvKeys[i].octave and mvKeysUn[i].angle.  Tcw: 3x4 float
 * row-major.  train_blocked (N bytes, may be NULL): current-frame keypoints a candidate loop must skip -- the ones that already carry a
 * map point with Observations() > 0 before the call, and, in dynamic-object mode, the ones with KeysStatic[i2] == false
 * (ORBmatcher.cc:1451-1457).  train_match[N] receives the last-frame index matched to each current keypoint or -1. */
int cs_match_by_projection_frame(cs_ctx *ctx, cs_matcher *m, int n_last, const float *world_pos, const uint8_t *valid,
                                 const uint8_t *blocks, const uint8_t *mp_desc, const int *last_octave, const float *last_angle,
                                 const float *Tcw, float fx, float fy, float cx, float cy, const float *scale_factors, int n_levels,
                                 float th, int check_orientation, const uint8_t *train_blocked, int *train_match, int *nmatches);
/* The same search for a whole WINDOW of a stream whose frames an extractor holds in HBM: pair p = (last frame f0 + p, current frame f0 + p + 1), p < n_pairs.  Frame
 * post-processing of every current frame (UndistortKeyPoints + AssignFeaturesToGrid, Frame.cc:303-318, 546-576, from the extractor's device buffers) and the searches of all
 * pairs run as a handful of launches over the window (the per-frame calls take five launches and three host round trips per frame); results equal the per-frame calls'.
 * Queries: the key points of the last frames, concatenated over the pairs in order (n_q = key points of frames f0 .. f0 + n_pairs - 1): world_pos (3 floats each), valid,
 * blocks; their level and angle are the last frame's key points' (ORBmatcher.cc:1424, 1483); mp_desc: the map points' descriptors (32 B per query) or NULL = the last
 * frame's own descriptors.  Tcw: 12 floats per pair.  train_match: concatenated over the current frames f0 + 1 .. f0 + n_pairs (key point counts as the extractor reports
 * them), the matched query's index WITHIN its last frame or -1; nmatches[n_pairs].  n_queries / n_train: what the caller sized the per-query arrays and train_match for -- the
 * call fails with CS_ERR_BAD_ARG when they are not the extractor's counts for the window (an extractor that ran again in between).  There is no train_blocked here: a current frame
 * of the window carries no map points before its own search.  The claims (a key point claimed by a map point with observations is skipped by later queries), the rotation
 * histogram and its three-maxima cut run on the device, one wave per pair; candidates never leave HBM. */
typedef struct cs_match_stream cs_match_stream;
int cs_match_stream_create(cs_match_stream **out);
void cs_match_stream_destroy(cs_ctx *ctx, cs_match_stream *m);
int cs_match_by_projection_stream(cs_ctx *ctx, cs_match_stream *m, const cs_orb *orb, int f0, int n_pairs, const float *K4, const float *dist5 /* nullable */,
                                  float minX, float maxX, float minY, float maxY, int n_queries, int n_train, const float *world_pos, const uint8_t *valid, const uint8_t *blocks,
                                  const uint8_t *mp_desc /* nullable */, const float *Tcw, float fx, float fy, float cx, float cy, const float *scale_factors, int n_levels,
                                  float th, int check_orientation, int *train_match, int *nmatches);
/* queries and window candidates of the last call (roofline accounting) */
int cs_match_stream_last_counts(const cs_match_stream *m, long *queries, long *candidates);
/* ORBmatcher::SearchByTracking (ORBmatcher.cc:1582-1725) for one pair.  m: a matcher whose frame is the CURRENT frame (cs_matcher_set_frame*: mvKeysUn and mGrid);
 * h: a KLT handle that holds both gray frames (cs_klt_set_frames), last_frame / current_frame their indices.  Per key point i of the last frame: last_keys[i] =
 * LastFrame.mvKeys[i] (pt and octave are read), eligible[i] = the caller's `mvpMapPoints[i] && !KeysStatic[i] && mvpMapPoints[i]->is_dynamic`, object_id[i] =
 * keypoint_associate_objectID[i]; numobject, th, scale_factors = CurrentFrame.mvScaleFactors (n_levels >= 3 entries).  For the current frame, N entries each or NULL:
 * keys_static = KeysStatic (NULL: empty), had_map_point[j] = `mvpMapPoints[j] != NULL` before the call.  The device runs the octave < 3 selection and its ordered
 * compaction (:1591-1603), the optical flow, the per-object mean flow with its float sums in index order (:1629-1664), the direction test (:1682-1689),
 * Frame::GetCloestFeaturesInArea (Frame.cc:461-523: cells ix outer, iy inner, strict <, levels [octave, 2]), the KeysStatic rejection (:1699) and the assignment (:1707),
 * which is sequential in the reference: the last i keeps a key point.  Outputs: train_match[N] = the last-frame key index whose map point key point j takes, or -1;
 * *n_tracked = the points selected; sel = lastptsinds, klt_last / klt_this = featuresklt_lastframe / featuresklt_thisframe ((0, 0) for rejected points), room for
 * n_last entries each; counters = kltmatches, goodmatches, findfeaturematches, uniquematches (key points that had no map point when first assigned).
 * A tracked point whose object id is outside [0, numobject) indexes out of bounds in the reference: CS_ERR_BAD_ARG.  An object whose mean flow is exactly zero gets
 * 0 / 0 as its direction, as in the reference; only the norm is read then.  *n_tracked above the KLT handle's max_points: CS_ERR_CAPACITY; a matcher without a frame:
 * CS_ERR_BAD_ARG. */
int cs_match_by_tracking(cs_ctx *ctx, cs_matcher *m, cs_klt *h, int last_frame, int current_frame, int n_last, const cs_keypoint *last_keys, const uint8_t *eligible,
                         const int *object_id, int numobject, float th, const float *scale_factors, int n_levels, const uint8_t *keys_static, const uint8_t *had_map_point,
                         int *train_match, int *n_tracked, int *sel, float *klt_last, float *klt_this, int *counters);
/* The same statement on the host, without a context: the two gray frames and the current frame's mvKeysUn with its bounds (mnMinX, mnMaxX, mnMinY, mnMaxY) directly. */
int cs_match_by_tracking_host(const uint8_t *last_gray, const uint8_t *current_gray, int width, int height, long stride_bytes, int n_last, const cs_keypoint *last_keys,
                              const uint8_t *eligible, const int *object_id, int numobject, float th, const float *scale_factors, int n_levels, const cs_keypoint *keysUn, int N,
                              float minX, float maxX, float minY, float maxY, const uint8_t *keys_static, const uint8_t *had_map_point, int *train_match, int *n_tracked, int *sel,
                              float *klt_last, float *klt_this, int *counters);
/* ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*>&, th) (:50-142). */
int cs_match_local_map(cs_ctx *ctx, cs_matcher *m, int n_mp, const float *proj_xy, const float *view_cos, const int *pred_level,
                       const uint8_t *in_view, const uint8_t *blocks, const uint8_t *mp_desc, const float *scale_factors, int n_levels,
                       float th, float nnratio, const uint8_t *train_blocked, int *train_match, int *nmatches);
/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (:429-542); F2 = the frame set above. */
int cs_match_for_initialization(cs_ctx *ctx, cs_matcher *m, const cs_keypoint *keys1Un, const uint8_t *desc1, int N1,
                                float *prev_matched, int window_size, float nnratio, int check_orientation,
                                int *matches12, int *nmatches);
/* ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (ORBmatcher.cc:852-1003), the search: for every valid map point (the
 * caller did the preamble :871-919 -- projection u, v, ur = u - bf/z, image bounds, distance and viewing-angle tests, PredictScale) the
 * keypoint of the key frame set with cs_matcher_set_frame that has the smallest descriptor distance among GetFeaturesInArea(u, v,
 * th * scale[level]), after the level (:941), KeysStatic (:944), and chi-square tests (stereo 7.8 / mono 5.99, :947-971); first one
 * wins ties.  u_right = mvuRight, inv_level_sigma2 = mvInvLevelSigma2.  best_idx -1 / best_dist 256: none; *n_fused = number with
 * best_dist <= TH_LOW (what the reference returns).  Replace / AddObservation (:985-1000) stay with the caller's map. */
int cs_match_fuse(cs_ctx *ctx, cs_matcher *m, const float *u_right, const float *inv_level_sigma2, int n_levels, const uint8_t *keys_static, int n_mp, const float *uv,
                  const float *ur, const int *pred_level, const uint8_t *valid, const uint8_t *mp_desc, const float *scale_factors, float th, int *best_idx,
                  int *best_dist, int *n_fused);
/* The searches that project map points through a Sim3 or a relocalisation pose.  Unlike cs_match_fuse / cs_match_local_map the per-map-point preamble runs on the device, bit for
 * bit as the reference computes it (cv::Mat products as one gemm per row, cv::norm and Mat::dot accumulated in double, MapPoint::PredictScale with glibc's logf restated,
 * cube_slam_amd/csrc/glibc_logf.h), so map points, normals and distance ranges can be handed over as they are stored.  Common to the four entries:
 *   world_pos[3 n], normal[3 n] = GetWorldPos / GetNormal; min_distance / max_distance = mfMinDistance / mfMaxDistance (the 0.8f / 1.2f of Get*DistanceInvariance are applied
 *   here); skip[i] != 0: the reference `continue`s before the transform; mp_desc[32 n] = GetDescriptor; train_blocked[N] (nullable): a key point of the searched frame that is
 *   never a candidate; log_scale_factor = mfLogScaleFactor, scale_factors[n_levels] = mvScaleFactors (n_levels <= 32).
 *   The transforms come decomposed, as the reference's own first lines produce them (Rcw = sRcw / scw, tcw, Ow = -Rcw.t() * tcw, sR12 = s12 * R12, ...): those are cv::MatExpr
 *   scale operations whose rounding depends on the OpenCV build, so the adapter lets OpenCV do them.  Row-major float[9] / float[3].
 *   Deviation: this fork's MapPoint::PredictScale (MapPoint.cc:524-533) does not clamp, and 0.8 min <= dist <= 1.2 max allows the levels -1, n_levels and n_levels + 1, where the
 *   reference reads past mvScaleFactors.  Such a point (and one whose mfMaxDistance / dist is not a positive normal float) is dropped like a rejected one and counted in
 *   *n_level_outside (nullable); the call succeeds.
 *   CS_ERR_BAD_ARG for NULL / out-of-range arguments as in cs_match_fuse, CS_ERR_CAPACITY when the windows hold more candidates than the matcher was created for (nothing is
 *   written past the arena; the matcher stays usable).  One wait per call; nothing is allocated.
 *
 * ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1727-1858), relocalisation.  The matcher holds
 * the current frame; map point i is pKF's i-th (kf_angle[i] = pKF->mvKeysUn[i].angle; skip[i] = no map point || isBad || in sAlreadyFound || is_dynamic); train_blocked[i2] =
 * CurrentFrame.mvpMapPoints[i2] != NULL || !KeysStatic[i2].  train_match[N]: the map point index a key point of the current frame received, -1 none (after the rotation cut
 * :1836-1855 when check_orientation); *nmatches: what the reference returns. */
int cs_match_by_projection_reloc(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *min_distance,
                                 const float *max_distance, const uint8_t *skip, const float *kf_angle, const uint8_t *mp_desc, const uint8_t *train_blocked /* nullable */, float fx,
                                 float fy, float cx, float cy, float log_scale_factor, const float *scale_factors, int n_levels, float th, int orb_dist, int check_orientation,
                                 int *train_match, int *nmatches, int *n_level_outside /* nullable */);
/* ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, th) (ORBmatcher.cc:309-427), loop closing.  The matcher
 * holds pKF; skip[i] = isBad || in spAlreadyFound || is_dynamic; train_blocked[idx] = vpMatched[idx] != NULL || !KeysStatic[idx].  train_match[N]: the index into vpPoints that
 * vpMatched[idx] receives, -1 none; *nmatches: what the reference returns. */
int cs_match_by_projection_sim3(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal,
                                const float *min_distance, const float *max_distance, const uint8_t *skip, const uint8_t *mp_desc, const uint8_t *train_blocked /* nullable */, float fx,
                                float fy, float cx, float cy, float log_scale_factor, const float *scale_factors, int n_levels, float th, int *train_match, int *nmatches,
                                int *n_level_outside /* nullable */);
/* ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1010-1139), the search :1033-1118.  The matcher holds pKF;
 * skip[i] = isBad || in pKF->GetMapPoints() || is_dynamic; train_blocked[idx] = !KeysStatic[idx].  best_idx[n_mp] / best_dist[n_mp]: the first minimum over the window
 * (-1 / INT_MAX: none); *n_fused = number with best_dist <= TH_LOW (what the reference returns).  vpReplacePoint / AddObservation / AddMapPoint (:1121-1135) stay with the
 * caller's map, as for cs_match_fuse. */
int cs_match_fuse_sim3(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal, const float *min_distance,
                       const float *max_distance, const uint8_t *skip, const uint8_t *mp_desc, const uint8_t *train_blocked /* nullable */, float fx, float fy, float cx, float cy,
                       float log_scale_factor, const float *scale_factors, int n_levels, float th, int *best_idx, int *best_dist, int *n_fused, int *n_level_outside /* nullable */);
/* Tracking::SearchLocalPoints (Tracking.cc:2673-2728) in one call: Frame::isInFrustum (Frame.cc:346-402) for every local map point and ORBmatcher::SearchByProjection(F,
 * vpMapPoints, th) (ORBmatcher.cc:50-142) -- cs_match_local_map with its preamble on the device.  The matcher holds the current frame; Rcw, tcw, Ow = mRcw, mtcw, mOw;
 * skip[i] = mnLastFrameSeen == mCurrentFrame.mnId || isBad || is_dynamic (:2702-2707; the loop over the frame's own points, :2676-2694, stays with the caller); blocks[i] =
 * Observations() > 0 (what a later point's candidate loop asks of a key point claimed by point i, :96-98); train_blocked[idx] = (mvpMapPoints[idx] && Observations() > 0) ||
 * !KeysStatic[idx]; bf = mbf; viewing_cos_limit = 0.5 at :2710; th = the search radius factor (:2720-2725), nnratio = 0.8 (:2719).
 * train_match[N]: the local point a key point receives, -1 none; *nmatches: what the search returns; *n_to_match = nToMatch.  What isInFrustum leaves on a map point comes back per
 * point: in_view[n] = mbTrackInView (the caller's IncreaseVisible), proj[3 n] = (mTrackProjX, mTrackProjY, mTrackProjXR), pred_level[n] = mnTrackScaleLevel (-1 when not in view),
 * view_cos[n] = mTrackViewCos (proj and view_cos 0 when not in view); the last three are nullable.
 * Deviations: (1) a predicted level outside the scale table drops the point and counts it in *n_level_outside, as above -- it is not in view and not in *n_to_match; (2) PcZ == 0
 * passes the reference's depth test, and where it leaves u or v not finite (NaN: the bounds comparisons are all false and the reference goes on to undefined float -> int casts) the
 * point is rejected.  With *n_to_match == 0 the reference does not call the search (:2717); here no query is valid then and train_match is all -1 all the same.  The stereo test on
 * mvuRight (:104-109) is not applied, as in cs_match_local_map; uR is only returned.  One wait per call; nothing is allocated. */
int cs_match_local_map_frustum(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal,
                               const float *min_distance, const float *max_distance, const uint8_t *skip, const uint8_t *blocks, const uint8_t *mp_desc,
                               const uint8_t *train_blocked /* nullable */, float fx, float fy, float cx, float cy, float bf, float log_scale_factor, const float *scale_factors, int n_levels,
                               float viewing_cos_limit, float th, float nnratio, int *train_match, int *nmatches, int *n_to_match, int *n_level_outside /* nullable */, uint8_t *in_view,
                               float *proj /* nullable */, int *pred_level /* nullable */, float *view_cos /* nullable */);
/* ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (ORBmatcher.cc:852-1003) with its preamble (:871-920) on the device: cs_match_fuse without the caller's part.  The
 * matcher holds pKF; Rcw, tcw, Ow = GetRotation / GetTranslation / GetCameraCenter; skip[i] = !pMP || isBad || IsInKeyFrame(pKF) || is_dynamic; bf = mbf; u_right, inv_level_sigma2,
 * keys_static, best_idx, best_dist, *n_fused as for cs_match_fuse; *n_level_outside as above. */
int cs_match_fuse_map(cs_ctx *ctx, cs_matcher *m, const float *u_right, const float *inv_level_sigma2, int n_levels, const uint8_t *keys_static /* nullable */, const float *Rcw,
                      const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal, const float *min_distance, const float *max_distance, const uint8_t *skip,
                      const uint8_t *mp_desc, float fx, float fy, float cx, float cy, float bf, float log_scale_factor, const float *scale_factors, float th, int *best_idx, int *best_dist,
                      int *n_fused, int *n_level_outside /* nullable */);
/* Tracking::UpdateLocalPoints (Tracking.cc:2740-2764).  kf_off[n_kf + 1] / kf_mp: the GetMapPointMatches() lists of mvpLocalKeyFrames in order, as indices into the caller's point
 * table (-1: no map point); skip[n_points] = isBad || (whether_dynamic_object && is_dynamic).  local_points (room for min(kf_off[n_kf], n_points)): mvpLocalMapPoints -- every point
 * that is not skipped, once, in the order of its first occurrence in the concatenated lists; *n_local its length.  The result does not depend on the order in which the device runs
 * anything.  CS_ERR_BAD_ARG for an index outside the point table. */
int cs_track_local_points(cs_ctx *ctx, int n_kf, const int *kf_off, const int *kf_mp, int n_points, const uint8_t *skip, int *local_points, int *n_local);
/* Tracking::UpdateLocalKeyFrames (Tracking.cc:2766-2874), on the host.  frame_mp[n_frame] = mCurrentFrame.mvpMapPoints as indices into the point table (-1 none); mp_skip[n_points] =
 * isBad || (whether_dynamic_object && is_dynamic) (clearing a bad point's slot, :2785, stays with the caller); obs_off[n_points + 1] / obs_kf = the key frames of GetObservations();
 * kf_bad[n_kf] = isBad; cov_off / cov_kf = mvpOrderedConnectedKeyFrames per key frame (its first ten are used); child_off / child_kf = GetChilds(); parent[n_kf] = GetParent() or -1.
 * The reference walks a std::map<KeyFrame*, int> and a std::set<KeyFrame*> in pointer order; that order is defined here as ascending index in the key-frame table (children: as
 * listed).  local_kf (room for n_kf) / *n_local = mvpLocalKeyFrames; *n_local = -1: no key frame received a vote, the reference returns early and the caller keeps its lists.
 * *kf_max = pKFmax (-1: mpReferenceKF stays). */
int cs_track_local_keyframes(int n_frame, const int *frame_mp, int n_points, const uint8_t *mp_skip, const int *obs_off, const int *obs_kf, int n_kf, const uint8_t *kf_bad,
                             const int *cov_off, const int *cov_kf, const int *child_off, const int *child_kf, const int *parent, int *local_kf, int *n_local, int *kf_max);
/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:1141-1371).  m1 / m2 hold KF1 / KF2 (two different matchers); point i of side k is the map
 * point of key point i of KFk (n_k = its key point count); skip1[i] = !pMP || vbAlreadyMatched1[i] || isBad, skip2 likewise (:1171-1181 stay with the caller);
 * train_blocked_k[idx] = !KFk.KeysStatic[idx] (nullable).  R1w, t1w, R2w, t2w = the key frames' poses; sR12 = s12 * R12, sR21 = (1.0 / s12) * R12.t(), t21 = -sR21 * t12 (:1158-1160).
 * The intrinsics are pKF1's for both directions, as in the reference.  matches12[n1]: the key point of KF2 whose map point vpMatches12[i1] receives, -1 none (both directions
 * accept at TH_HIGH and must agree, :1353-1368); *n_found: what the reference returns. */
int cs_match_by_sim3(cs_ctx *ctx, cs_matcher *m1, cs_matcher *m2, const float *R1w, const float *t1w, const float *R2w, const float *t2w, const float *sR12, const float *t12,
                     const float *sR21, const float *t21, int n1, const float *world_pos1, const float *min_distance1, const float *max_distance1, const uint8_t *skip1,
                     const uint8_t *mp_desc1, const uint8_t *train_blocked1 /* nullable */, int n2, const float *world_pos2, const float *min_distance2, const float *max_distance2,
                     const uint8_t *skip2, const uint8_t *mp_desc2, const uint8_t *train_blocked2 /* nullable */, float fx, float fy, float cx, float cy, float log_scale_factor,
                     const float *scale_factors, int n_levels, float th, int *matches12, int *n_found, int *n_level_outside /* nullable */);
/* ORBmatcher::SearchForTriangulation (ORBmatcher.cc:679-850).  node1 / node2: vocabulary node of every feature (the DBoW2 FeatureVector
 * built by KeyFrame::ComputeBoW, -1 = none: the `node` array of cs_bow_transform); skip = the feature already has a map point (or is
 * not static); u_right < 0 = monocular; F12 row-major 3x3 (float), (ex, ey) the epipole of KF1's centre in KF2 (:686-692).
 * matches12[N1] = index in KF2 or -1 (vMatchedPairs = the pairs with matches12 >= 0). */
int cs_match_for_triangulation(cs_ctx *ctx, const cs_keypoint *keys1Un, const uint8_t *desc1, int N1, const int *node1, const uint8_t *skip1, const float *u_right1,
                               const cs_keypoint *keys2Un, const uint8_t *desc2, int N2, const int *node2, const uint8_t *skip2, const float *u_right2,
                               const float *F12, float ex, float ey, const float *scale_factors2, const float *level_sigma2_2, int n_levels, int only_stereo,
                               int check_orientation, int *matches12, int *nmatches);
/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:171-310): node = vocabulary node of every feature
 * (-1 none: the `node` array of cs_bow_transform); skipKF = no usable map point (NULL / bad / dynamic / not static); skipF (nullable) = !KeysStatic.
 * matchesF[NF] = index of the key-frame feature whose map point the frame feature receives, -1 none. */
int cs_match_by_bow(cs_ctx *ctx, const cs_keypoint *keysKF, const uint8_t *descKF, int NK, const int *nodeKF, const uint8_t *skipKF, const cs_keypoint *keysF,
                    const uint8_t *descF, int NF, const int *nodeF, const uint8_t *skipF, float nnratio, int check_orientation, int *matchesF, int *nmatches);
/* ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12) (ORBmatcher.cc:544-677), the loop-closing overload: skip1 / skip2 =
 * the feature has no usable map point (NULL or isBad, :580-584, :598-603); a KF2 feature is claimed once (vbMatched2); the acceptance
 * test is bestDist1 < TH_LOW (strict here, :625) and the ratio test; the rotation histogram holds KF1 indices.  matches12[N1] = index
 * of the KF2 feature whose map point vpMatches12[idx1] receives, -1 none. */
int cs_match_by_bow_kf(cs_ctx *ctx, const cs_keypoint *keys1, const uint8_t *desc1, int N1, const int *node1, const uint8_t *skip1, const cs_keypoint *keys2,
                       const uint8_t *desc2, int N2, const int *node2, const uint8_t *skip2, float nnratio, int check_orientation, int *matches12, int *nmatches);
/* ORBmatcher::DescriptorDistance over all pairs: exact best / second-best per query (first index wins ties). */
int cs_hamming_knn2(cs_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int *best_idx, int *best_dist, int *second_dist);

/* ===================================================================== object bundle adjustment
 * Replaces the g2o machinery behind ORB_SLAM2::Optimizer::BundleAdjustment (orb_object_slam/include/Optimizer.h:39-41,
 * src/Optimizer.cc:64-251) and Optimizer::LocalBACameraPointObjects (:826-1534): SparseOptimizer::optimize with
 * OptimizationAlgorithmLevenberg + BlockSolver_6_3 (Schur) (vendored g2o core/optimization_algorithm_levenberg.cpp:61-189,
 * core/block_solver.hpp:143-604) over VertexSE3Expmap / VertexSBAPointXYZ / VertexCuboidFixScale vertices and
 * EdgeSE3ProjectXYZ / EdgeSE3CuboidFixScaleProj / EdgePointCuboidOnlyObjectFixScale edges (types_six_dof_expmap.*,
 * orb_object_slam/include/g2o_Object.h, src/g2o_Object.cpp).  Residuals, Jacobians (analytic for reprojection, central
 * differences with delta 1e-9 for the cuboid edges, as g2o does), Hessian blocks, the block-Schur reduction, the reduced
 * solve (block-band Cholesky) and the landmark back-substitution run on the GPU; the LM control loop runs on the host.
 * Poses are 7-vectors [tx ty tz qx qy qz qw] (SE3Quat::toVector). */
typedef struct cs_ba_problem {
    int n_cams; const double *cam_pose; const uint8_t *cam_fixed;                /* VertexSE3Expmap, world-to-camera */
    int n_points; const double *points;                                         /* VertexSBAPointXYZ, marginalised */
    int n_cuboids; const double *cuboid_pose; const double *cuboid_scale;       /* VertexCuboidFixScale (pose + fixedscale / scale) */
    const uint8_t *cuboid_flags;  /* bit0 whether_fixrollpitch, bit1 whether_fixrotation, bit2 whether_fixheight, bit3 fixedscale set */
    int n_obs; const int *obs_cam; const int *obs_point; const double *obs_uv; const double *obs_inv_sigma2; /* EdgeSE3ProjectXYZ */
    double fx, fy, cx, cy, huber_mono;                                          /* Huber delta (sqrt(5.991)), 0 = no kernel */
    int n_cobs; const int *cobs_cam; const int *cobs_cuboid; const double *cobs_bbox; const double *cobs_info; /* EdgeSE3CuboidFixScaleProj */
    double K[9], huber_obj;
    int n_pc; const int *pc_cuboid; const int *pc_offsets; const double *pc_points; double max_outside_margin_ratio; /* EdgePointCuboidOnlyObjectFixScale */
    /* EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.h:195-232, Optimizer.cc:158-184): obs_ur[o] >= 0 makes observation o a stereo edge
     * (u, v, u_right) with information inv_sigma2 * I3 and Huber(huber_stereo = sqrt(7.815)); NULL = all monocular */
    const double *obs_ur; double bf, huber_stereo;
} cs_ba_problem;

typedef struct cs_ba_stats {
    int iterations;            /* calls of OptimizationAlgorithmLevenberg::solve executed */
    int lm_trials;             /* linear solves (accepted + rejected trials) */
    double chi2_init, chi2_final, lambda_final;
    double chi2_trace[64];
} cs_ba_stats;

typedef struct cs_ba cs_ba;
/* all-reduce(sum) of n doubles in device memory across the ranks of a multi-GPU run; NULL for a single GPU */
typedef int (*cs_allreduce_fn)(void *user, double *device_buf, long n);

/* Builds the solver structure (index mapping, Schur pattern, ordering; BlockSolver::buildStructure) and uploads the graph.
 * rank/world: landmarks (and their observations) are sharded across `world` ranks, cameras and cuboids are replicated;
 * with world > 1 an all-reduce callback must be set.
 * Every argument is checked before anything is allocated (ba_plan_check of csrc/ba_plan.h).  CS_ERR_BAD_ARG: a NULL argument, rank outside
 * 0..world-1, n_cams < 1, a negative count, an array that is NULL while its count is positive, obs_cam / obs_point / cobs_cam / cobs_cuboid /
 * pc_cuboid outside its table, pc_offsets that do not start at 0 or decrease, no free camera and no cuboid.  (A pc_cuboid out of range, bad
 * pc_offsets and NULL arrays used to read or write out of bounds on the host; valid problems are planned exactly as before.)
 * CS_ERR_CAPACITY: CUBESLAM_BA_SOLVER=band / band1 on a camera system that is not narrow-banded, or a sparse factor whose widest column
 * does not fit the LDS; cs_last_error() says which. */
int cs_ba_create(cs_ctx *ctx, const cs_ba_problem *p, int rank, int world, cs_ba **out);
void cs_ba_destroy(cs_ctx *ctx, cs_ba *b);
int cs_ba_set_allreduce(cs_ba *b, cs_allreduce_fn fn, void *user);
/* SparseOptimizer::optimize(iterations).  stop_flag (may be NULL) is polled between iterations and LM trials like g2o's forceStopFlag
 * (sparse_optimizer.cpp:376, optimization_algorithm_levenberg.cpp:149). */
int cs_ba_optimize(cs_ctx *ctx, cs_ba *b, int iterations, const volatile int *stop_flag, cs_ba_stats *stats);
/* SparseOptimizer::setForceStopFlag(bool*) (Optimizer.cc:80-81, 943-944): a second flag, ONE BYTE wide -- the C++ `bool` another thread of the
 * caller raises (LocalMapping::InterruptBA, mbStopGBA) -- polled at the same points of every later cs_ba_optimize on this graph; NULL removes it. */
int cs_ba_set_stop_flag_bool(cs_ba *b, const volatile unsigned char *flag);
/* current estimates (any pointer may be NULL) */
int cs_ba_read(cs_ctx *ctx, cs_ba *b, double *cam_pose, double *points, double *cuboid_pose);
/* computeActiveErrors + activeRobustChi2 at the current estimates (this rank's share when sharded); err_* may be NULL */
int cs_ba_errors(cs_ctx *ctx, cs_ba *b, double *chi2, double *err_obs, double *err_cobs, double *err_pc);
/* Dense copy of this rank's reduced camera system (before the all-reduce) for lambda: H (6P x 6P row-major), b (6P); *P out */
int cs_ba_reduced_dense(cs_ctx *ctx, cs_ba *b, double lambda, double *H, double *bvec, int *P);

/* ===================================================================== dynamic-object bundle adjustment
 * Replaces the g2o machinery behind ORB_SLAM2::Optimizer::LocalBACameraPointObjectsDynamic (orb_object_slam/include/Optimizer.h:57-58,
 * src/Optimizer.cc:1537-2573): SparseOptimizer::optimize with OptimizationAlgorithmLevenberg + BlockSolverX + LinearSolverDense (:1670-1678)
 * over VertexSE3Expmap (key frames), one VertexCuboidFixScale per (object, key frame) (:1729-1786), VelocityPlanarVelocity (:2160-2165),
 * static VertexSBAPointXYZ (world frame, :1819-1830) and dynamic ones (object frame, :1934-1945), both marginalised, and the edges
 * EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ (:1843-1906), UnaryLocalPoint (:1947-1955), EdgeDynamicPointCuboidCamera (:1977-1993),
 * EdgePointCuboidOnlyObjectFixScale (:2096-2115), EdgeObjectMotion (:2192-2202), EdgeSE3CuboidFixScaleProj (:2279-2298)
 * (orb_object_slam/include/g2o_Object.h, src/g2o_Object.cpp).  The caller builds the graph (the map bookkeeping of :1540-1665 stays in the
 * reference) and flattens it into the arrays below; indices refer to these arrays.  *_level[o] != 0 = setLevel(1) (NULL: all zero);
 * obs_ur NULL or < 0 = monocular; every information matrix of the reference is diagonal.  The two stages of :2353-2415 are two handles:
 * optimize(5), read + errors, then a second problem with the levels / removed kernels, optimize(10). */
typedef struct cs_ba_dyn_problem {
    int n_cams; const double *cam_pose; const uint8_t *cam_fixed;                               /* world-to-camera 7-vectors */
    int n_objs; const double *obj_pose; const double *obj_scale; const uint8_t *obj_flags;      /* object-to-world; flags as in cs_ba_problem */
    int n_vels; const double *vel;                                                              /* [linear velocity, steering angle] */
    int n_points; const double *points;
    int n_dpoints; const double *dpoints;                                                       /* MapPoint::PosToObj */
    int fix_points;                                                                             /* fixPoint: setFixed(true) instead of setMarginalized(true) */
    int n_obs; const int *obs_cam; const int *obs_point; const double *obs_uv; const double *obs_ur; const double *obs_inv_sigma2; const uint8_t *obs_level;
    double fx, fy, cx, cy, bf, huber_mono, huber_stereo;
    double ulp_info, ulp_scale[3], ulp_ratio;                                                   /* UnaryLocalPoint: info * I, objectscale, max_outside_margin_ratio */
    int n_dobs; const int *dobs_cam; const int *dobs_obj; const int *dobs_point; const double *dobs_uv; const double *dobs_inv_sigma2; const uint8_t *dobs_level;
    double K[9], huber_dyn;
    int n_mot; const int *mot_from; const int *mot_to; const int *mot_vel; const double *mot_dt; double mot_info[3];
    int n_cobs; const int *cobs_cam; const int *cobs_obj; const double *cobs_bbox; const double *cobs_info; const uint8_t *cobs_level; double huber_obj;
    int n_pc; const int *pc_obj; const int *pc_offsets; const double *pc_points; double pc_ratio;
} cs_ba_dyn_problem;

typedef struct cs_ba_dyn cs_ba_dyn;
/* initializeOptimization: index mapping (non-fixed cameras, object poses, velocities; landmarks = static then dynamic points), the
 * pose-landmark slot lists, upload.  CS_ERR_BAD_ARG for an index out of range or a pose system above 4000 scalars. */
int cs_ba_dyn_create(cs_ctx *ctx, const cs_ba_dyn_problem *p, cs_ba_dyn **out);
void cs_ba_dyn_destroy(cs_ctx *ctx, cs_ba_dyn *b);
/* SparseOptimizer::optimize(iterations); stop_flag as in cs_ba_optimize */
int cs_ba_dyn_optimize(cs_ctx *ctx, cs_ba_dyn *b, int iterations, const volatile int *stop_flag, cs_ba_stats *stats);
int cs_ba_dyn_set_stop_flag_bool(cs_ba_dyn *b, const volatile unsigned char *flag); /* as cs_ba_set_stop_flag_bool */
/* current estimates (any pointer may be NULL) */
int cs_ba_dyn_read(cs_ctx *ctx, cs_ba_dyn *b, double *cam_pose, double *obj_pose, double *vel, double *points, double *dpoints);
/* computeError of every edge + activeRobustChi2 over the active ones: e_obs n x 3 (third 0 for mono), e_dobs n x 2, e_mot n x 3,
 * e_cobs n x 4, e_pc n x 3, e_ulp n_dpoints x 3; any output may be NULL */
int cs_ba_dyn_errors(cs_ctx *ctx, cs_ba_dyn *b, double *chi2, double *e_obs, double *e_dobs, double *e_mot, double *e_cobs, double *e_pc, double *e_ulp);
/* dense reduced pose system for lambda at the current estimates: H (n x n row-major), bvec (n); *n out (H NULL: query) */
int cs_ba_dyn_reduced_dense(cs_ctx *ctx, cs_ba_dyn *b, double lambda, double *H, double *bvec, int *n);

/* ===================================================================== LSD line detector
 * Replaces line_lbd_detect::detect_raw_lines / detect_filter_lines (line_lbd/include/line_lbd/line_lbd_allclass.h:37-52,
 * class/line_lbd_allclass.cpp:125-148,200-221) with use_LSD = true, one octave: LSDDetector::detectImpl
 * (libs/LSDDetector.cpp:153-287) over LineSegmentDetectorImpl (libs/lsd.cpp; LSD_REFINE_ADV, default parameters).
 * GPU: Gaussian blur + 0.8x bilinear resize in double, level-line angles and gradient norms (ll_angle).  Host (one thread
 * per frame): the pseudo-ordering and the inherently sequential region growing / rectangle / NFA stages. */
typedef struct cs_keyline {              /* the KeyLine fields (line_descriptor/descriptor.hpp:105-150) */
    float angle; int32_t class_id; int32_t octave; float pt_x, pt_y; float response; float size;
    float startPointX, startPointY, endPointX, endPointY;
    float sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
    float lineLength; int32_t numOfPixels;
} cs_keyline;
typedef struct cs_lsd cs_lsd;
int cs_lsd_create(cs_ctx *ctx, int width, int height, int max_frames, cs_lsd **out);
void cs_lsd_destroy(cs_ctx *ctx, cs_lsd *l);
/* detect_raw_lines on n_frames gray images: per frame counts[f] KeyLines at out[f*cap_per_frame ...] */
int cs_lsd_detect(cs_ctx *ctx, cs_lsd *l, const uint8_t *gray, int n_frames, int stride, cs_keyline *out, int cap_per_frame, int *counts);
/* detect_filter_lines(gray, linesmat): octave 0, lineLength > length_thres; lines: [f][cap_per_frame][4] floats (CV_32F N x 4) */
int cs_lsd_detect_filter_lines(cs_ctx *ctx, cs_lsd *l, const uint8_t *gray, int n_frames, int stride, float length_thres,
                               float *lines, int cap_per_frame, int *counts);
/* the same rows from the KeyLines of the last cs_lsd_run over the resident frames (counts[f] rows of frame f at lines + f * cap * 4); n_frames: the frames
 * `lines` and `counts` have room for -- CS_ERR_BAD_ARG when the last run processed more */
int cs_lsd_read_filter_lines(cs_ctx *ctx, cs_lsd *l, float length_thres, float *lines, int cap, int *counts, int n_frames);
/* introspection after a detect call: scaled image, gradient norm and level-line angle maps (sw x sh doubles each) */
int cs_lsd_get_maps(cs_ctx *ctx, cs_lsd *l, int frame, double *scaled, double *modgrad, double *angles, int *sw, int *sh);

/* Resident-batch form of the line front-end (what bench.py times): frames stay in HBM; cs_lsd_run detects the KeyLines of every
 * uploaded frame and, with_lbd != 0, their LBD descriptors (= line_lbd_detect::detect_descrip_lines before its length filter,
 * class/line_lbd_allclass.cpp:222-256); cs_lsd_read returns one frame's lines (out == NULL: count only) and descriptors. */
int cs_lsd_upload(cs_ctx *ctx, cs_lsd *l, const uint8_t *gray, int n_frames, int stride);
int cs_lsd_run(cs_ctx *ctx, cs_lsd *l, int with_lbd);
/* The region stage (lsd.cpp:464-535: region_grow ... rect_improve) of the last batch.  Batches of 512 frames and more run it on the device, one
 * wave per frame walking the reference's sequence (cube_slam_amd/csrc/lsd_regions.hip); smaller ones on the host's cores, one frame per thread;
 * cs_lsd_set_region_stage picks the stage for a detector's later runs.  Every stage gives the same KeyLines byte for byte.
 * out[0] 1 when the device stage was chosen, out[1] region_grow calls, out[2] rectangles that reached rect_improve,
 * out[3] 1 when the batch fell back to the host stage (a region larger than the device list), out[4] pixel-window fetches.  All 0 for the host stage. */
int cs_lsd_region_stats(cs_ctx *ctx, cs_lsd *l, long out[5]);
/* Which formulation of the region stage the detector's next runs take:
 *   CS_LSD_REGIONS_AUTO            the host stage below 512 frames per run, one wave per frame from 512 on (the default);
 *   CS_LSD_REGIONS_HOST            one frame per host thread (a frame: ~3.5 ms);
 *   CS_LSD_REGIONS_WAVE_PER_FRAME  one wave walks a frame's sequence (~110 ms per frame whatever the batch; 36 k frames/s with the chip full of frames);
 *   CS_LSD_REGIONS_BACKLOG         a walker lane per frame + rectangle waves (64 frames per wave slot, ~450 ms per frame, 134 k frames/s with the chip full): for an offline
 *                                  backlog of tens of thousands of frames whose lines nobody waits for. */
enum { CS_LSD_REGIONS_AUTO = 0, CS_LSD_REGIONS_HOST = 1, CS_LSD_REGIONS_WAVE_PER_FRAME = 2, CS_LSD_REGIONS_BACKLOG = 3 };
int cs_lsd_set_region_stage(cs_lsd *l, int stage);
int cs_lsd_read(cs_ctx *ctx, cs_lsd *l, int frame, cs_keyline *out, int cap, int *count, uint8_t *desc /* cap x 32 or NULL */);

/* ===================================================================== LBD line descriptor + matcher
 * Replaces BinaryDescriptor::compute (line_lbd/libs/binary_descriptor.cpp:588-790,1146-1509; what
 * line_lbd_detect::get_line_descriptors / detect_descrip_lines call, class/line_lbd_allclass.cpp:192-269) for one octave, and
 * line_lbd_detect::match_line_descrip (:339-356) = BinaryDescriptorMatcher::match (exact 1-NN in 256-bit Hamming space,
 * libs/binary_descriptor_matcher.cpp:196-262) followed by the distance threshold. */
int cs_lbd_compute(cs_ctx *ctx, const uint8_t *gray, int width, int height, int stride, const cs_keyline *keylines, int n,
                   uint8_t *desc /* n x 32 */, float *float_desc /* n x 72 or NULL */);
/* good matches: for every query whose nearest train descriptor is closer than dist_thres: (query, train, distance) */
int cs_lbd_match(cs_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, float dist_thres,
                 int *query_idx, int *train_idx, int *distance, int *n_matches);
/* introspection: the blurred image and the Sobel derivative maps of the last cs_lbd_compute-like pass over `gray` */
int cs_lbd_maps(cs_ctx *ctx, const uint8_t *gray, int width, int height, int stride, uint8_t *blur, int16_t *dx, int16_t *dy);

/* ===================================================================== Optimizer::PoseOptimization  
 * Replaces ORB_SLAM2::Optimizer::PoseOptimization(Frame*) (orb_object_slam/include/Optimizer.h:51, src/Optimizer.cc:253-472) for a
 * batch of frames: frame f owns the matches [edge_off[f], edge_off[f+1]) -- Xw (world point), obs (u, v, u_right; u_right < 0 =
 * monocular, Optimizer.cc:303), inv_sigma2 (mvInvLevelSigma2[octave]); intrinsics n_frames x 5 = fx fy cx cy bf; poses = Tcw as
 * [t, qx qy qz qw].  Out: optimised pose, per-match mvbOutlier flags, n_inliers[f] = nInitialCorrespondences - nBad (:471).
 * One workgroup per frame runs the 4 x 10 Levenberg-Marquardt rounds with the re-classification in between. */
int cs_pose_optimization(cs_ctx *ctx, int n_frames, const int *edge_off, const double *Xw, const double *obs, const double *inv_sigma2, const double *intrinsics,
                         const double *pose_in, double *pose_out, uint8_t *outlier, int *n_inliers);

/* ===================================================================== Optimizer::OptimizeSim3
 * Replaces ORB_SLAM2::Optimizer::OptimizeSim3(KeyFrame*, KeyFrame*, vector<MapPoint*>&, g2o::Sim3&, float, bool) (orb_object_slam/include/Optimizer.h,
 * src/Optimizer.cc:2838-3033) for a batch of problems: problem f owns the correspondences [corr_off[f], corr_off[f+1]) that survive the filter of :2893-2928
 * (vpMatches1[i] set, neither point bad, i2 >= 0), in the order of i.  P1c / P2c (3 each) are R1w * P3D1w + t1w and R2w * P3D2w + t2w as the reference's float
 * cv::Mat computes them (:2910, :2918); obs1 / obs2 (2 each) are mvKeysUn[i].pt of pKF1 and mvKeysUn[i2].pt of pKF2; inv_sigma2_* are mvInvLevelSigma2[octave] of
 * those key points; intrinsics n_problems x 8 = fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2; sim3_in n_problems x 8 = tx ty tz qx qy qz qw s, the coefficients g2o::Sim3 holds,
 * NOT normalised; th2 and fix_scale per problem.  Out: sim3_out (g2oS12; equal to sim3_in bit for bit where the function returns before writing it, :3003-3004),
 * removed[c] = 1 where the reference sets vpMatches1[idx] = NULL, n_inliers[f] = the return value.  One workgroup per problem runs optimize(5), the cut, and
 * optimize(10 or 5) with g2o's numeric Jacobians and Levenberg-Marquardt schedule in one launch.
 * corr_off[0] must be 0 and the offsets must not decrease, as for every batched entry; CS_ERR_BAD_ARG otherwise, for n_problems < 0, and for a NULL array that the
 * sizes say is read or written.  A refusal launches nothing and leaves sim3_out, removed and n_inliers as they were; n_problems == 0 succeeds and reads nothing. */
int cs_sim3_optimization(cs_ctx *ctx, int n_problems, const int *corr_off, const double *P1c, const double *P2c, const double *obs1, const double *obs2,
                         const double *inv_sigma2_1, const double *inv_sigma2_2, const double *intrinsics, const double *sim3_in, const float *th2,
                         const uint8_t *fix_scale, double *sim3_out, uint8_t *removed, int *n_inliers);

/* ===================================================================== Optimizer::OptimizeEssentialGraph
 * Replaces ORB_SLAM2::Optimizer::OptimizeEssentialGraph(Map*, KeyFrame*, KeyFrame*, const KeyFrameAndPose&, const KeyFrameAndPose&, const map<KeyFrame*,
 * set<KeyFrame*>>&, const bool&) (orb_object_slam/include/Optimizer.h, src/Optimizer.cc:2575-2836): the 7-dof pose graph LoopClosing::CorrectLoop runs over every key
 * frame once a loop is accepted, and the correction of every map point after it.  Sim3 layout as in cs_sim3_optimization: tx ty tz qx qy qz qw s, never normalised.
 *
 * cs_essential_graph_create: vertices are the dense indices 0 .. n_vertices - 1 (the caller maps mnId); edge e is an EdgeSim3 with vertex 0 = edge_i[e] (the key
 * frame the reference is visiting) and vertex 1 = edge_j[e], in the order the reference inserts them; edge_kind[e] = 0 for a loop-connection edge (:2645-2673, the
 * measurement from vScw on both ends), 1 for a spanning-tree, stored-loop or covisibility edge (:2676-2776, each end from NonCorrectedSim3 where it has an entry);
 * fixed_vertex is pLoopKF (:2628-2629); fix_scale is bFixScale.  Everything that depends on the structure alone is done here, once, on the host: incidence lists in
 * edge order, one slot per connected pair, a minimum-degree order, the elimination tree with its level sets and the structure of L.
 * CS_ERR_BAD_ARG: n_vertices < 2, n_edges < 1, an index out of range, edge_i[e] == edge_j[e], edge_kind outside {0, 1}.
 *
 * cs_essential_graph_optimize: Scw = vScw, the initial estimates (:2612-2626); Snc / has_nc = NonCorrectedSim3 (rows without an entry are not read).  The
 * measurements Sji = Sjw * Swi are computed by the library.  `iterations` Levenberg-Marquardt iterations (the reference runs 20) with setUserLambdaInit(1e-16), g2o's
 * numeric Jacobians (delta 1e-9) and information I.  Out: sim3_out n x 8 (the estimates; the fixed vertex as it came), Tiw_out n x 12 floats = the rows of
 * [R | t / s] that Converter::toCvSE3 stores (:2794-2800), stats (nullable).  Per LM trial the host reads one record of four doubles. */
#define CS_EG_MAX_TRIALS 256
typedef struct cs_essential_graph cs_essential_graph;
typedef struct cs_essential_graph_stats {
    int iterations, trials, accepted, rejected; /* iterations entered; LM trials; of those, accepted and undone */
    int levels, l_blocks, h_blocks;             /* height of the elimination tree; 7 x 7 blocks of L and of the lower triangle of H, diagonal included */
    int launches_per_trial;
    double chi2_first, chi2_last, lambda_last;
    uint8_t trial_accepted[CS_EG_MAX_TRIALS];   /* the first CS_EG_MAX_TRIALS trials in order: 1 accepted, 0 undone */
} cs_essential_graph_stats;
int cs_essential_graph_create(cs_ctx *ctx, int n_vertices, int n_edges, const int *edge_i, const int *edge_j, const uint8_t *edge_kind, int fixed_vertex, int fix_scale,
                              cs_essential_graph **out);
int cs_essential_graph_optimize(cs_ctx *ctx, cs_essential_graph *eg, const double *Scw, const double *Snc, const uint8_t *has_nc, int iterations, double *sim3_out,
                                float *Tiw_out, cs_essential_graph_stats *stats);
void cs_essential_graph_destroy(cs_essential_graph *eg);
/* The point correction of :2824-2831: P_out[p] = (float) correctedSwr.map(Srw.map(P[p])) with Srw = Scw[ref_vertex[p]] and correctedSwr = sim3_out[ref_vertex[p]].inverse();
 * P is Converter::toVector3d of the float position, ref_vertex the index of nIDr (:2813-2822, the caller's choice).  UpdateNormalAndDepth stays with the caller.
 * CS_ERR_BAD_ARG and no launch where a ref_vertex is out of range. */
int cs_sim3_correct_points(cs_ctx *ctx, int n_points, const double *P, const int *ref_vertex, int n_vertices, const double *Scw, const double *sim3_out, float *P_out);
/* Sim3::log (sim3.h:148-230) of n transforms -> n x 7 (omega, upsilon, sigma): a probe of the device function under the pose graph's error, for tests. */
int cs_sim3_log(cs_ctx *ctx, int n, const double *sim3, double *log_out);

/* ===================================================================== batch front-end runner
 * One pass of the per-frame path (ORBextractor::operator(), line_lbd_detect::detect_descrip_lines, detect_3d_cuboid::detect_cuboid --
 * what Tracking / main_obj.cpp call per frame, object_slam/src/main_obj.cpp:395-470) over a batch that is resident in HBM.  Handles
 * are borrowed: orb / batch run on `ctx` in the calling thread, every line detector on its own context in a worker thread; with two
 * detectors (both holding the same frames) consecutive passes alternate between them, so the host stage of LSD overlaps GPU work.
 * cs_frontend_step returns when ORB and the cuboid batch of this pass are done; cs_frontend_drain waits for the line passes.
 * Streams: the caller's, one per line detector and, for batches whose region stage runs on the device, one lowest-priority background stream per detector for
 * that stage's one long kernel, which the detector's worker thread waits for on the host: no stream waits for it on the device.  The HIP runtime creates four
 * hardware queues per stream priority by default and runs the streams that share one in launch order, so their short kernels do not overlap: export
 * GPU_MAX_HW_QUEUES=16 (or more) before the runtime starts in a process that uses the runner. */
typedef struct cs_frontend cs_frontend;
int cs_frontend_create(cs_ctx *ctx, cs_orb *orb /* nullable */, cs_cuboid_batch *batch /* nullable */, int n_line_workers, cs_ctx *const *line_ctx,
                       cs_lsd *const *lsd, cs_frontend **out);
/* 1: the process offers at least as many hardware queues (GPU_MAX_HW_QUEUES as the process saw it at cs_frontend_create, 4 when unset) as the runner keeps streams
 * busy (1 + 2 per line worker); 0: it does not -- cs_frontend_create has said so on stderr -- and streams that share a queue run their short kernels one after
 * the other (none of them is held up for the length of a region walk: the wait for a walk is the worker thread's, not a stream's); < 0: error. */
int cs_frontend_queues(const cs_frontend *fe, int *streams, int *hw_queues);
int cs_frontend_step(cs_frontend *fe);
int cs_frontend_drain(cs_frontend *fe);
/* Streaming source: the frames of every step arrive from the HOST (main_obj.cpp:420-449 / Frame.cc:320-326 take a new image per call) instead of staying resident.
 * cs_frontend_stream_begin gives the runner a ring of n_slots (2..8) device slots of n_frames x height x width bytes and a copy stream of its own;
 * cs_frontend_stream_push(gray) enqueues the H2D copy of the frames of the next step that has none yet (pinned host memory: asynchronous; it waits on the device for the
 * slot's last readers, on the host only for the line pass that last used the slot to have taken its frames) -- push step k + 1 before calling step k and the upload
 * overlaps step k; cs_frontend_step then feeds ORB, the cuboid batch (same boxes / poses / plan, new pixels) and the step's line pass from the slot by device copies.
 * A step without pushed frames is CS_ERR_BAD_ARG, a push with every slot waiting for its step CS_ERR_CAPACITY.  Not with phased passes.  cs_frontend_stream_end drains
 * and returns to resident frames. */
int cs_frontend_stream_begin(cs_frontend *fe, int n_frames, int width, int height, int n_slots);
int cs_frontend_stream_push(cs_frontend *fe, const uint8_t *gray);
/* ... with what detect_cuboid takes beside the pixels (detect_3d_cuboid/include/detect_3d_cuboid/detect_3d_cuboid.h:62-63, object_slam/src/main_obj.cpp:420-449): the
 * frames' camera poses (n_frames x 16), their 2-D boxes (box_offsets[n_frames + 1], rows of 5) and their edge lists (line_offsets NULL: the batch's lists stay).  The step that takes the slot hands them to the cuboid batch (cs_cuboid_batch_set_scene: the plan is rebuilt for them). */
int cs_frontend_stream_push_scene(cs_frontend *fe, const uint8_t *gray, const double *Twc, const int *box_offsets, const double *boxes, const int *line_offsets, const double *lines);
int cs_frontend_stream_end(cs_frontend *fe);
/* The results of the step that has just been enqueued, copied to the caller's (pinned) buffers on a copy stream of the ring behind the step's kernels: ORB key points /
 * descriptors packed like cs_orb_read_packed (first / total are filled at once), the cuboids like cs_cuboid_batch_read; either pair may be NULL.  Returns at once; the next
 * step's kernels wait on the device for the copies before they overwrite what is read; cs_frontend_stream_read_wait blocks until the copies of the last call have arrived
 * (and reports the batch's status).  One call per step at most. */
int cs_frontend_stream_read_async(cs_frontend *fe, cs_keypoint *kps, uint8_t *desc, long cap_total, int *first, long *total, cs_cuboid *cuboids, int *counts);
int cs_frontend_stream_read_wait(cs_frontend *fe);
/* the device-side hand-overs the streaming source uses (a copy on the context's stream, nothing waits): frames one behind the other, rows of `width` bytes */
int cs_orb_set_frames_device(cs_ctx *ctx, cs_orb *e, const uint8_t *d_gray, int n_frames);
int cs_lsd_set_frames_device(cs_ctx *ctx, cs_lsd *l, const uint8_t *d_gray, int n_frames);
int cs_cuboid_batch_set_gray_device(cs_ctx *ctx, cs_cuboid_batch *b, const uint8_t *d_gray);
/* Phased passes (off by default; results are the same either way).  With the device region stage of LSD (batches of >= 512 frames) a
 * super-step = one pass per line detector: the detectors stop in front of the region stage, and after the last pass of the super-step
 * (or at cs_frontend_drain) the region stages of all of them run together while `ctx`'s stream is idle -- that cs_frontend_step
 * returns when they have left the GPU.  The cuboid score kernel and the one-wave-per-frame region kernel then never share a CU. */
int cs_frontend_set_phased(cs_frontend *fe, int on);
/* The reference's chain (object_slam/src/main_obj.cpp:428-449: detect_cuboid consumes this frame's detect_filter_lines) as a pipeline: on != 0 makes
 * step k hand the lines of line pass k - W (octave 0, lineLength > length_thres; line pass k belongs to step k, W = number of line workers) to the cuboid
 * batch before that batch runs: a pass that was started at least W steps earlier, so in the steady state no step waits for a line pass.  The first W steps
 * after the switch run on the lists the batch holds.  Needs a cuboid batch and >= 1 line worker. */
int cs_frontend_set_chain(cs_frontend *fe, int on, float length_thres);
/* A backlog: `n_steps` more cs_frontend_step calls will follow on the frames the detectors hold.  The line passes of those steps are then started as soon as a
 * worker is free -- at most 2 W passes ahead of the caller's step -- instead of one per step, so the line pipeline is full from the first step and does not
 * drain behind the last one.  Nothing is added or dropped: step k still needs line pass k to have been started, cs_frontend_drain waits for every pass in
 * flight and cuts what is left of the backlog (passes already done are found done by the steps that follow).  No effect on phased passes. */
int cs_frontend_set_backlog(cs_frontend *fe, int n_steps);
/* The cuboid batch on a stream of its own: its launches (no host round trip among them) are enqueued on `cuboid_ctx` and run beside the ORB pass of the same step
 * instead of in front of the next one.  NULL: back onto the caller's stream.  cs_frontend_drain waits for that stream too. */
int cs_frontend_set_cuboid_ctx(cs_frontend *fe, cs_ctx *cuboid_ctx);
void cs_frontend_destroy(cs_frontend *fe);

/* ===================================================================== 9-dof g2o::cuboid of object_slam
 * Replaces, for batches, g2o::VertexCuboid::oplusImpl (object_slam/include/object_slam/g2o_Object.h:193-204: pose * exp(update[0:6]),
 * scale + update[6:9]) and g2o::EdgeSE3Cuboid::computeError (:227-252: cuboid::min_log_error of the measured cuboid moved to the
 * world by the camera, :77-101) with the numeric Jacobians BaseBinaryEdge::linearizeOplus builds for it (central differences, 1e-9;
 * Jcam n x 9 x 6, Jcub n x 9 x 9, row-major; pass both NULL for residuals only).  cuboid = [t, qx qy qz qw, half scale] (10 doubles). */
int cs_cuboid9_oplus(cs_ctx *ctx, int n, const double *cub, const double *upd, double *out);
int cs_cuboid9_edge_linearize(cs_ctx *ctx, int n, const double *cam_Tcw, const double *cub_global, const double *cub_meas_local, double *err, double *Jcam, double *Jcub);

/* ===================================================================== object association after detect_cuboid
 * cs_associate_keypoints replaces the keypoint -> local cuboid association of Tracking::DetectCuboid
 * (orb_object_slam/src/Tracking.cc:1717-1775, with bboxOverlapratio detect_3d_cuboid/src/object_3d_util.cpp:650-654) for a batch of
 * keyframes: boxes are cv::Rect (x, y, w, h) of pKF->local_cuboids in order, keypoints mvKeys[i].pt.  Out: keypoint_associate_objectID
 * (index of the single non-overlapped box that contains the rounded keypoint, else -1), keypoint_inany_object (only meaningful with
 * enable_ground_height_scale, may be NULL) and the per-box `overlapped` flags (IoU > 0.15 with an earlier unflagged box, may be NULL).
 * At most 64 boxes per frame. */
int cs_associate_keypoints(cs_ctx *ctx, int n_frames, const int *kp_off, const float *kp_xy, const int *box_off, const int *boxes, int enable_ground_height_scale,
                           int *assoc, uint8_t *inany, uint8_t *overlapped);
/* Tracking::AssociateCuboids (Tracking.cc:1848-1990, use_truth_trackid = false) on index arrays instead of MapObject* / MapPoint*:
 * candidates (cand_id = the id a candidate gets as a landmark, its GetPotentialMapPoints() as CSR cand_off / cand_pts) are taken
 * in order against LocalObjectsLandmarks (landmark_id, landmark_bad = isBad()), counting for every landmark the candidate's points
 * whose MapObjObservations (CSR pobs_off / pobs_obj / pobs_cnt, pobs_cnt NULL = all 1) contain it; the first landmark in list
 * order with the strictly largest count above the threshold absorbs the candidate (MergeIntoLandmark), otherwise the candidate
 * becomes a landmark (SetAsLandmark) and joins the list before the NEXT candidate; both add one vote per point
 * (MapPoint::AddObjectObservation, MapPoint.cc:219-242), which later candidates see.  Out: assoc[i] = landmark id candidate i ends
 * up in, created[i]; best_object / max_vote (n_points, in/out, may be NULL) follow the `best_object` bookkeeping of the points;
 * the changed votes come back as (point, object, new count) triples (upd_*, may be NULL; *n_upd = their number).  Host code: the
 * loop is serial by construction. */
int cs_associate_cuboids(int n_cand, const int *cand_id, const int *cand_off, const int *cand_pts, int n_landmarks, const int *landmark_id, const uint8_t *landmark_bad,
                         int n_points, const int *pobs_off, const int *pobs_obj, const int *pobs_cnt, int *best_object, int *max_vote, int largest_shared_num_points_thres,
                         int *assoc, uint8_t *created, int upd_cap, int *upd_point, int *upd_obj, int *upd_cnt, int *n_upd);

/* ===================================================================== place recognition: DBoW2 transform and key-frame database
 * Replaces what comes before the loop-closing and relocalisation searches: Frame::ComputeBoW / KeyFrame::ComputeBoW (orb_object_slam/src/Frame.cc:537-544,
 * KeyFrame.cc:81-90: TemplatedVocabulary::transform(features, v, fv, 4), Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1139-1271), the scores of
 * KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:74-305) and of LoopClosing::DetectLoop's minScore loop
 * (LoopClosing.cc:126-140: L1Scoring::score, ScoringObject.cpp:23-68).  Bit-exact: words, nodes, values and scores are the reference's, doubles as 64-bit patterns.
 * Only what the reference's ORBvoc uses is supported: TF_IDF weighting with L1 scoring. */
enum { CS_BOW_TF_IDF = 0, CS_BOW_TF = 1, CS_BOW_IDF = 2, CS_BOW_BINARY = 3 };                                                          /* DBoW2::WeightingType */
enum { CS_BOW_L1_NORM = 0, CS_BOW_L2_NORM = 1, CS_BOW_CHI_SQUARE = 2, CS_BOW_KL = 3, CS_BOW_BHATTACHARYYA = 4, CS_BOW_DOT_PRODUCT = 5 }; /* DBoW2::ScoringType */
typedef struct cs_bow_vocab cs_bow_vocab;
typedef struct cs_bow_db cs_bow_db;
/* The tree as TemplatedVocabulary::loadFromTextFile (:1350-1437) leaves it in m_nodes: node 0 is the root, parent[i] < i, children keep file order, word ids go to the flagged
 * leaves in node-id order, desc = n_nodes x 32 bytes (the root's is not read), levelsup = what transform() is called with (the reference: 4).  CS_ERR_BAD_ARG with *out = NULL
 * for a weighting / scoring other than TF_IDF / L1 and for what leaves the reference undefined: a leaf flag that disagrees with the node having no children, a leaf above
 * level L - levelsup (> 0), k outside 2..20 or L outside 1..10, a parent id that is not smaller than the node's own; also for a node with more than k children. */
int cs_bow_vocab_create(cs_ctx *ctx, int k, int L, int n_nodes, const int *parent, const uint8_t *is_leaf, const uint8_t *desc, const double *weight, int levelsup, int weighting,
                        int scoring, cs_bow_vocab **out);
/* The refusals of cs_bow_vocab_create alone (host code, needs no device): CS_OK or CS_ERR_BAD_ARG. */
int cs_bow_vocab_check(int k, int L, int n_nodes, const int *parent, const uint8_t *is_leaf, int levelsup, int weighting, int scoring);
int cs_bow_vocab_info(const cs_bow_vocab *v, int *k, int *L, int *n_nodes, int *n_words, int *levelsup); /* any pointer may be NULL */
void cs_bow_vocab_destroy(cs_bow_vocab *v);
/* transform() for a batch of frames: the features of frame f are desc[32 * offsets[f]] .. desc[32 * offsets[f + 1]) (offsets[0] = 0, at most 8192 per frame: CS_ERR_CAPACITY).
 * Per feature: word[i] and node[i] (the node at level L - levelsup, the root where that is <= 0), both -1 where the word's weight is not > 0 ("stopped", :1169); node is the
 * array cs_match_by_bow, cs_match_by_bow_kf and cs_match_for_triangulation take.  Per frame: the BowVector as bow_count[f] entries at offsets[f] of bow_word (ascending) and
 * bow_value; the entries behind them, up to offsets[f + 1], are word -1, value 0. */
int cs_bow_transform(cs_ctx *ctx, const cs_bow_vocab *v, int n_frames, const int *offsets, const uint8_t *desc, int *word, int *node, int *bow_count, int *bow_word,
                     double *bow_value);
/* L1Scoring::score(v1 = vector pair_a[p], v2 = vector pair_b[p]) of n_vec BowVectors given as off[n_vec + 1] / word (strictly ascending inside a vector) / value. */
int cs_bow_score(cs_ctx *ctx, int n_vec, const int *off, const int *word, const double *value, int n_pairs, const int *pair_a, const int *pair_b, double *score);
/* The BowVectors of the key frames, resident on the device, each with its id and the order in which it was added (KeyFrameDatabase::add / erase, KeyFrameDatabase.cc:38-66:
 * erasing and adding again moves a key frame to the end of that order).  add of an id that is in the database is CS_ERR_BAD_ARG; erase of one that is not changes nothing. */
int cs_bow_db_create(cs_ctx *ctx, cs_bow_db **out);
int cs_bow_db_add(cs_ctx *ctx, cs_bow_db *db, long id, int n, const int *word, const double *value);
int cs_bow_db_erase(cs_bow_db *db, long id);
int cs_bow_db_clear(cs_bow_db *db);
int cs_bow_db_size(const cs_bow_db *db, int *n_keyframes);
/* For every (query, key frame) that share at least one word, queries ascending and key frames in add order inside a query: the key frame's id and its add-order number, the
 * number of common words, the smallest common word id, and L1Scoring::score(query, key frame).  *n_out = their number; more than `cap`: CS_ERR_CAPACITY (*n_out is still set;
 * n_query * cs_bow_db_size always suffices). */
int cs_bow_db_query(cs_ctx *ctx, cs_bow_db *db, int n_query, const int *q_off, const int *q_word, const double *q_value, long cap, long *n_out, int *out_query, long *out_id,
                    long *out_order, int *out_common, int *out_minword, double *out_score);
void cs_bow_db_destroy(cs_bow_db *db);

/* ===================================================================== local mapping
 * The triangulation loop of ORB_SLAM2::LocalMapping::CreateNewMapPoints (orb_object_slam/src/LocalMapping.cc:319-570) and the per-point upkeep
 * MapPoint::ComputeDistinctiveDescriptors / MapPoint::UpdateNormalAndDepth (MapPoint.cc:381-446, :469-510).
 *
 * CreateNewMapPoints builds its matcher as ORBmatcher(0.6, false): SearchForTriangulation then neither cuts by rotation nor claims key points of the neighbour, so the match of
 * a key point idx1 in a neighbour depends on idx1 and that neighbour alone, and the only coupling between neighbours is pKF1->GetMapPoint(idx1) (ORBmatcher.cc:721-725), non-NULL
 * exactly where an earlier neighbour's triangulation succeeded.  The loop therefore equals: search every neighbour with the INITIAL skip1, triangulate all pairs of all
 * neighbours independently, and per idx1 keep the first neighbour in order whose pair was accepted.  The test :402-407 can never fire: the search has already skipped key points
 * that are not static (skip1 / skip2 of cs_match_for_triangulation), so there is no argument for it. */
typedef struct cs_lm_frame {             /* what :329-344, :381-393 and the loop read of a KeyFrame */
    const cs_keypoint *keysUn;           /* mvKeysUn */
    const float *keys_xy;                /* mvKeys[i].pt as x, y (KeyFrame::UnprojectStereo, KeyFrame.cc:675-691, reads the distorted key point) */
    const float *u_right, *depth;        /* mvuRight, mvDepth */
    int N;
    float Rcw[9], tcw[3], Ow[3];         /* GetRotation(), GetTranslation(), GetCameraCenter() as stored; the library forms Rwc = Rcw.t() and Tcw = [Rcw | tcw], both copies */
    float fx, fy, cx, cy, invfx, invfy, mbf, mb;
    const float *scale_factors, *level_sigma2; /* mvScaleFactors, mvLevelSigma2 */
    int n_levels;
    float scale_factor;                  /* mfScaleFactor (read of the current key frame only: ratioFactor = 1.5f * mfScaleFactor) */
} cs_lm_frame;
/* matches12[n_neigh * N1]: per neighbour the matches12 of cs_match_for_triangulation run with the initial skip1.  The pairs are the entries >= 0, in neighbour order and then
 * idx1 ascending (the order of vMatchedPairs): pair_off[n_neigh + 1] and, per pair, idx1, idx2, x3D[3] and a status byte -- 0 a point is created, else the first test that
 * failed: 1 parallax :467, 2 w == 0 :452, 3 z1 :473, 4 z2 :477, 5 reprojection in the current key frame :492 / :503, 6 in the neighbour :518 / :529, 7 zero distance :540,
 * 8 scale :548, 9 an earlier neighbour created the point of idx1, 10 a stereo key point (u_right >= 0) with depth <= 0 where the reference reads the empty Mat of UnprojectStereo.
 * x3D is 0 0 0 for 1, 2 and 10.  new_pair_of_idx1[N1] = the pair that creates the point of idx1, -1 none; *nnew their number.  The reference creates the points in pair order.
 * cv::SVD and cos(2 * atan2(mb / 2, depth)) are the library's stated definitions (csrc/triangulate_math.h).
 * CS_ERR_BAD_ARG (nothing written, nothing launched): NULL arguments, n_neigh outside 0..32, a matches12 entry >= N2 or < -1, an octave outside 0..n_levels - 1;
 * CS_ERR_CAPACITY (nothing written but pair_off) when there are more than pair_cap pairs. */
#define CS_LM_MAX_NEIGHBOURS 32
int cs_create_new_map_points(cs_ctx *ctx, const cs_lm_frame *kf, const cs_lm_frame *neighbours, int n_neigh, const int *matches12, int pair_cap, int *pair_off, int *pair_idx1,
                             int *pair_idx2, float *x3D, uint8_t *status, int *new_pair_of_idx1, int *nnew);
/* MapPoint::ComputeDistinctiveDescriptors for n_points points: the observations of point p are desc[32 * obs_off[p]] .. desc[32 * obs_off[p + 1]), in the iteration order of
 * mObservations with bad key frames left out (:400-406).  best[p] = index within the run of the first row whose sorted distances have the smallest vDists[int(0.5 * (N - 1))],
 * -1 for an empty run (the reference returns and keeps mDescriptor). */
int cs_mappoint_distinctive_descriptors(cs_ctx *ctx, int n_points, const int *obs_off, const uint8_t *desc, int *best);
/* MapPoint::UpdateNormalAndDepth for n_points points: obs_kf[obs_off[p]] .. = index into kf_Ow[3 * n_kf] (GetCameraCenter) of every observing key frame in the order of
 * mObservations; ref_kf[p] / ref_octave[p] = mpRefKF and the octave of its key point; scale_factors[n_levels] = mvScaleFactors.  normal[3 n] = mNormalVector, min_distance /
 * max_distance = mfMinDistance / mfMaxDistance; updated[p] = 1, or 0 for an empty run, whose three outputs are left untouched.  normali / cv::norm(normali) and normal / n are
 * float(v_k * (1.0 / s)) (the stated definition of the cv::MatExpr scale).  CS_ERR_BAD_ARG: an index outside its table. */
int cs_mappoint_update_normal_and_depth(cs_ctx *ctx, int n_points, const float *world_pos, const int *obs_off, const int *obs_kf, int n_kf, const float *kf_Ow,
                                        const int *ref_kf, const int *ref_octave, const float *scale_factors, int n_levels, float *normal, float *min_distance,
                                        float *max_distance, uint8_t *updated);

/* ---- Sim3Solver (orb_object_slam/src/Sim3Solver.cc), the RANSAC of LoopClosing::ComputeSim3 (LoopClosing.cc:231-342): every hypothesis of every loop candidate in one call.
 * Problem p (one Sim3Solver) has the correspondences corr_off[p] .. corr_off[p + 1] -- X3Dc1 / X3Dc2 the floats of mvX3Dc1 / mvX3Dc2 (:92-96), max_err1 / max_err2 =
 * mvnMaxError1 / 2 (:85-86; std::vector<size_t> in this reference, so the caller passes (float)(size_t)(9.210 * sigma2)) -- K8[8 p ..] = fx fy cx cy of mK1, then of mK2, fix_scale[p] = mbFixScale, and the hypotheses hyp_off[p] .. hyp_off[p + 1]; triples[3 h ..] are
 * the three indices (into the problem's correspondences) that iteration draws at :161-175.  Per hypothesis: ComputeSim3 (:224-334) on the triple and CheckInliers (:336-360)
 * on all N correspondences -> n_inliers[h] = mnInliersi, sRt[13 h ..] = ms12i, mR12i row-major, mt12i, and the mask of mvbInliersi: hypothesis h of problem p owns the
 * W_p = (N_p + 31) / 32 words from  sum over q < p of (hyp_off[q + 1] - hyp_off[q]) * W_q  +  (h - hyp_off[p]) * W_p,  bit (i & 31) of word (i >> 5) = mvbInliersi[i], the bits
 * from N_p up 0 (cs_sim3_solver_mask_words gives the total).  cv::eigen and atan2 + cv::Rodrigues are the library's stated definitions (csrc/horn_math.h, INTEGRATION.md
 * 8b'); where the reference's values turn NaN or inf (a coincident triple, a zero imaginary part, den == 0, a point with z == 0) they do here, and nothing is an inlier of a
 * NaN test.  One launch (one wave per hypothesis) and one read-back.
 * ctx == NULL evaluates the same text (csrc/horn_math.h) on the host, one thread, with the same checks and byte-equal results: the comparison side of tests and bench, asked
 * for explicitly -- a call with a context never runs it.
 * CS_ERR_BAD_ARG (nothing written, nothing launched): NULL arrays, offsets that do not start at 0 or decrease, a triple index outside 0..N_p - 1, two equal indices in a
 * triple, a problem with hypotheses and N_p < 3.  n_problems == 0 or a problem without hypotheses: success, nothing launched for it. */
int cs_sim3_solver_hypotheses(cs_ctx *ctx, int n_problems, const int *corr_off, const float *X3Dc1, const float *X3Dc2, const float *max_err1, const float *max_err2,
                              const float *K8, const uint8_t *fix_scale, const int *hyp_off, const int *triples, int *n_inliers, float *sRt, uint32_t *inlier_mask);
long cs_sim3_solver_mask_words(int n_problems, const int *corr_off, const int *hyp_off); /* -1 for NULL or decreasing offsets */
/* Sim3Solver::SetRansacParameters :118-133 -> mRansacMaxIts, with the float epsilon and the double log / pow as written; 0 for N < min_inliers, where iterate returns at :144
 * and the value is never read.  Where ceil(log / log) does not fit an int (N in the thousands at a small min_inliers) the reference's conversion is
 * undefined -- x86 yields one iteration --; the library takes max_iterations.  Host only. */
int cs_sim3_solver_max_iterations(double probability, int min_inliers, int max_iterations, int N);
/* The loop :156-199 and the test :201 of Sim3Solver::iterate(nIterations, bNoMore, ...) over the table n_inliers[ransac_max_its] of the solver's hypotheses in drawing order
 * (N >= min_inliers: :144 is the caller's, with cs_sim3_solver_max_iterations == 0).  *mnIterations and *mnBestInliers live across calls (both start at 0);
 * *best_hypothesis is the hypothesis of mBestT12 and friends (-1 until there is one).  Returns the hypothesis whose mBestT12 iterate returns, or -1 (cv::Mat()).  Host only. */
int cs_sim3_solver_walk(const int *n_inliers, int ransac_max_its, int min_inliers, int *mnIterations, int *mnBestInliers, int *best_hypothesis, int nIterations, int *bNoMore);

/* ---- PnPsolver (orb_object_slam/src/PnPsolver.cc), the RANSAC over EPnP of Tracking::Relocalization (Tracking.cc:2876-3030): every hypothesis of every relocalisation
 * candidate, and every distinct Refine(), in one call.  Problem p (one PnPsolver) has the correspondences corr_off[p] .. corr_off[p + 1] -- P3Dw / P2D the floats of mvP3Dw /
 * mvP2D (:89-93), max_err = mvMaxError (:155) --, K4[4 p ..] = fu fv uc vc (:104-107), min_inliers[p] = mRansacMinInliers as SetRansacParameters adjusted it (:133-138),
 * best_in[p] = mnBestInliers carried into this table (0 for a solver's first table) and the hypotheses hyp_off[p] .. hyp_off[p + 1]; quads[4 h ..] are the four indices (into
 * the problem's correspondences) that iteration draws at :187-200.  Per hypothesis: compute_pose (:482-532) on the quad and CheckInliers (:305-336) on all N correspondences ->
 * n_inliers[h] = mnInliersi, Rt[12 h ..] = mRi row-major, mti, and the mask of mvbInliersi in the word layout of cs_sim3_solver_hypotheses (cs_sim3_solver_mask_words gives
 * the total).  A hypothesis is a record where n_inliers[h] >= min_inliers[p] and n_inliers[h] > every earlier count of the problem and best_in[p] (:208-211); records are found
 * on the device.  Refine() (:258-303) always runs on mvbBestInliers, the mask of the latest record, so its distinct results are one per record: refined_n[h] =
 * mnRefinedInliers, refined_Rt[12 h ..], refined_mask (same layout) = mvbRefinedInliers; refined_n[h] = -1 and zeros where h is no record.
 * status[h]: bit 0 -- qr_solve met a zero column (:916-921) in the hypothesis, bit 1 -- in its refinement; there the reference leaves X unwritten, and the library adds the
 * previous iteration's increment (zeros before the first solve).  Bit 2: h is a record.  cvSVD, cvInvert, cvSolve and cvMulTransposed are the library's stated definitions
 * (csrc/cv_svd_math.h, INTEGRATION.md 8b''); inf and NaN arise where the reference's statements make them (betas[0] == 0 -- two pairs of coincident points in a quad, for
 * one --, Zc == 0) and nothing is an inlier of an inf or NaN test; a coplanar or collinear quad and a single pair of coincident points give finite poses, because the SVD forms of
 * cvInvert and cvSolve leave out the vanishing singular values.  Three launches back to back and one read-back; the per-point arrays of a refinement live in the call's scratch, there is no cap on N_p: the scratch
 * is reserved for every hypothesis, 104 N_p bytes each (which hypotheses are records is found on the device, and the bound the counts give -- N_p - min_inliers + 1 records -- is
 * no smaller than n_hyp_p at the parameters of Relocalization), so a call needs 104 * sum over p of n_hyp_p * N_p bytes of device memory: 23 MB at 16 x 35 x 400, 156 MB at
 * 300 hypotheses on 5 000 correspondences; CS_ERR_HIP where the device cannot give them.
 * ctx == NULL evaluates the same text (csrc/epnp_math.h) on the host, one thread, with the same checks and byte-equal results: the comparison side of tests and bench, asked
 * for explicitly -- a call with a context never runs it.
 * CS_ERR_BAD_ARG (nothing written, nothing launched): NULL arrays, offsets that do not start at 0 or decrease, a quad index outside 0..N_p - 1 or repeated within its quad, a
 * problem with hypotheses and N_p < 4 or min_inliers[p] < 4 (:136-137 make it at least minSet).  n_problems == 0 or a problem without hypotheses: success. */
int cs_pnp_solver_evaluate(cs_ctx *ctx, int n_problems, const int *corr_off, const float *P3Dw, const float *P2D, const float *max_err, const float *K4, const int *min_inliers,
                           const int *best_in, const int *hyp_off, const int *quads, int *n_inliers, double *Rt, uint32_t *status, uint32_t *inlier_mask, int *refined_n,
                           double *refined_Rt, uint32_t *refined_mask);
/* PnPsolver::SetRansacParameters :120-151 for N correspondences -> the adjusted mRansacMinInliers, mRansacMaxIts and mRansacEpsilon, with the float epsilon and the double
 * log / pow as written (pow(epsilon, 3), :149).  Where ceil(log / log) does not fit an int the library takes maxIterations, as cs_sim3_solver_max_iterations does.  Host only. */
int cs_pnp_solver_ransac_parameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, int N, int *mRansacMinInliers, int *mRansacMaxIts,
                                    float *mRansacEpsilon);
/* The loop :181-237 and the tail :239-255 of PnPsolver::iterate(nIterations, bNoMore, ...) over the tables n_inliers[n_hyp], refined_n[n_hyp] of the solver's hypotheses in
 * drawing order (N >= min_inliers: :172 is the caller's).  *mnIterations, *mnBestInliers (both start at 0) and *best_hypothesis (the hypothesis of mBestTcw and
 * mvbBestInliers, -1 until there is one) live across calls.  Returns the hypothesis whose pose iterate returns -- *refined = 1: mRefinedTcw of its refinement (:234),
 * *refined = 0: its own mBestTcw at exhaustion (:251) --, -1 for cv::Mat(), or -2 where the loop would read hypothesis n_hyp: it stops before consuming it, and the caller
 * resumes with a longer table and nIterations less the hypotheses this call consumed.  Note :181: a call made at mnIterations >= mRansacMaxIts still runs nIterations
 * hypotheses, and bNoMore is set only at :239-241.  Host only. */
int cs_pnp_solver_walk(const int *n_inliers, const int *refined_n, int n_hyp, int ransac_max_its, int min_inliers, int *mnIterations, int *mnBestInliers, int *best_hypothesis,
                       int nIterations, int *bNoMore, int *refined);

/* ---- Initializer (orb_object_slam/src/Initializer.cc), the two-view initialisation of Tracking::MonocularInitialization (Tracking.cc:948-983): FindHomography (:131-179),
 * FindFundamental (:181-229), the choice of :113-126 and the CheckRT passes of ReconstructF (:474-501) / ReconstructH (:579-724) for every frame pair of a batch in one call.
 * Problem p (one Initialize call) has the key points key1_off[p] .. key1_off[p + 1] of the reference frame (keys1: x y of mvKeys1, all of them: Normalize :754-800 runs over
 * every key point) and key2_off[p] .. of the current frame (mvKeys2), the correspondences corr_off[p] .. corr_off[p + 1] -- matches12[2 i ..] = mvMatches12[i].first, .second,
 * indices into the problem's key points (:55-64) --, K9[9 p ..] = mK row-major, sigma[p] = mSigma, and the hypotheses hyp_off[p] .. hyp_off[p + 1]; sets[8 h ..] are the eight
 * indices (into the problem's correspondences) of mvSets[it] (:83-98).  H = hyp_off[n_problems], NC = corr_off[n_problems], W_p = (N_p + 31) / 32.
 * Per hypothesis and model (0 = homography, 1 = fundamental; model m of hypothesis h is entry m * H + h): score = currentScore, matrix[9 ..] = H21i / F21i row-major, and the
 * mask of vbCurrentInliers in the word layout of cs_sim3_solver_hypotheses, the masks of model 1 following all of model 0 (cs_sim3_solver_mask_words gives the words of one
 * model).
 * Per problem: best[2 p + m] = the hypothesis (counted from hyp_off[p]) that :172 / :222 keep -- the first strict maximum of the scores above 0 --, -1 without one;
 * S[2 p + m] = SH, SF; RH[p] (:113); model[p] = 0 where RH > 0.40 (:117), else 1, or -1 ("no model") where the chosen model has no hypothesis with a score above 0: there RH is
 * a NaN and the reference goes on with an empty matrix, which OpenCV refuses.  n_inliers[p] = N of :477-480 / :582-585, the set bits of the chosen mask.  cand_Rt[12 (8 p + c) ..]
 * = R row-major, t of candidate c, n_cand[p] of them: the four of :498-501 in that order, or vR[i], vt[i] of :626-693, or none where ReconstructH returns at :604; zeros behind
 * them.  Per candidate, CheckRT (:802-911): nGood[8 p + c], cos_parallax[8 p + c] = vCosParallax[min(50, nGood - 1)] after the sort (0 where nGood == 0; the acos of :905 is
 * the walk's), good_mask = vbGood per correspondence -- candidate c of problem p owns the W_p words from  8 * sum over q < p of W_q  +  c * W_p  -- and points[3 (8 corr_off[p] +
 * c N_p + i) ..] = vP3D of correspondence i, zeros where :893 is not reached.  The reference indexes vbGood and vP3D by mvMatches12[i].first; the mirrors scatter.
 * cv::SVDecomp on CV_32F, Mat::inv, cv::determinant and the order of std::sort are the library's stated definitions (csrc/initializer_math.h, INTEGRATION.md 8b'''); inf and
 * NaN arise where the reference's statements make them, and nothing is an inlier of a NaN test that the reference writes with >.  Four launches back to back and one read-back.
 * ctx == NULL evaluates the same text on the host, one thread, with the same checks and byte-equal results: the comparison side of tests and bench, asked for explicitly -- a
 * call with a context never runs it.
 * CS_ERR_BAD_ARG (nothing written, nothing launched): NULL arrays, offsets that do not start at 0 or decrease, a match outside the key points of its frame, a set index outside
 * 0..N_p - 1 or repeated within its set, a problem with hypotheses and N_p < 8.  Which arrays may be NULL: with n_problems > 0 every per-problem and per-candidate output
 * (model .. cos_parallax, good_mask, points) is required, hypotheses or not -- they are written for a problem without hypotheses too --; score, matrix, inlier_mask and sets only
 * where the call has hypotheses; keys, matches12 only where there are key points, matches.  n_problems == 0: success whatever the arrays.  A problem without hypotheses: no model. */
int cs_initializer_evaluate(cs_ctx *ctx, int n_problems, const int *key1_off, const float *keys1, const int *key2_off, const float *keys2, const int *corr_off,
                            const int *matches12, const float *K9, const float *sigma, const int *hyp_off, const int *sets, float *score, float *matrix, uint32_t *inlier_mask,
                            int *model, int *best, float *S, float *RH, int *n_inliers, int *n_cand, float *cand_Rt, int *nGood, float *cos_parallax, uint32_t *good_mask,
                            float *points);
/* The decisions of ReconstructF :503-576 (model 1, n_cand 4) and ReconstructH :695-736 (model 0, n_cand 8; n_cand 0 is the return of :604) over the candidates' nGood[n_cand]
 * and cos_parallax[n_cand] of cs_initializer_evaluate and N = n_inliers: nsimilar and nMinGood, or best / second best, with the reference's strict comparisons and the first
 * among equals; parallax = acos(cos) * 180 / CV_PI as :905 writes it (acosf, a float product, a double quotient).  Initialize passes minParallax = 1.0, minTriangulated = 50
 * (:116-125).  Returns the candidate whose R21, t21, vP3D and vbTriangulated Initialize hands back, or -1 (false; also for model -1); *parallax (optional) = the parallax the
 * rule compared.  CS_ERR_BAD_ARG for a NULL table.  Host only. */
int cs_initializer_walk(int model, int n_cand, const int *nGood, const float *cos_parallax, int N, float minParallax, int minTriangulated, float *parallax);

#ifdef __cplusplus
}
#endif
#endif
