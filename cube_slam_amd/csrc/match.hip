// match.hip -- ORB_SLAM2::ORBmatcher Hamming searches on MI355X (gfx950).
//
// Replaces ORBmatcher::SearchByProjection (all four overloads), SearchForInitialization, SearchByBoW (both overloads), SearchForTriangulation, the search of both Fuse overloads,
// SearchBySim3 and DescriptorDistance (reference orb_object_slam/src/ORBmatcher.cc:50-142, :171-310, :309-427, :429-542, :544-677, :679-850, :934-981, :1010-1139, :1141-1371,
// :1373-1522, :1727-1858, :1905-1921) and the Frame grid
// (src/Frame.cc:303-318, :404-459, :525-535, :546-609).
//
//   match_grid           counting sort of the keypoints into the 64x48 grid, per-cell lists in keypoint order; one workgroup per frame (one frame or a window's frames)
//   match_undistort      Frame::UndistortKeyPoints: cv::undistortPoints with P = K, a thread per key point
//   match_project        per last-frame map point: Rcw*x+tcw (cv::gemm: double accumulate, one rounding), pinhole projection,
//                        window radius th*scale[octave]; one pose or one pose per pair of a window
//   match_project_map<M> per map point of a Sim3 / relocalisation search (:309-427, :1010-1139, :1141-1371, :1727-1858), of Tracking::SearchLocalPoints (Frame::isInFrustum,
//                        Frame.cc:346-402) or of Fuse(pKF, vpMapPoints, th) (:871-920) the whole preamble: transform, depth, image, distance and
//                        viewing-angle tests, MapPoint::PredictScale (glibc's logf restated), radius -- the query and its level window, written where match_candidates reads them
//   match_candidates     MC_G lanes per query: lane = grid cell of the window (ix outer, iy inner = the reference's candidate
//                        order), level + |dx|<r,|dy|<r filters, ordered compaction by a prefix sum, 256-bit Hamming
//                        distance as 4 x popcount(u64).  It counts, takes a slice of the candidate arena, fills it with (idx, dist).
//   match_resolve<V>     the greedy claim / best-second / ratio / rotation-histogram logic of the reference, which is sequential over the queries (a candidate
//                        claimed by an earlier query is skipped by later ones): one wave per search, 64 queries at a time, over the candidate lists
//   match_fuse_best      Fuse: per map point the best key point after the chi-square tests
//   match_map_best       Fuse(Scw) / SearchBySim3: per map point the first minimum of its candidate list; match_sim3_agree: SearchBySim3's agreement pass
//   match_triangulation  SearchForTriangulation: one wave per key point of KF1 over the KF2 features of its vocabulary node
//   match_orient_cut     the rotation cut of a search whose matches are independent of each other
//   match_bow_dists      SearchByBoW: the distances of a feature to its node's features, as candidate lists for match_resolve
//   match_knn2           all-pairs best / second best, train descriptors staged through LDS
#include "common.h"
#include "cv_math.h"
#include "frame_math.h"
#include "glibc_logf.h"
#include "stereo_search_math.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

namespace {
constexpr int GRID_ROWS = 48, GRID_COLS = 64, NCELL = GRID_ROWS * GRID_COLS; // Frame.h:32-33
constexpr int TH_HIGH = 100, TH_LOW = 50, HISTO_LENGTH = 30;                // ORBmatcher.cc:42-44

struct FrameP { int N; float minX, maxX, minY, maxY, wInv, hInv; };
// What a window search reads of a key point of the searched frame, laid out in CELL order (the entries of a cell -- and of the cells of a grid column -- lie one behind the
// other): a window's walk streams 16-byte records instead of chasing cell list -> index -> 28-byte key point record
struct CellRec { float x, y; int id, octave; };

// AssignFeaturesToGrid (Frame.cc:303-318), one workgroup per frame.  kfirst == NULL: one frame, key points 0 .. F.N.  Otherwise workgroup p takes key points
// kfirst[p] .. kfirst[p + 1] of `keys`; its cell lists (relative to the frame) lie at p x (NCELL + 1) / kfirst[p] of the outputs.
__global__ void __launch_bounds__(1024) match_grid(FrameP F, const cs_keypoint *keys_all, const int *kfirst, int *cell_start_all /*P x (NCELL+1)*/, int *cell_items_all, int *kp_cell_all, CellRec *cell_recs_all) {
    __shared__ int cnt[NCELL];
    __shared__ int s_part[1024];
    const int tid = threadIdx.x, p = blockIdx.x, kb = kfirst ? kfirst[p] : 0, N = kfirst ? kfirst[p + 1] - kb : F.N;
    const cs_keypoint *keys = keys_all + kb;
    int *cell_start = cell_start_all + (size_t)p * (NCELL + 1), *cell_items = cell_items_all + kb, *kp_cell = kp_cell_all + kb;
    CellRec *cell_recs = cell_recs_all + kb;
    for (int c = tid; c < NCELL; c += 1024) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += 1024) { // PosInGrid, Frame.cc:525-535
        int px = (int)roundf((keys[i].x - F.minX) * F.wInv), py = (int)roundf((keys[i].y - F.minY) * F.hInv);
        int c = (px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS) ? -1 : px * GRID_ROWS + py;
        kp_cell[i] = c;
        if (c >= 0) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    // exclusive scan over the cells: 3 cells per thread
    int c0 = cnt[tid * 3], c1 = cnt[tid * 3 + 1], c2 = cnt[tid * 3 + 2];
    s_part[tid] = c0 + c1 + c2;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        int v = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int base = s_part[tid] - (c0 + c1 + c2);
    cell_start[tid * 3] = base; cell_start[tid * 3 + 1] = base + c0; cell_start[tid * 3 + 2] = base + c0 + c1;
    if (tid == 1023) cell_start[NCELL] = s_part[1023];
    __syncthreads();
    cnt[tid * 3] = base; cnt[tid * 3 + 1] = base + c0; cnt[tid * 3 + 2] = base + c0 + c1; // running fill positions
    __syncthreads();
    for (int i = tid; i < N; i += 1024) { int c = kp_cell[i]; if (c >= 0) cell_items[atomicAdd(&cnt[c], 1)] = i; }
    __syncthreads();
    // mGrid[x][y] holds the indices in push_back order = ascending keypoint index: sort each (tiny) cell list
    for (int c = tid; c < NCELL; c += 1024) {
        int b = cell_start[c], e = cnt[c];
        for (int i = b + 1; i < e; i++) {
            int v = cell_items[i], j = i - 1;
            while (j >= b && cell_items[j] > v) { cell_items[j + 1] = cell_items[j]; j--; }
            cell_items[j + 1] = v;
        }
    }
    __syncthreads();
    for (int i = tid; i < cell_start[NCELL]; i += 1024) { const int id = cell_items[i]; const cs_keypoint k = keys[id]; cell_recs[i] = CellRec{k.x, k.y, id, k.octave}; }
}

// UndP, undistort_point, make_undp: frame_math.h
__global__ void match_undistort(int n, const cs_keypoint *in, UndP U, cs_keypoint *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cs_keypoint k = in[i];
    float x, y;
    undistort_point(U, k.x, k.y, x, y);
    k.x = x; k.y = y;
    out[i] = k;
}

// A window query.  `pair`: which train frame of a window it searches (0 for the one-frame calls).
struct QueryS { float x, y, r; int minLevel, maxLevel, valid, pair; };

// The queries of a SearchByProjection (ORBmatcher.cc:1397-1430).  Query i belongs to pair p with qfirst[p] <= i < qfirst[p + 1] and is projected with the pose
// T_all + 12 * p; qfirst == NULL: one pair, no bisection.  Its level is octave[i] or, with octave == NULL, the key point record's okeys[i].octave (:1424); a level outside the
// scale table raises *err and leaves the query invalid.
// STEREO (bMono == false, :1393-1394, :1433-1438, :1461): the level window follows the pair's direction (S.dir[pair], or S.dir0 with S.dir == NULL) and the query's predicted
// right coordinate ur = u - bf * invzc goes to S.ur[i], a separate array: QueryS keeps its layout.  The false instantiation is the monocular kernel, statement by statement.
struct StereoQ { const int *dir; int dir0; float bf; float *ur; };
template <bool STEREO> __global__ void __launch_bounds__(256) match_project(int nq, int n_pairs, const int *qfirst, const float *world_pos, const uint8_t *valid, const int *octave, const cs_keypoint *okeys,
                                                    const float *T_all, float fx, float fy, float cx, float cy, const float *scale_factors, int n_levels, float th, FrameP F, QueryS *q, int *err, StereoQ S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    int lo = 0, hi = qfirst ? n_pairs : 1; // qfirst[lo] <= i < qfirst[hi]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (qfirst[mid] <= i) lo = mid; else hi = mid; }
    const float *T = T_all + 12 * lo;
    QueryS Q{0, 0, 0, 0, 0, 0, lo};
    float ur = 0.0f;
    if (valid[i]) {
        const int o = octave ? octave[i] : okeys[i].octave;
        if (o < 0 || o >= n_levels) { *err = 1; q[i] = Q; if (STEREO) S.ur[i] = ur; return; }
        float x3Dc[3];
        for (int r = 0; r < 3; r++) {
            double sacc = 0;
            for (int k = 0; k < 3; k++) sacc += (double)T[r * 4 + k] * (double)world_pos[(size_t)i * 3 + k];
            x3Dc[r] = (float)(sacc * 1.0 + (double)T[r * 4 + 3] * 1.0);
        }
        const float xc = x3Dc[0], yc = x3Dc[1];
        const float invzc = (float)(1.0 / x3Dc[2]);
        if (!(invzc < 0)) {
            float u = fx * xc * invzc + cx;
            float v = fy * yc * invzc + cy;
            if (!(u < F.minX || u > F.maxX) && !(v < F.minY || v > F.maxY)) { Q.x = u; Q.y = v; Q.r = th * scale_factors[o]; Q.minLevel = o - 1; Q.maxLevel = o + 1; Q.valid = 1;
                if (STEREO) { stereo_search_levels(S.dir ? S.dir[lo] : S.dir0, o, Q.minLevel, Q.maxLevel); ur = u - S.bf * invzc; }
            }
        }
    }
    q[i] = Q;
    if (STEREO) S.ur[i] = ur;
}

// The preamble of the searches that project map points through a Sim3 or a relocalisation pose, with the reference's float arithmetic statement by statement (a cv::Mat
// product is one gemm per row: double accumulation over k ascending, one rounding; cv::norm and Mat::dot accumulate in double; 1 / z and 1.0 / z are a double division
// rounded to float; everything else is float in the reference's association -- the library is built with -ffp-contract=off):
//   PM_SIM3   SearchByProjection(pKF, Scw, ...) :346-382 and Fuse(pKF, Scw, ...) :1048-1085   p3Dc = Rcw p + tcw, z < 0, KeyFrame::IsInImage, dist = |p - Ow|, viewing angle
//   PM_PAIR   SearchBySim3 :1198-1228 / :1281-1311   p1 = R1w p + t1w, p2 = sR21 p1 + t21 (two gemms, two roundings), z < 0, IsInImage, dist = |p2|
//   PM_RELOC  SearchByProjection(CurrentFrame, pKF, sAlreadyFound, ...) :1755-1785   x3Dc = Rcw p + tcw, NO depth test, the Frame's bounds (both ends inclusive),
//             u = fx * xc * invzc + cx (the other modes: fx * (X * invz) + cx), dist = |p - Ow|, window levels [L - 1, L + 1] (the other modes: [L - 1, L])
// then MapPoint::PredictScale (MapPoint.cc:524-533) L = ceil(logf(mfMaxDistance / dist) / logScaleFactor) with glibc's logf, r = th * mvScaleFactors[L].
// This fork's PredictScale does not clamp and 0.8 min <= dist <= 1.2 max allows L = -1, n_levels, n_levels + 1, where the reference reads past mvScaleFactors: such a point
// (and one whose ratio is not a positive normal float) is an invalid query and is counted in *n_outside; the call goes on.
//   PM_FUSE     Fuse(pKF, vpMapPoints, th) :871-920   PM_SIM3's statements and ur = u - bf * invz (:900); the window has no level limits (:922), match_fuse_best applies them
//   PM_FRUSTUM  Frame::isInFrustum (Frame.cc:346-402) + the radius of SearchByProjection(F, vpMapPoints, th) (:54, :72-78)   Pc = Rcw p + tcw, PcZ < 0, invz = 1.0f / PcZ,
//             u = fx * PcX * invz + cx (PM_RELOC's association), the Frame's bounds (both ends inclusive), dist = |p - Ow|, viewCos = PO.dot(Pn) / dist (a double division
//             rounded to float) tested as viewCos < viewingCosLimit, uR = u - bf * invz; r = RadiusByViewingCos (viewCos > 0.998 compared in DOUBLE: float(0.998) > 0.998),
//             times th only when th != 1.0, times mvScaleFactors[L]; levels [L - 1, L].  PcZ == 0 passes the reference's depth test; where it leaves u or v not finite (0 * inf:
//             every comparison of the bounds test is false and the reference goes on to undefined float -> int casts) the point is rejected here.
// The last two modes also leave what the reference keeps per map point in O: valid / in view, (u, v, ur), the viewing cosine (PM_FRUSTUM) -- zeros for a rejected point -- and
// add the number of valid points to n_outside[1].
enum { PM_SIM3 = 0, PM_PAIR = 1, PM_RELOC = 2, PM_FUSE = 3, PM_FRUSTUM = 4 };
struct MapP { float R[9], t[3], Ow[3], R2[9], t2[3]; float fx, fy, cx, cy, log_sf, th; int n_levels; float bf, view_cos_limit; };
struct MapOut { uint8_t *valid; float *proj, *aux; }; // PM_FRUSTUM: proj = (u, v, uR) per point, aux = the viewing cosine; PM_FUSE: proj = (u, v), aux = ur, as match_fuse_best reads them
// gemm3 / norm3: cv_math.h
template <int MODE> __global__ void __launch_bounds__(256) match_project_map(int n, const float *world_pos, const float *normal, const float *min_distance, const float *max_distance, const uint8_t *skip,
                                                                             MapP P, const float *scale_factors, FrameP F, QueryS *q, int *level, int *n_outside, MapOut O) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    QueryS Q{0, 0, 0, 0, 0, 0, 0};
    int L = -1;
    float o_u = 0.0f, o_v = 0.0f, o_ur = 0.0f, o_cos = 0.0f;
    do {
        if (skip[i]) break;
        const float p[3] = {world_pos[(size_t)i * 3], world_pos[(size_t)i * 3 + 1], world_pos[(size_t)i * 3 + 2]};
        float pc[3];
        gemm3(P.R, p, P.t, pc);
        if (MODE == PM_PAIR) { float p2[3]; gemm3(P.R2, pc, P.t2, p2); pc[0] = p2[0]; pc[1] = p2[1]; pc[2] = p2[2]; }
        float u, v, invz = 0.0f;
        if (MODE == PM_RELOC || MODE == PM_FRUSTUM) {
            if (MODE == PM_FRUSTUM && pc[2] < 0.0f) break; // Frame.cc:360
            const float xc = pc[0], yc = pc[1];
            const float invzc = (float)(1.0 / (double)pc[2]); // (1.0f / PcZ of Frame.cc:364 is the same float: a quotient of two floats rounds once either way)
            u = P.fx * xc * invzc + P.cx;
            v = P.fy * yc * invzc + P.cy;
            if (MODE == PM_FRUSTUM && !(isfinite(u) && isfinite(v))) break;
            if (u < F.minX || u > F.maxX) break;
            if (v < F.minY || v > F.maxY) break;
            invz = invzc;
        } else {
            if (pc[2] < 0.0f) break;
            invz = (float)(1.0 / (double)pc[2]);
            const float x = pc[0] * invz, y = pc[1] * invz;
            u = P.fx * x + P.cx;
            v = P.fy * y + P.cy;
            if (!(u >= F.minX && u < F.maxX && v >= F.minY && v < F.maxY)) break; // KeyFrame::IsInImage (KeyFrame.cc:670-673)
        }
        const float maxDistance = 1.2f * max_distance[i], minDistance = 0.8f * min_distance[i]; // MapPoint::GetMax / GetMinDistanceInvariance (MapPoint.cc:512-522)
        float PO[3] = {pc[0], pc[1], pc[2]}; // SearchBySim3 measures the camera-frame vector (:1218, :1301), the others p - Ow
        if (MODE != PM_PAIR) for (int k = 0; k < 3; k++) PO[k] = p[k] - P.Ow[k];
        const float dist = norm3(PO);
        if (dist < minDistance || dist > maxDistance) break;
        float viewCos = 0.0f;
        if (MODE == PM_SIM3 || MODE == PM_FUSE || MODE == PM_FRUSTUM) { // viewing angle below 60 degrees (:374-377, :914, :1076-1079)
            double dot = 0;
            for (int k = 0; k < 3; k++) dot += (double)PO[k] * (double)normal[(size_t)i * 3 + k];
            if (MODE == PM_FRUSTUM) { // Frame.cc:385-388
                viewCos = (float)(dot / (double)dist);
                if (viewCos < P.view_cos_limit) break;
            } else if (dot < 0.5 * (double)dist) break;
        }
        const float ratio = max_distance[i] / dist;
        float lf = -1.0f;
        if (glibc_logf::in_domain(ratio)) lf = ceilf(glibc_logf::logf_(ratio) / P.log_sf);
        if (!(lf >= 0.0f && lf < (float)P.n_levels)) { atomicAdd(n_outside, 1); break; }
        L = (int)lf;
        float r = P.th;
        if (MODE == PM_FRUSTUM) { // RadiusByViewingCos (:144-150) and bFactor (:54, :74-75)
            r = (double)viewCos > 0.998 ? 2.5f : 4.0f;
            if (P.th != 1.0f) r *= P.th;
        }
        Q.x = u; Q.y = v; Q.r = r * scale_factors[L]; Q.valid = 1;
        if (MODE == PM_FUSE) { Q.minLevel = -1; Q.maxLevel = -1; }
        else { Q.minLevel = L - 1; Q.maxLevel = MODE == PM_RELOC ? L + 1 : L; }
        o_u = u; o_v = v; o_ur = u - P.bf * invz; o_cos = viewCos;
    } while (0);
    q[i] = Q; level[i] = L;
    if (MODE == PM_FUSE || MODE == PM_FRUSTUM) {
        O.valid[i] = (uint8_t)Q.valid;
        if (MODE == PM_FRUSTUM) { O.proj[(size_t)i * 3] = o_u; O.proj[(size_t)i * 3 + 1] = o_v; O.proj[(size_t)i * 3 + 2] = o_ur; O.aux[i] = o_cos; }
        else { O.proj[(size_t)i * 2] = o_u; O.proj[(size_t)i * 2 + 1] = o_v; O.aux[i] = o_ur; }
        const unsigned long long in = __ballot(Q.valid);
        if (in && lane_id() == __ffsll((long long)__ballot(1)) - 1) atomicAdd(n_outside + 1, __popcll(in)); // one update per wave, by its first live lane
    }
}

// GetFeaturesInArea (Frame.cc:404-459) for every query + the candidates' distances, in ONE pass: a wave walks its query's window twice -- it counts, takes a slice of the
// candidate arena from a global cursor, and fills the slice in the reference's candidate order (ix outer, iy inner, cell lists ascending).  Which slice a query gets depends
// on the atomics' order and on nothing else: cstart / ccount address it, and nothing reads the arena in another way.  A slice that would end past `cap` is not written and
// its count reads 0; the cursor still advances, so the host sees what the arena should have held and calls again.  The train frame of query q is key points
// kfirst[q.pair] .. of `keys` / `desc`, its cell lists at q.pair x (NCELL + 1) / kfirst[q.pair].  A candidate is (index | level << 24, distance).
// MC_G lanes per query, MC_Q queries per 256-thread workgroup, ONE cursor update per workgroup.  A window at th 15 covers 8 - 80 cells: with a whole wave per query most lanes had
// no cell, and the kernel is bound by the number of waves that wait out its seven dependent round trips (query -> frame -> cell bounds -> records, the cursor, records ->
// descriptors), not by bytes: 3.1 ms per window of 10^6 queries with 64 lanes per query whether the walk read 28-byte key point records through an index (654 MB) or
// cell-ordered 16-byte records (521 MB).  (Sixteen-wave workgroups were measured too: the same alone, 13 ms beside the region walks -- they wait for a CU with four free
// slots per SIMD.)
// STEREO: the mvuRight test of :1459-1465 / :104-109 is part of `passes`, ahead of the Hamming distance: a train key point with S.u_right[kb + id] > 0 whose distance to
// the query's predicted right coordinate S.ur_q[qi * S.ur_stride] exceeds the window radius is no candidate.  Both walks evaluate the same predicate, so the lists are the
// reference's lists after its test, in its order, and match_resolve runs on them as it is.  The false instantiation is the monocular kernel.
constexpr int MC_G = 16, MC_Q = 256 / MC_G;
struct StereoC { const float *u_right, *ur_q; int ur_stride; };
template <bool STEREO> __global__ void __launch_bounds__(256) match_candidates(FrameP F, const unsigned long long *desc, const int *kfirst, const int *cell_start_all, const CellRec *cell_recs_all, int nq,
                                                        const QueryS *q, const unsigned long long *qdesc, unsigned long long *cursor, long cap, long *cstart, int *ccount, int2 *cands, StereoC S) {
    __shared__ int s_tot[MC_Q];
    __shared__ unsigned long long s_base;
    const int grp = threadIdx.x / MC_G, qi = blockIdx.x * MC_Q + grp, lane = threadIdx.x % MC_G;
    QueryS Q{0, 0, 0, 0, 0, 0, 0};
    if (qi < nq) Q = q[qi];
    int total = 0;
    long base = 0;
    // (the window and the walk are the same for the counting and the filling half; the workgroup's groups meet in between to share one cursor update)
    const int kb = (Q.valid && kfirst) ? kfirst[Q.pair] : 0;
    const unsigned long long *td = desc + (size_t)kb * 4;
    const int *cell_start = cell_start_all + (size_t)Q.pair * (NCELL + 1); const CellRec *recs = cell_recs_all + kb;
    const float x = Q.x, y = Q.y, r = Q.r;
    const int nMinCellX = max(0, (int)floorf((x - F.minX - r) * F.wInv));
    const int nMaxCellX = min(GRID_COLS - 1, (int)ceilf((x - F.minX + r) * F.wInv));
    const int nMinCellY = max(0, (int)floorf((y - F.minY - r) * F.hInv));
    const int nMaxCellY = min(GRID_ROWS - 1, (int)ceilf((y - F.minY + r) * F.hInv));
    const bool window = Q.valid && !(nMinCellX >= GRID_COLS || nMaxCellX < 0 || nMinCellY >= GRID_ROWS || nMaxCellY < 0);
    const bool bCheckLevels = (Q.minLevel > 0) || (Q.maxLevel >= 0);
    const int ny = nMaxCellY - nMinCellY + 1, ncell = window ? (nMaxCellX - nMinCellX + 1) * ny : 0;
    unsigned long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    if (window && qdesc) { d0 = qdesc[(size_t)qi * 4]; d1 = qdesc[(size_t)qi * 4 + 1]; d2 = qdesc[(size_t)qi * 4 + 2]; d3 = qdesc[(size_t)qi * 4 + 3]; }
    float ur_q = 0.0f;
    const float *tur = nullptr;
    if (STEREO) { if (window) ur_q = S.ur_q[(size_t)qi * S.ur_stride]; tur = S.u_right + kb; }
    auto passes = [&](const CellRec &kp) {
        bool ok = true;
        if (bCheckLevels) { if (kp.octave < Q.minLevel) ok = false; if (Q.maxLevel >= 0 && kp.octave > Q.maxLevel) ok = false; }
        const float distx = kp.x - x, disty = kp.y - y;
        ok = ok && fabsf(distx) < r && fabsf(disty) < r;
        if (STEREO) { if (ok && stereo_search_drops(ur_q, tur[kp.id], r)) ok = false; } // (read only for a key point inside the window)
        return ok;
    };
    // (the groups of a wave walk in lockstep: the trip count is the longest window of the four; a group past its window does nothing)
    int ncell_w = ncell;
    for (int off = MC_G; off < 64; off <<= 1) ncell_w = max(ncell_w, __shfl_xor(ncell_w, off));
    auto walk = [&](bool fill) {
        int tot = 0;
        for (int k0 = 0; k0 < ncell_w; k0 += MC_G) {
            const int k = k0 + lane;
            int b = 0, e = 0;
            if (k < ncell) { int c = (nMinCellX + k / ny) * GRID_ROWS + nMinCellY + k % ny; b = cell_start[c]; e = cell_start[c + 1]; }
            int mine = 0;
            for (int p = b; p < e; p++) mine += passes(recs[p]);
            const int inc = wave_incl_scan<MC_G>(mine, lane);
            if (fill && mine) {
                long o = base + tot + inc - mine;
                for (int p = b; p < e; p++) {
                    const CellRec kp = recs[p];
                    if (passes(kp)) { cands[o] = make_int2(kp.id | ((kp.octave & 0xff) << 24), qdesc ? hamming256(td + (size_t)kp.id * 4, d0, d1, d2, d3) : 0); o++; }
                }
            }
            tot += __shfl(inc, MC_G - 1, MC_G);
        }
        return tot;
    };
    total = walk(false);
    if (lane == 0) s_tot[grp] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int k = 0; k < MC_Q; k++) sum += s_tot[k];
        s_base = sum ? atomicAdd(cursor, (unsigned long long)sum) : 0ull;
    }
    __syncthreads();
    base = (long)s_base;
    for (int k = 0; k < grp; k++) base += s_tot[k];
    const bool fits = base + total <= cap;
    if (!fits) total = 0;
    if (total) walk(true); // (the shuffles of a walk stay inside a group of MC_G lanes: a group without candidates may sit this one out)
    if (lane == 0 && qi < nq) { cstart[qi] = base; ccount[qi] = total; }
}

// ---- the order-dependent half of the searches: claims, best / second, ratio tests, rotation histogram (match_resolve) ---------------------------------------------------
// The reference walks the queries in order and lets query i see what queries < i did to the train key points: a key point claimed by a map point with observations is
// skipped (SearchByProjection, both overloads: ORBmatcher.cc:50-142, :1397-1494), a key point matched at a smaller or equal distance is skipped and a better match
// DISPLACES the earlier one (SearchForInitialization, :451-504), a key point matched once is never matched again (SearchByBoW, :171-310, :544-677).  One workgroup of one
// wave per search ("problem": one frame pair); the train-side state lives in LDS.  64 queries are resolved at a time, a lane each:
//   every lane picks its query's winner against the state BEFORE the batch plus the claims of the LOWER lanes of the batch (mask[idx]: which lanes claim key point idx;
//   the highest lane below mine is the one whose claim I would have seen last), publishes its claim, and the batch repeats until no lane changed its claim.  Lane 0 is
//   final after the first round, lane k after round k + 1 at the latest, and a round without change is the sequential result: a claim vector in which every lane's claim
//   is its choice given the lower lanes' claims is unique (induction over the lanes).  Typical batches settle in two or three rounds (5.6 candidates per query, 64 of
//   ~2 000 train key points touched).
// Then the batch commits (the highest claiming lane of a key point owns it), records (claim, rotation bin) per query, and the next batch starts.  After the last batch:
// the three-maxima cut over the histogram (:1860-1901) and the write-back.  Everything a query needs of a candidate (index, level, distance) is in the candidate list.
// RV_CLAIM: the loops of SearchByProjection(pKF, Scw, ...) (:392-423) and of the relocalisation search (:1792-1831) -- a key point that holds a map point, from before the call
// (tblocked, which also carries !KeysStatic) or claimed by an earlier query, is skipped (RV_BOW's rule); first strict minimum; accepted at best <= accept_dist; no ratio test.
enum { RV_PROJ = 0, RV_LOCAL = 1, RV_INIT = 2, RV_BOW = 3, RV_BOWKF = 4, RV_CLAIM = 5 };
struct ResolveP {
    const long *cstart; const int *ccount; const int2 *cands; // per query
    const int *qlist;        // the visiting order (query index per step) or NULL: step = query index
    const int *pfirst;       // problem p visits steps pfirst[p] .. pfirst[p + 1]; NULL: one problem, steps 0 .. n_steps
    const int *kfirst;       // problem p's train key points: kfirst[p] .. kfirst[p + 1] of tkeys / tblocked; NULL: 0 .. n_train
    int n_steps, n_train;
    const cs_keypoint *tkeys; // train key points (angle)
    const cs_keypoint *qkeys; const float *qangle; // the queries' angles: key point records or a plain array
    const uint8_t *blocks;    // per query: its map point has observations (RV_PROJ, RV_LOCAL)
    const uint8_t *tblocked;  // per train key point: never a candidate (nullable)
    float nnratio; int check_orientation;
    int *train_match;        // RV_PROJ, RV_LOCAL, RV_BOW: per train key point, at (kfirst[p] - kfirst[0]) + idx: the matched query (index within the problem) or -1
    int *q_match;            // RV_INIT, RV_BOWKF: per query, the matched train key point or -1
    int *q_rec;              // scratch, per query
    int *nmatches;           // per problem
    int accept_dist;         // RV_CLAIM: TH_LOW (:419) or the caller's ORBdist (:1815)
};
constexpr int RS_NC = 8; // candidates of a query kept in registers over the rounds of its batch (the rest is re-read)

__host__ __device__ inline void three_maxima(const int *sizes, int L, int &ind1, int &ind2, int &ind3) { // ORBmatcher.cc:1860-1901
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = sizes[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) ind3 = -1;
}
__host__ __device__ inline int rot_bin(float a1, float a2) { // :1483-1491
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = a1 - a2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

template <int V> __global__ void __launch_bounds__(64) match_resolve(ResolveP P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_mem[];
    __shared__ int s_cd[64], s_hist[32], s_ind[3];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int s0 = P.pfirst ? P.pfirst[p] : 0, s1 = P.pfirst ? P.pfirst[p + 1] : P.n_steps;
    const int kb = P.kfirst ? P.kfirst[p] : 0, N2 = P.kfirst ? P.kfirst[p + 1] - kb : P.n_train, out0 = P.kfirst ? kb - P.kfirst[0] : 0;
    const int qsub = P.qlist ? 0 : s0;
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(rs_mem); // lanes of the current batch that claim the key point
    int *owner = reinterpret_cast<int *>(mask + N2); // RV_PROJ / RV_LOCAL: -1 free, -2 never, else query << 1 | its map point has observations; others: -1 free, -2 never, else query
    float *tang = reinterpret_cast<float *>(owner + N2); // the train key points' angles (the rotation bin of a claim without a global round trip)
    int *mdist = reinterpret_cast<int *>(tang + N2);     // RV_INIT: vMatchedDistance
    for (int i = lane; i < N2; i += 64) {
        mask[i] = 0; owner[i] = (P.tblocked && P.tblocked[kb + i]) ? -2 : -1; tang[i] = P.check_orientation ? P.tkeys[kb + i].angle : 0.0f;
        if (V == RV_INIT) mdist[i] = INT_MAX;
    }
    if (lane < 32) s_hist[lane] = 0;
    __syncthreads();
    const unsigned long long bit = 1ull << lane, below = bit - 1;
    int n_claims = 0;
    // A batch's global reads are issued one (the first candidates) and two (start, count, flags, angle) batches ahead.  (Measured on a one-pair search of 2 000 queries:
    // 262 -> 230 us.  What is left is the rounds' walk over the lists -- a lane per query pays an LDS round trip per candidate, and the coarse levels' windows hold dozens:
    // staging a batch's lists in LDS cooperatively, or reading eight candidates' words at once, both measured slower, 368 and 329 us.)
    struct Meta { int q; long cs; int cnt; bool act, blk; float ang; };
    auto load_meta = [&](int b0) {
        Meta M{0, 0, 0, false, false, 0.0f};
        const int step = b0 + lane;
        M.act = step < s1;
        if (M.act) {
            M.q = P.qlist ? P.qlist[step] : step;
            M.cs = P.cstart[M.q]; M.cnt = P.ccount[M.q];
            if (V == RV_PROJ || V == RV_LOCAL) M.blk = P.blocks[M.q] != 0;
            if (P.check_orientation) M.ang = P.qkeys ? P.qkeys[M.q].angle : P.qangle[M.q];
        }
        return M;
    };
    Meta Mc = load_meta(s0), Mn = load_meta(s0 + 64);
    int2 rc[RS_NC], rn[RS_NC];
#pragma unroll
    for (int c = 0; c < RS_NC; c++) rc[c] = c < Mc.cnt ? P.cands[Mc.cs + c] : make_int2(0, 0);
    for (int b0 = s0; b0 < s1; b0 += 64) {
#pragma unroll
        for (int c = 0; c < RS_NC; c++) rn[c] = c < Mn.cnt ? P.cands[Mn.cs + c] : make_int2(0, 0);
        const Meta Mnn = load_meta(b0 + 128);
        const bool act = Mc.act;
        const int q = Mc.q, cnt = Mc.cnt;
        const long cs = Mc.cs;
        const bool myblk = Mc.blk;
        const unsigned long long blkmask = __ballot(myblk);
        int claim = -1, cdist = 0;
        for (;;) {
            int best = V == RV_INIT ? INT_MAX : 256, best2 = best, bidx = -1, blev = -1, blev2 = -1;
            auto visit = [&](int2 cd) {
                const int idx = cd.x & 0xffffff, dist = cd.y;
                // (frame to frame only the minimum matters, and only if it is at most TH_HIGH: a candidate that cannot become the accepted minimum is dropped before its
                //  key point's words are read -- most of a window's candidates are other corners at a Hamming distance near 128)
                if (V == RV_PROJ && (dist > TH_HIGH || dist >= best)) return;
                const unsigned long long m = mask[idx] & below;
                if (V == RV_PROJ || V == RV_LOCAL) {
                    bool blk;
                    if (m) blk = (blkmask >> (63 - __clzll((long long)m))) & 1;
                    else { const int o = owner[idx]; blk = o == -2 || (o >= 0 && (o & 1)); }
                    if (blk) return;
                } else if (V == RV_INIT) {
                    const int eff = m ? s_cd[63 - __clzll((long long)m)] : mdist[idx];
                    if (eff <= dist) return;
                } else {
                    if (m || owner[idx] != -1) return;
                }
                if (V == RV_PROJ) { if (dist < best) { best = dist; bidx = idx; } }
                else if (V == RV_LOCAL) {
                    const int lev = (int)((unsigned)cd.x >> 24);
                    if (dist < best) { best2 = best; best = dist; blev2 = blev; blev = lev; bidx = idx; }
                    else if (dist < best2) { blev2 = lev; best2 = dist; }
                } else {
                    if (dist < best) { best2 = best; best = dist; bidx = idx; }
                    else if (dist < best2) best2 = dist;
                }
            };
#pragma unroll
            for (int c = 0; c < RS_NC; c++) if (c < cnt) visit(rc[c]);
            for (int c = RS_NC; c < cnt; c++) visit(P.cands[cs + c]);
            bool accept;
            if (V == RV_PROJ) accept = best <= TH_HIGH;                                                                         // :1469
            else if (V == RV_LOCAL) accept = best <= TH_HIGH && !(blev == blev2 && (float)best > P.nnratio * (float)best2);      // :126-131
            else if (V == RV_INIT) accept = best <= TH_LOW && (float)best < (float)best2 * P.nnratio;                            // :476-478
            else if (V == RV_BOW) accept = best <= TH_LOW && (float)best < P.nnratio * (float)best2;                             // :266-268
            else if (V == RV_CLAIM) accept = best <= P.accept_dist;                                                              // :419, :1815
            else accept = best < TH_LOW && (float)best < P.nnratio * (float)best2;                                               // :625-627 (strict)
            const int nc = (accept && act && bidx >= 0) ? bidx : -1;
            const bool changed = nc != claim || (V == RV_INIT && nc >= 0 && best != cdist);
            __syncthreads(); // every lane has read the masks of this round
            if (nc != claim) {
                if (claim >= 0) atomicAnd(&mask[claim], ~bit);
                if (nc >= 0) atomicOr(&mask[nc], bit);
                claim = nc;
            }
            if (V == RV_INIT) { cdist = best; s_cd[lane] = best; }
            __syncthreads();
            if (__ballot(changed) == 0) break;
        }
        // commit: the highest claiming lane of a key point is the last writer of the sequential loop
        bool top = false; int bin = 0;
        if (claim >= 0) {
            top = (mask[claim] >> lane) == 1ull;
            if (P.check_orientation) bin = rot_bin(Mc.ang, tang[claim]) & 31;
        }
        __syncthreads();
        if (claim >= 0) {
            if (top) {
                if (V == RV_PROJ || V == RV_LOCAL) owner[claim] = ((q - qsub) << 1) | (int)myblk;
                else { owner[claim] = q - qsub; if (V == RV_INIT) mdist[claim] = cdist; }
            }
            mask[claim] = 0;
            if (P.check_orientation) atomicAdd(&s_hist[bin], 1);
        }
        if (act) P.q_rec[q] = claim >= 0 ? (claim | (bin << 24)) : -1;
        n_claims += __popcll(__ballot(claim >= 0));
        __syncthreads();
        Mc = Mn; Mn = Mnn;
#pragma unroll
        for (int c = 0; c < RS_NC; c++) rc[c] = rn[c];
    }
    // the rotation histogram's three maxima and the cut (:1496-1517, :506-527, :271-292, :630-651)
    const bool cut = P.check_orientation && V != RV_LOCAL;
    if (cut && lane == 0) { int i1 = -1, i2 = -1, i3 = -1; three_maxima(s_hist, HISTO_LENGTH, i1, i2, i3); s_ind[0] = i1; s_ind[1] = i2; s_ind[2] = i3; }
    __syncthreads();
    const int ind1 = cut ? s_ind[0] : -1, ind2 = cut ? s_ind[1] : -1, ind3 = cut ? s_ind[2] : -1;
    int n_cull = 0, n_keep = 0;
    for (int step = s0 + lane; step < s1; step += 64) {
        const int q = P.qlist ? P.qlist[step] : step;
        const int rec = __hip_atomic_load(&P.q_rec[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int res = -1;
        if (rec >= 0) {
            const int idx = rec & 0xffffff, bin = rec >> 24;
            const bool culled = cut && bin != ind1 && bin != ind2 && bin != ind3;
            if (V == RV_PROJ || V == RV_LOCAL || V == RV_BOW || V == RV_CLAIM) { if (culled) { owner[idx] = -1; n_cull++; } } // every claim of a cut bin clears the key point and counts (:1506-1512)
            else if (owner[idx] == q - qsub && !culled) { res = idx; n_keep++; }                             // a displaced or cut query has no match (:487-491, :516-522)
        }
        if (V == RV_INIT || V == RV_BOWKF) P.q_match[q] = res;
    }
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) { n_cull += __shfl_xor(n_cull, off); n_keep += __shfl_xor(n_keep, off); }
    if (V == RV_PROJ || V == RV_LOCAL || V == RV_BOW || V == RV_CLAIM)
        for (int i = lane; i < N2; i += 64) { const int o = owner[i]; P.train_match[out0 + i] = o >= 0 ? ((V == RV_BOW || V == RV_CLAIM) ? o : (o >> 1)) : -1; }
    if (lane == 0) P.nmatches[p] = (V == RV_INIT || V == RV_BOWKF) ? n_keep : n_claims - n_cull;
}

// ORBmatcher::Fuse's search (:934-981): per map point the best key point after the tests that need per-key-point data of the key frame; first minimum wins.  A thread per map point.
__global__ void __launch_bounds__(256) match_fuse_best(int n_mp, const long *cstart, const int *ccount, const int2 *cands, const cs_keypoint *keys, const float *u_right, const float *inv_level_sigma2,
                                                       int n_levels, const uint8_t *keys_static, const float *uv, const float *ur, const int *pred_level, const uint8_t *valid, int *best_idx, int *best_dist, int *err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_mp) return;
    int bestDist = 256, bestIdx = -1;
    if (valid[i]) {
        const float u = uv[i * 2], v = uv[i * 2 + 1];
        const long b = cstart[i]; const int n = ccount[i];
        for (int p = 0; p < n; p++) {
            const int2 cd = cands[b + p];
            const int idx = cd.x & 0xffffff;
            const cs_keypoint kp = keys[idx];
            const int kpLevel = kp.octave;
            if (kpLevel < pred_level[i] - 1 || kpLevel > pred_level[i]) continue;
            if (keys_static && !keys_static[idx]) continue;
            if (kpLevel < 0 || kpLevel >= n_levels) { *err = 1; break; }
            if (u_right[idx] >= 0) {
                const float ex = u - kp.x, ey = v - kp.y, er = ur[i] - u_right[idx];
                const float e2 = ex * ex + ey * ey + er * er;
                if (e2 * inv_level_sigma2[kpLevel] > 7.8) continue;
            } else {
                const float ex = u - kp.x, ey = v - kp.y;
                const float e2 = ex * ex + ey * ey;
                if (e2 * inv_level_sigma2[kpLevel] > 5.99) continue;
            }
            if (cd.y < bestDist) { bestDist = cd.y; bestIdx = idx; }
        }
    }
    best_idx[i] = bestIdx; best_dist[i] = bestDist;
}

// Fuse(pKF, Scw, ...) (:1096-1118) and both directions of SearchBySim3 (:1238-1266, :1321-1349): per map point the first strict minimum over its candidate list (the
// window and the level filter are match_candidates'); a key point with tblocked set (!KeysStatic) is no candidate.  accept < 0: best_idx as found (-1 / INT_MAX: none);
// otherwise best_idx = -1 unless best_dist <= accept.  A thread per map point.
__global__ void __launch_bounds__(256) match_map_best(int n_mp, const long *cstart, const int *ccount, const int2 *cands, const uint8_t *tblocked, int accept, int *best_idx, int *best_dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_mp) return;
    int bestDist = INT_MAX, bestIdx = -1;
    const long b = cstart[i]; const int n = ccount[i];
    for (int p = 0; p < n; p++) {
        const int2 cd = cands[b + p];
        const int idx = cd.x & 0xffffff;
        if (tblocked && tblocked[idx]) continue;
        if (cd.y < bestDist) { bestDist = cd.y; bestIdx = idx; }
    }
    best_idx[i] = (accept >= 0 && bestDist > accept) ? -1 : bestIdx;
    if (best_dist) best_dist[i] = bestDist;
}
// SearchBySim3's agreement pass (:1353-1368): matches12[i1] = vnMatch1[i1] where vnMatch2[vnMatch1[i1]] == i1, else -1; *n_found (zeroed by the caller) counts them
__global__ void __launch_bounds__(256) match_sim3_agree(int N1, const int *match1, int N2, const int *match2, int *matches12, int *n_found) {
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    if (i1 >= N1) return;
    const int idx2 = match1[i1];
    const bool ok = idx2 >= 0 && idx2 < N2 && match2[idx2] == i1;
    matches12[i1] = ok ? idx2 : -1;
    if (ok) atomicAdd(n_found, 1);
}

// The orientation cut of a search whose matches are independent of each other (SearchForTriangulation, :801-830): histogram, three maxima, cut, count.  One workgroup.
__global__ void __launch_bounds__(1024) match_orient_cut(int N1, const cs_keypoint *keys1, const cs_keypoint *keys2, int *matches12, int check_orientation, int *nmatches) {
    __shared__ int s_hist[32], s_ind[3], s_n;
    const int tid = threadIdx.x;
    if (tid < 32) s_hist[tid] = 0;
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (check_orientation)
        for (int i = tid; i < N1; i += 1024) { const int m = matches12[i]; if (m >= 0) atomicAdd(&s_hist[rot_bin(keys1[i].angle, keys2[m].angle) & 31], 1); }
    __syncthreads();
    if (tid == 0) { int i1 = -1, i2 = -1, i3 = -1; if (check_orientation) three_maxima(s_hist, HISTO_LENGTH, i1, i2, i3); s_ind[0] = i1; s_ind[1] = i2; s_ind[2] = i3; }
    __syncthreads();
    int n = 0;
    for (int i = tid; i < N1; i += 1024) {
        const int m = matches12[i];
        if (m < 0) continue;
        if (check_orientation) { const int bin = rot_bin(keys1[i].angle, keys2[m].angle) & 31; if (bin != s_ind[0] && bin != s_ind[1] && bin != s_ind[2]) { matches12[i] = -1; continue; } }
        n++;
    }
    atomicAdd(&s_n, n);
    __syncthreads();
    if (tid == 0) *nmatches = s_n;
}

__global__ void __launch_bounds__(256) match_knn2(const unsigned long long *q, int nq, const unsigned long long *t, int nt, int *best_idx, int *best_dist,
                                                  int *second_dist) {
    __shared__ unsigned long long tile[256 * 4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long a[4] = {0, 0, 0, 0};
    if (i < nq) for (int k = 0; k < 4; k++) a[k] = q[(long)i * 4 + k];
    int b = INT_MAX, b2 = INT_MAX, bi = -1;
    for (int j0 = 0; j0 < nt; j0 += 256) {
        const int nj = min(256, nt - j0);
        __syncthreads();
        for (int k = threadIdx.x; k < nj * 4; k += 256) tile[k] = t[(long)j0 * 4 + k];
        __syncthreads();
        if (i < nq)
            for (int j = 0; j < nj; j++) {
                int d = hamming256(a, tile[j * 4], tile[j * 4 + 1], tile[j * 4 + 2], tile[j * 4 + 3]);
                if (d < b) { b2 = b; b = d; bi = j0 + j; }
                else if (d < b2) b2 = d;
            }
    }
    if (i < nq) { best_idx[i] = bi; best_dist[i] = b; second_dist[i] = b2; }
}

// SearchForTriangulation (:679-850): one wave per keypoint of KF1; lanes stride over the KF2 features of the same vocabulary node
// (ascending index).  The reference keeps the LAST candidate that reaches the running minimum (`dist > bestDist -> continue` lets
// equal distances through and the winner only changes on a candidate that passes the geometric tests), i.e. among the candidates
// that pass every test the smallest distance and, for equal distances, the largest index: min over the key dist << 20 | (2^20-1 - idx2).
struct TriP { float F12[9]; float ex, ey; int only_stereo; };
__global__ void __launch_bounds__(256) match_triangulation(int N1, const cs_keypoint *keys1, const unsigned long long *desc1, const int *node1, const uint8_t *skip1,
                                                           const float *ur1, const cs_keypoint *keys2, const unsigned long long *desc2, const uint8_t *skip2,
                                                           const float *ur2, const int *node_start2, const int *node_items2, int n_nodes, TriP P,
                                                           const float *scale2, const float *sigma2_2, int *matches12) {
    const int i1 = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i1 >= N1) return;
    unsigned best = 0xffffffffu;
    const int nd = node1[i1];
    const bool stereo1 = ur1[i1] >= 0;
    if (nd >= 0 && nd < n_nodes && !skip1[i1] && !(P.only_stereo && !stereo1)) {
        const cs_keypoint kp1 = keys1[i1];
        const unsigned long long a0 = desc1[(long)i1 * 4], a1 = desc1[(long)i1 * 4 + 1], a2 = desc1[(long)i1 * 4 + 2], a3 = desc1[(long)i1 * 4 + 3];
        // epipolar line l = x1' F12 (CheckDistEpipolarLine :152-169), float, no contraction
        const float a = kp1.x * P.F12[0] + kp1.y * P.F12[3] + P.F12[6];
        const float b = kp1.x * P.F12[1] + kp1.y * P.F12[4] + P.F12[7];
        const float c = kp1.x * P.F12[2] + kp1.y * P.F12[5] + P.F12[8];
        const float den = a * a + b * b;
        for (int p = node_start2[nd] + lane; p < node_start2[nd + 1]; p += 64) {
            const int i2 = node_items2[p];
            if (skip2[i2]) continue;
            const bool stereo2 = ur2[i2] >= 0;
            if (P.only_stereo && !stereo2) continue;
            const int dist = hamming256(desc2 + (long)i2 * 4, a0, a1, a2, a3);
            if (dist > TH_LOW) continue;
            const cs_keypoint kp2 = keys2[i2];
            if (!stereo1 && !stereo2) {
                const float dx = P.ex - kp2.x, dy = P.ey - kp2.y;
                if (dx * dx + dy * dy < 100 * scale2[kp2.octave]) continue;
            }
            const float num = a * kp2.x + b * kp2.y + c;
            if (den == 0) continue;
            const float dsqr = num * num / den;
            if (!((double)dsqr < 3.84 * (double)sigma2_2[kp2.octave])) continue;
            const unsigned key = ((unsigned)dist << 20) | (0xfffffu - (unsigned)i2);
            best = min(best, key);
        }
    }
    for (int off = 32; off > 0; off >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, off));
    if (lane == 0) matches12[i1] = best == 0xffffffffu ? -1 : (int)(0xfffffu - (best & 0xfffffu));
}
// SearchByBoW (:171-310, :544-677): distances of every key-frame feature to the frame features of its vocabulary node, one wave per key-frame
// feature, written as that feature's candidate list (the node's features in ascending index, the slice length is the node's size); match_resolve claims in the reference's order.
__global__ void __launch_bounds__(256) match_bow_dists(int NK, const unsigned long long *descK, const int *nodeK, const unsigned long long *descF, const int *node_start,
                                                       const int *node_items, const long *out_off, int2 *cands) {
    const int ik = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ik >= NK) return;
    const int nd = nodeK[ik];
    if (nd < 0) return;
    const unsigned long long a0 = descK[(long)ik * 4], a1 = descK[(long)ik * 4 + 1], a2 = descK[(long)ik * 4 + 2], a3 = descK[(long)ik * 4 + 3];
    const int b = node_start[nd], n = node_start[nd + 1] - b;
    for (int p = lane; p < n; p += 64) { const int iF = node_items[b + p]; cands[out_off[ik] + p] = make_int2(iF, hamming256(descF + (long)iF * 4, a0, a1, a2, a3)); }
}

} // namespace

// The features of one set by vocabulary node: the node ids that occur, compacted to 0 .. n_nodes - 1 in ascending order, and per node the features in ascending index
// (a counting sort): node k's features are items[start[k]] .. items[start[k + 1]].
struct NodeLists {
    std::vector<int> ids, start, items; int n_nodes = 0;
    int compact(int nd) const { if (nd < 0) return -1; auto it = std::lower_bound(ids.begin(), ids.end(), nd); return (it != ids.end() && *it == nd) ? (int)(it - ids.begin()) : -1; }
    NodeLists(const int *node, int N) {
        for (int i = 0; i < N; i++) if (node[i] >= 0) ids.push_back(node[i]);
        std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        n_nodes = (int)ids.size();
        std::vector<int> nc((size_t)N);
        start.assign((size_t)n_nodes + 1, 0);
        for (int i = 0; i < N; i++) { nc[i] = compact(node[i]); if (nc[i] >= 0) start[nc[i] + 1]++; }
        for (int k = 0; k < n_nodes; k++) start[k + 1] += start[k];
        items.resize((size_t)std::max(start[n_nodes], 1));
        std::vector<int> pos(start.begin(), start.end() - 1);
        for (int i = 0; i < N; i++) if (nc[i] >= 0) items[pos[nc[i]]++] = i;
    }
};

static FrameP make_frame(int N, float minX, float maxX, float minY, float maxY) {
    FrameP F; F.N = N; F.minX = minX; F.maxX = maxX; F.minY = minY; F.maxY = maxY;
    F.wInv = static_cast<float>(GRID_COLS) / static_cast<float>(maxX - minX); // Frame.cc:285-286
    F.hInv = static_cast<float>(GRID_ROWS) / static_cast<float>(maxY - minY);
    return F;
}
// What a search left in the two cursor words ([0] what the candidate arena should have held, [1] an error flag in its low word), after a wait for everything queued before.
static int mt_cursor(cs_ctx *ctx, const unsigned long long *d_cursor, long cap, long *last_c) {
    unsigned long long cur[2] = {0, 0};
    CS_TRY(cs_d2h(ctx, cur, d_cursor, 2));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *last_c = (long)cur[0];
    if ((long)cur[0] > cap) { ctx->err = "matcher candidate capacity exceeded"; return CS_ERR_CAPACITY; }
    if ((int)(cur[1] & 0xffffffffu)) return CS_ERR_BAD_ARG; // a level outside the scale / sigma table
    return CS_OK;
}

struct cs_matcher {
    int max_kp = 0, max_q = 0; long max_cand = 0;
    FrameP F{};
    cs_owner own;
    std::vector<cs_keypoint> keys; // host copy of mvKeysUn (what set_frame_from_orb hands back; the vbPrevMatched update of SearchForInitialization)
    // the frame: per key point (max_kp) and its grid
    cs_keypoint *d_keys = nullptr; unsigned long long *d_desc = nullptr; float *d_ur = nullptr; uint8_t *d_tb = nullptr;
    float *d_uright = nullptr; bool has_uright = false; // the frame's mvuRight for the stereo searches (cs_matcher_set_u_right); every cs_matcher_set_frame* detaches it
    int *d_cell_start = nullptr, *d_cell_items = nullptr, *d_kp_cell = nullptr, *d_tm = nullptr /* max_kp + 1: train_match, nmatches behind its N entries */; CellRec *d_cell_recs = nullptr;
    // the queries: per query (max_q)
    QueryS *d_q = nullptr; unsigned long long *d_qdesc = nullptr; long *d_cstart = nullptr;
    int *d_ccount = nullptr, *d_qrec = nullptr, *d_qm = nullptr /* max_q + 1 */, *d_level = nullptr;
    float *d_wp = nullptr /* x 3 */, *d_uv = nullptr /* x 2 */, *d_qur = nullptr, *d_ang = nullptr; uint8_t *d_valid = nullptr, *d_blocks = nullptr;
    float *d_T = nullptr /* 12 */, *d_sf = nullptr /* 32 */, *d_inv = nullptr /* 32 */; // a pose and the per-level tables (n_levels <= 32)
    float *d_nrm = nullptr /* x 3 */, *d_mind = nullptr, *d_maxd = nullptr; int *d_nout = nullptr /* 2 */; // the Sim3 / relocalisation preamble: normals, distance ranges; points outside the scale table, nFound
    float *d_proj = nullptr /* x 3 */; uint8_t *d_inview = nullptr; // what the frustum / Fuse preamble leaves per map point: (u, v, uR), mbTrackInView (the viewing cosine goes to d_ang)
    int2 *d_cands = nullptr; unsigned long long *d_cursor = nullptr; // [0] the arena's cursor, [1] an error flag (its low word)
    std::vector<int> h_res; int h_nout[2] = {0, 0};
    long last_q = 0, last_c = 0;
};

// the window enumeration of nq queries in m->d_q against the frame set with cs_matcher_set_frame: cursor reset + one launch, nothing waits
// ur_q != NULL: the stereo form -- the queries' predicted right coordinates (ur_q[q * ur_stride]) against the mvuRight attached with cs_matcher_set_u_right
static int mt_candidates(cs_ctx *ctx, cs_matcher *m, int nq, bool with_desc, const float *ur_q = nullptr, int ur_stride = 0) {
    CS_HIP(ctx, hipMemsetAsync(m->d_cursor, 0, 16, ctx->stream));
    if (ur_q)
        CS_LAUNCH(ctx, "match_candidates", match_candidates<true>, dim3((nq + MC_Q - 1) / MC_Q), dim3(256), 0, m->F, m->d_desc, (const int *)nullptr, m->d_cell_start, m->d_cell_recs, nq, m->d_q,
                  with_desc ? m->d_qdesc : (const unsigned long long *)nullptr, m->d_cursor, m->max_cand, m->d_cstart, m->d_ccount, m->d_cands, StereoC{m->d_uright, ur_q, ur_stride});
    else
        CS_LAUNCH(ctx, "match_candidates", match_candidates<false>, dim3((nq + MC_Q - 1) / MC_Q), dim3(256), 0, m->F, m->d_desc, (const int *)nullptr, m->d_cell_start, m->d_cell_recs, nq, m->d_q,
                  with_desc ? m->d_qdesc : (const unsigned long long *)nullptr, m->d_cursor, m->max_cand, m->d_cstart, m->d_ccount, m->d_cands, StereoC{nullptr, nullptr, 0});
    m->last_q = nq;
    return CS_OK;
}
template <int V> static int mt_resolve(cs_ctx *ctx, const ResolveP &P, int n_problems, int n2max) {
    const size_t lds = (size_t)std::max(n2max, 1) * (V == RV_INIT ? 20 : 16) + 16;
    if (lds > 150 * 1024) { ctx->err = "match_resolve: more train key points than one workgroup's LDS holds"; return CS_ERR_CAPACITY; }
    if (lds > 48 * 1024) CS_HIP(ctx, hipFuncSetAttribute((const void *)match_resolve<V>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CS_LAUNCH(ctx, "match_resolve", match_resolve<V>, dim3(n_problems), dim3(64), lds, P);
    return CS_OK;
}
// results (n_res ints and the match count behind them) + the cursor, one wait
static int mt_finish(cs_ctx *ctx, cs_matcher *m, const int *d_res, int n_res, int *out, int *nmatches) {
    m->h_res.resize((size_t)n_res + 1);
    CS_TRY(cs_d2h(ctx, m->h_res.data(), d_res, (size_t)n_res + 1));
    CS_TRY(mt_cursor(ctx, m->d_cursor, m->max_cand, &m->last_c));
    if (n_res) memcpy(out, m->h_res.data(), sizeof(int) * (size_t)n_res);
    *nmatches = m->h_res[(size_t)n_res];
    return CS_OK;
}
static int mt_alloc(cs_ctx *ctx, cs_matcher *m) {
    const size_t nk = (size_t)m->max_kp, nq = (size_t)m->max_q;
    cs_owner &o = m->own;
    CS_TRY(o.alloc(ctx, &m->d_keys, nk)); CS_TRY(o.alloc(ctx, &m->d_desc, nk * 4)); CS_TRY(o.alloc(ctx, &m->d_ur, nk)); CS_TRY(o.alloc(ctx, &m->d_tb, nk)); CS_TRY(o.alloc(ctx, &m->d_uright, nk));
    CS_TRY(o.alloc(ctx, &m->d_cell_start, (size_t)NCELL + 1)); CS_TRY(o.alloc(ctx, &m->d_cell_items, nk)); CS_TRY(o.alloc(ctx, &m->d_kp_cell, nk)); CS_TRY(o.alloc(ctx, &m->d_tm, nk + 1));
    CS_TRY(o.alloc(ctx, &m->d_cell_recs, nk));
    CS_TRY(o.alloc(ctx, &m->d_q, nq)); CS_TRY(o.alloc(ctx, &m->d_qdesc, nq * 4)); CS_TRY(o.alloc(ctx, &m->d_cstart, nq));
    CS_TRY(o.alloc(ctx, &m->d_ccount, nq)); CS_TRY(o.alloc(ctx, &m->d_qrec, nq + 1)); CS_TRY(o.alloc(ctx, &m->d_qm, nq + 1)); CS_TRY(o.alloc(ctx, &m->d_level, nq));
    CS_TRY(o.alloc(ctx, &m->d_wp, nq * 3)); CS_TRY(o.alloc(ctx, &m->d_uv, nq * 2)); CS_TRY(o.alloc(ctx, &m->d_qur, nq)); CS_TRY(o.alloc(ctx, &m->d_ang, nq));
    CS_TRY(o.alloc(ctx, &m->d_valid, nq)); CS_TRY(o.alloc(ctx, &m->d_blocks, nq));
    CS_TRY(o.alloc(ctx, &m->d_T, (size_t)12)); CS_TRY(o.alloc(ctx, &m->d_sf, (size_t)32)); CS_TRY(o.alloc(ctx, &m->d_inv, (size_t)32));
    CS_TRY(o.alloc(ctx, &m->d_nrm, nq * 3)); CS_TRY(o.alloc(ctx, &m->d_mind, nq)); CS_TRY(o.alloc(ctx, &m->d_maxd, nq)); CS_TRY(o.alloc(ctx, &m->d_nout, (size_t)2));
    CS_TRY(o.alloc(ctx, &m->d_proj, nq * 3)); CS_TRY(o.alloc(ctx, &m->d_inview, nq));
    CS_TRY(o.alloc(ctx, &m->d_cands, (size_t)m->max_cand)); CS_TRY(o.alloc(ctx, &m->d_cursor, (size_t)2));
    return CS_OK;
}

struct cs_match_stream {
    cs_owner own;
    cs_dbuf<cs_keypoint> keys; cs_dbuf<int> cell_start, cell_items, kp_cell, kfirst, qfirst, ccount, qrec, tm, nm; cs_dbuf<CellRec> cell_recs; cs_dbuf<long> cstart; cs_dbuf<QueryS> q; cs_dbuf<int2> cands;
    cs_dbuf<float> wp, T; cs_dbuf<uint8_t> valid, blocks; cs_dbuf<unsigned long long> qdesc;
    cs_dbuf<float> ur, qur; cs_dbuf<int> dir; // the stereo form: mvuRight over the window's key points, the queries' predicted right coordinates, a direction per pair
    float *d_sf = nullptr; unsigned long long *d_cursor = nullptr;
    std::vector<int> h_tm;
    long last_q = 0, last_c = 0;
};
int cs_matcher_device_grid(const cs_matcher *m, cs_matcher_grid_view *out) {
    if (!m || !out || !(m->F.wInv > 0.0f)) return CS_ERR_BAD_ARG; // (no frame was ever set: the cell lists hold nothing yet)
    static_assert(sizeof(CellRec) == 16, "klt_math.h's KltCellRec names the same four words: x, y, id, octave");
    *out = cs_matcher_grid_view{m->F.N, m->F.minX, m->F.minY, m->F.wInv, m->F.hInv, m->d_cell_start, m->d_cell_recs};
    return CS_OK;
}

extern "C" {

void cs_matcher_destroy(cs_ctx *ctx, cs_matcher *m) {
    if (!m) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    m->own.free_all(ctx);
    delete m;
}

int cs_matcher_last_counts(const cs_matcher *m, int *queries, long *candidates) { // workload facts of the last search, for roofline accounting
    if (!m || !queries || !candidates) return CS_ERR_BAD_ARG;
    *queries = (int)m->last_q;
    *candidates = m->last_c;
    return CS_OK;
}

int cs_matcher_create(cs_ctx *ctx, int max_keypoints, int max_queries, long max_candidates, cs_matcher **out) {
    if (!ctx || !out || max_keypoints < 1 || max_keypoints >= (1 << 24) || max_queries < 1 || max_candidates < 1) return CS_ERR_BAD_ARG;
    *out = nullptr;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_matcher *m = new (std::nothrow) cs_matcher();
    if (!m) return CS_ERR_NOMEM;
    m->max_kp = max_keypoints; m->max_q = max_queries; m->max_cand = max_candidates;
    const int r = mt_alloc(ctx, m);
    if (r != CS_OK) { cs_matcher_destroy(ctx, m); return r; }
    *out = m;
    return CS_OK;
}

int cs_matcher_set_frame(cs_ctx *ctx, cs_matcher *m, const cs_keypoint *keysUn, const uint8_t *desc, int N, float minX, float maxX, float minY,
                         float maxY) {
    if (!ctx || !m || !keysUn || !desc || N < 0 || N > m->max_kp || !(maxX > minX) || !(maxY > minY)) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    m->F = make_frame(N, minX, maxX, minY, maxY); m->has_uright = false;
    m->keys.assign(keysUn, keysUn + N);
    CS_TRY(cs_h2d(ctx, m->d_keys, keysUn, (size_t)N));
    CS_TRY(cs_h2d(ctx, (uint8_t *)m->d_desc, desc, (size_t)N * 32));
    CS_LAUNCH(ctx, "match_grid", match_grid, dim3(1), dim3(1024), 0, m->F, m->d_keys, (const int *)nullptr, m->d_cell_start, m->d_cell_items, m->d_kp_cell, m->d_cell_recs);
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_frame_image_bounds(int cols, int rows, const float *K4, const float *dist5, float *bounds) { // Frame::ComputeImageBounds (Frame.cc:578-609)
    if (!K4 || !bounds || cols < 1 || rows < 1) return CS_ERR_BAD_ARG;
    const UndP U = make_undp(K4, dist5);
    if (U.identity) { bounds[0] = 0.0f; bounds[1] = (float)cols; bounds[2] = 0.0f; bounds[3] = (float)rows; return CS_OK; }
    const float cx[4] = {0.0f, (float)cols, 0.0f, (float)cols}, cy[4] = {0.0f, 0.0f, (float)rows, (float)rows};
    float ux[4], uy[4];
    for (int i = 0; i < 4; i++) undistort_point(U, cx[i], cy[i], ux[i], uy[i]);
    bounds[0] = std::min(ux[0], ux[2]); bounds[1] = std::max(ux[1], ux[3]); bounds[2] = std::min(uy[0], uy[1]); bounds[3] = std::max(uy[2], uy[3]);
    return CS_OK;
}
int cs_matcher_set_frame_from_orb(cs_ctx *ctx, cs_matcher *m, const cs_orb *orb, int frame, const float *K4, const float *dist5, float minX, float maxX, float minY,
                                  float maxY, cs_keypoint *keysUn_out, int *n_out) {
    if (!ctx || !m || !orb || !K4 || !(maxX > minX) || !(maxY > minY)) return CS_ERR_BAD_ARG;
    const cs_keypoint *d_k = nullptr; const unsigned long long *d_d = nullptr; int N = 0;
    CS_TRY(cs_orb_device_frame(orb, frame, &d_k, &d_d, &N));
    if (N > m->max_kp) return CS_ERR_CAPACITY;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    m->F = make_frame(N, minX, maxX, minY, maxY); m->has_uright = false;
    // UndistortKeyPoints + the descriptors, device to device; AssignFeaturesToGrid on the undistorted keypoints
    if (N > 0) {
        CS_LAUNCH(ctx, "match_undistort", match_undistort, dim3((N + 255) / 256), dim3(256), 0, N, d_k, make_undp(K4, dist5), m->d_keys);
        CS_HIP(ctx, hipMemcpyAsync(m->d_desc, d_d, (size_t)N * 32, hipMemcpyDeviceToDevice, ctx->stream));
    }
    CS_LAUNCH(ctx, "match_grid", match_grid, dim3(1), dim3(1024), 0, m->F, m->d_keys, (const int *)nullptr, m->d_cell_start, m->d_cell_items, m->d_kp_cell, m->d_cell_recs);
    // mvKeysUn for the caller (and for SearchForInitialization's vbPrevMatched update); a caller that wants neither passes NULL and the frame stays on the device:
    // every search takes what it needs of a train key point from the device copy
    if (keysUn_out) {
        m->keys.resize((size_t)N);
        CS_TRY(cs_d2h(ctx, m->keys.data(), m->d_keys, (size_t)N));
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(keysUn_out, m->keys.data(), sizeof(cs_keypoint) * (size_t)N);
    } else m->keys.clear();
    if (n_out) *n_out = N;
    return CS_OK;
}

int cs_matcher_features_in_area(cs_ctx *ctx, cs_matcher *m, float x, float y, float r, int minLevel, int maxLevel, int *out, int cap, int *n) {
    if (!ctx || !m || !n) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    QueryS Q{x, y, r, minLevel, maxLevel, 1, 0};
    CS_TRY(cs_h2d(ctx, m->d_q, &Q, 1));
    CS_TRY(mt_candidates(ctx, m, 1, false));
    long start = 0; int cnt = 0;
    CS_TRY(cs_d2h(ctx, &start, m->d_cstart, 1));
    CS_TRY(cs_d2h(ctx, &cnt, m->d_ccount, 1));
    CS_TRY(mt_cursor(ctx, m->d_cursor, m->max_cand, &m->last_c));
    *n = cnt;
    if (out && cnt > 0 && cap > 0) {
        std::vector<int2> c((size_t)cnt);
        CS_TRY(cs_d2h(ctx, c.data(), m->d_cands + start, (size_t)cnt));
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < cnt && i < cap; i++) out[i] = c[i].x & 0xffffff;
    }
    return CS_OK;
}

} // extern "C"
// cs_match_by_projection_frame and its stereo form (stereo: direction `dir`, mbf `bf`, the attached mvuRight)
static int mt_by_projection_frame(cs_ctx *ctx, cs_matcher *m, int n_last, const float *world_pos, const uint8_t *valid, const uint8_t *blocks,
                                  const uint8_t *mp_desc, const int *last_octave, const float *last_angle, const float *Tcw, float fx, float fy, float cx,
                                  float cy, const float *scale_factors, int n_levels, float th, int check_orientation, const uint8_t *train_blocked, int *train_match, int *nmatches,
                                  bool stereo, int dir, float bf) {
    if (!ctx || !m || n_last < 0 || n_last > m->max_q || !world_pos || !valid || !blocks || !mp_desc || !last_octave || !last_angle || !Tcw ||
        !scale_factors || n_levels < 1 || n_levels > 32 || !train_match || !nmatches)
        return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < n_last; i++) if (valid[i] && (last_octave[i] < 0 || last_octave[i] >= n_levels)) return CS_ERR_BAD_ARG;
    const int N = m->F.N;
    *nmatches = 0;
    if (n_last == 0) { for (int i = 0; i < N; i++) train_match[i] = -1; return CS_OK; }
    CS_TRY(cs_h2d(ctx, m->d_wp, world_pos, (size_t)n_last * 3));
    CS_TRY(cs_h2d(ctx, m->d_T, Tcw, 12));
    CS_TRY(cs_h2d(ctx, m->d_sf, scale_factors, (size_t)n_levels));
    CS_TRY(cs_h2d(ctx, m->d_valid, valid, (size_t)n_last));
    CS_TRY(cs_h2d(ctx, m->d_blocks, blocks, (size_t)n_last));
    CS_TRY(cs_h2d(ctx, m->d_level, last_octave, (size_t)n_last));
    CS_TRY(cs_h2d(ctx, (uint8_t *)m->d_qdesc, mp_desc, (size_t)n_last * 32));
    if (check_orientation) CS_TRY(cs_h2d(ctx, m->d_ang, last_angle, (size_t)n_last));
    if (train_blocked) CS_TRY(cs_h2d(ctx, m->d_tb, train_blocked, (size_t)N)); // map point from before the call / KeysStatic[i2] == false, :1451-1457
    // (the levels were checked above, before anything was queued; the kernel's own check only keeps its read of the scale table in range)
    if (stereo) {
        CS_LAUNCH(ctx, "match_project", match_project<true>, dim3((n_last + 255) / 256), dim3(256), 0, n_last, 1, (const int *)nullptr, m->d_wp, m->d_valid, m->d_level, (const cs_keypoint *)nullptr,
                  m->d_T, fx, fy, cx, cy, m->d_sf, n_levels, th, m->F, m->d_q, reinterpret_cast<int *>(m->d_cursor + 1), StereoQ{nullptr, dir, bf, m->d_qur});
        CS_TRY(mt_candidates(ctx, m, n_last, true, m->d_qur, 1));
    } else {
        CS_LAUNCH(ctx, "match_project", match_project<false>, dim3((n_last + 255) / 256), dim3(256), 0, n_last, 1, (const int *)nullptr, m->d_wp, m->d_valid, m->d_level, (const cs_keypoint *)nullptr,
                  m->d_T, fx, fy, cx, cy, m->d_sf, n_levels, th, m->F, m->d_q, reinterpret_cast<int *>(m->d_cursor + 1), StereoQ{nullptr, 0, 0.0f, nullptr});
        CS_TRY(mt_candidates(ctx, m, n_last, true));
    }
    // the greedy pass (:1397-1494) and the rotation cut (:1496-1517), on the device
    ResolveP P{};
    P.cstart = m->d_cstart; P.ccount = m->d_ccount; P.cands = m->d_cands; P.n_steps = n_last; P.n_train = N; P.tkeys = m->d_keys; P.qangle = m->d_ang; P.blocks = m->d_blocks;
    P.tblocked = train_blocked ? m->d_tb : nullptr; P.check_orientation = check_orientation; P.train_match = m->d_tm; P.q_rec = m->d_qrec; P.nmatches = m->d_tm + N;
    CS_TRY(mt_resolve<RV_PROJ>(ctx, P, 1, N));
    return mt_finish(ctx, m, m->d_tm, N, train_match, nmatches);
}
extern "C" {
int cs_match_by_projection_frame(cs_ctx *ctx, cs_matcher *m, int n_last, const float *world_pos, const uint8_t *valid, const uint8_t *blocks,
                                 const uint8_t *mp_desc, const int *last_octave, const float *last_angle, const float *Tcw, float fx, float fy, float cx,
                                 float cy, const float *scale_factors, int n_levels, float th, int check_orientation, const uint8_t *train_blocked, int *train_match, int *nmatches) {
    return mt_by_projection_frame(ctx, m, n_last, world_pos, valid, blocks, mp_desc, last_octave, last_angle, Tcw, fx, fy, cx, cy, scale_factors, n_levels, th, check_orientation, train_blocked,
                                  train_match, nmatches, false, SS_NEITHER, 0.0f);
}

// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1373-1522) for the pairs (f0 + p, f0 + p + 1), p < n_pairs, of the frames `orb` holds in HBM, with
// Frame::UndistortKeyPoints + AssignFeaturesToGrid (Frame.cc:303-318, 546-576) of every current frame: see include/cubeslam_hip.h.
void cs_match_stream_destroy(cs_ctx *ctx, cs_match_stream *m) {
    if (!m) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    m->own.free_all(ctx);
    delete m;
}
int cs_match_stream_create(cs_match_stream **out) {
    if (!out) return CS_ERR_BAD_ARG;
    *out = new (std::nothrow) cs_match_stream();
    return *out ? CS_OK : CS_ERR_NOMEM;
}
int cs_match_stream_last_counts(const cs_match_stream *m, long *queries, long *candidates) {
    if (!m || !queries || !candidates) return CS_ERR_BAD_ARG;
    *queries = m->last_q; *candidates = m->last_c;
    return CS_OK;
}
} // extern "C"
// cs_match_by_projection_stream and its stereo form.  SQ != NULL: the stereo form -- SQ->dir holds a direction per pair (host), SQ->bf = mbf, u_right the packed mvuRight of the current
// frames (n_train values, host or device)
struct StreamStereo { const int *dir; float bf; const float *u_right; int on_device; };
static int mt_by_projection_stream(cs_ctx *ctx, cs_match_stream *m, const cs_orb *orb, int f0, int n_pairs, const float *K4, const float *dist5, float minX, float maxX, float minY, float maxY,
                                   int n_queries, int n_train, const float *world_pos, const uint8_t *valid, const uint8_t *blocks, const uint8_t *mp_desc, const float *Tcw, float fx, float fy, float cx, float cy,
                                   const float *scale_factors, int n_levels, float th, int check_orientation, int *train_match, int *nmatches, const StreamStereo *SQ) {
    if (!ctx || !m || !orb || n_pairs < 1 || f0 < 0 || !K4 || !(maxX > minX) || !(maxY > minY) || !world_pos || !valid || !blocks || !Tcw || !scale_factors || n_levels < 1 || n_levels > 32 || !train_match || !nmatches)
        return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    // the frames f0 .. f0 + n_pairs lie one behind the other in the extractor's buffers
    std::vector<int> first((size_t)n_pairs + 2);
    const cs_keypoint *d_k0 = nullptr; const unsigned long long *d_d0 = nullptr;
    { int n0 = 0; CS_TRY(cs_orb_device_frame(orb, f0, &d_k0, &d_d0, &n0)); first[0] = 0; first[1] = n0; }
    for (int p = 1; p <= n_pairs; p++) {
        const cs_keypoint *dk; const unsigned long long *dd; int n = 0;
        CS_TRY(cs_orb_device_frame(orb, f0 + p, &dk, &dd, &n));
        if (dk != d_k0 + first[p]) { ctx->err = "cs_match_by_projection_stream: the extractor's frames are not contiguous"; return CS_ERR_BAD_ARG; }
        first[p + 1] = first[p] + n;
    }
    const int nq = first[n_pairs], nk_all = first[n_pairs + 1]; // queries: key points of frames f0 .. f0 + n_pairs - 1; train key points: frames f0 + 1 .. f0 + n_pairs (indices first[1] ..)
    const int nk = nk_all - first[1];
    // the caller sized world_pos / valid / blocks / mp_desc for n_queries and train_match for n_train: they must be what the extractor holds NOW
    if (n_queries != nq || n_train != nk) { ctx->err = "cs_match_by_projection_stream: n_queries / n_train differ from the extractor's key point counts"; return CS_ERR_BAD_ARG; }
    for (int p = 0; p < n_pairs; p++) nmatches[p] = 0;
    for (int i = 0; i < nk; i++) train_match[i] = -1;
    m->last_q = nq; m->last_c = 0;
    if (nq == 0 || nk == 0) return CS_OK;
    if (nk_all >= (1 << 24)) { int nmax = 0; for (int p = 1; p <= n_pairs; p++) nmax = std::max(nmax, first[p + 1] - first[p]); if (nmax >= (1 << 24)) return CS_ERR_CAPACITY; }
    const FrameP F = make_frame(0, minX, maxX, minY, maxY);
    CS_TRY(m->keys.grow(ctx, m->own, (size_t)nk_all)); CS_TRY(m->cell_items.grow(ctx, m->own, (size_t)nk_all)); CS_TRY(m->cell_recs.grow(ctx, m->own, (size_t)nk_all)); CS_TRY(m->kp_cell.grow(ctx, m->own, (size_t)nk_all)); CS_TRY(m->tm.grow(ctx, m->own, (size_t)nk));
    CS_TRY(m->cell_start.grow(ctx, m->own, (size_t)n_pairs * (NCELL + 1))); CS_TRY(m->kfirst.grow(ctx, m->own, (size_t)n_pairs + 2)); CS_TRY(m->qfirst.grow(ctx, m->own, (size_t)n_pairs + 2)); CS_TRY(m->T.grow(ctx, m->own, (size_t)n_pairs * 12)); CS_TRY(m->nm.grow(ctx, m->own, (size_t)n_pairs));
    CS_TRY(m->ccount.grow(ctx, m->own, (size_t)nq)); CS_TRY(m->cstart.grow(ctx, m->own, (size_t)nq)); CS_TRY(m->qrec.grow(ctx, m->own, (size_t)nq)); CS_TRY(m->q.grow(ctx, m->own, (size_t)nq)); CS_TRY(m->wp.grow(ctx, m->own, (size_t)nq * 3)); CS_TRY(m->valid.grow(ctx, m->own, (size_t)nq));
    CS_TRY(m->blocks.grow(ctx, m->own, (size_t)nq)); if (mp_desc) CS_TRY(m->qdesc.grow(ctx, m->own, (size_t)nq * 4));
    if (!m->d_sf) CS_TRY(m->own.alloc(ctx, &m->d_sf, (size_t)32));
    if (!m->d_cursor) CS_TRY(m->own.alloc(ctx, &m->d_cursor, (size_t)2));
    if (!m->cands.p) CS_TRY(m->cands.grow(ctx, m->own, std::max((size_t)nq * 12, (size_t)1 << 16))); // (5.6 candidates per query at th 15 on the bench stream; the cursor says what a window really needs)
    // UndistortKeyPoints of every frame of the window (device to device), AssignFeaturesToGrid of the current frames
    CS_LAUNCH(ctx, "match_undistort", match_undistort, dim3((nk_all + 255) / 256), dim3(256), 0, nk_all, d_k0, make_undp(K4, dist5), m->keys.p);
    std::vector<int> kfirst((size_t)n_pairs + 1);
    int n2max = 0;
    for (int p = 0; p <= n_pairs; p++) { kfirst[p] = first[p + 1]; if (p < n_pairs) n2max = std::max(n2max, first[p + 2] - first[p + 1]); } // train frame of pair p: key points kfirst[p] .. kfirst[p + 1] of the window's list
    CS_TRY(cs_h2d(ctx, m->kfirst.p, kfirst.data(), (size_t)n_pairs + 1));
    CS_TRY(cs_h2d(ctx, m->qfirst.p, first.data(), (size_t)n_pairs + 1));
    CS_TRY(cs_h2d(ctx, m->T.p, Tcw, (size_t)n_pairs * 12));
    CS_TRY(cs_h2d(ctx, m->d_sf, scale_factors, (size_t)n_levels));
    CS_TRY(cs_h2d(ctx, m->wp.p, world_pos, (size_t)nq * 3));
    CS_TRY(cs_h2d(ctx, m->valid.p, valid, (size_t)nq));
    CS_TRY(cs_h2d(ctx, m->blocks.p, blocks, (size_t)nq));
    if (mp_desc) CS_TRY(cs_h2d(ctx, (uint8_t *)m->qdesc.p, mp_desc, (size_t)nq * 32));
    const unsigned long long *d_qdesc = mp_desc ? m->qdesc.p : d_d0; // NULL: a last frame's key point is matched with its own descriptor
    int *d_err = reinterpret_cast<int *>(m->d_cursor + 1);
    CS_HIP(ctx, hipMemsetAsync(m->d_cursor, 0, 16, ctx->stream));
    CS_LAUNCH(ctx, "match_grid", match_grid, dim3(n_pairs), dim3(1024), 0, F, m->keys.p, m->kfirst.p, m->cell_start.p, m->cell_items.p, m->kp_cell.p, m->cell_recs.p);
    if (SQ) { // train key point id of pair p is entry kfirst[p] + id of the window's key point list: mvuRight lies behind the first frame's (unused) entries
        CS_TRY(m->ur.grow(ctx, m->own, (size_t)nk_all)); CS_TRY(m->qur.grow(ctx, m->own, (size_t)nq)); CS_TRY(m->dir.grow(ctx, m->own, (size_t)n_pairs));
        CS_HIP(ctx, hipMemcpyAsync(m->ur.p + first[1], SQ->u_right, sizeof(float) * (size_t)nk, SQ->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
        CS_TRY(cs_h2d(ctx, m->dir.p, SQ->dir, (size_t)n_pairs));
        CS_LAUNCH(ctx, "match_project", match_project<true>, dim3((nq + 255) / 256), dim3(256), 0, nq, n_pairs, m->qfirst.p, m->wp.p, m->valid.p, (const int *)nullptr, d_k0, m->T.p, fx, fy, cx, cy, m->d_sf, n_levels, th, F, m->q.p, d_err,
                  StereoQ{m->dir.p, 0, SQ->bf, m->qur.p});
    } else
        CS_LAUNCH(ctx, "match_project", match_project<false>, dim3((nq + 255) / 256), dim3(256), 0, nq, n_pairs, m->qfirst.p, m->wp.p, m->valid.p, (const int *)nullptr, d_k0 /* query j = raw key point j of frame f0 on */, m->T.p, fx, fy, cx, cy, m->d_sf, n_levels, th, F, m->q.p, d_err,
                  StereoQ{nullptr, 0, 0.0f, nullptr});
    // every pair's window enumeration (one launch) and its greedy pass + rotation cut (:1397-1517; one wave per pair): nothing of a candidate leaves the device.  The arena's
    // size is last call's need; a window that needs more says so through the cursor and the two launches run again on a larger one.
    for (int attempt = 0;; attempt++) {
        if (SQ)
            CS_LAUNCH(ctx, "match_candidates", match_candidates<true>, dim3((nq + MC_Q - 1) / MC_Q), dim3(256), 0, F, d_d0, m->kfirst.p, m->cell_start.p, m->cell_recs.p, nq, m->q.p, d_qdesc, m->d_cursor, (long)m->cands.cap,
                      m->cstart.p, m->ccount.p, m->cands.p, StereoC{m->ur.p, m->qur.p, 1});
        else
            CS_LAUNCH(ctx, "match_candidates", match_candidates<false>, dim3((nq + MC_Q - 1) / MC_Q), dim3(256), 0, F, d_d0, m->kfirst.p, m->cell_start.p, m->cell_recs.p, nq, m->q.p, d_qdesc, m->d_cursor, (long)m->cands.cap,
                      m->cstart.p, m->ccount.p, m->cands.p, StereoC{nullptr, nullptr, 0});
        ResolveP P{};
        P.cstart = m->cstart.p; P.ccount = m->ccount.p; P.cands = m->cands.p; P.pfirst = m->qfirst.p; P.kfirst = m->kfirst.p; P.tkeys = m->keys.p; P.qkeys = m->keys.p; P.blocks = m->blocks.p;
        P.check_orientation = check_orientation; P.train_match = m->tm.p; P.q_rec = m->qrec.p; P.nmatches = m->nm.p;
        CS_TRY(mt_resolve<RV_PROJ>(ctx, P, n_pairs, n2max));
        const int r = mt_cursor(ctx, m->d_cursor, (long)m->cands.cap, &m->last_c); // (BAD_ARG: a valid query whose key point's level is outside the scale table)
        if (r == CS_OK) break;
        if (r != CS_ERR_CAPACITY) return r;
        if (attempt) { ctx->err = "cs_match_by_projection_stream: candidate arena"; return CS_ERR_CAPACITY; }
        CS_TRY(m->cands.grow(ctx, m->own, (size_t)m->last_c));
        CS_HIP(ctx, hipMemsetAsync(m->d_cursor, 0, 8, ctx->stream)); // (the cursor; match_project's error flag behind it stays)
    }
    CS_TRY(cs_d2h(ctx, train_match, m->tm.p, (size_t)nk));
    CS_TRY(cs_d2h(ctx, nmatches, m->nm.p, (size_t)n_pairs));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CS_OK;
}
extern "C" {
int cs_match_by_projection_stream(cs_ctx *ctx, cs_match_stream *m, const cs_orb *orb, int f0, int n_pairs, const float *K4, const float *dist5, float minX, float maxX, float minY, float maxY,
                                  int n_queries, int n_train, const float *world_pos, const uint8_t *valid, const uint8_t *blocks, const uint8_t *mp_desc, const float *Tcw, float fx, float fy, float cx, float cy,
                                  const float *scale_factors, int n_levels, float th, int check_orientation, int *train_match, int *nmatches) {
    return mt_by_projection_stream(ctx, m, orb, f0, n_pairs, K4, dist5, minX, maxX, minY, maxY, n_queries, n_train, world_pos, valid, blocks, mp_desc, Tcw, fx, fy, cx, cy, scale_factors, n_levels, th,
                                   check_orientation, train_match, nmatches, nullptr);
}

} // extern "C"
// cs_match_local_map and its stereo form (proj_xr != NULL: mTrackProjXR per map point, tested against the attached mvuRight, :104-109)
static int mt_local_map(cs_ctx *ctx, cs_matcher *m, int n_mp, const float *proj_xy, const float *view_cos, const int *pred_level, const uint8_t *in_view,
                        const uint8_t *blocks, const uint8_t *mp_desc, const float *scale_factors, int n_levels, float th, float nnratio,
                        const uint8_t *train_blocked, int *train_match, int *nmatches, const float *proj_xr) {
    if (!ctx || !m || n_mp < 0 || n_mp > m->max_q || !proj_xy || !view_cos || !pred_level || !in_view || !blocks || !mp_desc || !scale_factors ||
        !train_match || !nmatches)
        return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const int N = m->F.N;
    *nmatches = 0;
    if (n_mp == 0) { for (int i = 0; i < N; i++) train_match[i] = -1; return CS_OK; }
    const bool bFactor = th != 1.0;
    std::vector<QueryS> q((size_t)n_mp);
    for (int i = 0; i < n_mp; i++) { // :58-78 (window radius from the viewing cosine)
        QueryS Q{0, 0, 0, 0, 0, 0, 0};
        if (in_view[i]) {
            if (pred_level[i] < 0 || pred_level[i] >= n_levels) return CS_ERR_BAD_ARG;
            float r = view_cos[i] > 0.998 ? 2.5f : 4.0f;
            if (bFactor) r *= th;
            Q.x = proj_xy[i * 2]; Q.y = proj_xy[i * 2 + 1]; Q.r = r * scale_factors[pred_level[i]];
            Q.minLevel = pred_level[i] - 1; Q.maxLevel = pred_level[i]; Q.valid = 1;
        }
        q[i] = Q;
    }
    CS_TRY(cs_h2d(ctx, m->d_q, q.data(), (size_t)n_mp));
    CS_TRY(cs_h2d(ctx, (uint8_t *)m->d_qdesc, mp_desc, (size_t)n_mp * 32));
    CS_TRY(cs_h2d(ctx, m->d_blocks, blocks, (size_t)n_mp));
    if (train_blocked) CS_TRY(cs_h2d(ctx, m->d_tb, train_blocked, (size_t)N));
    if (proj_xr) { CS_TRY(cs_h2d(ctx, m->d_qur, proj_xr, (size_t)n_mp)); CS_TRY(mt_candidates(ctx, m, n_mp, true, m->d_qur, 1)); }
    else CS_TRY(mt_candidates(ctx, m, n_mp, true));
    ResolveP P{}; // :86-140: best / second with their levels, the ratio rule, claims
    P.cstart = m->d_cstart; P.ccount = m->d_ccount; P.cands = m->d_cands; P.n_steps = n_mp; P.n_train = N; P.tkeys = m->d_keys; P.blocks = m->d_blocks;
    P.tblocked = train_blocked ? m->d_tb : nullptr; P.nnratio = nnratio; P.check_orientation = 0; P.train_match = m->d_tm; P.q_rec = m->d_qrec; P.nmatches = m->d_tm + N;
    CS_TRY(mt_resolve<RV_LOCAL>(ctx, P, 1, N));
    return mt_finish(ctx, m, m->d_tm, N, train_match, nmatches);
}
extern "C" {
int cs_match_local_map(cs_ctx *ctx, cs_matcher *m, int n_mp, const float *proj_xy, const float *view_cos, const int *pred_level, const uint8_t *in_view,
                       const uint8_t *blocks, const uint8_t *mp_desc, const float *scale_factors, int n_levels, float th, float nnratio,
                       const uint8_t *train_blocked, int *train_match, int *nmatches) {
    return mt_local_map(ctx, m, n_mp, proj_xy, view_cos, pred_level, in_view, blocks, mp_desc, scale_factors, n_levels, th, nnratio, train_blocked, train_match, nmatches, nullptr);
}

int cs_match_for_initialization(cs_ctx *ctx, cs_matcher *m, const cs_keypoint *keys1, const uint8_t *desc1, int N1, float *prev, int window_size,
                                float nnratio, int check_orientation, int *vnMatches12, int *nmatches) {
    if (!ctx || !m || !keys1 || !desc1 || N1 < 0 || N1 > m->max_q || !prev || !vnMatches12 || !nmatches) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    *nmatches = 0;
    if (N1 == 0) return CS_OK;
    if ((int)m->keys.size() != m->F.N) { ctx->err = "cs_match_for_initialization: the frame was set without a host copy of its key points"; return CS_ERR_BAD_ARG; }
    std::vector<QueryS> q((size_t)N1);
    std::vector<float> ang((size_t)N1);
    for (int i = 0; i < N1; i++) { // :441-449: level-0 keypoints only, window around vbPrevMatched
        QueryS Q{0, 0, 0, 0, 0, 0, 0};
        if (!(keys1[i].octave > 0)) { Q.x = prev[i * 2]; Q.y = prev[i * 2 + 1]; Q.r = (float)window_size; Q.minLevel = keys1[i].octave; Q.maxLevel = keys1[i].octave; Q.valid = 1; }
        q[i] = Q; ang[i] = keys1[i].angle;
    }
    CS_TRY(cs_h2d(ctx, m->d_q, q.data(), (size_t)N1));
    CS_TRY(cs_h2d(ctx, (uint8_t *)m->d_qdesc, desc1, (size_t)N1 * 32));
    CS_TRY(cs_h2d(ctx, m->d_ang, ang.data(), (size_t)N1));
    CS_TRY(mt_candidates(ctx, m, N1, true));
    ResolveP P{}; // :451-504 (vMatchedDistance, vnMatches21 and the displacement of an earlier match) and :506-527
    P.cstart = m->d_cstart; P.ccount = m->d_ccount; P.cands = m->d_cands; P.n_steps = N1; P.n_train = m->F.N; P.tkeys = m->d_keys; P.qangle = m->d_ang;
    P.nnratio = nnratio; P.check_orientation = check_orientation; P.q_match = m->d_qm; P.q_rec = m->d_qrec; P.nmatches = m->d_qm + N1;
    CS_TRY(mt_resolve<RV_INIT>(ctx, P, 1, m->F.N));
    CS_TRY(mt_finish(ctx, m, m->d_qm, N1, vnMatches12, nmatches));
    for (int i1 = 0; i1 < N1; i1++) // :529-532
        if (vnMatches12[i1] >= 0) { prev[i1 * 2] = m->keys[vnMatches12[i1]].x; prev[i1 * 2 + 1] = m->keys[vnMatches12[i1]].y; }
    return CS_OK;
}

int cs_match_fuse(cs_ctx *ctx, cs_matcher *m, const float *u_right, const float *inv_level_sigma2, int n_levels, const uint8_t *keys_static, int n_mp, const float *uv,
                  const float *ur, const int *pred_level, const uint8_t *valid, const uint8_t *mp_desc, const float *scale_factors, float th, int *best_idx,
                  int *best_dist, int *n_fused) {
    if (!ctx || !m || n_mp < 0 || n_mp > m->max_q || !u_right || !inv_level_sigma2 || n_levels < 1 || n_levels > 32 || (n_mp && (!uv || !ur || !pred_level || !valid || !mp_desc)) ||
        !scale_factors || !best_idx || !best_dist || !n_fused)
        return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    *n_fused = 0;
    if (n_mp == 0) return CS_OK;
    const int N = m->F.N;
    std::vector<QueryS> q((size_t)n_mp);
    for (int i = 0; i < n_mp; i++) { // :921-926: GetFeaturesInArea(u, v, th * scale[level]) without level limits
        QueryS Q{0, 0, 0, -1, -1, 0, 0};
        if (valid[i]) {
            if (pred_level[i] < 0 || pred_level[i] >= n_levels) return CS_ERR_BAD_ARG;
            Q.x = uv[i * 2]; Q.y = uv[i * 2 + 1]; Q.r = th * scale_factors[pred_level[i]]; Q.valid = 1;
        }
        q[i] = Q;
    }
    CS_TRY(cs_h2d(ctx, m->d_q, q.data(), (size_t)n_mp));
    CS_TRY(cs_h2d(ctx, (uint8_t *)m->d_qdesc, mp_desc, (size_t)n_mp * 32));
    CS_TRY(cs_h2d(ctx, m->d_uv, uv, (size_t)n_mp * 2));
    CS_TRY(cs_h2d(ctx, m->d_qur, ur, (size_t)n_mp));
    CS_TRY(cs_h2d(ctx, m->d_inv, inv_level_sigma2, (size_t)n_levels));
    CS_TRY(cs_h2d(ctx, m->d_level, pred_level, (size_t)n_mp));
    CS_TRY(cs_h2d(ctx, m->d_valid, valid, (size_t)n_mp));
    CS_TRY(cs_h2d(ctx, m->d_ur, u_right, (size_t)N));
    if (keys_static) CS_TRY(cs_h2d(ctx, m->d_tb, keys_static, (size_t)N));
    CS_TRY(mt_candidates(ctx, m, n_mp, true));
    // :934-981: the tests that need per-keypoint data of the key frame, first minimum wins
    CS_LAUNCH(ctx, "match_fuse_best", match_fuse_best, dim3((n_mp + 255) / 256), dim3(256), 0, n_mp, m->d_cstart, m->d_ccount, m->d_cands, m->d_keys, m->d_ur, m->d_inv, n_levels,
              keys_static ? m->d_tb : (const uint8_t *)nullptr, m->d_uv, m->d_qur, m->d_level, m->d_valid, m->d_qm, m->d_qrec, reinterpret_cast<int *>(m->d_cursor + 1));
    CS_TRY(cs_d2h(ctx, best_idx, m->d_qm, (size_t)n_mp));
    CS_TRY(cs_d2h(ctx, best_dist, m->d_qrec, (size_t)n_mp));
    CS_TRY(mt_cursor(ctx, m->d_cursor, m->max_cand, &m->last_c)); // (BAD_ARG: a candidate's level outside the sigma table)
    int nf = 0;
    for (int i = 0; i < n_mp; i++) if (best_dist[i] <= TH_LOW) nf++;
    *n_fused = nf;
    return CS_OK;
}

int cs_match_for_triangulation(cs_ctx *ctx, const cs_keypoint *keys1Un, const uint8_t *desc1, int N1, const int *node1, const uint8_t *skip1, const float *u_right1,
                               const cs_keypoint *keys2Un, const uint8_t *desc2, int N2, const int *node2, const uint8_t *skip2, const float *u_right2,
                               const float *F12, float ex, float ey, const float *scale_factors2, const float *level_sigma2_2, int n_levels, int only_stereo,
                               int check_orientation, int *matches12, int *nmatches) {
    if (!ctx || N1 < 0 || N2 < 0 || N2 >= (1 << 20) || !matches12 || !nmatches || !F12 || !scale_factors2 || !level_sigma2_2 || n_levels < 1 ||
        (N1 && (!keys1Un || !desc1 || !node1 || !skip1 || !u_right1)) || (N2 && (!keys2Un || !desc2 || !node2 || !skip2 || !u_right2)))
        return CS_ERR_BAD_ARG;
    *nmatches = 0;
    for (int i = 0; i < N1; i++) matches12[i] = -1;
    if (N1 == 0 || N2 == 0) return CS_OK;
    for (int i = 0; i < N2; i++) if (keys2Un[i].octave < 0 || keys2Un[i].octave >= n_levels) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const NodeLists L(node2, N2);
    std::vector<int> n1c((size_t)N1), res((size_t)N1 + 1);
    for (int i = 0; i < N1; i++) n1c[i] = L.compact(node1[i]);
    cs_scratch sc(ctx); // (after the host arrays: it waits for the copies out of and into them before they go)
    cs_keypoint *d_k1 = nullptr, *d_k2 = nullptr; unsigned long long *d_d1 = nullptr, *d_d2 = nullptr; int *d_n1 = nullptr, *d_st = nullptr, *d_it = nullptr, *d_m = nullptr;
    uint8_t *d_s1 = nullptr, *d_s2 = nullptr; float *d_u1 = nullptr, *d_u2 = nullptr, *d_sc = nullptr, *d_sg = nullptr;
    CS_TRY(sc.alloc(ctx, &d_k1, (size_t)N1)); CS_TRY(sc.alloc(ctx, &d_k2, (size_t)N2)); CS_TRY(sc.alloc(ctx, &d_d1, (size_t)N1 * 4)); CS_TRY(sc.alloc(ctx, &d_d2, (size_t)N2 * 4));
    CS_TRY(sc.alloc(ctx, &d_n1, (size_t)N1)); CS_TRY(sc.alloc(ctx, &d_st, L.start.size())); CS_TRY(sc.alloc(ctx, &d_it, L.items.size())); CS_TRY(sc.alloc(ctx, &d_m, (size_t)N1 + 1));
    CS_TRY(sc.alloc(ctx, &d_s1, (size_t)N1)); CS_TRY(sc.alloc(ctx, &d_s2, (size_t)N2)); CS_TRY(sc.alloc(ctx, &d_u1, (size_t)N1)); CS_TRY(sc.alloc(ctx, &d_u2, (size_t)N2));
    CS_TRY(sc.alloc(ctx, &d_sc, (size_t)n_levels)); CS_TRY(sc.alloc(ctx, &d_sg, (size_t)n_levels));
    CS_TRY(cs_h2d(ctx, d_k1, keys1Un, (size_t)N1)); CS_TRY(cs_h2d(ctx, d_k2, keys2Un, (size_t)N2));
    CS_TRY(cs_h2d(ctx, (uint8_t *)d_d1, desc1, (size_t)N1 * 32)); CS_TRY(cs_h2d(ctx, (uint8_t *)d_d2, desc2, (size_t)N2 * 32));
    CS_TRY(cs_h2d(ctx, d_n1, n1c.data(), (size_t)N1)); CS_TRY(cs_h2d(ctx, d_st, L.start.data(), L.start.size())); CS_TRY(cs_h2d(ctx, d_it, L.items.data(), L.items.size()));
    CS_TRY(cs_h2d(ctx, d_s1, skip1, (size_t)N1)); CS_TRY(cs_h2d(ctx, d_s2, skip2, (size_t)N2)); CS_TRY(cs_h2d(ctx, d_u1, u_right1, (size_t)N1)); CS_TRY(cs_h2d(ctx, d_u2, u_right2, (size_t)N2));
    CS_TRY(cs_h2d(ctx, d_sc, scale_factors2, (size_t)n_levels)); CS_TRY(cs_h2d(ctx, d_sg, level_sigma2_2, (size_t)n_levels));
    TriP P; for (int k = 0; k < 9; k++) P.F12[k] = F12[k];
    P.ex = ex; P.ey = ey; P.only_stereo = only_stereo;
    CS_LAUNCH(ctx, "match_triangulation", match_triangulation, dim3((N1 + 3) / 4), dim3(256), 0, N1, d_k1, d_d1, d_n1, d_s1, d_u1, d_k2, d_d2, d_s2, d_u2, d_st, d_it, L.n_nodes, P,
              d_sc, d_sg, d_m);
    CS_LAUNCH(ctx, "match_orient_cut", match_orient_cut, dim3(1), dim3(1024), 0, N1, d_k1, d_k2, d_m, check_orientation, d_m + N1); // :801-830
    CS_TRY(cs_d2h(ctx, res.data(), d_m, (size_t)N1 + 1));
    CS_TRY(sc.drain());
    memcpy(matches12, res.data(), sizeof(int) * (size_t)N1);
    *nmatches = res[(size_t)N1];
    return CS_OK;
}

} // extern "C"

// ---- the searches that project map points through a Sim3 or a relocalisation pose: preamble, window enumeration and the loops, all on the device ----------------------------------
struct MapIn { int n; const float *world_pos, *normal, *min_distance, *max_distance; const uint8_t *skip, *mp_desc, *train_blocked; };
static MapP make_mapp(const float *R, const float *t, const float *Ow, const float *R2, const float *t2, float fx, float fy, float cx, float cy, float log_sf, float th, int n_levels,
                      float bf = 0.0f, float view_cos_limit = 0.0f) {
    MapP P{};
    P.bf = bf; P.view_cos_limit = view_cos_limit;
    for (int k = 0; k < 9; k++) { P.R[k] = R[k]; if (R2) P.R2[k] = R2[k]; }
    for (int k = 0; k < 3; k++) { P.t[k] = t[k]; if (Ow) P.Ow[k] = Ow[k]; if (t2) P.t2[k] = t2[k]; }
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy; P.log_sf = log_sf; P.th = th; P.n_levels = n_levels;
    return P;
}
// uploads the map points, runs the preamble into m's query arrays (points outside the scale table add to *d_nout) and enumerates the windows in m's frame; nothing waits
// (ur_q: the stereo form of the window enumeration, see mt_candidates)
template <int MODE> static int mt_map_queries(cs_ctx *ctx, cs_matcher *m, const MapIn &I, const MapP &P, const float *scale_factors, int *d_nout, const MapOut &O = MapOut{nullptr, nullptr, nullptr},
                                              const float *ur_q = nullptr, int ur_stride = 0) {
    const int n = I.n, N = m->F.N;
    CS_TRY(cs_h2d(ctx, m->d_wp, I.world_pos, (size_t)n * 3));
    if (MODE == PM_SIM3 || MODE == PM_FUSE || MODE == PM_FRUSTUM) CS_TRY(cs_h2d(ctx, m->d_nrm, I.normal, (size_t)n * 3));
    CS_TRY(cs_h2d(ctx, m->d_mind, I.min_distance, (size_t)n));
    CS_TRY(cs_h2d(ctx, m->d_maxd, I.max_distance, (size_t)n));
    CS_TRY(cs_h2d(ctx, m->d_valid, I.skip, (size_t)n));
    CS_TRY(cs_h2d(ctx, (uint8_t *)m->d_qdesc, I.mp_desc, (size_t)n * 32));
    CS_TRY(cs_h2d(ctx, m->d_sf, scale_factors, (size_t)P.n_levels));
    if (I.train_blocked) CS_TRY(cs_h2d(ctx, m->d_tb, I.train_blocked, (size_t)N));
    CS_LAUNCH(ctx, "match_project_map", match_project_map<MODE>, dim3((n + 255) / 256), dim3(256), 0, n, m->d_wp, m->d_nrm, m->d_mind, m->d_maxd, m->d_valid, P, m->d_sf, m->F, m->d_q, m->d_level, d_nout, O);
    return mt_candidates(ctx, m, n, true, ur_q, ur_stride);
}
static bool map_in_ok(const cs_matcher *m, const MapIn &I, bool need_normal) {
    return I.n >= 0 && I.n <= m->max_q && (I.n == 0 || (I.world_pos && I.min_distance && I.max_distance && I.skip && I.mp_desc && (!need_normal || I.normal)));
}
// the order-dependent searches: RV_CLAIM over the queries in order, train_match + nmatches + the count of rule (d), one wait
template <int MODE> static int mt_map_claim(cs_ctx *ctx, cs_matcher *m, const MapIn &I, const MapP &P, const float *scale_factors, const float *kf_angle, int accept_dist, int check_orientation,
                                            int *train_match, int *nmatches, int *n_level_outside) {
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const int N = m->F.N;
    *nmatches = 0;
    if (n_level_outside) *n_level_outside = 0;
    if (I.n == 0) { for (int i = 0; i < N; i++) train_match[i] = -1; return CS_OK; }
    CS_HIP(ctx, hipMemsetAsync(m->d_nout, 0, 2 * sizeof(int), ctx->stream));
    if (check_orientation) CS_TRY(cs_h2d(ctx, m->d_ang, kf_angle, (size_t)I.n));
    CS_TRY(mt_map_queries<MODE>(ctx, m, I, P, scale_factors, m->d_nout));
    ResolveP R{};
    R.cstart = m->d_cstart; R.ccount = m->d_ccount; R.cands = m->d_cands; R.n_steps = I.n; R.n_train = N; R.tkeys = m->d_keys; R.qangle = m->d_ang;
    R.tblocked = I.train_blocked ? m->d_tb : nullptr; R.check_orientation = check_orientation; R.train_match = m->d_tm; R.q_rec = m->d_qrec; R.nmatches = m->d_tm + N; R.accept_dist = accept_dist;
    CS_TRY(mt_resolve<RV_CLAIM>(ctx, R, 1, N));
    int *nout = m->h_nout;
    CS_TRY(cs_d2h(ctx, nout, m->d_nout, 2));
    CS_TRY(mt_finish(ctx, m, m->d_tm, N, train_match, nmatches));
    if (n_level_outside) *n_level_outside = nout[0];
    return CS_OK;
}

extern "C" {

int cs_match_by_projection_reloc(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *min_distance,
                                 const float *max_distance, const uint8_t *skip, const float *kf_angle, const uint8_t *mp_desc, const uint8_t *train_blocked, float fx, float fy, float cx,
                                 float cy, float log_scale_factor, const float *scale_factors, int n_levels, float th, int orb_dist, int check_orientation, int *train_match, int *nmatches,
                                 int *n_level_outside) {
    if (!ctx || !m) return CS_ERR_BAD_ARG;
    const MapIn I{n_mp, world_pos, nullptr, min_distance, max_distance, skip, mp_desc, train_blocked};
    if (!Rcw || !tcw || !Ow || !map_in_ok(m, I, false) || (n_mp && check_orientation && !kf_angle) || !scale_factors || n_levels < 1 || n_levels > 32 || !train_match || !nmatches) return CS_ERR_BAD_ARG;
    return mt_map_claim<PM_RELOC>(ctx, m, I, make_mapp(Rcw, tcw, Ow, nullptr, nullptr, fx, fy, cx, cy, log_scale_factor, th, n_levels), scale_factors, kf_angle, orb_dist, check_orientation,
                                  train_match, nmatches, n_level_outside);
}

int cs_match_by_projection_sim3(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal, const float *min_distance,
                                const float *max_distance, const uint8_t *skip, const uint8_t *mp_desc, const uint8_t *train_blocked, float fx, float fy, float cx, float cy, float log_scale_factor,
                                const float *scale_factors, int n_levels, float th, int *train_match, int *nmatches, int *n_level_outside) {
    if (!ctx || !m) return CS_ERR_BAD_ARG;
    const MapIn I{n_mp, world_pos, normal, min_distance, max_distance, skip, mp_desc, train_blocked};
    if (!Rcw || !tcw || !Ow || !map_in_ok(m, I, true) || !scale_factors || n_levels < 1 || n_levels > 32 || !train_match || !nmatches) return CS_ERR_BAD_ARG;
    return mt_map_claim<PM_SIM3>(ctx, m, I, make_mapp(Rcw, tcw, Ow, nullptr, nullptr, fx, fy, cx, cy, log_scale_factor, th, n_levels), scale_factors, nullptr, TH_LOW, 0, train_match, nmatches,
                                 n_level_outside);
}

int cs_match_fuse_sim3(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal, const float *min_distance,
                       const float *max_distance, const uint8_t *skip, const uint8_t *mp_desc, const uint8_t *train_blocked, float fx, float fy, float cx, float cy, float log_scale_factor,
                       const float *scale_factors, int n_levels, float th, int *best_idx, int *best_dist, int *n_fused, int *n_level_outside) {
    if (!ctx || !m) return CS_ERR_BAD_ARG;
    const MapIn I{n_mp, world_pos, normal, min_distance, max_distance, skip, mp_desc, train_blocked};
    if (!Rcw || !tcw || !Ow || !map_in_ok(m, I, true) || !scale_factors || n_levels < 1 || n_levels > 32 || !best_idx || !best_dist || !n_fused) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    *n_fused = 0;
    if (n_level_outside) *n_level_outside = 0;
    if (n_mp == 0) return CS_OK;
    CS_HIP(ctx, hipMemsetAsync(m->d_nout, 0, 2 * sizeof(int), ctx->stream));
    CS_TRY(mt_map_queries<PM_SIM3>(ctx, m, I, make_mapp(Rcw, tcw, Ow, nullptr, nullptr, fx, fy, cx, cy, log_scale_factor, th, n_levels), scale_factors, m->d_nout));
    CS_LAUNCH(ctx, "match_map_best", match_map_best, dim3((n_mp + 255) / 256), dim3(256), 0, n_mp, m->d_cstart, m->d_ccount, m->d_cands, train_blocked ? m->d_tb : (const uint8_t *)nullptr, -1, m->d_qm, m->d_qrec);
    int *nout = m->h_nout;
    CS_TRY(cs_d2h(ctx, nout, m->d_nout, 2));
    CS_TRY(cs_d2h(ctx, best_idx, m->d_qm, (size_t)n_mp));
    CS_TRY(cs_d2h(ctx, best_dist, m->d_qrec, (size_t)n_mp));
    CS_TRY(mt_cursor(ctx, m->d_cursor, m->max_cand, &m->last_c));
    int nf = 0;
    for (int i = 0; i < n_mp; i++) if (best_dist[i] <= TH_LOW) nf++; // :1121
    *n_fused = nf;
    if (n_level_outside) *n_level_outside = nout[0];
    return CS_OK;
}

} // extern "C"
// cs_match_local_map_frustum and its stereo form (stereo: the uR the preamble leaves in MapOut.proj is tested against the attached mvuRight, :104-109)
static int mt_local_map_frustum(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal, const float *min_distance,
                                const float *max_distance, const uint8_t *skip, const uint8_t *blocks, const uint8_t *mp_desc, const uint8_t *train_blocked, float fx, float fy, float cx, float cy,
                                float bf, float log_scale_factor, const float *scale_factors, int n_levels, float viewing_cos_limit, float th, float nnratio, int *train_match, int *nmatches,
                                int *n_to_match, int *n_level_outside, uint8_t *in_view, float *proj, int *pred_level, float *view_cos, bool stereo) {
    if (!ctx || !m) return CS_ERR_BAD_ARG;
    const MapIn I{n_mp, world_pos, normal, min_distance, max_distance, skip, mp_desc, train_blocked};
    if (!Rcw || !tcw || !Ow || !map_in_ok(m, I, true) || (n_mp && (!blocks || !in_view)) || !scale_factors || n_levels < 1 || n_levels > 32 || !train_match || !nmatches || !n_to_match)
        return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const int N = m->F.N;
    *nmatches = 0; *n_to_match = 0;
    if (n_level_outside) *n_level_outside = 0;
    if (n_mp == 0) { for (int i = 0; i < N; i++) train_match[i] = -1; return CS_OK; }
    CS_HIP(ctx, hipMemsetAsync(m->d_nout, 0, 2 * sizeof(int), ctx->stream));
    CS_TRY(cs_h2d(ctx, m->d_blocks, blocks, (size_t)n_mp));
    // Tracking::SearchLocalPoints :2699-2715 (isInFrustum per point) and the window of ORBmatcher.cc:72-78, written where match_candidates reads it
    CS_TRY(mt_map_queries<PM_FRUSTUM>(ctx, m, I, make_mapp(Rcw, tcw, Ow, nullptr, nullptr, fx, fy, cx, cy, log_scale_factor, th, n_levels, bf, viewing_cos_limit), scale_factors, m->d_nout,
                                      MapOut{m->d_inview, m->d_proj, m->d_ang}, stereo ? m->d_proj + 2 : nullptr, 3));
    // (:2717: without a point in view the reference does not call the search; here no query is valid then and the search leaves train_match at -1 -- the same result without a
    //  second wait for the count)
    ResolveP P{}; // :86-140, as cs_match_local_map
    P.cstart = m->d_cstart; P.ccount = m->d_ccount; P.cands = m->d_cands; P.n_steps = n_mp; P.n_train = N; P.tkeys = m->d_keys; P.blocks = m->d_blocks;
    P.tblocked = train_blocked ? m->d_tb : nullptr; P.nnratio = nnratio; P.check_orientation = 0; P.train_match = m->d_tm; P.q_rec = m->d_qrec; P.nmatches = m->d_tm + N;
    CS_TRY(mt_resolve<RV_LOCAL>(ctx, P, 1, N));
    int *nout = m->h_nout;
    CS_TRY(cs_d2h(ctx, nout, m->d_nout, 2));
    CS_TRY(cs_d2h(ctx, in_view, m->d_inview, (size_t)n_mp));
    if (proj) CS_TRY(cs_d2h(ctx, proj, m->d_proj, (size_t)n_mp * 3));
    if (pred_level) CS_TRY(cs_d2h(ctx, pred_level, m->d_level, (size_t)n_mp));
    if (view_cos) CS_TRY(cs_d2h(ctx, view_cos, m->d_ang, (size_t)n_mp));
    CS_TRY(mt_finish(ctx, m, m->d_tm, N, train_match, nmatches));
    *n_to_match = nout[1];
    if (n_level_outside) *n_level_outside = nout[0];
    return CS_OK;
}
extern "C" {
int cs_match_local_map_frustum(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal, const float *min_distance,
                               const float *max_distance, const uint8_t *skip, const uint8_t *blocks, const uint8_t *mp_desc, const uint8_t *train_blocked, float fx, float fy, float cx, float cy,
                               float bf, float log_scale_factor, const float *scale_factors, int n_levels, float viewing_cos_limit, float th, float nnratio, int *train_match, int *nmatches,
                               int *n_to_match, int *n_level_outside, uint8_t *in_view, float *proj, int *pred_level, float *view_cos) {
    return mt_local_map_frustum(ctx, m, Rcw, tcw, Ow, n_mp, world_pos, normal, min_distance, max_distance, skip, blocks, mp_desc, train_blocked, fx, fy, cx, cy, bf, log_scale_factor, scale_factors,
                                n_levels, viewing_cos_limit, th, nnratio, train_match, nmatches, n_to_match, n_level_outside, in_view, proj, pred_level, view_cos, false);
}

int cs_match_fuse_map(cs_ctx *ctx, cs_matcher *m, const float *u_right, const float *inv_level_sigma2, int n_levels, const uint8_t *keys_static, const float *Rcw, const float *tcw, const float *Ow,
                      int n_mp, const float *world_pos, const float *normal, const float *min_distance, const float *max_distance, const uint8_t *skip, const uint8_t *mp_desc, float fx, float fy,
                      float cx, float cy, float bf, float log_scale_factor, const float *scale_factors, float th, int *best_idx, int *best_dist, int *n_fused, int *n_level_outside) {
    if (!ctx || !m) return CS_ERR_BAD_ARG;
    const MapIn I{n_mp, world_pos, normal, min_distance, max_distance, skip, mp_desc, nullptr};
    if (!Rcw || !tcw || !Ow || !map_in_ok(m, I, true) || !u_right || !inv_level_sigma2 || !scale_factors || n_levels < 1 || n_levels > 32 || !best_idx || !best_dist || !n_fused) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    *n_fused = 0;
    if (n_level_outside) *n_level_outside = 0;
    if (n_mp == 0) return CS_OK;
    const int N = m->F.N;
    CS_HIP(ctx, hipMemsetAsync(m->d_nout, 0, 2 * sizeof(int), ctx->stream));
    CS_TRY(cs_h2d(ctx, m->d_inv, inv_level_sigma2, (size_t)n_levels));
    CS_TRY(cs_h2d(ctx, m->d_ur, u_right, (size_t)N));
    if (keys_static) CS_TRY(cs_h2d(ctx, m->d_tb, keys_static, (size_t)N));
    CS_TRY(mt_map_queries<PM_FUSE>(ctx, m, I, make_mapp(Rcw, tcw, Ow, nullptr, nullptr, fx, fy, cx, cy, log_scale_factor, th, n_levels, bf), scale_factors, m->d_nout,
                                   MapOut{m->d_inview, m->d_uv, m->d_qur})); // :871-922
    CS_LAUNCH(ctx, "match_fuse_best", match_fuse_best, dim3((n_mp + 255) / 256), dim3(256), 0, n_mp, m->d_cstart, m->d_ccount, m->d_cands, m->d_keys, m->d_ur, m->d_inv, n_levels,
              keys_static ? m->d_tb : (const uint8_t *)nullptr, m->d_uv, m->d_qur, m->d_level, m->d_inview, m->d_qm, m->d_qrec, reinterpret_cast<int *>(m->d_cursor + 1)); // :934-981
    int *nout = m->h_nout;
    CS_TRY(cs_d2h(ctx, nout, m->d_nout, 2));
    CS_TRY(cs_d2h(ctx, best_idx, m->d_qm, (size_t)n_mp));
    CS_TRY(cs_d2h(ctx, best_dist, m->d_qrec, (size_t)n_mp));
    CS_TRY(mt_cursor(ctx, m->d_cursor, m->max_cand, &m->last_c)); // (BAD_ARG: a candidate's level outside the sigma table)
    int nf = 0;
    for (int i = 0; i < n_mp; i++) if (best_dist[i] <= TH_LOW) nf++;
    *n_fused = nf;
    if (n_level_outside) *n_level_outside = nout[0];
    return CS_OK;
}

int cs_match_by_sim3(cs_ctx *ctx, cs_matcher *m1, cs_matcher *m2, const float *R1w, const float *t1w, const float *R2w, const float *t2w, const float *sR12, const float *t12, const float *sR21,
                     const float *t21, int n1, const float *world_pos1, const float *min_distance1, const float *max_distance1, const uint8_t *skip1, const uint8_t *mp_desc1,
                     const uint8_t *train_blocked1, int n2, const float *world_pos2, const float *min_distance2, const float *max_distance2, const uint8_t *skip2, const uint8_t *mp_desc2,
                     const uint8_t *train_blocked2, float fx, float fy, float cx, float cy, float log_scale_factor, const float *scale_factors, int n_levels, float th, int *matches12, int *n_found,
                     int *n_level_outside) {
    if (!ctx || !m1 || !m2 || m1 == m2) return CS_ERR_BAD_ARG;
    // the points of KF1 are searched in KF2 (m2's frame and query arrays) and the other way round
    const MapIn I1{n1, world_pos1, nullptr, min_distance1, max_distance1, skip1, mp_desc1, train_blocked2}, I2{n2, world_pos2, nullptr, min_distance2, max_distance2, skip2, mp_desc2, train_blocked1};
    if (!R1w || !t1w || !R2w || !t2w || !sR12 || !t12 || !sR21 || !t21 || !map_in_ok(m2, I1, false) || !map_in_ok(m1, I2, false) || !scale_factors || n_levels < 1 || n_levels > 32 ||
        (n1 && !matches12) || !n_found)
        return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    *n_found = 0;
    if (n_level_outside) *n_level_outside = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0 || n2 == 0) return CS_OK; // (no agreement without both directions)
    CS_HIP(ctx, hipMemsetAsync(m2->d_nout, 0, 2 * sizeof(int), ctx->stream));
    CS_TRY(mt_map_queries<PM_PAIR>(ctx, m2, I1, make_mapp(R1w, t1w, nullptr, sR21, t21, fx, fy, cx, cy, log_scale_factor, th, n_levels), scale_factors, m2->d_nout)); // :1187-1267
    CS_LAUNCH(ctx, "match_map_best", match_map_best, dim3((n1 + 255) / 256), dim3(256), 0, n1, m2->d_cstart, m2->d_ccount, m2->d_cands, train_blocked2 ? m2->d_tb : (const uint8_t *)nullptr, TH_HIGH, m2->d_qm,
              (int *)nullptr);
    CS_TRY(mt_map_queries<PM_PAIR>(ctx, m1, I2, make_mapp(R2w, t2w, nullptr, sR12, t12, fx, fy, cx, cy, log_scale_factor, th, n_levels), scale_factors, m2->d_nout)); // :1270-1350
    CS_LAUNCH(ctx, "match_map_best", match_map_best, dim3((n2 + 255) / 256), dim3(256), 0, n2, m1->d_cstart, m1->d_ccount, m1->d_cands, train_blocked1 ? m1->d_tb : (const uint8_t *)nullptr, TH_HIGH, m1->d_qm,
              (int *)nullptr);
    CS_LAUNCH(ctx, "match_sim3_agree", match_sim3_agree, dim3((n1 + 255) / 256), dim3(256), 0, n1, m2->d_qm, n2, m1->d_qm, m2->d_qrec, m2->d_nout + 1); // :1353-1368
    int *nout = m2->h_nout;
    CS_TRY(cs_d2h(ctx, nout, m2->d_nout, 2));
    CS_TRY(cs_d2h(ctx, matches12, m2->d_qrec, (size_t)n1));
    const int r2 = mt_cursor(ctx, m2->d_cursor, m2->max_cand, &m2->last_c), r1 = mt_cursor(ctx, m1->d_cursor, m1->max_cand, &m1->last_c); // (the first one waits; both arenas are checked)
    if (r2 != CS_OK || r1 != CS_OK) { for (int i = 0; i < n1; i++) matches12[i] = -1; return r2 != CS_OK ? r2 : r1; }
    *n_found = nout[1];
    if (n_level_outside) *n_level_outside = nout[0];
    return CS_OK;
}

} // extern "C"

// Both SearchByBoW overloads: the K side's features are visited by (vocabulary node ascending, index ascending) -- the reference's std::map / vector order -- and each one's
// candidates are the F side's features of its node in ascending index.  The distances (one wave per K feature) and the greedy claims (match_resolve) run on the device; the
// host only lays out the node lists.  V = RV_BOW: out = matchesF[NF] (K feature per F feature); RV_BOWKF: out = matches12[NK] (F feature per K feature).
template <int V> static int bow_search(cs_ctx *ctx, const cs_keypoint *keysK, const uint8_t *descK, int NK, const int *nodeK, const uint8_t *skipK, const cs_keypoint *keysF, const uint8_t *descF, int NF,
                                       const int *nodeF, const uint8_t *skipF, float nnratio, int check_orientation, int *out, int *nmatches) {
    CS_HIP(ctx, hipSetDevice(ctx->device));
    if (NF >= (1 << 24)) return CS_ERR_CAPACITY;
    const NodeLists L(nodeF, NF);
    std::vector<int> nkc((size_t)NK, -1), cnt((size_t)NK, 0);
    std::vector<long> off((size_t)NK + 1, 0);
    for (int i = 0; i < NK; i++) { nkc[i] = skipK[i] ? -1 : L.compact(nodeK[i]); cnt[i] = nkc[i] >= 0 ? L.start[nkc[i] + 1] - L.start[nkc[i]] : 0; off[i + 1] = off[i] + cnt[i]; }
    const long total = off[NK];
    // the reference's order: nodes ascending (std::map), K features ascending inside a node
    std::vector<std::pair<int, int>> order;
    for (int i = 0; i < NK; i++) if (nkc[i] >= 0) order.push_back(std::make_pair(nodeK[i], i));
    std::sort(order.begin(), order.end());
    const int n_steps = (int)order.size();
    const int n_out = V == RV_BOW ? NF : NK;
    *nmatches = 0;
    if (n_steps == 0 || total == 0) return CS_OK; // (out is pre-filled with -1 by the callers)
    std::vector<int> qlist((size_t)n_steps);
    for (int s = 0; s < n_steps; s++) qlist[s] = order[s].second;
    std::vector<int> res((size_t)n_out + 1, -1);
    cs_scratch sc(ctx); // (after the host arrays: it waits for the copies out of and into them before they go)
    cs_keypoint *d_kk = nullptr, *d_kf = nullptr; unsigned long long *d_dk = nullptr, *d_df = nullptr; int *d_nk = nullptr, *d_st = nullptr, *d_it = nullptr, *d_cnt = nullptr, *d_ql = nullptr, *d_rec = nullptr, *d_out = nullptr;
    long *d_off = nullptr; int2 *d_ca = nullptr; uint8_t *d_sf = nullptr;
    CS_TRY(sc.alloc(ctx, &d_dk, (size_t)NK * 4)); CS_TRY(sc.alloc(ctx, &d_df, (size_t)NF * 4)); CS_TRY(sc.alloc(ctx, &d_nk, (size_t)NK)); CS_TRY(sc.alloc(ctx, &d_st, L.start.size())); CS_TRY(sc.alloc(ctx, &d_it, L.items.size()));
    CS_TRY(sc.alloc(ctx, &d_off, off.size())); CS_TRY(sc.alloc(ctx, &d_ca, (size_t)total)); CS_TRY(sc.alloc(ctx, &d_cnt, (size_t)NK)); CS_TRY(sc.alloc(ctx, &d_ql, (size_t)n_steps)); CS_TRY(sc.alloc(ctx, &d_rec, (size_t)NK));
    CS_TRY(sc.alloc(ctx, &d_out, (size_t)n_out + 1)); CS_TRY(sc.alloc(ctx, &d_kk, (size_t)NK)); CS_TRY(sc.alloc(ctx, &d_kf, (size_t)NF)); if (skipF) CS_TRY(sc.alloc(ctx, &d_sf, (size_t)NF));
    CS_TRY(cs_h2d(ctx, (uint8_t *)d_dk, descK, (size_t)NK * 32)); CS_TRY(cs_h2d(ctx, (uint8_t *)d_df, descF, (size_t)NF * 32)); CS_TRY(cs_h2d(ctx, d_nk, nkc.data(), (size_t)NK));
    CS_TRY(cs_h2d(ctx, d_st, L.start.data(), L.start.size())); CS_TRY(cs_h2d(ctx, d_it, L.items.data(), L.items.size())); CS_TRY(cs_h2d(ctx, d_off, off.data(), off.size()));
    CS_TRY(cs_h2d(ctx, d_cnt, cnt.data(), (size_t)NK)); CS_TRY(cs_h2d(ctx, d_ql, qlist.data(), (size_t)n_steps)); CS_TRY(cs_h2d(ctx, d_kk, keysK, (size_t)NK)); CS_TRY(cs_h2d(ctx, d_kf, keysF, (size_t)NF));
    if (skipF) CS_TRY(cs_h2d(ctx, d_sf, skipF, (size_t)NF));
    if (V == RV_BOWKF) CS_HIP(ctx, hipMemsetAsync(d_out, 0xff, sizeof(int) * (size_t)NK, ctx->stream)); // K features outside the visiting order have no match
    CS_LAUNCH(ctx, "match_bow_dists", match_bow_dists, dim3((NK + 3) / 4), dim3(256), 0, NK, d_dk, d_nk, d_df, d_st, d_it, d_off, d_ca);
    ResolveP P{};
    P.cstart = d_off; P.ccount = d_cnt; P.cands = d_ca; P.qlist = d_ql; P.n_steps = n_steps; P.n_train = NF; P.tkeys = d_kf; P.qkeys = d_kk; P.tblocked = d_sf; P.nnratio = nnratio;
    P.check_orientation = check_orientation; P.train_match = d_out; P.q_match = d_out; P.q_rec = d_rec; P.nmatches = d_out + n_out;
    CS_TRY(mt_resolve<V>(ctx, P, 1, NF));
    CS_TRY(cs_d2h(ctx, res.data(), d_out, (size_t)n_out + 1));
    CS_TRY(sc.drain());
    memcpy(out, res.data(), sizeof(int) * (size_t)n_out);
    *nmatches = res[(size_t)n_out];
    return CS_OK;
}

extern "C" {

int cs_match_by_bow(cs_ctx *ctx, const cs_keypoint *keysKF, const uint8_t *descKF, int NK, const int *nodeKF, const uint8_t *skipKF, const cs_keypoint *keysF,
                    const uint8_t *descF, int NF, const int *nodeF, const uint8_t *skipF, float nnratio, int check_orientation, int *matchesF, int *nmatches) {
    if (!ctx || NK < 0 || NF < 0 || !matchesF || !nmatches || (NK && (!keysKF || !descKF || !nodeKF || !skipKF)) || (NF && (!keysF || !descF || !nodeF))) return CS_ERR_BAD_ARG;
    *nmatches = 0;
    for (int i = 0; i < NF; i++) matchesF[i] = -1;
    if (NK == 0 || NF == 0) return CS_OK;
    return bow_search<RV_BOW>(ctx, keysKF, descKF, NK, nodeKF, skipKF, keysF, descF, NF, nodeF, skipF, nnratio, check_orientation, matchesF, nmatches); // :171-310
}

int cs_match_by_bow_kf(cs_ctx *ctx, const cs_keypoint *keys1, const uint8_t *desc1, int N1, const int *node1, const uint8_t *skip1, const cs_keypoint *keys2,
                       const uint8_t *desc2, int N2, const int *node2, const uint8_t *skip2, float nnratio, int check_orientation, int *matches12, int *nmatches) {
    if (!ctx || N1 < 0 || N2 < 0 || !nmatches || (N1 && (!keys1 || !desc1 || !node1 || !skip1 || !matches12)) || (N2 && (!keys2 || !desc2 || !node2 || !skip2))) return CS_ERR_BAD_ARG;
    *nmatches = 0;
    for (int i = 0; i < N1; i++) matches12[i] = -1;
    if (N1 == 0 || N2 == 0) return CS_OK;
    return bow_search<RV_BOWKF>(ctx, keys1, desc1, N1, node1, skip1, keys2, desc2, N2, node2, skip2, nnratio, check_orientation, matches12, nmatches); // :544-677 (vbMatched2 = a claimed key point; skip2 = no usable map point)
}

int cs_hamming_knn2(cs_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int *best_idx, int *best_dist, int *second_dist) {
    if (!ctx || !q || !t || nq < 0 || nt < 0 || !best_idx || !best_dist || !second_dist) return CS_ERR_BAD_ARG;
    if (nq == 0) return CS_OK;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    unsigned long long *dq = nullptr, *dt = nullptr; int *dres = nullptr;
    CS_TRY(sc.alloc(ctx, &dq, (size_t)nq * 4)); CS_TRY(sc.alloc(ctx, &dt, (size_t)std::max(nt, 1) * 4)); CS_TRY(sc.alloc(ctx, &dres, (size_t)nq * 3));
    CS_TRY(cs_h2d(ctx, (uint8_t *)dq, q, (size_t)nq * 32));
    CS_TRY(cs_h2d(ctx, (uint8_t *)dt, t, (size_t)nt * 32));
    CS_LAUNCH(ctx, "match_knn2", match_knn2, dim3((nq + 255) / 256), dim3(256), 0, dq, nq, dt, nt, dres, dres + nq, dres + 2 * nq);
    CS_TRY(cs_d2h(ctx, best_idx, dres, (size_t)nq));
    CS_TRY(cs_d2h(ctx, best_dist, dres + nq, (size_t)nq));
    CS_TRY(cs_d2h(ctx, second_dist, dres + 2 * nq, (size_t)nq));
    return sc.drain();
}

} // extern "C"

// ---- the stereo branches of both SearchByProjection overloads (include/cubeslam_hip/stereo_search.h) ------------------------------------------------------------------
#include "../../include/cubeslam_hip/stereo_search.h"
extern "C" {

int cs_stereo_search_version(void) { return CS_STEREO_SEARCH_VERSION; }

int cs_matcher_set_u_right(cs_ctx *ctx, cs_matcher *m, const float *u_right, int n, int on_device) {
    if (!ctx || !m || !u_right || !(m->F.wInv > 0.0f) || n != m->F.N) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    if (n > 0) CS_HIP(ctx, hipMemcpyAsync(m->d_uright, u_right, sizeof(float) * (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    m->has_uright = true;
    return CS_OK;
}

int cs_match_by_projection_frame_stereo(cs_ctx *ctx, cs_matcher *m, int n_last, const float *world_pos, const uint8_t *valid, const uint8_t *blocks, const uint8_t *mp_desc, const int *last_octave,
                                        const float *last_angle, const float *Tcw, float fx, float fy, float cx, float cy, const float *scale_factors, int n_levels, float th, int check_orientation,
                                        const uint8_t *train_blocked, int *train_match, int *nmatches, const float *Tlw, float bf, float mb, int mono, int *direction) {
    if (!ctx || !m || !Tcw || (!mono && (!Tlw || !m->has_uright))) return CS_ERR_BAD_ARG;
    const int dir = stereo_search_direction(Tcw, Tlw, mb, mono);
    const int r = mt_by_projection_frame(ctx, m, n_last, world_pos, valid, blocks, mp_desc, last_octave, last_angle, Tcw, fx, fy, cx, cy, scale_factors, n_levels, th, check_orientation, train_blocked,
                                         train_match, nmatches, !mono, dir, bf);
    if (r == CS_OK && direction) *direction = dir;
    return r;
}

int cs_match_by_projection_stream_stereo(cs_ctx *ctx, cs_match_stream *m, const cs_orb *orb, int f0, int n_pairs, const float *K4, const float *dist5, float minX, float maxX, float minY, float maxY,
                                         int n_queries, int n_train, const float *world_pos, const uint8_t *valid, const uint8_t *blocks, const uint8_t *mp_desc, const float *Tcw, float fx, float fy,
                                         float cx, float cy, const float *scale_factors, int n_levels, float th, int check_orientation, int *train_match, int *nmatches, const float *Tlw,
                                         const float *u_right, int u_right_on_device, float bf, float mb, int mono, int *direction) {
    if (!ctx || !m || n_pairs < 1 || !Tcw || (!mono && (!Tlw || (n_train > 0 && !u_right)))) return CS_ERR_BAD_ARG;
    std::vector<int> dir((size_t)n_pairs);
    for (int p = 0; p < n_pairs; p++) dir[p] = stereo_search_direction(Tcw + 12 * p, mono ? nullptr : Tlw + 12 * p, mb, mono);
    const StreamStereo SQ{dir.data(), bf, u_right, u_right_on_device};
    const int r = mt_by_projection_stream(ctx, m, orb, f0, n_pairs, K4, dist5, minX, maxX, minY, maxY, n_queries, n_train, world_pos, valid, blocks, mp_desc, Tcw, fx, fy, cx, cy, scale_factors, n_levels, th,
                                          check_orientation, train_match, nmatches, mono ? nullptr : &SQ);
    if (r == CS_OK && direction) for (int p = 0; p < n_pairs; p++) direction[p] = dir[p];
    return r;
}

int cs_match_local_map_stereo(cs_ctx *ctx, cs_matcher *m, int n_mp, const float *proj_xy, const float *view_cos, const int *pred_level, const uint8_t *in_view, const uint8_t *blocks,
                              const uint8_t *mp_desc, const float *scale_factors, int n_levels, float th, float nnratio, const uint8_t *train_blocked, int *train_match, int *nmatches,
                              const float *proj_xr) {
    if (!ctx || !m || !proj_xr || !m->has_uright) return CS_ERR_BAD_ARG;
    return mt_local_map(ctx, m, n_mp, proj_xy, view_cos, pred_level, in_view, blocks, mp_desc, scale_factors, n_levels, th, nnratio, train_blocked, train_match, nmatches, proj_xr);
}

int cs_match_local_map_frustum_stereo(cs_ctx *ctx, cs_matcher *m, const float *Rcw, const float *tcw, const float *Ow, int n_mp, const float *world_pos, const float *normal, const float *min_distance,
                                      const float *max_distance, const uint8_t *skip, const uint8_t *blocks, const uint8_t *mp_desc, const uint8_t *train_blocked, float fx, float fy, float cx,
                                      float cy, float bf, float log_scale_factor, const float *scale_factors, int n_levels, float viewing_cos_limit, float th, float nnratio, int *train_match,
                                      int *nmatches, int *n_to_match, int *n_level_outside, uint8_t *in_view, float *proj, int *pred_level, float *view_cos) {
    if (!ctx || !m || !m->has_uright) return CS_ERR_BAD_ARG;
    return mt_local_map_frustum(ctx, m, Rcw, tcw, Ow, n_mp, world_pos, normal, min_distance, max_distance, skip, blocks, mp_desc, train_blocked, fx, fy, cx, cy, bf, log_scale_factor, scale_factors,
                                n_levels, viewing_cos_limit, th, nnratio, train_match, nmatches, n_to_match, n_level_outside, in_view, proj, pred_level, view_cos, true);
}

} // extern "C"
