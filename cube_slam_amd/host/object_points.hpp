// object_points.hpp -- point coordinates out of cuboids with the reference's names, over the C-ABI extension (include/cubeslam_hip/object_points.h) and plain arrays:
//   cubeslam::ObjectPoints::TriangulateDynamicPoints    the triangulation block of Tracking::CreateNewKeyFrame (orb_object_slam/src/Tracking.cc:2144-2244) for a batch of key-frame pairs
//   cubeslam::ObjectPoints::MonoObjDepthInitialization  Tracking.cc:876-898
//   cubeslam::ObjectPoints::CreateNewKeyFrameObjectDepth       Tracking.cc:2339-2424
//   cubeslam::ObjectPoints::CreateNewMapPointsObjectDepth      LocalMapping.cc:574-652
// A null Context pointer takes the library's host form.  The caller keeps `new MapPoint`, SetupSimpleMapPoints, the flags is_dynamic and is_triangulated, srand / rand (its
// values go in as `draws`) and resolving the last key frame's cuboid pose.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip/object_points.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context

namespace cubeslam {

struct DynamicPairs { // the inputs of cs_triangulate_dynamic_points, one behind the other; first / cub_first_* start with 0
    std::vector<int> first{0}, cub_first_last{0}, cub_first_now{0};
    std::vector<float> Tcw_last, Tcw_now, K4;         // 12, 12, 4 floats per pair
    std::vector<double> cub_pose_last, cub_pose_now;  // 7 doubles per cuboid: t, qx qy qz qw
    std::vector<int> tracklet_last, tracklet_now;     // both empty: use_truth_trackid is false
    std::vector<float> kp1, kp2, world_pos;           // 2, 2, 3 floats per point
    std::vector<int> obj_last, obj_now, idx_last;
    int n_pairs() const { return (int)first.size() - 1; }
};
struct DynamicPoints {
    std::vector<uint8_t> status; // CS_DYN_*
    std::vector<float> x3D, PosToObj;
    std::vector<double> dpoints; // PosToObj as cs_ba_dyn_problem reads it
};

struct ObjectDepthFrames { // the inputs of cs_object_depth_points
    std::vector<int> first{0}, cub_first{0}, draw_first{0};
    std::vector<cs_keypoint> keys;            // mvKeysUn in the first-frame mode, mvKeys otherwise
    std::vector<uint8_t> has_map_point;       // pMP != NULL
    std::vector<int> keypoint_associate_objectID, draws;
    std::vector<float> cuboid_depth, K4, bounds, Twc; // 4, 4 and 12 floats per frame
    int n_frames() const { return (int)first.size() - 1; }
};
struct ObjectDepthPoints {
    std::vector<int> n_candidates, raw_depth_pts, max_initialize_pts, cand_first, candidates, shuffled, new_first, new_idx;
    std::vector<float> new_x3D;
};

struct ObjectPoints {
    static void check(const Context *c, int r, const char *what) {
        if (r != CS_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(r) + ")" + (c ? std::string(": ") + cs_last_error(c->ctx) : std::string()));
    }
    template <class T> static const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

    static DynamicPoints TriangulateDynamicPoints(const Context *c, const DynamicPairs &p) {
        const size_t n = p.first.empty() ? 0 : (size_t)p.first.back();
        if (p.obj_last.size() != n || p.obj_now.size() != n || p.idx_last.size() != n || p.kp1.size() != 2 * n || p.kp2.size() != 2 * n || p.world_pos.size() != 3 * n)
            throw std::invalid_argument("DynamicPairs: arrays disagree in length");
        DynamicPoints o;
        o.status.assign(n, 0); o.x3D.assign(3 * n, 0.f); o.PosToObj.assign(3 * n, 0.f); o.dpoints.assign(3 * n, 0.0);
        check(c, cs_triangulate_dynamic_points(c ? c->ctx : nullptr, p.n_pairs(), p.first.data(), ptr(p.Tcw_last), ptr(p.Tcw_now), ptr(p.K4), p.cub_first_last.data(), ptr(p.cub_pose_last),
                                               p.cub_first_now.data(), ptr(p.cub_pose_now), ptr(p.tracklet_last), ptr(p.tracklet_now), ptr(p.kp1), ptr(p.kp2), ptr(p.obj_last),
                                               ptr(p.obj_now), ptr(p.idx_last), ptr(p.world_pos), o.status.data(), o.x3D.data(), o.PosToObj.data(), o.dpoints.data()),
              "cs_triangulate_dynamic_points");
        return o;
    }

    static ObjectDepthPoints ObjectDepth(const Context *c, int mode, const ObjectDepthFrames &f) {
        const size_t F = (size_t)f.n_frames(), n = f.first.empty() ? 0 : (size_t)f.first.back();
        if (f.keys.size() != n || f.keypoint_associate_objectID.size() != n || (mode != CS_OBJECT_DEPTH_FIRST_FRAME && f.has_map_point.size() != n))
            throw std::invalid_argument("ObjectDepthFrames: arrays disagree in length");
        ObjectDepthPoints o;
        o.n_candidates.assign(F, 0); o.raw_depth_pts.assign(F, 0); o.max_initialize_pts.assign(F, 0); o.cand_first.assign(F + 1, 0); o.new_first.assign(F + 1, 0);
        o.candidates.assign(n, 0); o.shuffled.assign(n, 0); o.new_idx.assign(n, 0); o.new_x3D.assign(3 * n, 0.f);
        check(c, cs_object_depth_points(c ? c->ctx : nullptr, mode, (int)F, f.first.data(), ptr(f.keys), ptr(f.has_map_point), ptr(f.keypoint_associate_objectID), f.cub_first.data(),
                                        ptr(f.cuboid_depth), ptr(f.K4), ptr(f.bounds), ptr(f.Twc), f.draw_first.data(), ptr(f.draws), o.n_candidates.data(), o.raw_depth_pts.data(),
                                        o.max_initialize_pts.data(), o.cand_first.data(), o.candidates.data(), o.shuffled.data(), o.new_first.data(), o.new_idx.data(),
                                        o.new_x3D.data()),
              "cs_object_depth_points");
        o.candidates.resize((size_t)o.cand_first[F]); o.shuffled.resize((size_t)o.cand_first[F]);
        o.new_idx.resize((size_t)o.new_first[F]); o.new_x3D.resize(3 * (size_t)o.new_first[F]);
        return o;
    }
    static ObjectDepthPoints MonoObjDepthInitialization(const Context *c, const ObjectDepthFrames &f) { return ObjectDepth(c, CS_OBJECT_DEPTH_FIRST_FRAME, f); }
    static ObjectDepthPoints CreateNewKeyFrameObjectDepth(const Context *c, const ObjectDepthFrames &f) { return ObjectDepth(c, CS_OBJECT_DEPTH_TRACKING, f); }
    static ObjectDepthPoints CreateNewMapPointsObjectDepth(const Context *c, const ObjectDepthFrames &f) { return ObjectDepth(c, CS_OBJECT_DEPTH_LOCAL_MAPPING, f); }
};

} // namespace cubeslam
