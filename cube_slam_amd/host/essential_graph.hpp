// essential_graph.hpp -- dependency-free C++ host-side mirror of ORB_SLAM2::Optimizer::OptimizeEssentialGraph (orb_object_slam/include/Optimizer.h,
// src/Optimizer.cc:2575-2836) over the C-ABI (cs_essential_graph_*, cs_sim3_correct_points): the graph-level rules of :2603-2776 over a flattened map, then the
// optimisation and the point correction on the device.  The Python twin is cube_slam_amd.optimizer.build_essential_graph / OptimizeEssentialGraph; both give the same
// arrays.  The caller keeps SetPose, SetWorldPos, UpdateNormalAndDepth and the mnCorrectedByKF choice of nIDr (:2813-2822).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "detect_3d_cuboid.hpp" // cubeslam::Context

namespace cubeslam {

struct FlatKeyFrame {
    long mnId = 0;
    bool bad = false;
    long parent = -1;                 // mnId of GetParent(), -1 for none
    std::vector<long> loop_edges;     // GetLoopEdges() in its iteration order
    std::vector<long> covisibles;     // GetCovisiblesByWeight(100) in its order
    std::vector<long> children;       // mnIds
    std::map<long, int> weights;      // GetWeight, needed for the members of LoopConnections
};
struct FlatMap {
    std::vector<FlatKeyFrame> kfs;                                         // in the order of pMap->GetAllKeyFrames(); vertex v is kfs[v]
    std::set<long> bad;                                                    // bad key frames that are not in kfs but may appear among covisibles
    std::vector<std::pair<long, std::vector<long>>> loop_connections;      // LoopConnections in std::map / std::set iteration order
    long loop_kf = 0, cur_kf = 0;
    std::map<long, std::vector<double>> Scw;                               // per mnId: CorrectedSim3 where there is an entry, Sim3(Rcw, tcw, 1.0) otherwise; tx ty tz qx qy qz qw s
    std::map<long, std::vector<double>> non_corrected;
};
struct EssentialGraph {
    std::vector<long> mnId;
    std::vector<int> edge_i, edge_j;
    std::vector<uint8_t> edge_kind, has_nc;
    int fixed_vertex = 0;
    std::vector<double> Scw, Snc;
};

// The vertices and edges of Optimizer.cc:2603-2776.  A bad key frame in kfs, or an edge to a key frame that is not in kfs, throws: the reference dereferences a null
// vertex there (:2791).
inline EssentialGraph build_essential_graph(const FlatMap &flat) {
    const int minFeat = 100;
    std::map<long, int> index;
    for (size_t v = 0; v < flat.kfs.size(); v++) {
        const FlatKeyFrame &kf = flat.kfs[v];
        if (kf.bad) throw std::invalid_argument("build_essential_graph: key frame " + std::to_string(kf.mnId) + " is bad; the reference gives it no vertex and dereferences a null pointer at Optimizer.cc:2791");
        if (!index.emplace(kf.mnId, (int)v).second) throw std::invalid_argument("build_essential_graph: key frame " + std::to_string(kf.mnId) + " appears twice");
    }
    auto vertex = [&](long id) -> int {
        auto it = index.find(id);
        if (it == index.end())
            throw std::invalid_argument("build_essential_graph: key frame " + std::to_string(id) + (flat.bad.count(id) ? " is bad" : " is not in the map") + "; an edge to it has a null vertex in the reference");
        return it->second;
    };
    vertex(flat.loop_kf); vertex(flat.cur_kf);
    EssentialGraph g;
    std::set<std::pair<long, long>> inserted;
    auto add = [&](int i, int j, int kind) { g.edge_i.push_back(i); g.edge_j.push_back(j); g.edge_kind.push_back((uint8_t)kind); };
    for (const auto &lc : flat.loop_connections) { // :2645-2673
        const long i = lc.first;
        for (long j : lc.second) {
            const FlatKeyFrame &kf = flat.kfs[(size_t)vertex(i)];
            const auto w = kf.weights.find(j);
            if ((i != flat.cur_kf || j != flat.loop_kf) && (w == kf.weights.end() ? 0 : w->second) < minFeat) continue;
            add(vertex(i), vertex(j), 0);
            inserted.insert(std::make_pair(std::min(i, j), std::max(i, j)));
        }
    }
    for (const FlatKeyFrame &kf : flat.kfs) { // :2676-2776
        const long i = kf.mnId;
        if (kf.parent >= 0) add(index[i], vertex(kf.parent), 1);
        for (long l : kf.loop_edges) if (l < i) add(index[i], vertex(l), 1);
        for (long nb : kf.covisibles) {
            if (nb < 0 || nb == kf.parent || std::count(kf.children.begin(), kf.children.end(), nb) || std::count(kf.loop_edges.begin(), kf.loop_edges.end(), nb)) continue;
            if (flat.bad.count(nb) || !(nb < i)) continue;
            if (inserted.count(std::make_pair(std::min(i, nb), std::max(i, nb)))) continue;
            add(index[i], vertex(nb), 1);
        }
    }
    const size_t n = flat.kfs.size();
    g.fixed_vertex = index[flat.loop_kf];
    g.Scw.assign(n * 8, 0.0); g.Snc.assign(n * 8, 0.0); g.has_nc.assign(n, 0);
    for (size_t v = 0; v < n; v++) {
        g.mnId.push_back(flat.kfs[v].mnId);
        const auto it = flat.Scw.find(flat.kfs[v].mnId);
        if (it == flat.Scw.end() || it->second.size() != 8) throw std::invalid_argument("build_essential_graph: key frame " + std::to_string(flat.kfs[v].mnId) + " has no Scw of 8 numbers");
        std::copy(it->second.begin(), it->second.end(), g.Scw.begin() + v * 8);
    }
    for (const auto &nc : flat.non_corrected) {
        const auto it = index.find(nc.first);
        if (it == index.end()) continue;
        if (nc.second.size() != 8) throw std::invalid_argument("build_essential_graph: a NonCorrectedSim3 entry needs 8 numbers");
        std::copy(nc.second.begin(), nc.second.end(), g.Snc.begin() + (size_t)it->second * 8);
        g.has_nc[(size_t)it->second] = 1;
    }
    return g;
}

struct EssentialGraphResult {
    EssentialGraph graph;
    std::vector<double> sim3;   // n x 8: the optimised Siw
    std::vector<float> Tiw;     // n x 12: [R | t / s] by rows, what the caller hands to SetPose
    std::vector<float> points;  // np x 3, for SetWorldPos
    cs_essential_graph_stats stats;
};

// P: np x 3 doubles (toVector3d of the float positions), nIDr: the mnId of the reference key frame chosen per point (:2813-2822); both may be empty.
inline EssentialGraphResult OptimizeEssentialGraph(Context &c, const FlatMap &flat, bool bFixScale, const std::vector<double> &P = {}, const std::vector<long> &nIDr = {}, int iterations = 20) {
    auto check = [&](int r, const char *what) { if (r != CS_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(r) + "): " + cs_last_error(c.ctx)); };
    EssentialGraphResult res;
    res.graph = build_essential_graph(flat);
    const EssentialGraph &g = res.graph;
    const int n = (int)g.mnId.size();
    if (P.size() != nIDr.size() * 3) throw std::invalid_argument("OptimizeEssentialGraph: one nIDr per point");
    std::vector<int> ref;
    for (long id : nIDr) {
        const auto it = std::find(g.mnId.begin(), g.mnId.end(), id);
        if (it == g.mnId.end()) throw std::invalid_argument("OptimizeEssentialGraph: a point's reference key frame " + std::to_string(id) + " is not in the map");
        ref.push_back((int)(it - g.mnId.begin()));
    }
    cs_essential_graph *eg = nullptr;
    check(cs_essential_graph_create(c.ctx, n, (int)g.edge_i.size(), g.edge_i.data(), g.edge_j.data(), g.edge_kind.data(), g.fixed_vertex, bFixScale ? 1 : 0, &eg), "cs_essential_graph_create");
    res.sim3.assign((size_t)n * 8, 0.0); res.Tiw.assign((size_t)n * 12, 0.f);
    const int r = cs_essential_graph_optimize(c.ctx, eg, g.Scw.data(), g.Snc.data(), g.has_nc.data(), iterations, res.sim3.data(), res.Tiw.data(), &res.stats);
    cs_essential_graph_destroy(eg);
    check(r, "cs_essential_graph_optimize");
    res.points.assign(P.size(), 0.f);
    if (!ref.empty()) check(cs_sim3_correct_points(c.ctx, (int)ref.size(), P.data(), ref.data(), n, g.Scw.data(), res.sim3.data(), res.points.data()), "cs_sim3_correct_points");
    return res;
}

} // namespace cubeslam
