// Host-side plan of the object BA (ba.hip): argument checks, the landmark-sorted observations and their shard, the pose-edge incidence, the Schur
// slot pattern with its (u, v) trip lists, the band plan, the elimination order with the symbolic factor, and the slot order of ba_schur_slots.
// Plain C++ (also compiled into the CPU driver tests/cpp/ba_plan_driver.cpp): nothing here needs a device, cs_ba_create only uploads what this builds.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <iterator>
#include <map>
#include <utility>
#include <vector>

#include "../../include/cubeslam_hip.h"

// CUBESLAM_BA_SOLVER as cs_ba_create read it: unset / "sparse" / "band" / "band1" (band, one workgroup) / "cr" (nested dissection, decided by cs_ba_create:
// it needs the device's LDS size); any other value keeps the library's choice between the band kernels and leaves nested dissection out, as it always did
enum BaSolverChoice { BA_SOLVER_NONE = 0, BA_SOLVER_SPARSE, BA_SOLVER_BAND, BA_SOLVER_BAND1, BA_SOLVER_CR, BA_SOLVER_OTHER };

constexpr int BA_BAND_MAX = 20;                 // widest band half-width: (Bc+2)(Bc+1) blocks of 288 B must fit the 160 KB LDS
constexpr size_t BA_CHOL_LDS_MAX = 150 * 1024;  // ba_chol_factor keeps the pivot block and the widest column of L (36 + 36 max_col doubles) in LDS

struct BaTrip { int u, v; }; // contributing observation pair of a Schur block; the layout of HIP's int2, as which the device reads it

struct BaPlan {
    int P = 0, C = 0, Q = 0;                           // pose blocks = C free cameras, then Q cuboids
    int lm_b = 0, lm_e = 0, o_b = 0, o_e = 0;          // this rank: landmarks [lm_b, lm_e), sorted observations [o_b, o_e)
    bool pose_edges = false;                           // camera-cuboid and point-cuboid edges (and setLambda on the pose diagonal) live on rank 0
    int n_slots = 0, max_col = 0, max_part = 0;
    long band_len = 0, reduce_len = 0;                 // doubles of the sparse factor storage / of [slots | reduced right-hand side]
    std::vector<int> cam_idx, obs_perm;                // camera -> pose block (-1: fixed); sorted-by-landmark position -> caller's observation index
    std::vector<int> o_cam, o_pt;                      // the observations sorted by landmark (stable)
    std::vector<double> o_uv, o_w, o_ur;               // o_ur: empty without p->obs_ur
    std::vector<int> lm_off, pose_off, pose_obs;       // CSR by landmark (all ranks' observations); per pose block this rank's observations, ascending
    std::vector<int> pe_off, pe_list;                  // per pose block its camera-cuboid / point-cuboid edges, (edge << 2) | kind
    std::vector<std::pair<int, int>> slot_rc;          // block (rows first, cols second) of every slot; (-1, -1): dead (edge of a fixed camera)
    std::vector<int> slot_off; std::vector<BaTrip> trips; // CSR over the slots: this rank's trips
    std::vector<int> slot_perm;                        // order in which ba_schur_slots takes the slots
    std::vector<int> pos, col_off, rows, pair_off, upd_tgt, slot_dst; std::vector<uint8_t> slot_tr; // elimination order and symbolic factor
    int graph_bc = 0, band_bc = 0, band_targets = 0;   // graph_bc: the graph's own half-width; band_bc = max(graph_bc, 1)
    bool use_band = false, band_twist = false;
    std::vector<int> tgt_slot, ct_off, ct_list, cr_off, cr_list, cq_off, cq_list; std::vector<uint8_t> tgt_tr; // band plan, filled when use_band
};

// Every argument check of cs_ba_create, before anything is allocated: counts, NULL arrays with positive counts, every index in range, CSR offsets that
// start at 0 and do not decrease, at least one free vertex.
inline int ba_plan_check(const cs_ba_problem *p, int rank, int world) {
    if (!p || world < 1 || rank < 0 || rank >= world || p->n_cams < 1 || p->n_points < 0 || p->n_cuboids < 0 || p->n_obs < 0 || p->n_cobs < 0 || p->n_pc < 0) return CS_ERR_BAD_ARG;
    if (!p->cam_pose || !p->cam_fixed || (p->n_points && !p->points) || (p->n_cuboids && (!p->cuboid_pose || !p->cuboid_scale || !p->cuboid_flags)) ||
        (p->n_obs && (!p->obs_cam || !p->obs_point || !p->obs_uv || !p->obs_inv_sigma2)) || (p->n_cobs && (!p->cobs_cam || !p->cobs_cuboid || !p->cobs_bbox || !p->cobs_info)) ||
        (p->n_pc && (!p->pc_cuboid || !p->pc_offsets)))
        return CS_ERR_BAD_ARG;
    auto in = [](int v, int n) { return v >= 0 && v < n; };
    for (int o = 0; o < p->n_obs; o++) if (!in(p->obs_point[o], p->n_points) || !in(p->obs_cam[o], p->n_cams)) return CS_ERR_BAD_ARG;
    for (int o = 0; o < p->n_cobs; o++) if (!in(p->cobs_cam[o], p->n_cams) || !in(p->cobs_cuboid[o], p->n_cuboids)) return CS_ERR_BAD_ARG;
    if (p->n_pc && p->pc_offsets[0] != 0) return CS_ERR_BAD_ARG;
    for (int o = 0; o < p->n_pc; o++) if (!in(p->pc_cuboid[o], p->n_cuboids) || p->pc_offsets[o + 1] < p->pc_offsets[o]) return CS_ERR_BAD_ARG;
    if (p->n_pc && p->pc_offsets[p->n_pc] > 0 && !p->pc_points) return CS_ERR_BAD_ARG;
    int P = p->n_cuboids;
    for (int i = 0; i < p->n_cams; i++) P += !p->cam_fixed[i];
    return P >= 1 ? CS_OK : CS_ERR_BAD_ARG;
}

// index mapping: non-fixed cameras, then cuboids (sparse_optimizer.cpp:166-190: non-marginalised first, by vertex id); the observations sorted by
// landmark (stable) with their CSR; this rank's share of the landmarks and, per pose block, of the observations
inline void ba_plan_sort_shard(const cs_ba_problem *p, int rank, int world, BaPlan &X) {
    X.cam_idx.assign(p->n_cams, -1);
    int P = 0;
    for (int i = 0; i < p->n_cams; i++) if (!p->cam_fixed[i]) X.cam_idx[i] = P++;
    X.C = P; X.Q = p->n_cuboids;
    X.P = P += p->n_cuboids;
    X.obs_perm.resize(p->n_obs);
    for (int o = 0; o < p->n_obs; o++) X.obs_perm[o] = o;
    std::stable_sort(X.obs_perm.begin(), X.obs_perm.end(), [&](int a, int c) { return p->obs_point[a] < p->obs_point[c]; });
    X.o_cam.resize(p->n_obs); X.o_pt.resize(p->n_obs); X.lm_off.assign((size_t)p->n_points + 1, 0);
    X.o_uv.resize((size_t)p->n_obs * 2); X.o_w.resize(p->n_obs); X.o_ur.resize(p->obs_ur ? p->n_obs : 0);
    for (int q = 0; q < p->n_obs; q++) {
        const int o = X.obs_perm[q];
        X.o_cam[q] = p->obs_cam[o]; X.o_pt[q] = p->obs_point[o]; X.o_uv[q * 2] = p->obs_uv[o * 2]; X.o_uv[q * 2 + 1] = p->obs_uv[o * 2 + 1]; X.o_w[q] = p->obs_inv_sigma2[o];
        if (p->obs_ur) X.o_ur[q] = p->obs_ur[o];
        X.lm_off[X.o_pt[q] + 1]++;
    }
    for (int l = 0; l < p->n_points; l++) X.lm_off[l + 1] += X.lm_off[l];
    X.lm_b = (int)((long)p->n_points * rank / world); X.lm_e = (int)((long)p->n_points * (rank + 1) / world);
    X.o_b = X.lm_off[X.lm_b]; X.o_e = X.lm_off[X.lm_e];
    // per pose block: this rank's observations (ascending)
    X.pose_off.assign(P + 1, 0);
    for (int q = X.o_b; q < X.o_e; q++) if (X.cam_idx[X.o_cam[q]] >= 0) X.pose_off[X.cam_idx[X.o_cam[q]] + 1]++;
    for (int i = 0; i < P; i++) X.pose_off[i + 1] += X.pose_off[i];
    X.pose_obs.assign(X.pose_off[P], 0);
    std::vector<int> at(X.pose_off.begin(), X.pose_off.end() - 1);
    for (int q = X.o_b; q < X.o_e; q++) { const int pi = X.cam_idx[X.o_cam[q]]; if (pi >= 0) X.pose_obs[at[pi]++] = q; }
}

// pose-edge incidence (edge order: camera-cuboid edges, then point-cuboid edges)
inline void ba_plan_pose_edges(const cs_ba_problem *p, BaPlan &X) {
    std::vector<std::vector<int>> pe(X.P);
    for (int o = 0; o < p->n_cobs; o++) {
        if (X.cam_idx[p->cobs_cam[o]] >= 0) pe[X.cam_idx[p->cobs_cam[o]]].push_back((o << 2) | 0);
        pe[X.C + p->cobs_cuboid[o]].push_back((o << 2) | 1);
    }
    for (int o = 0; o < p->n_pc; o++) pe[X.C + p->pc_cuboid[o]].push_back((o << 2) | 2);
    X.pe_off.assign(X.P + 1, 0); X.pe_list.clear();
    for (int i = 0; i < X.P; i++) { X.pe_off[i + 1] = X.pe_off[i] + (int)pe[i].size(); X.pe_list.insert(X.pe_list.end(), pe[i].begin(), pe[i].end()); }
}

// Schur pattern (BlockSolver::buildStructure block_solver.hpp:143-295) over ALL landmarks (identical on every rank); the contributing (obs_u, obs_v)
// pairs only for this rank's landmarks.  Slot s < P: diagonal block of pose s; slot P + o: the block of camera-cuboid edge o; then the camera-camera
// blocks in the order the landmarks create them.
inline void ba_plan_slots(const cs_ba_problem *p, BaPlan &X) {
    const int P = X.P;
    std::map<std::pair<int, int>, int> slot_of;
    X.slot_rc.clear();
    for (int i = 0; i < P; i++) { slot_of[std::make_pair(i, i)] = i; X.slot_rc.push_back(std::make_pair(i, i)); }
    for (int o = 0; o < p->n_cobs; o++) { // one block per camera-cuboid edge, slot P + o (fixed cameras: unused block)
        const int pi = X.cam_idx[p->cobs_cam[o]], pj = X.C + p->cobs_cuboid[o];
        X.slot_rc.push_back(pi >= 0 ? std::make_pair(pi, pj) : std::make_pair(-1, -1)); // fixed camera: dead block
        if (pi >= 0) slot_of[std::make_pair(pi, pj)] = P + o;
    }
    std::vector<std::vector<BaTrip>> slot_trips(X.slot_rc.size());
    for (int l = 0; l < p->n_points; l++) {
        const bool mine = l >= X.lm_b && l < X.lm_e;
        for (int u = X.lm_off[l]; u < X.lm_off[l + 1]; u++) {
            const int i1 = X.cam_idx[X.o_cam[u]];
            if (i1 < 0) continue;
            for (int v = X.lm_off[l]; v < X.lm_off[l + 1]; v++) {
                const int i2 = X.cam_idx[X.o_cam[v]];
                if (i2 < i1 || (i2 == i1 && v != u)) continue;
                auto key = std::make_pair(i1, i2);
                auto it = slot_of.find(key);
                int s;
                if (it == slot_of.end()) { s = (int)X.slot_rc.size(); slot_of[key] = s; X.slot_rc.push_back(key); slot_trips.emplace_back(); }
                else s = it->second;
                if (mine) slot_trips[s].push_back(BaTrip{u, v});
            }
        }
    }
    X.n_slots = (int)X.slot_rc.size();
    X.slot_off.assign(X.n_slots + 1, 0); X.trips.clear();
    for (int s = 0; s < X.n_slots; s++) { X.slot_off[s + 1] = X.slot_off[s] + (int)slot_trips[s].size(); X.trips.insert(X.trips.end(), slot_trips[s].begin(), slot_trips[s].end()); }
}

// band path plan: cuboids eliminated first, cameras in index order; used when the camera system is narrow-banded.  CS_ERR_CAPACITY when a band
// solver is asked for and the system is not.
inline int ba_plan_band(const cs_ba_problem *p, BaSolverChoice choice, BaPlan &X, const char **err) {
    const int P = X.P, C = X.C, Q = X.Q;
    bool okb = C >= 1;
    int Bc = 0;
    for (auto &rc : X.slot_rc) {
        if (rc.first < 0) continue;
        if (rc.first >= C && rc.second >= C && rc.first != rc.second) okb = false; // two cuboids in one block: not a graph Optimizer.cc builds
        if (rc.first < C && rc.second < C) Bc = std::max(Bc, std::abs(rc.first - rc.second));
    }
    std::vector<std::vector<std::pair<int, int>>> cub_edges(Q); // (camera, slot), alive edges only
    for (int o = 0; o < p->n_cobs; o++) { const int pi = X.cam_idx[p->cobs_cam[o]]; if (pi >= 0) cub_edges[p->cobs_cuboid[o]].push_back(std::make_pair(pi, P + o)); }
    for (auto &e : cub_edges) { std::stable_sort(e.begin(), e.end()); if (!e.empty()) Bc = std::max(Bc, e.back().first - e.front().first); }
    X.graph_bc = Bc;
    Bc = std::max(Bc, 1); // one free camera, or free cameras that share nothing: band_back's chunks hold (Bc + 1) / 2 columns, none at Bc = 0; the extra block is explicit zeros
    if (choice == BA_SOLVER_SPARSE) okb = false;
    if (Bc > BA_BAND_MAX) okb = false;
    if ((choice == BA_SOLVER_BAND || choice == BA_SOLVER_BAND1) && !okb) { *err = "CUBESLAM_BA_SOLVER=band: the reduced camera system is not narrow-banded"; return CS_ERR_CAPACITY; }
    if (!okb) return CS_OK;
    X.use_band = true; X.band_bc = Bc; X.band_targets = C * (Bc + 1);
    X.band_twist = Bc >= 1 && C >= 6 * (Bc + 1) && choice != BA_SOLVER_BAND1; // two-sided elimination once the chain is long enough to split
    X.tgt_slot.assign((size_t)C * (Bc + 1), -1); X.tgt_tr.assign((size_t)C * (Bc + 1), 0);
    for (int s2 = 0; s2 < (int)X.slot_rc.size(); s2++) {
        const int r0 = X.slot_rc[s2].first, c0 = X.slot_rc[s2].second;
        if (r0 < 0 || r0 >= C || c0 >= C) continue;
        if (s2 >= P && s2 < P + p->n_cobs) continue;
        // stored block = (rows r0, cols c0); the band keeps block (i, k) with i >= k
        if (r0 >= c0) { X.tgt_slot[(size_t)c0 * (Bc + 1) + (r0 - c0)] = s2; X.tgt_tr[(size_t)c0 * (Bc + 1) + (r0 - c0)] = 0; }
        else { X.tgt_slot[(size_t)r0 * (Bc + 1) + (c0 - r0)] = s2; X.tgt_tr[(size_t)r0 * (Bc + 1) + (c0 - r0)] = 1; }
    }
    std::vector<std::vector<int>> ct((size_t)C * (Bc + 1));
    std::vector<std::vector<int>> cr(C);
    X.cq_off.assign(Q + 1, 0); X.cq_list.clear(); X.ct_list.clear(); X.cr_list.clear();
    for (int q = 0; q < Q; q++) {
        const auto &e = cub_edges[q];
        for (size_t a = 0; a < e.size(); a++) {
            cr[e[a].first].push_back(q); cr[e[a].first].push_back(e[a].second);
            X.cq_list.push_back(e[a].second); X.cq_list.push_back(e[a].first);
            for (size_t c2 = 0; c2 < e.size(); c2++) {
                if (e[a].first < e[c2].first) continue; // target block (i, k) with i >= k; equal cameras: every ordered pair
                auto &l = ct[(size_t)e[c2].first * (Bc + 1) + (e[a].first - e[c2].first)];
                l.push_back(q); l.push_back(e[a].second); l.push_back(e[c2].second);
            }
        }
        X.cq_off[q + 1] = (int)(X.cq_list.size() / 2);
    }
    X.ct_off.assign(ct.size() + 1, 0);
    for (size_t t = 0; t < ct.size(); t++) { X.ct_off[t + 1] = X.ct_off[t] + (int)(ct[t].size() / 3); X.ct_list.insert(X.ct_list.end(), ct[t].begin(), ct[t].end()); }
    X.cr_off.assign(C + 1, 0);
    for (int i = 0; i < C; i++) { X.cr_off[i + 1] = X.cr_off[i] + (int)(cr[i].size() / 2); X.cr_list.insert(X.cr_list.end(), cr[i].begin(), cr[i].end()); }
    return CS_OK;
}

// ordering of the pose blocks: minimum degree on the block graph (the reference lets Eigen::SimplicialLDLT order with AMD,
// linear_solver_eigen.h:60-75); the simulated elimination also yields the structure of every column of L.  Then the symbolic factor: the storage
// Lb = [P diagonal blocks | off-diagonal blocks column by column], the destination of every update pair and of every slot.
inline int ba_plan_factor(BaPlan &X, const char **err) {
    const int P = X.P;
    std::vector<std::vector<int>> adj(P);
    for (auto &rc : X.slot_rc) if (rc.first != rc.second && rc.first >= 0) { adj[rc.first].push_back(rc.second); adj[rc.second].push_back(rc.first); }
    for (auto &a : adj) { std::sort(a.begin(), a.end()); a.erase(std::unique(a.begin(), a.end()), a.end()); }
    std::vector<int> &pos = X.pos, &col_off = X.col_off, &rows = X.rows, &pair_off = X.pair_off;
    pos.assign(P, -1);
    std::vector<std::vector<int>> col_struct(P); // by elimination position: neighbour node ids at elimination time
    {
        std::vector<char> gone(P, 0);
        for (int k = 0; k < P; k++) {
            int v = -1;
            for (int i = 0; i < P; i++) if (!gone[i] && (v < 0 || adj[i].size() < adj[v].size())) v = i;
            gone[v] = 1; pos[v] = k;
            std::vector<int> nb = adj[v];
            col_struct[k] = nb;
            for (int a : nb) { // remove v, connect the neighbours pairwise (sorted-vector sets)
                std::vector<int> &s = adj[a];
                std::vector<int> merged;
                merged.reserve(s.size() + nb.size());
                std::set_union(s.begin(), s.end(), nb.begin(), nb.end(), std::back_inserter(merged));
                merged.erase(std::remove_if(merged.begin(), merged.end(), [&](int x) { return x == v || x == a; }), merged.end());
                s.swap(merged);
            }
            adj[v].clear();
        }
    }
    col_off.assign(P + 1, 0); rows.clear(); pair_off.assign(P + 1, 0);
    X.max_col = 0;
    for (int k = 0; k < P; k++) {
        std::vector<int> r;
        for (int v : col_struct[k]) r.push_back(pos[v]);
        std::sort(r.begin(), r.end());
        rows.insert(rows.end(), r.begin(), r.end());
        col_off[k + 1] = (int)rows.size();
        pair_off[k + 1] = pair_off[k] + (int)(r.size() * (r.size() + 1) / 2);
        X.max_col = std::max(X.max_col, (int)r.size());
    }
    if ((size_t)(36 + (size_t)X.max_col * 36) * sizeof(double) > BA_CHOL_LDS_MAX) { *err = "reduced camera system too dense for the LDS column buffer"; return CS_ERR_CAPACITY; }
    auto find_block = [&](int col, int row) { // storage index of L(row, col), row > col
        const int *lo = rows.data() + col_off[col], *hi = rows.data() + col_off[col + 1];
        const int *it = std::lower_bound(lo, hi, row);
        return (it != hi && *it == row) ? P + (int)(it - rows.data()) : -1;
    };
    X.upd_tgt.assign((size_t)pair_off[P], 0);
    for (int k = 0; k < P; k++) {
        const int m = col_off[k + 1] - col_off[k];
        for (int bi = 0; bi < m; bi++)
            for (int bk = 0; bk <= bi; bk++) {
                const int ri = rows[col_off[k] + bi], rk = rows[col_off[k] + bk];
                X.upd_tgt[(size_t)pair_off[k] + bi * (bi + 1) / 2 + bk] = bi == bk ? ri : find_block(rk, ri);
            }
    }
    X.slot_dst.assign(X.n_slots, 0); X.slot_tr.assign(X.n_slots, 0);
    for (int s = 0; s < X.n_slots; s++) {
        if (X.slot_rc[s].first < 0) { X.slot_dst[s] = -1; continue; }
        const int a = pos[X.slot_rc[s].first], c = pos[X.slot_rc[s].second];
        if (a == c) X.slot_dst[s] = a;
        else if (a > c) X.slot_dst[s] = find_block(c, a);              // block (rows first, cols second) sits below the diagonal as is
        else { X.slot_dst[s] = find_block(a, c); X.slot_tr[s] = 1; }   // stored transposed
        if (X.slot_dst[s] < 0) { *err = "internal: Schur block outside the symbolic factor"; return CS_ERR_BAD_ARG; }
    }
    X.band_len = ((long)P + (long)rows.size()) * 36;
    return CS_OK;
}

// XCD-aware slot order for ba_schur_slots: sort by the smaller pose index of the block, cut into 8 contiguous ranges, deal range x to the workgroups
// with blockIdx % 8 == x (4 slots per workgroup)
inline void ba_plan_slot_perm(BaPlan &X) {
    const int ns = X.n_slots;
    std::vector<int> by_pose((size_t)ns), perm((size_t)((ns + 3) / 4) * 4, 0);
    for (int i = 0; i < ns; i++) by_pose[i] = i;
    auto keyf = [&](int q) { const int a = X.slot_rc[q].first, c = X.slot_rc[q].second; return a < 0 ? (1 << 30) : std::min(a, c); };
    std::stable_sort(by_pose.begin(), by_pose.end(), [&](int x, int y) { return keyf(x) < keyf(y); });
    const int nblk = (ns + 3) / 4;
    int next = 0;
    for (int x = 0; x < 8; x++) // blocks x, x+8, x+16, ... take consecutive slots of the sorted list
        for (int blk = x; blk < nblk; blk += 8)
            for (int k = 0; k < 4; k++) perm[(size_t)blk * 4 + k] = next < ns ? by_pose[next++] : -1;
    // the kernel stops at n_slots positions, so the first n_slots positions must be a permutation: fill in block order, skipping the holes (-1) of
    // the partially filled last blocks
    X.slot_perm.assign((size_t)ns, 0);
    size_t w = 0;
    for (size_t i = 0; i < perm.size() && w < (size_t)ns; i++) if (perm[i] >= 0) X.slot_perm[w++] = perm[i];
}

// The one place of the "never empty" convention: a list that may have no entry gets one dummy entry (zeros), so that every plan array that goes to
// the device has something to upload and no kernel is handed a block nothing was written to.  The offsets beside each list do not count the dummy.
inline void ba_plan_never_empty(BaPlan &X) {
    if (X.pose_obs.empty()) X.pose_obs.assign(1, 0);
    if (X.pe_list.empty()) X.pe_list.assign(1, 0);
    if (X.trips.empty()) X.trips.assign(1, BaTrip{0, 0});
    if (X.rows.empty()) X.rows.assign(1, 0);
    if (X.upd_tgt.empty()) X.upd_tgt.assign(1, 0);
    if (!X.use_band) return;
    if (X.ct_list.empty()) X.ct_list.assign(3, 0);
    if (X.cr_list.empty()) X.cr_list.assign(2, 0);
    if (X.cq_list.empty()) X.cq_list.assign(2, 0);
}

// The whole plan of a problem that passed ba_plan_check: a pure function of its arguments.  CS_ERR_CAPACITY (with *err) when a band solver is asked
// for and the camera system is not narrow-banded, or when a column of the sparse factor does not fit the LDS.
inline int ba_plan_build(const cs_ba_problem *p, int rank, int world, BaSolverChoice choice, BaPlan &X, const char **err) {
    const char *unused = nullptr;
    if (!err) err = &unused;
    X = BaPlan();
    X.pose_edges = rank == 0;
    ba_plan_sort_shard(p, rank, world, X);
    ba_plan_pose_edges(p, X);
    ba_plan_slots(p, X);
    int r = ba_plan_band(p, choice, X, err);
    if (r == CS_OK) r = ba_plan_factor(X, err);
    if (r != CS_OK) return r;
    ba_plan_slot_perm(X);
    X.reduce_len = (long)X.n_slots * 36 + (long)X.P * 6;
    const int nl = X.lm_e - X.lm_b; // workgroups of the widest launch that leaves one partial sum per workgroup
    X.max_part = std::max(std::max((X.o_e - X.o_b + 255) / 256, (p->n_cobs + p->n_pc + 255) / 256), std::max((int)(((long)X.P * 6 + (long)nl * 3 + 255) / 256), (nl + 255) / 256)) + 1;
    ba_plan_never_empty(X);
    return CS_OK;
}
