// CPU driver of the object BA's host plan (cube_slam_amd/csrc/ba_plan.h): reads a cs_ba_problem from a flat binary file, runs ba_plan_check and
// ba_plan_build, prints the return codes and every array of the plan as text.  Test infrastructure (tests/test_ba_plan.py); a program of its own, so
// that the same source can also be built with -fsanitize=address,undefined.
//
//   ba_plan_driver FILE RANK WORLD CHOICE        CHOICE: none | sparse | band | band1 | cr | other
//
// FILE: int32 {n_cams, n_points, n_cuboids, n_obs, n_cobs, n_pc, has_ur, null_mask}, then cam_fixed int32[n_cams], obs_cam, obs_point int32[n_obs],
// obs_uv double[2 n_obs], obs_inv_sigma2 double[n_obs], obs_ur double[n_obs] (has_ur), cobs_cam, cobs_cuboid int32[n_cobs], pc_cuboid int32[n_pc],
// pc_offsets int32[n_pc + 1] (n_pc > 0).  The arrays the plan has no business reading (poses, points, scales, flags, boxes, information, cuboid points)
// are not in the file: each is one element long here when its count is positive and NULL otherwise.  Bit k of null_mask makes the k-th pointer of
// cs_ba_problem NULL (order: cam_pose, cam_fixed, points, cuboid_pose, cuboid_scale, cuboid_flags, obs_cam, obs_point, obs_uv, obs_inv_sigma2,
// cobs_cam, cobs_cuboid, cobs_bbox, cobs_info, pc_cuboid, pc_offsets, pc_points).
#include "../../cube_slam_amd/csrc/ba_plan.h"

#include <cstdio>
#include <cstring>

namespace {
struct Problem {
    cs_ba_problem p{};
    std::vector<uint8_t> cam_fixed;
    std::vector<int> obs_cam, obs_point, cobs_cam, cobs_cuboid, pc_cuboid, pc_offsets;
    std::vector<double> obs_uv, obs_w, obs_ur;
};
template <class T> bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

bool read_problem(const char *path, Problem &S) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int h[8];
    bool ok = fread(h, sizeof(int), 8, f) == 8;
    for (int k = 0; ok && k < 6; k++) ok = h[k] >= 0; // (negative counts are not what this driver is for)
    std::vector<int> fixed;
    cs_ba_problem &p = S.p;
    if (ok) {
        p.n_cams = h[0]; p.n_points = h[1]; p.n_cuboids = h[2]; p.n_obs = h[3]; p.n_cobs = h[4]; p.n_pc = h[5];
        ok = rd(f, fixed, (size_t)h[0]) && rd(f, S.obs_cam, (size_t)h[3]) && rd(f, S.obs_point, (size_t)h[3]) && rd(f, S.obs_uv, (size_t)h[3] * 2) && rd(f, S.obs_w, (size_t)h[3]) &&
             rd(f, S.obs_ur, h[6] ? (size_t)h[3] : 0) && rd(f, S.cobs_cam, (size_t)h[4]) && rd(f, S.cobs_cuboid, (size_t)h[4]) && rd(f, S.pc_cuboid, (size_t)h[5]) &&
             rd(f, S.pc_offsets, h[5] ? (size_t)h[5] + 1 : 0);
    }
    fclose(f);
    if (!ok) return false;
    S.cam_fixed.assign(fixed.begin(), fixed.end());
    static const double one_d[1] = {0};
    static const uint8_t one_b[1] = {0};
    const int n_pcp = S.pc_offsets.empty() ? 0 : S.pc_offsets.back();
    p.cam_pose = one_d; p.cam_fixed = ptr(S.cam_fixed); p.points = p.n_points ? one_d : nullptr;
    p.cuboid_pose = p.cuboid_scale = p.n_cuboids ? one_d : nullptr; p.cuboid_flags = p.n_cuboids ? one_b : nullptr;
    p.obs_cam = ptr(S.obs_cam); p.obs_point = ptr(S.obs_point); p.obs_uv = ptr(S.obs_uv); p.obs_inv_sigma2 = ptr(S.obs_w); p.obs_ur = ptr(S.obs_ur);
    p.cobs_cam = ptr(S.cobs_cam); p.cobs_cuboid = ptr(S.cobs_cuboid); p.cobs_bbox = p.cobs_info = p.n_cobs ? one_d : nullptr;
    p.pc_cuboid = ptr(S.pc_cuboid); p.pc_offsets = ptr(S.pc_offsets); p.pc_points = n_pcp > 0 ? one_d : nullptr;
    const void **fields[17] = {(const void **)&p.cam_pose, (const void **)&p.cam_fixed, (const void **)&p.points, (const void **)&p.cuboid_pose, (const void **)&p.cuboid_scale,
                               (const void **)&p.cuboid_flags, (const void **)&p.obs_cam, (const void **)&p.obs_point, (const void **)&p.obs_uv, (const void **)&p.obs_inv_sigma2,
                               (const void **)&p.cobs_cam, (const void **)&p.cobs_cuboid, (const void **)&p.cobs_bbox, (const void **)&p.cobs_info, (const void **)&p.pc_cuboid,
                               (const void **)&p.pc_offsets, (const void **)&p.pc_points};
    for (int k = 0; k < 17; k++) if (h[7] >> k & 1) *fields[k] = nullptr;
    return true;
}

void put(const char *name, const int *v, size_t n) { printf("i %s %zu", name, n); for (size_t i = 0; i < n; i++) printf(" %d", v[i]); printf("\n"); }
void put(const char *name, const std::vector<int> &v) { put(name, v.data(), v.size()); }
void put(const char *name, const std::vector<uint8_t> &v) { printf("i %s %zu", name, v.size()); for (uint8_t x : v) printf(" %d", (int)x); printf("\n"); }
void put(const char *name, const std::vector<double> &v) { printf("d %s %zu", name, v.size()); for (double x : v) printf(" %a", x); printf("\n"); }

void print_plan(const BaPlan &X) {
    printf("s P %d\ns C %d\ns Q %d\ns lm_b %d\ns lm_e %d\ns o_b %d\ns o_e %d\ns n_slots %d\ns max_col %d\ns max_part %d\ns band_len %ld\ns reduce_len %ld\n", X.P, X.C, X.Q, X.lm_b, X.lm_e, X.o_b,
           X.o_e, X.n_slots, X.max_col, X.max_part, X.band_len, X.reduce_len);
    printf("s graph_bc %d\ns band_bc %d\ns band_targets %d\ns use_band %d\ns band_twist %d\ns pose_edges %d\n", X.graph_bc, X.band_bc, X.band_targets, (int)X.use_band, (int)X.band_twist,
           (int)X.pose_edges);
    put("cam_idx", X.cam_idx); put("obs_perm", X.obs_perm); put("o_cam", X.o_cam); put("o_pt", X.o_pt); put("o_uv", X.o_uv); put("o_w", X.o_w); put("o_ur", X.o_ur);
    put("lm_off", X.lm_off); put("pose_off", X.pose_off); put("pose_obs", X.pose_obs); put("pe_off", X.pe_off); put("pe_list", X.pe_list);
    static_assert(sizeof(std::pair<int, int>) == 2 * sizeof(int) && sizeof(BaTrip) == 2 * sizeof(int), "pairs of ints, printed flat");
    put("slot_rc", X.slot_rc.empty() ? nullptr : &X.slot_rc[0].first, X.slot_rc.size() * 2);
    put("slot_off", X.slot_off); put("trips", X.trips.empty() ? nullptr : &X.trips[0].u, X.trips.size() * 2); put("slot_perm", X.slot_perm);
    put("pos", X.pos); put("col_off", X.col_off); put("rows", X.rows); put("pair_off", X.pair_off); put("upd_tgt", X.upd_tgt); put("slot_dst", X.slot_dst); put("slot_tr", X.slot_tr);
    put("tgt_slot", X.tgt_slot); put("tgt_tr", X.tgt_tr); put("ct_off", X.ct_off); put("ct_list", X.ct_list); put("cr_off", X.cr_off); put("cr_list", X.cr_list);
    put("cq_off", X.cq_off); put("cq_list", X.cq_list);
}

bool parse_choice(const char *s, BaSolverChoice &c) {
    static const char *names[6] = {"none", "sparse", "band", "band1", "cr", "other"};
    for (int k = 0; k < 6; k++) if (!strcmp(s, names[k])) { c = (BaSolverChoice)k; return true; }
    return false;
}
} // namespace

int main(int argc, char **argv) {
    Problem S;
    BaSolverChoice choice;
    if (argc != 5 || !parse_choice(argv[4], choice) || !read_problem(argv[1], S)) { fprintf(stderr, "usage: ba_plan_driver FILE RANK WORLD none|sparse|band|band1|cr|other\n"); return 2; }
    const int rank = atoi(argv[2]), world = atoi(argv[3]);
    const int rc = ba_plan_check(&S.p, rank, world);
    printf("s check %d\n", rc);
    if (rc != CS_OK) return 0;
    BaPlan X;
    const char *err = nullptr;
    const int rb = ba_plan_build(&S.p, rank, world, choice, X, &err);
    printf("s build %d\n", rb);
    if (err) printf("e %s\n", err);
    if (rb == CS_OK) print_plan(X);
    return 0;
}
