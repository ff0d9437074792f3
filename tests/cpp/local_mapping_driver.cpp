// TEST INFRASTRUCTURE: the HD text of cube_slam_amd/csrc/triangulate_math.h compiled by g++ (-ffp-contract=off) and called through ctypes by
// tests/test_local_mapping_mirrors.py -- the per-pair function the kernel lm_triangulate runs, the Jacobi it holds, and the per-point function of mp_normal_depth.
#include <cstring>

#include "triangulate_math.h"

extern "C" {
// cam: Rcw[9] tcw[3] Ow[3] fx fy cx cy invfx invfy mbf mb; obs: the eight floats of TriObs
int lm_driver_pair(const float *cam1, const float *obs1, const float *cam2, const float *obs2, float ratioFactor, float *x3D) {
    TriCam c1, c2;
    tri_make_cam(cam1, cam1 + 9, cam1 + 12, cam1[15], cam1[16], cam1[17], cam1[18], cam1[19], cam1[20], cam1[21], cam1[22], &c1);
    tri_make_cam(cam2, cam2 + 9, cam2 + 12, cam2[15], cam2[16], cam2[17], cam2[18], cam2[19], cam2[20], cam2[21], cam2[22], &c2);
    TriObs o1, o2;
    memcpy(&o1, obs1, sizeof o1); memcpy(&o2, obs2, sizeof o2);
    return triangulate_pair(c1, o1, c2, o2, ratioFactor, x3D);
}
void lm_driver_jacobi(const double *A16, double *v4) { jacobi_vmin4(A16, v4); }
void lm_driver_normal(const float *pos, const int *obs, int n_obs, const float *kf_Ow, int ref_kf, float level_scale, float top_scale, float *normal, float *min_distance,
                      float *max_distance) {
    mappoint_normal_depth(pos, obs, n_obs, kf_Ow, ref_kf, level_scale, top_scale, normal, min_distance, max_distance);
}
}
