// TEST INFRASTRUCTURE: the stated definitions of cube_slam_amd/csrc/cv_svd_math.h and the matrices EPnP (csrc/epnp_math.h) hands them, for tests/test_pnp_solver_svd.py
// (compiled there into a temporary directory, g++ -O2 -ffp-contract=off, and called over ctypes).
#include <vector>

#include "cube_slam_amd/csrc/pnp_host.h"

extern "C" {
void probe_svd_sym_ut(double *A, int n, double *D, double *Ut) { cvx_svd_sym_ut(CvxSeq(), A, n, D, Ut); }
void probe_svd_uv(const double *A, int n, double *D, double *U, double *V) { std::vector<double> work(2 * (size_t)n * n); cvx_svd_uv(CvxSeq(), A, n, D, U, V, work.data()); }
void probe_solve_svd(const double *A, int m, int n, const double *b, double *x) { std::vector<double> work((size_t)m * n + (size_t)n * n + n); cvx_solve_svd(CvxSeq(), A, m, n, b, x, work.data()); }
void probe_invert3_svd(const double *A, double *Ainv) { double work[21]; cvx_invert3_svd(CvxSeq(), A, Ainv, work); }
// compute_pose on n correspondences (P3Dw, P2D as the solver holds them) -> the matrices on the way: cc (:418-420), MtM (:497), L_6x10, rho, ABt of the third approximation
// (:607-619), cws, and the pose; returns the N of :523-527
int probe_epnp(int n, const float *P3Dw, const float *P2D, const double *K, double *cws, double *cc, double *mtm, double *l_6x10, double *rho, double *abt, double *Rt) {
    const CvxSeq x;
    EpnpWork w;
    std::vector<double> points((size_t)n * PNP_POINT_DOUBLES);
    pnp_work_init(&w, K, n, points.data());
    for (int i = 0; i < n; i++) { for (int k = 0; k < 3; k++) w.pws[3 * i + k] = P3Dw[3 * i + k]; w.us[2 * i] = P2D[2 * i]; w.us[2 * i + 1] = P2D[2 * i + 1]; }
    epnp_choose_control_points(x, &w);
    epnp_compute_barycentric_coordinates(x, &w);
    epnp_compute_MtM(x, &w);
    for (int i = 0; i < 144; i++) mtm[i] = w.mtm[i];
    const int N = epnp_compute_pose(x, &w, Rt, Rt + 9); // (the same stages again, and the rest)
    for (int i = 0; i < 12; i++) cws[i] = w.cws[i / 3][i % 3];
    for (int i = 0; i < 9; i++) { cc[i] = w.cc[i]; abt[i] = w.abt[i]; }
    for (int i = 0; i < 60; i++) l_6x10[i] = w.l_6x10[i];
    for (int i = 0; i < 6; i++) rho[i] = w.rho[i];
    return N;
}
}
