// posegraph.hip -- ORB_SLAM2::Optimizer::OptimizeEssentialGraph on MI355X (gfx950).
//
// Replaces Optimizer::OptimizeEssentialGraph (reference orb_object_slam/include/Optimizer.h, src/Optimizer.cc:2575-2836): the 7-dof pose graph over every key frame that
// LoopClosing::CorrectLoop runs once a loop is accepted -- one VertexSim3Expmap per key frame (pLoopKF fixed), one EdgeSim3 per loop connection, spanning-tree edge,
// stored loop edge and strong covisibility edge, information I, no robust kernel, g2o's Levenberg-Marquardt with setUserLambdaInit(1e-16) -- and the correction of the
// map points that follows it (:2805-2835).  Which edges exist is decided by the caller (cube_slam_amd/host/essential_graph.hpp, cube_slam_amd.optimizer).
//
//   * eg_measure: one thread per edge, Sji = Sjw * Swi with sim3_mul / sim3_inverse, each end from NonCorrectedSim3 where a "normal" edge has an entry (:2684-2707)
//   * eg_error: one thread per edge, EdgeSim3::computeError = log((C * S_i) * S_j^-1) (types_seven_dof_expmap.h:106-114) and its chi2 = e . e
//   * eg_linearize: one thread per (edge, column): the 14 central differences of BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp, delta 1e-9) through
//     VertexSim3Expmap::oplusImpl, Sim3(update) * estimate.  Under fix_scale oplusImpl zeroes update[6]: both evaluations of the scale column are the same number and
//     the column is exactly zero.  A fixed vertex gets no Jacobian
//   * eg_assemble: one workgroup per free vertex (H_ii = sum J^T J, b_i = -sum J^T e over its incidence list in edge order) and one per connected pair (H_ij over the
//     edges of the pair in edge order).  No atomics
//   * eg_factor: block-7 sparse Cholesky of H + lambda I, left-looking and level-scheduled on the elimination tree: the columns of one level are independent, one
//     launch per level and one workgroup per column, which gathers L_ik L_jk^T from the row structure in a fixed order, factors its 7 x 7 diagonal, scales its column
//     and does its part of the forward substitution.  Consecutive levels of one column each (the chain under the root) share one launch of one workgroup.
//     eg_back runs the back substitution over the same levels downwards.  A non-positive pivot sets a status word: the trial's "solve failed"
//   * eg_update (oplus on a copy of the estimates: the backup / restore of a trial is which of two buffers is current), eg_reduce (chi2 and computeScale's sum in a
//     fixed order: strided thread partials, shuffle tree, four waves -- sim3opt.hip's)
// The host runs optimization_algorithm_levenberg.cpp's schedule and reads one record of four doubles per trial.  Where the solve fails the step is taken as zero (g2o
// applies whatever its x held before); the trial is undone either way.
// cs_essential_graph_solve (include/cubeslam_hip/essential_graph_solve.h) is a test probe of one linear solve: the assembly and the factor + back substitution are issued
// by eg_launch_assemble / eg_launch_solve for the optimiser and the probe alike.
#include "common.h"
#include "lm_schedule.h"
#include "sim3_math.h"
#include "../../include/cubeslam_hip/essential_graph_solve.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <set>
#include <vector>

namespace {

constexpr int EG_THREADS = 256;

__global__ void __launch_bounds__(EG_THREADS) eg_measure(int m, const int *ei, const int *ej, const uint8_t *kind, const double *Scw, const double *Snc, const uint8_t *has_nc, double *Cm) {
    const int e = blockIdx.x * EG_THREADS + threadIdx.x;
    if (e >= m) return;
    const int i = ei[e], j = ej[e];
    const bool normal = kind[e] != 0;
    const Sim3 Siw = sim3_load((normal && has_nc[i] ? Snc : Scw) + (long)i * 8), Sjw = sim3_load((normal && has_nc[j] ? Snc : Scw) + (long)j * 8);
    sim3_store(sim3_mul(Sjw, sim3_inverse(Siw)), Cm + (long)e * 8);
}

__device__ __forceinline__ void eg_edge_error(const Sim3 &C, const Sim3 &Si, const Sim3 &Sj, double *err) { sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inverse(Sj)), err); }

__global__ void __launch_bounds__(EG_THREADS) eg_error(int m, const int *ei, const int *ej, const double *Cm, const double *X, double *err /* nullable */, double *chi) {
    const int e = blockIdx.x * EG_THREADS + threadIdx.x;
    if (e >= m) return;
    double r[7];
    eg_edge_error(sim3_load(Cm + (long)e * 8), sim3_load(X + (long)ei[e] * 8), sim3_load(X + (long)ej[e] * 8), r);
    double c = r[0] * r[0];
#pragma unroll
    for (int k = 1; k < 7; k++) c += r[k] * r[k];
    chi[e] = c;
    if (err) {
#pragma unroll
        for (int k = 0; k < 7; k++) err[(long)e * 7 + k] = r[k];
    }
}

// J[(e * 14 + side * 7 + d) * 7 + k] = d err_k / d update_d of the vertex on `side`
__global__ void __launch_bounds__(EG_THREADS) eg_linearize(int m, const int *ei, const int *ej, const double *Cm, const double *X, int fixed, int fix_scale, double *J) {
    const long item = (long)blockIdx.x * EG_THREADS + threadIdx.x;
    if (item >= (long)m * 14) return;
    const int e = (int)(item / 14), col = (int)(item % 14), side = col >= 7 ? 1 : 0, d = col - side * 7;
    double *out = J + item * 7;
    const int vi = ei[e], vj = ej[e];
    if ((side ? vj : vi) == fixed || (fix_scale && d == 6)) {
#pragma unroll
        for (int k = 0; k < 7; k++) out[k] = 0.0;
        return;
    }
    const Sim3 C = sim3_load(Cm + (long)e * 8), Si = sim3_load(X + (long)vi * 8), Sj = sim3_load(X + (long)vj * 8);
    double acc[7];
#pragma unroll 1 // one body for both signs
    for (int sgn = 0; sgn < 2; sgn++) {
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = (k == d) ? (sgn ? -1e-9 : 1e-9) : 0.0;
        const Sim3 T = sim3_mul(sim3_exp(u), side ? Sj : Si);
        double r[7];
        if (side) eg_edge_error(C, Si, T, r); else eg_edge_error(C, T, Sj, r);
#pragma unroll
        for (int k = 0; k < 7; k++) acc[k] = sgn ? acc[k] - r[k] : r[k];
    }
    const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll
    for (int k = 0; k < 7; k++) out[k] = scalar * acc[k];
}

// blocks [0, nf): the diagonal block and the b of the free vertex at position blockIdx.x; blocks [nf, nf + nslots): the off-diagonal block of one connected pair.
// inc / slot_edge hold edge * 2 + side: the side of this vertex (diagonal), the side of the pair's row vertex (off-diagonal).  H is in L's layout.
__global__ void __launch_bounds__(64) eg_assemble(int nf, const int *inc_off, const int *inc, const int *slot_off, const int *slot_edge, const int *slot_blk, const int *col_start,
                                                  const double *J, const double *err, double *H, double *b) {
    const int t = threadIdx.x;
    if ((int)blockIdx.x < nf) {
        const int p = blockIdx.x;
        if (t >= 56) return;
        const int r = t < 49 ? t / 7 : t - 49, c = t < 49 ? t % 7 : 0;
        double acc = 0;
        for (int q = inc_off[p]; q < inc_off[p + 1]; q++) {
            const int e = inc[q] >> 1, side = inc[q] & 1;
            const double *Jr = J + ((long)e * 14 + side * 7 + r) * 7, *Jc = J + ((long)e * 14 + side * 7 + c) * 7, *E = err + (long)e * 7;
            double s;
            if (t < 49) { s = Jr[0] * Jc[0]; for (int k = 1; k < 7; k++) s += Jr[k] * Jc[k]; }
            else { s = Jr[0] * (-E[0]); for (int k = 1; k < 7; k++) s += Jr[k] * (-E[k]); }
            acc += s;
        }
        if (t < 49) H[(long)col_start[p] * 49 + t] = acc; else b[(long)p * 7 + r] = acc;
    } else {
        const int sl = blockIdx.x - nf;
        if (t >= 49) return;
        const int r = t / 7, c = t % 7;
        double acc = 0;
        for (int q = slot_off[sl]; q < slot_off[sl + 1]; q++) {
            const int e = slot_edge[q] >> 1, side = slot_edge[q] & 1;
            const double *Jr = J + ((long)e * 14 + side * 7 + r) * 7, *Jc = J + ((long)e * 14 + (1 - side) * 7 + c) * 7;
            double s = Jr[0] * Jc[0];
            for (int k = 1; k < 7; k++) s += Jr[k] * Jc[k];
            acc += s;
        }
        H[(long)slot_blk[sl] * 49 + t] = acc;
    }
}

// Column j of L (blocks col_start[j] .. col_start[j + 1]: the diagonal, then the rows of its structure ascending; a block is 7 x 7 row-major) and y_j.
// seq = 0: one workgroup per column of cols[0 .. ncols); seq = 1: one workgroup takes the ncols columns in order (a chain: each is the parent of the one before).
__global__ void __launch_bounds__(EG_THREADS) eg_factor(const int *cols, int ncols, int seq, const int *col_start, const int *upd_off, const int *upd_a, const int *upd_b, const int *row_off,
                                                        const int *row_blk, const int *row_col, const double *H, const double *b, double lambda, double *L, double *y, int *status) {
    __shared__ double s_D[49], s_t[7];
    const int tid = threadIdx.x;
    for (int q = seq ? 0 : (int)blockIdx.x, qe = seq ? ncols : (int)blockIdx.x + 1; q < qe; q++) {
        const int j = cols[q], c0 = col_start[j], nb = col_start[j + 1] - c0;
        for (int item = tid; item < nb * 49; item += EG_THREADS) {
            const int blk = c0 + item / 49, en = item % 49, r = en / 7, c = en % 7;
            double acc = H[(long)blk * 49 + en];
            if (blk == c0 && r == c) acc += lambda;
            for (int u = upd_off[blk]; u < upd_off[blk + 1]; u++) {
                const double *La = L + (long)upd_a[u] * 49 + r * 7, *Lb = L + (long)upd_b[u] * 49 + c * 7;
                double s = La[0] * Lb[0];
#pragma unroll
                for (int k = 1; k < 7; k++) s += La[k] * Lb[k];
                acc -= s;
            }
            if (blk == c0) s_D[en] = acc; else L[(long)blk * 49 + en] = acc;
        }
        if (tid < 7) { // b_j - sum_k L_jk y_k over the row structure, k ascending
            double s = b[(long)j * 7 + tid];
            for (int u = row_off[j]; u < row_off[j + 1]; u++) {
                const double *Lr = L + (long)row_blk[u] * 49 + tid * 7, *yk = y + (long)row_col[u] * 7;
                double v = Lr[0] * yk[0];
#pragma unroll
                for (int k = 1; k < 7; k++) v += Lr[k] * yk[k];
                s -= v;
            }
            s_t[tid] = s;
        }
        __syncthreads();
        if (tid == 0) { // 7 x 7 Cholesky in place (lower), then y_j = D^-1 t
            bool bad = false;
            for (int c = 0; c < 7; c++) {
                double dd = s_D[c * 7 + c];
                for (int k = 0; k < c; k++) dd -= s_D[c * 7 + k] * s_D[c * 7 + k];
                if (!(dd > 0)) { bad = true; dd = 1.0; }
                dd = sqrt(dd);
                s_D[c * 7 + c] = dd;
                for (int r = c + 1; r < 7; r++) {
                    double v = s_D[r * 7 + c];
                    for (int k = 0; k < c; k++) v -= s_D[r * 7 + k] * s_D[c * 7 + k];
                    s_D[r * 7 + c] = v / dd;
                }
                for (int k = c + 1; k < 7; k++) s_D[c * 7 + k] = 0.0;
            }
            if (bad) *status = 1;
            for (int r = 0; r < 7; r++) {
                double v = s_t[r];
                for (int k = 0; k < r; k++) v -= s_D[r * 7 + k] * s_t[k];
                s_t[r] = v / s_D[r * 7 + r];
            }
        }
        __syncthreads();
        if (tid < 49) L[(long)c0 * 49 + tid] = s_D[tid];
        if (tid >= 64 && tid < 71) y[(long)j * 7 + (tid - 64)] = s_t[tid - 64];
        for (int item = tid; item < (nb - 1) * 7; item += EG_THREADS) { // L_ij = B D^-T, a row at a time
            double *row = L + (long)(c0 + 1 + item / 7) * 49 + (item % 7) * 7;
            double x[7];
#pragma unroll
            for (int c = 0; c < 7; c++) {
                double v = row[c];
#pragma unroll
                for (int k = 0; k < c; k++) v -= x[k] * s_D[c * 7 + k];
                x[c] = v / s_D[c * 7 + c];
            }
#pragma unroll
            for (int c = 0; c < 7; c++) row[c] = x[c];
        }
        __syncthreads(); // s_D / s_t are rewritten, and this column's blocks are read, by the next column of a chain
    }
}

// x_j = D^-T (y_j - sum_i L_ij^T x_i) over the structure of column j, rows ascending
__global__ void __launch_bounds__(64) eg_back(const int *cols, int ncols, int seq, const int *col_start, const int *row_idx, const double *L, const double *y, double *x) {
    __shared__ double s_t[7];
    const int tid = threadIdx.x;
    for (int q = seq ? ncols - 1 : (int)blockIdx.x, qe = seq ? 0 : (int)blockIdx.x; q >= qe; q--) {
        const int j = cols[q], c0 = col_start[j], c1 = col_start[j + 1];
        if (tid < 7) {
            double s = y[(long)j * 7 + tid];
            for (int blk = c0 + 1; blk < c1; blk++) {
                const double *Lb = L + (long)blk * 49, *xi = x + (long)row_idx[blk] * 7;
                double v = Lb[tid] * xi[0];
#pragma unroll
                for (int k = 1; k < 7; k++) v += Lb[k * 7 + tid] * xi[k];
                s -= v;
            }
            s_t[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            const double *D = L + (long)c0 * 49;
            for (int r = 6; r >= 0; r--) {
                double v = s_t[r];
                for (int k = r + 1; k < 7; k++) v -= D[k * 7 + r] * s_t[k];
                s_t[r] = v / D[r * 7 + r];
            }
            for (int r = 0; r < 7; r++) x[(long)j * 7 + r] = s_t[r];
        }
        __syncthreads();
    }
}

// VertexSim3Expmap::oplusImpl on every free vertex: Xt = Sim3(update) * X; under fix_scale update[6] = 0 is written through to the solver's x
__global__ void __launch_bounds__(EG_THREADS) eg_update(int n, const int *pos, int fix_scale, int failed_is_zero, const int *status, double *x, const double *X, double *Xt) {
    const int v = blockIdx.x * EG_THREADS + threadIdx.x;
    if (v >= n) return;
    const int p = pos[v];
    Sim3 S = sim3_load(X + (long)v * 8);
    if (p >= 0) {
        double u[7];
        const bool zero = failed_is_zero && *status != 0;
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = zero ? 0.0 : x[(long)p * 7 + k];
        if (fix_scale) u[6] = 0.0;
        if (zero || fix_scale) {
#pragma unroll
            for (int k = 0; k < 7; k++) x[(long)p * 7 + k] = u[k];
        }
        S = sim3_mul(sim3_exp(u), S);
    }
    sim3_store(S, Xt + (long)v * 8);
}

// rec[slot] = sum chi; rec[2] = sum x (lambda x + b) where nx > 0; rec[3] = status.  One workgroup, a fixed order.
__global__ void __launch_bounds__(EG_THREADS) eg_reduce(int m, const double *chi, int slot, int nx, const double *x, const double *b, double lambda, const int *status, double *rec) {
    __shared__ double s_red[8];
    const int tid = threadIdx.x;
    double v[2] = {0, 0};
    for (int i = tid; i < m; i += EG_THREADS) v[0] += chi[i];
    for (int i = tid; i < nx; i += EG_THREADS) v[1] += x[i] * (lambda * x[i] + b[i]);
    block_reduce_waves(v, s_red);
    if (tid == 0) {
        rec[slot] = block_reduce_sum<2>(s_red, 0);
        if (nx > 0) { rec[2] = block_reduce_sum<2>(s_red, 1); rec[3] = (double)*status; }
    }
}

__global__ void __launch_bounds__(EG_THREADS) sim3_inverse_kernel(int n, const double *S, double *Sinv) {
    const int v = blockIdx.x * EG_THREADS + threadIdx.x;
    if (v < n) sim3_store(sim3_inverse(sim3_load(S + (long)v * 8)), Sinv + (long)v * 8);
}
__global__ void __launch_bounds__(EG_THREADS) sim3_correct_points_kernel(int np, const double *P, const int *ref, const double *Scw, const double *Swc_corrected, float *out) {
    const int p = blockIdx.x * EG_THREADS + threadIdx.x;
    if (p >= np) return;
    const int r = ref[p];
    const double in[3] = {P[(long)p * 3], P[(long)p * 3 + 1], P[(long)p * 3 + 2]};
    double a[3], c[3];
    sim3_map(sim3_load(Scw + (long)r * 8), in, a);
    sim3_map(sim3_load(Swc_corrected + (long)r * 8), a, c);
    out[(long)p * 3] = (float)c[0]; out[(long)p * 3 + 1] = (float)c[1]; out[(long)p * 3 + 2] = (float)c[2];
}
__global__ void __launch_bounds__(EG_THREADS) sim3_log_kernel(int n, const double *S, double *out) {
    const int v = blockIdx.x * EG_THREADS + threadIdx.x;
    if (v >= n) return;
    double r[7];
    sim3_log(sim3_load(S + (long)v * 8), r);
#pragma unroll
    for (int k = 0; k < 7; k++) out[(long)v * 7 + k] = r[k];
}

} // namespace

struct cs_essential_graph {
    cs_ctx *ctx = nullptr;
    cs_owner own;
    int n = 0, m = 0, fixed = 0, fix_scale = 0, nf = 0, nslots = 0, nLb = 0, nHb = 0, nlev = 0;
    struct Launch { int first, count, seq; };
    std::vector<Launch> launches; // over lev_cols, levels ascending
    std::vector<int> pos;         // by vertex: its position in the elimination order, -1 the fixed vertex (d_pos on the host)
    int *d_ei = nullptr, *d_ej = nullptr, *d_pos = nullptr, *d_inc_off = nullptr, *d_inc = nullptr, *d_slot_off = nullptr, *d_slot_edge = nullptr, *d_slot_blk = nullptr, *d_col_start = nullptr,
        *d_row_idx = nullptr, *d_upd_off = nullptr, *d_upd_a = nullptr, *d_upd_b = nullptr, *d_row_off = nullptr, *d_row_blk = nullptr, *d_row_col = nullptr, *d_lev_cols = nullptr, *d_status = nullptr;
    uint8_t *d_kind = nullptr, *d_has = nullptr;
    double *d_H = nullptr, *d_L = nullptr, *d_b = nullptr, *d_y = nullptr, *d_x = nullptr, *d_X = nullptr, *d_Xt = nullptr, *d_C = nullptr, *d_e = nullptr, *d_chi = nullptr, *d_J = nullptr,
           *d_rec = nullptr, *d_Scw = nullptr, *d_Snc = nullptr;
};

// The launches of one linear solve, shared by cs_essential_graph_optimize and cs_essential_graph_solve.
// H and b from d_J and d_e
static void eg_launch_assemble(cs_ctx *ctx, cs_essential_graph *g) {
    CS_LAUNCH(ctx, "eg_assemble", eg_assemble, dim3(g->nf + g->nslots), dim3(64), 0, g->nf, g->d_inc_off, g->d_inc, g->d_slot_off, g->d_slot_edge, g->d_slot_blk, g->d_col_start, g->d_J, g->d_e, g->d_H,
              g->d_b);
}
// d_x = (H + lambda I)^-1 b by position and d_status: the status word cleared, the factor over the launch list upwards, the back substitution downwards
static int eg_launch_solve(cs_ctx *ctx, cs_essential_graph *g, double lambda) {
    CS_HIP(ctx, hipMemsetAsync(g->d_status, 0, sizeof(int), ctx->stream));
    for (const auto &l : g->launches)
        CS_LAUNCH(ctx, "eg_factor", eg_factor, dim3(l.seq ? 1 : l.count), dim3(EG_THREADS), 0, g->d_lev_cols + l.first, l.count, l.seq, g->d_col_start, g->d_upd_off, g->d_upd_a, g->d_upd_b, g->d_row_off,
                  g->d_row_blk, g->d_row_col, g->d_H, g->d_b, lambda, g->d_L, g->d_y, g->d_status);
    for (size_t k = g->launches.size(); k-- > 0;) {
        const auto &l = g->launches[k];
        CS_LAUNCH(ctx, "eg_back", eg_back, dim3(l.seq ? 1 : l.count), dim3(64), 0, g->d_lev_cols + l.first, l.count, l.seq, g->d_col_start, g->d_row_idx, g->d_L, g->d_y, g->d_x);
    }
    return CS_OK;
}

extern "C" {

int cs_essential_graph_create(cs_ctx *ctx, int n_vertices, int n_edges, const int *edge_i, const int *edge_j, const uint8_t *edge_kind, int fixed_vertex, int fix_scale,
                              cs_essential_graph **out) {
    if (!ctx || !out || n_vertices < 2 || n_edges < 1 || !edge_i || !edge_j || !edge_kind || fixed_vertex < 0 || fixed_vertex >= n_vertices) return CS_ERR_BAD_ARG;
    for (int e = 0; e < n_edges; e++)
        if (edge_i[e] < 0 || edge_i[e] >= n_vertices || edge_j[e] < 0 || edge_j[e] >= n_vertices || edge_i[e] == edge_j[e] || edge_kind[e] > 1) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const int n = n_vertices, m = n_edges, nf = n - 1;
    // free vertices in index order, then the minimum-degree order of their graph (ties to the lower index)
    std::vector<int> fv_of(n, -1);
    for (int v = 0, k = 0; v < n; v++) if (v != fixed_vertex) fv_of[v] = k++;
    std::vector<std::set<int>> adj((size_t)nf);
    for (int e = 0; e < m; e++) {
        const int a = fv_of[edge_i[e]], b = fv_of[edge_j[e]];
        if (a >= 0 && b >= 0) { adj[a].insert(b); adj[b].insert(a); }
    }
    int nslots = 0;
    for (int a = 0; a < nf; a++) nslots += (int)adj[a].size();
    nslots /= 2;
    std::vector<int> pos_of_fv(nf, -1);
    std::vector<std::vector<int>> nb_at((size_t)nf); // by position: the neighbours (fv) left when it was eliminated
    std::vector<char> gone(nf, 0);
    for (int k = 0; k < nf; k++) {
        int best = -1;
        for (int a = 0; a < nf; a++) if (!gone[a] && (best < 0 || adj[a].size() < adj[best].size())) best = a;
        gone[best] = 1; pos_of_fv[best] = k;
        nb_at[k].assign(adj[best].begin(), adj[best].end());
        for (int a : nb_at[k]) adj[a].erase(best);
        for (size_t s = 0; s < nb_at[k].size(); s++) for (size_t t = s + 1; t < nb_at[k].size(); t++) { adj[nb_at[k][s]].insert(nb_at[k][t]); adj[nb_at[k][t]].insert(nb_at[k][s]); }
    }
    // the structure of L by column, the elimination tree and its levels
    std::vector<int> col_start(nf + 1, 0), row_idx, parent(nf, -1), level(nf, 0);
    for (int k = 0; k < nf; k++) {
        std::vector<int> rows;
        for (int a : nb_at[k]) rows.push_back(pos_of_fv[a]);
        std::sort(rows.begin(), rows.end());
        row_idx.push_back(k);
        row_idx.insert(row_idx.end(), rows.begin(), rows.end());
        col_start[k + 1] = (int)row_idx.size();
        if (!rows.empty()) parent[k] = rows[0];
    }
    const int nLb = (int)row_idx.size();
    int nlev = 0;
    for (int k = 0; k < nf; k++) {
        if (parent[k] >= 0) level[parent[k]] = std::max(level[parent[k]], level[k] + 1);
        nlev = std::max(nlev, level[k] + 1);
    }
    auto block_of = [&](int row, int col) -> int { // the block (row, col) of L, row > col; it exists wherever it is asked for
        const int *a = row_idx.data() + col_start[col] + 1, *b = row_idx.data() + col_start[col + 1];
        const int *it = std::lower_bound(a, b, row);
        return (it != b && *it == row) ? (int)(it - row_idx.data()) : -1;
    };
    // row structure: for row j the blocks L_jk, k ascending
    std::vector<std::vector<int>> rl_blk((size_t)nf), rl_col((size_t)nf);
    for (int k = 0; k < nf; k++) for (int blk = col_start[k] + 1; blk < col_start[k + 1]; blk++) { rl_blk[row_idx[blk]].push_back(blk); rl_col[row_idx[blk]].push_back(k); }
    std::vector<int> row_off(nf + 1, 0), row_blk, row_col;
    for (int j = 0; j < nf; j++) { row_blk.insert(row_blk.end(), rl_blk[j].begin(), rl_blk[j].end()); row_col.insert(row_col.end(), rl_col[j].begin(), rl_col[j].end()); row_off[j + 1] = (int)row_blk.size(); }
    // updates: block (i, j) of column j receives L_ik L_jk^T for every k in the row structure of j with a block in row i, k ascending
    std::vector<std::vector<int>> ua((size_t)nLb), ub((size_t)nLb);
    for (int j = 0; j < nf; j++)
        for (size_t s = 0; s < rl_blk[j].size(); s++) {
            const int bjk = rl_blk[j][s], k = rl_col[j][s];
            ua[col_start[j]].push_back(bjk); ub[col_start[j]].push_back(bjk);
            for (int blk = bjk + 1; blk < col_start[k + 1]; blk++) { // rows of column k below j
                const int dst = block_of(row_idx[blk], j);
                if (dst < 0) return CS_ERR_CAPACITY; // cannot happen: the structure of a column contains that of its children above it
                ua[dst].push_back(blk); ub[dst].push_back(bjk);
            }
        }
    std::vector<int> upd_off(nLb + 1, 0), upd_a, upd_b;
    for (int blk = 0; blk < nLb; blk++) { upd_a.insert(upd_a.end(), ua[blk].begin(), ua[blk].end()); upd_b.insert(upd_b.end(), ub[blk].begin(), ub[blk].end()); upd_off[blk + 1] = (int)upd_a.size(); }
    // level sets, columns ascending inside a level; runs of one-column levels become one sequential launch
    std::vector<int> lev_cnt(nlev + 1, 0), lev_cols(nf);
    for (int k = 0; k < nf; k++) lev_cnt[level[k] + 1]++;
    for (int l = 0; l < nlev; l++) lev_cnt[l + 1] += lev_cnt[l];
    { std::vector<int> fill(lev_cnt.begin(), lev_cnt.end() - 1); for (int k = 0; k < nf; k++) lev_cols[fill[level[k]]++] = k; }
    cs_essential_graph *g = new cs_essential_graph();
    g->ctx = ctx; g->n = n; g->m = m; g->fixed = fixed_vertex; g->fix_scale = fix_scale ? 1 : 0; g->nf = nf; g->nslots = nslots; g->nLb = nLb; g->nHb = nf + nslots; g->nlev = nlev;
    for (int l = 0; l < nlev; l++) {
        const int first = lev_cnt[l], count = lev_cnt[l + 1] - lev_cnt[l];
        if (count == 1 && !g->launches.empty() && g->launches.back().seq && parent[lev_cols[first - 1]] == lev_cols[first]) g->launches.back().count++;
        else g->launches.push_back({first, count, count == 1 ? 1 : 0});
    }
    // incidence lists by position and the slots, both in edge order
    std::vector<int> pos(n, -1);
    for (int v = 0; v < n; v++) if (fv_of[v] >= 0) pos[v] = pos_of_fv[fv_of[v]];
    std::vector<std::vector<int>> inc_l((size_t)nf), slot_l((size_t)nLb);
    for (int e = 0; e < m; e++) {
        const int pi = pos[edge_i[e]], pj = pos[edge_j[e]];
        if (pi >= 0) inc_l[pi].push_back(e * 2);
        if (pj >= 0) inc_l[pj].push_back(e * 2 + 1);
        if (pi >= 0 && pj >= 0) {
            const int blk = block_of(std::max(pi, pj), std::min(pi, pj));
            if (blk < 0) { delete g; return CS_ERR_CAPACITY; }
            slot_l[blk].push_back(e * 2 + (pj > pi ? 1 : 0));
        }
    }
    std::vector<int> inc_off(nf + 1, 0), inc, slot_off(1, 0), slot_edge, slot_blk;
    for (int p = 0; p < nf; p++) { inc.insert(inc.end(), inc_l[p].begin(), inc_l[p].end()); inc_off[p + 1] = (int)inc.size(); }
    for (int blk = 0; blk < nLb; blk++) if (!slot_l[blk].empty()) { slot_edge.insert(slot_edge.end(), slot_l[blk].begin(), slot_l[blk].end()); slot_off.push_back((int)slot_edge.size()); slot_blk.push_back(blk); }
    if ((int)slot_blk.size() != nslots) { delete g; return CS_ERR_CAPACITY; }
    std::vector<int> vi(edge_i, edge_i + m), vj(edge_j, edge_j + m);
    std::vector<uint8_t> vk(edge_kind, edge_kind + m);
    cs_owner &o = g->own;
    int r = o.upload(ctx, &g->d_ei, vi.data(), vi.size());
    if (!r) r = o.upload(ctx, &g->d_ej, vj.data(), vj.size()); if (!r) r = o.upload(ctx, &g->d_kind, vk.data(), vk.size()); if (!r) r = o.upload(ctx, &g->d_pos, pos.data(), pos.size());
    if (!r) r = o.upload(ctx, &g->d_inc_off, inc_off.data(), inc_off.size()); if (!r) r = o.upload(ctx, &g->d_inc, inc.data(), inc.size());
    if (!r) r = o.upload(ctx, &g->d_slot_off, slot_off.data(), slot_off.size()); if (!r) r = o.upload(ctx, &g->d_slot_edge, slot_edge.data(), slot_edge.size()); if (!r) r = o.upload(ctx, &g->d_slot_blk, slot_blk.data(), slot_blk.size());
    if (!r) r = o.upload(ctx, &g->d_col_start, col_start.data(), col_start.size()); if (!r) r = o.upload(ctx, &g->d_row_idx, row_idx.data(), row_idx.size());
    if (!r) r = o.upload(ctx, &g->d_upd_off, upd_off.data(), upd_off.size()); if (!r) r = o.upload(ctx, &g->d_upd_a, upd_a.data(), upd_a.size()); if (!r) r = o.upload(ctx, &g->d_upd_b, upd_b.data(), upd_b.size());
    if (!r) r = o.upload(ctx, &g->d_row_off, row_off.data(), row_off.size()); if (!r) r = o.upload(ctx, &g->d_row_blk, row_blk.data(), row_blk.size()); if (!r) r = o.upload(ctx, &g->d_row_col, row_col.data(), row_col.size());
    if (!r) r = o.upload(ctx, &g->d_lev_cols, lev_cols.data(), lev_cols.size());
    const size_t N = (size_t)n, M = (size_t)m, NF = (size_t)nf, LB = (size_t)nLb;
    if (!r) r = o.alloc(ctx, &g->d_status, 1); if (!r) r = o.alloc(ctx, &g->d_has, N);
    if (!r) r = o.alloc(ctx, &g->d_H, LB * 49); if (!r) r = o.alloc(ctx, &g->d_L, LB * 49);
    if (!r) r = o.alloc(ctx, &g->d_b, NF * 7); if (!r) r = o.alloc(ctx, &g->d_y, NF * 7); if (!r) r = o.alloc(ctx, &g->d_x, NF * 7);
    if (!r) r = o.alloc(ctx, &g->d_X, N * 8); if (!r) r = o.alloc(ctx, &g->d_Xt, N * 8); if (!r) r = o.alloc(ctx, &g->d_Scw, N * 8); if (!r) r = o.alloc(ctx, &g->d_Snc, N * 8);
    if (!r) r = o.alloc(ctx, &g->d_C, M * 8); if (!r) r = o.alloc(ctx, &g->d_e, M * 7); if (!r) r = o.alloc(ctx, &g->d_chi, M); if (!r) r = o.alloc(ctx, &g->d_J, M * 98);
    if (!r) r = o.alloc(ctx, &g->d_rec, 4);
    if (!r) { // the fill-in blocks of H stay zero: eg_assemble writes the others
        const hipError_t e = hipMemsetAsync(g->d_H, 0, LB * 49 * sizeof(double), ctx->stream);
        if (e != hipSuccess) { ctx->err = hipGetErrorString(e); r = CS_ERR_HIP; }
    }
    g->pos = pos;
    const hipError_t e = hipStreamSynchronize(ctx->stream); // the host vectors above go out of scope
    if (!r && e != hipSuccess) { ctx->err = hipGetErrorString(e); r = CS_ERR_HIP; }
    if (r) { g->own.free_all(ctx); delete g; return r; }
    *out = g;
    return CS_OK;
}

void cs_essential_graph_destroy(cs_essential_graph *eg) {
    if (!eg) return;
    eg->own.free_all(eg->ctx);
    delete eg;
}

int cs_essential_graph_optimize(cs_ctx *ctx, cs_essential_graph *g, const double *Scw, const double *Snc, const uint8_t *has_nc, int iterations, double *sim3_out, float *Tiw_out,
                                cs_essential_graph_stats *stats) {
    if (!ctx || !g || g->ctx != ctx || !Scw || !Snc || !has_nc || iterations < 0 || !sim3_out || !Tiw_out) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const int n = g->n, m = g->m, nf = g->nf;
    const size_t N = (size_t)n;
    const dim3 gv((n + EG_THREADS - 1) / EG_THREADS), ge((m + EG_THREADS - 1) / EG_THREADS), gl((unsigned)(((long)m * 14 + EG_THREADS - 1) / EG_THREADS)), tb(EG_THREADS);
    int r = cs_h2d(ctx, g->d_Scw, Scw, N * 8);
    if (!r) r = cs_h2d(ctx, g->d_Snc, Snc, N * 8);
    if (!r) r = cs_h2d(ctx, g->d_has, has_nc, N);
    if (r) return r;
    CS_HIP(ctx, hipMemcpyAsync(g->d_X, g->d_Scw, N * 8 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    CS_LAUNCH(ctx, "eg_measure", eg_measure, ge, tb, 0, m, g->d_ei, g->d_ej, g->d_kind, g->d_Scw, g->d_Snc, g->d_has, g->d_C);
    cs_essential_graph_stats st;
    memset(&st, 0, sizeof st);
    st.levels = g->nlev; st.l_blocks = g->nLb; st.h_blocks = g->nHb;
    st.launches_per_trial = 2 * (int)g->launches.size() + 3;
    double *X = g->d_X, *Xt = g->d_Xt;
    double rec[4] = {0, 0, 0, 0};
    LmSchedule lm;
    for (int it = 0; it < iterations; it++) { // OptimizationAlgorithmLevenberg::solve
        CS_LAUNCH(ctx, "eg_error", eg_error, ge, tb, 0, m, g->d_ei, g->d_ej, g->d_C, X, g->d_e, g->d_chi);
        CS_LAUNCH(ctx, "eg_reduce", eg_reduce, dim3(1), tb, 0, m, g->d_chi, 0, 0, g->d_x, g->d_b, 0.0, g->d_status, g->d_rec);
        CS_LAUNCH(ctx, "eg_linearize", eg_linearize, gl, tb, 0, m, g->d_ei, g->d_ej, g->d_C, X, g->fixed, g->fix_scale, g->d_J);
        eg_launch_assemble(ctx, g);
        if (it == 0) lm.start(1e-16); // computeLambdaInit: _userLambdaInit > 0
        lm.begin_iteration();
        double currentChi = 0, iniChi = 0;
        st.iterations++;
        do {
            r = eg_launch_solve(ctx, g, lm.lambda);
            if (r) return r;
            CS_LAUNCH(ctx, "eg_update", eg_update, gv, tb, 0, n, g->d_pos, g->fix_scale, 1, g->d_status, g->d_x, X, Xt);
            CS_LAUNCH(ctx, "eg_error", eg_error, ge, tb, 0, m, g->d_ei, g->d_ej, g->d_C, Xt, (double *)nullptr, g->d_chi);
            CS_LAUNCH(ctx, "eg_reduce", eg_reduce, dim3(1), tb, 0, m, g->d_chi, 1, nf * 7, g->d_x, g->d_b, lm.lambda, g->d_status, g->d_rec);
            r = cs_d2h(ctx, rec, g->d_rec, 4);
            if (r) return r;
            CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (lm.qmax == 0) { currentChi = iniChi = rec[0]; if (it == 0) st.chi2_first = rec[0]; }
            const bool accepted = lm.trial(currentChi, rec[1], rec[3] == 0.0, rec[2]);
            if (accepted) {
                std::swap(X, Xt); // the trial's estimates stand; a rejected trial's are simply not taken
                st.accepted++;
            } else st.rejected++;
            if (st.trials < CS_EG_MAX_TRIALS) st.trial_accepted[st.trials] = accepted ? 1 : 0;
            st.trials++;
        } while (lm.retry());
        st.chi2_last = currentChi;
        if (lm.stop(iniChi, currentChi)) break;
    }
    st.lambda_last = lm.lambda;
    r = cs_d2h(ctx, sim3_out, X, N * 8);
    if (r) return r;
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int v = 0; v < n; v++) { // :2794-2800: toRotationMatrix, eigt *= (1. / s), toCvSE3's floats
        const Sim3 S = sim3_load(sim3_out + (size_t)v * 8);
        double R[3][3];
        qtoR(S.r, R);
        const double k = 1. / S.s;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) Tiw_out[(size_t)v * 12 + a * 4 + b] = (float)R[a][b];
            Tiw_out[(size_t)v * 12 + a * 4 + 3] = (float)(S.t[a] * k);
        }
    }
    if (stats) *stats = st;
    return CS_OK;
}

// include/cubeslam_hip/essential_graph_solve.h
int cs_essential_graph_solve_version(void) { return CS_ESSENTIAL_GRAPH_SOLVE_VERSION; }

int cs_essential_graph_solve(cs_ctx *ctx, cs_essential_graph *g, const double *J, const double *err, double lambda, double *x_out, int *status) {
    if (!ctx || !g || g->ctx != ctx || !J || !err || !x_out || !status) return CS_ERR_BAD_ARG;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t M = (size_t)g->m, NF = (size_t)g->nf;
    CS_TRY(cs_h2d(ctx, g->d_J, J, M * 98));
    CS_TRY(cs_h2d(ctx, g->d_e, err, M * 7));
    eg_launch_assemble(ctx, g);
    CS_TRY(eg_launch_solve(ctx, g, lambda));
    std::vector<double> x(NF * 7);
    int st = 0;
    CS_TRY(cs_d2h(ctx, x.data(), g->d_x, NF * 7));
    CS_TRY(cs_d2h(ctx, &st, g->d_status, 1));
    CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int v = 0; v < g->n; v++)
        for (int k = 0; k < 7; k++) x_out[(size_t)v * 7 + k] = g->pos[v] >= 0 ? x[(size_t)g->pos[v] * 7 + k] : 0.0;
    *status = st;
    return CS_OK;
}

int cs_sim3_correct_points(cs_ctx *ctx, int n_points, const double *P, const int *ref_vertex, int n_vertices, const double *Scw, const double *sim3_out, float *P_out) {
    if (!ctx || n_points < 0 || n_vertices < 1 || !Scw || !sim3_out || (n_points && (!P || !ref_vertex || !P_out))) return CS_ERR_BAD_ARG;
    for (int p = 0; p < n_points; p++) if (ref_vertex[p] < 0 || ref_vertex[p] >= n_vertices) return CS_ERR_BAD_ARG;
    if (n_points == 0) return CS_OK;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)n_vertices, NP = (size_t)n_points;
    cs_scratch sc(ctx);
    double *d_S = nullptr, *d_C = nullptr, *d_Ci = nullptr, *d_P = nullptr; int *d_ref = nullptr; float *d_out = nullptr;
    CS_TRY(sc.alloc(ctx, &d_S, N * 8)); CS_TRY(sc.alloc(ctx, &d_C, N * 8)); CS_TRY(sc.alloc(ctx, &d_Ci, N * 8)); CS_TRY(sc.alloc(ctx, &d_P, NP * 3)); CS_TRY(sc.alloc(ctx, &d_ref, NP)); CS_TRY(sc.alloc(ctx, &d_out, NP * 3));
    CS_TRY(cs_h2d(ctx, d_S, Scw, N * 8)); CS_TRY(cs_h2d(ctx, d_C, sim3_out, N * 8)); CS_TRY(cs_h2d(ctx, d_P, P, NP * 3)); CS_TRY(cs_h2d(ctx, d_ref, ref_vertex, NP));
    CS_LAUNCH(ctx, "sim3_inverse_kernel", sim3_inverse_kernel, dim3((n_vertices + EG_THREADS - 1) / EG_THREADS), dim3(EG_THREADS), 0, n_vertices, d_C, d_Ci);
    CS_LAUNCH(ctx, "sim3_correct_points_kernel", sim3_correct_points_kernel, dim3((n_points + EG_THREADS - 1) / EG_THREADS), dim3(EG_THREADS), 0, n_points, d_P, d_ref, d_S, d_Ci, d_out);
    CS_TRY(cs_d2h(ctx, P_out, d_out, NP * 3));
    const hipError_t e = hipStreamSynchronize(ctx->stream); sc.drained = true;
    if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return CS_ERR_HIP; }
    return CS_OK;
}

int cs_sim3_log(cs_ctx *ctx, int n, const double *sim3, double *log_out) {
    if (!ctx || n < 0 || (n && (!sim3 || !log_out))) return CS_ERR_BAD_ARG;
    if (n == 0) return CS_OK;
    CS_HIP(ctx, hipSetDevice(ctx->device));
    cs_scratch sc(ctx);
    double *d_S = nullptr, *d_o = nullptr;
    CS_TRY(sc.alloc(ctx, &d_S, (size_t)n * 8)); CS_TRY(sc.alloc(ctx, &d_o, (size_t)n * 7));
    CS_TRY(cs_h2d(ctx, d_S, sim3, (size_t)n * 8));
    CS_LAUNCH(ctx, "sim3_log_kernel", sim3_log_kernel, dim3((n + EG_THREADS - 1) / EG_THREADS), dim3(EG_THREADS), 0, n, d_S, d_o);
    CS_TRY(cs_d2h(ctx, log_out, d_o, (size_t)n * 7));
    const hipError_t e = hipStreamSynchronize(ctx->stream); sc.drained = true;
    if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return CS_ERR_HIP; }
    return CS_OK;
}

} // extern "C"
