// Device code of the band solver of the object BA's reduced camera system: included by ba.hip, inside its anonymous namespace, between the band
// assembly kernels and the sparse Cholesky (the order of the kernels in the translation unit is part of what is compared between builds).
// ---- block-band Cholesky of the camera system.  A: C columns x (Bc+1) blocks (block d of column j = block (j+d, j), row-major 6x6).
// The elimination is a serial chain over the columns (each step: 6x6 pivot, Bc panel blocks, Bc(Bc+1)/2 trailing blocks, all in
// LDS), so it is run from BOTH ends at once ("twisted" factorisation): workgroup 0 eliminates columns 0, 1, 2, ... of A,
// workgroup 1 eliminates C-1, C-2, ... (the same band algorithm on the index-reversed matrix, whose columns are gathered from A
// with a transpose), each stopping before a middle group of R = Bc cameras.  Neither side creates fill outside the band, the
// middle group receives the Schur updates of both sides (ba_band_mid adds them, factors the dense 6R x 6R block and solves it),
// and the two back substitutions again run concurrently.  Half the chain length, three launches instead of one.
// A "side" sees the principal submatrix of its ne eliminated columns plus the R tail (middle) columns, in its own (local) order.
#pragma once
struct BandView {
    const double *A, *rhs; // the assembled band and right-hand side (original order)
    int C, Bc, n, ne, rev; // n = ne + tail columns; rev: local column j is original column C-1-j
    int lf_base;           // first column of this side in the factor storage Lf / ybuf
};
__device__ __forceinline__ double band_a(const BandView &V, int cn, int i) { // element i (block d = i/36) of local column cn
    const int d = i / 36;
    if (cn + d >= V.n) return 0.0; // rows outside the side's submatrix
    if (!V.rev) return V.A[(long)cn * ((V.Bc + 1) * 36) + i];
    if (cn >= V.ne) return 0.0;    // middle x middle blocks (and the middle right-hand side) are counted once, by the forward side
    const int e = i - d * 36, r = e / 6, c = e - r * 6, o = V.C - 1 - cn;
    return V.A[(long)(o - d) * ((V.Bc + 1) * 36) + d * 36 + c * 6 + r]; // reversed block (cn+d, cn) = A(o, o-d)^T ... stored in column o-d
}
__device__ __forceinline__ double band_b(const BandView &V, int cn, int t) {
    if (cn >= V.n) return 0.0;
    if (!V.rev) return V.rhs[(long)cn * 6 + t];
    return cn < V.ne ? V.rhs[(long)(V.C - 1 - cn) * 6 + t] : 0.0;
}
// value of lane - n (DPP row_shr:n inside each row of 16 lanes; 0.0 where the row has no such lane)
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false), hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
constexpr int BAND_YB = 28; // doubles per column in ybuf: y_j (6), lower triangle of L_jj^-1 (21), pad
struct BandLds { double *W, *bw, *yj, *Linv, *part; int *pair_d; };
__device__ __forceinline__ BandLds band_lds(double *sh, int Bc) {
    const int NB = Bc + 1, NS = Bc + 2, CS = NB * 36;
    BandLds L;
    L.W = sh; L.bw = L.W + (long)NS * CS; L.yj = L.bw + NS * 6; L.Linv = L.yj + 6; L.part = L.Linv + 6; // part: 64 doubles; the factor of the current diagonal block (36) and the lower triangle of its inverse (21)
    L.pair_d = (int *)(L.part + 64); // pair -> (di << 8 | dk)
    return L;
}
static size_t band_lds_bytes(int Bc) { return sizeof(double) * ((size_t)(Bc + 2) * (Bc + 1) * 36 + (size_t)(Bc + 2) * 6 + 6 + 6 + 64) + sizeof(int) * (size_t)std::max(1, Bc * (Bc + 1) / 2); }

// Eliminates local columns 0..ne-1 (L to Lf, y_j and 1/diag to ybuf), forward solve fused.  LDS: a ring of Bc+2 columns (the extra
// slot receives column j+Bc+1 while column j is processed) and the matching right-hand-side window.  On return the window holds
// the updated tail columns ne..n-1.
typedef double band_v4d __attribute__((ext_vector_type(4)));
template <int NT> __device__ __forceinline__ bool band_factor(const BandView &V, const BandLds &S, double *Lf, double *ybuf) {
    const int Bc = V.Bc, NB = Bc + 1, NS = Bc + 2, CS = NB * 36;
    double *W = S.W, *bw = S.bw, *yj = S.yj;
    int *pair_d = S.pair_d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int pr = tid; pr < Bc * (Bc + 1) / 2; pr += NT) {
        int di = (int)((sqrt(8.0 * pr + 1.0) - 1.0) * 0.5);
        while (di * (di + 1) / 2 > pr) di--;
        while ((di + 1) * (di + 2) / 2 <= pr) di++;
        pair_d[pr] = ((di + 1) << 8) | (pr - di * (di + 1) / 2 + 1);
    }
    const int n0 = V.n < NB ? V.n : NB;
    for (int i = tid; i < n0 * CS; i += NT) W[i] = band_a(V, i / CS, i % CS); // columns 0..n0-1 sit in slots 0..n0-1
    for (int i = tid; i < n0 * 6; i += NT) bw[i] = band_b(V, i / 6, i % 6);
    // prefetch addressing of this thread's (up to four) elements of a column, hoisted out of the chain: element i of local column cn
    // lives at pk[u] + cn * cstep and exists while cn < plim[u]
    long pk[4]; int plim[4];
    const long cstep = V.rev ? -(long)CS : (long)CS;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int i = tid + u * NT, d = i / 36, e = i - d * 36, r = e / 6, c = e - r * 6;
        plim[u] = i < CS ? (V.rev ? min(V.n - d, V.ne) : V.n - d) : 0;
        pk[u] = V.rev ? (long)(V.C - 1 - d) * CS + d * 36 + c * 6 + r : (long)i;
    }
    // trailing update on the matrix cores (Bc <= 10): T -= P P^T with P = the nd*6 x 6 panel, as 16x16 tiles of v_mfma_f64_16x16x4_f64
    // (lower tiles only, K = 6 padded to 8).  Every wave owns up to two tiles; where its operands and results live inside a column
    // of the window does not depend on the column, so it is worked out once: offsets inside the column for the two A and two B
    // operand values, and for the four results (block distance dk of the target column, offset inside it, first panel block di that
    // must exist).  C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg.
    const bool use_mfma = Bc <= 10;
    int ta_off[2], tb_off[2], ta_di[2], tb_di[2], t_dk[2][4], t_in[2][4], t_di[2][4];
    const int k0 = lane >> 4;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int tl = wave >= 1 ? (wave - 1) + q * (NT / 64 - 1) : 99; // wave 0 owns the pivot and its bookkeeping, the other five the ten tiles
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= tl) ti++;
        const int tj = tl - ti * (ti + 1) / 2;
        const bool on = use_mfma && tl < 10;
        const int arow = ti * 16 + (lane & 15), bcol = tj * 16 + (lane & 15);
        ta_off[q] = (1 + arow / 6) * 36 + (arow % 6) * 6 + k0; ta_di[q] = on ? arow / 6 + 1 : 99;
        tb_off[q] = (1 + bcol / 6) * 36 + (bcol % 6) * 6 + k0; tb_di[q] = on ? bcol / 6 + 1 : 99;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int row = ti * 16 + k0 + 4 * g, col = bcol, di = row / 6 + 1, dk = col / 6 + 1;
            t_dk[q][g] = dk * CS; t_in[q][g] = (di - dk) * 36 + (row % 6) * 6 + col % 6; // slot distance in doubles, offset inside the column
            t_di[q][g] = (on && col <= row) ? di : 99; // needs panel block di (and dk <= di)
        }
    }
    const int NSCS = NS * CS;
    const int p_off = (1 + lane / 6) * 36 + (lane % 6) * 6, p_dd = 1 + lane / 6, p_r = lane % 6; // panel row / right-hand-side row of this lane (wave-local index)
    __syncthreads();
#ifdef BAND_PROF
    unsigned long long pt_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, p0_ = 0, p1_;
#define BP(k) do { p1_ = __builtin_readcyclecounter(); pt_[k] += p1_ - p0_; p0_ = p1_; } while (0)
    p0_ = __builtin_readcyclecounter();
#else
#define BP(k) do { } while (0)
#endif
    bool fail = false;
    int sj = 0, sjcs = 0; // j % NS, and times CS
    for (int j = 0; j < V.ne; j++) {
        double *Wc = W + (long)sj * CS;
        const int nd = (V.n - 1 - j) < Bc ? (V.n - 1 - j) : Bc;
        const int cn = j + Bc + 1, scn = sj == 0 ? NS - 1 : sj - 1; // slot of column cn = (j + NS - 1) % NS
        // next column: loads issued now, stored to the free LDS slot at the end of the step (global latency off the critical path)
        double pf[4] = {0, 0, 0, 0}, pfb = 0;
        if (cn < V.n) {
#pragma unroll
            for (int u = 0; u < 4; u++) if (cn < plim[u]) pf[u] = V.A[pk[u] + cn * cstep];
            if (tid < 6) pfb = band_b(V, cn, tid);
        }
        // L_jj = chol(A_jj), its inverse and y_j = L_jj^-1 b_j: every lane of WAVE 0 computes them in its own registers from LDS
        // broadcasts (six v_rsq_f64 + two Newton steps, ~150 fused multiply-adds) and goes straight on to its panel rows, which
        // with the explicit inverse are independent dot products instead of a 16-deep dependent chain -- no cross-lane traffic and no
        // barrier between the pivot and the panel (a shuffle-based version on six lanes cost 0.86 us per column).  The other waves wait.
        BP(0);
        double Lr[6][6], Mi[6][6], invs[6], yv[6];
        if (tid < 64) {
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = 0; c <= r; c++) Lr[r][c] = Wc[r * 6 + c];
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double d = Lr[c][c];
#pragma unroll
                for (int t = 0; t < c; t++) d = __builtin_fma(-Lr[c][t], Lr[c][t], d);
                if (!(d > 0)) { fail = true; d = 1; }
                double inv = __builtin_amdgcn_rsq(d);
                inv = inv * (1.5 - (0.5 * d) * (inv * inv));
                inv = inv * (1.5 - (0.5 * d) * (inv * inv));
                invs[c] = inv;
                Lr[c][c] = d * inv;
#pragma unroll
                for (int r = c + 1; r < 6; r++) {
                    double v = Lr[r][c];
#pragma unroll
                    for (int t = 0; t < c; t++) v = __builtin_fma(-Lr[r][t], Lr[c][t], v);
                    Lr[r][c] = v * inv;
                }
            }
#pragma unroll
            for (int c = 0; c < 6; c++) { // Mi = L_jj^-1 (lower triangular), column by column
                Mi[c][c] = invs[c];
#pragma unroll
                for (int r = c + 1; r < 6; r++) {
                    double v = 0;
#pragma unroll
                    for (int t = c; t < r; t++) v = __builtin_fma(Lr[r][t], Mi[t][c], v);
                    Mi[r][c] = -invs[r] * v;
                }
            }
#pragma unroll
            for (int t = 0; t < 6; t++) { // y = L_jj^-1 b
                double sacc = 0;
#pragma unroll
                for (int u = 0; u <= t; u++) sacc = __builtin_fma(Mi[t][u], bw[sj * 6 + u], sacc);
                yv[t] = sacc;
            }
            BP(1);
            for (int t = tid; t < nd * 6; t += 64) { // L_d = A_d L_jj^-T = A_d Mi^T, one block row per lane
                double *blk = Wc + (t == tid ? p_off : (1 + t / 6) * 36 + (t % 6) * 6);
                double a[6], row[6];
#pragma unroll
                for (int c = 0; c < 6; c++) a[c] = blk[c];
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    double v = 0;
#pragma unroll
                    for (int q = 0; q <= c; q++) v = __builtin_fma(a[q], Mi[c][q], v);
                    row[c] = v;
                }
#pragma unroll
                for (int c = 0; c < 6; c++) blk[c] = row[c];
            }
            if (tid == 0) { // the other waves only need y_j before the barrier
#pragma unroll
                for (int r = 0; r < 6; r++) yj[r] = yv[r];
            }
        }
        BP(2);
        lds_barrier();
        BP(3);
        if (use_mfma) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (ta_di[q] > 20) continue; // this wave has no such tile (uniform over the wave)
                double a0 = 0, a1 = 0, b0 = 0, b1 = 0;
                if (ta_di[q] <= nd) { a0 = -Wc[ta_off[q]]; if (k0 < 2) a1 = -Wc[ta_off[q] + 4]; } // K = 6: k0, k0 + 4 < 6
                if (tb_di[q] <= nd) { b0 = Wc[tb_off[q]]; if (k0 < 2) b1 = Wc[tb_off[q] + 4]; }
                band_v4d acc;
                double *tp[4];
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const unsigned x = (unsigned)(sjcs + t_dk[q][g]);
                    tp[g] = W + (int)(min(x, x - (unsigned)NSCS) + (unsigned)t_in[q][g]); // ((sj + dk) mod NS) * CS + offset, no multiply
                    acc[g] = t_di[q][g] <= nd ? *tp[g] : 0.0;
                }
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; g++) if (t_di[q][g] <= nd) *tp[g] = acc[g];
            }
            if (wave == NT / 64 - 1 && lane < nd * 6) { // b_{j+d} -= L_d y_j
                const double *Ld = Wc + p_off;
                double v = 0;
#pragma unroll
                for (int q = 0; q < 6; q++) v += Ld[q] * yj[q];
                int sl = sj + p_dd; if (sl >= NS) sl -= NS;
                bw[sl * 6 + p_r] -= v;
            }
        } else {
        const int npair = nd * (nd + 1) / 2;
        for (int t = tid; t < npair * 6 + nd * 6; t += NT) {
            if (t < npair * 6) { // row r of block (j+di, j+dk) -= (row r of L_di) L_dk^T: the row of L_di stays in registers
                const int pr = t / 6, r = t % 6, di = pair_d[pr] >> 8, dk = pair_d[pr] & 255;
                const double *Li = Wc + di * 36 + r * 6, *Lk = Wc + dk * 36;
                double a[6];
#pragma unroll
                for (int q = 0; q < 6; q++) a[q] = Li[q];
                int sl = sj + dk; if (sl >= NS) sl -= NS;
                double *T = W + (long)sl * CS + (di - dk) * 36 + r * 6;
                double tv[6];
#pragma unroll
                for (int c = 0; c < 6; c++) tv[c] = T[c];
#pragma unroll
                for (int c = 0; c < 6; c++) { // fused multiply-adds: the solver's round-off is not part of the parity contract
#pragma unroll
                    for (int q = 0; q < 6; q++) tv[c] = __builtin_fma(-a[q], Lk[c * 6 + q], tv[c]);
                }
#pragma unroll
                for (int c = 0; c < 6; c++) T[c] = tv[c];
            } else { // b_{j+d} -= L_d y_j
                const int u = t - npair * 6, d = 1 + u / 6, r = u % 6;
                const double *Ld = Wc + d * 36 + r * 6;
                double v = 0;
#pragma unroll
                for (int q = 0; q < 6; q++) v += Ld[q] * yj[q];
                int sl = sj + d; if (sl >= NS) sl -= NS;
                bw[sl * 6 + r] -= v;
            }
        }
        }
        BP(6);
        for (int i = 36 + tid; i < (nd + 1) * 36; i += NT) Lf[(long)(V.lf_base + j) * CS + i] = Wc[i]; // the panel; the diagonal block comes from wave 0's registers
        if (tid == 0) { // L_jj, y_j and L_jj^-1 (lower, packed) straight from registers to global memory, while the other waves update
            double *Lo = Lf + (long)(V.lf_base + j) * CS, *yo = ybuf + (long)(V.lf_base + j) * BAND_YB; // buffers this kernel has not read before: no stale L1 line possible
#pragma unroll
            for (int r = 0; r < 6; r++) {
                yo[r] = yv[r];
#pragma unroll
                for (int c = 0; c < 6; c++) { Lo[r * 6 + c] = c <= r ? Lr[r][c] : 0.0; if (c <= r) yo[6 + r * (r + 1) / 2 + c] = Mi[r][c]; }
            }
        }
        BP(7);
        if (cn < V.n) {
            double *dst = W + (long)scn * CS;
#pragma unroll
            for (int u = 0; u < 4; u++) if (tid + u * NT < CS) dst[tid + u * NT] = pf[u];
            if (tid < 6) bw[scn * 6 + tid] = pfb;
        }
        BP(4);
        lds_barrier();
        BP(5);
        if (++sj == NS) sj = 0;
        sjcs = sj * CS;
    }
#ifdef BAND_PROF
    if (tid == 0) printf("band_factor side %d cols %d cycles: top %llu pivot %llu panel %llu bar1 %llu mfma %llu store %llu commit %llu bar2 %llu\n", V.rev, V.ne, pt_[0], pt_[1], pt_[2], pt_[3], pt_[6], pt_[7], pt_[4], pt_[5]);
#endif
    return fail;
}

// L^T x = y for the local columns ne-1 .. 0, last first; xtail (may be NULL when n == ne): solved tail blocks in local order.
// The columns of L come back from global memory in chunks of KC columns through two LDS buffers (the whole workgroup loads chunk
// k+1 into registers while chunk k is used, one barrier per chunk); inside a chunk wave 0 works alone, without barriers: lane =
// part * 6 + c sums L_d^T x_{j+d} over the blocks d = 1 + part, 9 + part, 17 + part, shuffles reduce the 8 parts, lanes 0..5
// finish with L_jj^T by lane broadcasts.  Solved blocks: LDS ring xw; xout in original order.
template <int NT> __device__ __forceinline__ void band_back(const BandView &V, const BandLds &S, const double *Lf, const double *ybuf, const double *xtail, int xtail_rev, double *xout) {
    const int Bc = V.Bc, NB = Bc + 1, NS = Bc + 2, CS = NB * 36, C = V.ne;
    double *W = S.W;
    const int tid = threadIdx.x;
    double *xw = S.bw;
    const int R = V.n - V.ne;
    for (int i = tid; i < R * 6; i += NT) { const int t = i / 6; xw[((V.ne + t) % NS) * 6 + i % 6] = xtail[(long)(xtail_rev ? R - 1 - t : t) * 6 + i % 6]; }
    const int KC = (NS - 1) / 2, CB = KC * CS;           // chunk: KC columns of CS doubles; buffers W[0..CB) and W[CB..2CB), >= CS doubles left for ych
    double *ych = W + 2 * (long)CB;                      // 2 x KC x BAND_YB (y_j, L_jj^-1) -- fits: (NS - 2 KC) * CS >= CS >= 56 * KC for Bc >= 1
    const int nchunk = (C + KC - 1) / KC;
    auto chunk_lo = [&](int ch) { return C - (ch + 1) * KC < 0 ? 0 : C - (ch + 1) * KC; }; // chunk ch covers columns [lo, hi)
    auto chunk_hi = [&](int ch) { return C - ch * KC; };
    constexpr int UPF = (9216 + NT - 1) / NT; // doubles per thread per chunk: Bc <= 20 -> CB <= 8316 (checked by the host)
    double pf[UPF], pfy = 0;
    auto issue = [&](int ch) {
        const int lo = chunk_lo(ch), n = (chunk_hi(ch) - lo) * CS;
#pragma unroll
        for (int u = 0; u < UPF; u++) { const int i = tid + u * NT; pf[u] = i < n ? __builtin_nontemporal_load(Lf + (long)(V.lf_base + lo) * CS + i) : 0.0; }
        const int ny = (chunk_hi(ch) - lo) * BAND_YB;
        pfy = tid < ny ? __builtin_nontemporal_load(ybuf + (long)(V.lf_base + lo) * BAND_YB + tid) : 0.0;
    };
    auto commit = [&](int ch) {
        const int lo = chunk_lo(ch), n = (chunk_hi(ch) - lo) * CS;
        double *dst = W + (long)(ch & 1) * CB;
#pragma unroll
        for (int u = 0; u < UPF; u++) { const int i = tid + u * NT; if (i < n) dst[i] = pf[u]; }
        const int ny = (chunk_hi(ch) - lo) * BAND_YB;
        if (tid < ny) ych[(ch & 1) * KC * BAND_YB + tid] = pfy;
    };
    if (nchunk > 0) { issue(0); commit(0); }
    lds_barrier();
    const int c = (tid >> 3) < 6 ? (tid >> 3) : 0, pt = tid & 7; // wave 0: lane = c * 8 + part, lanes 48..63 idle
    const bool work = tid < 48, last = work && pt == 7;           // lane c*8+7 ends up with the sum over the 8 parts
    for (int ch = 0; ch < nchunk; ch++) {
        if (ch + 1 < nchunk) issue(ch + 1);
        if (tid < 64) {
            const int lo = chunk_lo(ch);
            const double *Lb0 = W + (long)(ch & 1) * CB, *yb0 = ych + (ch & 1) * KC * BAND_YB;
            int sj = (chunk_hi(ch) - 1) % NS; // slot of column j in the ring of solved blocks, kept incrementally
            for (int j = chunk_hi(ch) - 1; j >= lo; j--) {
                const int nd = (V.n - 1 - j) < Bc ? (V.n - 1 - j) : Bc;
                const double *Lc = Lb0 + (long)(j - lo) * CS, *yl = yb0 + (j - lo) * BAND_YB;
                // v_c = sum_d (L_d^T x_{j+d})_c: this lane's blocks d = 1 + pt, 9 + pt, 17 + pt, an independent accumulator each
                // (a dependent v_fma_f64 costs 40 cycles), then DPP row shifts over the 8 parts
                double va[3] = {0, 0, 0};
#pragma unroll
                for (int u = 0; u < 3; u++) {
                    const int d = 1 + pt + 8 * u;
                    if (work && d <= nd) {
                        int sl = sj + d; if (sl >= NS) sl -= NS; if (sl >= NS) sl -= NS;
                        const double *Ld = Lc + d * 36 + c, *xd = xw + sl * 6;
#pragma unroll
                        for (int q = 0; q < 6; q++) va[u] = __builtin_fma(Ld[q * 6], xd[q], va[u]);
                    }
                }
                double v = (va[0] + va[1]) + va[2];
                v += dpp_f64<0x114>(v); v += dpp_f64<0x112>(v); v += dpp_f64<0x111>(v);
                // x_j = L_jj^-T (y_j - v) with the explicit inverse from the factorisation: six independent broadcasts and a 3 + 3
                // multiply-add tree per lane instead of a six-step substitution chain
                const double sv = yl[c] - v;
                double s6[6];
#pragma unroll
                for (int k = 0; k < 6; k++) s6[k] = __shfl(sv, k * 8 + 7);
                double e = 0, o = 0;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const double m = k >= c ? yl[6 + k * (k + 1) / 2 + c] : 0.0; // (L^-1)[k][c]
                    if (k & 1) o = __builtin_fma(m, s6[k], o); else e = __builtin_fma(m, s6[k], e);
                }
                const double xv = e + o;
                if (last) { xw[sj * 6 + c] = xv; xout[(long)(V.rev ? V.C - 1 - j : j) * 6 + c] = xv; }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                sj = sj == 0 ? NS - 1 : sj - 1;
            }
        }
        if (ch + 1 < nchunk) commit(ch + 1);
        lds_barrier();
    }
}

constexpr int BAND_NT = 384; // 6 waves: the nd(nd+1)/2 * 6 + nd * 6 = 324 work items of a trailing update (Bc = 9) fit one pass
// one workgroup, whole chain (short systems, or CUBESLAM_BA_SOLVER=band1).  rhs: in b (6C), out x; ybuf: 28C scratch
__global__ void __launch_bounds__(BAND_NT) ba_band_chol(int C, int Bc, const double *A, double *Lf, double *rhs, double *ybuf, int *status) {
    extern __shared__ double sh[];
    const BandLds S = band_lds(sh, Bc);
    const BandView V{A, rhs, C, Bc, C, C, 0, 0};
    const bool fail = band_factor<BAND_NT>(V, S, Lf, ybuf);
    __syncthreads(); // every store to Lf / ybuf has completed
    band_back<BAND_NT>(V, S, Lf, ybuf, nullptr, 0, rhs);
    if (threadIdx.x == 0 && fail) *status = 1;
}
__device__ __forceinline__ BandView band_side(int side, int C, int Bc, const double *A, const double *rhs) { // side 0: columns [0, neF); side 1: the other end
    const int R = Bc, neF = (C - R) / 2, neB = C - R - neF;
    return side == 0 ? BandView{A, rhs, C, Bc, neF + R, neF, 0, 0} : BandView{A, rhs, C, Bc, neB + R, neB, 1, neF};
}
// mid: per side R columns of CS doubles (the updated tail columns, local order) followed by 6R right-hand-side entries
__global__ void __launch_bounds__(BAND_NT) ba_band_twist_factor(int C, int Bc, const double *A, const double *rhs, double *Lf, double *ybuf, double *mid, int *status) {
    extern __shared__ double sh[];
    const BandLds S = band_lds(sh, Bc);
    const BandView V = band_side(blockIdx.x, C, Bc, A, rhs);
    const bool fail = band_factor<BAND_NT>(V, S, Lf, ybuf);
    const int NS = Bc + 2, CS = (Bc + 1) * 36, R = V.n - V.ne;
    double *m = mid + (long)blockIdx.x * ((long)R * CS + R * 6);
    for (int i = threadIdx.x; i < R * CS; i += BAND_NT) m[i] = S.W[(long)((V.ne + i / CS) % NS) * CS + i % CS];
    for (int i = threadIdx.x; i < R * 6; i += BAND_NT) m[(long)R * CS + i] = S.bw[((V.ne + i / 6) % NS) * 6 + i % 6];
    if (threadIdx.x == 0 && fail) *status = 1;
}
// middle group: M = tail(forward) + reversed tail(backward), dense Cholesky in LDS (N = 6R <= 120), two triangular solves.  xm: 6R
__global__ void __launch_bounds__(256) ba_band_mid(int C, int Bc, const double *mid, double *xm, double *xout, int *status) {
    extern __shared__ double sh[];
    const int R = Bc, N = 6 * R, CS = (Bc + 1) * 36, tid = threadIdx.x;
    double *M = sh, *bv = M + (long)N * N;
    const double *m0 = mid, *m1 = mid + ((long)R * CS + R * 6);
    for (int i = tid; i < N * N; i += 256) M[i] = 0;
    __syncthreads();
    for (int i = tid; i < R * R * 36; i += 256) { // forward side: block (t+d, t) as stored
        const int t = i / (R * 36), d = (i / 36) % R, e = i % 36, r = e / 6, c = e % 6;
        if (t + d < R) M[(long)((t + d) * 6 + r) * N + t * 6 + c] = m0[(long)t * CS + d * 36 + e];
    }
    __syncthreads();
    for (int i = tid; i < R * R * 36; i += 256) { // backward side: its block (t+d, t) is the transposed original block (R-1-t, R-1-t-d)
        const int t = i / (R * 36), d = (i / 36) % R, e = i % 36, r = e / 6, c = e % 6;
        if (t + d < R && (d > 0 || r >= c)) { // diagonal blocks: only their lower triangle is maintained by the factor kernels
            const int bb = R - 1 - t, aa = bb - d;
            if (d > 0) M[(long)(bb * 6 + c) * N + aa * 6 + r] += m1[(long)t * CS + d * 36 + e];
            else M[(long)(bb * 6 + r) * N + bb * 6 + c] += m1[(long)t * CS + e];
        }
    }
    for (int i = tid; i < N; i += 256) bv[i] = m0[(long)R * CS + i] + m1[(long)R * CS + (R - 1 - i / 6) * 6 + i % 6];
    __syncthreads();
    __shared__ int s_fail;
    if (tid == 0) s_fail = 0;
    for (int k = 0; k < N; k++) { // right-looking Cholesky, lower triangle
        if (tid == 0) { double d = M[(long)k * N + k]; if (!(d > 0)) { s_fail = 1; d = 1; } M[(long)k * N + k] = sqrt(d); }
        __syncthreads();
        const double dk = M[(long)k * N + k];
        for (int i = k + 1 + tid; i < N; i += 256) M[(long)i * N + k] /= dk;
        __syncthreads();
        const int m = N - 1 - k; // trailing rows k+1..N-1: element (i, j), j <= i
        for (int e = tid; e < m * m; e += 256) { const int i = k + 1 + e / m, j = k + 1 + e % m; if (j <= i) M[(long)i * N + j] = __builtin_fma(-M[(long)i * N + k], M[(long)j * N + k], M[(long)i * N + j]); }
        __syncthreads();
    }
    for (int k = 0; k < N; k++) { // L y = b
        if (tid == 0) bv[k] /= M[(long)k * N + k];
        __syncthreads();
        const double yk = bv[k];
        for (int i = k + 1 + tid; i < N; i += 256) bv[i] = __builtin_fma(-M[(long)i * N + k], yk, bv[i]);
        __syncthreads();
    }
    for (int k = N - 1; k >= 0; k--) { // L^T x = y
        if (tid == 0) bv[k] /= M[(long)k * N + k];
        __syncthreads();
        const double xk = bv[k];
        for (int i = tid; i < k; i += 256) bv[i] = __builtin_fma(-M[(long)k * N + i], xk, bv[i]);
        __syncthreads();
    }
    const int neF = (C - R) / 2;
    for (int i = tid; i < N; i += 256) { xm[i] = bv[i]; xout[(long)neF * 6 + i] = bv[i]; }
    if (tid == 0 && s_fail) *status = 1;
}
__global__ void __launch_bounds__(BAND_NT) ba_band_twist_back(int C, int Bc, const double *Lf, const double *ybuf, const double *xm, double *xout) {
    extern __shared__ double sh[];
    const BandLds S = band_lds(sh, Bc);
    const BandView V = band_side(blockIdx.x, C, Bc, nullptr, nullptr);
    band_back<BAND_NT>(V, S, Lf, ybuf, xm, blockIdx.x, xout);
}
