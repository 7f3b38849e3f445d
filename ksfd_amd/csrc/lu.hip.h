// Dense direct stage solver (pc_type 5): A = shift*I - J(u) assembled from the exported Jacobian entries, blocked right-looking LU with
// partial pivoting (LAPACK getrf semantics), blocked triangular solves that gather b from and scatter x to the ghosted SoA planes.
//
// Unknown order: the device's SoA interior order q = dof*nloc + p.  A is column-major, lda = n, 64-bit element offsets.
// Factorization of column block [k0, k0+nb):
//   per column j of the panel: k_lu_pivot (one block: argmax |a_ij|, lowest index on ties, row interchange inside the panel)
//                              k_lu_panel_col (scale the column below the pivot, rank-1 update of the rest of the panel)
//   k_lu_laswp: the panel's interchanges on every column outside it
//   k_lu_trsm:  U12 = L11^-1 A12
//   k_lu_gemm:  A22 -= L21 U12 on v_mfma_f64_16x16x4_f64 (the flop-bound part)
// A zero or non-finite pivot sets *info = column + 1; every later kernel of the factorization sees it and returns.
#pragma once

#define KSFD_LU_NB 64           // panel width = K of the trailing update = block of the triangular solves
#define KSFD_LU_PIVT 1024       // threads of the pivot search
#define KSFD_LU_ROWS 256        // rows per block of the panel update and of the solve GEMVs

// A -= J entries (k_jac_csr order: per point the rho row, F*npts entries, then NL rows of npts+1), diagonal += shift.  One thread per
// point owns that point's F rows, so no two threads touch the same entry; duplicate columns (periodic extents of 1..4 points) add up.
template <int NL>
__global__ void __launch_bounds__(KSFD_BLOCK) k_lu_scatter(long long nloc, int dim, const long long *__restrict__ col,
                                                           const double *__restrict__ val, double shift, double *__restrict__ A)
{
    constexpr int F = NL + 1;
    const long long n = (long long)F * nloc;
    const int npts = 4 * dim + 1;
    const long long per = (long long)F * npts + (long long)NL * (npts + 1);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < nloc; p += stride) {
        long long e = p * per;
        for (int r = 0; r < F; r++) {
            const long long q = (long long)r * nloc + p;
            const int cnt = r == 0 ? F * npts : npts + 1;
            for (int m = 0; m < cnt; m++, e++) {
                const long long c = col[e];
                const long long pt = c / F, d = c - pt * F;
                A[q + (d * nloc + pt) * n] -= val[e];
            }
            A[q + q * n] += shift;
        }
    }
}

// Pivot of column j (rows j..n-1) and its interchange inside the panel columns [k0, k1).
__global__ void __launch_bounds__(KSFD_LU_PIVT) k_lu_pivot(double *__restrict__ A, long long n, long long j, long long k0, long long k1,
                                                            int *__restrict__ piv, int *__restrict__ info)
{
    __shared__ double sv[KSFD_LU_PIVT / KSFD_WAVE];
    __shared__ int si[KSFD_LU_PIVT / KSFD_WAVE];
    __shared__ int pr;
    if (*info) return;
    const double *a = A + j * n;
    double best = -1.0;
    int bi = (int)n;
    for (long long i = j + threadIdx.x; i < n; i += blockDim.x) {
        const double v = fabs(a[i]);
        if (v > best) { best = v; bi = (int)i; }   // rows ascend per thread: the first maximum stays
    }
    for (int o = KSFD_WAVE / 2; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if ((threadIdx.x & (KSFD_WAVE - 1)) == 0) { sv[threadIdx.x / KSFD_WAVE] = best; si[threadIdx.x / KSFD_WAVE] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < (int)(blockDim.x / KSFD_WAVE); q++)
            if (sv[q] > best || (sv[q] == best && si[q] < bi)) { best = sv[q]; bi = si[q]; }
        // NaN entries never win the comparison; an all-NaN, zero or infinite column ends the factorization
        if (!(best > 0.0) || !isfinite(best) || bi >= n) { *info = (int)j + 1; pr = -1; }
        else { piv[j] = bi; pr = bi; }
    }
    __syncthreads();
    const long long p = pr;
    if (p < 0 || p == j) return;
    for (long long c = k0 + threadIdx.x; c < k1; c += blockDim.x) {
        const double t = A[j + c * n];
        A[j + c * n] = A[p + c * n];
        A[p + c * n] = t;
    }
}

// l_ij = a_ij / a_jj below the pivot, a_ic -= l_ij a_jc for the panel columns right of j
__global__ void __launch_bounds__(KSFD_LU_ROWS) k_lu_panel_col(double *__restrict__ A, long long n, long long j, long long k1,
                                                               const int *__restrict__ info)
{
    if (*info) return;
    const long long i = j + 1 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double l = A[i + j * n] / A[j + j * n];
    A[i + j * n] = l;
    for (long long c = j + 1; c < k1; c++) A[i + c * n] -= l * A[j + c * n];
}

// the interchanges of rows k0..k1-1 on every column outside the panel (one thread per column, in pivot order)
__global__ void __launch_bounds__(KSFD_BLOCK) k_lu_laswp(double *__restrict__ A, long long n, long long k0, long long k1,
                                                         const int *__restrict__ piv, const int *__restrict__ info)
{
    __shared__ int sp[KSFD_LU_NB];
    if (*info) return;
    for (int t = threadIdx.x; t < k1 - k0; t += blockDim.x) sp[t] = piv[k0 + t];
    __syncthreads();
    const long long c0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long c = c0 < k0 ? c0 : c0 + (k1 - k0);
    if (c >= n) return;
    double *a = A + c * n;
    for (long long j = k0; j < k1; j++) {
        const long long p = sp[j - k0];
        if (p != j) { const double t = a[j]; a[j] = a[p]; a[p] = t; }
    }
}

// U12 = L11^-1 A12: one block per 64 columns right of the panel; the tile goes through LDS, one thread per column substitutes
__global__ void __launch_bounds__(KSFD_BLOCK) k_lu_trsm(double *__restrict__ A, long long n, long long k0, const int *__restrict__ info)
{
    constexpr int NB = KSFD_LU_NB;
    __shared__ double T[NB][NB + 1];
    __shared__ double L[NB][NB + 1];
    if (*info) return;
    const long long cb = k0 + NB + (long long)blockIdx.x * NB;
    for (int e = threadIdx.x; e < NB * NB; e += blockDim.x) {
        const int r = e % NB, c = e / NB;
        L[r][c] = A[(k0 + r) + (k0 + c) * n];
        T[r][c] = cb + c < n ? A[(k0 + r) + (cb + c) * n] : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < NB) {
        const int c = threadIdx.x;
        for (int r = 1; r < NB; r++) {
            double s = T[r][c];
            for (int q = 0; q < r; q++) s -= L[r][q] * T[q][c];
            T[r][c] = s;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NB * NB; e += blockDim.x) {
        const int r = e % NB, c = e / NB;
        if (cb + c < n) A[(k0 + r) + (cb + c) * n] = T[r][c];
    }
}

// A22 -= L21 U12 (K = NB).  64x64 tile per block, four waves of 32x32 = 2x2 MFMA tiles.  The product is formed transposed,
// D^T = U12^T L21^T, so that the accumulator's lane index runs along the rows of the column-major A: v_mfma_f64_16x16x4_f64 holds
// A-operand element [row l&15][k l>>4] and B-operand element [k l>>4][col l&15] in lane l, and result register i of lane l is
// D[row (l>>4) + 4i][col l&15] (NOT the f32 16x16x4 map).  Row of D^T = column c of A22, column of D^T = row r of A22.
typedef double ksfd_d4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(KSFD_BLOCK) k_lu_gemm(double *__restrict__ A, long long n, long long k0, int tiles_r,
                                                        const int *__restrict__ info)
{
    constexpr int NB = KSFD_LU_NB;
    __shared__ double Ls[NB][NB + 1];     // Ls[k][r] = L21[r][k]
    __shared__ double Us[NB][NB + 1];     // Us[c][k] = U12[k][c]
    if (*info) return;
    const long long b0 = k0 + NB, m = n - b0;
    const long long r0 = (long long)(blockIdx.x % tiles_r) * NB, c0 = (long long)(blockIdx.x / tiles_r) * NB;
    for (int e = threadIdx.x; e < NB * NB; e += blockDim.x) {
        const int x = e % NB, y = e / NB;
        Ls[y][x] = r0 + x < m ? A[(b0 + r0 + x) + (k0 + y) * n] : 0.0;    // row x, k y
        Us[y][x] = c0 + y < m ? A[(k0 + x) + (b0 + c0 + y) * n] : 0.0;    // k x, column y
    }
    __syncthreads();
    const int lane = threadIdx.x & (KSFD_WAVE - 1), w = threadIdx.x / KSFD_WAVE;
    const int wr = (w & 1) * 32, wc = (w >> 1) * 32;
    const int lr = lane & 15, lk = lane >> 4;
    ksfd_d4 acc[2][2];
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) acc[a][b] = ksfd_d4{ 0.0, 0.0, 0.0, 0.0 };
#pragma unroll 4
    for (int s = 0; s < NB / 4; s++) {
        const int k = 4 * s + lk;
        double ua[2], lb[2];
        for (int cc = 0; cc < 2; cc++) ua[cc] = Us[wc + cc * 16 + lr][k];
        for (int rr = 0; rr < 2; rr++) lb[rr] = Ls[k][wr + rr * 16 + lr];
        for (int cc = 0; cc < 2; cc++)
            for (int rr = 0; rr < 2; rr++) acc[cc][rr] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua[cc], lb[rr], acc[cc][rr], 0, 0, 0);
    }
    for (int cc = 0; cc < 2; cc++)
        for (int rr = 0; rr < 2; rr++) {
            const long long r = r0 + wr + rr * 16 + lr;
            if (r >= m) continue;
            for (int i = 0; i < 4; i++) {
                const long long c = c0 + wc + cc * 16 + lk + 4 * i;
                if (c < m) A[(b0 + r) + (b0 + c) * n] -= acc[cc][rr][i];
            }
        }
}

// ---- triangular solves x = U^-1 L^-1 P b --------------------------------------------------------------------------------------
// Block column kb of L (forward, kb = 0, 1, ...): every block solves the unit-lower diagonal block for z[k0..k0+kw) (block 0 stores
// it), then its rows below: y_i -= sum_c L[i][k0+c] z_c.  first: the right-hand side is gathered from the SoA planes through the
// row permutation (y_i = b[perm[i]]) instead of read from y.  Reads y[k0..k0+kw), writes rows >= k0+kw only: no race.
struct KLUVec {
    long long nloc, plane, ioff;      // SoA: unknown q = dof*nloc + p lives at dof*plane + ioff + p
};
__device__ __forceinline__ long long klu_off(const KLUVec &V, long long q)
{
    const long long d = q / V.nloc;
    return d * V.plane + V.ioff + (q - d * V.nloc);
}

__global__ void __launch_bounds__(KSFD_LU_ROWS) k_lu_fwd(const double *__restrict__ A, long long n, long long k0, int first,
                                                         KLUVec V, const double *__restrict__ b, const int *__restrict__ perm,
                                                         double *__restrict__ y, double *__restrict__ z)
{
    constexpr int NB = KSFD_LU_NB;
    __shared__ double L[NB][NB + 1];
    __shared__ double x[NB];
    const int kw = (int)min((long long)NB, n - k0);
    for (int e = threadIdx.x; e < kw * kw; e += blockDim.x) {
        const int r = e % kw, c = e / kw;
        L[r][c] = A[(k0 + r) + (k0 + c) * n];
    }
    if (threadIdx.x < kw) x[threadIdx.x] = first ? b[klu_off(V, perm[k0 + threadIdx.x])] : y[k0 + threadIdx.x];
    __syncthreads();
    for (int c = 0; c < kw - 1; c++) {
        if ((int)threadIdx.x > c && (int)threadIdx.x < kw) x[threadIdx.x] -= L[threadIdx.x][c] * x[c];
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x < kw) z[k0 + threadIdx.x] = x[threadIdx.x];
    const long long i = k0 + kw + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = first ? b[klu_off(V, perm[i])] : y[i];
    const double *a = A + i + k0 * n;
    for (int c = 0; c < kw; c++) s -= a[(long long)c * n] * x[c];
    y[i] = s;
}

// Block column kb of U (backward, kb = last ... 0): the upper diagonal block solves x[k0..k0+kw) from z (block 0 scatters it into the
// SoA output), then the rows above: z_i -= sum_c U[i][k0+c] x_c.  Reads z[k0..k0+kw), writes rows < k0 only.
__global__ void __launch_bounds__(KSFD_LU_ROWS) k_lu_bwd(const double *__restrict__ A, long long n, long long k0, KLUVec V,
                                                         double *__restrict__ z, double *__restrict__ out)
{
    constexpr int NB = KSFD_LU_NB;
    __shared__ double U[NB][NB + 1];
    __shared__ double x[NB];
    const int kw = (int)min((long long)NB, n - k0);
    for (int e = threadIdx.x; e < kw * kw; e += blockDim.x) {
        const int r = e % kw, c = e / kw;
        U[r][c] = A[(k0 + r) + (k0 + c) * n];
    }
    if (threadIdx.x < kw) x[threadIdx.x] = z[k0 + threadIdx.x];
    __syncthreads();
    for (int c = kw - 1; c >= 0; c--) {
        const double xc = x[c] / U[c][c];
        __syncthreads();
        if ((int)threadIdx.x < c) x[threadIdx.x] -= U[threadIdx.x][c] * xc;
        else if ((int)threadIdx.x == c) x[c] = xc;
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x < kw) out[klu_off(V, k0 + threadIdx.x)] = x[threadIdx.x];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k0) return;
    double s = z[i];
    const double *a = A + i + k0 * n;
    for (int c = 0; c < kw; c++) s -= a[(long long)c * n] * x[c];
    z[i] = s;
}

// ---- exact coarse-level solve of the multigrid V cycle (ksfd_set_mg_coarse kind 1; host side: mgc_setup / mgc_apply in
// lu_host.hip.h) ----------------------------------------------------------------------------------------------------------------
// The coarse matrix has at most KSFD_MG_DIRECT_MAX unknowns, so the per-column launch pairs of the factorization above are pure
// launch latency there.  k_lu_panel factors a whole panel in one launch, k_lu_invert forms the explicit inverse from the factors
// (applied 20 ... 130 times per step as a preconditioner), k_mgc_gemv applies it in one launch inside the cycle.
#define KSFD_LU_PANT 1024       // threads of the panel kernel
#define KSFD_MGC_COLS 16        // identity columns per block of the inversion
#define KSFD_MGC_ROWS 8         // rows per block of the apply (two per wave)

// Columns [k0, k1) of the factorization in ONE workgroup: per column the pivot search (k_lu_pivot's rule: largest |a_ij|, lowest row on
// ties; NaN never wins; zero / non-finite pivot sets *info = column + 1 and ends the kernel), the row interchange inside the panel,
// the scaling below the pivot and the rank-1 update of the panel columns to the right.  The pivot row and the scaled pivot column
// stay in the LDS for the update; the panel itself (at most 2048 x 64 doubles = 1 MB) streams from L2.  n <= KSFD_MG_DIRECT_MAX.
__global__ void __launch_bounds__(KSFD_LU_PANT) k_lu_panel(double *A, long long n, long long k0, long long k1,
                                                           int *__restrict__ piv, int *__restrict__ info)
{
    constexpr int NW = KSFD_LU_PANT / KSFD_WAVE;
    __shared__ double sv[NW];
    __shared__ int si[NW];
    __shared__ int pr;
    __shared__ double prow[KSFD_LU_NB];
    __shared__ double lcol[KSFD_MG_DIRECT_MAX];
    if (*info) return;
    const int t = threadIdx.x;
    const int tr = t & 255, tc = t >> 8;
    for (long long j = k0; j < k1; j++) {
        const double *a = A + j * n;
        double best = -1.0;
        int bi = (int)n;
        for (long long i = j + t; i < n; i += KSFD_LU_PANT) {
            const double v = fabs(a[i]);
            if (v > best) { best = v; bi = (int)i; }   // rows ascend per thread: the first maximum stays
        }
        for (int o = KSFD_WAVE / 2; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if ((t & (KSFD_WAVE - 1)) == 0) { sv[t / KSFD_WAVE] = best; si[t / KSFD_WAVE] = bi; }
        __syncthreads();
        if (t == 0) {
            for (int q = 1; q < NW; q++)
                if (sv[q] > best || (sv[q] == best && si[q] < bi)) { best = sv[q]; bi = si[q]; }
            if (!(best > 0.0) || !isfinite(best) || bi >= n) { *info = (int)j + 1; pr = -1; }
            else { piv[j] = bi; pr = bi; }
        }
        __syncthreads();
        const long long p = pr;
        if (p < 0) return;                              // the whole workgroup reads the same pr
        if (t < k1 - k0) {                              // interchange inside the panel; the pivot row goes to the LDS
            const long long c = k0 + t;
            double vj = A[j + c * n];
            if (p != j) { const double vp = A[p + c * n]; A[j + c * n] = vp; A[p + c * n] = vj; vj = vp; }
            prow[t] = vj;
        }
        __syncthreads();
        const double ajj = prow[j - k0];
        for (long long i = j + 1 + t; i < n; i += KSFD_LU_PANT) {
            const double l = A[i + j * n] / ajj;
            A[i + j * n] = l;
            lcol[i - j - 1] = l;
        }
        __syncthreads();
        // a_ic -= l_i a_jc: 256 row lanes x 4 column lanes, so a narrow remainder of the panel still fills the workgroup
        for (long long i = j + 1 + tr; i < n; i += 256) {
            const double l = lcol[i - j - 1];
            for (long long c = j + 1 + tc; c < k1; c += 4) A[i + c * n] -= l * prow[c - k0];
        }
        __syncthreads();
    }
}

// X = A^-1, ROW-major (X[i*n + c]), from the factors P A = L U (column-major, lda = n) and the interchanges piv.  Each block owns
// KSFD_MGC_COLS columns of the identity and runs both substitutions for them in place in its own columns of X: thread (rl, c) = 16 row
// lanes x 16 columns; block column by block column the 64 x 64 diagonal block is solved in the LDS, then the rows outside it take
// x_i -= sum_q a_iq x_q (the factors come from L2, the block's columns of X are contiguous 128 B per row).
// The right-hand side P e_c is a single one: its row is found by walking column c's index through the interchanges.
__global__ void __launch_bounds__(KSFD_BLOCK) k_lu_invert(const double *__restrict__ A, long long n, const int *__restrict__ piv,
                                                          double *X)
{
    constexpr int NB = KSFD_LU_NB, NC = KSFD_MGC_COLS, NR = KSFD_BLOCK / KSFD_MGC_COLS;
    __shared__ double D[NB][NB + 1];
    __shared__ double xb[NB][NC];
    __shared__ int pos[NC];
    const int t = threadIdx.x, c = t % NC, rl = t / NC;
    const long long col = (long long)blockIdx.x * NC + c;
    const bool live = col < n;
    if (t < NC) {
        long long q = (long long)blockIdx.x * NC + t;
        if (q < n)
            for (long long j = 0; j < n; j++) {
                const long long pj = piv[j];
                if (q == j) q = pj;
                else if (q == pj) q = j;
            }
        pos[t] = (int)q;
    }
    __syncthreads();
    if (live)
        for (long long i = rl; i < n; i += NR) X[i * n + col] = (i == pos[c]) ? 1.0 : 0.0;
    __syncthreads();
    const long long nbk = (n + NB - 1) / NB;
    // L y = P e_c (unit lower)
    for (long long kb = 0; kb < nbk; kb++) {
        const long long k0 = kb * NB;
        const int kw = (int)min((long long)NB, n - k0);
        for (int e = t; e < kw * kw; e += KSFD_BLOCK) {
            const int r = e % kw, q = e / kw;
            D[r][q] = A[(k0 + r) + (k0 + q) * n];
        }
        for (int q = rl; q < kw; q += NR) xb[q][c] = live ? X[(k0 + q) * n + col] : 0.0;
        __syncthreads();
        for (int q = 0; q < kw - 1; q++) {
            const double xq = xb[q][c];
            for (int r = q + 1 + rl; r < kw; r += NR) xb[r][c] -= D[r][q] * xq;
            __syncthreads();
        }
        if (live) {
            for (int q = rl; q < kw; q += NR) X[(k0 + q) * n + col] = xb[q][c];
            for (long long i = k0 + kw + rl; i < n; i += NR) {
                double s = X[i * n + col];
                const double *a = A + i + k0 * n;
                for (int q = 0; q < kw; q++) s -= a[(long long)q * n] * xb[q][c];
                X[i * n + col] = s;
            }
        }
        __syncthreads();
    }
    // U x = y
    for (long long kb = nbk - 1; kb >= 0; kb--) {
        const long long k0 = kb * NB;
        const int kw = (int)min((long long)NB, n - k0);
        for (int e = t; e < kw * kw; e += KSFD_BLOCK) {
            const int r = e % kw, q = e / kw;
            D[r][q] = A[(k0 + r) + (k0 + q) * n];
        }
        for (int q = rl; q < kw; q += NR) xb[q][c] = live ? X[(k0 + q) * n + col] : 0.0;
        __syncthreads();
        for (int q = kw - 1; q >= 0; q--) {
            if (rl == 0) xb[q][c] /= D[q][q];
            __syncthreads();
            const double xq = xb[q][c];
            for (int r = rl; r < q; r += NR) xb[r][c] -= D[r][q] * xq;
            __syncthreads();
        }
        if (live) {
            for (int q = rl; q < kw; q += NR) X[(k0 + q) * n + col] = xb[q][c];
            for (long long i = rl; i < k0; i += NR) {
                double s = X[i * n + col];
                const double *a = A + i + k0 * n;
                for (int q = 0; q < kw; q++) s -= a[(long long)q * n] * xb[q][c];
                X[i * n + col] = s;
            }
        }
        __syncthreads();
    }
}

// x = X b with the row-major inverse X of k_lu_invert: b is gathered from, x scattered to the level's ghosted SoA planes (KLUVec).  The
// right-hand side goes through the LDS once per block; one wave per row reads it coalesced, every lane sums its columns in ascending
// order and a butterfly of fixed shape adds the 64 partial sums: no atomics, the same bits on every run.  n <= KSFD_MG_DIRECT_MAX.
__global__ void __launch_bounds__(KSFD_BLOCK) k_mgc_gemv(const double *__restrict__ X, int n, KLUVec V, const double *__restrict__ b,
                                                         double *__restrict__ x)
{
    __shared__ double bs[KSFD_MG_DIRECT_MAX];
    for (int q = threadIdx.x; q < n; q += KSFD_BLOCK) bs[q] = b[klu_off(V, q)];
    __syncthreads();
    const int lane = threadIdx.x & (KSFD_WAVE - 1), w = threadIdx.x / KSFD_WAVE;
    constexpr int per_wave = KSFD_MGC_ROWS / (KSFD_BLOCK / KSFD_WAVE);
    for (int rr = 0; rr < per_wave; rr++) {
        const int i = blockIdx.x * KSFD_MGC_ROWS + w * per_wave + rr;
        if (i >= n) break;                              // the same for the whole wave
        const double *a = X + (long long)i * n;
        double s = 0.0;
        for (int q = lane; q < n; q += KSFD_WAVE) s += a[q] * bs[q];
        for (int o = KSFD_WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) x[klu_off(V, i)] = s;
    }
}
