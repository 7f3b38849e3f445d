// Banded direct stage solver for 1-D grids (pc_type 6): A = shift*I - J(u) in the folded unknown order of banded_plan.h is banded with
// kl = ku = 5F - 1; it is assembled into LAPACK band storage, factored P A = L U as dgbtf2 does (partial pivoting inside the band, the
// multipliers of a column stored unpermuted below its diagonal, U with kl rows of fill-in above) and solved as dgbtrs does.
//
// Elimination is sequential in the columns, so both kernels are ONE workgroup and are bound by the dependent LDS round trips of a
// column, not by flops or bandwidth.
//
// k_band_factor.  The live window of step j -- rows j .. j+kl, columns j .. j+kl+ku -- lives in the LDS as a ring in both directions
// (row r at r mod (kl+2), column c at c mod (kl+ku+2)); nothing of it is in global memory between steps.  Per column:
//   A  every thread reads the kl+1 pivot candidates itself (broadcast reads, no cross-lane reduction): first of largest modulus
//   B  the pivot row goes to a staging row (and to HBM: it is row j of U), the old row j takes its place in the ring; the multipliers
//      l_i = a_ij / pivot go to a staging column (and to HBM)                                                    -- barrier
//   C  rank-1 update of the kl x (kl+ku) rest of the window from the staging row and column; the row and the column that enter the
//      window of step j+1 are written into the ring slots that row j-1 and column j-1 left.  The entering row is untouched matrix
//      data, so it is loaded into registers two steps ahead; the entering column is fill-in space, zeros                -- barrier
// With one wave the barriers are waits for the LDS only.
//
// k_band_solve.  The forward sweep applies the interchanges as it goes, the backward sweep runs over the U band of width kl+ku; the
// right-hand side is read and the solution written in the handle's SoA layout through the fold map.  Live entries of the vector are
// a ring in the LDS; the column of L or U, the pivot index and the entering entry are loaded KSFD_BAND_AHEAD columns ahead.
#pragma once
#include "banded_plan.h"

#define KSFD_BAND_AHEAD 4           // columns the solve sweeps load ahead (registers, rotated by unrolling)
#define KSFD_BAND_SOLVE_T 64        // threads of the solve kernel: one wave
#define KSFD_BAND_YRING 256         // ring of the solve vectors (>= kl + ku + 2 = 130 at F = 13)
#define KSFD_BAND_FMAX 13           // widest block the index arithmetic below is sized for (KSFD_MAXL + 1)

struct KBandVec {
    long long plane, ioff;          // SoA: unknown (p, dof) lives at dof*plane + ioff + p
};

// doubles of LDS the factorization needs: the ring (odd row stride) and the two staging vectors
KSFD_BAND_HD int band_ring_stride(const BandPlan &B) { return (B.kl + B.ku + 2) | 1; }
KSFD_BAND_HD long long band_factor_lds(const BandPlan &B) { return (long long)(B.kl + 2) * band_ring_stride(B) + (B.kl + B.ku + 1) + (B.kl + 1); }

// AB -= J entries (k_jac_csr order), diagonal += shift; AB zeroed before.  One thread per point owns that point's F rows, and distinct
// (row, column) pairs have distinct slots, so no two threads touch the same entry.  An entry outside the band (never, by the fold) is
// not written and sets *info = -1.
template <int NL>
__global__ void __launch_bounds__(KSFD_BLOCK) k_band_scatter(BandPlan B, const long long *__restrict__ col, const double *__restrict__ val,
                                                             double shift, double *__restrict__ AB, int *__restrict__ info)
{
    constexpr int F = NL + 1;
    constexpr int npts = 5;
    constexpr long long per = (long long)F * npts + (long long)NL * (npts + 1);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < B.N; p += stride) {
        long long e = p * per;
        for (int r = 0; r < F; r++) {
            const long long i = band_unknown(B, p, r);
            const int cnt = r == 0 ? F * npts : npts + 1;
            for (int m = 0; m < cnt; m++, e++) {
                const long long c = col[e];
                const long long pt = c / F;
                const long long j = band_unknown(B, pt, (int)(c - pt * F));
                if (pt >= 0 && pt < B.N && band_inside(B, i, j)) AB[band_slot(B, i, j)] -= val[e];
                else *info = -1;
            }
            AB[band_slot(B, i, i)] += shift;
        }
    }
}

template <int NT>
__global__ void __launch_bounds__(NT) k_band_factor(BandPlan B, double *__restrict__ AB, int *__restrict__ ipiv, int *__restrict__ info)
{
    extern __shared__ double band_lds[];
    constexpr int PF = (10 * KSFD_BAND_FMAX - 1 + NT - 1) / NT;      // entering-row entries per thread (kl + ku + 1 <= 129)
    const int kl = B.kl, kv = B.kl + B.ku;
    const int R = kl + 2, C = kv + 2, Cs = band_ring_stride(B);
    double *W = band_lds;
    double *stg = W + R * Cs;                  // stg[t] = u_{j, j+t} (t = 0 .. kv), stg[kv + i] = l_{j+i, j} (i = 1 .. kl)
    const int n = (int)B.n;
    const int tid = threadIdx.x;
    if (*info) return;

    for (int e = tid; e < (kl + 1) * (kv + 1); e += NT) {
        const int r = e / (kv + 1), c = e - r * (kv + 1);
        if (r < n && c < n) W[r * Cs + c] = AB[band_slot(B, r, c)];
    }
    // entries tid + q*NT of the row that enters after step j: (j + kl + 1, j + 1 + idx)
    auto load_row = [&](int j, double (&v)[PF]) {
        const int re = j + kl + 1;
#pragma unroll
        for (int q = 0; q < PF; q++) {
            const int idx = tid + q * NT, c = j + 1 + idx;
            v[q] = (idx <= kv && re < n && c < n) ? AB[band_slot(B, re, c)] : 0.0;
        }
    };
    // this thread's first element of the rank-1 update and its stride through the kl x kv block
    const int e_i0 = 1 + tid / kv, e_t0 = 1 + tid % kv, e_di = NT / kv, e_dt = NT % kv;
    int jr = 0, jc = 0;                         // j mod R, j mod C
    bool dead = false;

    auto step = [&](int j, double (&pf)[PF]) {
        const int km = min(kl, n - 1 - j);
        // A: pivot
        double best = -1.0, piv = 0.0;
        int bi = 0;
        for (int i = 0; i <= km; i++) {
            int rr = jr + i; if (rr >= R) rr -= R;
            const double v = W[rr * Cs + jc], a = fabs(v);
            if (a > best) { best = a; bi = i; piv = v; }           // NaN never wins; the first maximum stays
        }
        if (!(best > 0.0) || !isfinite(best)) {
            if (tid == 0) *info = j + 1;
            dead = true;
            return;
        }
        if (tid == 0) ipiv[j] = j + bi;
        const double rinv = 1.0 / piv;
        int pr = jr + bi; if (pr >= R) pr -= R;
        // B: row j of U and column j of L leave the window
        for (int idx = tid; idx <= kv + km; idx += NT) {
            if (idx <= kv) {
                const int c = j + idx;
                if (c < n) {
                    int cc = jc + idx; if (cc >= C) cc -= C;
                    const double u = W[pr * Cs + cc];
                    if (bi != 0 && idx > 0) W[pr * Cs + cc] = W[jr * Cs + cc];
                    stg[idx] = u;
                    AB[band_slot(B, j, c)] = u;
                }
            } else {
                const int i = idx - kv;
                int rr = jr + i; if (rr >= R) rr -= R;
                const double l = (i == bi ? W[jr * Cs + jc] : W[rr * Cs + jc]) * rinv;
                stg[idx] = l;
                AB[band_slot(B, j + i, j)] = l;
            }
        }
        __syncthreads();
        // C: rank-1 update
        for (int i = e_i0, t = e_t0; i <= km;) {
            if (j + t < n) {
                int rr = jr + i; if (rr >= R) rr -= R;
                int cc = jc + t; if (cc >= C) cc -= C;
                W[rr * Cs + cc] -= stg[kv + i] * stg[t];
            }
            t += e_dt; i += e_di;
            if (t > kv) { t -= kv; i++; }
        }
        // what enters for step j + 1: row j+kl+1 (columns j+1 .. j+kv+1) and, above it, the zeros of column j+kv+1
        {
            const int re = j + kl + 1, ce = j + kv + 1;
            const int rre = jr == 0 ? R - 1 : jr - 1, cce = jc == 0 ? C - 1 : jc - 1;
#pragma unroll
            for (int q = 0; q < PF; q++) {
                const int idx = tid + q * NT;
                if (idx <= kv && re < n && j + 1 + idx < n) {
                    int cc = jc + 1 + idx; if (cc >= C) cc -= C;
                    W[rre * Cs + cc] = pf[q];
                }
            }
            if (ce < n)
                for (int i = 1 + tid; i <= kl; i += NT) {
                    int rr = jr + i; if (rr >= R) rr -= R;
                    W[rr * Cs + cce] = 0.0;
                }
        }
        load_row(j + 2, pf);
        __syncthreads();
        if (++jr == R) jr = 0;
        if (++jc == C) jc = 0;
    };

    double pf0[PF], pf1[PF];
    load_row(0, pf0);
    load_row(1, pf1);
    __syncthreads();
    for (int j = 0; j < n && !dead; j += 2) {
        step(j, pf0);
        if (j + 1 < n && !dead) step(j + 1, pf1);
    }
}

// x = U^-1 L^-1 P b
__global__ void __launch_bounds__(KSFD_BAND_SOLVE_T) k_band_solve(BandPlan B, const double *__restrict__ AB, const int *__restrict__ ipiv,
                                                                  KBandVec V, const double *__restrict__ b, double *__restrict__ zw,
                                                                  double *__restrict__ x)
{
    constexpr int NT = KSFD_BAND_SOLVE_T, M = KSFD_BAND_YRING - 1, D = KSFD_BAND_AHEAD;
    constexpr int UQ = (10 * KSFD_BAND_FMAX - 2 + NT - 1) / NT;      // entries of a U column above the diagonal per thread (kl + ku <= 128)
    constexpr int LQ = (5 * KSFD_BAND_FMAX - 1 + NT - 1) / NT;       // multipliers of an L column per thread (kl <= 64)
    __shared__ double y[KSFD_BAND_YRING];
    const int kl = B.kl, kv = B.kl + B.ku, F = B.F;
    const int n = (int)B.n;
    const int tid = threadIdx.x;
    auto vec = [&](int pos, int dof) { return (long long)dof * V.plane + V.ioff + band_point(B.N, pos); };

    // ---- forward: y <- L^-1 P b, z_j to zw ----
    struct FwdPF { double l[LQ]; double bnew; int piv; };
    int ep = (kl + 1) / F, ed = (kl + 1) % F;              // (position, dof) of the entry the next load brings in: unknown jn + kl + 1
    auto load_fwd = [&](int jn, FwdPF &p) {
        p.piv = jn < n ? ipiv[jn] : jn;
#pragma unroll
        for (int q = 0; q < LQ; q++) {
            const int i = 1 + tid + q * NT;
            p.l[q] = (i <= kl && jn + i < n) ? AB[band_slot(B, jn + i, jn)] : 0.0;
        }
        p.bnew = jn + kl + 1 < n ? b[vec(ep, ed)] : 0.0;
        if (++ed == F) { ed = 0; ep++; }
    };
    for (int q = tid; q <= kl && q < n; q += NT) y[q] = b[vec(q / F, q % F)];
    auto fwd = [&](int j, FwdPF &p) {
        const double bj = y[j & M], bp = y[p.piv & M];
        double v[LQ];
#pragma unroll
        for (int q = 0; q < LQ; q++) {
            const int r = j + 1 + tid + q * NT;
            v[q] = (r == p.piv ? bj : y[r & M]) - bp * p.l[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < LQ; q++) {
            const int i = 1 + tid + q * NT;
            if (i <= kl && j + i < n) y[(j + i) & M] = v[q];
        }
        if (tid == 0) {
            zw[j] = bp;
            if (j + kl + 1 < n) y[(j + kl + 1) & M] = p.bnew;
        }
        load_fwd(j + D, p);
        __syncthreads();
    };
    {
        FwdPF p[D];
#pragma unroll
        for (int d = 0; d < D; d++) load_fwd(d, p[d]);
        __syncthreads();
        for (int j = 0; j < n; j += D) {
#pragma unroll
            for (int d = 0; d < D; d++) if (j + d < n) fwd(j + d, p[d]);
        }
    }
    __threadfence();
    __syncthreads();

    // ---- backward: x <- U^-1 z ----
    struct BwdPF { double u[UQ]; double ujj, znew; };
    auto load_bwd = [&](int jn, BwdPF &p) {
#pragma unroll
        for (int q = 0; q < UQ; q++) {
            const int idx = tid + q * NT, i = jn - 1 - idx;
            p.u[q] = (jn >= 0 && idx < kv && i >= 0) ? AB[band_slot(B, i, jn)] : 0.0;
        }
        p.ujj = jn >= 0 ? AB[band_slot(B, jn, jn)] : 1.0;
        p.znew = jn - kv - 1 >= 0 ? zw[jn - kv - 1] : 0.0;
    };
    for (int q = tid; q <= kv && q < n; q += NT) y[(n - 1 - q) & M] = zw[n - 1 - q];
    int op = (n - 1) / F, od = (n - 1) % F;                 // (position, dof) of unknown j
    auto bwd = [&](int j, BwdPF &p) {
        const double xj = y[j & M] / p.ujj;
        double v[UQ];
#pragma unroll
        for (int q = 0; q < UQ; q++) {
            const int i = j - 1 - (tid + q * NT);
            v[q] = y[i & M] - xj * p.u[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < UQ; q++) {
            const int idx = tid + q * NT, i = j - 1 - idx;
            if (idx < kv && i >= 0) y[i & M] = v[q];
        }
        if (tid == 0) {
            x[vec(op, od)] = xj;
            if (j - kv - 1 >= 0) y[(j - kv - 1) & M] = p.znew;
        }
        if (--od < 0) { od = F - 1; op--; }
        load_bwd(j - D, p);
        __syncthreads();
    };
    {
        BwdPF p[D];
#pragma unroll
        for (int d = 0; d < D; d++) load_bwd(n - 1 - d, p[d]);
        __syncthreads();
        for (int j = n - 1; j >= 0; j -= D) {
#pragma unroll
            for (int d = 0; d < D; d++) if (j - d >= 0) bwd(j - d, p[d]);
        }
    }
}
