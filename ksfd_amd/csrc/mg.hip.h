// Geometric multigrid preconditioner for the stage systems (shift*I - J) y = b of the Rosenbrock-W step.
//
// Stands in for what `-pc_type lu -pc_factor_mat_solver_type mumps` (options84:58-60) gives the reference:
// a solve whose cost does not blow up when h*gamma*lambda_max(J) >> 1 (late-time steps h ~ 1..1e4).
// Matrix-free and rediscretised: level l uses the SAME analytic Jacobian-action kernels with the frozen
// coefficient planes [rho, G, G_rho, G_U] full-weighted onto a grid of spacing 2^l h.  Smoother: Chebyshev
// iteration preconditioned by the inverse of the point-block (F x F) diagonal of A_l.  Vertex-centred full
// coarsening on the periodic box, full-weighting restriction, bilinear prolongation, V(nu,nu) cycle, fixed
// polynomial smoothing on the coarsest grid -- every piece is a fixed linear operator, so plain
// right-preconditioned GMRES applies.  1-D, 2-D and 3-D, single rank or slab ranks.
// Slab ranks: every level is distributed like level 0 (ghost units, halo exchange) down to the last level on which a rank keeps >= 4
// slow units; ksfd_set_mg_agglomerate (opt-in, 2-D and 3-D) continues below it with REPLICATED levels that every rank holds whole and
// computes redundantly with wrapped indices.  What the one all-reduce per cycle costs between devices against the halo exchanges it
// saves has not been measured.
// Transfers: ONE restriction kernel and ONE prolongation kernel (k_mg_restrict, k_mg_prolong_add) for every dimension, storage type and
// placement; one rank, slab ranks and the border to the replicated levels differ in the slow-axis descriptor KMGSlow (and the border
// is an instance of its own, BORDER, of the same text).
#pragma once
#include "stencil.hip.h"

// The slow axis of a transfer between a fine level and the next coarser one (x in 1-D, y in 2-D, z in 3-D; a slow unit is a point, a row
// or a plane).  The inner axes are periodic and whole on every rank; the slow axis is this rank's slab, and how it is indexed is all
// that distinguishes one rank from slab ranks from the border below a replicated level: mg_host.hip.h (mg_slow) fills this in.
struct KMGSlow {
    long long nf;    // fine slow units this rank holds
    long long u0;    // restriction: first coarse slow unit of this rank's part inside the coarse array
                     // prolongation: first (global) fine slow unit of this rank's slab; 0 except across the border
    long long nc;    // slow extent of the coarse ARRAY: nf/2, or the global coarse extent across the border
    int wrap;        // slow neighbours wrap (one rank, replicated level) or are ghost units (slab ranks: the halo must be current)
};

// Full weighting: coarse(I,J,K) = sum_{a,b,d in -1..1} w_a w_b w_d fine(2I+d, 2J+b, 2K+a), w = (1/4, 1/2, 1/4), over the DIM axes the
// grid has.  The slow neighbours wrap or are the ghost units at local index -1 / nf (the slab must start on an even global unit).
// foff/coff = offset of local slow unit 0 inside a field plane (ng*inner).  TF / TK: storage type of the fine / coarse vector (the V
// cycle runs its level vectors in fp32 when the solve tolerance allows: mg_host.hip.h); the arithmetic is fp64.
// Across the border between the last distributed level (fine: this rank's slab with its ghost units) and the first replicated one
// (coarse: the WHOLE level on every rank, no ghost units; ksfd_set_mg_agglomerate) the kernel runs over the whole coarse array: the rank
// full-weights its own units into its part [u0, u0 + nf/2) and writes zeros everywhere else, so that the sum over the ranks (the
// transport's all-reduce; adding zeros is exact) is the gathered coarse vector, the same bits on every rank.  There the slow
// neighbours never wrap.  Everywhere else u0 = 0 and nc = nf/2: every coarse unit is the rank's own.
// BORDER: the same text compiled for the border alone, so that the launches of every other level pair carry neither the ownership test
// nor the offset (one trace had them 1-2 us slower on 4096^2 with both folded into one instance: profiles/mg_transfer_refactor.log)
template <int DIM, bool BORDER, typename TF, typename TK>
__global__ void __launch_bounds__(KSFD_BLOCK) k_mg_restrict(int nplanes, long long nxf, long long nyf, KMGSlow Z,
                                                            const TF *__restrict__ fine, long long fplane, long long foff,
                                                            TK *__restrict__ coarse, long long cplane, long long coff)
{
    const long long nxc = DIM > 1 ? nxf >> 1 : 1, nyc = DIM > 2 ? nyf >> 1 : 1, nsc = Z.nf >> 1, n = nxc * nyc * Z.nc;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const long long I = p % nxc, J = (p / nxc) % nyc, S = p / (nxc * nyc) - (BORDER ? Z.u0 : 0);
        const bool own = !BORDER || (S >= 0 && S < nsc), wrap = !BORDER && Z.wrap;
        long long xi[3], yj[3], zk[3];                          // fine indices -1, 0, +1 around (2I, 2J, 2S); the slow one is zk
        xi[1] = 2 * I; xi[0] = (xi[1] + nxf - 1) % nxf; xi[2] = (xi[1] + 1) % nxf;
        yj[1] = 2 * J; yj[0] = (yj[1] + nyf - 1) % nyf; yj[2] = (yj[1] + 1) % nyf;
        zk[1] = 2 * S; zk[0] = wrap ? (zk[1] + Z.nf - 1) % Z.nf : zk[1] - 1; zk[2] = wrap ? (zk[1] + 1) % Z.nf : zk[1] + 1;
        for (int c = 0; c < nplanes; c++) {
            double s = 0.0;
            if (own) {
                const TF *f = fine + (long long)c * fplane + foff;
                if constexpr (DIM == 1) {
                    s = 0.5 * (double)f[zk[1]] + 0.25 * ((double)f[zk[0]] + (double)f[zk[2]]);
                } else if constexpr (DIM == 2) {
                    const long long im = xi[0], i0 = xi[1], ip = xi[2], jm = zk[0], j0 = zk[1], jp = zk[2];
                    s = 0.25 * (double)f[i0 + nxf * j0] +
                        0.125 * ((double)f[im + nxf * j0] + (double)f[ip + nxf * j0] + (double)f[i0 + nxf * jm] + (double)f[i0 + nxf * jp]) +
                        0.0625 * ((double)f[im + nxf * jm] + (double)f[ip + nxf * jm] + (double)f[im + nxf * jp] + (double)f[ip + nxf * jp]);
                } else {
                    const double w[3] = { 0.25, 0.5, 0.25 };
#pragma unroll
                    for (int a = 0; a < 3; a++)
#pragma unroll
                        for (int b = 0; b < 3; b++)
#pragma unroll
                            for (int d = 0; d < 3; d++) s += w[a] * w[b] * w[d] * (double)f[xi[d] + nxf * (yj[b] + nyf * zk[a])];
                }
            }
            coarse[(long long)c * cplane + coff + p] = (TK)s;
        }
    }
}

// fine += P coarse: linear interpolation along each of the DIM axes.  k = the global fine slow unit (u0 is the slab's first one across
// the border, where the whole coarse array is indexed with wrapped global units; 0 otherwise); the coarse neighbour K + 1 of an odd
// unit wraps modulo nc or is the coarse ghost unit nc (slab ranks: the coarse halo must be current).
template <int DIM, bool BORDER, typename TK, typename TF>
__global__ void __launch_bounds__(KSFD_BLOCK) k_mg_prolong_add(int nplanes, long long nxf, long long nyf, KMGSlow Z,
                                                               const TK *__restrict__ coarse, long long cplane, long long coff,
                                                               TF *__restrict__ fine, long long fplane, long long foff)
{
    const long long nxc = DIM > 1 ? nxf >> 1 : 1, nyc = DIM > 2 ? nyf >> 1 : 1;
    const long long nxi = DIM > 1 ? nxf : 1, nyi = DIM > 2 ? nyf : 1, n = nxi * nyi * Z.nf;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const long long i = p % nxi, j = (p / nxi) % nyi, k = (BORDER ? Z.u0 : 0) + p / (nxi * nyi);
        const long long I = i >> 1, J = j >> 1, K = k >> 1;
        const long long I1 = (i & 1) ? (I + 1) % nxc : I, J1 = (j & 1) ? (J + 1) % nyc : J;
        const long long K1 = (k & 1) ? ((BORDER || Z.wrap) ? (K + 1) % Z.nc : K + 1) : K;
        for (int c = 0; c < nplanes; c++) {
            const TK *q = coarse + (long long)c * cplane + coff;
            const long long o = (long long)c * fplane + foff + p;
            if constexpr (DIM == 1) {
                fine[o] = (TF)((double)fine[o] + 0.5 * ((double)q[K] + (double)q[K1]));
            } else if constexpr (DIM == 2) {
                const double v = 0.25 * ((double)q[I + nxc * K] + (double)q[I1 + nxc * K] + (double)q[I + nxc * K1] + (double)q[I1 + nxc * K1]);
                fine[o] = (TF)((double)fine[o] + v);
            } else {
                const double v = 0.125 * ((double)q[I + nxc * (J + nyc * K)] + (double)q[I1 + nxc * (J + nyc * K)] + (double)q[I + nxc * (J1 + nyc * K)] +
                                          (double)q[I1 + nxc * (J1 + nyc * K)] + (double)q[I + nxc * (J + nyc * K1)] + (double)q[I1 + nxc * (J + nyc * K1)] +
                                          (double)q[I + nxc * (J1 + nyc * K1)] + (double)q[I1 + nxc * (J1 + nyc * K1)]);
                fine[o] = (TF)((double)fine[o] + v);
            }
        }
    }
}

// Inverse of the point-block diagonal of A = shift*I - J (F x F per point, row-major planes dinv[(r*F+c)*plane], stored in
// fp32: it only scales the smoother of a preconditioner, and it is read three times per smoothing sweep):
//   D_rr = shift - (lapG + rho*G_rho*c2),  D_rUl = -rho*G_Ul*c2,  D_Ulr = -s_l,  D_UlUl = shift + gamma_l - D_l*c2
// with c2 = sum_a (-30/12)/h_a^2 the centre weight of the 4th-order Laplacian.
template <int NL>
__global__ void __launch_bounds__(KSFD_BLOCK) k_blockdiag_inv(KGeom G, KPhys P, const double *__restrict__ C, double shift,
                                                              float *__restrict__ dinv)
{
    constexpr int F = NL + 1;
    const double *Gb = C + G.plane;
    double c2 = 0.0;
    for (int a = 0; a < G.dim; a++) c2 += -2.5 * P.inv_h2[a];
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < G.nloc; p += stride) {
        long long i, j, k;
        ksfd_decode(G, p, i, j, k);
        double lapG = 0.0;
        for (int a = 0; a < G.dim; a++) {
            KNbr n = ksfd_nbr(G, a, i, j, k);
            lapG += KSFD_D2(Gb[n.m2], Gb[n.m1], Gb[n.c], Gb[n.p1], Gb[n.p2]) * P.inv_h2[a];
        }
        const long long o = (long long)G.ng * G.inner + p;       // owned point inside a (ghosted) plane
        const double rho = C[o], gr = C[2 * G.plane + o];
        double M[F][F], Inv[F][F];
#pragma unroll
        for (int r = 0; r < F; r++)
#pragma unroll
            for (int c = 0; c < F; c++) { M[r][c] = 0.0; Inv[r][c] = (r == c) ? 1.0 : 0.0; }
        M[0][0] = shift - (lapG + rho * gr * c2);
#pragma unroll
        for (int l = 0; l < NL; l++) {
            M[0][l + 1] = -rho * C[(long long)(3 + l) * G.plane + o] * c2;
            M[l + 1][0] = -P.lig_s[l];
            M[l + 1][l + 1] = shift + P.lig_gamma[l] - P.lig_D[l] * c2;
        }
        // Gauss-Jordan without pivoting (the blocks are strongly diagonally dominated by shift + diffusion)
#pragma unroll
        for (int q = 0; q < F; q++) {
            const double ip = 1.0 / M[q][q];
#pragma unroll
            for (int c = 0; c < F; c++) { M[q][c] *= ip; Inv[q][c] *= ip; }
#pragma unroll
            for (int r = 0; r < F; r++) {
                if (r == q) continue;
                const double f = M[r][q];
#pragma unroll
                for (int c = 0; c < F; c++) { M[r][c] -= f * M[q][c]; Inv[r][c] -= f * Inv[q][c]; }
            }
        }
#pragma unroll
        for (int r = 0; r < F; r++)
#pragma unroll
            for (int c = 0; c < F; c++) dinv[(long long)(r * F + c) * G.plane + o] = (float)Inv[r][c];
    }
}

// z = scale * Dinv r   (and z2 = the same values when z2 != NULL: first Chebyshev sweep from a zero guess, x = d)
// rcopy != NULL: r itself, in the storage type of z (entry of an fp32 V cycle: the fp64 right-hand side is read once)
template <int NL, typename TR = double, typename TZ = double>
__global__ void __launch_bounds__(KSFD_BLOCK) k_dinv_apply(long long n, long long plane, const float *__restrict__ dinv,
                                                           const TR *__restrict__ r, double scale, TZ *__restrict__ z,
                                                           TZ *__restrict__ z2 = nullptr, TZ *__restrict__ rcopy = nullptr)
{
    constexpr int F = NL + 1;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        double rv[F];
#pragma unroll
        for (int c = 0; c < F; c++) {
            rv[c] = (double)r[(long long)c * plane + p];
            if (rcopy) rcopy[(long long)c * plane + p] = (TZ)rv[c];
        }
#pragma unroll
        for (int a = 0; a < F; a++) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < F; c++) s += dinv[(long long)(a * F + c) * plane + p] * rv[c];
            z[(long long)a * plane + p] = (TZ)(scale * s);
            if (z2) z2[(long long)a * plane + p] = (TZ)(scale * s);
        }
    }
}

// Last Chebyshev sweep: x += d_old + d_new with d_new = c1*d_old + c2*Dinv (r - Ad); r and d are dead afterwards.
template <int NL>
__global__ void __launch_bounds__(KSFD_BLOCK) k_cheb_last(long long n, long long plane, const float *__restrict__ dinv,
                                                          double *__restrict__ x, const double *__restrict__ r,
                                                          const double *__restrict__ d, const double *__restrict__ Ad,
                                                          double c1, double c2, int x_has_d)
{
    constexpr int F = NL + 1;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        double rv[F], dv[F];
#pragma unroll
        for (int c = 0; c < F; c++) {
            const long long o = (long long)c * plane + p;
            dv[c] = d[o];
            rv[c] = r[o] - Ad[o];
        }
#pragma unroll
        for (int a = 0; a < F; a++) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < F; c++) s += dinv[(long long)(a * F + c) * plane + p] * rv[c];
            const long long o = (long long)a * plane + p;
            // x_has_d: x already contains d_old (zero-guess start wrote x = d)
            x[o] += (x_has_d ? 0.0 : dv[a]) + c1 * dv[a] + c2 * s;
        }
    }
}

// One Chebyshev recurrence step after Ad = A d is known:
//   x += d ; r -= Ad ; d = c1*d + c2*(Dinv r)
template <int NL>
__global__ void __launch_bounds__(KSFD_BLOCK) k_cheb_step(long long n, long long plane, const float *__restrict__ dinv,
                                                          double *__restrict__ x, double *__restrict__ r, double *__restrict__ d,
                                                          const double *__restrict__ Ad, double c1, double c2)
{
    constexpr int F = NL + 1;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        double rv[F], dv[F];
#pragma unroll
        for (int c = 0; c < F; c++) {
            const long long o = (long long)c * plane + p;
            dv[c] = d[o];
            x[o] += dv[c];
            rv[c] = r[o] - Ad[o];
            r[o] = rv[c];
        }
#pragma unroll
        for (int a = 0; a < F; a++) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < F; c++) s += dinv[(long long)(a * F + c) * plane + p] * rv[c];
            d[(long long)a * plane + p] = c1 * dv[a] + c2 * s;
        }
    }
}

// deterministic pseudo-random fill for the power iteration
__global__ void __launch_bounds__(KSFD_BLOCK) k_hash_fill(long long n, double *__restrict__ v)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        unsigned long long z = (unsigned long long)p * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
        z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29;
        v[p] = (double)(z >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    }
}

// per-block max over points of 1/(shift * [Dinv]_00): ~ largest diagonal-to-shift ratio, i.e. an estimate of
// lambda_max/lambda_min of Dinv*A on a grid whose smoothest modes see only the shift
__global__ void __launch_bounds__(KSFD_BLOCK) k_ratio_est(long long n, const float *__restrict__ dinv00, double shift,
                                                          double *__restrict__ part)
{
    __shared__ double red[KSFD_BLOCK / KSFD_WAVE];
    double m = 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) m = fmax(m, 1.0 / fabs(shift * dinv00[p]));
    m = ksfd_wave_max(m);
    if ((threadIdx.x & (KSFD_WAVE - 1)) == 0) red[threadIdx.x / KSFD_WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < KSFD_BLOCK / KSFD_WAVE; q++) t = fmax(t, red[q]);
        part[blockIdx.x] = t;
    }
}
