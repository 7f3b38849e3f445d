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
#include "mg_tail_plan.h"

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

// ------------------------------------------------------------------------------------------------
// The coarse TAIL of the V cycle in one workgroup (ksfd_set_mg_tail, opt-in; which levels: mg_tail_plan.h).  The sub-cycle from the
// first tail level down to the level the cycle ends on and back -- pre-smoothing, residual, restriction, the Chebyshev sweeps of the
// end level, prolongation, post-smoothing: what mg_vcycle<double>(t) of mg_host.hip.h runs as tens of tiny launches -- is pointwise in
// every phase, so ONE block of MG_TAIL_THREADS threads runs it with every level vector in the LDS and __syncthreads() between the phases.
// The coefficient planes and the fp32 inverse point blocks stay in global memory (read-only, L2-resident).
//
// Rules of the text below:
//  * thread `tid` owns the points tid, tid + NT, ... of EVERY level (the loop has the compile-time trip count PPT of the plan and
//    tests p < np), so whatever a phase reads at its own point alone needs no barrier behind the phase that wrote it;
//  * every __syncthreads() stands in control flow that depends on kernel arguments alone (level count, sweep counts): uniform over
//    the block.  No loop bound is read from data; no atomics, no waiting on memory;
//  * a phase that replaces a vector whose neighbours other threads still read (d under A d) keeps the new values in registers (dn)
//    and stores them behind the barrier.
// The levels are whole (no ghost units, plane = points) and every axis wraps.  Formulas: the operator of k_jvp_generic on the dG plane of
// k_dg_frozen, the transfers of k_mg_restrict / k_mg_prolong_add, the Chebyshev recurrence of mg_smooth (direction form) with the
// coefficients of mg_cheb, the blocks of k_blockdiag_inv as they are in memory.
struct KMGTailLevel {
    const double *coef;                // [rho, G, G_rho, G_U..] planes of np doubles
    const float *dinv;                 // F*F planes of the inverse point blocks
    int n[3];                          // extents per axis (1 on the axes the grid does not have)
    int np;                            // points
    int sweeps;                        // Chebyshev sweeps: nu, on the last level those of the coarse solve
    int pad;
    double inv_h[3], inv_h2[3];
    double theta, delta, sig1, rho0;   // mg_cheb of the level's interval [lam_max / ratio, lam_max]
};
struct KMGTail {
    int nlev, dim;
    double shift;
    KMGTailLevel L[ksfd_ctl::MG_TAIL_MAX_LEVELS];
};
struct KMGTailVecs { double *x, *b, *r, *d, *dG; };

// the LDS of level q: behind the levels before it, each mg_tail_level_bytes long (the plan's formula): x, b, r, d (F planes), dG
__device__ __forceinline__ KMGTailVecs ksfd_tail_vecs(double *lds, const KMGTail &T, int q, int F)
{
    long long off = 0;
    for (int s = 0; s < q; s++) off += ksfd_ctl::mg_tail_level_bytes(T.L[s].np, F) / 8;
    const long long fp = (long long)F * T.L[q].np;
    KMGTailVecs V;
    V.x = lds + off; V.b = V.x + fp; V.r = V.b + fp; V.d = V.r + fp; V.dG = V.d + fp;
    return V;
}

// q = (shift I - J) v at point p of level D; v and dG in the LDS
template <int NL>
__device__ __forceinline__ void ksfd_tail_op(const KMGTailLevel &D, int dim, const KPhys &P, double shift, const double *v,
                                             const double *dG, int p, double *q)
{
    const int np = D.np, nx = D.n[0], ny = D.n[1];
    const double *__restrict__ rho = D.coef, *__restrict__ Gb = D.coef + np;
    const int idx[3] = { p % nx, (p / nx) % ny, p / (nx * ny) };
    const int str[3] = { 1, nx, nx * ny };
    double acc = 0.0, lapG = 0.0, lapdG = 0.0, lapV[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) lapV[l] = 0.0;
    for (int a = 0; a < dim; a++) {
        const int ext = D.n[a], base = p - idx[a] * str[a];
        int o[5];
#pragma unroll
        for (int m = 0; m < 5; m++) o[m] = base + ((idx[a] + m - 2) % ext + ext) % ext * str[a];
        const double r_m2 = ksfd_clamp(rho[o[0]], P.rhomin), r_m1 = ksfd_clamp(rho[o[1]], P.rhomin),
                     r_p1 = ksfd_clamp(rho[o[3]], P.rhomin), r_p2 = ksfd_clamp(rho[o[4]], P.rhomin);
        const double d1r = KSFD_D1(r_m2, r_m1, r_p1, r_p2) * D.inv_h[a];
        const double d1v = KSFD_D1(v[o[0]], v[o[1]], v[o[3]], v[o[4]]) * D.inv_h[a];
        const double d1g = KSFD_D1(Gb[o[0]], Gb[o[1]], Gb[o[3]], Gb[o[4]]) * D.inv_h[a];
        const double d1e = KSFD_D1(dG[o[0]], dG[o[1]], dG[o[3]], dG[o[4]]) * D.inv_h[a];
        acc += d1v * d1g + d1r * d1e;
        lapG += KSFD_D2(Gb[o[0]], Gb[o[1]], Gb[o[2]], Gb[o[3]], Gb[o[4]]) * D.inv_h2[a];
        lapdG += KSFD_D2(dG[o[0]], dG[o[1]], dG[o[2]], dG[o[3]], dG[o[4]]) * D.inv_h2[a];
#pragma unroll
        for (int l = 0; l < NL; l++) {
            const double *V = v + (l + 1) * np;
            lapV[l] += KSFD_D2(V[o[0]], V[o[1]], V[o[2]], V[o[3]], V[o[4]]) * D.inv_h2[a];
        }
    }
    const double v0 = v[p], rho0 = ksfd_clamp(rho[p], P.rhomin);
    q[0] = shift * v0 - (acc + v0 * lapG + rho0 * lapdG);
#pragma unroll
    for (int l = 0; l < NL; l++) {
        const double V0 = v[(l + 1) * np + p];
        q[l + 1] = shift * V0 - (-P.lig_gamma[l] * V0 + P.lig_s[l] * v0 + P.lig_D[l] * lapV[l]);
    }
}

// dG = G_rho v_rho + sum_l G_Ul v_Ul at point p from the F values w of v there
template <int NL>
__device__ __forceinline__ double ksfd_tail_dg(const KMGTailLevel &D, int p, const double *w)
{
    double d = D.coef[2 * D.np + p] * w[0];
#pragma unroll
    for (int l = 0; l < NL; l++) d += D.coef[(3 + l) * D.np + p] * w[l + 1];
    return d;
}

// z = scale * Dinv r at point p
template <int NL>
__device__ __forceinline__ void ksfd_tail_dinv(const KMGTailLevel &D, int p, const double *r, double scale, double *z)
{
    constexpr int F = NL + 1;
#pragma unroll
    for (int a = 0; a < F; a++) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < F; c++) s += D.dinv[(a * F + c) * D.np + p] * r[c];
        z[a] = scale * s;
    }
}

// dG of the vector v over the thread's points (own points only: no barrier needed behind the phase that wrote v there)
template <int NL, int PPT>
__device__ __forceinline__ void ksfd_tail_dg_pass(const KMGTailLevel &D, const double *v, double *dG)
{
    constexpr int F = NL + 1, NT = ksfd_ctl::MG_TAIL_THREADS;
#pragma unroll
    for (int s = 0; s < PPT; s++) {
        const int p = (int)threadIdx.x + s * NT;
        if (p < D.np) {
            double w[F];
#pragma unroll
            for (int c = 0; c < F; c++) w[c] = v[c * D.np + p];
            dG[p] = ksfd_tail_dg<NL>(D, p, w);
        }
    }
}

// D.sweeps Chebyshev sweeps on A x = b (V.b -> V.x), from the zero guess or as a correction of V.x.  On entry V.b (and V.x) are complete
// at the thread's own points at least -- and, for a correction, NOTHING but the own points of V.x is read before the first barrier.  On
// exit V.x is complete at the thread's own points: the caller puts a barrier before anything reads its neighbours.
template <int NL, int PPT>
__device__ __forceinline__ void ksfd_tail_smooth(const KMGTailLevel &D, int dim, const KPhys &P, double shift, const KMGTailVecs &V, bool zero_init)
{
    constexpr int F = NL + 1, NT = ksfd_ctl::MG_TAIL_THREADS;
    const int np = D.np, tid = (int)threadIdx.x;
    double dn[PPT][F];                                       // the direction d_k at the thread's points
    if (zero_init) {
        // r_0 = b, d_0 = Dinv b / theta, x = 0
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int p = tid + s * NT;
            if (p < np) {
                double rv[F];
#pragma unroll
                for (int c = 0; c < F; c++) { rv[c] = V.b[c * np + p]; V.r[c * np + p] = rv[c]; V.x[c * np + p] = 0.0; }
                ksfd_tail_dinv<NL>(D, p, rv, 1.0 / D.theta, dn[s]);
            }
        }
    } else {
        // r_0 = b - A x, d_0 = Dinv r_0 / theta
        ksfd_tail_dg_pass<NL, PPT>(D, V.x, V.dG);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int p = tid + s * NT;
            if (p < np) {
                double q[F], rv[F];
                ksfd_tail_op<NL>(D, dim, P, shift, V.x, V.dG, p, q);
#pragma unroll
                for (int c = 0; c < F; c++) { rv[c] = V.b[c * np + p] - q[c]; V.r[c * np + p] = rv[c]; }
                ksfd_tail_dinv<NL>(D, p, rv, 1.0 / D.theta, dn[s]);
            }
        }
        __syncthreads();                                     // the reads of x and dG are over: both change below
    }
    double rho = D.rho0;
    for (int k = 1; k < D.sweeps; k++) {
        // d_{k-1} and its dG plane into the LDS
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int p = tid + s * NT;
            if (p < np) {
#pragma unroll
                for (int c = 0; c < F; c++) V.d[c * np + p] = dn[s][c];
                V.dG[p] = ksfd_tail_dg<NL>(D, p, dn[s]);
            }
        }
        __syncthreads();
        // x += d ; r -= A d ; d = c1 d + c2 Dinv r
        const double rhon = 1.0 / (2.0 * D.sig1 - rho), c1 = rhon * rho, c2 = 2.0 * rhon / D.delta;
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int p = tid + s * NT;
            if (p < np) {
                double q[F], rv[F], z[F];
                ksfd_tail_op<NL>(D, dim, P, shift, V.d, V.dG, p, q);
#pragma unroll
                for (int c = 0; c < F; c++) { V.x[c * np + p] += dn[s][c]; rv[c] = V.r[c * np + p] - q[c]; V.r[c * np + p] = rv[c]; }
                ksfd_tail_dinv<NL>(D, p, rv, c2, z);
#pragma unroll
                for (int c = 0; c < F; c++) dn[s][c] = c1 * dn[s][c] + z[c];
            }
        }
        __syncthreads();                                     // the reads of d and dG are over
        rho = rhon;
    }
#pragma unroll
    for (int s = 0; s < PPT; s++) {
        const int p = tid + s * NT;
        if (p < np) {
#pragma unroll
            for (int c = 0; c < F; c++) V.x[c * np + p] += dn[s][c];
        }
    }
}

// x = (one V cycle from level T.L[0] down to T.L[nlev - 1] and back) b; b and x: F planes of T.L[0].np doubles in global memory
template <int NL>
__global__ void __launch_bounds__(ksfd_ctl::MG_TAIL_THREADS) k_mg_tail(KMGTail T, KPhys P, const double *__restrict__ bg, double *__restrict__ xg)
{
    constexpr int F = NL + 1, NT = ksfd_ctl::MG_TAIL_THREADS, PPT = ksfd_ctl::mg_tail_points_per_thread(F);
    extern __shared__ double mg_tail_lds[];
    const int tid = (int)threadIdx.x, dim = T.dim, last = T.nlev - 1;
    {
        const KMGTailVecs V = ksfd_tail_vecs(mg_tail_lds, T, 0, F);
        const int np = T.L[0].np;
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int p = tid + s * NT;
            if (p < np) {
#pragma unroll
                for (int c = 0; c < F; c++) V.b[c * np + p] = bg[(long long)c * np + p];
            }
        }
    }
    // down: pre-smoothing from the zero guess, residual, full weighting onto the next level
    for (int q = 0; q < last; q++) {
        const KMGTailLevel &D = T.L[q], &Dc = T.L[q + 1];
        const KMGTailVecs V = ksfd_tail_vecs(mg_tail_lds, T, q, F), Vc = ksfd_tail_vecs(mg_tail_lds, T, q + 1, F);
        const int np = D.np;
        ksfd_tail_smooth<NL, PPT>(D, dim, P, T.shift, V, true);
        ksfd_tail_dg_pass<NL, PPT>(D, V.x, V.dG);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int p = tid + s * NT;
            if (p < np) {
                double w[F];
                ksfd_tail_op<NL>(D, dim, P, T.shift, V.x, V.dG, p, w);
#pragma unroll
                for (int c = 0; c < F; c++) V.r[c * np + p] = V.b[c * np + p] - w[c];
            }
        }
        __syncthreads();
        // coarse b(I, J, K) = sum w_a w_b w_d r(2I + d, 2J + b, 2K + a), w = (1/4, 1/2, 1/4), over the axes the grid has
        const int nxf = D.n[0], nyf = D.n[1], nzf = D.n[2], nxc = Dc.n[0], nyc = Dc.n[1], npc = Dc.np;
        const int cx = 3, cy = dim > 1 ? 3 : 1, cz = dim > 2 ? 3 : 1;
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int p = tid + s * NT;
            if (p < npc) {
                const int I = p % nxc, J = (p / nxc) % nyc, K = p / (nxc * nyc);
                const double wt[3] = { 0.25, 0.5, 0.25 };
                for (int c = 0; c < F; c++) {
                    const double *f = V.r + c * np;
                    double sum = 0.0;
                    for (int a = 0; a < cz; a++) {
                        const int kz = cz == 1 ? 0 : (2 * K + a - 1 + nzf) % nzf;
                        for (int b = 0; b < cy; b++) {
                            const int jy = cy == 1 ? 0 : (2 * J + b - 1 + nyf) % nyf;
                            const double wab = (cz == 1 ? 1.0 : wt[a]) * (cy == 1 ? 1.0 : wt[b]);
                            for (int d = 0; d < cx; d++) sum += wab * wt[d] * f[(2 * I + d - 1 + nxf) % nxf + nxf * (jy + nyf * kz)];
                        }
                    }
                    Vc.b[c * npc + p] = sum;
                }
            }
        }
        __syncthreads();
    }
    // the level the cycle ends on: its Chebyshev sweeps over the whole interval, from the zero guess
    ksfd_tail_smooth<NL, PPT>(T.L[last], dim, P, T.shift, ksfd_tail_vecs(mg_tail_lds, T, last, F), true);
    __syncthreads();
    // up: x += P x_coarse (linear interpolation along each axis), post-smoothing as a correction
    for (int q = last - 1; q >= 0; q--) {
        const KMGTailLevel &D = T.L[q], &Dc = T.L[q + 1];
        const KMGTailVecs V = ksfd_tail_vecs(mg_tail_lds, T, q, F), Vc = ksfd_tail_vecs(mg_tail_lds, T, q + 1, F);
        const int np = D.np, nxf = D.n[0], nyf = D.n[1], nxc = Dc.n[0], nyc = Dc.n[1], nzc = Dc.n[2], npc = Dc.np;
        const int cy = dim > 1 ? 2 : 1, cz = dim > 2 ? 2 : 1;
        const double wsum = 1.0 / (2 * cy * cz);
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int p = tid + s * NT;
            if (p < np) {
                const int i = p % nxf, j = (p / nxf) % nyf, k = p / (nxf * nyf);
                const int Ii[2] = { i >> 1, (i & 1) ? ((i >> 1) + 1) % nxc : i >> 1 };
                const int Jj[2] = { j >> 1, (j & 1) ? ((j >> 1) + 1) % nyc : j >> 1 };
                const int Kk[2] = { k >> 1, (k & 1) ? ((k >> 1) + 1) % nzc : k >> 1 };
                for (int c = 0; c < F; c++) {
                    const double *g = Vc.x + c * npc;
                    double sum = 0.0;
                    for (int a = 0; a < cz; a++)
                        for (int b = 0; b < cy; b++) sum += g[Ii[0] + nxc * (Jj[b] + nyc * Kk[a])] + g[Ii[1] + nxc * (Jj[b] + nyc * Kk[a])];
                    V.x[c * np + p] += wsum * sum;
                }
            }
        }
        ksfd_tail_smooth<NL, PPT>(D, dim, P, T.shift, V, false);
        __syncthreads();
    }
    {
        const KMGTailVecs V = ksfd_tail_vecs(mg_tail_lds, T, 0, F);
        const int np = T.L[0].np;
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int p = tid + s * NT;
            if (p < np) {
#pragma unroll
                for (int c = 0; c < F; c++) xg[(long long)c * np + p] = V.x[c * np + p];
            }
        }
    }
}
