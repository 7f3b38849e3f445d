// libksfd_hip.so -- index plan of the banded direct solver (pc_type 6): the fold of the periodic 1-D ring, the band it leaves, and the
// LAPACK band storage of shift*I - J.  No handle, no device code of its own: banded.hip.h and banded_host.hip.h take every index from
// here (the functions are marked for both sides where a device compiler reads them), and a host-only driver can test them.
//
// The ring 0 .. N-1 is walked from both ends at once: 0, N-1, 1, N-2, 2, ...  Point p sits at folded position pos(p); unknown
// (p, dof) at F*pos(p) + dof.  Ring neighbours at distance <= 2 are then at most 4 folded positions apart -- also across the periodic
// seam and at the far end of the fold -- so the cyclic block-pentadiagonal matrix becomes plainly banded with block half-bandwidth 4:
// kl = ku = 5F - 1, no wrap-around corner.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define KSFD_BAND_HD __host__ __device__ inline
#else
#define KSFD_BAND_HD inline
#endif

#define KSFD_BAND_FOLD 4       // largest folded distance of two ring points at ring distance <= 2

struct BandPlan {
    long long N;               // ring points
    int F;                     // unknowns per point
    long long n;               // F * N
    int kl, ku;                // scalar half-bandwidths, min(5F - 1, n - 1)
    int ldab;                  // leading dimension of the band array: 2 kl + ku + 1 (kl rows of fill-in on top, LAPACK gbtrf)
};

KSFD_BAND_HD BandPlan band_plan(long long N, int F)
{
    BandPlan B;
    B.N = N; B.F = F; B.n = (long long)F * N;
    const long long full = (long long)(KSFD_BAND_FOLD + 1) * F - 1;
    B.kl = B.ku = (int)(full < B.n - 1 ? full : B.n - 1);
    B.ldab = 2 * B.kl + B.ku + 1;
    return B;
}

// folded position of ring point p, and the ring point at a folded position
KSFD_BAND_HD long long band_pos(long long N, long long p) { return p < (N + 1) / 2 ? 2 * p : 2 * (N - 1 - p) + 1; }
KSFD_BAND_HD long long band_point(long long N, long long pos) { return (pos & 1) ? N - 1 - (pos >> 1) : (pos >> 1); }

// band unknown of (point, dof) and back
KSFD_BAND_HD long long band_unknown(const BandPlan &B, long long p, int dof) { return (long long)B.F * band_pos(B.N, p) + dof; }
KSFD_BAND_HD void band_unknown_inv(const BandPlan &B, long long q, long long &p, int &dof)
{
    const long long pos = q / B.F;
    dof = (int)(q - pos * B.F);
    p = band_point(B.N, pos);
}

// entry (i, j) of the matrix, |i - j| inside the band (j - i <= kl + ku, i - j <= kl): AB[kl + ku + i - j][j], column-major
KSFD_BAND_HD bool band_inside(const BandPlan &B, long long i, long long j) { return i - j <= B.kl && j - i <= B.kl + B.ku && i >= 0 && j >= 0 && i < B.n && j < B.n; }
KSFD_BAND_HD long long band_slot(const BandPlan &B, long long i, long long j) { return (long long)(B.kl + B.ku) + i - j + j * (long long)B.ldab; }
KSFD_BAND_HD long long band_size(const BandPlan &B) { return (long long)B.ldab * B.n; }
