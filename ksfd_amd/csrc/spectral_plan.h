// libksfd_hip.so -- FFT plans and small host-side tables of the spectral preconditioner (no handle, no device code): shared by
// spectral_host.hip.h and the stand-alone kernel laboratory tools/spec_lab.hip
#pragma once
#include <math.h>
#include <string.h>
#include <vector>

// n = 2^lg (32 ... 16384) or 3 * 2^lg (48 ... 12288): the power-of-two part is radix 16 from the top with one smaller last stage; a
// factor 3 is a radix-3 stage in front of it (spectral.hip.h: KFFTPlan.m)
static bool spec_plan(long long n, KFFTPlan &P)
{
    int m = 1;
    long long n2 = n;
    if (n2 > 0 && n2 % 3 == 0) { m = 3; n2 /= 3; }
    if (n2 < (m == 3 ? 16 : 32) || n2 > (m == 3 ? 4096 : 16384) || (n2 & (n2 - 1))) return false;
    int lg = 0;
    while ((1LL << lg) < n2) lg++;
    P.n = (int)n; P.lg = lg; P.m = m; P.nstage = 0; P.flags = 0; P.lgw = -1;
    int left = lg;
    // radix 16 from the top, then one smaller stage -- except that a trailing [16, 2] becomes [8, 4]: a radix-2 stage costs a full LDS
    // pass and a barrier for a quarter of the work (512 = 16*8*4, 8192 = 16*16*8*4).  kspec_stage_any relies on exactly these shapes.
    // (n = 32 stays [16, 2]: the row kernels and the slab ownership want a leading radix 16)
    if (lg == 5) { P.radix[P.nstage++] = 16; P.radix[P.nstage++] = 2; left = 0; }
    while (left >= 4 && left != 5 && P.nstage < KSPEC_MAXSTAGE) { P.radix[P.nstage++] = 16; left -= 4; }
    if (left == 5) { P.radix[P.nstage++] = 8; P.radix[P.nstage++] = 4; left = 0; }
    if (left && P.nstage < KSPEC_MAXSTAGE) { P.radix[P.nstage++] = 1 << left; left = 0; }
    return left == 0;
}

// elements of one sequence in the LDS, padding included (device side: kspec_sstride)
static size_t spec_sstride(const KFFTPlan &P) { const size_t n2 = (size_t)1 << P.lg; return (size_t)P.m * (n2 + (n2 >> 4) + 1); }

// position of frequency k in the output of the DIF stages (see spectral.hip.h): pos = q0*(n/r0) + pos'(k / r0), q0 = k % r0
static int spec_pos(const KFFTPlan &P, int k)
{
    int pos = 0, n = P.n;
    if (P.m == 3) { pos = (k % 3) * (n / 3); k /= 3; n /= 3; }
    for (int s = 0; s < P.nstage; s++) {
        const int r = P.radix[s];
        pos += (k % r) * (n / r);
        k /= r;
        n /= r;
    }
    return pos;
}

// Slab ranks (P = 2, 4, 8): the x-transforms are local (a rank owns whole rows); for the y-transforms every rank needs whole
// columns, so the transposed work array is redistributed by an all-to-all: rank q gets the spectral positions whose TOP digit
// (= lowest radix-16 digit of kx) is in its share of the list below.  kx and -kx have top digits d and (16 - d) % 16, so with
// the digits handed out in these pairs both columns of every {kx, -kx} pair land on one rank.
static const int spec_digit_order[16] = { 0, 8, 1, 15, 2, 14, 3, 13, 4, 12, 5, 11, 6, 10, 7, 9 };

// The same for every plan (2-D).  The unit of ownership is a PIECE of w contiguous positions: the 16 top digits of a power-of-two
// plan (w = n/16), or, behind a radix-3 stage, the 48 pieces (q0, d) = (k % 3, (k / 3) % 16) of w = n/48 positions, piece id
// q0 * 16 + d = pos / w.  Since 3 | n, -k lies in (0, (16 - d) % 16) for q0 = 0 and in (2, 15 - d) for q0 = 1 (and back), so the
// ownership ORDER below keeps partners next to each other at an even index: first the q0 = 0 pieces in spec_digit_order (kx = 0 and
// kx = n/2, pieces (0,0) and (0,8), lead: they share a block of the column kernel and go to rank 0), then (1,0), (2,15), (1,1),
// (2,14), ...  Rank q owns the `per` = npiece/P pieces [q * per, (q + 1) * per) of the order -- an even count for P = 1, 2, 4, 8 --
// and stores them in that order: local index of a position = (index of its piece among the rank's) * w + pos % w.
struct SpecOwn {
    int P, npiece, w, per;         // ranks, pieces, positions per piece, pieces per rank
    int piece[48], order[48];      // piece[o] = id of the o-th piece of the order; order[id] = o
};
static bool spec_ownership(const KFFTPlan &Q, int P, SpecOwn &O)
{
    if ((P != 1 && P != 2 && P != 4 && P != 8) || Q.nstage < 1 || Q.radix[0] != 16) return false;
    O.P = P; O.npiece = 16 * Q.m; O.w = Q.n / O.npiece; O.per = O.npiece / P;
    for (int o = 0; o < 16; o++) O.piece[o] = spec_digit_order[o];
    if (Q.m == 3) for (int d = 0; d < 16; d++) { O.piece[16 + 2 * d] = 16 + d; O.piece[17 + 2 * d] = 32 + 15 - d; }
    for (int o = 0; o < O.npiece; o++) O.order[O.piece[o]] = o;
    return true;
}
static int spec_owner(const SpecOwn &O, int pos) { return O.order[pos / O.w] / O.per; }
static int spec_local_index(const SpecOwn &O, int pos) { return (O.order[pos / O.w] % O.per) * O.w + pos % O.w; }
static int spec_piece_start(const SpecOwn &O, int rank, int i) { return O.piece[rank * O.per + i] * O.w; }      // first position of rank's i-th piece

// Which slab handles have the 2-D solver -- the one place that decides it (the transport must also offer an all-to-all: spec_build).
// nx, ny each 2^k or 3 * 2^k (the plans); P = 1, 2, 4, 8; nyl = ny/P local rows, at least 4.  ny = 3 * 2^k gives a rank 3 * 2^j rows:
// they are handled as nch = 3 CHUNKS of cs = 2^j rows, so that the column kernel still sees a column as pieces of a power of two
// (3 P pieces of 2^j); cs >= 2 because it moves two elements at a time.
static bool spec_slab_eligible(const KFFTPlan &px, const KFFTPlan &py, int P, long long nyl, SpecOwn &O, int &nch)
{
    if (!spec_ownership(px, P, O)) return false;
    nch = py.m;
    if (nyl < 4 || nyl % nch) return false;
    const long long cs = nyl / nch;
    return cs >= 2 && !(cs & (cs - 1));
}
// The two all-to-alls move blocks (peer, field pair p, piece i of the receiver, chunk c) of w positions x cs rows, contiguous on both
// sides.  Sender: W[chunk][pair][pos][row in chunk] (the row kernels' transposed store, chunk-major); receiver:
// W2[sender * nch + chunk][pair][own position][row in chunk], i.e. piece number (global row / cs) of every column, as k_spec_cols
// addresses it.  Element offsets of a block:
static size_t spec_a2a_src(const SpecOwn &O, int nx, int npair, long long cs, int peer, int p, int i, int c)
{
    return (((size_t)c * npair + p) * nx + spec_piece_start(O, peer, i)) * cs;
}
static size_t spec_a2a_dst(const SpecOwn &O, int npair, int nch, long long cs, int sender, int p, int i, int c)
{
    return ((((size_t)sender * nch + c) * npair + p) * ((size_t)O.per * O.w) + (size_t)i * O.w) * cs;
}

// 3-D on z-slab ranks, the same scheme one axis up: x and y are local, the z columns are completed by an all-to-all over the x
// positions (ownership of px as above, so the columns (kx, ky) and (-kx, -ky) land on one rank).  nx, ny, nz each 2^k or 3 * 2^k;
// P = 1, 2, 4, 8 with P * nzl = nz; nz = 3 * 2^k gives a rank 3 * 2^j planes, handled as nch = 3 chunks of cs = 2^j planes (cs >= 2:
// the z kernel moves two elements at a time), else one chunk of nzl = 2^j >= 2 planes.
static bool spec_slab3_eligible(const KFFTPlan &px, const KFFTPlan &pz, int P, long long nzl, SpecOwn &O, int &nch)
{
    if (!spec_ownership(px, P, O)) return false;
    nch = pz.m;
    if (nzl < 2 || nzl * P != pz.n || nzl % nch) return false;
    const long long cs = nzl / nch;
    return cs >= 2 && !(cs & (cs - 1));
}
// Blocks (peer, field pair p, piece i of the receiver, chunk c) of w positions x ny x cs planes, contiguous on both sides.  Sender:
// W[chunk][pair][pos_x][pos_y][plane in chunk] (k_spec3_y_fwd's store, once per chunk); receiver:
// W2[sender * nch + chunk][pair][own pos_x][pos_y][plane in chunk]: a z column is P * nch pieces of cs elements at one stride
// (npair * nxl * ny * cs), piece number = global plane / cs, as k_spec3_z addresses it.  A (pos_x, pos_y) column of cs planes takes
// the place of a 2-D row-chunk element, so the offsets are the 2-D ones with ny * cs for cs.
static size_t spec_a2a3_src(const SpecOwn &O, int nx, int ny, int npair, long long cs, int peer, int p, int i, int c)
{
    return spec_a2a_src(O, nx, npair, ny * cs, peer, p, i, c);
}
static size_t spec_a2a3_dst(const SpecOwn &O, int ny, int npair, int nch, long long cs, int sender, int p, int i, int c)
{
    return spec_a2a_dst(O, npair, nch, ny * cs, sender, p, i, c);
}

// exp(-2 pi i j / 2^lg), j < 2^lg, for the power-of-two stages; behind it, for 3 * 2^lg, exp(-2 pi i j / n), j < 2^lg (radix-3 stage)
static std::vector<kcf> spec_twiddles(const KFFTPlan &P)
{
    const int n2 = 1 << P.lg;
    std::vector<kcf> t((size_t)n2 * (P.m == 3 ? 2 : 1));
    for (int k = 0; k < n2; k++) { const double a = -2.0 * M_PI * k / n2; t[k] = make_float2((float)cos(a), (float)sin(a)); }
    if (P.m == 3) for (int k = 0; k < n2; k++) { const double a = -2.0 * M_PI * k / P.n; t[n2 + k] = make_float2((float)cos(a), (float)sin(a)); }
    return t;
}
static std::vector<int> spec_positions(const KFFTPlan &Q) { std::vector<int> p(Q.n); for (int k = 0; k < Q.n; k++) p[k] = spec_pos(Q, k); return p; }
static std::vector<int> spec_inverse(const std::vector<int> &p) { std::vector<int> q(p.size()); for (size_t k = 0; k < p.size(); k++) q[p[k]] = (int)k; return q; }
// per POSITION of the transform's output: (position of the wavenumber -k, bit pattern of the symbol l[k]), k = the wavenumber at that position
static std::vector<int2> spec_partner_table(const KFFTPlan &Q, const std::vector<float> &l)
{
    const std::vector<int> pos = spec_positions(Q), kof = spec_inverse(pos);
    std::vector<int2> t(Q.n);
    for (int m = 0; m < Q.n; m++) {
        const int k = kof[m];
        int bits;
        memcpy(&bits, &l[k], sizeof bits);
        t[m] = make_int2(pos[(Q.n - k) % Q.n], bits);
    }
    return t;
}
static std::vector<float> spec_symbol_table(int n, double inv_h2);
static std::vector<float> spec_symbol_table(int n, double inv_h2)
{
    std::vector<float> l(n);
    for (int k = 0; k < n; k++) { const double th = 2.0 * M_PI * k / n; l[k] = (float)((-30.0 + 32.0 * cos(th) - 2.0 * cos(2.0 * th)) / 12.0 * inv_h2); }
    return l;
}

