// libksfd_hip.so -- FFT plans, slab ownership, small host-side tables and the shape planner of the spectral preconditioner (no handle, no
// device code, no HIP call): shared by spectral_host.hip.h, the stand-alone kernel laboratory tools/spec_lab.hip and the CPU tests
#pragma once
#include <limits.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

#ifndef __HIP__
// a host-only build (the drivers of the CPU tests, which declare the plan struct, float2 and int2 themselves): the vector type of the tables
struct int4 { int x, y, z, w; };
static int4 make_int4(int x, int y, int z, int w) { int4 r = { x, y, z, w }; return r; }
#endif

static int spec_log2(long long v) { int lg = 0; while ((1LL << lg) < v) lg++; return lg; }      // rounded up

// n = 2^lg (32 ... 16384) or 3 * 2^lg (48 ... 12288): the power-of-two part is radix 16 from the top with one smaller last stage; a
// factor 3 is a radix-3 stage in front of it (spectral.hip.h: KFFTPlan.m)
static bool spec_plan(long long n, KFFTPlan &P)
{
    int m = 1;
    long long n2 = n;
    if (n2 > 0 && n2 % 3 == 0) { m = 3; n2 /= 3; }
    if (n2 < (m == 3 ? 16 : 32) || n2 > (m == 3 ? 4096 : 16384) || (n2 & (n2 - 1))) return false;
    const int lg = spec_log2(n2);
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
// the place of a 2-D row-chunk element, so the offsets are the 2-D ones with ny * cs for cs (that is how spec_shape calls them).
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
static std::vector<float> spec_symbol_table(int n, double inv_h2)
{
    std::vector<float> l(n);
    for (int k = 0; k < n; k++) { const double th = 2.0 * M_PI * k / n; l[k] = (float)((-30.0 + 32.0 * cos(th) - 2.0 * cos(2.0 * th)) / 12.0 * inv_h2); }
    return l;
}

// ------------------------------------------------------------------------------------------------
// The shape planner: every integer decision of the host side, from the grid and the knobs alone (no handle, no HIP call, no environment read),
// so that all of it runs on a CPU (tests/test_spectral_shape_cpu.py).  spec_build (spectral_host.hip.h) turns its answer into
// allocations, kernel instances and all-to-all lists; tools/spec_lab.hip takes its launch shape from here too.
struct SpecKnobs {                 // the KSFD_SPEC_* experiment knobs (read by spec_knobs, spectral_host.hip.h); these defaults = none set
    bool no3d = false, single = false, transposed = false;
    int cz = INT_MAX, pb = INT_MAX, rb = INT_MAX;      // upper limits of the planner's own choice
    int split = 0;                                     // 1 / 2: force cols_split (tests of the split paths on small grids)
    int lgw = -1;
    int thr_rows = 0, thr_cols = 0, thr_z = 0;         // > 0: block size of the row / column / z launches
    int diag = 0, fuse = 7, fuse3 = 3;
};
struct SpecGrid {
    int dim;
    long long n[3];                // global extents
    int F, P, rank;
    bool ring;                     // slab layout + all-to-alls (also a ring of ONE rank: every piece is its own)
    long long sloc;                // local rows (3-D: z planes)
    int ng;                        // ghost depth
};
struct SpecShape {
    int dim = 2, npair = 0;
    KFFTPlan px, py, pz;
    int nch = 1;                   // slab ranks with 3 * 2^j rows (3-D: z planes): 3 chunks of 2^j; else 1
    int rb = 0, lg_rb = 0, ntiles = 0;     // rows per tile of the row kernels, tiles of a chunk
    int nyp = 0;                   // column stride of the work arrays = rows (3-D: ny * planes) of a chunk; one rank in 2-D: rounded up to 2^lg_pl
    int nxl = 0, lg_pl = 0;        // owned x positions; log2 of the rows (3-D: planes) of a chunk, rounded up
    int cols_split = 0;            // k_spec_cols_split in two phases (spectral.hip.h): 1 = the 2*npair columns of a pair block exceed the LDS (one field
                                   // pair per block), 2 = the two columns of one pair do too (columns of more than 8192 points: one column per block)
    bool tile_major = false, need_w2 = false;
    bool a2a_back_from_w = false;  // the backward all-to-all goes W -> W2 instead of W2 -> W (split column kernel, see spec_shape)
    int lgw = -1;                  // layout of the forward work array (kspec_wt_index)
    int lg_cz = 0, pb = 1;         // 3-D: log2 of the z planes per block of the y kernels, table entries per block of the z kernel
    int nent = 0, nblk_cols = 0;   // entries of the 3-D table / of the 2-D table = blocks of the column kernel
    size_t lds_rows = 0, lds_cols = 0, lds_y3 = 0, lds_z3 = 0;
    size_t welems = 0;             // elements of a work array
    int thr_rows = 0, thr_cols = 0, thr_y = 0, thr_z = 0;      // block sizes (forward and inverse rows share thr_rows, y forward and inverse thr_y)
    int diag = 0, fuse = 0, fuse3 = 0;     // KFFTPlan.flags of the 2-D kernels / of the y and z kernels; diag: stages left out (timing only)
};
struct SpecBlock { int peer; size_t src, dst, bytes; };        // element offsets in the array sent from / received into
struct SpecTables {
    // 2-D: per block of the column kernel (local index of kx, of -kx, kx, 0), and (local index of 0, of nx/2, 0, nx/2 + 1) for the two
    // self-paired columns, which share a block.  3-D: per pair of columns {(kx, ky), (-kx, -ky)} (local column of the first, of the
    // second, kx | ky << 16, 1 if the column is its own partner); a column is local position of kx * ny + position of ky
    std::vector<int4> pairtab;
    std::vector<SpecBlock> a2a_fwd, a2a_back;
};

// 3-D (see spectral.hip.h): a plan per axis, two work arrays.  One rank: every extent with a plan, 2^k or 3 * 2^k per axis.  z-slab
// ranks (P = 2, 4, 8, and the ring of one), the same extents: the x and y transforms are local (a rank owns whole z planes); for the z
// transforms every rank needs whole z columns, so W[pair][pos_x][pos_y][z_local] is redistributed by an all-to-all over pos_x exactly
// as in 2-D (same ownership: the columns (kx, ky) and (-kx, -ky) land on one rank), a received column consisting of P pieces of nz/P
// elements.  3 * 2^j local rows (planes) are nch = 3 chunks of cs = 2^j: both work arrays are chunk-major, the row and y kernels run
// once per chunk, and a received column is 3 P pieces of 2^j elements.
static bool spec_shape(const SpecGrid &I, const SpecKnobs &K, SpecShape &S, SpecTables &T)
{
    S = SpecShape();
    T = SpecTables();
    const bool d3 = I.dim == 3, ring = I.ring;
    if ((I.dim != 2 && !d3) || (d3 && (K.no3d || (!ring && I.ng != 0)))) return false;
    const long long nsl = I.sloc;
    if (!spec_plan(I.n[0], S.px) || !spec_plan(I.n[1], S.py) || (d3 && !spec_plan(I.n[2], S.pz))) return false;
    const int nx = S.px.n, ny = S.py.n;
    SpecOwn O;
    int nch = 1;
    if (ring && !(d3 ? spec_slab3_eligible(S.px, S.pz, I.P, nsl, O, nch) : spec_slab_eligible(S.px, S.py, I.P, nsl, O, nch))) return false;
    if (d3 ? (S.px.radix[0] != 16 || nx > 32768 || ny > 32768 || nsl < 2) : nsl < 4) return false;
    const long long cs = nsl / nch;                                  // rows (planes) per chunk: a power of two on slab ranks
    const long long crows = d3 ? ny * cs : cs;                       // x rows of a chunk
    S.dim = I.dim;
    S.nch = nch;
    S.npair = (I.F + 1) / 2;
    const size_t lds_max = 160 * 1024 - 1024, row_bytes = sizeof(kcf) * spec_sstride(S.px);
    // rows per tile: as many as the LDS holds (wider store segments of the transposed write), but keep >= 2 tiles per CU
    int rb = 16;
    if (d3) {
        while (rb > 1 && row_bytes * rb > lds_max) rb >>= 1;
        while (rb > 2 && crows / rb < 512) rb >>= 1;
        if (row_bytes * rb > lds_max || crows % rb || ny % rb) return false;      // a tile must not straddle two z planes' y ranges unevenly
    } else {
        rb = (int)std::min<size_t>(lds_max / row_bytes, 16);
        while (rb & (rb - 1)) rb &= rb - 1;                          // a power of two ...
        while (rb > 1 && (nsl % rb)) rb >>= 1;                       // ... that divides the rows
        if (rb < 1) return false;
        while (rb > 2 && nsl / rb < 512) rb >>= 1;
        rb = std::max(1, std::min(rb, K.rb));
    }
    S.rb = rb;
    S.lg_rb = spec_log2(rb);
    S.ntiles = (int)(crows / rb);
    S.lds_rows = row_bytes * rb;
    S.thr_rows = K.thr_rows > 0 ? K.thr_rows : (int)std::min<long long>(1024, std::max<long long>(256, (long long)rb * nx / 16));
    S.nxl = nx / I.P;
    S.lg_pl = spec_log2(cs);
    S.diag = K.diag;
    S.fuse3 = K.fuse3 & 3;
    if (d3) {
        const size_t ycol = sizeof(kcf) * spec_sstride(S.py) * S.npair, zcol = sizeof(kcf) * spec_sstride(S.pz) * 2 * S.npair;
        int cz = 16, pb = 16;
        while (cz > 1 && (ycol * cz > lds_max / 2 || cs % cz)) cz >>= 1;          // <= half the LDS: two blocks per CU
        cz = std::max(1, std::min(cz, K.cz));
        // small blocks, many per CU: their load / transform / store phases overlap (512^3: pb 8 -> 2, 1.27 -> 1.12 ms)
        while (pb > 1 && zcol * pb > lds_max / 8) pb >>= 1;
        pb = std::max(1, std::min(pb, K.pb));
        if (ycol * cz > lds_max || zcol * pb > lds_max) return false;
        S.lg_cz = spec_log2(cz);
        S.pb = pb;
        S.lds_y3 = ycol * cz;
        S.lds_z3 = zcol * pb;
        // (whole waves: 3 * 2^k extents with three or more field pairs give odd multiples of 32)
        S.thr_y = (int)std::min<long long>(1024, std::max<long long>(256, ((long long)S.npair * cz * ny / 16 + 63) & ~63LL));
        S.thr_z = K.thr_z > 0 ? K.thr_z : (int)std::min<long long>(1024, std::max<long long>(128, ((long long)2 * S.npair * pb * S.pz.n / 16 + 63) & ~63LL));
        S.nyp = (int)crows;
        S.tile_major = S.need_w2 = true;
        S.fuse = K.fuse & 7;
    } else {
        const size_t col = sizeof(kcf) * spec_sstride(S.py);
        S.lds_cols = col * 2 * S.npair;
        S.cols_split = (S.lds_cols > lds_max || (K.split == 1 && S.npair > 1) || K.split == 2) ? 1 : 0;
        if (S.cols_split) S.lds_cols = col * 2;                                   // one field pair per block
        if (S.cols_split && (S.lds_cols > lds_max || K.split == 2)) {             // ... one column per block (more than 8192 points)
            S.cols_split = 2;
            S.lds_cols = col;
        }
        if (S.lds_cols > lds_max) return false;
        S.thr_cols = K.thr_cols > 0 ? K.thr_cols
                                    : (int)std::min<long long>(512, std::max<long long>(128, (long long)(S.cols_split == 2 ? 1 : 2) * (S.cols_split ? 1 : S.npair) * ny / 16));
        // column stride of W: the rows of this rank, rounded up to the power of two the column kernel addresses pieces with (equal for
        // 2^k rows); slab ranks: the rows of one chunk, W = [chunk][pair][pos][row in chunk]
        S.nyp = (int)(ring ? cs : 1LL << S.lg_pl);
        S.tile_major = !ring && rb >= 2 && !K.transposed;
        S.need_w2 = ring || S.tile_major || S.cols_split;
        // one rank: the forward work array is tile-major; knob lgw = k makes it position-group-major with groups of 2^k (kspec_wt_index;
        // k = 2 at 4 rows per tile: one 128-B line per (group, tile).  Measured with the kernel laboratory at 4096^2 (tools/spec_lab.hip,
        // median of 7 batches): row kernel 70 -> 74 us, column kernel 94 -> 96 us -- no gain once the symbol stage stopped waiting on table
        // look-ups)
        if (S.tile_major) S.lgw = std::max(-1, std::min(K.lgw, 8));
        if (S.lgw >= 0 && (S.nxl & ((1 << S.lgw) - 1))) S.lgw = -1;
        // bit 3 of fuse (the column kernel stores tile-major for the inverse row kernel): one rank, plain column kernel only
        S.fuse = (ring || S.cols_split || !S.tile_major) ? (K.fuse & 7) : K.fuse;
    }
    S.welems = (size_t)S.npair * nx * S.nyp * nch;
    // ownership of the x positions on slab ranks: as above (one rank: the work array is used in place, positions are their own index)
    auto mine = [&](int j) { return !ring || spec_owner(O, j) == I.rank; };
    auto local_index = [&](int j) { return !ring ? j : spec_local_index(O, j); };
    const std::vector<int> posx = spec_positions(S.px), posy = spec_positions(S.py);
    for (int kx = 0; kx <= nx / 2; kx++) {
        const int kxm = (nx - kx) % nx, ja = local_index(posx[kx]), jb = local_index(posx[kxm]);
        if (!mine(posx[kx])) continue;
        if (!d3) {
            if (kx == 0) T.pairtab.push_back(make_int4(ja, local_index(posx[nx / 2]), 0, nx / 2 + 1));
            else if (kx != nx / 2) T.pairtab.push_back(make_int4(ja, jb, kx, 0));
        } else for (int ky = 0; ky < ny; ky++) {
            const int kym = (ny - ky) % ny;
            const bool self = kxm == kx && kym == ky;
            if (!self && (kxm < kx || (kxm == kx && kym < ky))) continue;         // the partner comes first: it owns the pair
            T.pairtab.push_back(make_int4(ja * ny + posy[ky], jb * ny + posy[kym], kx | (ky << 16), self ? 1 : 0));
        }
    }
    // neighbouring blocks of the column kernel should own neighbouring positions (they share the 128-B lines of the tile-major
    // array, and of the transposed one through the inverse row kernel's tiles)
    std::sort(T.pairtab.begin(), T.pairtab.end(), [](const int4 &a, const int4 &b) { return a.x < b.x; });
    (d3 ? S.nent : S.nblk_cols) = (int)T.pairtab.size();
    if (!d3 && S.nblk_cols != S.nxl / 2) return false;               // (cannot happen: the ownership order keeps kx and -kx together)
    if (ring) {
        // blocks of the two all-to-alls: one per (peer, pair, piece of the receiver, chunk) = w positions x ce elements, contiguous on
        // both sides (2^k extents: nx/16 positions x all rows / planes of the rank).  Forward W -> W2; backward the mirror, W2 -> W --
        // except behind the split column kernel: its phase 2 leaves the result in W (used as scratch in the layout of W2), and it
        // comes home into W2 (in the layout of W), which is where the inverse row kernel then reads
        const long long ce = d3 ? ny * cs : cs;
        const size_t bytes = sizeof(kcf) * (size_t)O.w * ce;
        for (int q = 0; q < I.P; q++)
            for (int p = 0; p < S.npair; p++)
                for (int i = 0; i < O.per; i++) for (int c = 0; c < nch; c++) {
                    const size_t mine_for_q = spec_a2a_src(O, nx, S.npair, ce, q, p, i, c);          // my rows of q's columns
                    const size_t from_q = spec_a2a_dst(O, S.npair, nch, ce, q, p, i, c);             // q's rows of my columns
                    T.a2a_fwd.push_back({ q, mine_for_q, from_q, bytes });
                    T.a2a_back.push_back({ q, from_q, mine_for_q, bytes });
                }
        S.a2a_back_from_w = S.cols_split != 0;
    }
    return true;
}
