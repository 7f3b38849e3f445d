"""CPU: the slab-rank plan of the 3-D spectral solver (ksfd_amd/csrc/spectral_plan.h: spec_slab3_eligible, spec_a2a3_src / _dst), and
the 2-D two-phase column path on slab ranks with 3 * 2^k extents (three chunks, the roles of the two work arrays swapped on the way
home).  As in test_spectral_ownership_cpu.py a small driver compiled with the host compiler runs exactly what spec_build3d / spec_build
run; the device-side names the header mentions are declared by the driver.

3-D layout under test: sender W[chunk][pair][pos_x][pos_y][plane in chunk], receiver W2[sender * nch + chunk][pair][own pos_x][pos_y]
[plane in chunk]; a block is (peer, pair, piece of the receiver, chunk) = w x-positions x ny x cs planes."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
struct float2 { float x, y; };
struct int2 { int x, y; };
static float2 make_float2(float x, float y) { float2 r = { x, y }; return r; }
static int2 make_int2(int x, int y) { int2 r = { x, y }; return r; }
typedef float2 kcf;
#define KSPEC_MAXSTAGE 7
struct KFFTPlan { int n, lg, nstage, m; int radix[KSPEC_MAXSTAGE]; int flags, lgw; };
#include "spectral_plan.h"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (argv[1][0] == 'e') {
        /* elig <nx>: one line "nz P nzl ok nch" per (nz, P, nzl) with nz over the extents given after nx, P = 1..8, nzl = nz / P where
           P | nz; and one line with a wrong nzl (P * nzl != nz) per (nz, P) */
        const int nx = atoi(argv[2]);
        KFFTPlan px, pz;
        if (!spec_plan(nx, px)) { printf("refused\n"); return 0; }
        for (int a = 3; a < argc; a++) {
            const int nz = atoi(argv[a]);
            if (!spec_plan(nz, pz)) { printf("refused\n"); return 0; }
            for (int P = 1; P <= 8; P++) {
                SpecOwn O;
                int nch = 0;
                if (nz % P == 0) { const bool ok = spec_slab3_eligible(px, pz, P, nz / P, O, nch); printf("%d %d %d %d %d\n", nz, P, nz / P, ok ? 1 : 0, ok ? nch : 0); }
                const bool ok = spec_slab3_eligible(px, pz, P, nz / P + 2, O, nch);
                printf("%d %d %d %d %d\n", nz, P, nz / P + 2, ok ? 1 : 0, 0);
            }
        }
        return 0;
    }
    if (argv[1][0] == 'z') {
        /* zblocks <nx> <ny> <nz> <P> <npair>: "nch cs w per", then per block: sender offset, receiver offset, elements */
        const int nx = atoi(argv[2]), ny = atoi(argv[3]), nz = atoi(argv[4]), P = atoi(argv[5]), npair = atoi(argv[6]);
        KFFTPlan px, py, pz;
        SpecOwn O;
        int nch = 0;
        if (!spec_plan(nx, px) || !spec_plan(ny, py) || !spec_plan(nz, pz) || nz % P || !spec_slab3_eligible(px, pz, P, nz / P, O, nch)) { printf("refused\n"); return 0; }
        const long long cs = nz / P / nch;
        printf("%d %lld %d %d\n", nch, cs, O.w, O.per);
        for (int q = 0; q < P; q++) for (int p = 0; p < npair; p++) for (int i = 0; i < O.per; i++) for (int c = 0; c < nch; c++)
            printf("%zu %zu %lld\n", spec_a2a3_src(O, nx, ny, npair, cs, q, p, i, c), spec_a2a3_dst(O, ny, npair, nch, cs, q, p, i, c), (long long)O.w * ny * cs);
        return 0;
    }
    if (argv[1][0] == 'c') {
        /* cols3 <nx> <ny> <P> <rank>: "w per nxl", then per wavenumber pair (kx, ky) of a sample: owner and local column
           (local pos_x * ny + pos_y) of (kx, ky) and of (-kx, -ky) */
        const int nx = atoi(argv[2]), ny = atoi(argv[3]), P = atoi(argv[4]);
        KFFTPlan px, py;
        SpecOwn O;
        if (!spec_plan(nx, px) || !spec_plan(ny, py) || !spec_ownership(px, P, O)) { printf("refused\n"); return 0; }
        printf("%d %d %d\n", O.w, O.per, O.per * O.w);
        for (int kx = 0; kx < nx; kx += (nx > 256 ? 37 : 1)) for (int ky = 0; ky < ny; ky += (ny > 64 ? ny / 16 - 1 : 5)) {
            const int a = spec_pos(px, kx), b = spec_pos(px, (nx - kx) % nx);
            printf("%d %d %d %d %d %d\n", kx, ky, spec_owner(O, a), spec_local_index(O, a) * ny + spec_pos(py, ky),
                   spec_owner(O, b), spec_local_index(O, b) * ny + spec_pos(py, (ny - ky) % ny));
        }
        return 0;
    }
    /* yblocks <nx> <ny> <P> <npair>: the 2-D blocks (spec_slab_eligible, spec_a2a_src / _dst) as test_spectral_ownership_cpu.py prints them */
    const int nx = atoi(argv[2]), ny = atoi(argv[3]), P = atoi(argv[4]), npair = atoi(argv[5]);
    KFFTPlan px, py;
    SpecOwn O;
    int nch = 0;
    if (!spec_plan(nx, px) || !spec_plan(ny, py) || ny % P || !spec_slab_eligible(px, py, P, ny / P, O, nch)) { printf("refused\n"); return 0; }
    const long long cs = ny / P / nch;
    printf("%d %lld %d %d\n", nch, cs, O.w, O.per);
    for (int q = 0; q < P; q++) for (int p = 0; p < npair; p++) for (int i = 0; i < O.per; i++) for (int c = 0; c < nch; c++)
        printf("%zu %zu %lld\n", spec_a2a_src(O, nx, npair, cs, q, p, i, c), spec_a2a_dst(O, npair, nch, cs, q, p, i, c), (long long)O.w * cs);
    return 0;
}
'''

POW2 = [1 << k for k in range(5, 15)]
THREE = [3 << k for k in range(4, 13)]
RANKS = (1, 2, 4, 8)


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('hipcc') or (hipcc if os.path.exists(hipcc) else None)
    if not cxx:
        pytest.fail('no C++ compiler found (g++, c++, hipcc): the library cannot have been built either')
    d = tmp_path_factory.mktemp('own3')
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / 'drv'
    subprocess.run([cxx, '-x', 'c++', '-O1', '-std=c++17', '-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, check=True, timeout=60)
        return [[int(x) for x in line.split()] if line != 'refused' else None for line in r.stdout.splitlines()]
    return run


def _pow2(n):
    return n >= 1 and n & (n - 1) == 0


def _element_maps(blocks):
    """offset on the sender -> offset on the receiver, element by element"""
    fwd = {}
    for src, dst, n in blocks:
        for e in range(n):
            fwd[src + e] = dst + e
    return fwd


def _expect_eligible(nz, P, nzl):
    """the rule of the issue, written out independently: P in {1, 2, 4, 8}, P | nz, nz/P = 2^j or 3 * 2^j, chunk >= 2"""
    if P not in RANKS or nzl * P != nz:
        return 0
    if _pow2(nzl):
        return 1 if nzl >= 2 else 0
    if nzl % 3 == 0 and _pow2(nzl // 3):
        return 3 if nzl // 3 >= 2 else 0
    return 0


@pytest.mark.parametrize('nx', [32, 48])
def test_3d_eligibility_is_exactly_the_rule(driver, nx):
    """every valid nz, P = 1 ... 8 (3, 5, 6, 7 refused), matching and non-matching local plane counts"""
    out = driver('elig', nx, *(POW2 + THREE))
    assert None not in out
    seen = set()
    for nz, P, nzl, ok, nch in out:
        want = _expect_eligible(nz, P, nzl)
        assert (ok, nch) == ((1, want) if want else (0, 0)), (nz, P, nzl)
        seen.add((nz, P, nzl * P == nz))
    for nz in POW2 + THREE:
        for P in RANKS:
            assert (nz, P, True) in seen and (nz, P, False) in seen
    # every valid extent on 1, 2, 4, 8 ranks has at least 2 planes per chunk: the rule refuses none of them
    assert all(_expect_eligible(nz, P, nz // P) for nz in POW2 + THREE for P in RANKS)
    assert _expect_eligible(48, 3, 16) == 0 and [48, 3, 16, 0, 0] in out


def test_3d_extents_without_a_plan_and_other_rank_counts_are_refused(driver):
    for args in [(48, 32, 40, 2, 1), (40, 32, 48, 2, 1), (48, 32, 48, 3, 1), (48, 32, 96, 16, 1), (24, 32, 48, 2, 1), (48, 32, 24, 2, 1)]:
        assert driver('zblocks', *args) == [None], args


BLOCK3_CASES = [(48, 32, 32, 2, 1), (32, 48, 32, 2, 1), (32, 32, 48, 2, 1), (48, 48, 96, 4, 2), (96, 32, 48, 4, 1), (48, 32, 48, 1, 1),
                (64, 64, 64, 2, 1), (32, 32, 32, 8, 1), (48, 48, 48, 8, 2), (384, 48, 384, 8, 1), (96, 64, 192, 1, 2)]


@pytest.mark.parametrize('nx,ny,nz,P,npair', BLOCK3_CASES)
def test_3d_alltoall_blocks_tile_both_work_arrays_exactly_once(driver, nx, ny, nz, P, npair):
    out = driver('zblocks', nx, ny, nz, P, npair)
    assert out[0] is not None
    nch, cs, w, per = out[0]
    assert nch == (3 if nz % 3 == 0 else 1) and nch * cs * P == nz and _pow2(cs) and cs >= 2 and w * per * P == nx
    blocks = out[1:]
    assert len(blocks) == P * npair * per * nch
    assert all(b[2] == w * ny * cs for b in blocks)
    total = npair * nx * ny * (nz // P)                                   # elements of either work array of a rank
    for side in (0, 1):                                                   # a bijection: no gap, no overlap, on the sender and on the receiver
        ivals = sorted((b[side], b[side] + b[2]) for b in blocks)
        assert ivals[0][0] == 0 and ivals[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(ivals, ivals[1:])), (nx, ny, nz, P, side)
    # the backward all-to-all is the mirror: spec_build3d sends block k from its receiver-side offset (in W2) back to its sender-side
    # offset (in W).  Mirrored, the blocks tile both arrays once as well, and the round trip puts every element back where it was.
    home = [(b[1], b[0], b[2]) for b in blocks]
    for side in (0, 1):
        ivals = sorted((b[side], b[side] + b[2]) for b in home)
        assert ivals[0][0] == 0 and ivals[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(ivals, ivals[1:])), (nx, ny, nz, P, side)
    if total <= 1 << 18:
        fwd, back = _element_maps(blocks), _element_maps(home)
        assert len(fwd) == total and sorted(fwd.values()) == list(range(total))
        assert all(back[fwd[e]] == e for e in range(total))
    # sender: block (q, p, i, c) starts at a piece of w whole x positions of chunk c's array [pair][pos_x][pos_y][plane in chunk]
    nxl = nx // P
    pstride = npair * nxl * ny * cs
    k = 0
    starts = set()
    for q in range(P):
        for p in range(npair):
            for i in range(per):
                for c in range(nch):
                    src, dst, _ = blocks[k]
                    k += 1
                    chunk, rest = divmod(src, npair * nx * ny * cs)
                    pair, rest = divmod(rest, nx * ny * cs)
                    assert (chunk, pair) == (c, p) and rest % (w * ny * cs) == 0
                    starts.add((q, rest // (ny * cs)))
                    # receiver: sender q's chunk c is piece number q * nch + c of every owned column, all pieces one stride apart
                    assert dst == (q * nch + c) * pstride + (p * nxl + i * w) * ny * cs
    # the x positions a rank sends to q are the same for every pair and chunk, and all P peers together get every position once
    assert sorted(s for _, s in starts) == [j * w for j in range(nx // w)]


@pytest.mark.parametrize('nx,ny,P', [(48, 32, 2), (96, 48, 4), (48, 48, 8), (32, 48, 2), (384, 96, 8), (12288, 32, 8), (6144, 48, 4)])
def test_3d_column_pairs_stay_on_one_rank_with_distinct_local_columns(driver, nx, ny, P):
    """(kx, ky) and (-kx, -ky) have one owner; local column numbers are below nxl * ny and distinct unless the column is its own partner"""
    out = driver('cols3', nx, ny, P, 0)
    assert out[0] is not None
    w, per, nxl = out[0]
    assert nxl * P == nx
    for kx, ky, qa, ca, qb, cb in out[1:]:
        assert qa == qb, (kx, ky)
        assert 0 <= ca < nxl * ny and 0 <= cb < nxl * ny
        self_paired = (2 * kx) % nx == 0 and (2 * ky) % ny == 0
        assert (ca == cb) == self_paired, (kx, ky)
        if self_paired:
            assert qa == 0                                                # kx = 0 and kx = nx/2 lead the ownership order


@pytest.mark.parametrize('nx,ny,P,npair', [(64, 96, 2, 2), (96, 64, 2, 2), (96, 192, 4, 2), (48, 96, 2, 1), (48, 96, 1, 2), (6144, 6144, 8, 2), (48, 12288, 8, 1)])
def test_2d_split_path_three_chunks_and_the_swapped_arrays_on_the_way_home(driver, nx, ny, P, npair):
    """The two-phase column kernel on slab ranks: forward W -> W2 as for the plain kernel; phase 2 leaves its result in W used in the
    LAYOUT of W2, and it comes home into W2 in the LAYOUT of W (spec_build: send from W + (dst offset), receive at W2 + (src offset)).
    So the home trip must be the exact inverse of the forward map, block by block, and every column the split kernel addresses is
    nch * P pieces of cs = 2^lg_pl elements at one stride."""
    out = driver('yblocks', nx, ny, P, npair)
    assert out[0] is not None
    nch, cs, w, per = out[0]
    assert nch == (3 if ny % 3 == 0 else 1) and nch * cs * P == ny and _pow2(cs) and cs >= 2
    blocks = out[1:]
    nxl = nx // P
    total = npair * nx * (ny // P)
    pstride = npair * nxl * cs
    # home: block k is sent from offset dst_k (in W) and received at offset src_k (in W2)
    home = [(b[1], b[0], b[2]) for b in blocks]
    for side in (0, 1):
        ivals = sorted((b[side], b[side] + b[2]) for b in home)
        assert ivals[0][0] == 0 and ivals[-1][1] == total and all(a[1] == b[0] for a, b in zip(ivals, ivals[1:]))
    if total <= 1 << 16:
        fwd, back = _element_maps(blocks), _element_maps(home)
        assert all(back[fwd[e]] == e for e in range(total))
    # the piece (y >> lg_pl) of column (pair p, own position jl) as k_spec_cols_split's colat addresses it is where the block of
    # (sender y / (nch * cs), chunk (y / cs) % nch) put it
    k = 0
    for q in range(P):
        for p in range(npair):
            for i in range(per):
                for c in range(nch):
                    piece = q * nch + c
                    assert blocks[k][1] == piece * pstride + ((p * nxl + i * w) * cs) and blocks[k][2] == w * cs
                    k += 1
    assert cs % 2 == 0                                                    # a float4 (two elements from an even y) never straddles two pieces
