"""CPU: which slab rank owns which spectral x position (ksfd_amd/csrc/spectral_plan.h), for power-of-two plans and for plans with a
leading radix-3 stage, and how the blocks of the all-to-all transposes tile the two work arrays.  The header is host-only, so a small
driver compiled with the host compiler runs exactly what spec_build runs; the few device-side names it mentions (the plan struct, the
vector types) are declared by the driver.

Every valid n = 2^k (32 ... 16384) and 3 * 2^k (48 ... 12288), P = 1, 2, 4, 8 (n/16 >= P always holds): P = 8 with a radix-3 stage is
the tightest case, 6 pieces per rank."""
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

/* today's map of the power-of-two plans, written out independently: the top radix-16 digit, dealt in spec_digit_order */
static const int digit_order[16] = { 0, 8, 1, 15, 2, 14, 3, 13, 4, 12, 5, 11, 6, 10, 7, 9 };

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (argv[1][0] == 'o') {
        /* own <n> <P>: one line per wavenumber k: position, owner, local index */
        const int n = atoi(argv[2]), P = atoi(argv[3]);
        KFFTPlan Q;
        SpecOwn O;
        if (!spec_plan(n, Q) || !spec_ownership(Q, P, O)) { printf("refused\n"); return 0; }
        printf("%d %d %d %d\n", O.npiece, O.w, O.per, Q.m);
        for (int k = 0; k < n; k++) { const int pos = spec_pos(Q, k); printf("%d %d %d\n", pos, spec_owner(O, pos), spec_local_index(O, pos)); }
        if (Q.m == 1) {
            const int nd = 16 / P, n16 = n / 16;
            for (int q = 0; q < P; q++) for (int di = 0; di < nd; di++) printf("%d %d %d\n", digit_order[q * nd + di] * n16, q, di * n16);      /* (first position, owner, local index) of a digit */
        }
        return 0;
    }
    /* a2a <nx> <ny> <P> <npair>: eligibility, then one line per block of the all-to-all: sender-side offset, receiver-side offset, elements */
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
    d = tmp_path_factory.mktemp('own')
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / 'drv'
    subprocess.run([cxx, '-x', 'c++', '-O1', '-std=c++17', '-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, check=True, timeout=60)
        return [[int(x) for x in line.split()] if line != 'refused' else None for line in r.stdout.splitlines()]
    return run


@pytest.mark.parametrize('n', POW2 + THREE)
def test_every_position_has_one_owner_and_partners_share_it(driver, n):
    for P in RANKS:
        out = driver('own', n, P)
        assert out[0] is not None, (n, P)
        npiece, w, per, m = out[0]
        assert m == (3 if n % 3 == 0 else 1) and npiece == 16 * m and npiece * w == n and per * P == npiece
        rows = out[1:1 + n]
        pos = [r[0] for r in rows]
        owner = [r[1] for r in rows]
        assert sorted(pos) == list(range(n))                              # the transform's output order is a permutation
        assert all(0 <= q < P for q in owner)
        # every rank owns n/P positions, stored once each at the local indices 0 .. n/P - 1
        for q in range(P):
            assert sorted(r[2] for r in rows if r[1] == q) == list(range(n // P)), (n, P, q)
        # k and -k on one rank; the two self-paired wavenumbers on rank 0
        assert all(owner[k] == owner[(n - k) % n] for k in range(n)), (n, P)
        assert owner[0] == 0 and owner[n // 2] == 0
        if m == 1:
            # unchanged for the power-of-two plans: owner and local index by the top digit in spec_digit_order
            digits = {r[0] // (n // 16): (r[1], r[2]) for r in out[1 + n:]}
            assert len(digits) == 16
            for p_, q, loc in rows:
                dq, dloc = digits[p_ // (n // 16)]
                assert (q, loc) == (dq, dloc + p_ % (n // 16)), (n, P, p_)


def test_rank_counts_outside_1_2_4_8_are_refused(driver):
    for P in (3, 5, 6, 16):
        assert driver('own', 96, P) == [None]
        assert driver('own', 64, P) == [None]


A2A_CASES = [(48, 64, 2, 1), (64, 96, 2, 1), (48, 48, 2, 2), (96, 192, 4, 2), (192, 48, 4, 1), (48, 48, 8, 1), (384, 384, 8, 2),
             (64, 64, 2, 1), (128, 64, 4, 2), (1536, 1536, 8, 2), (96, 96, 1, 1)]


@pytest.mark.parametrize('nx,ny,P,npair', A2A_CASES)
def test_alltoall_blocks_tile_both_work_arrays_exactly_once(driver, nx, ny, P, npair):
    out = driver('a2a', nx, ny, P, npair)
    assert out[0] is not None
    nch, cs, w, per = out[0]
    assert nch == (3 if ny % 3 == 0 else 1) and nch * cs * P == ny and cs & (cs - 1) == 0 and w * per * P == nx
    blocks = out[1:]
    assert len(blocks) == P * npair * per * nch
    total = npair * nx * (ny // P)                                        # elements of either work array of a rank
    for side in (0, 1):
        ivals = sorted((b[side], b[side] + b[2]) for b in blocks)
        assert ivals[0][0] == 0 and ivals[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(ivals, ivals[1:])), (nx, ny, P, side)
    # receiver side: sender r's chunk c is piece number r * nch + c of every column (piece stride npair * nxl * cs)
    nxl = nx // P
    k = 0
    for q in range(P):
        for p in range(npair):
            for i in range(per):
                for c in range(nch):
                    assert blocks[k][1] == (((q * nch + c) * npair + p) * nxl + i * w) * cs
                    k += 1


@pytest.mark.parametrize('nx,ny,P', [(48, 24, 8), (48, 96, 3), (48, 48, 16), (40, 48, 2), (48, 80, 2), (24, 48, 2), (48, 12, 2)])
def test_ineligible_slab_handles_are_refused(driver, nx, ny, P):
    """fewer than 4 local rows or an odd count, rank counts outside {1, 2, 4, 8}, extents that are neither 2^k nor 3 * 2^k or too short"""
    assert driver('a2a', nx, ny, P, 1) == [None]
