"""CPU: the shape planner of the spectral solver (ksfd_amd/csrc/spectral_plan.h: spec_shape) -- the tables the column and z kernels walk,
the LDS budgets and divisibility rules the launches rely on, the choice of the split column kernel, and the refusals.  As in
test_spectral_ownership_cpu.py a small driver compiled with the host compiler runs exactly what spec_build runs; the device-side names
the header mentions are declared by the driver (int4 by the header itself in a host-only build).  The checks are properties the kernels depend on, worked out here independently."""
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

static void print_shape(const SpecGrid &I, bool ok, const SpecShape &S)
{
    printf("%d %lld %lld %lld %d %d %d %lld %d  %d %d %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %d\n", I.dim, I.n[0], I.n[1], I.n[2], I.F, I.P, I.ring ? 1 : 0, I.sloc, ok ? 1 : 0,
           S.rb, S.lg_rb, S.nch, S.lg_cz, S.lg_pl, S.nyp, S.nxl, S.cols_split, S.pb, S.lds_rows, S.lds_cols, S.lds_y3, S.lds_z3, S.welems, S.need_w2 ? 1 : 0);
}

/* one axis: per wavenumber its position, the owner of that position and its local index there (one rank without a ring: the position itself) */
static void print_axis(long long n, int P, bool ring)
{
    KFFTPlan Q;
    SpecOwn O;
    if (!spec_plan(n, Q) || (ring && !spec_ownership(Q, P, O))) { printf("refused\n"); exit(0); }
    for (int k = 0; k < n; k++) { const int pos = spec_pos(Q, k); printf("%d %d %d\n", pos, ring ? spec_owner(O, pos) : 0, ring ? spec_local_index(O, pos) : pos); }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    SpecKnobs K;
    SpecShape S;
    SpecTables T;
    if (argv[1][0] == 't') {
        /* table <dim> <nx> <ny> <nz> <P> <ring>: the x axis (and in 3-D the y axis) as print_axis prints it, then per rank "nxl entries" and the table */
        const int dim = atoi(argv[2]), P = atoi(argv[6]);
        const bool ring = atoi(argv[7]) != 0;
        SpecGrid I = { dim, { atoll(argv[3]), atoll(argv[4]), atoll(argv[5]) }, 2, P, 0, ring, atoll(argv[2 + dim]) / P, ring ? 2 : 0 };
        print_axis(I.n[0], P, ring);
        if (dim == 3) print_axis(I.n[1], 1, false);
        for (I.rank = 0; I.rank < P; I.rank++) {
            if (!spec_shape(I, K, S, T)) { printf("refused\n"); return 0; }
            printf("%d %d %zu\n", S.nxl, dim == 3 ? S.nent : S.nblk_cols, T.pairtab.size());
            for (const int4 &e : T.pairtab) printf("%d %d %d %d\n", e.x, e.y, e.z, e.w);
        }
        return 0;
    }
    if (argv[1][0] == 'b') {
        /* budget <dim> <axis> <F> <other extent> <extents ...>: the shape of the last rank for every extent on that axis, P = 1 (no ring), 1, 2, 4, 8 (ring) */
        const int dim = atoi(argv[2]), axis = atoi(argv[3]), F = atoi(argv[4]);
        const long long other = atoll(argv[5]);
        for (int a = 6; a < argc; a++) for (int c = 0; c < 5; c++) {
            const int P = c == 0 ? 1 : 1 << (c - 1);
            SpecGrid I = { dim, { other, other, dim == 3 ? other : 1 }, F, P, P - 1, c > 0, 0, c > 0 ? 2 : 0 };
            I.n[axis] = atoll(argv[a]);
            I.sloc = I.n[dim - 1] / P;
            print_shape(I, spec_shape(I, K, S, T), S);
        }
        return 0;
    }
    /* shape <dim> <nx> <ny> <nz> <F> <P> <ring> <sloc> <ng> <split knob> */
    SpecGrid I = { atoi(argv[2]), { atoll(argv[3]), atoll(argv[4]), atoll(argv[5]) }, atoi(argv[6]), atoi(argv[7]), 0, atoi(argv[8]) != 0, atoll(argv[9]), atoi(argv[10]) };
    K.split = atoi(argv[11]);
    print_shape(I, spec_shape(I, K, S, T), S);
    return 0;
}
'''

POW2 = [1 << k for k in range(5, 15)]
THREE = [3 << k for k in range(4, 13)]
LAYOUTS = ((1, 0), (1, 1), (2, 1), (4, 1), (8, 1))                        # (ranks, ring): one rank in place, the ring of one, slab ranks
LDS_BUDGET = 160 * 1024 - 1024
SHAPE_FIELDS = ('dim nx ny nz F P ring sloc ok rb lg_rb nch lg_cz lg_pl nyp nxl cols_split pb lds_rows lds_cols lds_y3 lds_z3 welems need_w2').split()


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('hipcc') or (hipcc if os.path.exists(hipcc) else None)
    if not cxx:
        pytest.fail('no C++ compiler found (g++, c++, hipcc): the library cannot have been built either')
    d = tmp_path_factory.mktemp('shape')
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / 'drv'
    subprocess.run([cxx, '-x', 'c++', '-O2', '-std=c++17', '-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, check=True, timeout=60)
        return [[int(x) for x in line.split()] if line != 'refused' else None for line in r.stdout.splitlines()]
    return run


def _pow2(n):
    return n >= 1 and n & (n - 1) == 0


def _shapes(out):
    return [dict(zip(SHAPE_FIELDS, row)) for row in out]


@pytest.mark.parametrize('nx', POW2 + THREE)
def test_2d_pair_table_names_every_column_once_with_its_partner(driver, nx):
    for P, ring in LAYOUTS:
        out = driver('table', 2, nx, 64, 1, P, ring)
        assert None not in out, (nx, P, ring)
        axis, rest = out[:nx], out[nx:]
        pos, owner, local = ([r[i] for r in axis] for i in range(3))
        seen_kx = []
        for rank in range(P):
            nxl, nblk, count = rest[0]
            table, rest = rest[1:1 + count], rest[1 + count:]
            assert nxl == nx // P and nblk == count == nxl // 2, (nx, P, rank)
            assert [e[0] for e in table] == sorted(e[0] for e in table)
            assert sorted([e[0] for e in table] + [e[1] for e in table]) == list(range(nxl)), (nx, P, rank)
            for a, b, kx, w in table:
                if w:                                                     # the block of the two self-paired columns
                    assert (kx, w, rank) == (0, nx // 2 + 1, 0)
                    partner = nx // 2
                else:
                    assert 0 < kx < nx // 2
                    partner = nx - kx
                assert (owner[kx], owner[partner]) == (rank, rank) and (a, b) == (local[kx], local[partner]), (nx, P, rank, kx)
                seen_kx += [kx, partner]
        assert rest == [] and sorted(seen_kx) == list(range(nx)), (nx, P)
        assert sorted(pos) == list(range(nx))


@pytest.mark.parametrize('nx', [32, 48, 64, 96])
@pytest.mark.parametrize('ny', [32, 48, 64, 96])
def test_3d_entry_table_names_every_column_once_with_its_partner(driver, nx, ny):
    for P, ring in LAYOUTS:
        out = driver('table', 3, nx, ny, 32, P, ring)
        assert None not in out, (nx, ny, P, ring)
        xaxis, yaxis, rest = out[:nx], out[nx:nx + ny], out[nx + ny:]
        col = lambda kx, ky: xaxis[kx % nx][2] * ny + yaxis[ky % ny][0]   # noqa: E731  local column of a wavenumber pair on its owner
        named = []
        for rank in range(P):
            nxl, nent, count = rest[0]
            table, rest = rest[1:1 + count], rest[1 + count:]
            assert nxl == nx // P and nent == count
            assert [e[0] for e in table] == sorted(e[0] for e in table)
            nself = 0
            for a, b, k, self_flag in table:
                kx, ky = k & 0xffff, k >> 16
                assert xaxis[kx][1] == rank and xaxis[-kx % nx][1] == rank, (nx, ny, P, kx)
                assert (a, b) == (col(kx, ky), col(-kx, -ky)), (nx, ny, P, kx, ky)
                assert self_flag == (1 if (2 * kx) % nx == 0 and (2 * ky) % ny == 0 else 0)
                nself += self_flag
                named.append((kx, ky))
                if not self_flag:
                    named.append((-kx % nx, -ky % ny))
            assert 2 * nent - nself == nxl * ny, (nx, ny, P, rank)
            assert nself == (4 if rank == 0 else 0)
        assert rest == [] and sorted(named) == [(kx, ky) for kx in range(nx) for ky in range(ny)], (nx, ny, P)


@pytest.mark.parametrize('F', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('dim,axis', [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
def test_budgets_and_divisibility_of_every_accepted_shape(driver, dim, axis, F):
    """every valid extent on one axis (the others 48 in 2-D, 32 in 3-D); every shape the planner accepts must fit the LDS and divide evenly"""
    shapes = _shapes(driver('budget', dim, axis, F, 48 if dim == 2 else 32, *(POW2 + THREE)))
    assert len(shapes) == 5 * len(POW2 + THREE)
    if dim == 2:
        assert all(s['ok'] for s in shapes)                               # 2-D: every extent has a plan on 1, 2, 4, 8 ranks (n/16 >= P, >= 4 rows)
    assert sum(s['ok'] for s in shapes) >= len(shapes) // 2
    for s in shapes:
        if not s['ok']:
            continue
        key = tuple(s[k] for k in ('dim', 'nx', 'ny', 'nz', 'F', 'P', 'ring'))
        assert max(s['lds_rows'], s['lds_cols'], s['lds_y3'], s['lds_z3']) <= LDS_BUDGET, key
        assert s['lds_rows'] > 0 and (s['lds_cols'] > 0 if dim == 2 else s['lds_y3'] > 0 and s['lds_z3'] > 0), key
        rows = s['sloc'] if dim == 2 else s['ny'] * s['sloc']
        assert _pow2(s['rb']) and s['rb'] == 1 << s['lg_rb'] and rows % s['rb'] == 0, key
        assert s['nch'] in (1, 3) and s['sloc'] % s['nch'] == 0
        chunk = s['sloc'] // s['nch']                                     # rows (3-D: planes) of a chunk
        assert 1 << s['lg_pl'] >= chunk and (1 << s['lg_pl'] < 2 * chunk), key
        if s['ring']:
            assert 1 << s['lg_pl'] == chunk, key
        if dim == 3:
            assert s['ny'] % s['rb'] == 0 and chunk % (1 << s['lg_cz']) == 0 and s['pb'] >= 1, key
        assert s['nxl'] * s['P'] == s['nx']
        assert s['welems'] == (F + 1) // 2 * s['nx'] * s['nyp'] * s['nch'] and s['nyp'] >= (chunk if dim == 2 else s['ny'] * chunk), key


# 8 bytes per element of a column of 2^lg (+ 1/16 + 1) points, three of them behind a radix-3 stage (spec_sstride); a pair block of the
# plain column kernel holds 2 * npair columns, of the split kernel two, of the by-column split kernel one
def _col_bytes(ny):
    m = 3 if ny % 3 == 0 else 1
    return 8 * m * (ny // m + ny // m // 16 + 1)


@pytest.mark.parametrize('ny,F,split,lds_cols', [(8192, 2, 0, None), (8192, 3, 1, 139280), (16384, 2, 2, 139272), (12288, 2, 2, 104472),
                                                  (6144, 3, 1, 104496), (6144, 2, 0, None)])
def test_cols_split_follows_from_the_lds_budget(driver, ny, F, split, lds_cols):
    s, = _shapes(driver('shape', 2, 64, ny, 1, F, 1, 0, ny, 0, 0))
    npair = (F + 1) // 2
    assert s['ok'] and s['cols_split'] == split
    assert s['lds_cols'] == (lds_cols if split else 2 * npair * _col_bytes(ny)) == _col_bytes(ny) * (2 * npair, 2, 1)[split] <= LDS_BUDGET
    if split:
        assert _col_bytes(ny) * (2 * npair, 2, 1)[split - 1] > LDS_BUDGET            # the next larger block does not fit
        assert s['need_w2']


@pytest.mark.parametrize('F,knob,split', [(2, 1, 0), (3, 1, 1), (2, 2, 2), (3, 2, 2), (2, 0, 0)])
def test_split_knob(driver, F, knob, split):
    s, = _shapes(driver('shape', 2, 64, 128, 1, F, 1, 0, 128, 0, knob))
    assert s['ok'] and s['cols_split'] == split
    assert s['lds_cols'] == _col_bytes(128) * (2 * ((F + 1) // 2), 2, 1)[split]


# (dim, nx, ny, nz, F, P, ring, sloc, ng): a refused grid, each next to an accepted neighbour that differs in the one thing refused
REFUSED = [
    ('slab rank with fewer than 4 local rows', (2, 64, 32, 1, 2, 8, 1, 2, 2), (2, 64, 32, 1, 2, 8, 1, 4, 2)),
    ('3 local rows: a chunk of one', (2, 64, 48, 1, 2, 8, 1, 3, 2), (2, 64, 48, 1, 2, 8, 1, 6, 2)),
    ('rows of a chunk not a power of two', (2, 64, 64, 1, 2, 2, 1, 24, 2), (2, 64, 64, 1, 2, 2, 1, 32, 2)),
    ('rows of a chunk not a power of two, three chunks', (2, 64, 96, 1, 2, 2, 1, 36, 2), (2, 64, 96, 1, 2, 2, 1, 48, 2)),
    ('3-D: nzl * P != nz', (3, 32, 32, 64, 2, 2, 1, 16, 2), (3, 32, 32, 64, 2, 2, 1, 32, 2)),
    ('3-D, one rank without a ring but with ghost planes', (3, 32, 32, 32, 2, 1, 0, 32, 2), (3, 32, 32, 32, 2, 1, 0, 32, 0)),
    ('three ranks', (2, 96, 96, 1, 2, 3, 1, 32, 2), (2, 96, 96, 1, 2, 2, 1, 48, 2)),
    ('three ranks, 3-D', (3, 48, 32, 96, 2, 3, 1, 32, 2), (3, 48, 32, 96, 2, 4, 1, 24, 2)),
    ('nx = 40 has no plan', (2, 40, 64, 1, 2, 1, 0, 64, 0), (2, 48, 64, 1, 2, 1, 0, 64, 0)),
    ('ny = 480 has no plan', (2, 64, 480, 1, 2, 1, 0, 480, 0), (2, 64, 384, 1, 2, 1, 0, 384, 0)),
    ('nz = 40 has no plan', (3, 32, 32, 40, 2, 1, 0, 40, 0), (3, 32, 32, 48, 2, 1, 0, 48, 0)),
    ('ny = 480 has no plan, 3-D', (3, 32, 480, 32, 2, 1, 0, 32, 0), (3, 32, 384, 32, 2, 1, 0, 32, 0)),
    ('1-D', (1, 64, 1, 1, 2, 1, 0, 64, 0), (2, 64, 64, 1, 2, 1, 0, 64, 0)),
]


@pytest.mark.parametrize('why,refused,accepted', REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_stay_refusals(driver, why, refused, accepted):
    assert _shapes(driver('shape', *refused, 0))[0]['ok'] == 0, why
    assert _shapes(driver('shape', *accepted, 0))[0]['ok'] == 1, why
