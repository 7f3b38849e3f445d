"""CPU: the level list of the multigrid hierarchy on slab ranks with coarse-level agglomeration (ksfd_set_mg_agglomerate) is a pure
function of (dim, global extents, ranks, max_points) in ksfd_amd/csrc/mg_agglomerate_plan.h (plain C++: the small driver below compiles
with the host compiler alone).  Checked here: its distributed prefix is the list of the slab rule mg_build has always applied, restated
in Python; with agglomeration on, the global extents are those of the single-rank hierarchy whenever every distributed level has even
local rows; the named cases of the production grids; the option flag parses into what KSFDHip.set_mg_agglomerate takes."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from ksfd_amd import lib as klib
from ksfd_amd import options as ko_opts

DRIVER = r'''
#include "mg_agglomerate_plan.h"
#include <stdio.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncases;
    if (fscanf(f, "%d", &ncases) != 1) return 3;
    for (int k = 0; k < ncases; k++) {
        int dim, ranks, ring; long long n[3] = { 1, 1, 1 }, maxp;
        if (fscanf(f, "%d %lld %lld %lld %d %d %lld", &dim, &n[0], &n[1], &n[2], &ranks, &ring, &maxp) != 7) return 3;
        ksfd_ctl::MGPlanLevel lev[64];
        const int nl = ksfd_ctl::mg_agglomerate_plan(dim, n, ranks, ring, maxp, lev, 64);
        printf("%d", nl);
        for (int l = 0; l < nl; l++) printf(" %lld %lld %lld %lld %d", lev[l].n[0], lev[l].n[1], lev[l].n[2], lev[l].sloc, lev[l].rep);
        printf("\n");
    }
    fclose(f);
    return 0;
}
'''


def slab_rule(shape, ranks, ring):
    """what mg_build does without agglomeration, restated: [(global extents, local slow units)]; the slow axis is the last one"""
    n = list(shape)
    rows = n[-1] // ranks
    out = [(tuple(n), rows)]
    while True:
        inner_ok = all(x % 2 == 0 and x // 2 >= 8 for x in n[:-1])
        if not inner_ok or rows % 2 or rows * ranks // 2 < 8 or (ring and rows // 2 < 4):
            return out
        n = [x // 2 for x in n]
        rows //= 2
        out.append((tuple(n), rows))


def single_rule(shape):
    n = list(shape)
    out = [tuple(n)]
    while all(x % 2 == 0 and x // 2 >= 8 for x in n):
        n = [x // 2 for x in n]
        out.append(tuple(n))
    return out


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('hipcc') or (hipcc if os.path.exists(hipcc) else None)
    if not cxx:
        pytest.fail('no C++ compiler found (g++, c++, hipcc): the library cannot have been built either')
    d = tmp_path_factory.mktemp('mgagg')
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / 'drv'
    subprocess.run([cxx, '-x', 'c++', '-O1', '-std=c++17', '-Wall', '-Werror', '-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(cases):
        """cases: (shape, ranks, ring, max_points) -> per case [(global extents, sloc, rep)], or None where the plan refuses"""
        inp = d / 'cases.txt'
        with open(inp, 'w') as f:
            f.write('%d\n' % len(cases))
            for shape, ranks, ring, maxp in cases:
                n = list(shape) + [1] * (3 - len(shape))
                f.write('%d %d %d %d %d %d %d\n' % (len(shape), n[0], n[1], n[2], ranks, ring, maxp))
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, check=True, timeout=60)
        out = []
        for (shape, _, _, _), line in zip(cases, r.stdout.splitlines()):
            v = [int(x) for x in line.split()]
            if v[0] < 0:
                out.append(None)
                continue
            assert len(v) == 1 + 5 * v[0]
            out.append([(tuple(v[1 + 5 * l:1 + 5 * l + len(shape)]), v[4 + 5 * l], v[5 + 5 * l]) for l in range(v[0])])
        assert len(out) == len(cases)
        return out
    return run


SHAPES = [(64, 64), (64, 96), (96, 64), (256, 64), (48, 40), (4096, 4096), (1536, 1536), (384, 384), (40, 24), (33, 20), (64, 20), (16, 16), (32, 16),
          (64, 64, 64), (512, 512, 512), (32, 32, 96), (24, 24, 24), (16, 16, 16), (96,), (256,)]
RANKS = (1, 2, 3, 4, 8, 16)
MAXP = (0, 1, 64, 300, 5000, 10 ** 9)


def _sweep():
    return [(shape, P, ring, maxp) for shape, P, ring, maxp in itertools.product(SHAPES, RANKS, (0, 1), MAXP)
            if shape[-1] % P == 0 and (ring or P == 1)]


def test_distributed_prefix_is_the_slab_rule(driver):
    cases = _sweep()
    got = driver(cases)
    nrep = 0
    for (shape, P, ring, maxp), lev in zip(cases, got):
        today = slab_rule(shape, P, ring)
        dist = [(n, s) for n, s, rep in lev if not rep]
        assert dist == today[:len(dist)] and len(dist) >= 1, (shape, P, ring, maxp, lev)
        reps = [rep for _, _, rep in lev]
        assert reps == sorted(reps)                                   # replicated levels form the tail
        if maxp == 0 or not ring or len(shape) == 1:
            assert dist == today and not any(reps), (shape, P, ring, maxp, lev)      # off, no transport, 1-D: today's list
        for l, (n, s, rep) in enumerate(lev):
            if rep:
                assert l >= 1 and s == n[-1]                          # whole level on every rank, never level 0
                # replicated where the slab rule refuses the level, or by its global size
                pts = 1
                for x in n:
                    pts *= x
                assert pts <= maxp or len(dist) == len(today), (shape, P, maxp, lev)
            elif l >= 1 and ring and maxp > 0 and len(shape) > 1:
                pts = 1
                for x in n:
                    pts *= x
                assert pts > maxp, (shape, P, maxp, lev)              # a level small enough is never left distributed
        nrep += any(reps)
    assert nrep > 50


def test_global_extents_are_the_single_rank_hierarchy(driver):
    cases = [c for c in _sweep() if c[2] and c[3] > 0 and len(c[0]) > 1]
    got = driver(cases)
    checked = 0
    for (shape, P, ring, maxp), lev in zip(cases, got):
        # a distributed level with odd local rows ends the hierarchy as it always did: its slabs do not start on coarse rows
        if any(s % 2 for _, s, rep in lev if not rep):
            continue
        assert [n for n, _, _ in lev] == single_rule(shape), (shape, P, maxp, lev)
        checked += 1
    assert checked > 100


def test_named_cases(driver):
    g = driver([((4096, 4096), 8, 1, 1), ((512, 512, 512), 8, 1, 1), ((1536, 1536), 16, 1, 1), ((64, 64), 2, 1, 1), ((64, 64), 2, 1, 300),
                ((64, 96), 3, 1, 1), ((64, 96), 3, 1, 96), ((64, 64), 4, 1, 1), ((64, 64, 64), 4, 1, 1), ((4096, 4096), 8, 1, 0)])
    assert g[0][-1] == ((8, 8), 8, 1) and [n[0] for n, _, rep in g[0] if rep] == [16, 8] and g[0][7] == ((32, 32), 4, 0)
    assert g[1][-1] == ((8, 8, 8), 8, 1) and [n[0] for n, _, rep in g[1] if rep] == [16, 8]
    assert g[2][-1] == ((12, 12), 12, 1) and [n[0] for n, _, rep in g[2] if rep] == [48, 24, 12] and g[2][4] == ((96, 96), 6, 0)
    assert g[3] == [((64, 64), 32, 0), ((32, 32), 16, 0), ((16, 16), 8, 0), ((8, 8), 4, 0)]       # the global rule stops first
    assert g[4] == [((64, 64), 32, 0), ((32, 32), 16, 0), ((16, 16), 16, 1), ((8, 8), 8, 1)]
    # (64, 96) on 3 ranks: 32, 16, 8, 4 local rows, all allowed; the global rule ends at (8, 12); 96 points replicate that level alone
    assert g[5] == [((64, 96), 32, 0), ((32, 48), 16, 0), ((16, 24), 8, 0), ((8, 12), 4, 0)]
    assert g[6] == [((64, 96), 32, 0), ((32, 48), 16, 0), ((16, 24), 8, 0), ((8, 12), 12, 1)]
    assert g[7] == [((64, 64), 16, 0), ((32, 32), 8, 0), ((16, 16), 4, 0), ((8, 8), 8, 1)]
    assert g[8] == [((64, 64, 64), 16, 0), ((32, 32, 32), 8, 0), ((16, 16, 16), 4, 0), ((8, 8, 8), 8, 1)]
    assert g[9][-1] == ((32, 32), 4, 0) and len(g[9]) == 8                                     # off: today's 32^2


def test_refused_arguments(driver):
    assert driver([((64, 64), 3, 1, 1), ((64, 64), 2, 1, -1), ((64, 64), 0, 1, 1)]) == [None, None, None]


BASE = ['-ts_type', 'rosw', '-ts_adapt_type', 'basic', '-ksp_rtol', '1e-8', '-ksfd_pc_type', 'mg', '-pc_type', 'lu']


def test_flag_parses_into_max_points():
    m = ko_opts.mg_agglomerate_from
    assert m(BASE + ['-ksfd_mg_agglomerate', '1']) == 1
    assert m(['-ksfd_mg_agglomerate', '4096'] + BASE) == 4096
    assert m(BASE + ['-ksfd_mg_agglomerate', '0']) == 0
    assert m(BASE) is None and m([]) is None
    assert m(BASE + ['-ksfd_mg_coarse', 'lu']) is None and ko_opts.mg_coarse_from(BASE + ['-ksfd_mg_agglomerate', '1']) is None


@pytest.mark.parametrize('bad', [['-ksfd_mg_agglomerate'], ['-ksfd_mg_agglomerate', '-1'], ['-ksfd_mg_agglomerate', 'on'], ['-ksfd_mg_agglomerate', '1e3'],
                                 ['-ksfd_mg_agglomerate', '2.5'], ['-ksfd_mg_agglomerate', str(2 ** 63)], ['-ksfd_mg_agglomerates', '1', '-ksfd_mg_agglomerate', 'x']])
def test_bad_values_raise(bad):
    with pytest.raises(ValueError):
        ko_opts.mg_agglomerate_from(BASE + bad)


def test_existing_flags_return_what_they_did():
    ps = ko_opts.Params(ko_opts.parse_commandline(['dim=1', 'nelements=16']))
    raw = lambda o: bytes(ctypes.string_at(ctypes.addressof(o), ctypes.sizeof(o)))
    plain = ko_opts.step_opts_from(ps, BASE)
    withflag = ko_opts.step_opts_from(ps, BASE[:4] + ['-ksfd_mg_agglomerate', '1'] + BASE[4:])
    assert raw(plain) == raw(withflag) and plain.pc_type == 1
    assert ko_opts.deflation_from(BASE + ['-ksfd_mg_agglomerate', '1']) is None


def test_header_binding_and_library_have_the_new_symbol():
    txt = open(os.path.join(ROOT, 'include', 'ksfd_hip.h')).read()
    assert re.search(r'\bint\s+ksfd_set_mg_agglomerate\s*\(\s*ksfd_handle\s*\*\s*h\s*,\s*int64_t\s+max_points\s*\)', txt)
    assert 'ksfd_set_mg_agglomerate' in klib.ABI_SYMBOLS
    if not os.path.exists(klib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(ctypes.CDLL(klib.LIB_PATH), 'ksfd_set_mg_agglomerate')
    assert callable(klib.KSFDHip.set_mg_agglomerate)
