"""CPU: the host side of the coarse tail of the multigrid V cycle (ksfd_set_mg_tail).  Which levels run as one workgroup launch is a pure
function of the level sizes, which levels are whole on the rank, F, the level the cycle ends on, max_points and the LDS budget
(ksfd_amd/csrc/mg_tail_plan.h, plain C++: the small driver below compiles with the host compiler alone).  It is checked against a
restatement of its rule written here, on the worked examples of the design and on the edges of the budget and of max_points; the
option flag parses like -ksfd_mg_agglomerate; the new symbols are in the header, the binding and the built library.

Per-level formula (the header's, unchanged from the design): 8 * points * (4 F + 1) bytes -- x, b, r, d of F planes each and one dG
plane in fp64.  Budget 163 840 bytes, at most 8 levels."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from ksfd_amd import lib as klib
from ksfd_amd import options as ko_opts

BUDGET = 163840
MAX_LEVELS = 8

DRIVER = r'''
#include "mg_tail_plan.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncases;
    if (fscanf(f, "%d", &ncases) != 1) return 3;
    printf("%lld %d %d\n", ksfd_ctl::MG_TAIL_LDS_BUDGET, ksfd_ctl::MG_TAIL_MAX_LEVELS, ksfd_ctl::MG_TAIL_THREADS);
    for (int k = 0; k < ncases; k++) {
        int F, end, nlevels, local[64]; long long maxp, budget, pts[64];
        if (fscanf(f, "%d %d %lld %lld %d", &F, &end, &maxp, &budget, &nlevels) != 5 || nlevels > 64) return 3;
        for (int l = 0; l < nlevels; l++) if (fscanf(f, "%lld %d", &pts[l], &local[l]) != 2) return 3;
        long long lds = -7;
        const int t = ksfd_ctl::mg_tail_first_level(pts, local, end, F, maxp, budget, &lds);
        printf("%d %lld %lld %d\n", t, lds, ksfd_ctl::mg_tail_max_points(F, budget), ksfd_ctl::mg_tail_points_per_thread(F));
    }
    return 0;
}
'''


def _prod(n):
    p = 1
    for x in n:
        p *= x
    return p


def hierarchy(shape):
    """points per level as mg_build makes them on one rank: halve every extent while all are even and stay >= 8"""
    n = list(shape)
    out = [_prod(n)]
    while all(x % 2 == 0 and x // 2 >= 8 for x in n):
        n = [x // 2 for x in n]
        out.append(_prod(n))
    return out


def level_bytes(points, F):
    return 8 * points * (4 * F + 1)


def tail_rule(points, local, end, F, maxp, budget):
    """the rule of the design, restated: the smallest t >= 1 such that every level t .. end is local, has <= max_points points, the sum of
    the level bytes fits the budget, and there are at most MAX_LEVELS of them"""
    if end < 1 or F < 1 or maxp <= 0:
        return -1, 0
    for t in range(1, end + 1):
        lv = range(t, end + 1)
        total = sum(level_bytes(points[l], F) for l in lv)
        if all(local[l] and 1 <= points[l] <= maxp for l in lv) and total <= budget and len(lv) <= MAX_LEVELS:
            return t, total
    return -1, 0


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('hipcc') or (hipcc if os.path.exists(hipcc) else None)
    if not cxx:
        pytest.fail('no C++ compiler found (g++, c++, hipcc): the library cannot have been built either')
    d = tmp_path_factory.mktemp('mgtail')
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / 'drv'
    subprocess.run([cxx, '-x', 'c++', '-O1', '-std=c++17', '-Wall', '-Werror', '-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(cases):
        """cases: (points, local, end, F, max_points, budget) -> [(t, lds_bytes, max points of a level, points per thread)]"""
        inp = d / 'cases.txt'
        with open(inp, 'w') as f:
            f.write('%d\n' % len(cases))
            for points, local, end, F, maxp, budget in cases:
                f.write('%d %d %d %d %d %s\n' % (F, end, maxp, budget, len(points), ' '.join('%d %d' % (p, int(q)) for p, q in zip(points, local))))
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, check=True, timeout=60)
        rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert rows[0] == (BUDGET, MAX_LEVELS, 1024)
        return rows[1:]
    return run


def one(points, F, maxp, local=None, end=None, budget=BUDGET):
    return (points, local if local is not None else [1] * len(points), len(points) - 1 if end is None else end, F, maxp, budget)


def test_worked_examples(driver):
    """the table of the design: hierarchy, max_points, F -> tail levels and LDS bytes"""
    h4096, h384, h512c, h96 = hierarchy((4096, 4096)), hierarchy((384, 384)), hierarchy((512, 512, 512)), hierarchy((96,))
    assert h4096[-3:] == [32 * 32, 16 * 16, 8 * 8] and h384[-3:] == [48 * 48, 24 * 24, 12 * 12] and h512c[-2:] == [16 ** 3, 8 ** 3] and h96 == [96, 48, 24, 12]
    got = driver([one(h4096, 3, 1024), one(h384, 3, 1024), one(h384, 3, 4096), one(h512c, 2, 4096), one(h96, 2, 64)])
    t = [g[0] for g in got]
    assert t == [len(h4096) - 3, len(h384) - 2, len(h384) - 2, len(h512c) - 1, 1]
    assert got[0][1] == 139776 and got[1][1] == 74880 and got[2][1] == 74880
    assert level_bytes(48 * 48, 3) + 74880 == 314496 > BUDGET          # why 48^2 stays outside at max_points 4096: 314 KB
    assert got[3][1] == level_bytes(512, 2) and level_bytes(4096, 2) > BUDGET     # 16^3 has 4096 points but not the LDS
    assert got[4][1] == sum(level_bytes(p, 2) for p in (48, 24, 12))


def test_plan_matches_its_rule(driver):
    shapes = [(4096, 4096), (384, 384), (1536, 1536), (512, 512, 512), (64, 64, 64), (96,), (256,), (130,), (32, 32), (96, 48), (40, 24), (36, 36),
              (16, 16, 16), (32, 16, 16), (33, 20), (4096,), (16384,)]
    cases = []
    for shape in shapes:
        pts = hierarchy(shape)
        for F in (1, 2, 3, 4, 5, 13):
            for maxp in (-3, 0, 1, 63, 64, 65, 143, 144, 145, 256, 575, 576, 577, 1023, 1024, 1025, 2304, 4096, 10 ** 9):
                cases.append(one(pts, F, maxp))
                if len(pts) > 2:
                    cases.append(one(pts, F, maxp, end=len(pts) - 2))      # the cycle ends above the coarsest level
    got = driver(cases)
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g[:2] == tail_rule(*c), (c, g)
        F = c[3]
        assert g[2] == BUDGET // level_bytes(1, F) and g[3] == -(-g[2] // 1024)
        if g[0] >= 1:
            assert all(p <= g[2] <= g[3] * 1024 for p in c[0][g[0]:c[2] + 1])     # every tail level fits the threads' point loops
    assert any(g[0] == -1 for g in got) and any(g[0] == 1 for g in got) and any(g[0] > 1 for g in got)
    assert all(g[0] != 0 for g in got)                                  # level 0 never qualifies


def test_budget_edges(driver):
    pts, F = [9216, 2304, 576, 144], 3
    two, three = level_bytes(576, F) + level_bytes(144, F), level_bytes(2304, F) + level_bytes(576, F) + level_bytes(144, F)
    got = driver([one(pts, F, 4096, budget=b) for b in (two - 1, two, two + 1, three - 1, three, level_bytes(144, F) - 1, level_bytes(144, F))])
    assert [g[:2] for g in got] == [(3, level_bytes(144, F)), (2, two), (2, two), (2, two), (1, three), (-1, 0), (3, level_bytes(144, F))]


def test_max_points_edges(driver):
    pts = [9216, 2304, 576, 144]
    got = driver([one(pts, 1, m) for m in (143, 144, 575, 576, 2303, 2304, 9216)])
    assert [g[0] for g in got] == [-1, 3, 3, 2, 2, 1, 1]               # never level 0, whatever max_points allows
    # a level in the middle above max_points stops the tail below it
    assert driver([one([9216, 600, 2304, 576, 144], 1, 1000)])[0][0] == 3


def test_distributed_and_replicated_levels(driver):
    pts = [4096, 1024, 256, 64]
    cases = [one(pts, 2, 4096, local=[0, 0, 0, 0]),                     # slab ranks without agglomeration: nothing qualifies
             one(pts, 2, 4096, local=[0, 0, 1, 1]),                     # replicated levels qualify: the tail starts on the first of them
             one(pts, 2, 4096, local=[0, 1, 0, 1]),                     # a distributed level in the middle stops the tail below it
             one(pts, 2, 4096, local=[1, 1, 1, 0]),                     # the level the cycle ends on is distributed
             one(pts, 2, 4096, local=[1, 1, 1, 1])]
    assert [g[0] for g in driver(cases)] == [-1, 2, 3, -1, 1]


def test_nothing_fits(driver):
    """12 ligands, F = 13: a 24^2 level alone needs 8 * 576 * 53 = 244 224 bytes"""
    assert level_bytes(576, 13) == 244224 > BUDGET
    got = driver([one([2304, 576], 13, 4096), one(hierarchy((200, 200)), 13, 10 ** 6), one([64], 2, 4096), one([], 2, 4096, end=-1),
                  one([256, 64], 0, 4096), one(hierarchy((384, 384)), 13, 4096)])
    assert [g[0] for g in got[:5]] == [-1] * 5 and all(g[1] == 0 for g in got[:5])
    assert got[5][:2] == (5, level_bytes(144, 13))                      # ... while the 12^2 level below it fits


def test_at_most_eight_levels(driver):
    pts = hierarchy((4096,))                                            # 1-D: 4096, 2048, ..., 8: nine levels below level 0 would fit F = 1
    assert len(pts) == 10 and sum(level_bytes(p, 1) for p in pts[1:]) <= BUDGET
    assert driver([one(pts, 1, 4096)])[0][0] == 2


BASE = ['-ts_type', 'rosw', '-ts_adapt_type', 'basic', '-ksp_rtol', '1e-8', '-ksfd_pc_type', 'mg', '-pc_type', 'lu']


def test_flag_parses_into_max_points():
    m = ko_opts.mg_tail_from
    assert m(BASE + ['-ksfd_mg_tail', '1024']) == 1024
    assert m(['-ksfd_mg_tail', '0'] + BASE) == 0
    assert m(BASE[:4] + ['-ksfd_mg_tail', '4096'] + BASE[4:]) == 4096
    assert m(['-ksfd_mg_tail', '1', '-ksfd_mg_tail', '256']) == 256
    assert m(BASE) is None and m([]) is None
    assert m(BASE + ['-ksfd_mg_agglomerate', '1']) is None and ko_opts.mg_agglomerate_from(BASE + ['-ksfd_mg_tail', '64']) is None


@pytest.mark.parametrize('bad', [['-ksfd_mg_tail'], ['-ksfd_mg_tail', '-1'], ['-ksfd_mg_tail', 'many'], ['-ksfd_mg_tail', '1e3'], ['-ksfd_mg_tail', '1.5'],
                                 ['-ksfd_mg_tail', str(2 ** 63)], ['-ksfd_mg_tail', '-ksp_rtol']])
def test_bad_values_raise(bad):
    with pytest.raises(ValueError):
        ko_opts.mg_tail_from(BASE + bad)


def test_existing_flags_return_what_they_did():
    ps = ko_opts.Params(ko_opts.parse_commandline(['dim=1', 'nelements=16']))
    raw = lambda o: bytes(ctypes.string_at(ctypes.addressof(o), ctypes.sizeof(o)))
    plain = ko_opts.step_opts_from(ps, BASE)
    withflag = ko_opts.step_opts_from(ps, BASE[:4] + ['-ksfd_mg_tail', '1024'] + BASE[4:])
    assert raw(plain) == raw(withflag) and plain.pc_type == 1
    assert ko_opts.deflation_from(BASE + ['-ksfd_mg_tail', '1024']) is None and ko_opts.mg_coarse_from(BASE + ['-ksfd_mg_tail', '1024']) is None


def test_header_binding_and_library_have_the_new_symbols():
    names = ('ksfd_set_mg_tail', 'ksfd_get_mg_tail_info')
    txt = open(os.path.join(ROOT, 'include', 'ksfd_hip.h')).read()
    assert re.search(r'\bKSFD_MGP_TAIL\s*=\s*8\b', txt)
    for name in names:
        assert re.search(r'\bint\s+%s\s*\(' % name, txt) and name in klib.ABI_SYMBOLS
    if not os.path.exists(klib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(klib.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    for name in ('set_mg_tail', 'mg_tail_info'):
        assert callable(getattr(klib.KSFDHip, name))
    # int32 level, nlevels; int64 max_points, points[8], lds_bytes, launches
    assert ctypes.sizeof(klib.MGTailInfo) == 2 * 4 + 11 * 8
    assert klib.MGP_TAIL == 8
    import inspect
    from ksfd_amd import ts
    assert 'mg_tail' in inspect.signature(ts.KSFDTS.__init__).parameters
