"""CPU: the host side of the exact coarse solve of the multigrid V cycle (ksfd_set_mg_coarse).  Which level the cycle ends on is a pure
function over the level sizes (ksfd_amd/csrc/mg_coarse_plan.h, plain C++: the small driver below compiles with the host compiler alone)
and is checked against a restatement of its rule in Python over a table of hierarchies; the two option flags parse into what
KSFDHip.set_mg_coarse takes, bad values raise like -ksfd_pc_type does, a list without them yields what it yields today; the new symbols are in
the header, the binding and the built library."""
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

CAP = 2048

DRIVER = r'''
#include "mg_coarse_plan.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncases;
    if (fscanf(f, "%d", &ncases) != 1) return 3;
    for (int k = 0; k < ncases; k++) {
        int kind, nlevels; long long maxu, cap, unk[32];
        if (fscanf(f, "%d %lld %lld %d", &kind, &maxu, &cap, &nlevels) != 4 || nlevels > 32) return 3;
        for (int l = 0; l < nlevels; l++) if (fscanf(f, "%lld", &unk[l]) != 1) return 3;
        printf("%d\n", ksfd_ctl::mg_coarse_level(unk, nlevels, kind, maxu, cap));
    }
    return 0;
}
'''


def hierarchy(shape, F, ranks=1):
    """F * points per level as mg_build makes them on one rank: halve every extent while all are even and stay >= 8"""
    n = list(shape)
    out = [F * _prod(n)]
    while all(x % 2 == 0 and x // 2 >= 8 for x in n):
        n = [x // 2 for x in n]
        out.append(F * _prod(n))
    return out


def _prod(n):
    p = 1
    for x in n:
        p *= x
    return p


def level_rule(unk, kind, maxu, cap):
    """the rule of the issue, restated: finest level below 0 with <= max unknowns, else (max <= 0) the coarsest, else refuse"""
    if len(unk) < 2 or kind not in (0, 1):
        return -1
    if kind == 0:
        return len(unk) - 1
    if maxu > cap:
        return -1
    if maxu <= 0:
        return len(unk) - 1 if unk[-1] <= cap else -1
    fits = [l for l in range(1, len(unk)) if unk[l] <= maxu]
    return fits[0] if fits else -1


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('hipcc') or (hipcc if os.path.exists(hipcc) else None)
    if not cxx:
        pytest.fail('no C++ compiler found (g++, c++, hipcc): the library cannot have been built either')
    d = tmp_path_factory.mktemp('mgcoarse')
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / 'drv'
    subprocess.run([cxx, '-x', 'c++', '-O1', '-std=c++17', '-Wall', '-Werror', '-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(cases):
        inp = d / 'cases.txt'
        with open(inp, 'w') as f:
            f.write('%d\n' % len(cases))
            for kind, maxu, cap, unk in cases:
                f.write('%d %d %d %d %s\n' % (kind, maxu, cap, len(unk), ' '.join(str(x) for x in unk)))
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, check=True, timeout=60)
        return [int(x) for x in r.stdout.split()]
    return run


HIERARCHIES = [((96,), 2), ((130,), 2), ((32, 32), 2), ((48, 40), 2), ((40, 24), 3), ((16, 16, 16), 2), ((64, 64), 4), ((24, 24, 24), 3),
               ((7, 5, 7), 2), ((384, 384), 2), ((2048, 2048), 2), ((33, 20), 2), ((384,), 3), ((16,), 2), ((15,), 2)]


def test_level_choice_matches_its_rule(driver):
    cases = []
    for (shape, F), kind, maxu in itertools.product(HIERARCHIES, (0, 1, 2, -1), (-5, 0, 1, 23, 24, 128, 240, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 10 ** 7)):
        cases.append((kind, maxu, CAP, hierarchy(shape, F)))
    cases.append((1, 0, CAP, []))
    cases.append((1, 100, 50, [400, 100, 25]))          # max above the cap: refused although a level would fit
    got = driver(cases)
    assert len(got) == len(cases)
    for (kind, maxu, cap, unk), g in zip(cases, got):
        assert g == level_rule(unk, kind, maxu, cap), (kind, maxu, unk, g)
    assert -1 in got and any(g > 0 for g in got)


def test_level_choice_of_the_cases_the_gpu_tests_use(driver):
    """the levels tests/test_gpu_mg_coarse.py asserts on the device, from the same function"""
    table = [((96,), 2, 0, 3, 24), ((130,), 2, 0, 1, 130), ((32, 32), 2, 0, 2, 128), ((48, 40), 2, 0, 2, 240), ((40, 24), 3, 0, 1, 720),
             ((16, 16, 16), 2, 0, 1, 1024), ((64, 64), 4, 2048, 2, 1024)]
    got = driver([(1, maxu, CAP, hierarchy(shape, F)) for shape, F, maxu, _, _ in table])
    for (shape, F, maxu, level, unknowns), g in zip(table, got):
        assert g == level and hierarchy(shape, F)[g] == unknowns, (shape, F, g)
    # refusals: the coarsest level of 24^3 x 3 fields has 12^3 * 3 = 5184 unknowns; 7 x 5 x 7 has no hierarchy; max above the cap
    assert driver([(1, 0, CAP, hierarchy((24, 24, 24), 3)), (1, 0, CAP, hierarchy((7, 5, 7), 2)), (1, 4096, CAP, hierarchy((64, 64), 4))]) == [-1, -1, -1]


BASE = ['-ts_type', 'rosw', '-ts_adapt_type', 'basic', '-ksp_rtol', '1e-8', '-ksfd_pc_type', 'mg', '-pc_type', 'lu']


def test_flags_parse_into_kind_and_max():
    m = ko_opts.mg_coarse_from
    assert m(BASE + ['-ksfd_mg_coarse', 'lu']) == (1, 0)
    assert m(['-ksfd_mg_coarse', 'lu', '-ksfd_mg_coarse_max', '1024'] + BASE) == (1, 1024)
    assert m(['-ksfd_mg_coarse_max', '2048', '-ksfd_mg_coarse', 'lu']) == (1, 2048)
    assert m(BASE + ['-ksfd_mg_coarse', 'cheb']) == (0, 0)
    assert m(['-ksfd_mg_coarse_max', '0', '-ksfd_mg_coarse', 'lu']) == (1, 0)
    assert m(BASE) is None and m([]) is None
    assert ko_opts.KSFD_MG_COARSE == {'cheb': 0, 'lu': 1} and ko_opts.MG_COARSE_MAX_LIMIT == klib.MG_DIRECT_MAX == CAP


@pytest.mark.parametrize('bad', [['-ksfd_mg_coarse', 'ilu'], ['-ksfd_mg_coarse'], ['-ksfd_mg_coarse', '1'], ['-ksfd_mg_coarse', 'lu', '-ksfd_mg_coarse_max', '4096'],
                                 ['-ksfd_mg_coarse_max', '-1'], ['-ksfd_mg_coarse_max', 'many'], ['-ksfd_mg_coarse_max'], ['-ksfd_mg_coarse_max', '1e3']])
def test_bad_values_raise(bad):
    with pytest.raises(ValueError):
        ko_opts.mg_coarse_from(BASE + bad)


def test_existing_flags_return_what_they_did():
    ps = ko_opts.Params(ko_opts.parse_commandline(['dim=1', 'nelements=16']))
    raw = lambda o: bytes(ctypes.string_at(ctypes.addressof(o), ctypes.sizeof(o)))
    plain = ko_opts.step_opts_from(ps, BASE)
    withflags = ko_opts.step_opts_from(ps, BASE[:4] + ['-ksfd_mg_coarse', 'lu', '-ksfd_mg_coarse_max', '1024'] + BASE[4:])
    assert raw(plain) == raw(withflags) and plain.pc_type == 1
    assert ko_opts.deflation_from(BASE + ['-ksfd_mg_coarse', 'lu']) is None


def test_header_binding_and_library_have_the_new_symbols():
    names = ('ksfd_set_mg_coarse', 'ksfd_get_mg_coarse_info', 'ksfd_mg_coarse_apply')
    txt = open(os.path.join(ROOT, 'include', 'ksfd_hip.h')).read()
    assert re.search(r'#define\s+KSFD_MG_DIRECT_MAX\s+2048\b', txt)
    for name in names:
        assert re.search(r'\bint\s+%s\s*\(' % name, txt) and name in klib.ABI_SYMBOLS
    if not os.path.exists(klib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(klib.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    for name in ('set_mg_coarse', 'mg_coarse_info', 'mg_coarse_apply'):
        assert callable(getattr(klib.KSFDHip, name))
    # int32 kind, level, nlevels, F; int64 n[3], unknowns; int32 factorizations, solves, fallbacks, reserved
    assert ctypes.sizeof(klib.MGCoarseInfo) == 4 * 4 + 4 * 8 + 4 * 4
    assert klib.PC_MG_COARSE_DIRECT == 64 and (klib.MG_COARSE_CHEB, klib.MG_COARSE_LU) == (0, 1)
