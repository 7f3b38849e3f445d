"""CPU: the index plan of the banded direct solver (ksfd_amd/csrc/banded_plan.h) -- the fold of the periodic 1-D ring, the band it
leaves and the LAPACK band slots -- and the spellings that reach the solver (-ksfd_pc_type banded, ksfd_banded_apply).  The header is
host-only plain C++, so a small driver compiled with the host compiler runs exactly what the kernels and the host code run."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from ksfd_amd import options as ko_opts

DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "banded_plan.h"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const long long N = atoll(argv[2]);
    if (argv[1][0] == 'p') {
        /* pos <N>: one line per ring point: pos(p), point(p taken as a position) */
        for (long long p = 0; p < N; p++) printf("%lld %lld\n", band_pos(N, p), band_point(N, p));
        return 0;
    }
    /* band <N> <F>: the plan, then what the stencil entries (every dof pair of every ring pair at distance <= 2) do in the band array */
    const int F = atoi(argv[3]);
    const BandPlan B = band_plan(N, F);
    printf("%lld %d %d %d %lld\n", B.n, B.kl, B.ku, B.ldab, band_size(B));
    std::vector<unsigned char> used((size_t)band_size(B), 0);
    long long entries = 0, outside = 0, out_of_array = 0, shared = 0, maxdist = 0, inv_bad = 0;
    for (long long p = 0; p < N; p++)
        for (int m = -2; m <= 2; m++) {
            const long long q = ((p + m) % N + N) % N;
            if (m != 0 && q == p) continue;
            for (int a = 0; a < F; a++)
                for (int b = 0; b < F; b++) {
                    const long long i = band_unknown(B, p, a), j = band_unknown(B, q, b);
                    long long pp; int dd;
                    band_unknown_inv(B, i, pp, dd);
                    if (pp != p || dd != a) inv_bad++;
                    entries++;
                    const long long d = i > j ? i - j : j - i;
                    if (d > maxdist) maxdist = d;
                    if (!band_inside(B, i, j) || i - j > B.kl || j - i > B.ku) { outside++; continue; }
                    const long long s = band_slot(B, i, j);
                    if (s < 0 || s >= band_size(B)) { out_of_array++; continue; }
                    if (s != (long long)(B.kl + B.ku) + i - j + j * (long long)(2 * B.kl + B.ku + 1)) out_of_array++;
                    if (used[(size_t)s]) shared++;
                    used[(size_t)s] = 1;
                }
        }
    printf("%lld %lld %lld %lld %lld %lld\n", entries, outside, out_of_array, shared, maxdist, inv_bad);
    return 0;
}
'''

SIZES = list(range(5, 71)) + [166, 256, 683, 4096]


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('hipcc') or (hipcc if os.path.exists(hipcc) else None)
    if not cxx:
        pytest.fail('no C++ compiler found (g++, c++, hipcc): the library cannot have been built either')
    d = tmp_path_factory.mktemp('band')
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / 'drv'
    subprocess.run([cxx, '-x', 'c++', '-O1', '-std=c++17', '-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, check=True, timeout=60)
        return [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    return run


def test_fold_is_a_permutation_and_keeps_ring_neighbours_within_four(driver):
    for N in SIZES:
        rows = driver('pos', N)
        pos = [r[0] for r in rows]
        point = [r[1] for r in rows]
        assert sorted(pos) == list(range(N)), N
        assert all(point[pos[p]] == p for p in range(N)), N                    # the inverse inverts it
        assert pos[:3] == [0, 2, 4] and pos[N - 1] == 1 and pos[N - 2] == 3     # 0, N-1, 1, N-2, 2, ...
        far = max(abs(pos[p] - pos[(p + m) % N]) for p in range(N) for m in (1, 2))
        assert far <= 4, (N, far)
        if N >= 9:
            assert far == 4, N


@pytest.mark.parametrize('F', range(1, 14))
def test_band_slots_of_the_stencil(driver, F):
    for N in SIZES:
        (n, kl, ku, ldab, size), (entries, outside, out_of_array, shared, maxdist, inv_bad) = driver('band', N, F)
        assert n == N * F and kl == ku == min(5 * F - 1, n - 1) and ldab == 2 * kl + ku + 1 and size == ldab * n, (N, F)
        assert entries == N * 5 * F * F, (N, F)
        assert outside == 0 and out_of_array == 0 and shared == 0 and inv_bad == 0, (N, F, outside, out_of_array, shared, inv_bad)
        assert maxdist <= kl, (N, F, maxdist)
        if N >= 9:
            assert maxdist == 5 * F - 1, (N, F, maxdist)                        # the band is exactly this wide
        if N == 5:
            assert kl == n - 1                                                  # clamps to the full matrix


def test_pc_type_spellings():
    ps = ko_opts.Params(ko_opts.parse_commandline(['dim=1', 'nelements=16']))
    assert ko_opts.step_opts_from(ps, ['-ksfd_pc_type', 'banded']).pc_type == 6
    for name, v in (('auto', 2), ('none', 0), ('mg', 1), ('poly', 3), ('spectral', 4), ('lu', 5)):
        assert ko_opts.step_opts_from(ps, ['-ksfd_pc_type', name]).pc_type == v
    assert ko_opts.step_opts_from(ps, []).pc_type == 2
    with pytest.raises(ValueError):
        ko_opts.step_opts_from(ps, ['-ksfd_pc_type', 'band'])


def test_header_and_python_declare_the_banded_entry():
    from ksfd_amd import lib as klib
    text = open(os.path.join(ROOT, 'include', 'ksfd_hip.h')).read()
    assert re.search(r'int\s+ksfd_banded_apply\(ksfd_handle \*h, double shift, const double \*v, double \*out, int32_t layout\);', text)
    assert 'ksfd_banded_apply' in klib.ABI_SYMBOLS and klib.PC_BANDED == 32 and klib.PC_DIRECT == 16
    assert hasattr(klib.KSFDHip, 'banded_apply')
