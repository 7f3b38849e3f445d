"""CPU: the -ksfd_pc_type flag of the options parser and the C declarations of the direct solver (pc_type 5)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from ksfd_amd import lib as klib
from ksfd_amd.options import step_opts_from


class _Params:
    values0 = {'rtol': 1e-5, 'atol': 1e-5}


@pytest.mark.parametrize('spelling,pc', [('auto', 2), ('none', 0), ('mg', 1), ('poly', 3), ('spectral', 4), ('lu', 5)])
def test_ksfd_pc_type_spellings(spelling, pc):
    o = step_opts_from(_Params(), ['-ts_type', 'rosw', '-ksfd_pc_type', spelling, '-ksp_rtol', '1e-8'])
    assert o.pc_type == pc and o.ksp_rtol == 1e-8


@pytest.mark.parametrize('bad', [['-ksfd_pc_type', 'cholesky'], ['-ksfd_pc_type'], ['-ksfd_pc_type', '5']])
def test_ksfd_pc_type_unknown_value_raises(bad):
    with pytest.raises(ValueError):
        step_opts_from(_Params(), bad)


def test_bare_pc_type_lu_keeps_the_automatic_choice():
    """the reference's options files say -ksp_type preonly -pc_type lu; that stays the automatic iterative choice"""
    o = step_opts_from(_Params(), ['-ksp_type', 'preonly', '-pc_type', 'lu'])
    assert o.pc_type == 2
    assert step_opts_from(_Params(), ['-pc_type', 'lu', '-ksfd_pc_type', 'lu']).pc_type == 5


def test_header_declares_the_direct_solver(tmp_path):
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    src = tmp_path / 'direct.c'
    src.write_text('''
#include "ksfd_hip.h"
typedef int (*direct_fn)(ksfd_handle *, double, const double *, double *, int32_t);
int main(void) {
    direct_fn f = ksfd_direct_apply;
    char check[KSFD_DIRECT_MAX == 32768 ? 1 : -1];
    (void)check;
    return f == 0;
}
''')
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-I', os.path.join(ROOT, 'include'),
                    str(src)], check=True)
    assert klib.DIRECT_MAX == 32768 and klib.PC_DIRECT == 16 and 'ksfd_direct_apply' in klib.ABI_SYMBOLS
