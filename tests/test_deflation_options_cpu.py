"""CPU: the three flags of the deflated-restart stage solver (-ksfd_ksp_type, -ksfd_dgmres_eigen, -ksfd_dgmres_carry) parse into what
KSFDHip.set_deflation takes, bad values raise like -ksfd_pc_type does, and a list without them yields exactly what it yields today."""
import ctypes

import pytest

from ksfd_amd import lib as klib
from ksfd_amd import options as ko_opts

BASE = ['-ts_type', 'rosw', '-ts_adapt_type', 'basic', '-ts_adapt_clip', '0.1,5', '-ksp_rtol', '1e-8', '-ksp_gmres_restart', '40',
        '-ksfd_pc_type', 'mg', '-pc_type', 'lu']


def _bytes(o):
    return bytes(ctypes.string_at(ctypes.addressof(o), ctypes.sizeof(o)))


def _params():
    return ko_opts.Params(ko_opts.parse_commandline(['dim=1', 'nelements=16']))


def test_flags_parse_into_keep_and_carry():
    d = ko_opts.deflation_from
    assert d(BASE + ['-ksfd_ksp_type', 'dgmres']) == (8, ko_opts.DGMRES_CARRY_DEFAULT)
    assert ko_opts.DGMRES_EIGEN_DEFAULT == 8 and ko_opts.DGMRES_CARRY_DEFAULT in (0, 1)
    assert d(['-ksfd_ksp_type', 'dgmres', '-ksfd_dgmres_eigen', '12'] + BASE) == (12, ko_opts.DGMRES_CARRY_DEFAULT)
    assert d(['-ksfd_dgmres_carry', '0', '-ksfd_ksp_type', 'dgmres', '-ksfd_dgmres_eigen', '1']) == (1, 0)
    assert d(['-ksfd_ksp_type', 'dgmres', '-ksfd_dgmres_eigen', '16', '-ksfd_dgmres_carry', '1']) == (16, 1)
    # plain GMRES: asked for, or nothing said; the dgmres knobs alone select nothing
    assert d(BASE) is None and d([]) is None
    assert d(BASE + ['-ksfd_ksp_type', 'gmres']) is None
    assert d(['-ksfd_dgmres_eigen', '4', '-ksfd_dgmres_carry', '1']) is None


@pytest.mark.parametrize('bad', [['-ksfd_ksp_type', 'fgmres'], ['-ksfd_ksp_type'], ['-ksfd_ksp_type', 'dgmres', '-ksfd_dgmres_eigen', '0'],
                                 ['-ksfd_ksp_type', 'dgmres', '-ksfd_dgmres_eigen', '17'], ['-ksfd_dgmres_eigen', 'many'],
                                 ['-ksfd_dgmres_eigen'], ['-ksfd_dgmres_carry', '2'], ['-ksfd_dgmres_carry', 'yes'],
                                 ['-ksfd_ksp_type', 'dgmres', '-ksfd_dgmres_carry']])
def test_bad_values_raise(bad):
    with pytest.raises(ValueError):
        ko_opts.deflation_from(BASE + bad)


def test_existing_flags_return_what_they_did():
    """the step options are a plain C struct: compare them byte for byte with and without the new flags in the list"""
    ps = _params()
    plain = ko_opts.step_opts_from(ps, BASE)
    assert (plain.ksp_rtol, plain.ksp_restart, plain.pc_type, plain.adapt, plain.clip_lo, plain.clip_hi) == (1e-8, 40, 1, 1, 0.1, 5.0)
    withflags = ko_opts.step_opts_from(ps, BASE[:4] + ['-ksfd_ksp_type', 'dgmres', '-ksfd_dgmres_eigen', '12', '-ksfd_dgmres_carry', '0'] + BASE[4:])
    assert _bytes(plain) == _bytes(withflags)
    dflt = klib.default_step_opts(rtol=plain.rtol, atol=plain.atol)
    assert _bytes(ko_opts.step_opts_from(ps, [])) == _bytes(dflt)
    assert ctypes.sizeof(klib.DeflationStats) == 10 * 4         # 2 + 4 + 4 int32, as in include/ksfd_hip.h


def test_binding_exposes_the_deflation_entries():
    for name in ('ksfd_set_deflation', 'ksfd_get_deflation_stats', 'ksfd_basis_rotate'):
        assert name in klib.ABI_SYMBOLS
    for name in ('set_deflation', 'deflation_stats', 'basis_rotate'):
        assert callable(getattr(klib.KSFDHip, name))
    assert (klib.ROT_MAXIN, klib.ROT_MAXOUT) == (121, 18)
