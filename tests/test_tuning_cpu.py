"""CPU: the record of the library's switches (ksfd_amd/csrc/tuning.h) on its own.  The header is plain C++ without device code and
without the handle -- that the small driver below compiles with the host compiler alone, warnings as errors, is the proof -- so the
driver replays calls of the record's two writers and prints the whole record after each one.
(a) tuning words and segment lengths through tuning_apply, power_its through tuning_mg_graph, against the table of the tuning word
    written out by hand below (bit -> field and the value a set bit gives it; every clear bit gives the default);
(b) the macros of include/ksfd_hip.h: distinct, bits 0..23 exactly once, the constants of ksfd_amd.lib name for name;
(c) the same driver built with the address and undefined-behaviour sanitizers, as a stand-alone program, over the single-bit words."""
import re
import subprocess

import pytest

from conftest import ROOT
from ksfd_amd import lib as klib
from test_handle_state_cpu import _cxx

DRIVER = r'''
#include "tuning.h"
#include <stdio.h>
#include <stdlib.h>
using namespace ksfd_ctl;
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0;
    if (fscanf(f, "%d", &n) != 1) return 3;
    Tuning t;
    for (int r = 0; r < n; r++) {
        int op = 0;
        long a = 0, b = 0, c = 0;
        if (fscanf(f, "%d %ld %ld %ld", &op, &a, &b, &c) != 4) return 3;
        switch (op) {
        case 0: t = Tuning(); break;                                       /* a new handle */
        case 1: tuning_apply(t, (int32_t)a, (int32_t)b, (int32_t)c); break;
        case 2: tuning_mg_graph(t, (int32_t)a); break;
        default: return 4;
        }
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", t.use_fused, t.use_frozen, t.overlap, t.async_mode, t.rec_mode,
               t.rec_keep, t.poly_fp32, t.fuse_stage, t.zero_copy, t.mg_fuse, t.rhs3d_strip, t.spec_guess, t.rhs_carry, t.spec_predict, t.restart_grow,
               t.mg_warm_power, t.mg_fp32, t.rec_mg, t.rhs_dots, t.old_boundary, t.rhs_gplane, t.yseg, t.yseg_jvp, t.zseg, t.mg_use_graph);
    }
    return 0;
}
'''

FIELDS = ('use_fused', 'use_frozen', 'overlap', 'async_mode', 'rec_mode', 'rec_keep', 'poly_fp32', 'fuse_stage', 'zero_copy', 'mg_fuse', 'rhs3d_strip',
          'spec_guess', 'rhs_carry', 'spec_predict', 'restart_grow', 'mg_warm_power', 'mg_fp32', 'rec_mg', 'rhs_dots', 'old_boundary', 'rhs_gplane',
          'yseg', 'yseg_jvp', 'zseg', 'mg_use_graph')
NEW, APPLY, MG_GRAPH = range(3)

# a new handle
DEFAULT = dict(use_fused=1, use_frozen=1, overlap=1, async_mode=0, rec_mode=1, rec_keep=3, poly_fp32=1, fuse_stage=1, zero_copy=1, mg_fuse=1,
               rhs3d_strip=1, spec_guess=1, rhs_carry=1, spec_predict=1, restart_grow=1, mg_warm_power=1, mg_fp32=1, rec_mg=0, rhs_dots=1,
               old_boundary=0, rhs_gplane=1, yseg=48, yseg_jvp=16, zseg=32, mg_use_graph=1)
# the tuning word: bit -> (field, its value when the bit is set).  A clear bit gives the field's default above -- bit 0 is the one whose
# default is "set", so a clear bit 0 gives 0.  Bits 4/5 and the field of bits 6-8 have rules of their own (_expect)
BITS = {0: ('use_fused', 1), 1: ('use_frozen', 0), 2: ('overlap', 0), 3: ('async_mode', 1), 9: ('poly_fp32', 0), 10: ('fuse_stage', 0),
        11: ('zero_copy', 0), 12: ('mg_fuse', 0), 13: ('rhs3d_strip', 0), 14: ('spec_guess', 0), 15: ('rhs_carry', 0), 16: ('spec_predict', 0),
        17: ('restart_grow', 0), 18: ('mg_warm_power', 0), 19: ('mg_fp32', 0), 20: ('rec_mg', 1), 21: ('rhs_dots', 0), 22: ('old_boundary', 1),
        23: ('rhs_gplane', 0)}
ALL24 = (1 << 24) - 1


def _expect(prev, word, yseg=0, yseg_jvp=0):
    """the record after ksfd_set_tuning(word, yseg, yseg_jvp) on the record prev, by the rules of the public header"""
    t = dict(prev)
    if word >= 0:                                                              # a negative word changes no switch
        for b, (field, when_set) in BITS.items():
            t[field] = when_set if word >> b & 1 else (0 if b == 0 else DEFAULT[field])
        t['rec_mode'] = 0 if word >> 4 & 1 else 2 if word >> 5 & 1 else 1      # bit 4 wins over bit 5
        if word >> 6 & 7:                                                      # 0 keeps the count in force
            t['rec_keep'] = min(word >> 6 & 7, 4)
    if yseg > 0:
        t['yseg'] = yseg
    if yseg_jvp > 0:
        t['yseg_jvp'] = yseg_jvp
    return t


def _build(d, name, extra):
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / name
    subprocess.run([_cxx(), '-x', 'c++', '-O1', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + extra +
                   ['-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(rows, tag='script'):
        inp = d / (name + '_' + tag + '.txt')
        inp.write_text('%d\n' % len(rows) + ''.join('%d %d %d %d\n' % tuple((list(row) + [0, 0, 0])[:4]) for row in rows))
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = [dict(zip(FIELDS, (int(x) for x in line.split()))) for line in r.stdout.splitlines()]
        assert len(out) == len(rows) and all(len(o) == len(FIELDS) for o in out)
        return out
    return run


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('tuning'), 'drv', [])


# ---- (a) the writers ------------------------------------------------------------------------------------------------------------------
def _single_bit_rows():
    rows = []
    for b in range(24):
        rows += [(NEW,), (APPLY, 1 | 1 << b)]
    return rows


def _check_single_bits(out):
    for b in range(24):
        assert out[2 * b] == DEFAULT, b
        got, want = out[2 * b + 1], _expect(DEFAULT, 1 | 1 << b)
        assert got == want, (b, {f: v for f, v in got.items() if want[f] != v})
    # ... and the table itself, spelled out once more for the bits with rules of their own
    diff = lambda b: {f: v for f, v in out[2 * b + 1].items() if DEFAULT[f] != v}
    assert diff(0) == {} and diff(4) == dict(rec_mode=0) and diff(5) == dict(rec_mode=2)
    assert diff(6) == dict(rec_keep=1) and diff(7) == dict(rec_keep=2) and diff(8) == dict(rec_keep=4)
    assert all(diff(b) == {BITS[b][0]: BITS[b][1]} for b in BITS if b)


def test_every_single_bit_on_top_of_word_1(driver):
    _check_single_bits(driver(_single_bit_rows(), 'bits'))


def test_word_0_all_bits_and_bits_4_and_5_together(driver):
    out = driver([(NEW,), (APPLY, 0), (NEW,), (APPLY, ALL24), (NEW,), (APPLY, 1 | 16 | 32), (APPLY, 1 | 32), (APPLY, 1)], 'words')
    assert out[1] == {**DEFAULT, 'use_fused': 0}                           # every other clear bit is the default; the field 0 keeps the 3
    flipped = {f: v for f, v in BITS.values()}
    assert out[3] == {**DEFAULT, **flipped, 'rec_mode': 0, 'rec_keep': 4}   # bit 4 wins over bit 5; 7 vectors asked for, 4 given
    assert out[5]['rec_mode'] == 0 and out[6]['rec_mode'] == 2 and out[7] == DEFAULT
    assert out[1] == _expect(DEFAULT, 0) and out[3] == _expect(DEFAULT, ALL24)


@pytest.mark.parametrize('prior', [2, 4])
def test_vectors_kept_per_stage_0_keeps_5_to_7_give_4(driver, prior):
    rows, want, t = [(NEW,)], [DEFAULT], DEFAULT
    for v in range(8):
        for word in (1 | prior << 6, 1 | v << 6):
            rows.append((APPLY, word))
            t = _expect(t, word)
            want.append(t)
    out = driver(rows, 'keep%d' % prior)
    assert out == want
    assert [out[2 + 2 * v]['rec_keep'] for v in range(8)] == [prior, 1, 2, 3, 4, 4, 4, 4]
    assert all(out[1 + 2 * v]['rec_keep'] == prior for v in range(8))


def test_a_negative_word_and_segment_lengths_that_keep(driver):
    odd = 1 << 1 | 1 << 3 | 1 << 5 | 2 << 6 | 1 << 12 | 1 << 20 | 1 << 22               # bit 0 clear as well
    out = driver([(NEW,), (APPLY, odd, 24, 8), (APPLY, -1), (APPLY, -5, 0, -3), (APPLY, -1, 32, 0), (APPLY, -1, 0, 12), (APPLY, 1, -1, 0), (APPLY, 1, 40, 20)], 'keep')
    moved = dict(use_fused=0, use_frozen=0, async_mode=1, rec_mode=2, rec_keep=2, mg_fuse=0, rec_mg=1, old_boundary=1, yseg=24, yseg_jvp=8)
    assert out[1] == {**DEFAULT, **moved}
    assert out[2] == out[1] and out[3] == out[1]                                         # nothing moves
    assert out[4] == {**out[1], 'yseg': 32} and out[5] == {**out[4], 'yseg_jvp': 12}
    assert out[6] == {**DEFAULT, 'rec_keep': 2, 'yseg': 32, 'yseg_jvp': 12}              # the word replaces the switches; the count and the lengths are kept
    assert out[7] == {**out[6], 'yseg': 40, 'yseg_jvp': 20}
    assert all(o['zseg'] == 32 and o['mg_use_graph'] == 1 for o in out)                  # no word reaches these


def test_power_its_minus_7_asks_for_eager_launches_every_other_call_for_the_graph(driver):
    assert klib.MG_EAGER == -7
    for order in ((-7, 0, 5), (5, 0, -7), (0, -7, 5), (-7, -7, 0)):
        out = driver([(NEW,)] + [(MG_GRAPH, p) for p in order] + [(APPLY, ALL24), (APPLY, -1)], 'graph')
        assert [o['mg_use_graph'] for o in out] == [1] + [int(p != -7) for p in order] + [int(order[-1] != -7)] * 2
        assert all({**o, 'mg_use_graph': 1} == DEFAULT for o in out[:4])                 # ... and touches nothing else


# ---- (b) the names --------------------------------------------------------------------------------------------------------------------
def test_header_macros_cover_the_word_once_and_equal_the_python_constants():
    text = open(ROOT + '/include/ksfd_hip.h').read()
    macros = {m.group(1): int(m.group(2)) << int(m.group(3)) for m in re.finditer(r'^#define KSFD_TUNE_(\w+) \((\d+) << (\d+)\)', text, re.M)}
    assert len(macros) == len(re.findall(r'^#define KSFD_TUNE_\w+ ', text, re.M))        # every object-like macro has the form above
    assert len(set(macros.values())) == len(macros)
    assert sum(macros.values()) == ALL24 and not any(a & b for n, a in macros.items() for m, b in macros.items() if n != m)
    order = list(macros.values())
    assert order == sorted(order)                                                        # in bit order
    assert macros == {n[5:]: v for n, v in vars(klib).items() if n.startswith('TUNE_') and isinstance(v, int)}
    assert re.search(r'^#define KSFD_TUNE_REC_KEEP\(v\) \(\(\(v\) & 7\) << 6\)$', text, re.M)
    assert [klib.TUNE_REC_KEEP(v) for v in (0, 1, 4, 7)] == [0, 64, 256, klib.TUNE_REC_KEEP_MASK] == [0, 64, 256, macros['REC_KEEP_MASK']]
    assert re.search(r'^#define KSFD_MG_EAGER \(-7\)$', text, re.M)


# ---- (c) sanitizers -------------------------------------------------------------------------------------------------------------------
def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    run = _build(tmp_path, 'drv_san', ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    _check_single_bits(run(_single_bit_rows(), 'bits'))
