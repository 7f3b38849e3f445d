"""CPU: the launch-geometry constants tests/test_gpu_stage_ops.py copies from the library's sources are the ones the sources hold, so the
Python copies of strips_for / k3d_for there cannot drift unnoticed on shapes the GPU file does not run."""
import os
import re

from conftest import ROOT
import test_gpu_stage_ops as T

CSRC = os.path.join(ROOT, 'ksfd_amd', 'csrc')


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return int(m[0])


def test_geometry_constants_are_those_of_the_sources():
    ops, stencil, handle, tuning = _src('ops.hip.h'), _src('stencil.hip.h'), _src('handle.hip.h'), _src('tuning.h')
    assert _one(r'#define KSFD_STRIP_OUT (\d+)', stencil) == T.STRIP_OUT
    assert _one(r'#define KSFD_J3L_ROWS (\d+)', stencil) == 8                       # rows of Case.jvp_geometry on the LDS path
    assert _one(r'waves_jvp = \d+, waves_rhs = (\d+);', handle) == T.WAVES_RHS        # EnvKnobs: the defaults of KSFD_WAVES_RHS / _JVP
    assert _one(r'waves_jvp = (\d+), waves_rhs = \d+;', handle) == T.WAVES_JVP
    # ... and each environment variable is read into the member of its name, by the one line that names it
    assert re.findall(r'getenv\("KSFD_WAVES_(\w+)"\)\) E\.(\w+) = atoll\(v\);', handle) == [('JVP', 'waves_jvp'), ('RHS', 'waves_rhs')]
    assert len(re.findall(r'KSFD_WAVES_\w+"', handle + ops)) == 2 and ops.count('jvp ? env_knobs().waves_jvp : env_knobs().waves_rhs') == 1    # make_strips
    assert _one(r'int yseg = (\d+);', tuning) == T.YSEG_RHS
    assert _one(r'int yseg_jvp = (\d+);', tuning) == T.YSEG_JVP
    assert _one(r'int zseg = (\d+);', tuning) == T.ZSEG
    assert _one(r'rows == 8 \? 512 : (\d+)\)', ops) == T.BLOCKS3D                   # make_k3d, four rows per block
    assert _one(r'k3d_for\(h->G, KSFD_J3L_ROWS, 0, h->tune.zseg, (\d+)\)', ops) == T.BLOCKS3D


def test_python_copies_of_the_geometry_rules():
    """the two rules on the shapes of the issue's table, by hand: segments of two rows or planes on every small grid"""
    assert T.strips(8, 5, T.YSEG_RHS, T.WAVES_RHS) == dict(seg=2, nseg=3, nstrips=1)
    assert T.strips(124, 6, T.YSEG_RHS, T.WAVES_RHS)['nstrips'] == 1 and T.strips(126, 8, T.YSEG_RHS, T.WAVES_RHS)['nstrips'] == 2
    assert T.strips(250, 9, T.YSEG_JVP, T.WAVES_JVP) == dict(seg=2, nseg=5, nstrips=3)
    assert T.strips(130, 37, 32, 1) == dict(seg=32, nseg=2, nstrips=2) and T.strips(130, 37, 5, 1)['nseg'] == 8
    assert T.k3d((8, 64, 512), 8)['seg'] == 4 and T.k3d((8, 60, 512), 4)['seg'] == 7 and T.k3d((16, 10, 9), 4) == dict(seg=2, nseg=5, nstrips=1, rows=4)
