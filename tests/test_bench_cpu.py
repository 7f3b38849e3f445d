"""CPU: bench.py's command line (--full, --dump-outputs, --steps) and what --dump-outputs writes, with a stand-in handle."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import bench  # noqa: E402


def test_plain_run_is_the_default_and_full_is_opt_in():
    a = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse_args(['--full', '--dump-outputs', 'out'])
    assert a.full and a.dump_outputs == 'out'
    for bad in (['--steps', '0'], ['--warmup', '-1']):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


class _Handle:
    def __init__(self, n):
        self.u = np.arange(n, dtype=np.float64) * 0.5

    def get_state(self):
        return self.u.copy()


def _last():
    return {'t': 1.25, 'h': 0.3, 'vmax': np.array([1.0, 2.0, 0.0]), 'st': types.SimpleNamespace(h_used=0.2, wrms=0.7)}


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_small_state_whole(tmp_path):
    d = str(tmp_path / 'o')
    bench.dump_outputs(d, _Handle(1000), None, _last(), 0, 1, None)
    z = _read(d)
    assert sorted(z) == ['state', 'step_scalars', 'velocity_max']
    assert all(a.dtype == np.float64 for a in z.values())
    assert np.array_equal(z['state'], np.arange(1000) * 0.5)
    assert list(z['step_scalars']) == [1.25, 0.3, 0.2, 0.7] and list(z['velocity_max']) == [1.0, 2.0, 0.0]


def test_dump_outputs_large_state_fixed_sample_within_64mb(tmp_path):
    n = bench.DUMP_FULL_MAX + 12345
    outs = []
    for i in range(2):
        d = str(tmp_path / ('o%d' % i))
        bench.dump_outputs(d, _Handle(n), None, _last(), 0, 1, None)
        outs.append(_read(d))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    z = outs[0]
    assert sorted(z) == ['state_sample', 'state_sample_index', 'step_scalars', 'velocity_max']
    idx = z['state_sample_index']
    assert idx.size == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(z['state_sample'], idx * 0.5)
    assert all(np.array_equal(outs[1][k], z[k]) for k in z)          # same positions on every run


def test_dump_outputs_only_rank0_writes(tmp_path):
    d = str(tmp_path / 'o')
    bench.dump_outputs(d, _Handle(10), None, _last(), 1, 1, None)
    assert not os.path.exists(d)
