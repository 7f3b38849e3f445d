"""GPU: no entry reads a product of an older state.  The handle keeps derived data between calls -- coefficient planes and their fp32 copy,
the grid means of the spectral preconditioner, coarse planes, the shift set-up and the captured coarse cycle, direct and banded factors
(csrc/handle_state.h has the record of which of them is current, DESIGN.md the table).  Every event that writes the state or moves the
parameters has to end what was made before it.

For each event: handle A calls every entry (so the products exist), goes through the event, and calls every entry again; a fresh handle B
with the same configuration is given A's state and calls the same entries.  The results must be equal bit for bit: the kernels, their
inputs and the launch geometry are the same on both handles, and the V cycle entry sets the hierarchy up cold on both."""
import dataclasses

import numpy as np
import pytest

from ksfd_amd import lib as klib
from test_gpu_mg_coarse import _cfg, _state

pytestmark = pytest.mark.gpu
GAMMA = 0.43586652150845900
SHIFT = 1.0 / (GAMMA * 5.0)                   # a stiff step: the shift of the V cycle tests
GRIDS = {'32x32': (32, 32), '64': (64,)}      # 2-D: the smallest grid with both a spectral plan and a hierarchy; 1-D: the banded entry


def _entries(k, dim):
    """every entry that reads a product, on fixed inputs: name -> result"""
    rng = np.random.default_rng(11)
    v = rng.standard_normal(k.nlocal)
    vc = rng.standard_normal(k.mg_coarse_info()['unknowns'])
    pts = k.nlocal // k.F
    out = dict(jvp=k.jvp(v), rhs=k.rhs(), velocity_max=k.velocity_max(),
               cycle=k.mg_part(klib.MGP_CYCLE, 0, v.reshape(k.F, pts), variant=0, shift=SHIFT),
               coarse_op=k.mg_coarse_apply(SHIFT, vc, op=0), direct=k.direct_apply(SHIFT, v))
    if dim == 2:
        out['spectral'] = k.spectral_apply(SHIFT, v)
    else:
        out['banded'] = k.banded_apply(SHIFT, v)
    return out


def _step(k, **kw):
    return k.step(0.0, kw.pop('h', 0.05), klib.default_step_opts(atol=0.01, rtol=1e-6, **kw), raise_on_error=False)


def ev_set_state(k, cfg):
    k.set_state(_state(cfg, 5, amp=0.05))


def ev_set_state_random(k, cfg):
    k.set_state_random(np.random.default_rng(6).standard_normal((4,) * cfg.dim), rho0=9000.0)


def ev_scale_rho(k, cfg):
    k.scale_rho(0.5)


def ev_mul_rho(k, cfg):
    k.mul_rho(1.0 + 0.1 * np.random.default_rng(7).random(k.nlocal // k.F))


def ev_update_params(k, cfg):
    new = dataclasses.replace(cfg, s2=2.0 * cfg.s2)
    k.update_params(new)
    return new


def ev_accepted_step(k, cfg):
    t, h, st, rc = _step(k, adapt=0)
    assert rc == 0 and st.accepted


def ev_rejected_attempt(k, cfg):
    # one attempt per call (reserved bit 1) with an absurd step size; the direct solver, so that the attempt gets as far as the controller
    before = k.get_state()
    t, h, st, rc = _step(k, h=1.0e4, adapt=1, reserved=2, pc_type=5)
    assert rc == 0 and not st.accepted and st.rejections == 1, (rc, st.accepted, st.rejections, k.last_error())
    assert np.array_equal(k.get_state(), before)


def ev_groom(k, cfg):
    k.groom()


def ev_checkpoint_replay(k, cfg):
    k.checkpoint()
    for _ in range(2):
        t, h, st, rc = _step(k, adapt=0)
        assert rc == 0
    k.restore()


EVENTS = [ev_set_state, ev_set_state_random, ev_scale_rho, ev_mul_rho, ev_update_params, ev_accepted_step, ev_rejected_attempt, ev_groom,
          ev_checkpoint_replay]


@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('event', EVENTS, ids=[e.__name__[3:] for e in EVENTS])
def test_entries_after_an_event_equal_entries_on_a_fresh_handle(event, grid):
    shape = GRIDS[grid]
    cfg = _cfg(shape, 1)
    a = klib.KSFDHip(cfg)
    a.set_state(_state(cfg, 3, amp=0.05))
    before = _entries(a, len(shape))                       # the products exist
    cfg_after = event(a, cfg) or cfg
    got = _entries(a, len(shape))
    b = klib.KSFDHip(cfg_after)
    b.set_state(a.get_state())
    want = _entries(b, len(shape))
    a.close()
    b.close()
    assert set(got) == set(want) == set(before)
    stale = [n for n in want if not np.array_equal(got[n], want[n])]
    assert not stale, 'read from a product of the older state: %s' % ', '.join(stale)
    if event not in (ev_groom, ev_rejected_attempt, ev_checkpoint_replay):
        # the event moved the state or the parameters: had the entries answered from the old products, this test could not tell
        assert not np.array_equal(got['jvp'], before['jvp'])
