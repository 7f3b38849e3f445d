"""GPU: the opt-in coarse tail of the multigrid V cycle (ksfd_set_mg_tail): the sub-cycle from the first tail level down to the level the
cycle ends on and back in ONE launch of one workgroup with the level vectors in the LDS (k_mg_tail).  Handles, inputs, references and
bounds are those of tests/test_gpu_mg_parts.py (imported): the tail is compared through the test entry MGP_TAIL -- which runs the wrapper
the cycle calls -- with mr.vcycle(levels, l = t) fed the DOWNLOADED planes, blocks and bounds, in longdouble;

    bound = 32 x max(d_ref, 1e-12),  d_ref = rel-L2 between the reference's own float64 and longdouble evaluations

(nothing tuned on the kernel).  Shapes: the smallest that exercise each way to go wrong -- wrap of the +-2 star on an 8-point axis, more
points than threads (48 x 24 = 1152) with anisotropic extents, F = 4 blocks, odd coarsest extents, 3-D (a level of exactly 1024 points),
1-D with three tail levels, 1-D with one odd level.  Measured distances and head-room: profiles/mg_tail_runs.log (the lines this file
prints).

Two departures from the letter of the design, both because its own numbers say so:
  * the fp32 cycle's reference rounds the level vectors of the levels ABOVE the tail only (the tail's levels keep fp64 vectors and read
    the fp64 planes), the reference pair and the 4 x d32 bound are otherwise those of test_gpu_mg_parts.py::test_cycle;
  * two slab ranks of 64^2 keep 4 rows each down to 8^2, so set_mg_agglomerate(1) replicates nothing there and no level qualifies for
    the tail: that is asserted (tail level -1, steps bit for bit those without the call), and the replicated-levels test proper runs on
    the same two ranks with set_mg_agglomerate(300) (levels 16^2 and 8^2 whole on every rank, as tests/test_gpu_mg_agglomerate.py has them)."""
import os

import numpy as np
import pytest

import mg_reference as mr
from conftest import rel_l2
from ksfd_amd import lib as klib
from test_gpu_dist import _free_port
from test_gpu_mg_coarse import STIFF, _cfg, _oracle_step, _state
from test_gpu_mg_parts import LD, MARGIN, MG_RATIO, S_CYCLE, TOL_OP, Case

pytestmark = pytest.mark.gpu

#        name         shape       ligands  max_points  first tail level  points of the tail's levels
CASES = {'32x32': ((32, 32), 1, 1024, 1, [256, 64]),
         '96x48': ((96, 48), 1, 2304, 1, [1152, 288]),
         '40x24': ((40, 24), 3, 1024, 1, [240]),
         '36x36': ((36, 36), 2, 1024, 1, [324, 81]),
         '16x16x16': ((16, 16, 16), 1, 1024, 1, [512]),
         '32x16x16': ((32, 16, 16), 2, 1024, 1, [1024]),
         '96': ((96,), 1, 1024, 1, [48, 24, 12]),
         '130': ((130,), 2, 1024, 1, [65])}


def lds_bytes(points, F):
    return sum(8 * p * (4 * F + 1) for p in points)


class TailCase(Case):
    """Case of tests/test_gpu_mg_parts.py (same state, same downloads) on the shapes above, with the tail planned"""

    def __init__(self, name):
        shape, nlig, maxp = CASES[name][:3]
        self.name, self.shape, self.nlig, self.dim = name, shape, nlig, len(shape)
        self.cfg = _cfg(shape, nlig, tuple((0.01 if len(shape) == 3 else 0.0025) * n for n in shape))
        self.k = klib.KSFDHip(self.cfg)
        self.u = _state(self.cfg, 3, amp=0.05)
        self.k.set_state(self.u)
        self.F = self.cfg.F
        self.lig = dict(s=list(self.cfg.lig_s), gamma=list(self.cfg.lig_gamma), D=list(self.cfg.lig_D))
        self.h0 = [self.cfg.L[a] / shape[a] for a in range(self.dim)]
        self.nlev = self.k.mg_level_info(0)['nlevels']
        self.info = [self.k.mg_level_info(l) for l in range(self.nlev)]
        self._coef, self._setup = {}, {}
        self.k.set_mg_tail(maxp)
        self.tail = self.k.mg_tail_info()
        self._lv = {}

    def reference_levels(self):
        if not self._lv:
            self._lv['f64'], self._lv['ld'] = self.levels(S_CYCLE), self.levels(S_CYCLE, 0, LD)
        return self._lv['f64'], self._lv['ld']


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = TailCase(name)
    return _CASES[name]


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for c in _CASES.values():
        c.k.close()
    _CASES.clear()


def _rhs(c, l, seed):
    """the inputs of Case.inputs: random, both impulses in one right-hand side, the last impulse alone"""
    ins = c.inputs(l, seed)
    return [ins[0], ('impulses', ins[1][1] + ins[2][1]), ins[2]]


# ---- 0. the plan on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_tail_plan(name):
    c = case(name)
    shape, nlig, maxp, t, points = CASES[name]
    assert c.tail == dict(level=t, nlevels=len(points), max_points=maxp, points=points, lds_bytes=lds_bytes(points, c.F), launches=c.tail['launches'])
    assert [c.info[t + q]['points'] for q in range(len(points))] == points and t + len(points) == c.nlev
    assert c.k.mg_coarse_info()['level'] == c.nlev - 1


# ---- 1. the tail against numpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nu', [1, 2, 3])
@pytest.mark.parametrize('name', list(CASES))
def test_tail_against_numpy(name, nu):
    c = case(name)
    t = c.tail['level']
    lv64, lvld = c.reference_levels()
    try:
        c.k.set_mg_params(nu=nu)
        n0 = c.k.mg_tail_info()['launches']
        for what, b in _rhs(c, t, 131):
            x64 = mr.vcycle(lv64, c.lig, S_CYCLE, b, nu, MG_RATIO, l=t)
            xld = mr.vcycle(lvld, c.lig, S_CYCLE, b.astype(LD), nu, MG_RATIO, l=t)
            d_ref = mr.rel_l2(x64, xld)
            got = c.field(c.k.mg_part(klib.MGP_TAIL, t, b, shift=S_CYCLE), t)
            d, bound = mr.rel_l2(got, xld), MARGIN * max(d_ref, TOL_OP)
            print('mg_tail TAIL %s level %d (%d levels, sweeps on the last %d) nu %d %s: d_ref %.3e distance %.3e head-room %.1f' %
                  (name, t, c.tail['nlevels'], lv64[-1].sweeps, nu, what, d_ref, d, bound / max(d, 1e-300)))
            assert d <= bound, ('TAIL', nu, what, d, d_ref)
            if what == 'random':
                assert np.array_equal(got, c.field(c.k.mg_part(klib.MGP_TAIL, t, b, shift=S_CYCLE), t))      # two calls: bit for bit
        assert c.k.mg_tail_info()['launches'] == n0 + 4
    finally:
        c.k.set_mg_params(nu=2)


# ---- 2. the whole cycle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_whole_cycle(name):
    """MGP_CYCLE at level 0 with the tail on: fp64 and (2-D) fp32 level vectors against the references and bounds of
    test_gpu_mg_parts.py::test_cycle; captured graph and eager launches bit for bit, two calls bit for bit, one tail launch per cycle"""
    c = case(name)
    t = c.tail['level']
    lv64, lvld = c.reference_levels()
    nstore = sum(1 for l in range(t) if c.info[l]['f32'])      # fp32 level vectors: above the tail only
    try:
        for what, b in _rhs(c, 0, 121):
            x64 = mr.vcycle(lv64, c.lig, S_CYCLE, b, 2, MG_RATIO)
            xld = mr.vcycle(lvld, c.lig, S_CYCLE, b.astype(LD), 2, MG_RATIO)
            d_ref = mr.rel_l2(x64, xld)
            if nstore:
                if 'copies' not in c._lv:
                    c._lv['copies'] = c.levels(S_CYCLE, copies=nstore)
                x64c = mr.vcycle(c._lv['copies'], c.lig, S_CYCLE, b, 2, MG_RATIO)
                x32c = mr.vcycle(c._lv['copies'], c.lig, S_CYCLE, b, 2, MG_RATIO, store=mr.store_f32, nstore=nstore)
            got = {}
            for eager in (False, True):
                c.k.set_mg_params(power_its=klib.MG_EAGER if eager else 0)
                n0 = c.k.mg_tail_info()['launches']
                g = c.field(c.k.mg_part(klib.MGP_CYCLE, 0, b, variant=0, shift=S_CYCLE), 0)
                assert c.k.mg_tail_info()['launches'] == n0 + 1
                d, bound = mr.rel_l2(g, xld), MARGIN * max(d_ref, TOL_OP)
                print('mg_tail CYCLE fp64 %s %s %s: d_ref %.3e distance %.3e head-room %.1f' % (name, 'eager' if eager else 'graph', what, d_ref, d, bound / max(d, 1e-300)))
                assert d <= bound, ('CYCLE', eager, d, d_ref)
                got[eager] = g
                if eager:
                    assert np.array_equal(g, c.field(c.k.mg_part(klib.MGP_CYCLE, 0, b, variant=0, shift=S_CYCLE), 0))
                if nstore:
                    g32 = c.field(c.k.mg_part(klib.MGP_CYCLE, 0, b, variant=1, shift=S_CYCLE), 0)
                    d32, dg = mr.rel_l2(x32c, x64c), mr.rel_l2(g32, x64c)
                    print('mg_tail CYCLE fp32 %s %s %s: %d fp32 levels, d32 %.3e distance %.3e head-room %.2f' %
                          (name, 'eager' if eager else 'graph', what, nstore, d32, dg, 4 * d32 / max(dg, 1e-300)))
                    assert d32 < 1e-5 and dg <= 4 * d32, ('CYCLE fp32', eager, dg, d32)
                    got[(eager, 32)] = g32
            assert np.array_equal(got[False], got[True])
            if nstore:
                assert np.array_equal(got[(False, 32)], got[(True, 32)])
        assert (nstore > 0) == (c.dim == 2)
    finally:
        c.k.set_mg_params(power_its=0)


# ---- 3. launches -------------------------------------------------------------------------------------------------------------------------
def _profile_launches(k):
    return sum(v['launches'] for v in k.profile().values())


@pytest.mark.parametrize('name', ['32x32', '16x16x16', '96'])
def test_launch_count(name):
    """one fixed stiff step (pc_type 1, h = 5) with eager launches: fewer launches with the tail, and ONE tail launch per V cycle: the
    launches a cycle saves are counted on the same handle at the same state (two MGP_CYCLE calls, eager), and the launches the step
    saves must be that number times the tail launches the handle counted"""
    shape, nlig, maxp = CASES[name][:3]
    cfg = _cfg(shape, nlig, tuple((0.01 if len(shape) == 3 else 0.0025) * n for n in shape))
    u = _state(cfg, 3, amp=0.01)
    b = np.random.default_rng(5).standard_normal((cfg.F,) + mr.grid_shape(shape))
    opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-9, pc_type=1)
    rec = {}
    for on in (False, True):
        k = klib.KSFDHip(cfg)
        k.set_mg_params(power_its=klib.MG_EAGER)
        if on:
            k.set_mg_tail(maxp)
        k.set_state(u)
        l0 = _profile_launches(k)
        k.mg_part(klib.MGP_CYCLE, 0, b, shift=S_CYCLE)
        per_cycle = _profile_launches(k) - l0
        n0 = k.mg_tail_info()['launches']
        t, hn, st, rc = k.step(0.0, 5.0, opts)
        rec[on] = (st.launches, st.linear_its, per_cycle, k.mg_tail_info()['launches'] - n0)
        assert st.pc_used & klib.PC_MULTIGRID
        k.close()
    (l_off, its_off, c_off, t_off), (l_on, its_on, c_on, t_on) = rec[False], rec[True]
    print('mg_tail launches %s: step without the tail %d, with it %d (linear_its %d / %d); per V cycle %d -> %d; tail launches %d' %
          (name, l_off, l_on, its_off, its_on, c_off, c_on, t_on))
    assert l_on < l_off and c_on < c_off and t_off == 0
    assert its_on == its_off and t_on >= its_on > 0
    assert l_off - l_on == t_on * (c_off - c_on)


# ---- 4. steps against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', list(STIFF))
def test_stiff_steps_vs_oracle(which):
    """the stiff steps of tests/test_gpu_mg_coarse.py (ksp_rtol 1e-11) with the tail on: 1e-10 against the oracle's LU step, and the
    linear iterations of the run without the tail (a difference of one is printed for the log; more than one fails)"""
    cfg, u, h = STIFF[which]()
    un = _oracle_step(which, cfg, u, h)
    opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-11, pc_type=1)
    out = {}
    for maxp in (0, 1024):
        k = klib.KSFDHip(cfg)
        k.set_mg_tail(maxp)
        k.set_state(u)
        t, hn, st, rc = k.step(0.0, h, opts)
        out[maxp] = (k.get_state(), st.linear_its, st.ksp_resid, st.launches, k.mg_tail_info())
        k.close()
    (s0, its0, res0, l0, _), (s1, its1, res1, l1, info) = out[0], out[1024]
    d0, d1 = rel_l2(s0, un), rel_l2(s1, un)
    print('mg_tail step %s: tail levels %d..%d (%s points), linear_its %d -> %d, last residual %.3e -> %.3e, launches %d -> %d, rel-L2 vs oracle %.3e -> %.3e' %
          (which, info['level'], info['level'] + info['nlevels'] - 1, info['points'], its0, its1, res0, res1, l0, l1, d0, d1))
    assert info['level'] >= 1 and info['launches'] >= its1
    assert d1 < 1e-10, (d1, d0)
    assert abs(its1 - its0) <= 1, (its0, its1)
    if its1 != its0:
        print('mg_tail step %s: linear_its differ by one; residuals that crossed the tolerance: %.3e (off) %.3e (on)' % (which, res0, res1))


# ---- 5. off is off -----------------------------------------------------------------------------------------------------------------------
def _three_steps(k, u, n=3):
    k.set_state(u)
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, pc_type=1)
    t, h, out = 0.0, 5.0, []
    for _ in range(n):
        t, h, st, rc = k.step(t, h, opts)
        assert st.pc_used & klib.PC_MULTIGRID
        out.append((t, h, st.linear_its, st.rejections, st.launches, k.get_state()))
    return out


def _same(a, b):
    for x, y in zip(a, b):
        assert x[:5] == y[:5] and np.array_equal(x[5], y[5])


def test_off_is_off():
    cfg, u, _ = STIFF['2d']()
    runs = []
    for touch in (False, True):
        k = klib.KSFDHip(cfg)
        if touch:
            k.set_mg_tail(1024)
            assert k.mg_tail_info()['level'] == 1
            k.set_mg_tail(0)
            assert k.mg_tail_info()['level'] == -1 and k.mg_tail_info()['max_points'] == 0
        runs.append(_three_steps(k, u))
        assert k.mg_tail_info()['launches'] == 0
        k.close()
    _same(*runs)


def test_no_level_qualifies():
    """max_points below the coarsest level's points: KSFD_OK, the info entry says -1, the steps are those of a fresh handle"""
    cfg, u, _ = STIFF['2d']()
    runs = []
    for touch in (False, True):
        k = klib.KSFDHip(cfg)
        if touch:
            k.set_mg_tail(63)                                  # the coarsest level of 32 x 32 has 64 points
            info = k.mg_tail_info()
            assert info['level'] == -1 and info['nlevels'] == 0 and info['points'] == [] and info['lds_bytes'] == 0 and info['max_points'] == 63
        runs.append(_three_steps(k, u))
        assert k.mg_tail_info()['launches'] == 0
        k.close()
    _same(*runs)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def _einval(fn, word):
    with pytest.raises(klib.KSFDError) as e:
        fn()
    assert e.value.code == klib.EINVAL and word in str(e.value), str(e.value)


def test_refusals_leave_the_handle_as_it_was():
    """each refusal on a fresh handle: KSFD_EINVAL with a message, nothing changed, and the following step is the one of a handle that
    never made the refused call"""
    cfg, u, _ = STIFF['2d']()

    def step_after(prepare):
        k = klib.KSFDHip(cfg)
        prepare(k)
        out = _three_steps(k, u, 1)
        k.close()
        return out
    plain = step_after(lambda k: None)
    with_tail = step_after(lambda k: k.set_mg_tail(1024))

    def negative(k):
        _einval(lambda: k.set_mg_tail(-1), 'negative')
        assert k.mg_tail_info()['level'] == -1 and k.mg_tail_info()['max_points'] == 0
    _same(step_after(negative), plain)

    def coarse_then_tail(k):
        k.set_mg_coarse(1)
        before = k.mg_coarse_info()
        _einval(lambda: k.set_mg_tail(1024), 'exclude')
        assert k.mg_tail_info()['level'] == -1 and k.mg_tail_info()['max_points'] == 0 and k.mg_coarse_info() == before
        k.set_mg_coarse(0)
    _same(step_after(coarse_then_tail), plain)

    def tail_then_coarse(k):
        k.set_mg_tail(1024)
        info = k.mg_tail_info()
        _einval(lambda: k.set_mg_coarse(1), 'exclude')
        assert k.mg_coarse_info()['kind'] == 0 and k.mg_tail_info() == info and info['level'] == 1
    _same(step_after(tail_then_coarse), with_tail)

    def wrong_level(k):
        k.set_mg_tail(1024)
        k.set_state(u)
        _einval(lambda: k.mg_part(klib.MGP_TAIL, 2, np.ones((3, 8, 8)), shift=S_CYCLE), 'tail')
        _einval(lambda: k.mg_part(klib.MGP_TAIL, 0, np.ones((3, 32, 32)), shift=S_CYCLE), 'tail')
        assert k.mg_tail_info()['launches'] == 0
    _same(step_after(wrong_level), with_tail)

    def tail_off(k):
        k.set_state(u)
        _einval(lambda: k.mg_part(klib.MGP_TAIL, 1, np.ones((3, 16, 16)), shift=S_CYCLE), 'tail')
    _same(step_after(tail_off), plain)
    # a handle without a hierarchy
    cfg = _cfg((33, 20), 1, (0.0825, 0.05))
    u = _state(cfg, 3, amp=0.05)
    out = []
    for attempt in (False, True):
        k = klib.KSFDHip(cfg)
        if attempt:
            _einval(lambda: k.set_mg_tail(1024), 'hierarchy')
            _einval(lambda: k.mg_tail_info(), 'hierarchy')
            k.set_mg_tail(0)                                   # nothing to switch off
        k.set_state(u)
        t, h, st, rc = k.step(0.0, 5.0, klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, pc_type=1))
        out.append((t, h, st.linear_its, st.rejections, st.pc_used, k.get_state()))
        k.close()
    assert out[0][:5] == out[1][:5] and np.array_equal(out[0][5], out[1][5])


# ---- 7. replicated levels on two slab ranks ---------------------------------------------------------------------------------------------
def _pair_worker(rank, size, port, outdir):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        from ksfd_amd.dist import open_handle, local_slab, gather_slabs
        cfg = _cfg((64, 64), 1, (0.16, 0.16))
        u_loc = local_slab(_state(cfg, 3, amp=0.01), cfg, rank, size)
        opts = lambda rtol: klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=rtol, pc_type=1)

        def steps(k):
            k.set_state(u_loc)
            n0 = k.mg_tail_info()['launches']
            t, states, log = 0.0, [], []
            for rtol in (1e-11, 1e-7, 1e-7, 1e-7):             # the four steps of tests/test_gpu_mg_agglomerate.py
                t, _, st, rc = k.step(t, 5.0, opts(rtol))
                states.append(k.get_state())
                log.append([st.linear_its, st.launches])
            return states, np.array(log, dtype=np.int64), k.mg_tail_info()['launches'] - n0
        ks, keep = open_handle(cfg, rank, size, 0, transport='host')
        res = {}
        rep = lambda: [int(ks.mg_level_info(l)['sloc'] == 64 >> l) for l in range(ks.mg_level_info(0)['nlevels'])]
        # the letter of the design: agglomerate(1) replicates nothing on two ranks of 64^2 (4 rows each down to 8^2): no level qualifies
        ks.set_mg_agglomerate(1)
        res['rep1'] = np.array(rep())
        ks.set_mg_tail(1024)
        res['level1'] = ks.mg_tail_info()['level']
        s_a, res['log1_on'], res['tail1'] = steps(ks)
        ks.set_mg_tail(0)
        s_b, res['log1_off'], _ = steps(ks)
        res['same1'] = np.array([np.array_equal(a, b) for a, b in zip(s_a, s_b)])
        # replicated levels: 16^2 and 8^2 whole on every rank; the tail is re-planned by the rebuild
        ks.set_mg_tail(1024)
        ks.set_mg_agglomerate(300)
        res['rep'] = np.array(rep())
        info = ks.mg_tail_info()
        res['level'], res['points'], res['lds'] = info['level'], np.array(info['points']), info['lds_bytes']
        s_on, res['log_on'], res['tail'] = steps(ks)
        ks.set_mg_tail(0)
        res['level_off'] = ks.mg_tail_info()['level']
        s_off, res['log_off'], res['tail_off'] = steps(ks)
        res['dist'] = np.array([rel_l2(gather_slabs(a, cfg), gather_slabs(b, cfg)) for a, b in zip(s_on, s_off)])
        ks.close()
        np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **res)
    finally:
        dist.destroy_process_group()


def test_replicated_levels_on_two_slab_ranks(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_pair_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    z = [np.load(str(tmp_path / ('rank%d.npz' % r))) for r in range(2)]
    for zz in z:
        assert zz['rep1'].tolist() == [0, 0, 0, 0] and int(zz['level1']) == -1 and int(zz['tail1']) == 0
        assert zz['same1'].all() and np.array_equal(zz['log1_on'], zz['log1_off'])
        assert zz['rep'].tolist() == [0, 0, 1, 1]
        assert int(zz['level']) == 2 and zz['points'].tolist() == [256, 64] and int(zz['lds']) == lds_bytes([256, 64], 2)      # the first replicated level
        assert int(zz['level_off']) == -1 and int(zz['tail_off']) == 0 and int(zz['tail']) >= int(zz['log_on'][:, 0].sum())
        assert np.array_equal(zz['log_on'], z[0]['log_on']) and np.array_equal(zz['log_off'], z[0]['log_off'])
        assert np.array_equal(zz['log_on'][:, 0], zz['log_off'][:, 0])       # the same iteration counts
        assert np.all(zz['log_on'][:, 1] < zz['log_off'][:, 1])              # fewer launches in every step
        assert np.all(zz['dist'] < 1e-9), zz['dist']
    print('mg_tail 2 slab ranks 64x64 x 2 fields, agglomerate(300) + tail(1024): tail levels 2..3, [linear_its, launches] per step without %s, with %s; rel-L2 between them %s' %
          (z[0]['log_off'].tolist(), z[0]['log_on'].tolist(), ['%.2e' % d for d in z[0]['dist']]))
