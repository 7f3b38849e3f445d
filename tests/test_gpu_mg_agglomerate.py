"""GPU, slab ranks sharing cuda:0 through the host transport: coarse-level agglomeration of the multigrid hierarchy
(ksfd_set_mg_agglomerate).  Below the last level the slab rule allows, every rank holds the WHOLE level; checked here are the level list
against the single-rank handle's, the transfers across the border (k_restrict2d_border / k_restrict3d_border + the all-reduce,
k_prolong_add2d_border / k_prolong_add3d_border) against tests/mg_reference.py on the gathered arrays, the coefficient planes and the
operator of the replicated levels against the single-rank handle's levels of the same index, the cycle against the numpy V cycle on the
gathered problem, the stiff steps of tests/test_gpu_dist.py against the single-rank state, off == never on, the refusals.

Bounds are those of tests/test_gpu_mg_parts.py for the same parts (transfers: (m + 2) eps |W| |v| elementwise; fp32 fine vector: one
float32 ulp; operator: rel-L2 1e-12 per field; cycle: 32 x max(d_ref, 1e-12), fp32 cycle: 4 x d32) and of tests/test_gpu_dist.py for the
steps (1e-9 at ksp_rtol 1e-11, 2e-6 at 1e-7, iterations <= 2 x single rank + 8).  One process group per case; every rank writes a file.

The fp32 border case is (256, 64) on 4 ranks: levels (256, 64), (128, 32), (64, 16) stay distributed (16, 8, 4 rows a rank), the strip
kernel serves all three (64 columns, 4 rows), so the border level (64, 16) reports f32 = 1 and (32, 8) is the first replicated level."""
import os

import numpy as np
import pytest

import mg_reference as mr
from ksfd_amd import lib as klib
from test_gpu_dist import _free_port
from test_gpu_mg_coarse import _cfg, _state
from test_gpu_mg_parts import EPS, LD, MARGIN, MG_RATIO, S_CYCLE, TOL_OP, f32, per_field, ulp32

pytestmark = pytest.mark.gpu

#        name        shape          ligands ranks max_points  steps
CASES = {'64x64': ((64, 64), 1, 4, 1, True),
         '64x64x64': ((64, 64, 64), 1, 4, 1, True),
         '32x32x32': ((32, 32, 32), 1, 4, 1, True),       # one more 3-D state: (32^3, 8 planes), (16^3, 4 planes), 8^3 replicated
         '64x64-300': ((64, 64), 1, 2, 300, False),       # also: the all-reduce of the border in pieces of 100 doubles (KSFD_VRED_MAX)
         '256x64': ((256, 64), 1, 4, 1, False)}


def _problem(name):
    shape, nlig = CASES[name][:2]
    cfg = _cfg(shape, nlig, tuple((0.01 if len(shape) == 3 else 0.0025) * n for n in shape))
    return cfg, _state(cfg, 3, amp=0.05)


def _levels(k):
    """[(extents as the level reports them, sloc, points)] of the handle's hierarchy"""
    n = k.mg_level_info(0)['nlevels']
    return [(lambda i: (i['n'], i['sloc'], i['points']))(k.mg_level_info(l)) for l in range(n)]


def _step_state(cfg):
    """state of the step sequence: 1 % noise, which four fixed steps h = 5 without error control leave physical on every handle
    (at the 5 % of the parts' state the third one no longer converges, single rank included)"""
    return _state(cfg, 3, amp=0.01)


def _steps(k, u_local, ksp_rtols=(1e-11, 1e-7, 1e-7, 1e-7)):
    """the h = 5 fixed steps of tests/test_gpu_dist.py (pc_type 1; ksp_rtol 1e-11, then 1e-7) and two more at 1e-7:
    (state after each, [linear_its, launches, host_syncs] of each)"""
    k.set_state(u_local)
    t, states, log = 0.0, [], []
    for rtol in ksp_rtols:
        t, _, st, rc = k.step(t, 5.0, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=rtol, pc_type=1))
        states.append(k.get_state())
        log.append([st.linear_its, st.launches, st.host_syncs])
    return states, np.array(log, dtype=np.int64)


def _inputs(shape_l, seed):
    v = np.random.default_rng(seed).standard_normal(shape_l)
    v.reshape(-1)[0] += 1.0                      # the first and the last point: index errors at the wrap show
    v.reshape(-1)[-1] += 1.0
    return v


def _worker(rank, size, port, name, outdir):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        from ksfd_amd.dist import open_handle, local_slab, gather_slabs
        shape, nlig, _, maxp, with_steps = CASES[name]
        dim = len(shape)
        cfg, u = _problem(name)
        F = cfg.F
        if name == '64x64-300':
            os.environ['KSFD_VRED_MAX'] = '100'                  # 512 doubles of the border vector, 1024 of its planes: 6 and 11 pieces
        ks, keep = open_handle(cfg, rank, size, 0, transport='host')
        u_loc = local_slab(u, cfg, rank, size)
        ks.set_state(u_loc)
        res = {}
        today = _levels(ks)
        if name == '64x64':
            # refusals change nothing and involve no collective
            assert ks.L.ksfd_set_mg_agglomerate(ks.h, -1) == klib.EINVAL and 'negative' in ks.last_error()
            assert _levels(ks) == today
        ks.set_mg_agglomerate(maxp)
        info = [ks.mg_level_info(l) for l in range(ks.mg_level_info(0)['nlevels'])]
        nlev = len(info)
        ks.set_mg_agglomerate(0)
        assert _levels(ks) == today                              # off: today's list
        ks.set_mg_agglomerate(maxp)
        assert [ks.mg_level_info(l) for l in range(nlev)] == info
        if name == '64x64':
            assert ks.L.ksfd_set_mg_coarse(ks.h, 1, 0) == klib.EINVAL and 'single rank' in ks.last_error()      # as on every transport handle
        # global extents per level; a level is replicated where it reports the whole slow extent (more than one rank: sloc == global)
        nglob = [tuple(shape[a] >> l for a in range(dim)) for l in range(nlev)]
        rep = [info[l]['sloc'] == nglob[l][dim - 1] for l in range(nlev)]
        res['nlev'], res['ntoday'] = nlev, len(today)
        res['n'] = np.array([list(i['n']) for i in info])
        res['sloc'] = np.array([i['sloc'] for i in info])
        res['points'] = np.array([i['points'] for i in info])
        res['f32'] = np.array([i['f32'] for i in info])
        res['end'] = np.array([i['end_level'] for i in info])
        gshape = lambda l, planes=F: (planes,) + mr.grid_shape(nglob[l])

        def mine(a, l):                                          # what this rank passes of a global level array
            if rep[l]:
                return a
            s = info[l]['sloc']
            return np.ascontiguousarray(a[:, rank * s:(rank + 1) * s])
        # transfers between every pair of levels: within the slabs, across the border, within the replicated levels
        for l in range(nlev - 1):
            v, w = _inputs(gshape(l), 21 + l), _inputs(gshape(l + 1), 41 + l)
            res['r%d' % l] = ks.mg_part(klib.MGP_RESTRICT, l, mine(v, l))
            res['p%d' % l] = ks.mg_part(klib.MGP_PROLONG_ADD, l, mine(v, l), mine(w, l + 1))
            if info[l]['f32'] and rep[l + 1]:                    # the border with an fp32 fine vector
                res['r32_%d' % l] = ks.mg_part(klib.MGP_RESTRICT, l, mine(v, l), variant=1)
                res['p32_%d' % l] = ks.mg_part(klib.MGP_PROLONG_ADD, l, mine(v, l), mine(w, l + 1), variant=1)
        # planes, operator, set-up of every level; the cycle
        for l in range(nlev):
            inf = ks.mg_level_info(l, S_CYCLE)
            c, c32 = ks.mg_part(klib.MGP_COEF, l)
            res['coef%d' % l] = c
            if c32 is not None:
                res['coef32_%d' % l] = c32
            res['coef32bit%d' % l] = inf['coef32'] & 1
            res['dinv%d' % l] = ks.mg_part(klib.MGP_DINV, l, shift=S_CYCLE)
            res['set%d' % l] = np.array([inf['lam_max'], inf['ratio'], inf['coarse_sweeps']])
            if rep[l]:
                res['op%d' % l] = ks.mg_part(klib.MGP_OPERATOR, l, _inputs(gshape(l), 95 + l), variant=1, shift=S_CYCLE)
        b = _inputs(gshape(0), 121)
        res['cycle'] = ks.mg_part(klib.MGP_CYCLE, 0, mine(b, 0), variant=0, shift=S_CYCLE)
        if dim == 2:
            res['cycle32'] = ks.mg_part(klib.MGP_CYCLE, 0, mine(b, 0), variant=1, shift=S_CYCLE)
        if with_steps:
            us = _step_state(cfg)
            u_loc = local_slab(us, cfg, rank, size)
            states, log = _steps(ks, u_loc)
            res['log_on'] = log
            for q, s in enumerate(states):
                g = gather_slabs(s, cfg)
                if rank == 0:
                    res['state_on%d' % q] = g
            # parent behaviour for the record, and off == never on: switched on, then off, against a handle never touched
            ks.set_mg_agglomerate(0)
            states_off, res['log_off'] = _steps(ks, u_loc)
            k2, keep2 = open_handle(cfg, rank, size, 0, transport='host')
            states_never, res['log_never'] = _steps(k2, u_loc)
            k2.close()
            res['off_equals_never'] = np.array([np.array_equal(a, c) for a, c in zip(states_off, states_never)])
        ks.close()
        if rank == 0:
            one = klib.KSFDHip(cfg)
            one.set_state(u)
            assert one.L.ksfd_set_mg_agglomerate(one.h, 1) == klib.OK        # no transport: nothing changes
            i1 = [one.mg_level_info(l) for l in range(one.mg_level_info(0)['nlevels'])]
            res['one_n'] = np.array([list(i['n']) for i in i1])
            for l in range(min(nlev, len(i1))):
                if rep[l] or l == 0:
                    res['one_coef%d' % l] = one.mg_part(klib.MGP_COEF, l)[0]
                if rep[l]:
                    res['one_op%d' % l] = one.mg_part(klib.MGP_OPERATOR, l, _inputs(gshape(l), 95 + l), variant=1, shift=S_CYCLE)
            if with_steps:
                states, res['log_one'] = _steps(one, _step_state(cfg))
                for q, s in enumerate(states):
                    res['state_one%d' % q] = s
            one.close()
        np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **res)
    finally:
        dist.destroy_process_group()


_RESULTS = {}


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    """one spawn per case, shared by the tests of that case"""
    import torch.multiprocessing as mp

    def get(name):
        if name not in _RESULTS:
            d, size = tmp_path_factory.mktemp('agg-' + name), CASES[name][2]
            mp.spawn(_worker, args=(size, _free_port(), name, str(d)), nprocs=size, join=True)
            _RESULTS[name] = [dict(np.load(str(d / ('rank%d.npz' % r)))) for r in range(size)]
        return _RESULTS[name]
    yield get
    _RESULTS.clear()


def _geometry(name, z):
    shape, nlig, size, maxp, _ = CASES[name]
    dim, nlev = len(shape), int(z[0]['nlev'])
    nglob = [tuple(shape[a] >> l for a in range(dim)) for l in range(nlev)]
    rep = [int(z[0]['sloc'][l]) == nglob[l][dim - 1] for l in range(nlev)]
    return dim, nlig + 1, size, nlev, nglob, rep


def _whole(name, z, key, l, planes=None):
    """the global array of level l from what the ranks returned: slabs joined, or rank 0's copy of a replicated level"""
    dim, F, size, nlev, nglob, rep = _geometry(name, z)
    planes = planes or F
    if rep[l]:
        return z[0][key].reshape((planes,) + mr.grid_shape(nglob[l]))
    g = mr.grid_shape(nglob[l])
    loc = (planes, g[0] // size) + g[1:]
    return np.concatenate([zz[key].reshape(loc) for zz in z], axis=1)


@pytest.mark.parametrize('name', ['64x64', '64x64x64', '32x32x32', '64x64-300', '256x64'])
def test_level_list(run, name):
    z = run(name)
    dim, F, size, nlev, nglob, rep = _geometry(name, z)
    want_rep = {'64x64': [0, 0, 0, 1], '64x64x64': [0, 0, 0, 1], '32x32x32': [0, 0, 1], '64x64-300': [0, 0, 1, 1], '256x64': [0, 0, 0, 1]}[name]
    assert [int(r) for r in rep] == want_rep and int(z[0]['ntoday']) == {'64x64-300': 4, '32x32x32': 2}.get(name, 3)
    one_n = z[0]['one_n']
    assert one_n.shape[0] == nlev                                   # as deep as the single-rank hierarchy
    for zz in z:                                                    # every rank
        assert int(zz['nlev']) == nlev and np.all(zz['end'] == nlev - 1)
        for l in range(nlev):
            n = [int(x) for x in zz['n'][l]]
            sloc = int(zz['sloc'][l])
            assert sloc == (nglob[l][dim - 1] if rep[l] else nglob[l][dim - 1] // size)
            n[dim - 1] = sloc if rep[l] else sloc * size
            assert n == [int(x) for x in one_n[l]], (l, n)
            assert int(zz['points'][l]) == sloc * int(np.prod(nglob[l][:dim - 1]))
            assert not (rep[l] and zz['f32'][l])                    # replicated levels keep fp64 vectors
    if name == '256x64':
        assert z[0]['f32'][2] and not rep[2] and rep[3]             # the border level has fp32 vectors


@pytest.mark.parametrize('name', ['64x64', '64x64x64', '32x32x32', '64x64-300', '256x64'])
def test_transfers(run, name):
    z = run(name)
    dim, F, size, nlev, nglob, rep = _geometry(name, z)
    gshape = lambda l: (F,) + mr.grid_shape(nglob[l])
    border = 0
    for l in range(nlev - 1):
        v, w = _inputs(gshape(l), 21 + l), _inputs(gshape(l + 1), 41 + l)
        ref = mr.restrict(v.astype(LD), dim)
        bound = (3 ** dim + 2) * EPS * mr.restrict(np.abs(v), dim)
        got = _whole(name, z, 'r%d' % l, l + 1)
        assert np.all(np.abs(got - ref.astype(np.float64)) <= bound), ('RESTRICT', l)
        if rep[l + 1]:
            for zz in z[1:]:                                        # the gathered vector: the same bits on every rank
                assert np.array_equal(zz['r%d' % l], z[0]['r%d' % l]), ('RESTRICT', l)
        ref = v.astype(LD) + mr.prolong(w.astype(LD), dim)
        bound = (2 ** dim + 1 + 2) * EPS * (np.abs(v) + mr.prolong(np.abs(w), dim))
        got = _whole(name, z, 'p%d' % l, l)
        assert np.all(np.abs(got - ref.astype(np.float64)) <= bound), ('PROLONG_ADD', l)
        if rep[l]:
            for zz in z[1:]:
                assert np.array_equal(zz['p%d' % l], z[0]['p%d' % l]), ('PROLONG_ADD', l)
        border += rep[l + 1] and not rep[l]
        if 'r32_%d' % l in z[0]:
            # fine fp32, coarse fp64 (k_restrict2d_border<float>, k_prolong_add2d_border<float>): the bounds of the same storage-type pair
            ref = mr.restrict(f32(v).astype(LD), dim)
            bound = (9 + 2) * EPS * mr.restrict(np.abs(f32(v)), dim)
            assert np.all(np.abs(_whole(name, z, 'r32_%d' % l, l + 1) - ref.astype(np.float64)) <= bound), ('RESTRICT<float,double>', l)
            for zz in z[1:]:
                assert np.array_equal(zz['r32_%d' % l], z[0]['r32_%d' % l])
            ref = f32(f32(v).astype(LD) + mr.prolong(w.astype(LD), dim))
            assert np.all(np.abs(_whole(name, z, 'p32_%d' % l, l) - ref) <= ulp32(ref)), ('PROLONG_ADD<double,float>', l)
    assert border == 1
    lb = rep.index(True) - 1                                        # the border level: its fp32 variant ran wherever it has fp32 vectors
    assert ('r32_%d' % lb in z[0]) == bool(z[0]['f32'][lb])
    if name == '256x64':
        assert 'r32_2' in z[0]


@pytest.mark.parametrize('name', ['64x64', '64x64x64', '64x64-300'])
def test_planes_and_operator_of_replicated_levels(run, name):
    z = run(name)
    dim, F, size, nlev, nglob, rep = _geometry(name, z)
    nlig = F - 1
    for l in range(nlev):
        if not rep[l]:
            continue
        for zz in z[1:]:
            assert np.array_equal(zz['coef%d' % l], z[0]['coef%d' % l]) and np.array_equal(zz['op%d' % l], z[0]['op%d' % l])
        assert 'coef32_%d' % l not in z[0]                          # fp64 planes only
        # planes: the full weighting of the level above, as tests/test_gpu_mg_parts.py asserts it ...
        fine, coarse = _whole(name, z, 'coef%d' % (l - 1), l - 1, 3 + nlig), _whole(name, z, 'coef%d' % l, l, 3 + nlig)
        ref = mr.restrict(fine.astype(LD), dim)
        bound = (3 ** dim + 2) * EPS * mr.restrict(np.abs(fine), dim)
        assert np.all(np.abs(coarse - ref.astype(np.float64)) <= bound), ('COEF', l)
        # ... and the single-rank handle's level of the same index.  Both are l full weightings of level 0, each within the bound above
        # of the exact one: the distance is at most what separates the two level-0 planes, restricted l times, plus 2 l of those bounds
        c0 = _whole(name, z, 'coef0', 0, 3 + nlig)
        e0, a = np.abs(c0 - z[0]['one_coef0'].reshape(c0.shape)), np.abs(c0)
        for _ in range(l):
            e0, a = mr.restrict(e0, dim), mr.restrict(a, dim)
        one = z[0]['one_coef%d' % l].reshape(coarse.shape)
        assert np.all(np.abs(coarse - one) <= e0 + 2 * l * (3 ** dim + 2) * EPS * a), ('COEF single rank', l)
        got, want = (z[0][k % l].reshape((F,) + mr.grid_shape(nglob[l])) for k in ('op%d', 'one_op%d'))
        assert per_field(got, want) < TOL_OP, ('OPERATOR', l, per_field(got, want))


def _reference_levels(name, z, copies=0):
    dim, F, size, nlev, nglob, rep = _geometry(name, z)
    shape, nlig = CASES[name][:2]
    h0 = 0.01 if dim == 3 else 0.0025
    out = []
    for l in range(nlev):
        for zz in z[1:]:
            assert np.array_equal(zz['set%d' % l], z[0]['set%d' % l])            # every rank runs the same cycle
        key = 'coef32_%d' % l if ('coef32_%d' % l in z[0] and (l < copies or (l == 0 and int(z[0]['coef32bit0'])))) else 'coef%d' % l
        lam, ratio, sweeps = z[0]['set%d' % l]
        out.append(mr.Level(_whole(name, z, key, l, 3 + nlig), [h0 * 2 ** l] * dim, mr.planes_to_blocks(_whole(name, z, 'dinv%d' % l, l, F * F), F),
                            float(lam), float(ratio), int(sweeps)))
    return out


@pytest.mark.parametrize('name', ['64x64', '64x64x64', '32x32x32', '64x64-300', '256x64'])
def test_cycle(run, name):
    z = run(name)
    dim, F, size, nlev, nglob, rep = _geometry(name, z)
    cfg, _ = _problem(name)
    lig = dict(s=list(cfg.lig_s), gamma=list(cfg.lig_gamma), D=list(cfg.lig_D))
    b = _inputs((F,) + mr.grid_shape(nglob[0]), 121)
    levels = _reference_levels(name, z)
    x64 = mr.vcycle(levels, lig, S_CYCLE, b, 2, MG_RATIO)
    xld = mr.vcycle([L.astype(LD) for L in levels], lig, S_CYCLE, b.astype(LD), 2, MG_RATIO)
    d_ref, d = mr.rel_l2(x64, xld), mr.rel_l2(_whole(name, z, 'cycle', 0), xld)
    print('mg_agglomerate CYCLE fp64 %s: sweeps on the last level %d, d_ref %.3e distance %.3e head-room %.1f' %
          (name, levels[-1].sweeps, d_ref, d, MARGIN * max(d_ref, TOL_OP) / max(d, 1e-300)))
    assert d <= MARGIN * max(d_ref, TOL_OP)
    if dim == 2:
        nstore = int(sum(zz for zz in z[0]['f32']))
        lvc = _reference_levels(name, z, copies=nstore)
        x64c = mr.vcycle(lvc, lig, S_CYCLE, b, 2, MG_RATIO)
        x32c = mr.vcycle(lvc, lig, S_CYCLE, b, 2, MG_RATIO, store=mr.store_f32, nstore=nstore)
        d32, dg = mr.rel_l2(x32c, x64c), mr.rel_l2(_whole(name, z, 'cycle32', 0), x64c)
        print('mg_agglomerate CYCLE fp32 %s: %d fp32 levels, d32 %.3e distance %.3e head-room %.2f' % (name, nstore, d32, dg, 4 * d32 / max(dg, 1e-300)))
        assert nstore >= 1 and d32 < 1e-5 and dg <= 4 * d32


@pytest.mark.parametrize('name', ['64x64', '64x64x64', '32x32x32'])
def test_steps(run, name):
    z = run(name)
    from conftest import rel_l2
    d11, d7 = rel_l2(z[0]['state_on0'], z[0]['state_one0']), rel_l2(z[0]['state_on1'], z[0]['state_one1'])
    print('mg_agglomerate steps %s: [linear_its, launches, host_syncs] per step: single rank %s, slabs off %s, slabs on %s; rel-L2 %.3e (1e-11), %.3e (1e-7)' %
          (name, z[0]['log_one'].tolist(), z[0]['log_off'].tolist(), z[0]['log_on'].tolist(), d11, d7))
    assert d11 < 1e-9 and d7 < 2e-6
    assert z[0]['log_on'].shape == (4, 3) and z[0]['log_one'].shape == (4, 3)
    for q in range(4):                                              # the stiff step and the three behind it
        assert 0 < z[0]['log_on'][q, 0] <= 2 * z[0]['log_one'][q, 0] + 8, (q, z[0]['log_on'][q, 0], z[0]['log_one'][q, 0])
    for zz in z:
        assert np.array_equal(zz['log_on'], z[0]['log_on'])         # every rank takes the same decisions
        # off == never on: the same states bit for bit, the same iterations, launches and host waits
        assert zz['off_equals_never'].all() and np.array_equal(zz['log_off'], zz['log_never'])


def _einval(fn, word):
    with pytest.raises(klib.KSFDError) as e:
        fn()
    assert e.value.code == klib.EINVAL and word in str(e.value), str(e.value)


def test_refusals_and_the_plain_handle():
    from ksfd_amd.dist import open_self_ring
    # a handle without a transport: KSFD_OK, nothing changes (a negative value is refused all the same)
    cfg = _cfg((32, 32), 1)
    k = klib.KSFDHip(cfg)
    k.set_state(_state(cfg, 3, amp=0.05))
    v = np.random.default_rng(1).standard_normal((2, 32, 32))
    before, x0 = _levels(k), k.mg_part(klib.MGP_CYCLE, 0, v, shift=S_CYCLE)
    k.set_mg_agglomerate(1)
    k.set_mg_agglomerate(10 ** 6)
    assert _levels(k) == before and np.array_equal(k.mg_part(klib.MGP_CYCLE, 0, v, shift=S_CYCLE), x0)
    _einval(lambda: k.set_mg_agglomerate(-1), 'negative')
    k.close()
    # 1-D with a transport, and a transport handle without a hierarchy (odd nx)
    for shape, word in (((96,), '1-D'), ((33, 20), 'hierarchy')):
        cfg = _cfg(shape, 1)
        k, keep = open_self_ring(cfg, 0, 'host')
        k.set_state(_state(cfg, 3, amp=0.05))
        before = _levels(k) if len(shape) == 1 else None
        _einval(lambda: k.set_mg_agglomerate(1), word)
        _einval(lambda: k.set_mg_agglomerate(-3), 'negative')
        if before:
            assert _levels(k) == before
        k.close()


def test_ring_of_one_replicates_by_size():
    """(64, 48) on a ring of one rank: the slab rule allows (64, 48), (32, 24), (16, 12); 400 points replicate (16, 12), 800 also (32, 24).
    The whole border path -- slice of the zeroed vector, all-reduce through the transport, wrapped prolongation -- in one process, and the
    cycle against the reference on the downloaded planes, blocks and bounds"""
    from ksfd_amd.dist import open_self_ring
    cfg = _cfg((64, 48), 1, (0.16, 0.12))
    lig = dict(s=list(cfg.lig_s), gamma=list(cfg.lig_gamma), D=list(cfg.lig_D))
    k, keep = open_self_ring(cfg, 0, 'host')
    k.set_state(_state(cfg, 3, amp=0.05))
    before = _levels(k)
    assert [n[:2] for n, _, _ in before] == [(64, 48), (32, 24), (16, 12)]
    b = _inputs((2, 48, 64), 121)
    for maxp in (400, 800):
        k.set_mg_agglomerate(maxp)
        assert _levels(k) == before                                 # one rank: slab and whole level have the same extents
        levels = []
        for l in range(3):
            inf = k.mg_level_info(l, S_CYCLE)
            c, c32 = k.mg_part(klib.MGP_COEF, l)
            if l >= 1:
                assert (c32 is None) == (l >= (2 if maxp == 400 else 1))      # a replicated level has fp64 planes only
            g = mr.grid_shape(inf['n'][:2])
            C = (c32 if (l == 0 and inf['coef32'] & 1) else c).reshape((4,) + g)
            levels.append(mr.Level(C, [0.0025 * 2 ** l] * 2, mr.planes_to_blocks(k.mg_part(klib.MGP_DINV, l, shift=S_CYCLE).reshape((4,) + g), 2),
                                   inf['lam_max'], inf['ratio'], inf['coarse_sweeps']))
        for l in range(2):
            g, gc = mr.grid_shape(before[l][0][:2]), mr.grid_shape(before[l + 1][0][:2])
            v, w = _inputs((2,) + g, 21 + l), _inputs((2,) + gc, 41 + l)
            got = k.mg_part(klib.MGP_RESTRICT, l, v).reshape((2,) + gc)
            assert np.all(np.abs(got - mr.restrict(v.astype(LD), 2).astype(np.float64)) <= 11 * EPS * mr.restrict(np.abs(v), 2)), (maxp, l)
            got = k.mg_part(klib.MGP_PROLONG_ADD, l, v, w).reshape((2,) + g)
            ref = v.astype(LD) + mr.prolong(w.astype(LD), 2)
            assert np.all(np.abs(got - ref.astype(np.float64)) <= 7 * EPS * (np.abs(v) + mr.prolong(np.abs(w), 2))), (maxp, l)
        x64 = mr.vcycle(levels, lig, S_CYCLE, b, 2, MG_RATIO)
        xld = mr.vcycle([L.astype(LD) for L in levels], lig, S_CYCLE, b.astype(LD), 2, MG_RATIO)
        d_ref, d = mr.rel_l2(x64, xld), mr.rel_l2(k.mg_part(klib.MGP_CYCLE, 0, b, shift=S_CYCLE).reshape(b.shape), xld)
        print('mg_agglomerate CYCLE fp64 ring of one, max_points %d: d_ref %.3e distance %.3e' % (maxp, d_ref, d))
        assert d <= MARGIN * max(d_ref, TOL_OP)
    k.set_mg_agglomerate(0)
    assert _levels(k) == before
    k.close()
