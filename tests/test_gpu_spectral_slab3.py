"""GPU, 2 or 4 ranks sharing cuda:0 over the host transport: the slab-distributed spectral solver on 3 * 2^k grids (the reference's own
384^2 and 1536^2 are of this kind).  Two things are new against the power-of-two slabs of test_gpu_dist.py: the ownership of the
spectral x positions behind a radix-3 stage (48 pieces of nx/48 positions), and local row counts 3 * 2^j, which travel as three
chunks of 2^j rows so that the column kernel still sees pieces of a power of two.  Same worker, same assertions and tolerances as
test_slab_distributed_spectral_solver_matches_single_rank: the error source is the same (fp32 transforms, other summation order)."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import rel_l2
from ksfd_amd.config import ProblemConfig
from test_gpu_dist import _free_port, _spectral_worker

pytestmark = pytest.mark.gpu


def _run_spectral(size, shape, nlig, tmp_path):
    outfile = str(tmp_path / 'result.npz')
    mp.spawn(_spectral_worker, args=(size, _free_port(), shape, nlig, outfile), nprocs=size, join=True)
    z = np.load(outfile)
    print('ranks %d shape %s nlig %d: pc_used %d, operator rel_l2 %.3e, state rel_l2 %.3e, iterations %d (one rank: %d)' %
          (size, shape, nlig, int(z['got_pc']), rel_l2(z['got_spec'], z['ref_spec']), rel_l2(z['got_state'], z['ref_state']),
           int(z['got_its']), int(z['ref_its'])))
    assert int(z['got_pc']) & 8                                   # the spectral solver really ran on the slabs
    assert rel_l2(z['got_spec'], z['ref_spec']) < 1e-5
    assert rel_l2(z['got_state'], z['ref_state']) < 1e-9
    assert z['got_its'] <= z['ref_its'] + 4


@pytest.mark.parametrize('size,shape,nlig', [
    (2, (48, 64), 1),       # radix-3 ownership only (power-of-two local rows); nx/48 = 1 column per piece
    (2, (64, 96), 1),       # non-power-of-two local rows only (48 = 3 * 16)
    (2, (48, 48), 3),       # both; local rows 24; F = 4, two complex pairs (grouped ligands)
    (4, (96, 192), 2),      # both; four ranks; odd field count (one half-empty pair)
    (4, (192, 48), 1),      # local rows 12 = 3 * 4, the smallest chunk of the cases; more x pieces than rows
])
def test_slab_spectral_solver_on_three_times_power_of_two_grids(size, shape, nlig, tmp_path):
    _run_spectral(size, shape, nlig, tmp_path)


def test_power_of_two_slabs_still_reproduce_one_rank(tmp_path):
    _run_spectral(2, (64, 64), 1, tmp_path)


def test_ring_of_one_rccl_transport_three_chunks():
    """ksfd_dist{size 1, transport 1} on (48, 96): the all-to-all blocks (48 pieces x 3 chunks of 32 rows) are all this rank's own and
    go through the RCCL transport's device copies; against the plain wrap-index handle"""
    from ksfd_amd import lib as klib
    from ksfd_amd.dist import open_self_ring, spectral_selftest
    shape, nlig = (48, 96), 1
    cfg = ProblemConfig.standard(2, shape, L=tuple(n * 4.0 / 1536 for n in shape), nlig=nlig)
    rng = np.random.default_rng(3)
    N = cfg.N
    rho = 9000 + 90 * rng.standard_normal(N)
    u = np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] * (1 + 0.01 * rng.standard_normal(N)) for l in range(nlig)])
    v = rng.standard_normal(cfg.F * N)
    ks, keep = open_self_ring(cfg, 0, 'rccl')
    one = klib.KSFDHip(cfg)
    try:
        assert ks.transport_name == 'rccl-self'
        assert spectral_selftest(ks, cfg, 0, 1)
        ks.set_state(u), one.set_state(u)
        e_op = rel_l2(ks.spectral_apply(3.0, v), one.spectral_apply(3.0, v))
        sp = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-11, pc_type=4)
        t, h, st, rc = ks.step(0.0, 0.3, sp)
        t1, h1, st1, rc = one.step(0.0, 0.3, sp)
        e_st = rel_l2(ks.get_state(), one.get_state())
        print('ring of one, rccl, %s: operator rel_l2 %.3e, state rel_l2 %.3e, pc_used %d / %d' % (shape, e_op, e_st, st.pc_used, st1.pc_used))
        assert e_op < 1e-5                                        # fp32 transforms, different summation order
        assert st.pc_used & 8 and st1.pc_used & 8
        assert e_st < 1e-9
    finally:
        ks.close()
        one.close()


def _ineligible_worker(rank, size, port, shape, outfile):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        from ksfd_amd import lib as klib
        from ksfd_amd.dist import open_handle, local_slab, gather_slabs, spectral_selftest
        cfg = ProblemConfig.standard(2, shape, L=tuple(n * 4.0 / 1536 for n in shape), nlig=1)
        rng = np.random.default_rng(3)
        N = cfg.N
        rho = 9000 + 90 * rng.standard_normal(N)
        u = np.concatenate([rho, rho * cfg.lig_s[0] / cfg.lig_gamma[0] * (1 + 0.01 * rng.standard_normal(N))])
        v = rng.standard_normal(cfg.F * N)
        ks, keep = open_handle(cfg, rank, size, 0, transport='host')
        mine = lambda a: local_slab(a, cfg, rank, size)
        assert spectral_selftest(ks, cfg, rank, size)             # nothing to check: True
        ks.set_state(mine(u))
        code = -1
        try:
            ks.spectral_apply(3.0, mine(v))
        except klib.KSFDError as e:
            code = e.code
        codes = [None] * size
        dist.all_gather_object(codes, code)
        opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-11)          # pc_type 2, the default
        t, h, st, rc = ks.step(0.0, 0.3, opts)
        state = gather_slabs(ks.get_state(), cfg)
        ks.close()
        if rank == 0:
            one = klib.KSFDHip(cfg)
            one.set_state(u)
            one.step(0.0, 0.3, opts)
            np.savez(outfile, codes=np.array(codes), einval=np.array(klib.EINVAL), pc=np.array(st.pc_used), got=state, ref=one.get_state())
            one.close()
    finally:
        dist.destroy_process_group()


def test_too_few_local_rows_keep_the_other_solvers(tmp_path):
    """A slab handle below the spectral solver's extents ends as before: KSFD_EINVAL from spectral_apply on every rank, steps through
    the other solvers.  Shape (48, 12) on 2 ranks: 6 = 3 * 2 local rows of a y extent shorter than the shortest plan (48).  The
    shape with 3 local rows, (48, 6), cannot be opened on 2 ranks at all -- ksfd_create and dist.slab_range ask for >= 4 slab units
    per rank because of the width-2 ghosts, checked first below -- so the smallest 3 * 2^k shape that can be opened stands in."""
    from ksfd_amd.dist import slab_range
    with pytest.raises(ValueError):
        slab_range(6, 0, 2)
    outfile = str(tmp_path / 'result.npz')
    mp.spawn(_ineligible_worker, args=(2, _free_port(), (48, 12), outfile), nprocs=2, join=True)
    z = np.load(outfile)
    assert list(z['codes']) == [int(z['einval'])] * 2
    assert not int(z['pc']) & 8
    assert rel_l2(z['got'], z['ref']) < 1e-9
