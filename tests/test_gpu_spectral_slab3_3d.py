"""GPU, 2 to 4 ranks sharing cuda:0 over the host transport: the slab-distributed spectral solver on the shapes that were left to the
other solvers on slab ranks -- 3-D boxes with a 3 * 2^k extent on any axis (x: radix-3 ownership of the spectral positions; y: local,
the R3 y kernels behind the ring path; z: 3 * 2^j local planes travelling as three chunks of 2^j, a received z column being 3 P
pieces), and the 2-D two-phase column kernel (KSFD_SPEC_SPLIT) with 3 * 2^k extents.  Same worker, same assertions and tolerances as
test_slab_distributed_spectral_solver_matches_single_rank: the error source is the same (fp32 transforms in another summation order).
The smallest shapes that reach each piece of the new code; P = 8 is covered by test_spectral_ownership3d_cpu.py."""
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
    (2, (48, 32, 32), 1),   # radix-3 ownership of x in 3-D, one position per piece
    (2, (32, 48, 32), 1),   # y = 3 * 2^k on slab ranks (local: the R3 y kernels behind the ring path)
    (2, (32, 32, 48), 1),   # z = 3 * 2^k: 24 local planes = 3 chunks of 8
    (4, (48, 48, 96), 2),   # all three axes, four ranks, odd field count (half-empty pair)
    (4, (96, 32, 48), 1),   # 12 local planes = 3 chunks of 4, the smallest chunk of the cases
])
def test_slab_spectral_solver_3d_on_three_times_power_of_two_boxes(size, shape, nlig, tmp_path):
    _run_spectral(size, shape, nlig, tmp_path)


@pytest.mark.parametrize('size,shape,nlig,split', [
    (2, (64, 96), 2, 1),    # split columns of 3 * 2^k points as 3 P pieces
    (2, (96, 64), 2, 1),    # split columns behind radix-3 x ownership only
    (4, (96, 192), 3, 1),   # both, F = 4 (two full pairs), four ranks
    (2, (48, 96), 1, 2),    # one column per block (kspec_cols_symbol_split1) across pieces
])
def test_slab_split_column_kernel_on_three_times_power_of_two_grids(size, shape, nlig, split, tmp_path, monkeypatch):
    monkeypatch.setenv('KSFD_SPEC_SPLIT', str(split))             # the ranks inherit the knob
    _run_spectral(size, shape, nlig, tmp_path)


def _state(cfg, nlig, seed=3):
    rng = np.random.default_rng(seed)
    N = cfg.N
    rho = 9000 + 90 * rng.standard_normal(N)
    u = np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] * (1 + 0.01 * rng.standard_normal(N)) for l in range(nlig)])
    return u, rng.standard_normal(cfg.F * N)


@pytest.mark.parametrize('shape,nlig,split', [((48, 32, 48), 1, None), ((48, 96), 2, '1')])
def test_ring_of_one_rccl_transport_3d_chunks_and_split_columns(shape, nlig, split, monkeypatch):
    """ksfd_dist{size 1, transport 1}: every all-to-all block is this rank's own and goes through the RCCL transport's device copies.
    (48, 32, 48): 48 x pieces x 3 chunks of 16 planes, z columns of 3 pieces; (48, 96) split: 3 chunks of 32 rows, the result coming
    home with the two work arrays' roles swapped.  Against the plain wrap-index handle."""
    from ksfd_amd import lib as klib
    from ksfd_amd.dist import open_self_ring, spectral_selftest
    if split:
        monkeypatch.setenv('KSFD_SPEC_SPLIT', split)
    cfg = ProblemConfig.standard(len(shape), shape, L=tuple(n * 4.0 / 1536 for n in shape), nlig=nlig)
    u, v = _state(cfg, nlig)
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
        print('ring of one, rccl, %s: operator rel_l2 %.3e, state rel_l2 %.3e, pc_used %d / %d, iterations %d / %d' %
              (shape, e_op, e_st, st.pc_used, st1.pc_used, st.linear_its, st1.linear_its))
        assert e_op < 1e-5                                        # fp32 transforms, different summation order
        assert st.pc_used & 8 and st1.pc_used & 8
        assert e_st < 1e-9
        assert st.linear_its <= st1.linear_its + 4
    finally:
        ks.close()
        one.close()


def test_one_rank_3d_three_times_power_of_two_box_vs_numpy():
    """the one-rank path of the same box shapes (plain handle, no transport; z column = one piece of 96 elements) against numpy.fft.fftn
    and the closed-form block inverse, at the bound of test_spectral_operator_3d_vs_numpy"""
    from ksfd_amd import lib as klib
    from test_gpu_spectral import GAMMA, _numpy_spectral3d
    shape = (48, 32, 96)
    cfg = ProblemConfig.standard(3, shape, L=tuple(n * 4.0 / 1536 for n in shape), nlig=1)
    u, v = _state(cfg, 1)
    k = klib.KSFDHip(cfg)
    try:
        k.set_state(u)
        for h in (0.02, 5.0):
            shift = 1.0 / (GAMMA * h)
            e = rel_l2(k.spectral_apply(shift, v), _numpy_spectral3d(cfg, u, shift, v))
            print('one rank %s, h %g: operator rel_l2 against numpy %.3e' % (shape, h, e))
            assert e < 2e-5                                       # fp32 FFTs and symbol; it is a preconditioner
    finally:
        k.close()


def _ineligible_worker3d(rank, size, port, shape, outfile):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        from ksfd_amd import lib as klib
        from ksfd_amd.dist import open_handle, local_slab, gather_slabs, spectral_selftest
        cfg = ProblemConfig.standard(3, shape, L=tuple(n * 4.0 / 1536 for n in shape), nlig=1)
        u, v = _state(cfg, 1)
        ks, keep = open_handle(cfg, rank, size, 0, transport='host')
        mine = lambda a: local_slab(a, cfg, rank, size)
        assert spectral_selftest(ks, cfg, rank, size)             # nothing to check: True
        ks.set_state(mine(u))
        code, msg = -1, ''
        try:
            ks.spectral_apply(3.0, mine(v))
        except klib.KSFDError as e:
            code, msg = e.code, str(e)
        found = [None] * size
        dist.all_gather_object(found, (code, msg))
        opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-11)          # pc_type 2, the default
        t, h, st, rc = ks.step(0.0, 0.3, opts)
        state = gather_slabs(ks.get_state(), cfg)
        ks.close()
        if rank == 0:
            one = klib.KSFDHip(cfg)
            one.set_state(u)
            one.step(0.0, 0.3, opts)
            np.savez(outfile, codes=np.array([f[0] for f in found]), msgs=np.array([f[1] for f in found]), einval=np.array(klib.EINVAL),
                     pc=np.array(st.pc_used), got=state, ref=one.get_state())
            one.close()
    finally:
        dist.destroy_process_group()


def test_three_ranks_keep_the_other_solvers(tmp_path):
    """(48, 32, 48) on three ranks: 16 planes each, so the handle opens, but rank counts other than 1, 2, 4, 8 stay without the solver:
    KSFD_EINVAL from spectral_apply on every rank, with a message that names the rule as it now is; the default pc_type 2 step goes
    through the other solvers and matches one rank."""
    outfile = str(tmp_path / 'result.npz')
    mp.spawn(_ineligible_worker3d, args=(3, _free_port(), (48, 32, 48), outfile), nprocs=3, join=True)
    z = np.load(outfile)
    assert list(z['codes']) == [int(z['einval'])] * 3
    for m in z['msgs']:
        m = str(m)
        assert 'power-of-two' not in m and 'power of two' not in m
        assert '3*2^k' in m and '1, 2, 4 or 8' in m
    assert not int(z['pc']) & 8
    assert rel_l2(z['got'], z['ref']) < 1e-9
