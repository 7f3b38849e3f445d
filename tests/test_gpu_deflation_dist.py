"""GPU, 2 slab ranks sharing cuda:0 through the host transport: GMRES with deflated restarting must reproduce the single-rank result.
The rotation is pointwise and the dots go through the existing all-reduce, but the solver takes many host-side decisions on reduced
scalars (restart plan accepted or not, least-squares breakdown, residual checks): every rank has to take the same ones, or the ranks
wait for each other in the next reduction."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import rel_l2
from ksfd_amd.config import ProblemConfig
from test_gpu_dist import _free_port

pytestmark = pytest.mark.gpu

SHAPE, H, KEEP, RESTART = (24, 20), 0.5, 4, 12


def _problem():
    cfg = ProblemConfig.standard(2, SHAPE, L=[0.2, 0.25], nlig=1)
    rng = np.random.default_rng(3)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)
    u = np.concatenate([rho, rho * cfg.lig_s[0] / cfg.lig_gamma[0] + rng.standard_normal(cfg.N)])
    return cfg, u


def _steps(ks, klib):
    """two fixed unpreconditioned steps with a short restart: the solves restart deflated, with and without the carry to later stages"""
    opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, pc_type=0, ksp_restart=RESTART, ksp_rtol=1e-11, ksp_max_it=5000)
    t, log = 0.0, []
    for carry in (0, 1):
        ks.set_deflation(KEEP, carry)
        t, hn, st, rc = ks.step(t, H, opts)
        ds = ks.deflation_stats()
        log.append((st.linear_its, ds['restarts'], ds['projections']))
    return np.array(log, dtype=np.float64)


def _worker(rank, size, port, outfile):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        from ksfd_amd import lib as klib
        from ksfd_amd.dist import open_handle, local_slab, gather_slabs
        cfg, u = _problem()
        ks, keepalive = open_handle(cfg, rank, size, 0, transport='host')
        ks.set_state(local_slab(u, cfg, rank, size))
        log = _steps(ks, klib)
        state = gather_slabs(ks.get_state(), cfg)
        ks.close()
        if rank == 0:
            one = klib.KSFDHip(cfg)
            one.set_state(u)
            log1 = _steps(one, klib)
            ref = one.get_state()
            one.close()
            np.savez(outfile, state=state, ref=ref, log=log, log1=log1)
    finally:
        dist.destroy_process_group()


def test_two_slab_ranks_match_single_rank_with_deflation(tmp_path):
    outfile = str(tmp_path / 'result.npz')       # results come back through a file: a queue would block on join
    mp.spawn(_worker, args=(2, _free_port(), outfile), nprocs=2, join=True)
    z = np.load(outfile)
    print('2 ranks (its, restarts, projections) per step %s; 1 rank %s; rel-L2 %.3e' % (z['log'].tolist(), z['log1'].tolist(), rel_l2(z['state'], z['ref'])))
    assert z['log'][:, 1].min() >= 1 and z['log1'][:, 1].min() >= 1          # deflated restarts in every step, on both handles
    assert z['log'][1, 2] >= 1                                               # the carried relation was used on the slabs
    assert rel_l2(z['state'], z['ref']) < 1e-8
