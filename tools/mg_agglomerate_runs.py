"""Iteration counts and collectives of the multigrid-preconditioned stage solves on slab ranks, with and without coarse-level
agglomeration (ksfd_set_mg_agglomerate), against the single-rank handle.  Ranks share cuda:0 through the host transport, so NOTHING here
is a timing between devices: the columns are linear iterations, kernel launches and host waits per step, and the hierarchy each handle
runs (extents, rows per rank, replicated or not, Chebyshev sweeps on the last level).

    python tools/mg_agglomerate_runs.py [--ranks 4] [--max-points 1] > profiles/mg_agglomerate_runs.log

Cases: (64, 64) x 2 fields and (64, 64, 64) x 2 fields.  Steps: one fixed step h = 5 at ksp_rtol 1e-11 (the stiff step of
tests/test_gpu_dist.py), then three more at h = 5 and ksp_rtol 1e-7 (fp32 level vectors in 2-D)."""
import argparse
import os
import socket
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

GAMMA = 0.43586652150845900
CASES = [((64, 64), 1), ((64, 64, 64), 1)]
RTOLS = (1e-11, 1e-7, 1e-7, 1e-7)


def problem(shape, nlig):
    from ksfd_amd.config import ProblemConfig
    dim = len(shape)
    cfg = ProblemConfig.standard(dim, shape, L=tuple((0.01 if dim == 3 else 0.0025) * n for n in shape), nlig=nlig)
    rho = 9000.0 * (1.0 + 0.01 * np.random.default_rng(3).standard_normal(cfg.N))
    return cfg, np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(nlig)])


def hierarchy(k, size, dim):
    n = k.mg_level_info(0)['nlevels']
    out = []
    for l in range(n):
        i = k.mg_level_info(l, 1.0 / (GAMMA * 5.0))
        out.append('%s rows %d%s' % ('x'.join(str(x) for x in i['n'][:dim]), i['sloc'], ' sweeps %d' % i['coarse_sweeps'] if l == n - 1 else ''))
    return '; '.join(out)


def steps(k, klib, u):
    k.set_state(u)
    t, log = 0.0, []
    for rtol in RTOLS:
        # a solve that does not converge or leaves the finite numbers is reported (-1) and ends the sequence of that handle; every rank
        # sees the same residuals, so every rank ends it at the same step
        try:
            t, _, st, rc = k.step(t, 5.0, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=rtol, pc_type=1))
            log.append((st.linear_its, st.launches, st.host_syncs))
        except klib.KSFDError as e:
            if e.code not in (klib.ELINEAR, klib.ENAN):
                raise
            log += [(-1, -1, -1)] * (len(RTOLS) - len(log))
            break
    return log, k.get_state()


def worker(rank, size, port, maxp, outdir):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        from ksfd_amd import lib as klib
        from ksfd_amd.dist import open_handle, local_slab, gather_slabs
        lines = []
        for shape, nlig in CASES:
            cfg, u = problem(shape, nlig)
            dim = len(shape)
            ks, keep = open_handle(cfg, rank, size, 0, transport='host')
            mine = local_slab(u, cfg, rank, size)
            ks.set_state(mine)
            rows = {}
            for label, agg in (('slabs, off', 0), ('slabs, on', maxp)):
                ks.set_mg_agglomerate(agg)
                h = hierarchy(ks, size, dim)
                log, state = steps(ks, klib, mine)
                rows[label] = (h, log, gather_slabs(state, cfg))
            ks.close()
            if rank == 0:
                one = klib.KSFDHip(cfg)
                one.set_state(u)
                h = hierarchy(one, 1, dim)
                log, state = steps(one, klib, u)
                one.close()
                lines.append('%s x %d fields, %d ranks, max_points %d' % ('x'.join(str(x) for x in shape), cfg.F, size, maxp))
                lines.append('  %-12s levels: %s' % ('single rank', h))
                for label in rows:
                    lines.append('  %-12s levels: %s' % (label, rows[label][0]))
                lines.append('  step (h = 5): ksp_rtol | linear_its launches host_syncs: single rank | slabs, off | slabs, on')
                for q, rtol in enumerate(RTOLS):
                    lines.append('    %d  %.0e | %4d %6d %5d | %4d %6d %5d | %4d %6d %5d' % ((q, rtol) + log[q] + rows['slabs, off'][1][q] + rows['slabs, on'][1][q]))
                for label in rows:
                    d = np.linalg.norm(rows[label][2] - state) / np.linalg.norm(state)
                    lines.append('  %-12s rel-L2 distance of the final state from the single-rank one: %.3e' % (label, d))
        if rank == 0:
            with open(os.path.join(outdir, 'out.txt'), 'w') as f:
                f.write('\n'.join(lines) + '\n')
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ranks', type=int, default=4)
    ap.add_argument('--max-points', type=int, default=1)
    a = ap.parse_args()
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(worker, args=(a.ranks, port, a.max_points, d), nprocs=a.ranks, join=True)
        print('# tools/mg_agglomerate_runs.py: ranks share one device through the host transport; counts only, no timing between devices')
        sys.stdout.write(open(os.path.join(d, 'out.txt')).read())


if __name__ == '__main__':
    main()
