"""Functional rehearsal of the slab-distributed spectral solver on a 3 * 2^k grid: the options84 problem (attractant + repellent, 3
fields, spacing 4/1536, atol 0.01, rtol 1e-6) at 384^2, adaptive steps from dt = 1e-8 with pc_type 4, on N ranks SHARING one GPU
through the host transport, against the same steps on one rank.  Prints, per step, accept/reject, (t, h) and the number of spectral
applications on both sides, then the differences.  Not a performance statement: every transpose crosses PCIe twice here.
The stage systems are solved to ksp_rtol 1e-11 on both sides (which sweep crosses a looser tolerance depends on the summation order).
usage: python tools/slab_rehearsal.py [--ranks 2] [--grid 384] [--steps 20]"""
import argparse
import os
import socket
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problem(grid):
    from ksfd_amd.config import ProblemConfig
    cfg = ProblemConfig.standard(2, (grid, grid), L=(grid * 4.0 / 1536,) * 2, nlig=2)
    rng = np.random.default_rng(84)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)                  # srho0 = 90
    u = np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(cfg.nlig)])
    return cfg, u


def walk(ks, nsteps):
    from ksfd_amd import lib as klib
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, ksp_rtol=1e-11, pc_type=4)
    t, h, log = 0.0, 1e-8, []
    for _ in range(nsteps):
        t, h, st, rc = ks.step(t, h, opts)
        assert rc == 0, ks.last_error()
        log.append((int(st.accepted), int(st.rejections), t, h, int(st.linear_its), int(st.pc_used)))
    return log


def worker(rank, size, port, grid, nsteps, outfile):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        from ksfd_amd.dist import open_handle, local_slab, gather_slabs
        cfg, u = problem(grid)
        ks, keep = open_handle(cfg, rank, size, 0, transport='host')
        ks.set_state(local_slab(u, cfg, rank, size))
        log = walk(ks, nsteps)
        state = gather_slabs(ks.get_state(), cfg)
        ks.close()
        if rank == 0:
            np.savez(outfile, log=np.array(log, dtype=np.float64), state=state)
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ranks', type=int, default=2)
    ap.add_argument('--grid', type=int, default=384)
    ap.add_argument('--steps', type=int, default=20)
    a = ap.parse_args()
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    with tempfile.TemporaryDirectory() as d:
        outfile = os.path.join(d, 'slabs.npz')
        mp.spawn(worker, args=(a.ranks, port, a.grid, a.steps, outfile), nprocs=a.ranks, join=True)
        z = np.load(outfile)
        slog, sstate = z['log'], z['state']
    from ksfd_amd import lib as klib
    cfg, u = problem(a.grid)
    one = klib.KSFDHip(cfg)
    one.set_state(u)
    olog = np.array(walk(one, a.steps), dtype=np.float64)
    ostate = one.get_state()
    one.close()
    print('%d^2 x %d fields, %d adaptive steps from dt = 1e-8, pc_type 4, ksp_rtol 1e-11: %d slab ranks on one GPU (host transport) | one rank' % (a.grid, cfg.F, a.steps, a.ranks))
    print('step  acc rej  t                       h                       spectral applications (pc_used) | the same on one rank')
    for i, (p, q) in enumerate(zip(slog, olog)):
        print('%4d  %3d %3d  %.15e  %.15e  %3d (%d) | %3d %3d  %.15e  %.15e  %3d (%d)' %
              (i + 1, p[0], p[1], p[2], p[3], p[4], p[5], q[0], q[1], q[2], q[3], q[4], q[5]))
    same = bool(np.array_equal(slog[:, :2], olog[:, :2]))
    dth = float(np.max(np.abs(slog[:, 2:4] - olog[:, 2:4]) / np.abs(olog[:, 2:4])))
    F = cfg.F
    dfield = [float(np.linalg.norm(x - y) / np.linalg.norm(y)) for x, y in zip(sstate.reshape(F, -1), ostate.reshape(F, -1))]
    allspec = bool(np.all(slog[:, 5].astype(int) & 8) and np.all(olog[:, 5].astype(int) & 8))
    print('accept/reject sequence equal: %s; max relative difference of (t, h): %.3e; rel-L2 per field: %s; spectral solver in every step on both sides: %s'
          % (same, dth, ' '.join('%.3e' % e for e in dfield), allspec))
    ok = same and dth <= 1e-8 and max(dfield) <= 1e-8 and allspec
    print('REHEARSAL %s' % ('OK' if ok else 'FAILED'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
