"""Timing of the banded direct stage solver for 1-D grids (pc_type 6, csrc/banded.hip.h) against the automatic choice (pc_type 2) and the
dense LU (pc_type 5).

    python tools/banded_bench.py                                  # this tree: every case, pc_type 2, 5 (where it fits) and 6
    python tools/banded_bench.py --parent-root DIR --rounds 2     # the same session alternating with a built checkout of the parent
                                                                  # commit in DIR (pc_type 2 and 5 there), round by round
    python tools/banded_bench.py --log profiles/banded_runs.log   # append the table to a log

Per case (grid, ligands, state, step size h) and solver: ms per step attempt -- wall clock between two device synchronisations around a
batch of fixed-size steps (adapt = 0: one attempt per step) from a checkpoint of the same state, median of the batches after a warm-up
step; a 1-D step is bound by launches and host hand-overs, which only the wall clock sees.  For pc_type 6 also ms per factorization
(assembly and the read-back of info included) and per solve from HIP events on the compute stream (ksfd_bench_kernel), and from them
the cost per column.  A solver that fails a case (GMRES out of iterations at h = 50, say) is reported as such with its message.

Cases: N = 256, 384, 512, 4096, 16384 with one and two ligands; a near-uniform state (rho = 9000 (1 + 0.01 noise)) and a strongly
varying one (rho over two decades); h = 0.1 and h = 50.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (256, 384, 512, 4096, 16384)
NLIGS = (1, 2)
STATES = ('uniform', 'varying')
STEPS = (0.1, 50.0)
DIRECT_MAX = 32768


def make_state(cfg, kind):
    rng = np.random.default_rng(3)
    if kind == 'uniform':
        rho = 9000.0 * (1.0 + 0.01 * rng.standard_normal(cfg.N))
        return np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(cfg.nlig)])
    x = np.arange(cfg.N) / cfg.N
    rho = 1900.0 * 10 ** (1.15 * np.sin(2 * np.pi * (2 * x + 0.3)) + 0.005 * rng.standard_normal(cfg.N))
    return np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] * (1 + 0.05 * rng.standard_normal(cfg.N)) for l in range(cfg.nlig)])


def time_steps(k, klib, pc, h, batches, per_batch):
    opts = klib.default_step_opts(pc_type=pc, adapt=0, atol=0.01, rtol=1e-6)
    k.restore()
    t, hn, st, rc = k.step(0.0, h, opts, raise_on_error=False)          # warm-up: allocations, first-touch, set-ups
    if rc:
        return dict(failed=k.last_error()[:120])
    ts = []
    for _ in range(batches):
        k.restore()
        k.synchronize()
        t0 = time.perf_counter()
        t = 0.0
        for _ in range(per_batch):
            t, hn, st, rc = k.step(t, h, opts, raise_on_error=False)
            if rc:
                return dict(failed=k.last_error()[:120])
        k.synchronize()
        ts.append((time.perf_counter() - t0) / per_batch)
    return dict(ms=1e3 * statistics.median(ts), its=st.linear_its, launches=st.launches, pc_used=st.pc_used)


def child(a):
    """every case with the library of the tree in a.root; one JSON line per (case, solver)"""
    sys.path.insert(0, a.root)
    from ksfd_amd import lib as klib
    from ksfd_amd.config import ProblemConfig
    pcs = [int(p) for p in a.pcs.split(',')]
    gamma = 0.43586652150845900
    for N in [int(x) for x in a.grids.split(',')]:
        for nlig in NLIGS:
            cfg = ProblemConfig.standard(1, (N,), L=(0.4 * N / 256,), nlig=nlig)
            n = cfg.F * N
            for kind in STATES:
                k = klib.KSFDHip(cfg)
                k.set_state(make_state(cfg, kind))
                k.checkpoint()
                for h in STEPS:
                    for pc in pcs:
                        if pc == 5 and n > a.direct_max:
                            continue
                        big = n > 4096
                        r = time_steps(k, klib, pc, h, a.batches, 1 if (big and pc == 5) else a.per_batch)
                        if pc == 6 and 'ms' in r:
                            k.restore()
                            k.banded_apply(1.0 / (gamma * h), np.ones(k.nlocal))
                            r['factor_ms'] = statistics.median(k.bench_kernel(klib.BENCH_BAND_FACTOR, 5)[0] for _ in range(a.batches))
                            r['solve_ms'] = statistics.median(k.bench_kernel(klib.BENCH_BAND_SOLVE, 20)[0] for _ in range(a.batches))
                        r.update(N=N, nlig=nlig, state=kind, h=h, pc=pc, tree=a.tag)
                        print('BANDED_BENCH ' + json.dumps(r), flush=True)
                k.close()


def run_child(root, tag, pcs, a):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--root', root, '--tag', tag, '--pcs', pcs, '--grids', a.grids,
           '--batches', str(a.batches), '--per-batch', str(a.per_batch), '--direct-max', str(a.direct_max)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    rows = [json.loads(line[len('BANDED_BENCH '):]) for line in out.stdout.splitlines() if line.startswith('BANDED_BENCH ')]
    if out.returncode:
        raise SystemExit('child (%s) ended with %d after %d rows:\n%s' % (tag, out.returncode, len(rows), out.stderr[-2000:]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--tag', default='this')
    ap.add_argument('--pcs', default='2,5,6')
    ap.add_argument('--grids', default=','.join(str(g) for g in GRIDS))
    ap.add_argument('--batches', type=int, default=5)
    ap.add_argument('--per-batch', type=int, default=3)
    ap.add_argument('--direct-max', type=int, default=DIRECT_MAX, help='largest F*N pc_type 5 is timed at')
    ap.add_argument('--parent-root', default=None, help='built checkout of the parent commit (its pc_type 2 and 5 run alternating with this tree)')
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--child-timeout', type=int, default=900)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    rows = []
    for _ in range(a.rounds):
        rows += run_child(HERE, 'this', a.pcs, a)
        if a.parent_root:
            rows += run_child(a.parent_root, 'parent', '2,5', a)
    # best round per (case, tree, solver): the rounds alternate, so both trees see the same drift
    best = {}
    for r in rows:
        key = (r['N'], r['nlig'], r['state'], r['h'], r['tree'], r['pc'])
        if key not in best or ('ms' in r and r['ms'] < best[key].get('ms', float('inf'))):
            best[key] = r
    lines = ['# ms per step attempt (wall clock, median of %d batches, best of %d alternating rounds); pc_type 6 also ms per factorization / per solve'
             % (a.batches, a.rounds),
             '# (HIP events) and ns per column (unknown) of each',
             '%6s %4s %8s %5s | %10s %10s %10s | %10s %10s | %9s %9s %8s %8s' % ('N', 'nlig', 'state', 'h', 'pc2', 'pc5', 'pc6', 'parent pc2', 'parent pc5',
                                                                                 'factor ms', 'solve ms', 'ns/col f', 'ns/col s')]

    def cell(key):
        r = best.get(key)
        if r is None:
            return '-'
        return '%.3f' % r['ms'] if 'ms' in r else 'failed'
    fails = []
    for N in [int(x) for x in a.grids.split(',')]:
        for nlig in NLIGS:
            for kind in STATES:
                for h in STEPS:
                    c = (N, nlig, kind, h)
                    b6 = best.get(c + ('this', 6), {})
                    n = (nlig + 1) * N
                    lines.append('%6d %4d %8s %5g | %10s %10s %10s | %10s %10s | %9s %9s %8s %8s' % (
                        N, nlig, kind, h, cell(c + ('this', 2)), cell(c + ('this', 5)), cell(c + ('this', 6)), cell(c + ('parent', 2)), cell(c + ('parent', 5)),
                        '%.3f' % b6['factor_ms'] if 'factor_ms' in b6 else '-', '%.3f' % b6['solve_ms'] if 'solve_ms' in b6 else '-',
                        '%.0f' % (1e6 * b6['factor_ms'] / n) if 'factor_ms' in b6 else '-', '%.0f' % (1e6 * b6['solve_ms'] / n) if 'solve_ms' in b6 else '-'))
                    for tree in ('this', 'parent'):
                        for pc in (2, 5, 6):
                            r = best.get(c + (tree, pc))
                            if r and 'failed' in r:
                                fails.append('# failed: N %d nlig %d %s h %g %s pc_type %d: %s' % (N, nlig, kind, h, tree, pc, r['failed']))
                            elif r and pc == 2:
                                lines[-1] += '   [%s pc2: %d its, %d launches, pc_used %d]' % (tree, r['its'], r['launches'], r['pc_used'])
    text = '\n'.join(lines + fails)
    print(text)
    if a.log:
        with open(a.log, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
