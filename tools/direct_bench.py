"""Timing of the dense direct stage solver (pc_type 5, csrc/lu.hip.h).

    python tools/direct_bench.py                       # wall clock of ksfd_direct_apply per size + one pc_type 5 step at 128^2 x 2
    python tools/direct_bench.py --breakdown STATS.csv --n N
        # per-phase device time from `rocprofv3 --kernel-trace --stats` of `python tools/direct_bench.py --sizes N --reps 0 --no-step`
        # (one assembly + factorization + solve): assembly, panel factorization, interchanges, U12 solve, trailing update, solves

Rates: factorization 2/3 n^3 flop (fp64 GF/s), one solve 8 n^2 bytes of factors read (GB/s).  Sizes are F*N unknowns of 2-D grids
with 2 fields: 32x16 (1024), 64x32 (4096), 128x64 (16384), 128x128 (32768 = KSFD_DIRECT_MAX).
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = {1024: (32, 16), 4096: (64, 32), 16384: (128, 64), 32768: (128, 128)}
GAMMA = 0.43586652150845900

PHASES = [('assembly', ('k_jac_csr', 'k_lu_scatter', 'fill', 'memset')), ('panel', ('k_lu_pivot', 'k_lu_panel_col')),
          ('laswp', ('k_lu_laswp',)), ('trsm', ('k_lu_trsm',)), ('trailing update (MFMA)', ('k_lu_gemm',)),
          ('solve', ('k_lu_fwd', 'k_lu_bwd'))]


def _handle(n):
    from ksfd_amd import lib as klib
    from ksfd_amd.config import ProblemConfig
    shape = GRIDS[n]
    cfg = ProblemConfig.standard(2, shape, L=(0.4 * shape[0] / 128, 0.4 * shape[1] / 128))
    rng = np.random.default_rng(0)
    rho = 9000.0 * (1.0 + 0.01 * rng.standard_normal(cfg.N))
    k = klib.KSFDHip(cfg)
    k.set_state(np.concatenate([rho, rho * cfg.lig_s[0] / cfg.lig_gamma[0]]))
    return k, cfg


def apply_times(sizes, reps):
    shift = 1.0 / (GAMMA * 0.05)
    for n in sizes:
        k, cfg = _handle(n)
        v = np.random.default_rng(1).standard_normal(k.nlocal)
        k.direct_apply(shift, v)                          # allocation of the factors, first-touch
        if reps < 1:
            k.close()
            continue
        ts = []
        for _ in range(reps):
            k.synchronize()
            t0 = time.perf_counter()
            k.direct_apply(shift, v)
            ts.append(time.perf_counter() - t0)
        t = min(ts)
        print('direct_apply n=%6d (%dx%d x 2 fields): %9.2f ms (assembly + factorization + one solve + host copies, min of %d); '
              '2/3 n^3 / t = %7.1f GF/s' % (n, cfg.n[0], cfg.n[1], 1e3 * t, reps, (2.0 / 3.0) * n ** 3 / t / 1e9), flush=True)
        k.close()


def step_time():
    from ksfd_amd import lib as klib
    k, cfg = _handle(32768)
    opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, pc_type=5)
    t, h = 0.0, 0.05
    k.step(t, h, opts)
    k.synchronize()
    t0 = time.perf_counter()
    t, hn, st, rc = k.step(t, h, opts)
    k.synchronize()
    dt = time.perf_counter() - t0
    print('pc_type 5 step 128x128 x 2 fields (32768 unknowns): %.1f ms, pc_used %d, linear_its %d, residual_evals %d, ksp_resid %.2e, '
          'launches %d' % (1e3 * dt, st.pc_used, st.linear_its, st.residual_evals, st.ksp_resid, st.launches), flush=True)
    k.close()


def breakdown(path, n):
    tot = {}
    calls = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row['Name']
            for ph, keys in PHASES:
                if any(key in name for key in keys):
                    tot[ph] = tot.get(ph, 0.0) + float(row['TotalDurationNs']) * 1e-6
                    calls[ph] = calls.get(ph, 0) + int(row['Calls'])
                    break
    fact = sum(tot.get(p, 0.0) for p in ('panel', 'laswp', 'trsm', 'trailing update (MFMA)'))
    print('device time, n = %d (rocprofv3 kernel trace, one assembly + factorization + solve):' % n)
    for ph, _ in PHASES:
        print('  %-24s %10.3f ms  %7d launches' % (ph, tot.get(ph, 0.0), calls.get(ph, 0)))
    if fact > 0:
        print('  factorization            %10.3f ms  -> %.1f GF/s fp64 (2/3 n^3)' % (fact, (2.0 / 3.0) * n ** 3 / (fact * 1e-3) / 1e9))
        g = tot.get('trailing update (MFMA)', 0.0)
        flop_g = 2.0 * sum((n - k1) ** 2 * 64 for k1 in range(64, n, 64))
        print('  trailing update          %10.3f ms  -> %.1f GF/s on its own %.3g flop (%.0f %% of the factorization time)'
              % (g, flop_g / (g * 1e-3) / 1e9 if g else 0.0, flop_g, 100.0 * g / fact))
    s = tot.get('solve', 0.0)
    if s > 0:
        print('  solve                    %10.3f ms  -> %.1f GB/s (8 n^2 B of factors)' % (s, 8.0 * n * n / (s * 1e-3) / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1024,4096,16384,32768')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--breakdown', default=None, help='kernel_stats.csv of rocprofv3 --stats')
    ap.add_argument('--n', type=int, default=32768)
    a = ap.parse_args()
    if a.breakdown:
        breakdown(a.breakdown, a.n)
        return
    apply_times([int(s) for s in a.sizes.split(',')], a.reps)
    if not a.no_step:
        step_time()


if __name__ == '__main__':
    main()
