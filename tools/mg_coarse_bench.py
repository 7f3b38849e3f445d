"""Device time of the exact coarse solve of the multigrid V cycle (ksfd_set_mg_coarse kind 1; csrc/lu.hip.h: k_lu_panel, k_lu_invert,
k_mgc_gemv): one set-up (assembly, factorization with one launch per panel, inversion, the host wait for the pivot flag), one apply, and
the two-launches-per-column factorization of pc_type 5 on the same matrix for comparison.

    python tools/mg_coarse_bench.py [--batches 7] [--reps 10]

HIP events on the compute stream around `reps` repetitions after three warm-up ones (ksfd_bench_kernel); printed: the median of the
batches and their spread.  Grids are chosen so that the level the cycle ends on has n = 128, 432, 1024 and 2048 unknowns."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from ksfd_amd import lib as klib
from ksfd_amd.config import ProblemConfig

#        n: (fine grid, ligands, max_unknowns)     level the cycle ends on
CASES = {128: ((32, 32), 1, 0),                  # 8 x 8 x 2
         432: ((48, 48), 2, 0),                  # 12 x 12 x 3
         1024: ((64, 64), 3, 1024),              # 16 x 16 x 4, cut above the coarsest level
         2048: ((128, 128), 1, 2048)}            # 32 x 32 x 2, cut above the coarsest level


def _cfg(shape, nlig):
    L = tuple(0.0025 * n for n in shape)
    if nlig <= 2:
        return ProblemConfig.standard(2, shape, L=L, nlig=nlig)
    return ProblemConfig(dim=2, n=shape, L=L, lig_group=[0, 1, 0], lig_w=[1.0, 1.0, 0.5], lig_s=[0.01, 0.001, 0.003], lig_gamma=[0.01, 0.001, 0.004],
                         lig_D=[1e-6, 1e-5, 3e-6], grp_alpha=[1500.0, 1500.0], grp_beta=[5.56e-4, -5.56e-4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    print('n      set-up ms (min..max)        apply us (min..max)        per-column factorization ms (min..max)   launches: panels / columns')
    for n, (shape, nlig, maxu) in CASES.items():
        cfg = _cfg(shape, nlig)
        rng = np.random.default_rng(0)
        rho = 9000.0 * (1.0 + 0.01 * rng.standard_normal(cfg.N))
        k = klib.KSFDHip(cfg)
        k.set_state(np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(nlig)]))
        k.set_mg_coarse(1, maxu)
        info = k.mg_coarse_info()
        assert info['unknowns'] == n, info
        med = {}
        for name, cls, reps in (('setup', klib.BENCH_MGC_SETUP, a.reps), ('apply', klib.BENCH_MGC_APPLY, 20 * a.reps),
                                ('columns', klib.BENCH_MGC_FACTOR_COLUMNS, max(1, a.reps // 5))):
            ms = sorted(k.bench_kernel(cls, reps)[0] for _ in range(a.batches))
            med[name] = (ms[len(ms) // 2], ms[0], ms[-1])
        panels = (n + 63) // 64
        print('%-6d %7.3f (%.3f..%.3f)   %8.1f (%.1f..%.1f)   %8.3f (%.3f..%.3f)   %d / %d' %
              ((n,) + med['setup'] + tuple(1e3 * x for x in med['apply']) + med['columns'] + (4 * panels + 4, 2 * n + 3 * panels + 3)), flush=True)
        k.close()


if __name__ == '__main__':
    main()
