"""Bitwise digest of the multigrid V cycle of one libksfd_hip.so: one line per item with the SHA-256 of the output bytes.

    python tools/mg_cycle_digest.py path/to/libksfd_hip.so > digest.txt

Two builds that make the same launches with the same arguments in the same order print the same file; run it once per library (one
library per process) and diff.  Items, all on seeded inputs at the state of tests/test_gpu_mg_parts.py:
  cycle    MGP_CYCLE variants 0 (fp64 level vectors) and 1 (fp32), captured and eager, Chebyshev and exact coarse solve, on 32x32
           (1 ligand) and 64x48 (2 ligands): three levels, an fp32 -> fp64 border inside the cycle; variant 0 on 16x16x16 and 96
  smooth   MGP_SMOOTH nu = 2 (zero guess, nonzero guess) and nu = 3 on levels 0 and 1 of 32x32
  operator MGP_OPERATOR variants 2 and 32 on level 1 of 64x48
  steps    the state after 3 multigrid-preconditioned steps on 64x64 at ksp_rtol 1e-5 (fp32 cycle) and 1e-11 (fp64 cycle), and with each
           the launches, bytes and algorithmic bytes of every kernel class (ksfd_get_profile)
  transfer MGP_RESTRICT (variants 0, 1, 2) and MGP_PROLONG_ADD (0, 1) on every level of 32x32, 64x48, 16x16x16 and 96, in every variant the
           level admits; the same on a ring of one rank (host transport) with set_mg_agglomerate(300) on 64x64 and (5000) on 32x32x32:
           the transfers across the border to the replicated levels in one process (rank offset 0; the offsets of further ranks need
           more than one rank: tests/test_gpu_mg_agglomerate.py::test_transfers)"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ksfd_amd import lib as klib                     # noqa: E402
from ksfd_amd.config import ProblemConfig            # noqa: E402

GAMMA = 0.43586652150845900
S_CYCLE = 1.0 / (GAMMA * 5.0)                        # a stiff step, the shift of the CYCLE tests


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def handle(shape, nlig, ring=False):
    cfg = ProblemConfig.standard(len(shape), shape, L=tuple((0.01 if len(shape) == 3 else 0.0025) * n for n in shape), nlig=nlig)
    rho = 9000.0 * (1.0 + 0.05 * np.random.default_rng(3).standard_normal(cfg.N))
    if ring:
        from ksfd_amd.dist import open_self_ring
        k, k.keep = open_self_ring(cfg, 0, 'host')
    else:
        k = klib.KSFDHip(cfg)
    k.set_state(np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(cfg.nlig)]))
    return cfg, k


def vec(k, level, seed):
    inf = k.mg_level_info(level)
    return np.random.default_rng(seed).standard_normal((inf['F'], inf['points']))


def cycles(name, shape, nlig, variants, coarse_kinds):
    cfg, k = handle(shape, nlig)
    b = vec(k, 0, 121)
    for kind in coarse_kinds:
        k.set_mg_coarse(kind)
        for variant in variants:
            for eager in (False, True):
                k.set_mg_params(power_its=klib.MG_EAGER if eager else 0)
                x = k.mg_part(klib.MGP_CYCLE, 0, b, variant=variant, shift=S_CYCLE)
                print('cycle %s coarse %s variant %d %s %s' % (name, 'lu' if kind else 'cheb', variant, 'eager' if eager else 'graph', sha(x)))
    k.close()


def smoother_and_operator():
    cfg, k = handle((32, 32), 1)
    for level in (0, 1):
        b, x0 = vec(k, level, 7 + level), vec(k, level, 17 + level)
        for nu, guess in ((2, None), (2, x0), (3, None)):
            x = k.mg_part(klib.MGP_SMOOTH, level, b, guess, nu=nu, shift=S_CYCLE, ratio=6.0)
            print('smooth 32x32 level %d nu %d %s %s' % (level, nu, 'zero' if guess is None else 'guess', sha(x)))
    k.close()
    cfg, k = handle((64, 48), 2)
    v, y = vec(k, 1, 31), vec(k, 1, 32)
    for variant in (2, 32):
        print('operator 64x48 level 1 variant %d %s' % (variant, sha(k.mg_part(klib.MGP_OPERATOR, 1, v, y, variant=variant, shift=S_CYCLE))))
    k.close()


def steps(ksp_rtol):
    cfg, k = handle((64, 64), 1)
    k.set_profiling(True)
    k.profile(reset=True)
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, ksp_rtol=ksp_rtol, pc_type=1)
    t, h, its = 0.0, 5.0, 0
    for _ in range(3):
        t, h, st, rc = k.step(t, h, opts)
        its += st.linear_its
    print('steps 64x64 ksp_rtol %g t %s h %s its %d state %s' % (ksp_rtol, float(t).hex(), float(h).hex(), its, sha(k.get_state())))
    for cls, p in sorted(k.profile().items()):
        print('steps 64x64 ksp_rtol %g class %s launches %d bytes %r alg_bytes %r' % (ksp_rtol, cls, p['launches'], float(p['bytes']), float(p['alg_bytes'])))
    k.close()


def transfers(name, shape, nlig, agglomerate=0):
    cfg, k = handle(shape, nlig, ring=agglomerate > 0)
    if agglomerate:
        k.set_mg_agglomerate(agglomerate)
    info = [k.mg_level_info(l) for l in range(k.mg_level_info(0)['nlevels'])]
    for l, (fine, coarse) in enumerate(zip(info, info[1:])):
        v, w = vec(k, l, 51 + l), vec(k, l + 1, 61 + l)
        for variant in [0] + [1] * fine['f32'] + [2] * (len(shape) == 2 and coarse['f32']):
            print('transfer %s level %d restrict variant %d %s' % (name, l, variant, sha(k.mg_part(klib.MGP_RESTRICT, l, v, variant=variant))))
        for variant in [0] + [1] * fine['f32']:
            print('transfer %s level %d prolong variant %d %s' % (name, l, variant, sha(k.mg_part(klib.MGP_PROLONG_ADD, l, v, w, variant=variant))))
    k.close()


def main():
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    klib.LIB_PATH = os.path.abspath(sys.argv[1])     # before the first handle loads the library
    for name, shape, nlig in (('32x32', (32, 32), 1), ('64x48', (64, 48), 2)):
        cycles(name, shape, nlig, (0, 1), (0, 1))
    cycles('16x16x16', (16, 16, 16), 1, (0,), (0,))
    cycles('96', (96,), 1, (0,), (0,))
    smoother_and_operator()
    for ksp_rtol in (1e-5, 1e-11):
        steps(ksp_rtol)
    for name, shape, nlig in (('32x32', (32, 32), 1), ('64x48', (64, 48), 2), ('16x16x16', (16, 16, 16), 1), ('96', (96,), 1)):
        transfers(name, shape, nlig)
    transfers('64x64 ring of one, agglomerate 300', (64, 64), 1, 300)
    transfers('32x32x32 ring of one, agglomerate 5000', (32, 32, 32), 1, 5000)


if __name__ == '__main__':
    main()
