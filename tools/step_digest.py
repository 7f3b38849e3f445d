"""Step-by-step digest of the stage solvers of one libksfd_hip.so that tools/spec_digest.py does not reach: one line per step.

    python tools/step_digest.py path/to/libksfd_hip.so > digest.txt

Two builds whose host side takes the same decisions print the same file; run it once per library (one library per process) and diff.
Cases, 3-4 steps each on 64x64 (seeded states, spacing of tests/test_gpu_spectral.py unless said):
  poly       pc_type 3 at h = 0.05 (X ~ 10): Chebyshev polynomial, its eigenvalue estimate refreshed by its own schedule
  mg-guess   pc_type 1 at h = 10: V cycle, stages 2-4 from the guess built on the earlier ones (correction solves, recycling)
  aggregate  pc_type 2 at h = 2 on a state with two planted aggregates: slow sweeps, hand-over to GMRES, fallback, back-off
  restart8   pc_type 0, ksp_restart 8, h = 0.5 on the spacing 0.2 / 64 (40+ iterations per stage): cycles of 8, 16, 32, ...
  nogrowth   the same with restart growth off (TUNE_NO_RESTART_GROWTH)
  pipelined  the same with the pipelined solver (TUNE_ASYNC_GMRES) and ksp_restart 64: cycles of 32
  bit<b>     every bit b of the tuning word alone on top of bit 0 (the field of bits 6-8 with the values 1 and 4), two steps of the case
             the bit acts in: mg-guess, the spectral solver at ksp_rtol 1e-6 (pc_type 2 at h = 2 on the smooth state), restart8, poly, or
             plain GMRES at h = 0.05 (the recycling bits 4, 5, 6-8 in restart8 and in poly).  Written as 1 << b, the frozen encoding itself, so
             that the group checks the numbers and not the names: it runs against any libksfd_hip.so whose tuning word has this encoding"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ksfd_amd import lib as klib                     # noqa: E402
from ksfd_amd.config import ProblemConfig            # noqa: E402

N = 64
FIELDS = ('linear_its', 'pc_used', 'rejections', 'residual_evals', 'predicted_final', 'launches', 'host_syncs')


def smooth(cfg, seed):
    rng = np.random.default_rng(seed)
    rho = 9000.0 + 90.0 * rng.standard_normal(cfg.N)
    return np.concatenate([rho, rho * cfg.lig_s[0] / cfg.lig_gamma[0] * (1 + 0.01 * rng.standard_normal(cfg.N))])


def aggregated(cfg, seed):
    """the state of test_automatic_choice_leaves_the_spectral_preconditioner_when_coefficients_vary"""
    rng = np.random.default_rng(seed)
    x = np.arange(N)
    bump = np.exp(-((x[None, :] - 20.0) ** 2 + (x[:, None] - 40.0) ** 2) / 30.0) + np.exp(-((x[None, :] - 50.0) ** 2 + (x[:, None] - 12.0) ** 2) / 20.0)
    rho = (800.0 + 24000.0 * bump).reshape(-1) * (1 + 0.01 * rng.standard_normal(cfg.N))
    return np.concatenate([rho, rho * 1.0])


def run(name, width, state, h0, nsteps, tuning=1, **opts):
    cfg = ProblemConfig.standard(2, (N, N), L=(width, width), nlig=1)
    k = klib.KSFDHip(cfg)
    k.set_tuning(use_fused=tuning)
    k.set_state(state(cfg, 7))
    o = klib.default_step_opts(atol=0.01, rtol=1e-6, **opts)
    t, h = 0.0, h0
    for step in range(nsteps):
        t, h, st, rc = k.step(t, h, o, raise_on_error=False)
        sha = hashlib.sha256(np.ascontiguousarray(k.get_state(), dtype=np.float64).tobytes()).hexdigest()
        print('%s step %d rc %d t %r h %r %s state %s' % (name, step, rc, t, h, ' '.join('%s %d' % (f, getattr(st, f)) for f in FIELDS), sha))
        if rc:
            print('%s error %s' % (name, k.last_error()))
            break
    k.close()


def main():
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    klib.LIB_PATH = os.path.abspath(sys.argv[1])     # before the first handle loads the library
    spec, stiff = N * 4.0 / 1536, 0.2
    run('poly', spec, smooth, 0.05, 4, adapt=0, pc_type=3)
    run('mg-guess', spec, smooth, 10.0, 3, adapt=0, pc_type=1)
    run('aggregate', spec, aggregated, 2.0, 3, adapt=0, pc_type=2, ksp_rtol=1e-11)
    long_opts = dict(adapt=0, pc_type=0, ksp_rtol=1e-10, ksp_max_it=4000)
    run('restart8', stiff, smooth, 0.5, 3, ksp_restart=8, **long_opts)
    run('nogrowth', stiff, smooth, 0.5, 3, tuning=klib.TUNE_FUSED | klib.TUNE_NO_RESTART_GROWTH, ksp_restart=8, **long_opts)
    run('pipelined', stiff, smooth, 0.5, 3, tuning=klib.TUNE_FUSED | klib.TUNE_ASYNC_GMRES, ksp_restart=64, **long_opts)
    for b in range(24):
        if b in (7, 8):                                  # bits 6-8 are one field: the values 1 and 4 stand for it
            continue
        for word, name in ((1 << 6, 'bit6-8=1'), (4 << 6, 'bit6-8=4')) if b == 6 else ((1 << b, 'bit%d' % b),):
            if b in (12, 18, 19, 20):
                run(name, spec, smooth, 10.0, 2, tuning=1 | word, adapt=0, pc_type=1)
            elif b in (14, 16, 21):
                run(name, spec, smooth, 2.0, 2, tuning=1 | word, adapt=0, pc_type=2, ksp_rtol=1e-6)
            elif b in (3, 4, 5, 6, 17):
                run(name, stiff, smooth, 0.5, 2, tuning=1 | word, ksp_restart=8, **long_opts)
                if b in (4, 5, 6):                       # restart8 prints the same lines with and without these bits: poly is where they show
                    run(name + ' poly', spec, smooth, 0.05, 2, tuning=1 | word, adapt=0, pc_type=3)
            elif b == 9:
                run(name, spec, smooth, 0.05, 2, tuning=1 | word, adapt=0, pc_type=3)
            else:
                run(name, stiff, smooth, 0.05, 2, tuning=1 | word, adapt=0, pc_type=0, ksp_rtol=1e-10)


if __name__ == '__main__':
    main()
