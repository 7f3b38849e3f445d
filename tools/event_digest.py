"""Step-by-step digest of one libksfd_hip.so with the entries that end derived data interleaved between the steps: one line per step.

    python tools/event_digest.py path/to/libksfd_hip.so > digest.txt

Two builds that end the same products at the same events (csrc/handle_state.h) take the same decisions, make the same launches and print
the same file; run it once per library (one library per process) and diff.  Cases, all on 64x64 with the states of tools/step_digest.py:
  mg         pc_type 1 at h = 10 on the smooth state
  auto       pc_type 2 at h = 2, ksp_rtol 1e-11, on the state with two planted aggregates, set again before every third step (the fourth
             step from it at this h is no longer finite)
  poly       pc_type 3 at h = 0.05 on the smooth state
Each case takes one step after each of: nothing, set_mg_params (nu 3, and back), the mg_fuse tuning bit (cleared, and back),
set_mg_coarse (1, 600) and back, set_mg_tail (1024) and off, update_params (s2 * 1.1), scale_rho (0.9), a checkpoint save; then one step
further on and one after the restore; then one each after an mg_part cycle, a krylov_op multi-dot, a spectral_apply, and an
mg_coarse_apply op 1 (under set_mg_coarse(1), and one more after the way back).
  ring       a ring of one rank over the host transport: a pc_type 1 step, set_mg_agglomerate(300), another step, (0), another"""
import dataclasses
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from ksfd_amd import lib as klib                     # noqa: E402
from ksfd_amd.config import ProblemConfig            # noqa: E402
from step_digest import FIELDS, N, aggregated, smooth            # noqa: E402

GAMMA = 0.43586652150845900


def events(k, cfg, tuning):
    """(label, what to do before the step) in order"""
    rng = np.random.default_rng(5)
    v = rng.standard_normal(k.nlocal)

    def coarse_solve():
        k.set_mg_coarse(1, 600)
        k.mg_coarse_apply(1.0 / (GAMMA * 5.0), rng.standard_normal(k.mg_coarse_info()['unknowns']), op=1)
    return [
        ('first', lambda: None),
        ('mg_params nu 3', lambda: k.set_mg_params(nu=3)), ('mg_params nu 2', lambda: k.set_mg_params(nu=2)),
        ('mg_fuse off', lambda: k.set_tuning(use_fused=tuning | klib.TUNE_UNFUSED_SMOOTHER)), ('mg_fuse on', lambda: k.set_tuning(use_fused=tuning)),
        ('mg_coarse 1', lambda: k.set_mg_coarse(1, 600)), ('mg_coarse 0', lambda: k.set_mg_coarse(0)),
        ('mg_tail 1024', lambda: k.set_mg_tail(1024)), ('mg_tail 0', lambda: k.set_mg_tail(0)),
        ('update_params', lambda: k.update_params(dataclasses.replace(cfg, s2=1.1 * cfg.s2))),
        ('scale_rho', lambda: k.scale_rho(0.9)),
        ('checkpoint', k.checkpoint), ('restore', k.restore),
        ('mg_part', lambda: k.mg_part(klib.MGP_CYCLE, 0, v.reshape(k.F, -1), variant=0, shift=1.0 / (GAMMA * 5.0))),
        ('krylov_op', lambda: k.krylov_op(klib.KOP_MULTIDOT, 2, vecs=rng.standard_normal((3, k.nlocal)))),
        ('spectral_apply', lambda: k.spectral_apply(1.0 / (GAMMA * 5.0), v)),
        ('coarse_apply', coarse_solve), ('mg_coarse 0 again', lambda: k.set_mg_coarse(0)),
    ]


def line(name, label, k, t, h, st, rc):
    sha = hashlib.sha256(np.ascontiguousarray(k.get_state(), dtype=np.float64).tobytes()).hexdigest()
    print('%s [%s] rc %d t %r h %r %s state %s' % (name, label, rc, t, h, ' '.join('%s %d' % (f, getattr(st, f)) for f in FIELDS), sha))
    if rc:
        print('%s error %s' % (name, k.last_error()))


def run(name, state, h0, tuning=1, reset_every=0, **opts):
    width = N * 4.0 / 1536
    cfg = ProblemConfig.standard(2, (N, N), L=(width, width), nlig=1)
    k = klib.KSFDHip(cfg)
    k.set_tuning(use_fused=tuning)
    k.set_state(state(cfg, 7))
    o = klib.default_step_opts(atol=0.01, rtol=1e-6, adapt=0, **opts)
    t = 0.0
    for i, (label, before) in enumerate(events(k, cfg, tuning)):
        if reset_every and i and i % reset_every == 0:
            k.set_state(state(cfg, 7))
        before()
        t, _, st, rc = k.step(t, h0, o, raise_on_error=False)
        line(name, label, k, t, h0, st, rc)
        if label == 'checkpoint':                          # a second step further on before the restore
            t, _, st, rc = k.step(t, h0, o, raise_on_error=False)
            line(name, 'on', k, t, h0, st, rc)
    k.close()


def ring():
    from ksfd_amd.dist import open_self_ring
    width = N * 4.0 / 1536
    cfg = ProblemConfig.standard(2, (N, N), L=(width, width), nlig=1)
    k, keep = open_self_ring(cfg, 0, 'host')
    k.set_state(smooth(cfg, 7))
    o = klib.default_step_opts(atol=0.01, rtol=1e-6, adapt=0, pc_type=1)
    t = 0.0
    for label, agg in (('first', None), ('agglomerate 300', 300), ('agglomerate 0', 0)):
        if agg is not None:
            k.set_mg_agglomerate(agg)
        t, _, st, rc = k.step(t, 10.0, o, raise_on_error=False)
        line('ring', label, k, t, 10.0, st, rc)
    k.close()


def main():
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    klib.LIB_PATH = os.path.abspath(sys.argv[1])     # before the first handle loads the library
    run('mg', smooth, 10.0, pc_type=1)
    run('auto', aggregated, 2.0, reset_every=3, pc_type=2, ksp_rtol=1e-11)
    run('poly', smooth, 0.05, pc_type=3)
    ring()


if __name__ == '__main__':
    main()
