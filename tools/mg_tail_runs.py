"""The coarse tail of the V cycle in one workgroup launch (ksfd_set_mg_tail): what it costs and saves, per run and per tail.

    python tools/mg_tail_runs.py [--runs 384,agg2048,1d256,64c] [--points 0,256,1024,2304,4096] [--log file]

Per run and max_points (0 = off: the parent's launches, kernel for kernel -- profiles/mg_tail_code_objects.txt): ms per step (wall clock
around the steps, device synchronised), linear iterations per step, launches per step, the tail's levels.  Every setting starts from the
same saved state on a fresh handle; the settings are visited in turn, twice (a b c ... a b c ...), and the faster visit is reported
with the other beside it.
  384      384^2 x 3 fields, options81 spacing: adaptive steps from the start values until the V cycle has owned 60 steps, that state
           saved; then 30 adaptive steps (tools/late_phase.py's run)
  agg2048  2048^2 x 2 fields tiled from a 256^2 run in the same phase (tools/agg_profile.py's state), 5 adaptive steps
  1d256    1-D nx = 256 x 3 fields, 10 fixed stiff steps h = 5, pc_type 1
  64c      64^3 x 2 fields, 3 fixed steps h = 5, pc_type 1
  whole384 the options81-style run itself (tools/long_run.py): 384^2 x 3 fields from dt = 1e-8, 1421 adaptive steps (or model time 2e5),
           whole wall time; not in the default list (about 40 s a visit): --runs whole384 --points 0,1024
Per tail (one line per run and max_points > 0 that plans one): the tail's own duration from HIP events around its launch against the
summed event durations of the launches it replaces on the same levels, both from the 'mg' class of ksfd_get_profile with eager
launches: set-up alone (S), set-up + tail through MGP_TAIL (S + T), set-up + cycle without and with the tail (S + C0, S + C1);
tail = T, replaced = C0 - C1 + T.
Handles with a halo transport are not timed here: nothing crosses between devices on one GPU, launch counts are what
tests/test_gpu_mg_tail.py asserts."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ksfd_amd import lib as klib                     # noqa: E402
from ksfd_amd.config import ProblemConfig            # noqa: E402
from ksfd_amd.initial import start_values            # noqa: E402

GAMMA = 0.43586652150845900
LOG = None


def say(line):
    print(line, flush=True)
    if LOG:
        with open(LOG, 'a') as f:
            f.write(line + '\n')


def into_the_v_cycle_regime(cfg, own=60, cap=2500):
    """adaptive steps from the start values until multigrid has preconditioned `own` steps: (state, t, h)"""
    k = klib.KSFDHip(cfg)
    k.set_state(start_values(cfg))
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6)
    t, h, n, mg = 0.0, 1e-8, 0, 0
    while n < cap and mg < own:
        t, h, st, rc = k.step(t, h, opts, raise_on_error=False)
        n += 1
        if rc:
            break
        mg += 1 if st.pc_used & klib.PC_MULTIGRID else 0
    u = k.get_state()
    k.close()
    return u, t, h, n


def problem(run):
    """(cfg, state, t, h, steps, step options, fixed step or None)"""
    adaptive = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6)
    stiff = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, pc_type=1)
    if run == '384':
        cfg = ProblemConfig.standard(2, (384, 384), L=(1.0, 1.0), nlig=2)
        u, t, h, n = into_the_v_cycle_regime(cfg)
        say('mg_tail_runs 384: state after %d steps, t %.5g h %.4g' % (n, t, h))
        return cfg, u, t, h, 30, adaptive, None
    if run == 'whole384':
        cfg = ProblemConfig.standard(2, (384, 384), L=(1.0, 1.0), nlig=2)
        return cfg, start_values(cfg), 0.0, 1e-8, 1421, adaptive, None
    if run == 'agg2048':
        m, n = 256, 2048
        small = ProblemConfig.standard(2, (m, m), L=(m / 384.0,) * 2, nlig=1)
        u, t, h, ns = into_the_v_cycle_regime(small)
        cfg = ProblemConfig.standard(2, (n, n), L=(n / 384.0,) * 2, nlig=1)
        say('mg_tail_runs agg2048: tile state after %d steps, t %.5g h %.4g' % (ns, t, h))
        return cfg, np.tile(u.reshape(small.F, m, m), (1, n // m, n // m)).reshape(-1), t, h, 5, adaptive, None
    if run == '1d256':
        cfg = ProblemConfig.standard(1, (256,), L=(256 / 384.0,), nlig=2)
        rho = 9000 + 90 * np.random.default_rng(8).standard_normal(256)
        return cfg, np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(2)]), 0.0, 5.0, 10, stiff, 5.0
    if run == '64c':
        cfg = ProblemConfig.standard(3, (64, 64, 64), L=(0.64, 0.64, 0.64), nlig=1)
        rho = 9000.0 * (1.0 + 0.01 * np.random.default_rng(3).standard_normal(cfg.N))
        return cfg, np.concatenate([rho, rho * cfg.lig_s[0] / cfg.lig_gamma[0]]), 0.0, 5.0, 3, stiff, 5.0
    raise SystemExit('unknown run %s' % run)


def visit(cfg, u, t, h, steps, opts, fixed, maxp):
    k = klib.KSFDHip(cfg)
    k.set_mg_tail(maxp)
    info = k.mg_tail_info()
    k.set_state(u)
    k.synchronize()
    t0 = time.perf_counter()
    its = launches = done = 0
    for _ in range(steps):
        t, h, st, rc = k.step(t, fixed or h, opts, raise_on_error=False)
        if rc:
            break
        its, launches, done = its + st.linear_its, launches + st.launches, done + 1
        if t > 2e5:
            break
    k.synchronize()
    wall = time.perf_counter() - t0
    tail = k.mg_tail_info()['launches']
    k.close()
    done = max(done, 1)
    return dict(ms=1e3 * wall / done, its=its / done, launches=launches / done, tail=tail / done, info=info, steps=done, wall=wall, t=t)


def tail_against_its_launches(cfg, u, shift, maxp):
    def mg_ms(k):
        return k.profile(reset=True)['mg']['ms']
    out = {}
    for on in (False, True):
        k = klib.KSFDHip(cfg)
        k.set_mg_params(power_its=klib.MG_EAGER)
        if on:
            k.set_mg_tail(maxp)
        info = k.mg_tail_info()
        k.set_state(u)
        k.set_profiling(True, only='mg')
        b = np.random.default_rng(1).standard_normal((cfg.F, cfg.N))
        res = {}
        for rep in range(3):                           # the first visit warms the code objects up; the smallest of the others counts
            k.profile(reset=True)
            k.mg_level_info(0, shift)
            s = mg_ms(k)
            k.mg_part(klib.MGP_CYCLE, 0, b, shift=shift)
            c = mg_ms(k) - s
            tl = None
            if on and info['level'] >= 1:
                bt = np.random.default_rng(2).standard_normal((cfg.F, info['points'][0]))
                k.mg_part(klib.MGP_TAIL, info['level'], bt, shift=shift)
                tl = mg_ms(k) - s
            if rep:
                res['c'] = min(res.get('c', 1e30), c)
                if tl is not None:
                    res['t'] = min(res.get('t', 1e30), tl)
        out[on] = (res, info)
        k.close()
    (r0, _), (r1, info) = out[False], out[True]
    if 't' not in r1:
        return None
    return dict(tail_us=1e3 * r1['t'], replaced_us=1e3 * (r0['c'] - r1['c'] + r1['t']), info=info)


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', default='384,agg2048,1d256,64c')
    ap.add_argument('--points', default='0,256,1024,2304,4096')
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    LOG = a.log
    points = [int(x) for x in a.points.split(',')]
    for run in a.runs.split(','):
        cfg, u, t, h, steps, opts, fixed = problem(run)
        best = {}
        for turn in range(2):
            for maxp in points:
                r = visit(cfg, u, t, h, steps, opts, fixed, maxp)
                if maxp not in best or r['ms'] < best[maxp]['ms']:
                    r['other'] = best[maxp]['ms'] if maxp in best else None
                    best[maxp] = r
                else:
                    best[maxp]['other'] = r['ms']
        for maxp in points:
            r = best[maxp]
            say('mg_tail_runs %s max_points %d: tail levels %s (%s points, %d B LDS); %d steps to t = %.4g in %.2f s: %.2f ms/step (other visit %.2f), %.1f its/step, %.0f launches/step, %.1f tail launches/step' %
                (run, maxp, 'none' if r['info']['level'] < 0 else '%d..%d' % (r['info']['level'], r['info']['level'] + r['info']['nlevels'] - 1),
                 r['info']['points'], r['info']['lds_bytes'], r['steps'], r['t'], r['wall'], r['ms'], r['other'] or float('nan'), r['its'], r['launches'], r['tail']))
        if run == 'whole384':
            continue
        shift = 1.0 / (GAMMA * (fixed or h))
        seen = set()
        for maxp in points:
            lv = tuple(best[maxp]['info']['points'])
            if maxp == 0 or not lv or lv in seen:
                continue
            seen.add(lv)
            r = tail_against_its_launches(cfg, u, shift, maxp)
            if r:
                say('mg_tail_runs %s max_points %d: the tail (%s points) %.1f us against %.1f us of the launches it replaces (HIP events, eager, shift %.4g)' %
                    (run, maxp, list(lv), r['tail_us'], r['replaced_us'], shift))


if __name__ == '__main__':
    main()
