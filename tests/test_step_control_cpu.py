"""CPU: the decisions of the step driver (ksfd_amd/csrc/step_control.h) on their own.  The header is plain C++ without device code and
without the handle -- that the small driver below compiles with the host compiler alone is the proof -- so the driver exercises exactly
what ksfd_step runs: the TSAdaptBasic controller against the oracle's, the stage-guess least squares against numpy, and the shift-floor
search, the spectral back-off and the regime table against restatements of their rules in Python; the verdict after a defect-correction
sweep of the spectral solver (predicted last sweep, contraction memory) on residual histories with the verdicts written out by hand and
on a grid against a restatement; the refresh schedule of the polynomial's eigenvalue estimate on a scripted run of steps."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import ko

DRIVER = r'''
#include "step_control.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
using namespace ksfd_ctl;
static FILE *f;
static double rd() { double v; if (fscanf(f, "%lf", &v) != 1) exit(3); return v; }
static int ri() { return (int)rd(); }
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    f = fopen(argv[2], "r");
    if (!f) return 2;
    const int n = ri();
    if (!strcmp(argv[1], "adapt")) {
        for (int k = 0; k < n; k++) {
            const double h = rd(), e = rd(); const int prev = ri();
            const double safety = rd(), rs = rd(), lo = rd(), hi = rd(), dmin = rd(), dmax = rd();
            const AdaptChoice c = adapt_basic(h, e, prev != 0, safety, rs, lo, hi, dmin, dmax);
            printf("%d %.17g\n", c.accept ? 1 : 0, c.hnext);
        }
    } else if (!strcmp(argv[1], "guess")) {
        for (int k = 0; k < n; k++) {
            const int i = ri(), j0 = ri(), ng = ri();
            double gb[4][4], cf[3];
            for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) gb[a][b] = rd();
            const bool ok = stage_guess(gb, i, j0, ng, cf);
            printf("%d %.17g %.17g %.17g\n", ok ? 1 : 0, cf[0], cf[1], cf[2]);
        }
    } else if (!strcmp(argv[1], "floor")) {
        StepMemo m;
        for (int k = 0; k < n; k++) {
            const double its = rd(), shift = rd();
            shift_floor_update(m, its, shift);
            printf("%.17g %d %d %d %.17g %.17g\n", m.mg_shift_floor, m.sf_dir, m.sf_hold, m.sf_tried_down ? 1 : 0, m.sf_prev_its, m.sf_prev_floor);
        }
    } else if (!strcmp(argv[1], "backoff")) {
        StepMemo m;
        for (int k = 0; k < n; k++) {
            const int failed = ri(), its = ri(); const long long nsteps = (long long)rd();
            spec_backoff_update(m, failed != 0, its, nsteps);
            printf("%lld %d\n", m.spec_bad_until, m.spec_backoff);
        }
    } else if (!strcmp(argv[1], "regime")) {
        for (int k = 0; k < n; k++) {
            RegimeIn in;
            in.pc_type = ri(); in.reserved = ri(); in.stiff = rd(); in.direct = ri(); in.dr_on = ri(); in.spec_ok = ri(); in.user_off = ri();
            in.use_frozen = ri(); in.fused2d = ri(); in.mg_ok = ri(); in.mg_threshold = rd(); in.spec_from = rd();
            in.nsteps = (long long)rd(); in.bad_until = (long long)rd(); in.unknowns = rd(); in.ring = ri(); in.device_allreduce = ri(); in.async_mode = ri();
            const Regime r = choose_regime(in);
            printf("%d %d %d %d %d\n", r.spec ? 1 : 0, r.mg ? 1 : 0, r.poly_wanted ? 1 : 0,
                   pipelined_allowed(in, r, r.poly_wanted) ? 1 : 0, pipelined_allowed(in, r, false) ? 1 : 0);
        }
    } else if (!strcmp(argv[1], "sweep")) {
        /* a script over one StepMemo.  op 0: set (rho_step, rho_prev) = (a, b); 1: spec_rho_roll; 2: spec_sweep.  Every row prints
           verdict (-1 for ops 0 and 1), rho_step, rho_prev, spec_pred_bound(m, rn, bn) */
        StepMemo m;
        for (int r = 0; r < n; r++) {
            const int op = ri(), k = ri(), cap = ri(); const double rn = rd(), rprev = rd(), tol = rd(); const int guess = ri(), predict = ri(); const double bn = rd();
            int v = -1;
            if (op == 0) { m.spec_rho_step = rn; m.spec_rho_prev = rprev; }
            else if (op == 1) spec_rho_roll(m);
            else v = (int)spec_sweep(k, cap, rn, rprev, tol, guess != 0, predict != 0, m);
            printf("%d %.17g %.17g %.17g\n", v, m.spec_rho_step, m.spec_rho_prev, spec_pred_bound(m, rn, bn));
        }
    } else if (!strcmp(argv[1], "specmisc")) {
        for (int r = 0; r < n; r++) {
            const int pc_type = ri(), backoff = ri(), mg_ok = ri(); const double stiff = rd(); const int sp = ri(), reserved = ri(); const double rtol = rd();
            const int venv = ri(); const double rn = rd(), bn = rd(), grel = rd();
            const bool zero = spec_handover(rn, bn);
            printf("%d %d %d %d %.17g\n", spec_gmres_cap(pc_type, backoff), spec_fallback_mg(mg_ok != 0, stiff) ? 1 : 0,
                   spec_predict_on(sp != 0, reserved, rtol, venv) ? 1 : 0, zero ? 1 : 0, spec_handover_rel(grel, zero, rn, bn));
        }
        printf("%d %.17g %.17g %.17g\n", SPEC_SWEEP_CAP, SPEC_SLOW_RATIO, SPEC_PRED_SAFETY, SPEC_PRED_MIN_RTOL);
    } else if (!strcmp(argv[1], "lam")) {
        /* one row per step: the estimate the power iteration would return if it ran.  Prints due, iterations, lam_age, lam_period */
        StepMemo m;
        for (int r = 0; r < n; r++) {
            const double est = rd();
            const bool due = lam_due(m);
            int its = 0;
            if (due) { const double before = m.lamJ; its = lam_power_its(before); m.lamJ = est; lam_estimated(m, before); }
            printf("%d %d %d %d\n", due ? 1 : 0, its, m.lam_age, m.lam_period);
        }
    } else if (!strcmp(argv[1], "memo")) {          /* the initial values */
        StepMemo m;
        printf("%.17g %d %d %.17g %d %d %d %.17g %.17g %lld %lld %d %.17g %.17g\n", m.lamJ, m.lam_age, m.lam_period, m.mg_shift_floor, m.sf_dir, m.sf_hold,
               m.sf_tried_down ? 1 : 0, m.sf_prev_its, m.sf_prev_floor, m.nsteps, m.spec_bad_until, m.spec_backoff, m.spec_rho_step, m.spec_rho_prev);
    } else return 2;
    return 0;
}
'''


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    # the host compiler, else the compiler the library itself is built with (the header is plain C++ either way)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('hipcc') or (hipcc if os.path.exists(hipcc) else None)
    if not cxx:
        pytest.fail('no C++ compiler found (g++, c++, hipcc): the library cannot have been built either')
    d = tmp_path_factory.mktemp('stepctl')
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / 'drv'
    subprocess.run([cxx, '-x', 'c++', '-O1', '-std=c++17', '-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(mode, rows):
        inp = d / (mode + '.txt')
        with open(inp, 'w') as f:
            f.write('%d\n' % len(rows))
            f.write('\n'.join(' '.join(repr(float(x)) for x in row) for row in rows) + '\n')
        r = subprocess.run([str(exe), mode, str(inp)], capture_output=True, text=True, check=True, timeout=60)
        return [[float(x) for x in line.split()] for line in r.stdout.splitlines()]
    return run


def test_memo_starts_as_the_handle_did(driver):
    # lamJ, lam_age, lam_period, mg_shift_floor, sf_dir, sf_hold, sf_tried_down, sf_prev_its, sf_prev_floor, nsteps, bad_until, backoff, rho_step, rho_prev
    assert driver('memo', [])[0] == [-1.0, 0, 1, 0.0, 0, 0, 0, 0.0, 0.0, 0, 0, 8, 0.0, 0.0]


def test_controller_matches_the_oracle(driver):
    dt_min, dt_max, safety, rs, clip = 1e-20, 1e4, 0.9, 0.5, (0.1, 5.0)
    enorms = [0.0, 1e-9, 1e-3, 0.5, 1.0, np.nextafter(1.0, 2.0), 2.0, 1e3, 1e12]
    hs = [dt_min, dt_min * (1 + 1e-9), 1e-3, dt_max / 2]
    cases = list(itertools.product(enorms, [True, False], hs))
    out = driver('adapt', [[h, e, prev, safety, rs, clip[0], clip[1], dt_min, dt_max] for e, prev, h in cases])
    assert len(out) == len(cases)
    n_rejected = 0
    for (e, prev, h), (acc, hn) in zip(cases, out):
        want, wacc = ko.adapt_basic(h, e, safety=safety, clip=clip, dt_min=dt_min, dt_max=dt_max, prev_accept=prev, reject_safety=rs)
        assert bool(acc) == wacc, (e, prev, h)
        # the same formula in doubles through the same pow: the margin covers a differing contraction between two compilers and nothing else
        assert abs(hn - want) <= 2 * np.spacing(max(abs(hn), abs(want))), (e, prev, h, hn, want)
        n_rejected += not wacc
    assert n_rejected > 0 and n_rejected < len(cases)


# ---- stage guess ---------------------------------------------------------------------------------------------------------------------
def _rhs_family(seed, eps1):
    """four right-hand sides as they come in a step: b_1 = c b_0 + eps1 * noise, the later ones a few per cent off the span of the earlier
    ones.  b_0 and every noise vector have unit norm, so eps1 is the angle between b_0 and b_1 (up to c) and the condition number of
    their Gram matrix is ~ 4 / eps1^2 whatever the seed."""
    rng = np.random.default_rng(seed)
    unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.standard_normal(500))
    b = [unit()]
    b.append(0.8 * b[0] + eps1 * unit())
    b.append(0.5 * b[0] + 0.6 * b[1] + 0.04 * unit())
    b.append(-0.3 * b[0] + 0.7 * b[1] + 0.5 * b[2] + 0.05 * unit())
    B = np.array(b)
    return B @ B.T


def _guess_rows(G, blocks):
    rows, refs = [], []
    for i, j0 in blocks:
        ng = i - j0
        A = G[j0:i, j0:i].copy()
        A[np.diag_indices(ng)] *= 1.0 + 1e-13
        rows.append([i, j0, ng] + list(G.ravel()))
        refs.append((np.linalg.solve(A, G[i, j0:i]), np.linalg.cond(A)))
    return rows, refs


BLOCKS = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]        # (stage i, first stage j0 of the guess): ng = 1, 2, 3 and j0 > 0

# eps1 = 0.03: the largest condition number of a regularised Gram block over BLOCKS is 5.07e3 (seed 1), 4.74e3 (seed 2), 4.81e3 (seed 3),
# asserted <= 1e4; the coefficients must match to 1e-10 = 100 * kappa * eps at kappa = 1e4.  With the 1e-3 that a step really shows
# between b_0 and b_1 no seed gets there -- the blocks that hold both have kappa ~ 4 / 1e-6 (4.31e6 for seed 1, 4.29e6 for seed 2) -- so
# that family is checked as well, by the same rule with its own bound on kappa: 100 * 1e7 * eps = 2.2e-7.
@pytest.mark.parametrize('seed,eps1,kappa_max', [(1, 0.03, 1e4), (2, 0.03, 1e4), (3, 0.03, 1e4), (1, 1e-3, 1e7), (2, 1e-3, 1e7)])
def test_stage_guess_matches_numpy(driver, seed, eps1, kappa_max):
    G = _rhs_family(seed, eps1)
    rows, refs = _guess_rows(G, BLOCKS)
    out = driver('guess', rows)
    worst = max(k for _, k in refs)
    print('seed %d eps1 %g: largest condition number %.3g' % (seed, eps1, worst))
    assert worst <= kappa_max
    tol = 1e-10 if kappa_max == 1e4 else 100 * kappa_max * np.finfo(float).eps
    for (i, j0), (ok, *cf), (ref, kappa) in zip(BLOCKS, out, refs):
        ng = i - j0
        assert ok == 1, (i, j0)
        err = np.linalg.norm(np.array(cf[:ng]) - ref) / np.linalg.norm(ref)
        print('  i %d j0 %d: kappa %.3g, relative error %.2e' % (i, j0, kappa, err))
        assert err <= tol, (i, j0, err)
        assert all(c == 0.0 for c in cf[ng:])


def test_stage_guess_refusals(driver):
    G = _rhs_family(1, 0.03)
    orth = G.copy(); orth[3, :3] = 0.0; orth[:3, 3] = 0.0       # b_3 orthogonal to the earlier ones: predicted residual = ||b_3||^2 >= 0.09 ||b_3||^2
    zero = G.copy(); zero[:3, :3] = 0.0                          # all-zero Gram block
    nan = G.copy(); nan[1, 1] = float('nan')
    nan_rhs = G.copy(); nan_rhs[3, 2] = nan_rhs[2, 3] = float('nan')
    far = G.copy(); far[3, 3] *= 30.0                            # b_3 mostly outside the span: solvable, but the guess would not pay
    rows = [[3, 0, 3] + list(orth.ravel()), [3, 1, 2] + list(orth.ravel()), [3, 0, 3] + list(zero.ravel()), [2, 1, 1] + list(zero.ravel()),
            [3, 0, 3] + list(nan.ravel()), [2, 1, 1] + list(nan.ravel()), [3, 1, 2] + list(nan_rhs.ravel()), [3, 0, 3] + list(far.ravel()),
            [3, 3, 0] + list(G.ravel())]
    out = driver('guess', rows)
    assert [o[0] for o in out] == [0] * len(rows)
    assert driver('guess', [[3, 0, 3] + list(G.ravel())])[0][0] == 1   # the same call on the unspoilt matrix gives a guess


# ---- shift-floor search --------------------------------------------------------------------------------------------------------------
class FloorSearch:
    """the rule of the online search for the multigrid shift floor, restated: when a step needs > 64 iterations, double the floor while
    that pays (> 5 % fewer iterations), else go back and try halving, else settle for 25 steps"""

    def __init__(self):
        self.floor, self.dir, self.hold, self.tried_down, self.prev_its, self.prev_floor = 0.0, 0, 0, False, 0.0, 0.0
        self.seen = set()

    def update(self, its, shift):
        if self.dir == 0:
            if self.hold > 0:
                self.hold -= 1
                self.seen.add('holding')
            elif its > 64.0:
                self.prev_its, self.prev_floor = its, self.floor
                self.floor = 2.0 * max(self.floor, shift)
                self.dir, self.tried_down = 1, False
                self.seen.add('probe starts')
            else:
                self.seen.add('quiet')
        elif its < 0.95 * self.prev_its:
            self.seen.add('doubling pays' if self.dir > 0 else 'halving pays')
            self.prev_its, self.prev_floor = its, self.floor
            self.floor = 2.0 * self.floor if self.dir > 0 else 0.5 * self.floor
            if self.floor <= shift:
                self.dir, self.hold = 0, 25
                self.seen.add('floor at or below the shift')
        else:
            self.floor = self.prev_floor
            if self.dir > 0 and not self.tried_down and 0.5 * self.prev_floor > shift:
                self.dir, self.tried_down = -1, True
                self.floor = 0.5 * self.prev_floor
                self.seen.add('doubling does not pay, halving tried')
            else:
                if self.dir > 0 and not self.tried_down:
                    self.seen.add('halving refused: half the previous floor is not above the shift')
                self.dir, self.hold = 0, 25
                self.seen.add('settled')

    def fields(self):
        return [self.floor, self.dir, self.hold, int(self.tried_down), self.prev_its, self.prev_floor]


# seeds whose 400 steps reach every branch (a settled search holds for 25 steps, so not every sequence does); asserted below
@pytest.mark.parametrize('seed', [11, 13, 15])
def test_shift_floor_search(driver, seed):
    rng = np.random.default_rng(seed)
    n = 400
    # iterations per step: mostly above the trigger, falling or rising from step to step; shifts: a slow walk over three decades with single-step excursions
    its = np.round(rng.choice([20.0, 70.0, 120.0, 300.0], n) * rng.uniform(0.6, 1.4, n))
    walk = np.cumsum(rng.normal(0.0, 0.15, n))
    spike = np.where(rng.random(n) < 0.15, rng.normal(0.0, 1.5, n), 0.0)
    shift = 10.0 ** (-1.5 + np.clip(walk, -1.5, 1.5) + spike)
    out = driver('floor', list(zip(its, shift)))
    ref = FloorSearch()
    for k in range(n):
        ref.update(float(its[k]), float(shift[k]))
        assert out[k] == ref.fields(), (k, out[k], ref.fields())
    for branch in ('doubling pays', 'doubling does not pay, halving tried', 'halving refused: half the previous floor is not above the shift',
                   'floor at or below the shift', 'holding', 'settled'):
        assert branch in ref.seen, branch


def test_spectral_backoff(driver):
    # failures at steps 10, 11, ...: bad_until = nsteps + the back-off as it was before the doubling; 8 -> 16 -> ... -> 512 and stays
    rows = [[1, 4, 10 + k] for k in range(9)]
    rows += [[0, 48, 30]]                 # a good step (48 iterations = 12 per stage is still good): back to 8, bad_until untouched
    rows += [[0, 49, 31]]                 # > 48 iterations without a failure counts as bad
    rows += [[0, 4, 32]]
    out = driver('backoff', rows)
    before = [8, 16, 32, 64, 128, 256, 512, 512, 512]
    for k in range(9):
        assert out[k] == [10 + k + before[k], min(2 * before[k], 512)], k
    assert out[9] == [18 + 512, 8]
    assert out[10] == [31 + 8, 16]
    assert out[11] == [31 + 8, 8]


# ---- regime table --------------------------------------------------------------------------------------------------------------------
def regime(pc_type, reserved, X, direct, dr_on, spec_ok, user_off, use_frozen, fused, mg_ok, mg_threshold, spec_from, nsteps, bad_until,
           unknowns, ring, dev_allreduce, async_mode):
    """the choice of ksfd_step restated: (spectral, V cycle, polynomial wanted, pipelined if the polynomial is confirmed, ... if it is not)"""
    mg_from = mg_threshold * (3.0 if unknowns < 8.0e6 else 1.0)
    spec = (not direct) and spec_ok and use_frozen and (
        pc_type == 4 or (pc_type == 2 and X >= (spec_from if fused else max(spec_from, 0.3)) and nsteps > bad_until and not user_off))
    mg = (not direct) and (not spec) and mg_ok and use_frozen and (pc_type == 1 or (pc_type == 2 and X > mg_from))
    poly = (not spec) and (not mg) and use_frozen and pc_type in (2, 3) and X >= 0.3
    small = unknowns <= 6.0e6

    def pipelined(use_poly):
        return ((not dr_on) and (not direct) and (not spec) and (not mg) and (not use_poly) and use_frozen and not (reserved & 1) and X >= 1e-3
                and ((not ring) or dev_allreduce) and (async_mode == 1 or (async_mode == 2 and small)))
    return [int(spec), int(mg), int(poly), int(pipelined(poly)), int(pipelined(False))]


def test_regime_table(driver):
    Xs = [0.05, 0.1, 0.29, 0.3, 1.0, 74.0, 76.0, 224.0, 226.0, 300.0]
    unknowns = [np.nextafter(8e6, 0), np.nextafter(8e6, 1e9), np.nextafter(6e6, 0), np.nextafter(6e6, 1e9), 6e6, 8e6]
    # (dr_on, ring, device all-reduce, use_frozen)
    modes = [(0, 0, 0, 1), (1, 0, 0, 1), (0, 1, 1, 1), (0, 1, 0, 1), (0, 0, 0, 0)]
    rows = []
    for pc, X, unk, spec_ok, user_off, late, mg_ok, fused, res, am, (dr, ring, dev, frozen) in itertools.product(
            range(6), Xs, unknowns, (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), modes):
        # late: nsteps > bad_until; else nsteps == bad_until (the last step of a back-off period)
        rows.append([pc, res, X, int(pc == 5), dr and pc != 5, spec_ok, user_off, frozen, fused, mg_ok, 75.0, 0.1, 41 if late else 40, 40, unk, ring, dev, am])
    out = driver('regime', rows)
    assert len(out) == len(rows)
    seen = set()
    for row, got in zip(rows, out):
        want = regime(*row)
        assert got == want, (row, got, want)
        seen.add(tuple(want))
    # every regime occurs: spectral, V cycle, polynomial, pipelined, plain
    assert {(1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 1, 0, 1), (0, 0, 0, 1, 1), (0, 0, 0, 0, 0)} <= seen


# ---- defect-correction sweeps of the spectral solver -----------------------------------------------------------------------------------
NOT_FINITE, CONVERGED, SLOW, CONTINUE, FINAL = range(5)
CAP = 24


def _sweep_script(driver, rows):
    """rows: ('set', rho_step, rho_prev) | ('roll',) | ('sweep', k, rn, rprev, tol, guess, predict[, cap]); ||b|| = 1"""
    raw = []
    for r in rows:
        if r[0] == 'set':
            raw.append([0, 0, 0, r[1], r[2], 0.0, 0, 0, 1.0])
        elif r[0] == 'roll':
            raw.append([1, 0, 0, 0.0, 0.0, 0.0, 0, 0, 1.0])
        else:
            _, k, rn, rprev, tol, guess, predict = r[:7]
            raw.append([2, k, r[7] if len(r) > 7 else CAP, rn, rprev, tol, guess, predict, 1.0])
    return driver('sweep', raw)


def test_sweep_verdicts_on_scripted_histories(driver):
    # contraction 0.01 per sweep from zero, no guess, nothing remembered, tol 1e-7: sweep 0 records nothing and predicts nothing; sweep 1
    # records 0.01 but 4 * 0.01 * 1e-4 = 4e-6 > tol; sweep 2: 4 * 0.01 * 1e-6 = 4e-8 <= tol -- the next sweep is the predicted last one
    out = _sweep_script(driver, [('sweep', 0, 1e-2, 1.0, 1e-7, 0, 1), ('sweep', 1, 1e-4, 1e-2, 1e-7, 0, 1), ('sweep', 2, 1e-6, 1e-4, 1e-7, 0, 1)])
    assert [o[0] for o in out] == [CONTINUE, CONTINUE, FINAL]
    assert out[0][1:3] == [0.0, 0.0]
    assert out[1][1:3] == [1e-4 / 1e-2, 0.0] and out[2][1:3] == [max(1e-4 / 1e-2, 1e-6 / 1e-4), 0.0]
    assert out[2][3] == 4.0 * out[2][1] * 1e-6                   # the bound a predicted exit reports (||b|| = 1)
    # the previous step left rho_prev = 0.01 and tol = 1e-3 would allow 4 * 0.01 * 1e-2 = 4e-4 after sweep 0: from zero that sweep is
    # not predicted from, with a guess it is
    out = _sweep_script(driver, [('set', 0.0, 0.01), ('sweep', 0, 1e-2, 1.0, 1e-3, 0, 1), ('sweep', 0, 1e-2, 1.0, 1e-3, 1, 1),
                                 ('sweep', 1, 1e-4, 1e-2, 1e-5, 0, 1)])
    assert [o[0] for o in out[1:]] == [CONTINUE, FINAL, FINAL]
    assert out[1][1:3] == [0.0, 0.01] and out[2][1:3] == [0.0, 0.01]      # sweep 0 is never recorded, guess or not
    # with a guess but nothing remembered there is nothing to predict from
    assert _sweep_script(driver, [('sweep', 0, 1e-2, 1.0, 1e-3, 1, 1)])[0][0] == CONTINUE
    # exactly a quarter is not slow, the next double above it is; neither a slow nor a converged sweep is recorded
    above = float(np.nextafter(0.25, 1.0))
    out = _sweep_script(driver, [('sweep', 1, 0.25, 1.0, 1e-7, 0, 1), ('set', 0.0, 0.0), ('sweep', 1, above, 1.0, 1e-7, 0, 1),
                                 ('sweep', 1, 1e-8, 1.0, 1e-7, 0, 1), ('sweep', 1, float('nan'), 1.0, 1e-7, 0, 1)])
    assert [o[0] for o in out] == [CONTINUE, -1, SLOW, CONVERGED, NOT_FINITE]
    assert out[0][1] == 0.25 and out[2][1] == 0.0 and out[3][1] == 0.0 and out[4][1] == 0.0
    # no predicted last sweep when there is no sweep left under the cap
    out = _sweep_script(driver, [('set', 0.0, 0.01), ('sweep', CAP - 2, 1e-4, 1e-2, 1e-5, 0, 1), ('sweep', CAP - 1, 1e-4, 1e-2, 1e-5, 0, 1),
                                 ('sweep', 2, 1e-4, 1e-2, 1e-5, 0, 1, 3), ('sweep', 1, 1e-4, 1e-2, 1e-5, 0, 1, 3)])
    assert [o[0] for o in out[1:]] == [FINAL, CONTINUE, CONTINUE, FINAL]
    # prediction off: plain continue everywhere, the memory still fills
    out = _sweep_script(driver, [('set', 0.0, 0.01), ('sweep', 0, 1e-2, 1.0, 1e-3, 1, 0), ('sweep', 1, 1e-4, 1e-2, 1e-5, 0, 0),
                                 ('sweep', 2, 1e-6, 1e-4, 1e-7, 1, 0)])
    assert [o[0] for o in out[1:]] == [CONTINUE] * 3 and out[3][1] > 0.0
    # start of a step: this step's maximum replaces the last one's; a step that recorded none keeps the previous one
    out = _sweep_script(driver, [('set', 0.02, 0.01), ('roll',), ('roll',), ('set', 0.0, 0.0), ('roll',)])
    assert [o[1:3] for o in out] == [[0.02, 0.01], [0.0, 0.02], [0.0, 0.02], [0.0, 0.0], [0.0, 0.0]]


def sweep_rule(k, cap, rn, rprev, tol, guess, predict, rho_step, rho_prev):
    """spec_solve's rule after the true residual of sweep k, restated: -> (verdict, rho_step)"""
    if rn != rn:
        return NOT_FINITE, rho_step
    if rn <= tol:
        return CONVERGED, rho_step
    if rn > 0.25 * rprev:
        return SLOW, rho_step
    if k >= 1:
        rho_step = max(rho_step, rn / rprev)
    rho_hat = max(rho_step, rho_prev)
    final = predict and rho_hat > 0.0 and (k >= 1 or guess) and k + 1 < cap and 4.0 * rho_hat * rn <= tol
    return (FINAL if final else CONTINUE), rho_step


def test_sweep_verdict_grid(driver):
    ratios = [1e-3, 0.1, 0.25, float(np.nextafter(0.25, 1.0)), 0.5, float('nan')]
    over_tol = [0.5, 1.0, float(np.nextafter(1.0, 2.0)), 3.0, 30.0, 1e3]         # rn / tol
    rows, want = [], []
    for k, ratio, ot, guess, predict, rho_prev, rho_step in itertools.product(
            [0, 1, 2, CAP - 2, CAP - 1], ratios, over_tol, (0, 1), (0, 1), [0.0, 0.005, 0.05, 0.3], [0.0, 0.02]):
        rprev = 0.5
        rn = ratio * rprev
        tol = rn / ot if rn == rn else 1e-6
        rows += [('set', rho_step, rho_prev), ('sweep', k, rn, rprev, tol, guess, predict)]
        want.append(sweep_rule(k, CAP, rn, rprev, tol, guess, predict, rho_step, rho_prev))
    out = _sweep_script(driver, rows)[1::2]
    assert len(out) == len(want)
    for (v, rs, rp, _), (wv, wrs), row in zip(out, want, rows[1::2]):
        assert (v, rs) == (wv, wrs), (row, v, rs, wv, wrs)
    assert {w[0] for w in want} == {NOT_FINITE, CONVERGED, SLOW, CONTINUE, FINAL}


def test_spectral_attempt_rules(driver):
    rows = []
    for pc, backoff, mg_ok, stiff, sp, res, rtol, venv, (rn, bn) in itertools.product(
            (0, 2, 4), (8, 9, 16, 512), (0, 1), (0.3, float(np.nextafter(0.3, 1.0)), 5.0), (0, 1), (0, 8, 9), (1e-6, 1e-8, float(np.nextafter(1e-8, 0.0))),
            (0, 1, 2), [(0.5, 1.0), (1.0, 1.0), (2.0, 1.0), (float('nan'), 1.0)]):
        rows.append([pc, backoff, mg_ok, stiff, sp, res, rtol, venv, rn, bn, 1e-3])
    out = driver('specmisc', rows)
    assert out.pop() == [24, 0.25, 4.0, 1e-8]
    assert len(out) == len(rows)
    for (pc, backoff, mg_ok, stiff, sp, res, rtol, venv, rn, bn, grel), got in zip(rows, out):
        zero = not rn < bn                                          # the sweeps made it worse (or NaN): restart from zero
        want = [(8 if backoff > 8 else 40) if pc == 2 else 0, int(bool(mg_ok) and stiff > 0.3),
                int(bool(sp) and not (res & 8) and rtol >= 1e-8 and venv != 2), int(zero), grel * (1.0 if zero else rn / bn)]
        assert got == want, (pc, backoff, mg_ok, stiff, sp, res, rtol, venv, rn, bn, got, want)


def test_eigenvalue_estimate_policy(driver):
    # estimates as the power iteration would return them, one per step (looked at only on the steps where one is due)
    est = [10.0] + [10.1] * 22 + [10.1 * 1.03] + [10.4] * 3
    out = driver('lam', [[e] for e in est])
    due = [k for k, o in enumerate(out) if o[0] == 1]
    # first step: due, 8 iterations; then every period steps with 2; the period doubles 1, 2, 4, 8, 8 while the estimate holds still,
    # so estimates fall on steps 0, 1, 3, 7, 15, 23; the 3 % move at step 23 resets it to 1: step 24 is due again
    assert due == [0, 1, 3, 7, 15, 23, 24, 26]
    assert [out[k][1] for k in due] == [8] + [2] * 7
    assert [out[k][3] for k in due] == [1, 2, 4, 8, 8, 1, 2, 4]
    assert all(o[1] == 0 for k, o in enumerate(out) if k not in due)
    # lam_age: untouched on the first step (there is no estimate yet), then steps since the last estimate
    want_age, last = [], 0
    for k in range(len(est)):
        last = k if k in due else last
        want_age.append(k - last)
    assert [o[2] for o in out] == want_age
