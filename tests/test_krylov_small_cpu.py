"""CPU: the small host algebra of the Krylov solvers (ksfd_amd/csrc/krylov_small.h) on its own.  The header is plain C++ without device
code and without the handle -- that the small driver below compiles with the host compiler alone is the proof -- so the driver exercises
exactly what gmres(), gmres_async() and gmres_dr() run: the incremental Hessenberg QR and hess_lsq against numpy.linalg.lstsq, the
algebraic second Gram-Schmidt projection against the explicit one, the recycling rules, the cycle lengths and the basis size against
restatements in Python, and the Chebyshev coefficients of the polynomial preconditioner (poly_setup) against numpy's Chebyshev polynomials."""
import contextlib
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

try:        # hundreds of tiny least-squares problems: a threaded BLAS spends twenty times their cost on its threads
    from threadpoolctl import threadpool_limits
except ImportError:
    threadpool_limits = lambda limits: contextlib.nullcontext()

EPS = np.finfo(float).eps

DRIVER = r'''
#include "krylov_small.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
using namespace ksfd_krylov;
static FILE *f;
static double rd() { double v; if (fscanf(f, "%lf", &v) != 1) exit(3); return v; }
static int ri() { return (int)rd(); }
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    f = fopen(argv[2], "r");
    if (!f) return 2;
    const int n = ri();
    if (!strcmp(argv[1], "qr")) {
        /* one line per pushed column: free back substitution bit-equal (0/1), residual estimate, y[0..j] */
        for (int c = 0; c < n; c++) {
            const int m = ri(), ldx = ri(); const double beta = rd();
            HessQR qr(m);
            qr.reset(beta);
            std::vector<double> hcol(m + 2), Hx((size_t)ldx * m), gx(ldx), yx(m);
            for (int j = 0; j < m; j++) {
                for (int i = 0; i <= j + 1; i++) hcol[i] = rd();
                const double est = qr.push_column(j, hcol.data());
                if (memcmp(&qr.Hraw[(size_t)qr.ld * j], hcol.data(), sizeof(double) * (j + 2))) return 4;      /* the column as it came is kept */
                qr.solve(j + 1);
                for (int q = 0; q <= j; q++) for (int i = 0; i <= m; i++) Hx[(size_t)ldx * q + i] = qr.H[(size_t)qr.ld * q + i];
                for (int i = 0; i <= m; i++) gx[i] = qr.g[i];
                hess_backsolve(Hx.data(), ldx, gx.data(), j + 1, yx.data());
                printf("%d %.17g", memcmp(yx.data(), qr.y.data(), sizeof(double) * (j + 1)) == 0 ? 1 : 0, est);
                for (int i = 0; i <= j; i++) printf(" %.17g", qr.y[i]);
                printf("\n");
            }
        }
    } else if (!strcmp(argv[1], "lsq")) {
        for (int c = 0; c < n; c++) {
            const int k = ri();
            std::vector<double> H((size_t)(k + 1) * k), g(k + 1), y(k), Hy(k + 1);
            for (size_t i = 0; i < H.size(); i++) H[i] = rd();
            for (int i = 0; i <= k; i++) g[i] = rd();
            hess_lsq(H.data(), k, g.data(), y.data(), Hy.data());
            for (int i = 0; i < k; i++) printf("%.17g ", y[i]);
            for (int i = 0; i <= k; i++) printf("%.17g ", Hy[i]);
            printf("\n");
        }
    } else if (!strcmp(argv[1], "cgs2")) {
        for (int c = 0; c < n; c++) {
            const int k = ri(), ld = ri(); const double ww = rd();
            std::vector<double> d(k), hcol(k), Gm((size_t)ld * ld, 0.0);
            for (int i = 0; i < k; i++) d[i] = rd();
            for (int i = 0; i < k; i++) for (int l = 0; l < k; l++) Gm[(size_t)i * ld + l] = rd();
            double hn2 = 0.0;
            const bool direct = cgs2_algebraic(Gm.data(), ld, k, d.data(), ww, hcol.data(), &hn2);
            printf("%d %.17g", direct ? 1 : 0, hn2);
            for (int i = 0; i < k; i++) printf(" %.17g", hcol[i]);
            printf("\n");
        }
    } else if (!strcmp(argv[1], "recycle")) {
        for (int c = 0; c < n; c++) {
            const int stage = ri(), q = ri(), rec_mode = ri(), pcmode = ri(), rec_mg = ri(), use_frozen = ri(), restart_alloc = ri(), rec_vtop = ri();
            const RecycleChoice r = recycle_decide(pcmode, stage, rec_mode, rec_mg != 0, use_frozen != 0, restart_alloc, rec_vtop);
            printf("%d %d %d %d %d\n", r.rec_on ? 1 : 0, r.rec_full ? 1 : 0, r.reset ? 1 : 0,
                   recycle_uses(stage, q, rec_mode, false) ? 1 : 0, recycle_uses(stage, q, rec_mode, true) ? 1 : 0);
        }
    } else if (!strcmp(argv[1], "cheb")) {
        for (int c = 0; c < n; c++) {
            const double lamJ = rd(), shift = rd(), target = rd(); const int max_deg = ri();
            double alpha[8] = { 0.0 };
            printf("%d", cheb_setup(lamJ, shift, target, max_deg, alpha));
            for (int i = 0; i < 8; i++) printf(" %.17g", alpha[i]);
            printf("\n");
        }
    } else if (!strcmp(argv[1], "cycle")) {
        for (int c = 0; c < n; c++) {
            const int restart_alloc = ri(), vb = ri(), m_opt = ri(), rec_on = ri(), rec_full = ri(), m_cur = ri(), grow = ri(), reserved = ri(), k = ri();
            const int ksp_restart = ri(), maxk = ri(); const double rn = rd(), bn = rd(), tol_abs = rd(), ksp_rtol = rd();
            const int room = cycle_room(restart_alloc, vb);
            printf("%d %d %d %d %d %.17g\n", room, cycle_first(m_opt, room, rec_on != 0, rec_full != 0), cycle_next(m_cur, room, grow != 0),
                   gs_classic(reserved, k) ? 1 : 0, async_cycle(ksp_restart, restart_alloc, maxk), rel_of(rn, bn, tol_abs, ksp_rtol));
        }
    } else if (!strcmp(argv[1], "fit")) {           /* env < 0: KSFD_RESTART_MAX not set */
        for (int c = 0; c < n; c++) {
            const double mfree = rd(), vecbytes = rd(); const int env = ri();
            const int cap = env < 0 ? RESTART_MAX : restart_cap(env);
            printf("%d %d\n", cap, restart_fit(mfree, vecbytes, cap));
        }
        printf("%d %d %d\n", RESTART_DEFAULT, RESTART_MAX, RESTART_MIN);
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
    d = tmp_path_factory.mktemp('krylov_small')
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


# ---- Hessenberg QR and hess_lsq ------------------------------------------------------------------------------------------------------
MS = [1, 2, 3, 5, 8, 13, 30, 31, 64, 120]


def _hessenberg(m, seed):
    """(m+1) x m upper Hessenberg: standard normal upper triangle, +4 on the diagonal, subdiagonal uniform in [0.5, 1.5]; beta in [0.5, 2]"""
    rng = np.random.default_rng(1000 * m + seed)
    H = np.zeros((m + 1, m))
    H[:m, :] = np.triu(rng.standard_normal((m, m))) + 4.0 * np.eye(m)
    H[np.arange(1, m + 1), np.arange(m)] = rng.uniform(0.5, 1.5, m)
    return H, rng.uniform(0.5, 2.0), rng


@pytest.fixture(scope='module')
def hess_cases():
    cases = []
    for m in MS:
        for seed in range(3):
            H, beta, rng = _hessenberg(m, seed)
            cases.append((m, seed, H, beta, np.linalg.cond(H), rng))
    return cases


def test_hessenberg_qr_matches_lstsq(driver, hess_cases):
    """After every pushed column: the returned residual estimate is the least-squares residual norm of the leading problem
    min ||beta e_0 - H[:j+2, :j+1] y||, and y is numpy's solution, both to 100 * cond(H) * eps -- y relative to ||y||, the residual norm
    relative to beta, the norm of the right-hand side (the residual itself falls to 1e-70 * beta over 120 columns, far below what
    ||beta e_0 - H y|| can be evaluated to from any y in doubles).  The free back substitution on a copy with a larger leading dimension
    gives the same y bit for bit."""
    rows = []
    for m, seed, H, beta, kappa, _ in hess_cases:
        rows.append([m, m + 1 + 3, beta] + [H[i, j] for j in range(m) for i in range(j + 2)])
    out = iter(driver('qr', rows))
    worst_kappa = worst_y = worst_r = 0.0
    for m, seed, H, beta, kappa, _ in hess_cases:
        assert kappa <= 1e4, (m, seed, kappa)
        tol = 100 * kappa * EPS
        worst_kappa = max(worst_kappa, kappa)
        with threadpool_limits(limits=1):
            refs = [np.linalg.lstsq(H[:j + 2, :j + 1], beta * np.eye(j + 2)[0], rcond=None)[0] for j in range(m)]
        for j, yref in enumerate(refs):
            same, est, *y = next(out)
            assert same == 1, (m, seed, j)
            assert len(y) == j + 1
            rref = np.linalg.norm(beta * np.eye(j + 2)[0] - H[:j + 2, :j + 1] @ yref)
            ey = np.linalg.norm(np.array(y) - yref) / np.linalg.norm(yref)
            er = abs(est - rref) / beta
            worst_y, worst_r = max(worst_y, ey / EPS), max(worst_r, er / EPS)
            assert ey <= tol, (m, seed, j, ey, tol)
            assert er <= tol, (m, seed, j, er, tol)
    assert next(out, None) is None
    print('largest cond(H) %.3g; largest deviation: y %.1f eps, residual estimate %.1f eps' % (worst_kappa, worst_y, worst_r))


def test_hess_lsq_matches_lstsq(driver, hess_cases):
    """hess_lsq on the leading k <= 4 columns, as the projection on a kept space uses it (k <= 4 kept vectors), with a general right-hand
    side: y and H y against numpy, to the same margin."""
    rows, refs = [], []
    for m, seed, H, beta, kappa, rng in hess_cases:
        for k in range(1, min(m, 4) + 1):
            A = H[:k + 1, :k]
            g = rng.standard_normal(k + 1)
            rows.append([k] + list(A.T.ravel()) + list(g))            # column-major, ld = k + 1
            yref = np.linalg.lstsq(A, g, rcond=None)[0]
            refs.append((k, yref, A @ yref, kappa))
    out = driver('lsq', rows)
    assert len(out) == len(rows)
    for got, (k, yref, Hyref, kappa) in zip(out, refs):
        tol = 100 * kappa * EPS
        y, Hy = np.array(got[:k]), np.array(got[k:])
        assert len(Hy) == k + 1
        assert np.linalg.norm(y - yref) <= tol * np.linalg.norm(yref)
        assert np.linalg.norm(Hy - Hyref) <= tol * np.linalg.norm(Hyref)


# ---- algebraic second projection -------------------------------------------------------------------------------------------------------
KS = [1, 2, 4, 5, 8, 9, 16, 17, 30]
PERTURB = [0.0, 1e-12, 1e-6]


def _basis(k, pert, rng):
    """200 x k: orthonormal columns plus pert * noise; and an orthonormal basis of what they span"""
    Q = np.linalg.qr(rng.standard_normal((200, k)))[0]
    V = Q + pert * rng.standard_normal((200, k))
    return V, np.linalg.qr(V)[0]


def _unit_inside_and_outside(V, Qv, rng):
    a = rng.standard_normal(V.shape[1])
    inside = V @ a
    u = rng.standard_normal(200)
    u -= Qv @ (Qv.T @ u)
    u -= Qv @ (Qv.T @ u)
    return inside / np.linalg.norm(inside), u / np.linalg.norm(u)


def _cgs2_row(V, w, ld):
    d, G, ww = V.T @ w, V.T @ V, float(w @ w)
    return [V.shape[1], ld, ww] + list(d) + list(G.ravel()), (d, G, ww)


def _check_cgs2(V, w, d, G, ww, got):
    """coefficients = d + (I - G) d and hn2 = ||w - V c||^2"""
    k = V.shape[1]
    direct, hn2, *c = got
    c = np.array(c)
    M = np.eye(k) - G
    # two summation orders of k terms differ by at most 2 k eps sum |terms|; the final addition rounds once on either side
    assert np.all(np.abs(c - (d + M @ d)) <= 2 * k * EPS * (np.abs(M) @ np.abs(d)) + 2 * EPS * np.abs(c))
    r = w - V @ c
    err = abs(hn2 - float(r @ r))
    assert err <= 16 * k * EPS * ww, (k, err / (k * EPS * ww))
    return direct, hn2, err / (k * EPS * ww)


def test_cgs2_algebraic_matches_explicit_projection(driver):
    cases, rows = [], []
    for k, pert, share, seed in itertools.product(KS, PERTURB, [0.0, 0.9, 0.999999], range(4)):
        rng = np.random.default_rng([k, seed, int(share * 1e6), int(pert * 1e12)])
        V, Qv = _basis(k, pert, rng)
        inside, outside = _unit_inside_and_outside(V, Qv, rng)
        w = share * inside + np.sqrt(1.0 - share * share) * outside       # unit norm, `share` of it inside span(V)
        row, (d, G, ww) = _cgs2_row(V, w, k + (seed % 2) * 3)            # leading dimension k and larger
        rows.append(row); cases.append((V, w, d, G, ww))
    out = driver('cgs2', rows)
    assert len(out) == len(cases) == 324
    smallest, worst = 1.0, 0.0
    for (V, w, d, G, ww), got in zip(cases, out):
        direct, hn2, err = _check_cgs2(V, w, d, G, ww, got)
        assert direct == 1                                              # hn2 / ww >= ~2e-6: normalise directly
        smallest, worst = min(smallest, hn2 / ww), max(worst, err)
    print('smallest hn2 / ww %.3g; largest error of hn2 %.2f k eps ww' % (smallest, worst))
    assert 1e-6 < smallest < 1e-5


def test_cgs2_algebraic_asks_for_the_second_pass_on_cancellation(driver):
    """w = V a + 1e-5 * (unit vector orthogonal to V), ||V a|| = 1: hn2 / ww ~ 1e-10, two decades below the 1e-8 threshold, and the error
    of hn2 (<= 16 k eps ww ~ 1e-13 ww) is five decades below the threshold on either side: the verdict does not depend on rounding"""
    cases, rows = [], []
    for k, pert, seed in itertools.product(KS, PERTURB, range(2)):
        rng = np.random.default_rng([k, seed, int(pert * 1e12), 7])
        V, Qv = _basis(k, pert, rng)
        inside, outside = _unit_inside_and_outside(V, Qv, rng)
        w = inside + 1e-5 * outside
        row, (d, G, ww) = _cgs2_row(V, w, k + 1)
        rows.append(row); cases.append((V, w, d, G, ww))
    out = driver('cgs2', rows)
    assert len(out) == len(cases)
    for (V, w, d, G, ww), got in zip(cases, out):
        direct, hn2, _ = _check_cgs2(V, w, d, G, ww, got)
        assert direct == 0
        assert 0.5e-10 < hn2 / ww < 2e-10


# ---- recycling rules -------------------------------------------------------------------------------------------------------------------
SEL = {1: (0,), 2: (0,), 3: (0, 2)}          # stage -> the earlier stages whose space it projects on by default


def uses(stage, q, rec_mode, rec_full):
    return 0 <= stage <= 3 and (rec_mode == 2 or rec_full or q in SEL.get(stage, ()))


def decide(pcmode, stage, rec_mode, rec_mg, use_frozen, restart_alloc, rec_vtop):
    """gmres(): recycle within a step (stage 0..3) on frozen coefficients; under the V cycle (pcmode 1) only when whole cycles are kept
    (rec_mg); stage 0, no recycling or less than 6 (16) free basis slots drop what is kept, and only stage 0 then goes on recycling"""
    in_step = 0 <= stage < 4 and use_frozen and rec_mode > 0
    full = pcmode == 1 and rec_mg and in_step
    on = in_step and (pcmode != 1 or full)
    reset = (not on) or stage == 0 or restart_alloc - rec_vtop < (16 if full else 6)
    if reset and stage != 0:
        on = False
    return [int(on), int(full), int(reset)]


def test_recycling_rules(driver):
    rows = []
    for stage, q, rec_mode, pcmode, rec_mg, frozen, ralloc in itertools.product(range(-1, 5), range(4), (0, 1, 2), range(4), (0, 1), (0, 1), (8, 30, 120)):
        for vtop in (0, 3, ralloc - 5, ralloc - 16):
            rows.append([stage, q, rec_mode, pcmode, rec_mg, frozen, ralloc, vtop])
    out = driver('recycle', rows)
    assert len(out) == len(rows)
    seen = set()
    for row, got in zip(rows, out):
        stage, q, rec_mode, pcmode, rec_mg, frozen, ralloc, vtop = row
        want = decide(pcmode, stage, rec_mode, rec_mg, frozen, ralloc, vtop) + [int(uses(stage, q, rec_mode, False)), int(uses(stage, q, rec_mode, True))]
        assert got == want, (row, got, want)
        seen.add(tuple(want[:3]))
    # every outcome occurs: off (reset), on and fresh (stage 0), on behind kept spaces, the same two with whole cycles
    assert seen == {(0, 0, 1), (1, 0, 1), (1, 0, 0), (1, 1, 1), (1, 1, 0), (0, 1, 1)}


# ---- Chebyshev polynomial preconditioner ------------------------------------------------------------------------------------------------
CHEB_CASES = list(itertools.product([0.5, 1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4], [0.1, 1.0, 2.3, 115.0], [1, 3, 6, 7]))
CHEB_TARGET = 0.02
# 1 - shift l p(l) against numpy's T_n(mu(l)) / T_n(mu(0)): the recurrence restated in Python is within 8.5e-11 of numpy on exactly this grid
# (cancellation between monomial terms at the large-kappa end); the margin covers a different summation order
CHEB_TOL = 1e-9


def cheb_degree(lamJ, shift, target, max_deg):
    """the degree rule restated: (a, b, kappa, degree), degree 0 = do not precondition"""
    a, b = 0.97, 1.0 + 1.15 * lamJ / shift
    kappa = b / a
    if kappa < 1.3:
        return a, b, kappa, 0
    rc = (np.sqrt(kappa) - 1.0) / (np.sqrt(kappa) + 1.0)
    d = int(np.ceil(np.log(target) / np.log(rc))) - 1
    return a, b, kappa, min(max(d, 1), max(max_deg, 1))


def test_chebyshev_coefficients_match_numpy(driver):
    out = driver('cheb', [[lamJ, shift, CHEB_TARGET, md] for lamJ, shift, md in CHEB_CASES])
    assert len(out) == len(CHEB_CASES)
    degrees, worst, worst_over = set(), 0.0, 0.0
    for (lamJ, shift, md), (d, *alpha) in zip(CHEB_CASES, out):
        a, b, kappa, want = cheb_degree(lamJ, shift, CHEB_TARGET, md)
        assert d == want, (lamJ, shift, md, d, want)
        assert (d == 0) == (kappa < 1.3)
        degrees.add(int(d))
        if d == 0:
            assert alpha == [0.0] * 8
            continue
        d = int(d)
        assert all(x == 0.0 for x in alpha[d + 1:])
        n = d + 1
        m0, m1 = (b + a) / (b - a), -2.0 / (b - a)
        ls = np.linspace(a, b, 65)
        p = sum(alpha[i] * ls ** i for i in range(d + 1))
        r = 1.0 - shift * ls * p
        Tn = np.zeros(n + 1); Tn[n] = 1.0
        t0 = np.polynomial.chebyshev.chebval(m0, Tn)
        ref = np.polynomial.chebyshev.chebval(m0 + m1 * ls, Tn) / t0
        err = float(np.max(np.abs(r - ref)))
        worst = max(worst, err)
        assert err <= CHEB_TOL, (lamJ, shift, md, d, err)
        over = float(np.max(np.abs(r))) - 1.0 / abs(t0)             # equioscillation: |r| <= 1 / |T_n(mu(0))| on [a, b]
        worst_over = max(worst_over, over)
        assert over <= CHEB_TOL, (lamJ, shift, md, d, over)
    print('degrees %s; largest deviation from numpy %.2e, largest excess over 1/|T_n(mu(0))| %.2e' % (sorted(degrees), worst, worst_over))
    assert {0, 1, 3, 6, 7} <= degrees          # no preconditioner, and each max_deg active as the clamp


# ---- cycle length and basis size -------------------------------------------------------------------------------------------------------
def test_cycle_rules(driver):
    rows = []
    for ralloc, vb, ksp_restart, (rec_on, rec_full), grow, reserved, k in itertools.product(
            (8, 30, 120), (0, 5), (0, 8, 30, 64, 200), [(0, 0), (1, 0), (1, 1), (0, 1)], (0, 1), (0, 1, 2), (1, 30, 31, 64)):
        m_opt = min(ksp_restart if ksp_restart > 0 else 30, ralloc)
        for m_cur in (m_opt, 2 * m_opt):
            for rn, bn, tol_abs, rtol in [(1e-7, 2.0, -1.0, 1e-6), (1e-7, 2.0, 3e-6, 1e-6), (1e-7, 2.0, 3e-6, 0.0)]:
                rows.append([ralloc, vb, m_opt, rec_on, rec_full, m_cur, grow, reserved, k, ksp_restart, 32, rn, bn, tol_abs, rtol])
    out = driver('cycle', rows)
    assert len(out) == len(rows)
    seen = set()
    for (ralloc, vb, m_opt, rec_on, rec_full, m_cur, grow, reserved, k, ksp_restart, maxk, rn, bn, tol_abs, rtol), got in zip(rows, out):
        room = ralloc - vb
        first = room if (rec_full and rec_on) else min(m_opt, room)              # whole cycles kept: the whole room
        nxt = min(2 * m_cur, room) if grow else m_cur                            # doubling, capped at the room; growth off
        classic = int(bool(reserved & 1) or k > 30)
        pipelined = min(ksp_restart if ksp_restart > 0 else 30, ralloc, maxk)    # clamp of the pipelined solver
        rel = rn / (tol_abs / rtol if (tol_abs > 0.0 and rtol > 0.0) else bn)
        assert got == [room, first, nxt, classic, pipelined, rel], (ralloc, vb, m_opt, rec_on, rec_full, m_cur, grow, reserved, k, ksp_restart, got)
        seen |= {('full', first == room and first > m_opt), ('capped', bool(grow) and nxt == room < 2 * m_cur), ('clamp', pipelined == 32 < ksp_restart)}
    assert {('full', True), ('capped', True), ('clamp', True)} <= seen
    # the two sides of the classical threshold, and the request bit
    pick = lambda reserved, k: driver('cycle', [[30, 0, 30, 0, 0, 30, 1, reserved, k, 30, 32, 1.0, 1.0, -1.0, 1e-6]])[0][3]
    assert (pick(0, 30), pick(0, 31), pick(1, 1), pick(2, 30)) == (0, 1, 1, 0)


def fit_rule(mfree, vecbytes, cap):
    room = 0.92 * mfree / vecbytes - 30.0
    fit_room = int(np.floor(min((room - 1.0) / 2.0, 1.0e6)))
    fit_40 = int(np.floor(min(0.4 * mfree / vecbytes / 2.0, 1.0e6)))
    return max(min(cap, fit_room, fit_40), min(30, fit_room))


def test_basis_size_from_free_memory(driver):
    vecbytes = 8.0 * 4096 * 4096 * 2
    # free memory in vectors -> what fits, by hand: below the floor of 8; between 8 and 30 (what fits behind the 30 other vectors);
    # the 40 % bound; the cap of 120; a cap from the environment (it bounds only what goes beyond the default 30)
    by_hand = [(40.0, -1, 2), (56.0, -1, 10), (80.0, -1, 21), (97.5, -1, 29), (300.0, -1, 60), (1000.0, -1, 120), (1e9, -1, 120),
               (1000.0, 64, 64), (300.0, 64, 60), (1000.0, 8, 30), (80.0, 8, 21), (50.0, 8, 7), (1000.0, 4, 30), (1000.0, 500, 120)]
    rows = [[nv * vecbytes, vecbytes, env] for nv, env, _ in by_hand]
    grid = [[nv * vecbytes, vecbytes, env] for nv in np.linspace(31.3, 700.7, 97) for env in (-1, 8, 40, 120)]
    out = driver('fit', rows + grid)
    assert out.pop() == [30, 120, 8]
    for (mfree, vb, env), (cap, fit), want in zip(rows, out, [w for _, _, w in by_hand]):
        assert cap == (120 if env < 0 else max(8, min(env, 120)))
        assert fit == want == fit_rule(mfree, vb, int(cap)), (mfree / vb, env, fit, want)
    for (mfree, vb, env), (cap, fit) in zip(grid, out[len(rows):]):
        assert fit == fit_rule(mfree, vb, int(cap)), (mfree / vb, env, fit)
