"""GPU: the banded direct stage solver for 1-D grids (pc_type 6): device assembly of shift*I - J into band storage in the folded unknown
order, LU with partial pivoting inside the band by one workgroup, the two sweeps of a solve, the Rosenbrock step on it, and its guards.
Every test fails without the solver: without it ksfd_banded_apply does not exist and pc_type 6 runs plain GMRES (pc_used 1)."""
import numpy as np
import pytest

from conftest import load_golden, rel_l2
from ksfd_amd.config import ProblemConfig
from ksfd_amd.layout import PETSC, cijk_to_soa
from ksfd_amd import lib as klib
from oracle import ko
from test_gpu_direct import DIRECT_TOL, GAMMA, _cfg, _dense_A, _indefinite_case, _state

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _banded_opts(**kw):
    return klib.default_step_opts(pc_type=6, **kw)


def _varying_state(cfg, seed):
    """rho over two decades (about 135 ... 27000) along the ring, the ligands near their local equilibrium"""
    rng = np.random.default_rng(seed)
    x = np.arange(cfg.N) / cfg.N
    rho = 1900.0 * 10 ** (1.15 * np.sin(2 * np.pi * (2 * x + rng.uniform())) + 0.005 * rng.standard_normal(cfg.N))
    return np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] * (1 + 0.05 * rng.standard_normal(cfg.N)) for l in range(cfg.nlig)])


def _fold(N, F):
    """band unknown of every unknown of the reference's Vec order (F*point + dof): F*pos(point) + dof, pos = 0, N-1, 1, N-2, ..."""
    p = np.arange(N)
    pos = np.where(p < (N + 1) // 2, 2 * p, 2 * (N - 1 - p) + 1)
    return (F * pos[:, None] + np.arange(F)[None, :]).ravel()


def _band_of(Af, k):
    """LAPACK band array (solve_banded's ab) of a matrix with half-bandwidths k; everything outside the band must be zero"""
    n = Af.shape[0]
    i, j = np.nonzero(Af)
    assert np.abs(i - j).max() <= k
    ab = np.zeros((2 * k + 1, n))
    ab[k + i - j, j] = Af[i, j]
    return ab


# ---- 1. ksfd_banded_apply against numpy and LAPACK's banded solver ---------------------------------------------------------------
APPLY_CASES = [(5, 1), (6, 1), (7, 2), (8, 2), (9, 2), (24, 1), (166, 1), (256, 2), (683, 2), (69, 5), (21, 12)]


@pytest.mark.parametrize('state', ['uniform', 'varying'])
@pytest.mark.parametrize('N,nlig', APPLY_CASES)
def test_banded_apply_against_numpy(N, nlig, state):
    """shifts from far above the spectrum of J (10 rho(J)) over 1/(gamma h) of a moderate step to one inside it (at least a tenth of the
    eigenvalues on either side).  Relative residual <= max(1e-13, 10 x the residual scipy.linalg.solve_banded -- the same algorithm in
    LAPACK -- leaves on the same folded matrix and right-hand side; the 10 for another summation order in the rank-1 updates); distance to
    numpy.linalg.solve <= 100 eps cond(A); PETSC and SoA entries bit-equal; agreement with the dense solver to 100 eps cond(A)."""
    from scipy.linalg import solve_banded
    cfg = _cfg(1, (N,), nlig, seed=7 + N)
    u = _state(cfg, 3, amp=0.05) if state == 'uniform' else _varying_state(cfg, 3)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    A0, _ = _dense_A(k, 0.0)
    n, F = A0.shape[0], cfg.F
    q = _fold(N, F)
    kb = min(5 * F - 1, n - 1)
    lam = np.linalg.eigvals(-A0)                            # spectrum of J
    R = float(np.abs(lam).max())
    lr = np.sort(lam.real)
    i0, i1 = len(lr) // 10, max(len(lr) // 10 + 1, 9 * len(lr) // 10)
    g = i0 + int(np.argmax(np.diff(lr[i0:i1 + 1])))
    inside = 0.5 * (lr[g] + lr[g + 1])
    assert (lam.real > inside).sum() >= len(lr) // 10 and (lam.real < inside).sum() >= len(lr) // 10
    rng = np.random.default_rng(5)
    soa = lambda a: a.reshape(-1, F).T.ravel()
    for shift in (10.0 * R, 1.0 / (GAMMA * 0.05), inside):
        A = A0 + shift * np.eye(n)
        b = rng.standard_normal(n)
        Af = np.zeros_like(A)
        Af[np.ix_(q, q)] = A
        bf = np.zeros(n)
        bf[q] = b
        xs = solve_banded((kb, kb), _band_of(Af, kb), bf)
        res_lapack = np.linalg.norm(bf - Af @ xs) / np.linalg.norm(b)
        z = k.banded_apply(shift, b, layout=PETSC)
        res = np.linalg.norm(b - A @ z) / np.linalg.norm(b)
        cond = np.linalg.cond(A)
        print('N %d nlig %d %s shift %.3e: residual %.2e (LAPACK %.2e), distance %.2e, cond %.2e' % (N, nlig, state, shift, res, res_lapack, rel_l2(z, np.linalg.solve(A, b)), cond))
        assert res <= max(1e-13, 10.0 * res_lapack), (shift, res, res_lapack)
        assert rel_l2(z, np.linalg.solve(A, b)) <= 100 * EPS * cond, (shift, cond)
        assert np.array_equal(k.banded_apply(shift, soa(b)), soa(z))
        assert rel_l2(z, k.direct_apply(shift, b, layout=PETSC)) <= 100 * EPS * cond, (shift, cond)
    k.close()


# ---- 2. goldens (reference operators + exact sparse LU) with pc_type 6 -----------------------------------------------------------
def _fixed(z):
    return _banded_opts(adapt=0, atol=float(z['atol']), rtol=float(z['rtol']), ksp_rtol=1e-12)


def test_banded_fixed_steps_vs_reference_lu_golden():
    z = load_golden('step_1d_n1')
    k = klib.KSFDHip(ProblemConfig.from_golden(z))
    k.set_state(cijk_to_soa(z['u0']))
    t, h = float(z['t0']), float(z['h'])
    for s in range(int(z['nsteps'])):
        t, hn, st, rc = k.step(t, h, _fixed(z))
        assert st.accepted and st.pc_used == klib.PC_BANDED and st.linear_its == 4 and st.residual_evals == 4
        assert abs(st.wrms - z['wrms'][s]) <= 1e-6 * z['wrms'][s] + 1e-12
        if s == 0:
            assert rel_l2(k.get_state(), cijk_to_soa(z['u1'])) < DIRECT_TOL
    assert rel_l2(k.get_state(), cijk_to_soa(z['uN'])) < DIRECT_TOL
    k.close()


def test_banded_manufactured_per_stage_sources_vs_golden():
    z = load_golden('step_1d_manufactured')
    cfg = ProblemConfig.from_golden(z)
    k = klib.KSFDHip(cfg)
    k.set_state(cijk_to_soa(z['u0']))
    t, h = 0.0, float(z['h'])
    for s in range(int(z['nsteps'])):
        for i in range(4):
            sv = z['src_v'][4 * s + i]
            for c in range(cfg.F):
                k.set_source(c, sv[c] if np.any(sv[c]) else None, stage=i)
        t, hn, st, rc = k.step(t, h, _fixed(z))
        assert st.pc_used == klib.PC_BANDED and st.linear_its == 4 and st.residual_evals == 4
    u = k.get_state()
    assert rel_l2(u, cijk_to_soa(z['uN'])) < DIRECT_TOL
    assert np.abs(u - cijk_to_soa(z['exactN'])).max() < 2e-6
    k.close()


# ---- 3. the oracle's LU at the library default ksp_rtol --------------------------------------------------------------------------
@pytest.mark.parametrize('h', [0.1, 5.0])
@pytest.mark.parametrize('shape,nlig,L', [((24,), 1, (0.05,)), ((256,), 1, (0.4,)), ((384,), 2, (0.6,))])
def test_banded_step_vs_oracle_lu_at_default_ksp_rtol(shape, nlig, L, h):
    cfg = ProblemConfig.standard(1, shape, L=L, nlig=nlig)
    rng = np.random.default_rng(11)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)
    u = np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(nlig)])
    un, err, wr, _ = ko.Oracle(cfg).rosw_step(u, h, 0.01, 1e-6, solver='lu')
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    t, hn, st, rc = k.step(0.0, h, _banded_opts(adapt=0, atol=0.01, rtol=1e-6))
    print('%s nlig %d h %g: state %.2e wrms %.2e' % (shape, nlig, h, rel_l2(k.get_state(), un), abs(st.wrms - wr) / wr))
    assert st.pc_used == klib.PC_BANDED and st.linear_its == 4 and st.residual_evals == 4
    assert rel_l2(k.get_state(), un) <= 1e-12
    assert abs(st.wrms - wr) <= 1e-9 * wr
    k.close()


# ---- 4. adaptive run: the same run as the dense solver ---------------------------------------------------------------------------
def _adaptive_start():
    cfg = ProblemConfig.standard(1, (256,), L=(0.4,), nlig=1)
    rng = np.random.default_rng(11)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)
    return cfg, np.concatenate([rho, rho * cfg.lig_s[0] / cfg.lig_gamma[0]])


def test_banded_adaptive_run_matches_the_dense_solver():
    cfg, u = _adaptive_start()
    runs = []
    for pc in (6, 5):
        k = klib.KSFDHip(cfg)
        k.set_state(u)
        opts = klib.default_step_opts(pc_type=pc, adapt=1, atol=0.01, rtol=1e-6)
        t, h, log = 0.0, 1e-3, []
        for _ in range(12):
            t, h, st, rc = k.step(t, h, opts)
            assert st.accepted and st.pc_used == (klib.PC_BANDED if pc == 6 else klib.PC_DIRECT)
            assert st.linear_its == 4 * (1 + st.rejections)
            log.append((st.rejections, st.h_used, h))
        runs.append((log, k.get_state()))
        k.close()
    (lb, ub), (ld, ud) = runs
    assert [r[0] for r in lb] == [r[0] for r in ld]
    assert all(abs(a[1] - b[1]) <= 1e-9 * b[1] and abs(a[2] - b[2]) <= 1e-9 * b[2] for a, b in zip(lb, ld))
    assert rel_l2(ub, ud) <= 1e-11


def test_banded_planted_rejection_refactors_every_attempt():
    cfg, u = _adaptive_start()
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    t, h, st, rc = k.step(0.0, 0.1, _banded_opts(adapt=1, atol=0.01, rtol=1e-6))     # the error norm of this first attempt is in the hundreds
    assert st.accepted and st.rejections >= 1 and st.pc_used == klib.PC_BANDED
    assert st.linear_its == 4 * (1 + st.rejections) and st.residual_evals == st.linear_its
    k.close()


# ---- 5. the 1-D cases of the indefinite sweep ------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [114, 115, 127])
def test_banded_random_problem_indefinite_step_vs_oracle(seed):
    """test_gpu_direct's construction and bound (max(1e-8, 1e-12 cond), reasoning there), no exception list"""
    cfg, u, h, cond = _indefinite_case(seed - 100)
    assert cfg.dim == 1
    un, err, wr, _ = ko.Oracle(cfg).rosw_step(u, h, 0.01, 1e-6, solver='lu')
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    t, hn, st, rc = k.step(0.0, h, _banded_opts(adapt=0, atol=0.01, rtol=1e-6), raise_on_error=False)
    state = k.get_state()
    msg = k.last_error()
    k.close()
    print('seed %d n %s nlig %d h %.3e cond %.2e: %.2e' % (seed, cfg.n, cfg.nlig, h, cond, rel_l2(state, un)))
    assert rc == 0 and st.pc_used == klib.PC_BANDED, (seed, rc, msg, cfg.n, cfg.nlig, h, cond)
    assert rel_l2(state, un) <= max(1e-8, 1e-12 * cond), (seed, rel_l2(state, un), cond, cfg.n, cfg.nlig, h, st.linear_its)


# ---- 6. guards --------------------------------------------------------------------------------------------------------------------
def test_banded_refuses_a_2d_handle_and_leaves_everything_untouched():
    cfg = ProblemConfig.standard(2, (32, 24), L=(0.2, 0.15))
    u = _state(cfg, 2)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    before = k.get_state()
    t, hn, st, rc = k.step(0.5, 0.05, _banded_opts(adapt=0, atol=0.01, rtol=1e-6), raise_on_error=False)
    assert rc == klib.EINVAL and t == 0.5 and hn == 0.05
    assert 'pc_type 2' in k.last_error() and 'pc_type 5' in k.last_error()
    with pytest.raises(klib.KSFDError) as e:
        k.banded_apply(100.0, u)
    assert e.value.code == klib.EINVAL and 'pc_type 2' in k.last_error() and 'pc_type 5' in k.last_error()
    assert np.array_equal(k.get_state(), before)
    # the same handle still steps with the default solver
    t, hn, st, rc = k.step(0.0, 0.05, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12))
    un, _, wr, _ = ko.Oracle(cfg).rosw_step(u, 0.05, 0.01, 1e-6, solver='lu')
    assert st.pc_used & klib.PC_BANDED == 0 and rel_l2(k.get_state(), un) < 1e-10
    k.close()


def test_banded_apply_rejects_a_non_finite_shift():
    cfg = ProblemConfig.standard(1, (24,), L=(0.05,))
    u = _state(cfg, 2)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    for bad in (float('nan'), float('inf')):
        with pytest.raises(klib.KSFDError) as e:
            k.banded_apply(bad, u)
        assert e.value.code == klib.EINVAL
    assert np.array_equal(k.get_state(), u)
    assert np.isfinite(k.banded_apply(100.0, u)).all()
    k.close()


def test_banded_handle_goes_on_with_the_other_solvers_and_replays_after_restore():
    cfg = ProblemConfig.standard(1, (64,), L=(0.1,), nlig=2)
    u = _state(cfg, 5)
    o = ko.Oracle(cfg)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    ref = u
    for pc, bit in ((6, klib.PC_BANDED), (2, None), (5, klib.PC_DIRECT), (6, klib.PC_BANDED)):
        t, hn, st, rc = k.step(0.0, 0.05, klib.default_step_opts(pc_type=pc, adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12))
        ref = o.rosw_step(ref, 0.05, 0.01, 1e-6, solver='lu')[0]
        assert (st.pc_used == bit) if bit else (st.pc_used & (klib.PC_BANDED | klib.PC_DIRECT) == 0)
        assert rel_l2(k.get_state(), ref) < 1e-10, pc
    # checkpoint, pc_type 6 steps, restore, the same steps again: bitwise
    opts = _banded_opts(adapt=1, atol=0.01, rtol=1e-6)
    k.checkpoint()

    def run():
        t, h, out = 0.0, 1e-3, []
        for _ in range(3):
            t, h, st, rc = k.step(t, h, opts)
            out.append((t, h, st.rejections, st.linear_its))
        return out, k.get_state()
    a, ua = run()
    k.restore()
    b, ub = run()
    assert a == b and np.array_equal(ua, ub)
    k.close()


# ---- 7. one larger grid: beyond what the dense solver takes ----------------------------------------------------------------------
def test_banded_apply_49152_unknowns_against_lapack():
    """16384 points x 3 fields > KSFD_DIRECT_MAX: one solve against scipy.linalg.solve_banded on the folded matrix; cond(A) in the 1-norm
    from scipy's sparse LU and onenormest"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    from scipy.linalg import solve_banded
    N, nlig = 16384, 2
    cfg = ProblemConfig.standard(1, (N,), L=(25.6,), nlig=nlig)
    F = cfg.F
    assert F * N > klib.DIRECT_MAX
    k = klib.KSFDHip(cfg)
    k.set_state(_state(cfg, 1))
    rp, col, val = k.jacobian_csr()
    n = rp.size - 1
    shift = 1.0 / (GAMMA * 0.05)
    A = (shift * sp.identity(n, format='csr') - sp.csr_matrix((val, col, rp), shape=(n, n))).tocsr()
    b = np.random.default_rng(9).standard_normal(n)
    z = k.banded_apply(shift, b, layout=PETSC)
    k.close()
    q = _fold(N, F)
    C = A.tocoo()
    kb = 5 * F - 1
    i, j = q[C.row], q[C.col]
    assert np.abs(i - j).max() <= kb
    ab = np.zeros((2 * kb + 1, n))
    np.add.at(ab, (kb + i - j, j), C.data)
    bf = np.zeros(n)
    bf[q] = b
    xs = solve_banded((kb, kb), ab, bf)
    ref = xs[q]
    res_lapack = np.linalg.norm(b - A @ ref) / np.linalg.norm(b)
    res = np.linalg.norm(b - A @ z) / np.linalg.norm(b)
    lu = spl.splu(A.tocsc())
    inv = spl.LinearOperator((n, n), matvec=lu.solve, rmatvec=lambda v: lu.solve(v, 'T'))
    cond = spl.onenormest(A) * spl.onenormest(inv)
    print('49152 unknowns: residual %.2e (LAPACK %.2e), distance %.2e, cond1 %.2e' % (res, res_lapack, rel_l2(z, ref), cond))
    assert res <= max(1e-13, 10.0 * res_lapack)
    assert rel_l2(z, ref) <= 100 * EPS * cond


# ---- 8. the front end: -ksfd_pc_type banded on a 1-D options file ----------------------------------------------------------------
def test_solver_main_runs_a_1d_options_file_with_the_banded_solver(tmp_path):
    import os
    from conftest import GOLDEN
    from ksfd_amd import solver
    ts = solver.main('ksfd', '@' + os.path.join(GOLDEN, 'options', 'ks1d_manufactured.txt'), '--save=' + str(tmp_path / 'run'),
                     '--petsc', '-ksfd_pc_type', 'banded', '--')
    # dt = 1, -ts_adapt_type none, tmax = 20: the loop runs while t <= tmax, so the run ends with step 21 at t = 21
    assert ts.opts.pc_type == 6 and ts.getSNESFailures() == 0
    assert abs(ts.getTime() - 21.0) < 1e-9 and len(ts.stats_log) == 21
    assert ts.last_stats.pc_used == klib.PC_BANDED and all(s[0] == 1 and s[2] == 4 for s in ts.stats_log)      # every step accepted on 4 solves
    ts.cleanup()
