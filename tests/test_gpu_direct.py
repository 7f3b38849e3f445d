"""GPU: the dense direct stage solver (pc_type 5): device assembly of shift*I - J, LU with partial pivoting, triangular solves,
the Rosenbrock step on it, and its guards.  Every test fails without the solver: without it pc_type 5 runs plain GMRES (pc_used
would be 1, not PC_DIRECT) and ksfd_direct_apply does not exist."""
import numpy as np
import pytest

from conftest import golden_cases, load_golden, rel_l2
from ksfd_amd.config import ProblemConfig
from ksfd_amd.layout import PETSC, cijk_to_soa
from ksfd_amd import lib as klib
from oracle import ko
from test_gpu_random_sweep import random_problem

pytestmark = pytest.mark.gpu
GAMMA = 0.43586652150845900
DIRECT_TOL = 1e-11      # rel-L2 of the state against the goldens (GMRES suite: 1e-10)


def _cfg(dim, shape, nlig, seed, L=None):
    rng = np.random.default_rng(seed)
    ngroups = min(nlig, 2)
    return ProblemConfig(dim=dim, n=shape, L=L or tuple(float(x) for x in rng.uniform(0.1, 0.6, size=dim)),
                         lig_group=np.arange(nlig, dtype=np.int32) % ngroups, lig_w=rng.uniform(0.5, 1.5, size=nlig),
                         lig_s=10 ** rng.uniform(-3, -1.5, size=nlig), lig_gamma=10 ** rng.uniform(-3, -1.5, size=nlig),
                         lig_D=10 ** rng.uniform(-6.5, -4.5, size=nlig), grp_alpha=rng.uniform(500, 3000, size=ngroups),
                         grp_beta=np.array([5.56e-4, -5.56e-4][:ngroups]))


def _state(cfg, seed, level=9000.0, amp=0.01):
    rng = np.random.default_rng(seed)
    rho = level * (1.0 + amp * rng.standard_normal(cfg.N))
    return np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(cfg.nlig)])


def _dense_A(k, shift):
    """shift*I - J in the reference's Vec order (F*point + dof) from the exported CSR"""
    rp, col, val = k.jacobian_csr()
    n = rp.size - 1
    J = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    np.add.at(J, (rows, col), val)
    return shift * np.eye(n) - J, (rp, col, val)


def _direct_opts(**kw):
    return klib.default_step_opts(pc_type=5, **kw)


# ---- 1. ksfd_direct_apply against numpy ------------------------------------------------------------------------------------------
APPLY_CASES = [(1, (24,), 1), (1, (256,), 1), (3, (7, 5, 7), 2), (2, (25, 21), 3), (1, (683,), 2)]


@pytest.mark.parametrize('dim,shape,nlig', APPLY_CASES)
def test_direct_apply_against_numpy(dim, shape, nlig):
    """shifts from far above the spectrum of J (10 rho(J)) over 1/(gamma h) of a moderate step to one inside it (shift*I - J indefinite,
    at least a tenth of the eigenvalues on either side); relative residual <= 1e-13 and the distance to numpy.linalg.solve
    <= 100 eps cond(A)"""
    cfg = _cfg(dim, shape, nlig, seed=7 + sum(shape))
    u = _state(cfg, 3, amp=0.05)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    A0, (rp, col, val) = _dense_A(k, 0.0)
    n, F, npts = A0.shape[0], cfg.F, 4 * dim + 1
    # one-rank CSR numbering = the SoA point index: entry dof*npts of point p's rho row is the centre column F*p + dof
    per = F * npts + cfg.nlig * (npts + 1)
    p = np.arange(cfg.N)
    for dof in range(F):
        assert np.array_equal(col[p * per + dof * npts], F * p + dof)
    lam = np.linalg.eigvals(-A0)                            # spectrum of J
    R = float(np.abs(lam).max())
    # inside: the middle of the widest gap between the real parts of the central 80 % of the spectrum
    lr = np.sort(lam.real)
    i0, i1 = len(lr) // 10, max(len(lr) // 10 + 1, 9 * len(lr) // 10)
    g = i0 + int(np.argmax(np.diff(lr[i0:i1 + 1])))
    inside = 0.5 * (lr[g] + lr[g + 1])
    assert (lam.real > inside).sum() >= len(lr) // 10 and (lam.real < inside).sum() >= len(lr) // 10
    rng = np.random.default_rng(5)
    for shift in (10.0 * R, 1.0 / (GAMMA * 0.05), inside):
        A = A0 + shift * np.eye(n)
        b = rng.standard_normal(n)
        z = k.direct_apply(shift, b, layout=PETSC)
        res = np.linalg.norm(b - A @ z) / np.linalg.norm(b)
        assert res <= 1e-13, (shift, res)
        ref = np.linalg.solve(A, b)
        cond = np.linalg.cond(A)
        assert rel_l2(z, ref) <= 100 * np.finfo(float).eps * cond, (shift, rel_l2(z, ref), cond)
        # the SoA entry gives the same answer (layout transform only)
        soa = lambda a: a.reshape(-1, cfg.F).T.ravel()
        assert np.array_equal(k.direct_apply(shift, soa(b)), soa(z))
    k.close()


def test_direct_apply_32768_unknowns_against_splu():
    """128 x 128 x 2 fields = KSFD_DIRECT_MAX unknowns (8.6 GB of factors) against scipy's sparse LU"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    cfg = ProblemConfig.standard(2, (128, 128), L=(0.4, 0.4))
    assert cfg.F * cfg.N == klib.DIRECT_MAX
    k = klib.KSFDHip(cfg)
    k.set_state(_state(cfg, 1))
    rp, col, val = k.jacobian_csr()
    n = rp.size - 1
    shift = 1.0 / (GAMMA * 0.05)
    A = (shift * sp.identity(n, format='csc') - sp.csr_matrix((val, col, rp), shape=(n, n)).tocsc()).tocsc()
    b = np.random.default_rng(9).standard_normal(n)
    z = k.direct_apply(shift, b, layout=PETSC)
    ref = spl.splu(A).solve(b)
    assert np.linalg.norm(b - A @ z) / np.linalg.norm(b) <= 1e-13
    assert rel_l2(z, ref) <= 1e-12
    k.close()


# ---- 2. goldens (reference operators + exact sparse LU) with pc_type 5 -----------------------------------------------------------
def _fixed(z, **kw):
    return _direct_opts(adapt=0, atol=float(z['atol']), rtol=float(z['rtol']), ksp_rtol=1e-12, **kw)


@pytest.mark.parametrize('name', [n for n in golden_cases('step_') if 'manufactured' not in n and 'tdep' not in n])
def test_direct_fixed_steps_vs_reference_lu_golden(name):
    z = load_golden(name)
    k = klib.KSFDHip(ProblemConfig.from_golden(z))
    k.set_state(cijk_to_soa(z['u0']))
    t, h = float(z['t0']), float(z['h'])
    for s in range(int(z['nsteps'])):
        t, hn, st, rc = k.step(t, h, _fixed(z))
        assert st.accepted and st.pc_used == klib.PC_DIRECT and st.linear_its == 4 and st.residual_evals == 4
        assert abs(st.wrms - z['wrms'][s]) <= 1e-6 * z['wrms'][s] + 1e-12
        if s == 0:
            assert rel_l2(k.get_state(), cijk_to_soa(z['u1'])) < DIRECT_TOL
    assert rel_l2(k.get_state(), cijk_to_soa(z['uN'])) < DIRECT_TOL
    k.close()


def test_direct_manufactured_per_stage_sources_vs_golden():
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
        assert st.pc_used == klib.PC_DIRECT and st.linear_its == 4
    u = k.get_state()
    assert rel_l2(u, cijk_to_soa(z['uN'])) < DIRECT_TOL
    assert np.abs(u - cijk_to_soa(z['exactN'])).max() < 2e-6
    k.close()


def test_direct_stage_time_parameters_vs_golden():
    """ksfd_update_params at every step start (the Jacobian's table) and ksfd_set_stage_params (the stage RHS tables); with
    TUNE_RECOMPUTE_JVP (use_frozen off) as well: the factorization takes its coefficient planes through ensure_coef either way"""
    from test_gpu_ts import _tdep_cfg
    z = load_golden('step_2d_n1_tdep')
    for tuning in (klib.TUNE_FUSED, klib.TUNE_FUSED | klib.TUNE_RECOMPUTE_JVP):
        k = klib.KSFDHip(_tdep_cfg(z, 0, 0))
        k.set_tuning(use_fused=tuning)
        k.set_state(cijk_to_soa(z['u0']))
        t, h = float(z['t0']), float(z['h'])
        for s in range(int(z['nsteps'])):
            k.update_params(_tdep_cfg(z, s, 0))
            for i in range(4):
                k.set_stage_params(i, _tdep_cfg(z, s, i + 1))
            t, hn, st, rc = k.step(t, h, _fixed(z))
            assert st.pc_used == klib.PC_DIRECT and st.linear_its == 4
            assert abs(st.wrms - z['wrms'][s]) <= 1e-6 * z['wrms'][s]
        assert rel_l2(k.get_state(), cijk_to_soa(z['uN'])) < DIRECT_TOL, tuning
        k.close()


@pytest.mark.parametrize('name', golden_cases('adapt_'))
def test_direct_adaptive_sequence_vs_golden(name):
    """the accept/reject sequence of the golden; every attempt refactors (a rejection changes h), 4 solves per attempt"""
    z = load_golden(name)
    k = klib.KSFDHip(ProblemConfig.from_golden(z))
    k.set_state(cijk_to_soa(z['u0']))
    opts = _direct_opts(adapt=1, atol=float(z['atol']), rtol=float(z['rtol']), ksp_rtol=1e-12)
    t, h = 0.0, float(z['dt0'])
    for s in range(int(z['nsteps'])):
        t, h, st, rc = k.step(t, h, opts)
        assert st.accepted and st.rejections == z['rej'][s] and st.pc_used == klib.PC_DIRECT
        assert st.linear_its == 4 * (1 + st.rejections)
        assert abs(st.h_used - z['h_acc'][s]) <= 1e-7 * z['h_acc'][s]
        assert abs(t - z['t_acc'][s]) <= 1e-9 * max(t, 1e-30)
    assert abs(h - float(z['h_next'])) <= 1e-6 * h
    assert rel_l2(k.get_state(), cijk_to_soa(z['uN'])) < DIRECT_TOL
    k.close()


# ---- 3. the oracle's dense LU at the library default ksp_rtol ---------------------------------------------------------------------
@pytest.mark.parametrize('shape,nlig,L,h', [((48, 40), 1, (0.1, 0.1), 0.05), ((32, 32), 2, (0.2, 0.2), 0.1),
                                             ((24,), 1, (0.05,), 0.2), ((256,), 1, (0.4,), 0.1)])
def test_direct_step_vs_oracle_lu_at_default_ksp_rtol(shape, nlig, L, h):
    """ksp_rtol = 1e-6 (library default): GMRES lands near 1e-10 of the exact step there; the direct solve is exact to rounding"""
    dim = len(shape)
    cfg = ProblemConfig.standard(dim, shape, L=L, nlig=nlig)
    rng = np.random.default_rng(11)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)
    u = np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(nlig)])
    un, err, wr, _ = ko.Oracle(cfg).rosw_step(u, h, 0.01, 1e-6, solver='lu')
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    t, hn, st, rc = k.step(0.0, h, _direct_opts(adapt=0, atol=0.01, rtol=1e-6))
    assert st.pc_used == klib.PC_DIRECT and st.linear_its == 4 and st.residual_evals == 4
    assert rel_l2(k.get_state(), un) <= 1e-12
    assert abs(st.wrms - wr) <= 1e-9 * wr
    k.close()


# ---- 4. the indefinite random sweep, every case ----------------------------------------------------------------------------------
def _indefinite_case(i):
    """case 100 + i of the indefinite sweep: (cfg, u, h, cond(shift*I - J))"""
    import scipy.sparse as sp
    cfg, u, rng = random_problem(100 + i, for_step=True)
    rp, col, val = ko.Oracle(cfg).jacobian_csr(u)
    J = sp.csr_matrix((val, col, rp)).toarray()
    lam = np.linalg.eigvals(J)
    growth = float(lam.real.max())
    if growth > 0.0:
        shift = 0.5 * growth
        for _ in range(50):
            if np.abs(lam - shift).min() >= 0.02 * shift:
                break
            shift *= 1.03
        h = 1.0 / (GAMMA * shift)
    else:
        h = float(10 ** rng.uniform(-3, 0.5))
    return cfg, u, h, float(np.linalg.cond(np.eye(J.shape[0]) / (GAMMA * h) - J))


@pytest.mark.parametrize('i', range(40))
def test_direct_random_problem_indefinite_step_vs_oracle(i):
    """The construction of test_gpu_random_sweep.test_random_problem_indefinite_step_vs_oracle (shift = 1/(gamma h) at half the largest
    growth rate of the state, 2 % clear of every eigenvalue), with no exception list: 119 (unpreconditioned GMRES stagnates) and 127
    (GMRES needs 3e-8 there) included.  A case without a growing mode takes the random h of the capped sweep instead of being skipped.
    ksp_rtol is the library default: the true-residual test of 1e-12 the GMRES sweep uses cannot be met in fp64 by any solver on the
    nearly singular systems of this sweep (case 121: shift 3.3e-6, cond 1.0e7; the backward-stable residual floor is eps*||A|| ||x||).
    Bound: 1e-8, or 1e-12 cond(shift*I - J) where that is larger -- the device and the oracle evaluate the stage right-hand sides with
    different rounding (~1e-13 relative) and the stage solves amplify that by up to cond; the same floor put case 127 on 3e-8 in the
    GMRES sweep.  Measured (rel-L2 vs the oracle's LU step): worst 127: 2.35e-8 at cond 8.3e4 (bound 8.3e-8); next 121: 5.1e-10 at
    cond 1.0e7; 119: 2.2e-13."""
    cfg, u, h, cond = _indefinite_case(i)
    un, err, wr, _ = ko.Oracle(cfg).rosw_step(u, h, 0.01, 1e-6, solver='lu')
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    t, hn, st, rc = k.step(0.0, h, _direct_opts(adapt=0, atol=0.01, rtol=1e-6), raise_on_error=False)
    state = k.get_state()
    msg = k.last_error()
    k.close()
    assert rc == 0 and st.pc_used == klib.PC_DIRECT, (100 + i, rc, msg, cfg.n, cfg.nlig, h, cond)
    assert rel_l2(state, un) <= max(1e-8, 1e-12 * cond), (100 + i, rel_l2(state, un), cond, cfg.n, cfg.nlig, h, st.linear_its)


# ---- 5. guards --------------------------------------------------------------------------------------------------------------------
def test_direct_guards_leave_everything_untouched():
    cfg = ProblemConfig.standard(2, (129, 128), L=(0.4, 0.4))
    assert cfg.F * cfg.N > klib.DIRECT_MAX
    u = _state(cfg, 2)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    before = k.get_state()
    t, hn, st, rc = k.step(0.5, 0.05, _direct_opts(adapt=0, atol=0.01, rtol=1e-6), raise_on_error=False)
    assert rc == klib.EINVAL and t == 0.5 and hn == 0.05
    assert 'KSFD_DIRECT_MAX' in k.last_error() and 'pc_type 2' in k.last_error()
    with pytest.raises(klib.KSFDError) as e:
        k.direct_apply(100.0, u)
    assert e.value.code == klib.EINVAL
    assert np.array_equal(k.get_state(), before)
    # the same handle still steps with the default solver
    opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12)
    t, hn, st, rc = k.step(0.0, 0.05, opts)
    un, _, wr, _ = ko.Oracle(cfg).rosw_step(u, 0.05, 0.01, 1e-6, solver='gmres', ksp_rtol=1e-12)
    assert st.pc_used != klib.PC_DIRECT and rel_l2(k.get_state(), un) < 1e-10
    k.close()


def test_direct_refuses_a_ring_of_one():
    from ksfd_amd import dist
    cfg = ProblemConfig.standard(2, (32, 32), L=(0.2, 0.2))
    u = _state(cfg, 4)
    ks, keep = dist.open_self_ring(cfg, 0, 'host')
    ks.set_state(u)
    t, hn, st, rc = ks.step(0.0, 0.1, _direct_opts(adapt=0, atol=0.01, rtol=1e-6), raise_on_error=False)
    assert rc == klib.EINVAL and 'single rank' in ks.last_error() and t == 0.0 and hn == 0.1
    with pytest.raises(klib.KSFDError) as e:
        ks.direct_apply(100.0, u)
    assert e.value.code == klib.EINVAL
    assert np.array_equal(ks.get_state(), u)
    t, hn, st, rc = ks.step(0.0, 0.1, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12))
    un, _, _, _ = ko.Oracle(cfg).rosw_step(u, 0.1, 0.01, 1e-6, solver='lu')
    assert rel_l2(ks.get_state(), un) < 1e-10
    ks.close()


# ---- 6. the direct machinery leaves the default path alone -----------------------------------------------------------------------
def test_direct_apply_leaves_the_default_stepper_unchanged():
    cfg = ProblemConfig.standard(2, (48, 40), L=(0.1, 0.1))
    u = _state(cfg, 6)
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6)
    out = []
    for with_direct in (True, False):
        k = klib.KSFDHip(cfg)
        k.set_state(u)
        if with_direct:
            k.direct_apply(1.0 / (GAMMA * 0.05), np.ones(k.nlocal))
        t, h = 0.0, 0.01
        for _ in range(5):
            t, h, st, rc = k.step(t, h, opts)
            assert st.pc_used & klib.PC_DIRECT == 0
        out.append((k.get_state(), t, h))
        k.close()
    assert rel_l2(out[0][0], out[1][0]) <= 1e-13 and out[0][1] == out[1][1] and out[0][2] == out[1][2]
