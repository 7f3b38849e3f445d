"""GPU: GMRES with deflated restarting (ksfd_set_deflation) -- the in-place basis rotation kernel against numpy, the solver on the
indefinite stage systems of the random sweep against the oracle's LU step, its iteration counts against plain restarted GMRES, the
preconditioned modes, and the guarantees around it (off means off, bitwise replay, guards)."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from ksfd_amd import lib as klib
from ksfd_amd.config import ProblemConfig
from oracle import ko
from test_gpu_random_sweep import random_problem

pytestmark = pytest.mark.gpu

GAMMA = 0.43586652150845900


# ---- 1. rotation kernel -------------------------------------------------------------------------------------------------------
# 24x10 and 26x8 have an even point count (16-byte loads), 25x9 an odd one (8-byte loads): the two instantiations of the kernel.
# The library has no single-field problem (one ligand at least), so every 2-D / 1-D grid runs with its smallest field count, F = 2.
ROT_GRIDS = [((24, 10), 1), ((26, 8), 1), ((25, 9), 1), ((6, 5, 7), 2), ((166,), 1)]


@pytest.mark.parametrize('shape,nlig', ROT_GRIDS)
@pytest.mark.parametrize('nin,nout', [(2, 1), (31, 11), (31, 18), (None, 17)])
def test_rotation_kernel_vs_numpy(shape, nlig, nin, nout):
    cfg = ProblemConfig.standard(len(shape), shape, L=tuple(0.01 * n for n in shape), nlig=nlig)
    k = klib.KSFDHip(cfg)
    if nin is None:
        nin = min(klib.ROT_MAXIN, k.basis_capacity())
    rng = np.random.default_rng(nin * 100 + nout + len(shape))
    P = np.linalg.qr(rng.standard_normal((nin, nout)))[0]                # orthonormal columns
    vin = rng.standard_normal((nin, k.nlocal))
    out = k.basis_rotate(P, vin)
    ref = P.T @ vin
    err = np.linalg.norm(out[:nout] - ref) / np.linalg.norm(ref)
    print('rotation %s nin %d nout %d rel-L2 %.3e' % (shape, nin, nout, err))
    assert err < 1e-13                                                   # fp64 sums of <= 121 terms, ||P|| = 1
    assert np.array_equal(out[nout:], vin[nout:])                        # vectors nout .. nin-1 are untouched
    k.close()


def test_rotation_rejects_sizes_outside_its_limits():
    cfg = ProblemConfig.standard(2, (24, 10), L=(0.24, 0.1), nlig=1)
    k = klib.KSFDHip(cfg)
    for nin, nout in [(20, 19), (3, 4), (klib.ROT_MAXIN + 1, 2)]:
        with pytest.raises(klib.KSFDError) as e:
            k.basis_rotate(np.zeros((nin, nout)), np.zeros((nin, k.nlocal)))
        assert e.value.code == klib.EINVAL
    k.close()


# ---- shared references (computed once per case) -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def indefinite_case(case):
    """the construction of test_random_problem_indefinite_step_vs_oracle: shift at half the largest growth rate, 2 % clear of the spectrum"""
    import scipy.sparse as sp
    cfg, u, rng = random_problem(case, for_step=True)
    rp, col, val = ko.Oracle(cfg).jacobian_csr(u)
    lam = np.linalg.eigvals(sp.csr_matrix((val, col, rp)).toarray())
    growth = float(lam.real.max())
    assert growth > 0.0
    shift = 0.5 * growth
    for _ in range(50):
        if np.abs(lam - shift).min() >= 0.02 * shift:
            break
        shift *= 1.03
    assert int((lam.real > shift).sum()) >= 1
    h = 1.0 / (GAMMA * shift)
    un, err, wr, _ = ko.Oracle(cfg).rosw_step(u, h, 0.01, 1e-6, solver='lu')
    un.setflags(write=False)
    return cfg, u, h, un


def indefinite_opts(restart=30):
    return klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, pc_type=0, ksp_restart=restart, ksp_rtol=1e-12, ksp_max_it=20000)


@functools.lru_cache(maxsize=None)
def deflated_indefinite_run(case, carry, tuning=None):
    cfg, u, h, un = indefinite_case(case)
    k = klib.KSFDHip(cfg)
    if tuning is not None:
        k.set_tuning(use_fused=tuning)
    k.set_state(u)
    k.set_deflation(10, carry)
    t, hn, st, rc = k.step(0.0, h, indefinite_opts(), raise_on_error=False)
    state, ds, msg = k.get_state(), k.deflation_stats(), k.last_error()
    k.close()
    state.setflags(write=False)
    return rc, state, st.linear_its, ds, msg


# ---- 2. correct on indefinite systems -----------------------------------------------------------------------------------------
BOUND = {127: 3e-8, 119: 1e-7}        # 127 as in the existing sweep; 119: cond(A) = 4.4e4 times 1e-12, a factor ~2 for the four stages


@pytest.mark.parametrize('carry', [1, 0])
@pytest.mark.parametrize('case', [100, 102, 103, 108, 110, 119, 127])
def test_deflated_gmres_on_indefinite_systems_vs_oracle(case, carry):
    """Measured on an MI355X (profiles/deflation_runs.log): every case returns 0; rel-L2 against the LU step 2e-13 ... 7e-11 for
    100, 102, 103, 108, 110, 119 and 1.4e-9 (carry) / 2.4e-9 (no carry) for case 127 (condition 8.3e4; bound 3e-8)."""
    cfg, u, h, un = indefinite_case(case)
    rc, state, its, ds, msg = deflated_indefinite_run(case, carry)
    err = rel_l2(state, un)
    print('case %d carry %d: rc %d its %d rel-L2 %.3e stats %s %s' % (case, carry, rc, its, err, ds, msg))
    assert rc == 0, (cfg.n, cfg.nlig, h, its, msg)
    assert err < BOUND.get(case, 1e-8), (cfg.n, cfg.nlig, h, its)
    assert ds['restarts'] >= 1
    assert sum(ds['stage_its']) == its


# ---- 3. it deflates -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [100, 102, 110])
def test_deflation_halves_the_iterations_of_restarted_gmres(case):
    cfg, u, h, un = indefinite_case(case)
    k = klib.KSFDHip(cfg)
    k.set_tuning(use_fused=klib.TUNE_FUSED | klib.TUNE_NO_RESTART_GROWTH)
    k.set_deflation(0, 1)
    k.set_state(u)
    t, hn, st, rc = k.step(0.0, h, indefinite_opts(), raise_on_error=False)
    its_gmres = st.linear_its
    k.set_state(u)
    k.set_deflation(10, 1)
    t, hn, st, rc_d = k.step(0.0, h, indefinite_opts(), raise_on_error=False)
    its_dgmres = st.linear_its
    k.close()
    print('case %d: GMRES(30) %d its (rc %d), GMRES-DR(30,10) %d its (rc %d)' % (case, its_gmres, rc, its_dgmres, rc_d))
    assert rc_d == 0
    assert 2 * its_dgmres <= its_gmres


# ---- 4. preconditioned modes --------------------------------------------------------------------------------------------------
PC_GRIDS = [((32, 32), (0.08, 0.08), 50.0, 4), ((128,), (128 / 384.0,), 5.0, 8), ((8, 8, 8), (0.02, 0.02, 0.02), 20.0, 6)]


@functools.lru_cache(maxsize=None)
def stiff_case(idx):
    shape, L, h, seed = PC_GRIDS[idx]
    cfg = ProblemConfig.standard(len(shape), shape, L=L, nlig=1)
    rng = np.random.default_rng(seed)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)
    u = np.concatenate([rho, rho * cfg.lig_s[0] / cfg.lig_gamma[0]])
    un, err, wr, _ = ko.Oracle(cfg).rosw_step(u, h, 0.01, 1e-6, solver='lu')
    return cfg, u, h, un, wr


@pytest.mark.parametrize('pc_type', [1, 3])
@pytest.mark.parametrize('idx', range(len(PC_GRIDS)))
def test_deflated_preconditioned_modes_give_the_lu_answer(idx, pc_type):
    cfg, u, h, un, wr = stiff_case(idx)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    k.set_deflation(6, 1)
    t, hn, st, rc = k.step(0.0, h, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12, ksp_max_it=20000, ksp_restart=12,
                                                          pc_type=pc_type), raise_on_error=False)
    err, ds, msg = rel_l2(k.get_state(), un), k.deflation_stats(), k.last_error()
    k.close()
    print('%s pc_type %d: rc %d pc_used %d its %d rel-L2 %.3e wrms %.6e vs %.6e stats %s %s' % (cfg.n, pc_type, rc, st.pc_used, st.linear_its, err, st.wrms, wr, ds, msg))
    assert rc == 0, msg
    assert err < 1e-9
    assert abs(st.wrms - wr) <= 1e-5 * wr + 1e-12


# ---- 5. off means off ---------------------------------------------------------------------------------------------------------
def test_keep_zero_is_bitwise_the_untouched_handle():
    import scipy.sparse as sp
    cfg, u, rng = random_problem(100, for_step=True)
    h = float(10 ** rng.uniform(-3, 0.5))
    rp, col, val = ko.Oracle(cfg).jacobian_csr(u)
    growth = max(0.0, float(np.linalg.eigvals(sp.csr_matrix((val, col, rp)).toarray()).real.max()))
    if growth > 0.0:
        h = min(h, 0.5 / (GAMMA * growth))
    res = []
    for touch in (False, True):
        k = klib.KSFDHip(cfg)
        if touch:
            k.set_deflation(10, 1)
            k.set_deflation(0, 1)
        k.set_state(u)
        t, hn, st, rc = k.step(0.0, h, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12, ksp_max_it=20000))
        res.append((k.get_state(), st.linear_its, k.deflation_stats()))
        k.close()
    assert np.array_equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]
    assert res[1][2]['restarts'] == 0 and sum(res[1][2]['stage_its']) == 0


# ---- 6. replay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('carry', [1, 0])
def test_checkpoint_replay_is_bitwise_with_deflation_on(carry):
    """step, save, two steps, restore, two steps.  Fixed steps at a twentieth of the indefinite one (shift at ten times the largest growth
    rate: definite) with a short restart, so that the solves converge quickly and still restart"""
    cfg, u, h, un = indefinite_case(100)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    k.set_deflation(3, carry)
    opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, pc_type=0, ksp_restart=8, ksp_rtol=1e-10, ksp_max_it=5000)
    t, hh, st, rc = k.step(0.0, 0.05 * h, opts)
    restarts = k.deflation_stats()['restarts']
    k.checkpoint()
    runs = []
    for rep in range(2):
        if rep:
            k.restore()
        tt, h2, log = t, hh, []
        for _ in range(2):
            tt, h2, st, rc = k.step(tt, h2, opts, raise_on_error=False)
            log.append((rc, st.linear_its, k.deflation_stats()['restarts']))
        runs.append((k.get_state(), tt, h2, log))
    k.close()
    print('replay carry %d: first step %d restarts, then %s' % (carry, restarts, runs[0][3]))
    assert all(rc == 0 for rc, _, _ in runs[0][3])
    assert restarts + sum(r for _, _, r in runs[0][3]) >= 1              # deflation was at work
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1:] == runs[1][1:]


# ---- 7. guards ----------------------------------------------------------------------------------------------------------------
def test_guards():
    cfg, u, h, un = indefinite_case(100)
    k = klib.KSFDHip(cfg)
    with pytest.raises(klib.KSFDError) as e:
        k.set_deflation(17, 1)
    assert e.value.code == klib.EINVAL
    k.set_state(u)
    k.set_deflation(10, 1)
    before = k.get_state()
    t, hn, st, rc = k.step(0.0, h, indefinite_opts(restart=12), raise_on_error=False)
    assert rc == klib.EINVAL and t == 0.0
    assert np.array_equal(k.get_state(), before)                        # state untouched
    k.close()


def test_async_tuning_bit_runs_the_synchronous_deflated_solver():
    cfg, u, h, un = indefinite_case(100)
    rc, state, its, ds, msg = deflated_indefinite_run(100, 1)
    rc_a, state_a, its_a, ds_a, msg_a = deflated_indefinite_run(100, 1, klib.TUNE_FUSED | klib.TUNE_ASYNC_GMRES)
    assert rc_a == 0 and rc == 0
    assert ds_a['restarts'] >= 1 and its_a == its
    assert np.array_equal(state_a, state)
    assert rel_l2(state_a, un) < 1e-8
