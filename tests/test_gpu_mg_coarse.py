"""GPU: the opt-in exact coarse solve of the multigrid V cycle (ksfd_set_mg_coarse kind 1): shift*I - J_c assembled on the level the cycle
ends on from its restricted coefficient planes, dense LU with one launch per panel (k_lu_panel), explicit inverse (k_lu_invert), one GEMV
per cycle (k_mgc_gemv).  Every test calls set_mg_coarse, which the library does not have without the feature."""
import threading

import numpy as np
import pytest

from conftest import rel_l2
from ksfd_amd.config import ProblemConfig
from ksfd_amd import lib as klib
from oracle import ko

pytestmark = pytest.mark.gpu
GAMMA = 0.43586652150845900
EPS = np.finfo(float).eps


def _cfg(shape, nlig, L=None):
    dim = len(shape)
    L = L or tuple(0.0025 * n for n in shape)
    if nlig <= 2:
        return ProblemConfig.standard(dim, shape, L=L, nlig=nlig)
    # attractant + repellent of options84, then one more attractant in the first group (as tests/test_gpu_step.py builds three ligands)
    return ProblemConfig(dim=dim, n=shape, L=L, lig_group=[0, 1, 0][:nlig], lig_w=[1.0, 1.0, 0.5][:nlig], lig_s=[0.01, 0.001, 0.003][:nlig],
                         lig_gamma=[0.01, 0.001, 0.004][:nlig], lig_D=[1e-6, 1e-5, 3e-6][:nlig], grp_alpha=[1500.0, 1500.0],
                         grp_beta=[5.56e-4, -5.56e-4])


def _state(cfg, seed, amp=0.01):
    rng = np.random.default_rng(seed)
    rho = 9000.0 * (1.0 + amp * rng.standard_normal(cfg.N))
    return np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(cfg.nlig)])


def _probe(k, shift, n):
    """dense shift*I - J_c, column by column, from the level's own operator kernels"""
    A = np.empty((n, n))
    e = np.zeros(n)
    for c in range(n):
        e[c] = 1.0
        A[:, c] = k.mg_coarse_apply(shift, e, op=0)
        e[c] = 0.0
    return A


# ---- 1. the coarse solve against numpy ---------------------------------------------------------------------------------------------
#              shape, ligands, max_unknowns, level, extents of that level, unknowns      edge of the panel / inversion / GEMV kernels
SOLVE_CASES = [((96,), 1, 0, 3, (12, 1, 1), 24),                                       # less than one panel
               ((130,), 1, 0, 1, (65, 1, 1), 130),                                      # odd, ragged
               ((32, 32), 1, 0, 2, (8, 8, 1), 128),                                     # two full panels
               ((48, 40), 1, 0, 2, (12, 10, 1), 240),                                   # ragged last panel
               ((40, 24), 2, 0, 1, (20, 12, 1), 720),                                   # many panels
               ((16, 16, 16), 1, 0, 1, (8, 8, 8), 1024),                                # exact multiple of 64
               ((64, 64), 3, 2048, 2, (16, 16, 1), 1024)]                               # cut above the coarsest level


@pytest.mark.parametrize('shape,nlig,maxu,level,ext,unknowns', SOLVE_CASES)
def test_coarse_solve_against_numpy(shape, nlig, maxu, level, ext, unknowns):
    """A_c(shift) probed with op 0 on unit vectors, numpy.linalg.solve on it, op 1 on random vectors: distance <= 100 eps cond_2(A_c), the
    bound of the LU solves of tests/test_gpu_direct.py (an inverse-times-vector solve obeys a forward bound of that form; the 1e-13
    residual bound of the triangular solves it does not, so none is asserted).  Shifts: 10 rho(J_c), 1/(gamma h) of a moderate step, and
    one inside the spectrum (half the largest growth rate of J_c, moved by 3 % steps until 2 % clear of every eigenvalue).
    Measured head-room (bound / distance) per case and shift: profiles/mg_coarse_runs.log."""
    # spacing 0.0025 as in the fp32-cycle test; the 3-D box is four times as wide: on the 0.04^3 box the 8^3 level has no growing mode
    # (largest real part of eig(J_c) -3.3e-3), so there would be no shift inside the spectrum; on 0.16^3 it has about thirty
    cfg = _cfg(shape, nlig, tuple((0.01 if len(shape) == 3 else 0.0025) * n for n in shape))
    k = klib.KSFDHip(cfg)
    k.set_state(_state(cfg, 3, amp=0.05))
    before = k.mg_coarse_info()
    assert before['kind'] == 0 and before['level'] == before['nlevels'] - 1 and before['factorizations'] == 0
    k.set_mg_coarse(1, maxu)
    info = k.mg_coarse_info()
    assert (info['kind'], info['level'], info['n'], info['unknowns'], info['F']) == (1, level, ext, unknowns, cfg.F), info
    n = unknowns
    s_mod = 1.0 / (GAMMA * 0.05)
    A0 = _probe(k, 0.0, n)                                   # -J_c
    A1 = _probe(k, s_mod, n)
    # the operator at two shifts differs by the shift on the diagonal and by nothing else: off the diagonal bit for bit; on the diagonal
    # to rounding: each probed entry shift - j_ii is a rounded result (half an ulp of it) and so is the difference formed here
    D = A1 - A0
    d = np.diag(D)
    assert not (D - np.diag(d)).any()
    half_ulp = lambda a: 0.5 * np.spacing(np.abs(a))
    assert np.all(np.abs(d - s_mod) <= half_ulp(np.diag(A1)) + half_ulp(np.diag(A0)) + half_ulp(d)), float(np.abs(d - s_mod).max())
    lam = np.linalg.eigvals(-A0)                             # spectrum of J_c
    R = float(np.abs(lam).max())
    growth = float(lam.real.max())
    assert growth > 0.0                                      # these states have growing modes the coarse level resolves
    inside = 0.5 * growth
    for _ in range(50):
        if np.abs(lam - inside).min() >= 0.02 * inside:
            break
        inside *= 1.03
    assert int((lam.real > inside).sum()) >= 1
    rng = np.random.default_rng(5)
    for name, shift in (('10rho', 10.0 * R), ('moderate', s_mod), ('inside', inside)):
        A = A0 + shift * np.eye(n)
        b = rng.standard_normal(n)
        z = k.mg_coarse_apply(shift, b, op=1)
        ref = np.linalg.solve(A, b)
        cond = np.linalg.cond(A)
        dist, bound = rel_l2(z, ref), 100 * EPS * cond
        print('mg_coarse solve %s F=%d n=%d shift %s=%.4g cond %.3e distance %.3e bound %.3e head-room %.1f' %
              ('x'.join(str(s) for s in shape), cfg.F, n, name, shift, cond, dist, bound, bound / max(dist, 1e-300)))
        assert dist <= bound, (name, shift, dist, cond)
    after = k.mg_coarse_info()
    assert after['factorizations'] == 3 and after['solves'] == 3 and after['fallbacks'] == 0
    k.close()


# ---- 2. steps equal the LU oracle --------------------------------------------------------------------------------------------------
def _stiff_2d():
    """set-up of tests/test_gpu_step.py::test_multigrid_makes_very_stiff_steps_cheap"""
    cfg = ProblemConfig.standard(2, (32, 32), L=(0.08, 0.08), nlig=2)
    rng = np.random.default_rng(4)
    rho = 9000 + 90 * rng.standard_normal(32 * 32)
    return cfg, np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(2)]), 50.0


def _stiff_3d():
    """... ::test_multigrid_3d_stiff_step_vs_oracle_lu"""
    cfg = ProblemConfig.standard(3, (16, 16, 16), L=(0.04, 0.04, 0.04), nlig=1)
    rng = np.random.default_rng(6)
    rho = 9000 + 90 * rng.standard_normal(16 ** 3)
    return cfg, np.concatenate([rho, rho]), 20.0


def _stiff_1d(n, h):
    """... ::test_multigrid_1d_stiff_step_vs_oracle_lu"""
    cfg = ProblemConfig.standard(1, (n,), L=(n / 384.0,), nlig=2)
    rng = np.random.default_rng(8)
    rho = 9000 + 90 * rng.standard_normal(n)
    return cfg, np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(2)]), h


_ORACLE = {}


def _oracle_step(key, cfg, u, h):
    """the oracle's step, computed once and shared (never modified)"""
    if key not in _ORACLE:
        if cfg.dim == 3:
            _ORACLE[key] = ko.Oracle(cfg).rosw_step(u, h, 0.01, 1e-6, solver='gmres', ksp_rtol=1e-12, maxit=6000)[0]
        else:
            _ORACLE[key] = ko.Oracle(cfg).rosw_step(u, h, 0.01, 1e-6, solver='lu')[0]
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


STIFF = {'2d': _stiff_2d, '3d': _stiff_3d, '1d-96': lambda: _stiff_1d(96, 5.0), '1d-384': lambda: _stiff_1d(384, 50.0),
         '1d-130': lambda: _stiff_1d(130, 2.0)}


def _one_step(cfg, u, h, kind, ksp_rtol, maxu=0, eager=False):
    k = klib.KSFDHip(cfg)
    if eager:
        k.set_mg_params(power_its=klib.MG_EAGER)
    if kind is not None:
        k.set_mg_coarse(kind, maxu)
    k.set_state(u)
    t, hn, st, rc = k.step(0.0, h, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=ksp_rtol, pc_type=1))
    out = (k.get_state(), st, k.mg_coarse_info())
    k.close()
    return out


@pytest.mark.parametrize('which', list(STIFF))
def test_stiff_step_with_exact_coarse_solve_vs_oracle(which):
    cfg, u, h = STIFF[which]()
    un = _oracle_step(which, cfg, u, h)
    state, st, info = _one_step(cfg, u, h, 1, 1e-11)
    print('mg_coarse step %s: level %d of %d, %d unknowns, its %d, rel-L2 vs oracle %.3e' %
          (which, info['level'], info['nlevels'], info['unknowns'], st.linear_its, rel_l2(state, un)))
    assert rel_l2(state, un) < 1e-9
    assert st.pc_used & klib.PC_MG_COARSE_DIRECT and st.pc_used & klib.PC_MULTIGRID
    assert info['factorizations'] >= 1 and info['solves'] >= st.linear_its and info['fallbacks'] == 0


@pytest.mark.parametrize('shape,nlig,L,h,maxu', [((32, 32), 2, (0.08, 0.08), 50.0, 0),         # the 2-D stiff step above
                                                  ((64, 64), 3, None, 10.0, 2048)])            # the cycle ends on a level that would run in fp32
def test_fp32_cycle_with_exact_coarse_solve_vs_chebyshev(shape, nlig, L, h, maxu):
    """ksp_rtol = 1e-6: the V cycle keeps its level vectors in fp32 down to the level of the exact solve, which runs in fp64 behind the border
    conversion the cycle has.  Both runs solve the same stage systems to the same tolerance with different preconditioners, so they
    agree as two solves of one system do: 5e-6, what tests/test_gpu_step.py::test_multigrid_cycle_with_fp32_level_vectors allows between
    its fp32-cycle step and another solver's."""
    cfg = _cfg(shape, nlig, L)
    rng = np.random.default_rng(4)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)
    u = np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(nlig)])
    s0, st0, _ = _one_step(cfg, u, h, 0, 1e-6)
    s1, st1, info = _one_step(cfg, u, h, 1, 1e-6, maxu)
    print('mg_coarse fp32 %s F=%d: its cheb %d lu %d, rel-L2 between them %.3e' % (shape, cfg.F, st0.linear_its, st1.linear_its, rel_l2(s1, s0)))
    assert st0.pc_used & 64 == 0 and st1.pc_used & 64
    assert info['solves'] >= st1.linear_its and info['fallbacks'] == 0
    assert rel_l2(s1, s0) < 5e-6


# ---- 3. captured and eager launches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ksp_rtol', [1e-11, 1e-6])
def test_graph_and_eager_cycles_are_bitwise_equal(ksp_rtol):
    cfg, u, h = _stiff_2d()
    sg, stg, ig = _one_step(cfg, u, h, 1, ksp_rtol)
    se, ste, ie = _one_step(cfg, u, h, 1, ksp_rtol, eager=True)
    assert stg.pc_used & 64 and ste.pc_used & 64
    assert stg.linear_its == ste.linear_its and ig['solves'] == ie['solves']
    assert np.array_equal(sg, se)


# ---- 4. off is off ------------------------------------------------------------------------------------------------------------------
def test_switched_off_equals_never_switched_on():
    cfg, u, h = _stiff_2d()
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, pc_type=1)
    out = []
    for touch in (True, False):
        k = klib.KSFDHip(cfg)
        if touch:
            k.set_mg_coarse(1)
            k.set_mg_coarse(0)
        k.set_state(u)
        t, hh, rec = 0.0, 5.0, []
        for _ in range(3):
            t, hh, st, rc = k.step(t, hh, opts)
            assert st.pc_used & 2 and st.pc_used & 64 == 0
            rec.append((t, hh, st.linear_its, st.rejections, k.get_state()))
        assert k.mg_coarse_info()['solves'] == 0
        out.append(rec)
        k.close()
    for a, b in zip(*out):
        assert a[:4] == b[:4] and np.array_equal(a[4], b[4])


# ---- 5. checkpoint ------------------------------------------------------------------------------------------------------------------
def test_checkpoint_restore_replays_the_same_steps_with_exact_coarse_solve():
    """set-up of tests/test_gpu_step.py::test_checkpoint_restore_replays_the_same_steps_in_the_multigrid_regime; nothing of the coarse
    solve joins the checkpoint, its factors are rebuilt from the restored state"""
    cfg = ProblemConfig.standard(2, (64, 64), L=(0.16, 0.16), nlig=2)
    rng = np.random.default_rng(37)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)
    u = np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(2)])
    k = klib.KSFDHip(cfg)
    k.set_mg_coarse(1)
    k.set_state(u)
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, pc_type=1)
    t, h = 0.0, 5.0
    for _ in range(2):
        t, h, st, rc = k.step(t, h, opts)
    k.checkpoint()
    tc, hc = t, h

    def run():
        tt, hh, out = tc, hc, []
        for _ in range(2):
            tt, hh, st, rc = k.step(tt, hh, opts)
            assert st.pc_used & 64
            out.append((tt, hh, st.linear_its, st.rejections, st.pc_used, k.get_state().copy()))
        return out
    first = run()
    k.restore()
    second = run()
    for a, b in zip(first, second):
        assert a[:5] == b[:5]
        assert np.array_equal(a[5], b[5])
    k.close()


# ---- 6. guards ----------------------------------------------------------------------------------------------------------------------
def _refused(k, kind, maxu, word):
    before = k.mg_coarse_info() if word != 'hierarchy' else None
    with pytest.raises(klib.KSFDError) as e:
        k.set_mg_coarse(kind, maxu)
    assert e.value.code == klib.EINVAL and word in str(e.value), str(e.value)
    if before is not None:
        assert k.mg_coarse_info() == before


@pytest.mark.parametrize('shape,nlig,maxu,word', [((32, 32), 2, 4096, 'KSFD_MG_DIRECT_MAX'),      # max_unknowns above the cap
                                                   ((24, 24, 24), 2, 0, 'unknowns'),               # coarsest level: 12^3 x 3 = 5184
                                                   ((32, 32), 2, 100, 'unknowns'),                 # no level that small (coarsest: 192)
                                                   ((7, 5, 7), 1, 0, 'hierarchy')])                # no hierarchy
def test_refused_settings_leave_the_handle_unchanged(shape, nlig, maxu, word):
    cfg = _cfg(shape, nlig, tuple(0.0025 * n for n in shape))
    u = _state(cfg, 2)
    opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-9, pc_type=1)
    out = []
    for attempt in (True, False):
        k = klib.KSFDHip(cfg)
        if attempt:
            _refused(k, 1, maxu, word)
        k.set_state(u)
        t, hn, st, rc = k.step(0.0, 1.0, opts)
        assert st.pc_used & 64 == 0
        out.append((st.linear_its, k.get_state()))
        k.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


class _PairRing:
    """transport-2 callbacks of rank `rank` of two ranks living in two threads of this process: the buffers meet in shared slots at a barrier"""

    def __init__(self, rank, shared):
        self.rank, self.sh = rank, shared
        self._ex = klib.EXCHANGE_FN(self._exchange)
        self._ar = klib.ALLREDUCE_FN(self._allreduce)
        self._a2a = klib.ALLTOALL_FN(lambda ctx, send, recv, nbytes: 1)      # no spectral solver on these grids

    def _exchange(self, ctx, slo, shi, rlo, rhi, count):
        try:
            n = int(count)
            arr = lambda p: np.ctypeslib.as_array(p, shape=(n,))
            self.sh['ex'][self.rank] = (arr(slo).copy(), arr(shi).copy())
            self.sh['bar'].wait(60)
            olo, ohi = self.sh['ex'][1 - self.rank]      # both neighbours are the other rank: its send_lo is my high ghost
            arr(rhi)[:] = olo
            arr(rlo)[:] = ohi
            self.sh['bar'].wait(60)
            return 0
        except Exception:                                 # never let an exception cross the C boundary
            return 1

    def _allreduce(self, ctx, buf, count, op):
        try:
            v = np.ctypeslib.as_array(buf, shape=(int(count),))
            self.sh['ar'][self.rank] = v.copy()
            self.sh['bar'].wait(60)
            a, b = self.sh['ar'][0], self.sh['ar'][1]
            r = np.maximum(a, b) if op else a + b
            self.sh['bar'].wait(60)
            v[:] = r
            return 0
        except Exception:
            return 1

    def cdist(self):
        d = klib.CDist()
        d.rank, d.size, d.transport, d.device = self.rank, 2, 2, 0
        d.nccl_id = None
        d.exchange, d.allreduce, d.ctx, d.alltoall = self._ex, self._ar, None, self._a2a
        return d


def _pair_step(cfg, u, attempt):
    """one stiff step on two slab ranks in two threads; attempt: each rank first asks for the exact coarse solve and must be refused"""
    from ksfd_amd.dist import local_slab
    shared = {'bar': threading.Barrier(2), 'ex': [None, None], 'ar': [None, None]}
    res, errs = [None, None], []

    def work(rank):
        try:
            ring = _PairRing(rank, shared)
            k = klib.KSFDHip(cfg, ring.cdist())
            if attempt:
                _refused(k, 1, 0, 'halo transport')
            k.set_state(local_slab(u, cfg, rank, 2))
            t, hn, st, rc = k.step(0.0, 5.0, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-9, pc_type=1))
            res[rank] = (st.linear_its, st.pc_used, k.get_state())
            k.close()
        except BaseException as e:
            errs.append(repr(e))
            shared['bar'].abort()
    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    return res


def test_two_rank_handle_refuses_and_stays_as_it_was():
    cfg = ProblemConfig.standard(2, (64, 48), L=(0.2, 0.25), nlig=1)
    u = _state(cfg, 3)
    a, b = _pair_step(cfg, u, True), _pair_step(cfg, u, False)
    for r in range(2):
        assert a[r][1] & 2 and a[r][1] & 64 == 0
        assert a[r][0] == b[r][0] and np.array_equal(a[r][2], b[r][2])


# ---- 7. an indefinite step ----------------------------------------------------------------------------------------------------------
INDEFINITE_CASE = 106      # 20 x 20, 3 ligands: levels 20^2 and 10^2 (400 coarse unknowns); see the docstring below


def test_indefinite_step_with_exact_coarse_solve_vs_oracle():
    """Case INDEFINITE_CASE of the indefinite random sweep (tests/test_gpu_random_sweep.py: shift = 1/(gamma h) at half the largest growth
    rate, 2 % clear of every eigenvalue): the first one whose grid has a multigrid hierarchy and whose coarsest level resolves a growing
    mode, picked on the CPU from the oracle's spectrum: of the 40 cases, 106, 115 and 127 have a hierarchy (every extent even, half of it >= 8)
    and a growing mode; in 106 the one eigenvalue of J above the shift belongs to the uniform mode (wavenumber 0 on both axes in the FFT
    of its density component), which every level resolves.  Bound: the sweep's, 1e-8 against the oracle's LU step.  Iteration counts with the Chebyshev and the exact coarse solve are printed, not asserted."""
    import scipy.sparse as sp
    from test_gpu_random_sweep import random_problem
    cfg, u, rng = random_problem(INDEFINITE_CASE, for_step=True)
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
    un = ko.Oracle(cfg).rosw_step(u, h, 0.01, 1e-6, solver='lu')[0]
    its = {}
    for kind in (0, 1):
        k = klib.KSFDHip(cfg)
        k.set_mg_coarse(kind)
        k.set_state(u)
        t, hn, st, rc = k.step(0.0, h, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12, ksp_max_it=20000, pc_type=1),
                               raise_on_error=False)
        state, info, msg = k.get_state(), k.mg_coarse_info(), k.last_error()
        k.close()
        its[kind] = (rc, st.linear_its, rel_l2(state, un))
        if kind == 1:
            assert rc == 0, (msg, cfg.n, cfg.nlig, h)
            assert st.pc_used & 64 and info['fallbacks'] == 0
            assert rel_l2(state, un) < 1e-8, (cfg.n, cfg.nlig, h, st.linear_its)
    print('mg_coarse indefinite case %d %s F=%d h=%.4g: (rc, its, rel-L2) cheb %s lu %s' % (INDEFINITE_CASE, cfg.n, cfg.F, h, its[0], its[1]))
