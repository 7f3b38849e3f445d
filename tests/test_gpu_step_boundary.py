"""GPU: the boundary of a step -- groom only when it can change a value, completion out of place (no roll-back copy), the embedded
error vector and the fp32 coefficient copy made when somebody asks for them, the stage-0 right-hand side with G from the coefficient
planes.  "Old" is a second handle with TUNE_OLD_BOUNDARY (groom every step, error vector stored by the completion, fp32 copy stored by the
coefficient kernel) given the same state and options: everything but the G plane must be invisible bit for bit, so those comparisons
are np.array_equal with the G plane switched off (TUNE_NO_GPLANE) on both handles."""
import dataclasses
import os
import socket

import numpy as np
import pytest

from conftest import rel_l2
from ksfd_amd.config import ProblemConfig
from ksfd_amd import lib as klib
from oracle import ko

pytestmark = pytest.mark.gpu

NEW = klib.TUNE_FUSED | klib.TUNE_NO_GPLANE               # TUNE_FUSED: the fused kernels (the default)
OLD = NEW | klib.TUNE_OLD_BOUNDARY
STEP_TOL = 1e-10                  # tests/test_gpu_step.py: rel-L2 of the state against the oracle's step
GRIDS = [((64, 32), 1), ((32, 64), 2), ((128, 96), 3)]


def make_cfg(shape, nlig, **kw):
    L = tuple(n / 320.0 for n in shape)
    cfg = ProblemConfig.standard(2, shape, L=L, nlig=min(nlig, 2))
    if nlig == 3:
        cfg = dataclasses.replace(cfg, lig_group=[0, 1, 0], lig_w=[1.0, 1.0, 0.5], lig_s=[0.01, 0.001, 0.005],
                                  lig_gamma=[0.01, 0.001, 0.005], lig_D=[1e-6, 1e-5, 3e-6])
    return dataclasses.replace(cfg, **kw) if kw else cfg


def smooth_state(cfg, seed=7, amp=600.0):
    """rho = 9000 + amp * (two waves) + a little noise, U_l at its equilibrium with a ripple; SoA, x fastest"""
    nx, ny = cfg.n[0], cfg.n[1]
    rng = np.random.default_rng(seed)
    x = (np.arange(nx) + 0.5) / nx
    y = (np.arange(ny) + 0.5) / ny
    X, Y = np.meshgrid(x, y, indexing='xy')                          # [y][x]: x fastest when flattened
    rho = 9000.0 + amp * np.sin(2 * np.pi * X) * np.cos(4 * np.pi * Y) + 0.5 * amp * np.cos(6 * np.pi * X + 1.0) + 5.0 * rng.standard_normal((ny, nx))
    planes = [rho.reshape(-1)]
    for l in range(cfg.nlig):
        planes.append(rho.reshape(-1) * cfg.lig_s[l] / cfg.lig_gamma[l] * (1.0 + 0.02 * np.sin(2 * np.pi * (l + 1) * Y).reshape(-1)))
    return np.concatenate(planes)


def handle(cfg, tuning, u=None):
    k = klib.KSFDHip(cfg)
    k.set_tuning(use_fused=tuning)
    if u is not None:
        k.set_state(u)
    return k


def adaptive(**kw):
    o = dict(adapt=1, atol=0.01, rtol=1e-6, ksp_rtol=1e-10)
    o.update(kw)
    return klib.default_step_opts(**o)


def run_steps(k, n, opts, t=0.0, h=0.02):
    """n steps; per step (state, t, h_next, wrms, launches, rejections, accepted)"""
    log = []
    for _ in range(n):
        t, h, st, rc = k.step(t, h, opts)
        log.append((k.get_state(), t, h, st.wrms, st.launches, st.rejections, st.accepted))
    return log


def same_steps(a, b):
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]), 'state after step %d' % (s + 1)
        assert x[1] == y[1] and x[2] == y[2] and x[3] == y[3], ('t, h, wrms after step %d' % (s + 1), x[1:4], y[1:4])
        assert x[5] == y[5] and x[6] == y[6]


# ---- groom ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,nlig', GRIDS)
def test_groom_left_out_on_a_smooth_state(shape, nlig):
    """every value far above its floor: from the second step on the groom is not launched and nothing else changes.  pc_type 4 (the
    spectral solver at any stiffness) so that no reader of the fp32 coefficient copy adds a launch of its own"""
    cfg = make_cfg(shape, nlig)
    u = smooth_state(cfg)
    opts = adaptive(pc_type=4)
    new, old = handle(cfg, NEW, u), handle(cfg, OLD, u)
    a, b = run_steps(new, 3, opts), run_steps(old, 3, opts)
    same_steps(a, b)
    assert all(x[6] for x in a)
    print('launches per step: new %s old %s' % ([x[4] for x in a], [x[4] for x in b]))
    assert a[0][4] == b[0][4]                                         # after set_state the groom runs
    assert a[1][4] == b[1][4] - 1 and a[2][4] == b[2][4] - 1
    new.close(), old.close()


@pytest.mark.parametrize('shape,nlig', [((64, 32), 1), ((32, 64), 2)])
def test_groom_that_clamps_matches_old_boundary_and_oracle(shape, nlig):
    """rhomin at the 30th percentile of the initial rho: the groom really clamps, and a completion really leaves values below the
    floor (the count is not 0), so the groom must run again"""
    base = make_cfg(shape, nlig)
    u = smooth_state(base)
    N = base.N
    cfg = make_cfg(shape, nlig, rhomin=float(np.percentile(u[:N], 30)))
    opts = adaptive(ksp_rtol=1e-12, ksp_max_it=4000)
    new, old = handle(cfg, NEW, u), handle(cfg, OLD, u)
    a, b = run_steps(new, 3, opts, h=0.01), run_steps(old, 3, opts, h=0.01)
    same_steps(a, b)
    assert all(x[6] for x in a)
    o = ko.Oracle(cfg)
    uo, t_prev, below = u, 0.0, []
    for s, x in enumerate(a):
        below.append(int((x[0][:N] < cfg.rhomin).sum()))
        uo, _, wr, _ = o.rosw_step(uo, x[1] - t_prev, 0.01, 1e-6, solver='gmres', ksp_rtol=1e-13, maxit=4000)
        t_prev = x[1]
        e = rel_l2(x[0], uo)
        print('step %d: rel-L2 against the oracle %.3e, values below rhomin afterwards %d' % (s + 1, e, below[-1]))
        assert e < STEP_TOL
    assert (u[:N] < cfg.rhomin).sum() > 0 and max(below[:-1]) > 0     # both really happened
    new.close(), old.close()


@pytest.mark.parametrize('what', ['scale_rho', 'set_state', 'set_params', 'checkpoint', 'checkpoint_then_params'])
def test_groom_runs_again_after_the_state_or_the_floor_moved(what):
    """two steps (the second one without a groom on the new boundary), then something that moves the state or the floor so that the
    groom of the next step has values to clamp"""
    base = make_cfg((64, 32), 1)
    u = smooth_state(base)
    N = base.N
    # Umin a little under the smallest equilibrium value of U (= rho here): a state whose U plane is pushed under it is clamped by the
    # groom and then relaxes upwards, so the completion leaves nothing below.  rhomin 1e-4: above rho * 1e-9
    cfg = make_cfg((64, 32), 1, Umin=0.95 * float(u[:N].min()), rhomin=1e-4)
    low = u.copy()
    low[N:] *= 1.0 - 0.2 * np.sin(np.pi * np.arange(N) / N) ** 2
    assert (u[N:] >= cfg.Umin).all() and (low[N:] < cfg.Umin).sum() > N // 10
    opts = adaptive()
    out = []
    for tuning in (NEW, OLD):
        k = handle(cfg, tuning, u)
        log = run_steps(k, 2, opts)
        t, h = log[-1][1], log[-1][2]
        if what == 'scale_rho':
            k.scale_rho(1e-9)                                         # every rho under rhomin
            assert (k.get_state()[:N] < cfg.rhomin).all()
        elif what == 'set_state':
            k.set_state(low)
        elif what == 'set_params':
            k.update_params(dataclasses.replace(cfg, rhomin=float(np.percentile(log[-1][0][:N], 40))))
        elif what == 'checkpoint_then_params':
            k.checkpoint()                                            # of a state with nothing below its floors ...
            k.update_params(dataclasses.replace(cfg, rhomin=float(np.percentile(log[-1][0][:N], 40))))
            k.restore()                                               # ... which is no longer true of it under the new floor
        else:
            k.set_state(low)                                          # needs its groom
            k.checkpoint()
            log += run_steps(k, 1, opts, t, h)                        # groomed and completed ...
            assert (log[-1][0][N:] >= cfg.Umin).all() and (log[-1][0][:N] >= cfg.rhomin).all()   # ... with nothing below
            k.restore()                                               # the state that needs its groom is back
            assert np.array_equal(k.get_state(), low)
        log += run_steps(k, 1, opts, t, h)
        out.append(log)
        k.close()
    same_steps(out[0], out[1])
    assert out[0][-1][6]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _slab_worker(rank, size, port, outfile):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        from ksfd_amd.dist import open_handle, local_slab, gather_slabs
        base = make_cfg((64, 32), 1)
        u = smooth_state(base)
        cfg = make_cfg((64, 32), 1, rhomin=float(np.percentile(u[:base.N], 30)))
        opts = adaptive(ksp_rtol=1e-11)
        res = {}
        for name, tuning in (('new', NEW), ('old', OLD)):
            ks, keep = open_handle(cfg, rank, size, 0, transport='host')
            ks.set_tuning(use_fused=tuning)
            ks.set_state(local_slab(u, cfg, rank, size))
            t, h, rows = 0.0, 0.01, []
            for s in range(3):
                t, h, st, rc = ks.step(t, h, opts)
                rows.append([t, h, st.wrms, st.launches, st.accepted, st.rejections])
                res['%s_state%d' % (name, s)] = gather_slabs(ks.get_state(), cfg)
            res[name + '_err'] = gather_slabs(ks.last_error_vector(), cfg)
            res[name + '_rows'] = np.array(rows)
            ks.close()
        if rank == 0:
            np.savez(outfile, **res)
    finally:
        dist.destroy_process_group()


def test_groom_and_floor_count_on_two_slab_ranks(tmp_path):
    """the count of values below their floor goes through the all-reduce: both ranks take the same decision, and the new state's
    stale ghost rows are exchanged before anything reads them"""
    import torch.multiprocessing as mp
    outfile = str(tmp_path / 'result.npz')
    mp.spawn(_slab_worker, args=(2, _free_port(), outfile), nprocs=2, join=True)
    z = np.load(outfile)
    for s in range(3):
        assert np.array_equal(z['new_state%d' % s], z['old_state%d' % s]), s
    assert np.array_equal(z['new_err'], z['old_err'])
    assert np.array_equal(z['new_rows'][:, [0, 1, 2, 4, 5]], z['old_rows'][:, [0, 1, 2, 4, 5]])
    assert z['new_rows'][:, 4].all()


# ---- roll-back --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,nlig', GRIDS)
def test_rejected_single_attempt_leaves_the_groomed_state(shape, nlig):
    base = make_cfg(shape, nlig)
    u = smooth_state(base)
    cfg = make_cfg(shape, nlig, rhomin=float(np.percentile(u[:base.N], 30)))     # the one groom of the call has something to do
    tight = adaptive(atol=1e-9, rtol=1e-12, reserved=2)               # bit 1: one attempt per call
    vecs = []
    for tuning in (NEW, OLD):
        k = handle(cfg, tuning, u)
        t, hn, st, rc = k.step(0.0, 50.0, tight)
        assert not st.accepted and st.rejections == 1 and hn < 50.0 and t == 0.0
        assert np.array_equal(k.get_state(), ko.Oracle(cfg).groom(u))
        vecs.append((k.last_error_vector(), k.last_error_vector(), hn, st.wrms))     # rejected attempt: its vector, twice in a row
        k.close()
    assert np.array_equal(vecs[0][0], vecs[1][0]) and np.array_equal(vecs[0][1], vecs[1][1]) and np.array_equal(vecs[0][0], vecs[0][1])
    assert vecs[0][2:] == vecs[1][2:]


@pytest.mark.parametrize('shape,nlig', GRIDS)
def test_adaptive_step_with_rejections_matches_old_boundary(shape, nlig):
    cfg = make_cfg(shape, nlig)
    u = smooth_state(cfg)
    opts = adaptive(atol=1e-4, rtol=1e-8)
    new, old = handle(cfg, NEW, u), handle(cfg, OLD, u)
    a, b = run_steps(new, 2, opts, h=5.0), run_steps(old, 2, opts, h=5.0)
    same_steps(a, b)
    assert a[0][6] and a[0][5] >= 1, 'the first step was meant to be rejected at least once'
    assert np.array_equal(new.last_error_vector(), old.last_error_vector())
    new.close(), old.close()


@pytest.mark.parametrize('shape,nlig', GRIDS)
def test_failed_stage_solve_leaves_the_state(shape, nlig):
    cfg = make_cfg(shape, nlig)
    u = smooth_state(cfg)
    o = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12, ksp_max_it=1, pc_type=0)
    logs = []
    for tuning in (NEW, OLD):
        k = handle(cfg, tuning, u)
        t, hn, st, rc = k.step(0.0, 5.0, o, raise_on_error=False)
        assert rc == klib.ELINEAR and not st.accepted and t == 0.0
        assert np.array_equal(k.get_state(), ko.Oracle(cfg).groom(u))
        logs.append(run_steps(k, 1, adaptive()))                      # ... and the handle steps on from it
        k.close()
    same_steps(logs[0], logs[1])
    assert logs[0][0][6]


# ---- error vector -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('between', ['nothing', 'jvp', 'spectral_apply', 'velocity_max'])
@pytest.mark.parametrize('shape,nlig', GRIDS)
def test_error_vector_on_demand(shape, nlig, between):
    """after an accepted step, asked twice, with other entry points between the step and the query"""
    cfg = make_cfg(shape, nlig)
    u = smooth_state(cfg)
    v = np.random.default_rng(1).standard_normal(cfg.F * cfg.N)
    opts = adaptive()
    got = []
    for tuning in (NEW, OLD):
        k = handle(cfg, tuning, u)
        log = run_steps(k, 2, opts)
        assert log[-1][6]
        if between == 'jvp':
            k.jvp(v)
        elif between == 'spectral_apply':
            k.spectral_apply(3.0, v)
        elif between == 'velocity_max':
            k.velocity_max()
        got.append((k.last_error_vector(), k.last_error_vector(), log))
        k.close()
    same_steps(got[0][2], got[1][2])
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0], got[0][1])
    assert np.abs(got[0][0]).max() > 0.0
    # the vector is what the controller's norm was made of
    e, un = got[0][0], got[0][2][-1][0]
    wr = np.sqrt(np.mean((e / (0.01 + 1e-6 * np.maximum(np.abs(un), np.abs(un + e)))) ** 2))
    assert abs(wr - got[0][2][-1][3]) <= 1e-10 * wr


# ---- fp32 coefficient copy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,nlig', GRIDS)
def test_coef32_on_demand_serves_polynomial_and_fp32_cycle(shape, nlig):
    """two spectral steps (nobody reads the copy), then the polynomial preconditioner and the V cycle with fp32 level vectors read it"""
    cfg = make_cfg(shape, nlig)
    u = smooth_state(cfg)
    out = []
    for tuning in (NEW, OLD):
        k = handle(cfg, tuning, u)
        log = run_steps(k, 2, adaptive(pc_type=4))
        t, h = log[-1][1], log[-1][2]
        k.set_spectral_params(enable=0)
        poly = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-6, pc_type=3)
        t, hn, st, rc = k.step(t, 0.5, poly)
        assert st.pc_used & 4, 'the polynomial preconditioner was meant to run (pc_used %d)' % st.pc_used
        log.append((k.get_state(), t, hn, st.wrms, st.launches, st.rejections, st.accepted))
        mg = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-6, pc_type=1)
        t, hn, st, rc = k.step(t, 2.0, mg)
        assert st.pc_used & 2
        log.append((k.get_state(), t, hn, st.wrms, st.launches, st.rejections, st.accepted))
        out.append(log)
        k.close()
    same_steps(out[0], out[1])


# ---- stage-0 right-hand side with G from the coefficient planes -------------------------------------------------------------------
@pytest.mark.parametrize('shape,nlig', GRIDS)
def test_stage0_rhs_from_the_g_plane(shape, nlig):
    """1e-12: the bound of the operator goldens in tests/test_gpu_operators.py, which both ways of getting G must meet"""
    cfg = make_cfg(shape, nlig)
    u = smooth_state(cfg)
    opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12, ksp_max_it=4000)
    states = []
    for tuning in (klib.TUNE_FUSED, klib.TUNE_FUSED | klib.TUNE_NO_GPLANE):
        k = handle(cfg, tuning, u)
        t, hn, st, rc = k.step(0.0, 0.05, opts)
        assert st.accepted and st.rhs_evals == 4
        states.append(k.get_state())
        k.close()
    d = rel_l2(states[0], states[1])
    print('G plane on against off, %s x %d ligands: rel-L2 of the state %.3e%s' % (shape, nlig, d, ' (identical)' if d == 0.0 else ''))
    assert d <= 1e-12
