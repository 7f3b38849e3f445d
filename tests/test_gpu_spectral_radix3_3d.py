"""GPU: the 3-D spectral solver on boxes with 3 * 2^k extents (one rank): k_spec3_y_fwd / k_spec3_y_inv / k_spec3_z with a radix-3
axis (ksfd_amd/csrc/spectral.hip.h, template parameter R3).

As in test_gpu_spectral.py: (a) the operator against a numpy restatement (fftn + the closed-form arrow-block inverse) to fp32
accuracy, (b) whole implicit steps solved WITH it against the oracle to 1e-10.  The helpers are restated from there."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import rel_l2
from ksfd_amd import lib as klib
from ksfd_amd.config import ProblemConfig
from oracle import ko

pytestmark = pytest.mark.gpu
GAMMA = 4.3586652150845900e-01


def _sym_d2(n, h):
    th = 2 * np.pi * np.fft.fftfreq(n)
    return (-30 + 32 * np.cos(th) - 2 * np.cos(2 * th)) / (12 * h * h)


def _numpy_spectral3d(cfg, u, shift, v):
    """(shift I - J0)^-1 v with J0 from the grid means of rho*G_rho, rho*G_Ul (tophat cap), exact 4th-order symbol"""
    nx, ny, nz = cfg.n
    F, nl = cfg.F, cfg.nlig
    ug = np.maximum(u.reshape(F, nz, ny, nx), np.array([cfg.rhomin] + [cfg.Umin] * nl)[:, None, None, None])
    rho = ug[0]
    ms = cfg.maxscale * cfg.s2
    th = np.tanh((rho - cfg.rhomax) / cfg.cushion)
    a_rr = np.mean(rho * (cfg.s2 / rho + ms * (1 - th * th) / cfg.cushion))
    a_rU = []
    for l in range(nl):
        g = cfg.lig_group[l]
        ssum = cfg.grp_alpha[g] + sum(cfg.lig_w[m] * ug[m + 1] for m in range(nl) if cfg.lig_group[m] == g)
        a_rU.append(np.mean(rho * (-cfg.grp_beta[g] * cfg.lig_w[l] / ssum)))
    L2 = (_sym_d2(nx, cfg.L[0] / nx)[None, None, :] + _sym_d2(ny, cfg.L[1] / ny)[None, :, None] + _sym_d2(nz, cfg.L[2] / nz)[:, None, None])
    vh = np.fft.fftn(v.reshape(F, nz, ny, nx), axes=(1, 2, 3))
    d = [shift + cfg.lig_gamma[l] - cfg.lig_D[l] * L2 for l in range(nl)]
    den = shift - a_rr * L2 - sum(a_rU[l] * L2 * cfg.lig_s[l] / d[l] for l in range(nl))
    z0 = (vh[0] + sum(a_rU[l] * L2 / d[l] * vh[l + 1] for l in range(nl))) / den
    zs = [z0] + [(vh[l + 1] + cfg.lig_s[l] * z0) / d[l] for l in range(nl)]
    return np.real(np.fft.ifftn(np.array(zs), axes=(1, 2, 3))).reshape(-1)


def _many_ligands(dim, shape, L, nl):
    """nl ligands in three groups (fourier_series()-style expansions): exercises the larger symbol blocks"""
    rng = np.random.default_rng(100 + nl)
    return ProblemConfig(dim=dim, n=shape, L=L, lig_group=[l % 3 for l in range(nl)], lig_w=0.5 + rng.random(nl),
                         lig_s=0.005 + 0.01 * rng.random(nl), lig_gamma=0.005 + 0.01 * rng.random(nl), lig_D=1e-6 * (1 + rng.random(nl)),
                         grp_alpha=[1500.0, 1200.0, 1800.0], grp_beta=[5.56e-4, -3e-4, 2e-4])


def _state(cfg, seed, amp=90.0):
    rng = np.random.default_rng(seed)
    rho = 9000.0 + amp * rng.standard_normal(cfg.N)
    return np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] * (1 + 0.01 * rng.standard_normal(cfg.N)) for l in range(cfg.nlig)])


def _config(shape, nlig):
    L = tuple(n * 4.0 / 1536 for n in shape)
    return _many_ligands(len(shape), shape, L, nlig) if nlig > 2 else ProblemConfig.standard(len(shape), shape, L=L, nlig=nlig)


@pytest.mark.parametrize('shape,nlig', [
    # one radix-3 axis at a time, plan [3][16]
    ((48, 32, 32), 1), ((32, 48, 32), 1), ((32, 32, 48), 1),
    # plans [3][16,2] / [3][16,4], mixed with each other and with a 2^k axis that keeps its fused edge stage
    ((96, 48, 32), 2), ((32, 96, 192), 1), ((192, 32, 96), 2),
    # all three axes, with one, two and a run-time number of field pairs
    ((48, 48, 48), 1), ((48, 48, 48), 2), ((48, 48, 48), 4),
    # longer plans on one axis ([3][16,8], [3][16,16], [3][16,8,4]): the pb / cz / rb choices of spec_build3d
    ((32, 32, 384), 1), ((32, 768, 32), 1), ((32, 32, 1536), 1), ((1536, 32, 32), 1)])
@pytest.mark.parametrize('h', [0.02, 5.0])
def test_spectral_operator_3d_radix3_vs_numpy(shape, nlig, h):
    cfg = _config(shape, nlig)
    u = _state(cfg, 3)
    v = np.random.default_rng(4).standard_normal(u.size)
    shift = 1.0 / (GAMMA * h)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    got = k.spectral_apply(shift, v)
    k.close()
    err = rel_l2(got, _numpy_spectral3d(cfg, u, shift, v))
    print('rel_l2', shape, nlig, h, err)
    assert err < 2e-5              # fp32 FFTs and symbol; it is a preconditioner


def test_unfused_edge_stages_3d_radix3_give_the_same_operator():
    """(64, 48, 32): the y axis takes the generic staging paths whatever KSFD_SPEC_FUSE3 says, the z axis loses its fused edge stages
    with KSFD_SPEC_FUSE3=0 (read once per process, hence the child) -- a re-ordering of the same transforms, so not bitwise equal to
    the default run: the operator is compared with numpy."""
    shape, nlig = (64, 48, 32), 2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = _config(shape, nlig)
    u = _state(cfg, 3)
    v = np.random.default_rng(4).standard_normal(u.size)
    shift = 1.0 / (GAMMA * 0.02)
    code = '''
import sys, numpy as np
sys.path.insert(0, %r)
from ksfd_amd import lib as klib
from ksfd_amd.config import ProblemConfig
d = np.load(sys.argv[1])
shape = %r
cfg = ProblemConfig.standard(3, shape, L=tuple(n * 4.0 / 1536 for n in shape), nlig=%d)
k = klib.KSFDHip(cfg)
k.set_state(d['u'])
np.save(sys.argv[2], k.spectral_apply(float(d['shift']), d['v']))
k.close()
''' % (root, shape, nlig)
    res = {}
    with tempfile.TemporaryDirectory() as d:
        inp = os.path.join(d, 'in.npz')
        np.savez(inp, u=u, v=v, shift=shift)
        for name, extra in (('default', {}), ('unfused', {'KSFD_SPEC_FUSE3': '0'})):
            out = os.path.join(d, name + '.npy')
            r = subprocess.run([sys.executable, '-c', code, inp, out], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=200)
            assert r.returncode == 0, r.stderr[-1500:]
            res[name] = np.load(out)
    want = _numpy_spectral3d(cfg, u, shift, v)
    for name in res:
        err = rel_l2(res[name], want)
        print('rel_l2', name, err)
        assert err < 2e-5


_ORACLE_STEPS = {}


def _oracle_step(shape):
    """one fixed step h = 0.1 by the oracle (GMRES to 1e-13: a few hundred iterations on the host), once per shape"""
    if shape not in _ORACLE_STEPS:
        cfg = _config(shape, 1)
        u = _state(cfg, 9)
        un, err, wr, _ = ko.Oracle(cfg).rosw_step(u, 0.1, 0.01, 1e-6, solver='gmres', ksp_rtol=1e-13, maxit=4000)
        un.setflags(write=False)
        _ORACLE_STEPS[shape] = (cfg, u, un)
    return _ORACLE_STEPS[shape]


@pytest.mark.parametrize('shape', [(48, 32, 32), (32, 48, 32), (32, 32, 48)])
@pytest.mark.parametrize('pc', [4, 2])
def test_step_3d_radix3_with_spectral_solver_vs_oracle(shape, pc):
    cfg, u, un = _oracle_step(shape)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    t, hn, st, rc = k.step(0.0, 0.1, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-12, pc_type=pc))
    state = k.get_state()
    k.close()
    print('step', shape, pc, st.pc_used, st.linear_its, rel_l2(state, un))
    assert st.pc_used & klib.PC_SPECTRAL
    assert st.linear_its <= 4 * 18, st.linear_its
    assert rel_l2(state, un) < 1e-10


@pytest.mark.parametrize('dim,shape', [(3, (40, 32, 32)), (1, (96,))])
def test_spectral_unavailable_is_still_reported(dim, shape):
    """unchanged refusals: a 3-D extent without a plan (40 = 5 * 8), and 1-D grids -- spectral_apply raises, pc_type 4 steps without it"""
    cfg = ProblemConfig.standard(dim, shape, L=tuple(n * 4.0 / 1536 for n in shape))
    k = klib.KSFDHip(cfg)
    k.set_state(_state(cfg, 1))
    with pytest.raises(klib.KSFDError):
        k.spectral_apply(1.0, np.zeros(cfg.F * cfg.N))
    t, h, st, rc = k.step(0.0, 0.05, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, pc_type=4))
    assert st.accepted and not (st.pc_used & klib.PC_SPECTRAL)
    k.close()
