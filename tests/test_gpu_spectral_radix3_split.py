"""GPU: the two-phase ("split") column kernel of the 2-D spectral solver on column extents 3 * 2^k (one rank): k_spec_cols_split<true>
(ksfd_amd/csrc/spectral.hip.h).  Real sizes that need it (columns of 12288 points; 6144 rows x 3 fields) and, through KSFD_SPEC_SPLIT,
both variants on small grids.  Helpers restated from test_gpu_spectral.py; the body is that of
test_spectral_split_column_kernel_vs_numpy."""
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


def _numpy_spectral(cfg, u, shift, v):
    """(shift I - J0)^-1 v with J0 from the grid means of rho*G_rho, rho*G_Ul (tophat cap), exact 4th-order symbol"""
    nx, ny = cfg.n[0], cfg.n[1]
    F, nl = cfg.F, cfg.nlig
    ug = np.maximum(u.reshape(F, ny, nx), np.array([cfg.rhomin] + [cfg.Umin] * nl)[:, None, None])
    rho = ug[0]
    ms = cfg.maxscale * cfg.s2
    th = np.tanh((rho - cfg.rhomax) / cfg.cushion)
    a_rr = np.mean(rho * (cfg.s2 / rho + ms * (1 - th * th) / cfg.cushion))
    a_rU = []
    for l in range(nl):
        g = cfg.lig_group[l]
        ssum = cfg.grp_alpha[g] + sum(cfg.lig_w[m] * ug[m + 1] for m in range(nl) if cfg.lig_group[m] == g)
        a_rU.append(np.mean(rho * (-cfg.grp_beta[g] * cfg.lig_w[l] / ssum)))
    L2 = _sym_d2(nx, cfg.L[0] / nx)[None, :] + _sym_d2(ny, cfg.L[1] / ny)[:, None]
    vh = np.fft.fft2(v.reshape(F, ny, nx))
    d = [shift + cfg.lig_gamma[l] - cfg.lig_D[l] * L2 for l in range(nl)]
    den = shift - a_rr * L2 - sum(a_rU[l] * L2 * cfg.lig_s[l] / d[l] for l in range(nl))
    z0 = (vh[0] + sum(a_rU[l] * L2 / d[l] * vh[l + 1] for l in range(nl))) / den
    zs = [z0] + [(vh[l + 1] + cfg.lig_s[l] * z0) / d[l] for l in range(nl)]
    return np.real(np.fft.ifft2(np.array(zs))).reshape(-1)


def _lu_step(cfg, u, h, atol=0.01, rtol=1e-6):
    """one RA34PW2 step with the oracle's operators and an exact SPARSE LU of shift*I - J; returns (unew, wrms)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    o = ko.Oracle(cfg)
    At, Gi, bt, b2t, asum = ko.tableau()
    gam = 1.0 / Gi[0, 0]
    F, N = cfg.F, cfg.N
    to_vec = lambda a: a.reshape(F, N).T.reshape(-1)
    to_soa = lambda x: x.reshape(N, F).T.reshape(-1)
    ug = o.groom(u)
    rp, col, val = o.jacobian_csr(ug)
    J = sp.csr_matrix((val, col, rp), shape=(F * N, F * N))
    lu = spla.splu((sp.identity(F * N, format='csc') / (gam * h) - J).tocsc())
    Y = []
    for i in range(4):
        Z = ug + sum(At[i, j] * Y[j] for j in range(i))
        Zdot = sum((Gi[i, j] / h) * Y[j] for j in range(i)) if i else 0.0
        Y.append(to_soa(lu.solve(to_vec(o.rhs(Z) - Zdot))))
    unew = ug + sum(bt[j] * Y[j] for j in range(4))
    err = sum((b2t[j] - bt[j]) * Y[j] for j in range(4))
    return unew, ko.wrms(unew, err, atol, rtol)


def _three_ligands(shape, L):
    """two ligands sharing group 0 (weights) + a repellent in its own group: F = 4 -> two complex pairs"""
    return ProblemConfig(dim=2, n=shape, L=L, lig_group=[0, 0, 1], lig_w=[1.0, 0.5, 1.0], lig_s=[0.01, 0.02, 0.001],
                         lig_gamma=[0.01, 0.03, 0.001], lig_D=[1e-6, 3e-6, 1e-5], grp_alpha=[1500.0, 1500.0],
                         grp_beta=[5.56e-4, -5.56e-4])


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


@pytest.mark.parametrize('shape,nlig,forced', [
    # real sizes, no knob: columns of 12288 points (one column per block); rows of 12288 points (one row per block of the row
    # kernels); 6144 rows x 3 fields = 209 KB for a block's four columns (one field pair per block)
    ((32, 12288), 1, 0), ((12288, 32), 1, 0), ((32, 6144), 2, 0),
    # forced on small 3 * 2^k grids: one field pair per block with 2 and 3 field pairs ...
    ((64, 96), 2, 1), ((96, 48), 3, 1), ((48, 192), 5, 1),
    # ... and one column per block with 1, 2 and 3 field pairs
    ((64, 96), 1, 2), ((96, 48), 2, 2), ((48, 96), 3, 2), ((32, 384), 5, 2)])
def test_spectral_split_column_kernel_radix3_vs_numpy(shape, nlig, forced, monkeypatch):
    if forced:
        monkeypatch.setenv('KSFD_SPEC_SPLIT', str(forced))
    L = tuple(n * 4.0 / 1536 for n in shape)
    cfg = _three_ligands(shape, L) if nlig == 3 else _many_ligands(2, shape, L, nlig) if nlig > 3 else ProblemConfig.standard(2, shape, L=L, nlig=nlig)
    u = _state(cfg, 3)
    v = np.random.default_rng(4).standard_normal(u.size)
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    for h in (0.02, 5.0):
        shift = 1.0 / (GAMMA * h)
        err = rel_l2(k.spectral_apply(shift, v), _numpy_spectral(cfg, u, shift, v))
        print('rel_l2', shape, nlig, forced, h, err)
        assert err < 2e-5
    # and through a whole step (defect correction on top of it), against the sparse-LU step where that is small enough
    t, hn, st, rc = k.step(0.0, 0.3, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, ksp_rtol=1e-11, pc_type=4))
    assert st.pc_used & 8
    if cfg.N <= 64 * 128:
        un, _ = _lu_step(cfg, u, 0.3, 0.01, 1e-6)
        err = rel_l2(k.get_state(), un)
        print('step', shape, nlig, forced, err)
        assert err < 1e-9
    k.close()
