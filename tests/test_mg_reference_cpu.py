"""CPU: the numpy reference of the multigrid V cycle (tests/mg_reference.py) checked against facts that do not depend on it: the
variational pair R = P^T / 2^dim, what P and R do to constants, linear functions and the mean, the symbol of the 4th-order star, numpy's own
Chebyshev polynomials, the point blocks against the dense operator, and float64 against longdouble.  tests/test_gpu_mg_parts.py compares the
HIP kernels with this reference."""
import numpy as np
import pytest

import mg_reference as mr
from ksfd_amd.config import ProblemConfig
from oracle import ko

GAMMA = 0.43586652150845900
EPS = np.finfo(float).eps
LD = np.longdouble


def synthetic_levels(n, nlig, seed, dtype=np.float64):
    """coefficient planes of a diffusion-dominated state on the grid n and its coarsenings (full weighting, spacings doubled), with inverse
    point blocks, a power-iteration bound and a coarse interval: everything a cycle needs, made by the reference alone"""
    rng = np.random.default_rng(seed)
    dim = len(n)
    shp = mr.grid_shape(n)
    rho = 9000.0 * (1.0 + 0.01 * rng.standard_normal(shp))
    planes = [rho, 1e-7 * rng.standard_normal(shp), 1e-8 * (1.0 + 0.1 * rng.standard_normal(shp))]
    planes += [-1e-9 * (1.0 + 0.1 * rng.standard_normal(shp)) for _ in range(nlig)]
    C = np.stack(planes).astype(dtype)
    lig = dict(s=[0.01, 0.001, 0.003][:nlig], gamma=[0.01, 0.001, 0.004][:nlig], D=[1e-6, 1e-5, 3e-6][:nlig])
    h = [0.0025] * dim
    levels = []
    while True:
        levels.append(mr.Level(C, h))
        if any(x % 2 or x // 2 < 8 for x in C.shape[1:]):
            break
        C, h = mr.restrict(C, dim), [2 * x for x in h]
    return levels, lig


def set_up(levels, lig, shift, seed=1):
    rng = np.random.default_rng(seed)
    for L in levels:
        L.Dinv = mr.block_inverse(mr.block_diag(L.C, L.h, lig, shift))
        F = L.Dinv.shape[-1]
        v = rng.standard_normal((F,) + L.C.shape[1:]).astype(L.C.dtype)
        lam = 0.0
        for _ in range(12):
            w = mr.dinv_apply(L.Dinv, mr.op_apply(L.C, v, L.h, lig, shift))
            lam = float(np.linalg.norm(w.ravel()) / np.linalg.norm(v.ravel()))
            v = w / np.linalg.norm(w.ravel())
        L.lam_max, L.ratio, L.sweeps = 1.15 * lam, 30.0, 8


# ---- transfer operators -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [(16,), (8,), (12, 8), (16, 10), (8, 8, 8), (10, 8, 12)])
def test_restriction_is_the_scaled_transpose_of_prolongation(n):
    dim = len(n)
    nc = tuple(x // 2 for x in n)
    R = mr.transfer_matrix(mr.restrict, n, dim)
    P = mr.transfer_matrix(mr.prolong, nc, dim)
    assert R.shape == (int(np.prod(nc)), int(np.prod(n))) and P.shape == R.shape[::-1]
    assert np.array_equal(R, P.T / 2 ** dim)            # every weight is a power of two: exact
    assert np.array_equal(R.sum(axis=1), np.ones(R.shape[0])) and np.array_equal(P.sum(axis=1), np.ones(P.shape[0]))


@pytest.mark.parametrize('n', [(16,), (12, 8), (8, 10, 12)])
def test_prolongation_reproduces_constants_and_linear_functions(n):
    dim = len(n)
    nc = tuple(x // 2 for x in n)
    shp, shc = mr.grid_shape(n), mr.grid_shape(nc)
    assert np.array_equal(mr.prolong(np.full((1,) + shc, 3.25), dim), np.full((1,) + shp, 3.25))
    # f = sum_a (a + 2) * i_a with integer values: interpolation is exact away from the last point of each axis, where the ring closes
    idx_c = np.meshgrid(*[np.arange(m) for m in shc], indexing='ij')
    idx_f = np.meshgrid(*[np.arange(m) for m in shp], indexing='ij')
    fc = sum((q + 2.0) * 2.0 * i for q, i in enumerate(idx_c))
    ff = sum((q + 2.0) * i for q, i in enumerate(idx_f))
    got = mr.prolong(fc[None], dim)[0]
    inner = tuple(slice(0, m - 1) for m in shp)
    assert np.array_equal(got[inner], ff[inner])
    assert not np.array_equal(got, ff)                   # ... and not at the wrap: the ring is closed, not extrapolated


@pytest.mark.parametrize('n', [(16,), (12, 8), (8, 10, 12)])
def test_restriction_preserves_the_mean(n):
    dim = len(n)
    v = np.random.default_rng(2).standard_normal((2,) + mr.grid_shape(n)).astype(LD)
    r = mr.restrict(v, dim)
    for c in range(2):
        assert abs(r[c].mean() - v[c].mean()) <= 8 * np.finfo(LD).eps * np.abs(v[c]).mean()


# ---- operator -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,nlig', [((16,), 1), ((12, 8), 2), ((8, 10, 12), 1)])
def test_operator_on_constant_planes_is_the_symbol_of_the_star(n, nlig):
    """constant rho, G, G_rho, G_U: J is block-circulant, and on v = c * cos(k.x) it acts by the 2 x 2 (F x F) symbol
       [[rho G_rho s(k), rho G_U s(k)], [s_l, -gamma_l + D_l s(k)]] with s(k) the symbol of the 4th-order Laplacian star"""
    dim, F = len(n), nlig + 1
    shp = mr.grid_shape(n)
    h = [0.01, 0.02, 0.015][:dim]
    lig = dict(s=[0.01, 0.001][:nlig], gamma=[0.01, 0.001][:nlig], D=[1e-6, 1e-5][:nlig])
    rho, grho, gu = 9000.0, 2e-8, [-1e-6, 3e-7][:nlig]
    C = np.stack([np.full(shp, x) for x in [rho, 0.37, grho] + gu]).astype(LD)
    for k in [(1, 2, 3)[:dim], (0, 3, 1)[:dim], tuple(m // 2 for m in n)]:
        theta = [2.0 * np.pi * kk / m for kk, m in zip(k, n)]
        idx = np.meshgrid(*[np.arange(m) for m in shp], indexing='ij')
        phase = sum(t * idx[dim - 1 - a] for a, t in enumerate(theta))
        mode = np.cos(phase).astype(LD)
        amp = np.array([1.0, -0.5, 2.0][:F])
        v = np.stack([a * mode for a in amp])
        s = mr.star_symbol(theta, h)
        S = np.zeros((F, F))
        S[0, 0] = rho * grho * s
        for l in range(nlig):
            S[0, 1 + l] = rho * gu[l] * s
            S[1 + l, 0] = lig['s'][l]
            S[1 + l, 1 + l] = -lig['gamma'][l] + lig['D'][l] * s
        want = np.stack([c * mode for c in S @ amp])
        got = mr.jac_apply(C, v, h, lig)
        scale = np.abs(S).max() * np.abs(amp).max()
        assert np.abs(got - want).max() <= 64 * EPS * scale, (k, float(np.abs(got - want).max()), scale)     # the symbol itself is float64


def test_point_blocks_are_the_diagonal_blocks_of_the_dense_operator():
    levels, lig = synthetic_levels((8, 10), 2, 3, LD)
    L, F, shift = levels[0], 3, 7.5
    A = mr.dense_operator(L.C, L.h, lig, shift, F)
    M = mr.block_diag(L.C, L.h, lig, shift)
    N = A.shape[0] // F
    blocks = np.array([[[A[r * N + p, c * N + p] for c in range(F)] for r in range(F)] for p in range(N)]).reshape(L.C.shape[1:] + (F, F))
    assert np.abs(blocks - M).max() <= 16 * np.finfo(LD).eps * np.abs(M).max()
    X = mr.block_inverse(M)
    eye = np.einsum('...ij,...jk->...ik', M, X)
    assert np.all(np.abs(eye - np.eye(F)) <= 64 * np.finfo(LD).eps * np.einsum('...ij,...jk->...ik', np.abs(M), np.abs(X)))     # the blocks are badly scaled
    assert np.array_equal(mr.planes_to_blocks(mr.blocks_to_planes(X), F), X)


# ---- smoother -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nu', [1, 2, 3, 5])
@pytest.mark.parametrize('guess', [False, True])
def test_chebyshev_smoother_is_numpys_chebyshev_polynomial(nu, guess):
    """on A = diag(lambda), Dinv = I the error obeys e_nu = T_nu((theta - lambda) / delta) / T_nu(theta / delta) e_0"""
    lam = np.linspace(0.05, 2.4, 40).astype(LD)
    lam_max, ratio = 2.2, 6.0
    rng = np.random.default_rng(nu)
    b = rng.standard_normal((1, 40)).astype(LD)
    x0 = rng.standard_normal((1, 40)).astype(LD) if guess else None
    Dinv = np.ones((40, 1, 1), dtype=LD)
    x = mr.cheb_smooth(lambda v: lam * v, Dinv, b, x0, nu, lam_max, ratio)
    xs = b / lam
    e0 = (x0 if guess else 0.0) - xs
    p = mr.cheb_residual_polynomial(nu, lam_max, ratio)(lam.astype(np.float64))
    assert np.abs((x - xs) - p * e0).max() <= 256 * EPS * np.abs(e0).max() * max(1.0, np.abs(p).max())


# ---- cycle --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,nlig,exact', [((32,), 1, False), ((16, 16), 2, False), ((16, 16), 1, True), ((16, 16, 16), 1, False)])
def test_cycle_in_float64_and_longdouble_agree_to_rounding(n, nlig, exact):
    """32 x 1e-12: the budget tests/test_gpu_mg_parts.py gives the kernels relative to the operator tolerance; the reference must not need it"""
    lv64, lig = synthetic_levels(n, nlig, 5)
    assert len(lv64) >= 2
    shift = 1.0 / (GAMMA * 5.0)
    set_up(lv64, lig, shift)
    lvld = [L.astype(LD) for L in lv64]
    b = np.random.default_rng(6).standard_normal((nlig + 1,) + mr.grid_shape(n))
    x64 = mr.vcycle(lv64, lig, shift, b, 2, 6.0, exact=exact)
    xld = mr.vcycle(lvld, lig, shift, b.astype(LD), 2, 6.0, exact=exact)
    assert xld.dtype == LD and x64.dtype == np.float64
    d = mr.rel_l2(x64, xld)
    print('reference cycle %s F=%d exact=%s: float64 vs longdouble %.3e' % (n, nlig + 1, exact, d))
    assert 0.0 < d < 32e-12
    # the cycle reduces the error of A x = b: it is a preconditioner, not noise
    A = lambda v: mr.op_apply(lvld[0].C, v, lvld[0].h, lig, shift)
    assert np.linalg.norm((b - A(xld)).ravel()) < 0.7 * np.linalg.norm(b.ravel())
    # fp32 level vectors: a perturbation of float32 size, and nothing else
    x32 = mr.vcycle(lv64, lig, shift, b, 2, 6.0, exact=exact, store=mr.store_f32, nstore=len(lv64) - 1)
    d32 = mr.rel_l2(x32, x64)
    assert 1e-9 < d32 < 1e-5, d32


# ---- shifts of the DINV test -----------------------------------------------------------------------------------------------------------
def _cfg(shape, nlig):
    dim = len(shape)
    L = tuple(0.0025 * n for n in shape)
    if nlig <= 2:
        return ProblemConfig.standard(dim, shape, L=L, nlig=nlig)
    return ProblemConfig(dim=dim, n=shape, L=L, lig_group=[0, 1, 0][:nlig], lig_w=[1.0, 1.0, 0.5][:nlig], lig_s=[0.01, 0.001, 0.003][:nlig],
                         lig_gamma=[0.01, 0.001, 0.004][:nlig], lig_D=[1e-6, 1e-5, 3e-6][:nlig], grp_alpha=[1500.0, 1500.0],
                         grp_beta=[5.56e-4, -5.56e-4])


@pytest.mark.parametrize('shape,nlig', [((32, 32), 1), ((64, 48), 2), ((40, 24), 3), ((16, 16, 16), 1), ((96,), 1), ((130,), 2)])
def test_point_blocks_of_the_test_states_are_well_conditioned(shape, nlig):
    """tests/test_gpu_mg_parts.py compares k_blockdiag_inv (Gauss-Jordan without pivoting, fp32 result) with float32(numpy.linalg.inv) to one
    ulp, which needs cond <= 1e6 of every block: checked here at level 0 on the point blocks of the oracle's assembled Jacobian, for the states
    and the two shifts that test uses; the GPU test repeats it on every level with the reference blocks."""
    import scipy.sparse as sp
    cfg = _cfg(shape, nlig)
    rng = np.random.default_rng(3)
    rho = 9000.0 * (1.0 + 0.05 * rng.standard_normal(cfg.N))
    u = np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(cfg.nlig)])
    rp, col, val = ko.Oracle(cfg).jacobian_csr(u)
    J = sp.csr_matrix((val, col, rp)).tocsr()
    F = cfg.F
    blocks = np.stack([J[F * p:F * p + F, F * p:F * p + F].toarray() for p in range(cfg.N)])
    for hstep in (0.05, 50.0):
        shift = 1.0 / (GAMMA * hstep)
        cond = np.linalg.cond(shift * np.eye(F) - blocks)
        assert cond.max() <= 1e6, (hstep, float(cond.max()))
