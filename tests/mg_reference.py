"""Plain numpy reference of the geometric multigrid V cycle of csrc/mg.hip.h, part by part.  Matrix-free on periodic arrays (np.roll), 1-, 2-
and 3-D, generic in the dtype: the same code runs in float64 and in np.longdouble, and the distance between the two is the rounding error
of the reference itself (tests/test_mg_reference_cpu.py, tests/test_gpu_mg_parts.py).

Arrays: a level vector is (planes, *grid) with grid = the extents slowest first ((ny, nx) in 2-D, (nz, ny, nx) in 3-D), so that
a.reshape(planes, -1) is the SoA layout of the library (x fastest).  Spacings h = (hx, hy, hz)[:dim]; axis a of the library is numpy axis
-(a + 1).  Nothing here is transcribed from the strip kernels: the Jacobian action is written from the formula the assembled-Jacobian
export (k_jac_csr) and k_blockdiag_inv document,

    (J v)_rho = sum_a D1a(v_rho) D1a(G) + v_rho lap(G) + sum_a D1a(rho) D1a(e) + rho lap(e),   e = G_rho v_rho + sum_l G_Ul v_Ul
    (J v)_Ul  = -gamma_l v_Ul + s_l v_rho + D_l lap(v_Ul)

with the 4th-order central differences D1 = (8 (f[+1] - f[-1]) - (f[+2] - f[-2])) / (12 h), D2 = (16 (f[+1] + f[-1]) - (f[+2] + f[-2]) -
30 f[0]) / (12 h^2), and coefficient planes C = [rho, G, G_rho, G_U1, ...]."""
import numpy as np


def grid_shape(n):
    """numpy shape of a grid with extents n = (nx[, ny[, nz]])"""
    return tuple(int(x) for x in reversed(n))


def _ax(a):
    return -(a + 1)


# ---- transfer operators -----------------------------------------------------------------------------------------------------------
def restrict(v, dim):
    """full weighting, weights (1/4, 1/2, 1/4) per axis, coarse point I at fine point 2 I; every extent even"""
    for a in range(dim):
        ax = _ax(a)
        even = [slice(None)] * v.ndim
        even[ax] = slice(0, None, 2)
        even = tuple(even)
        v = v.dtype.type(0.5) * v[even] + v.dtype.type(0.25) * (np.roll(v, 1, ax)[even] + np.roll(v, -1, ax)[even])
    return v


def prolong(c, dim):
    """linear / bilinear / trilinear interpolation: fine 2 I = coarse I, fine 2 I + 1 = mean of coarse I and I + 1 (periodic), per axis"""
    for a in range(dim):
        ax = _ax(a)
        shp = list(c.shape)
        shp[ax] *= 2
        f = np.empty(shp, dtype=c.dtype)
        ev, od = [slice(None)] * c.ndim, [slice(None)] * c.ndim
        ev[ax], od[ax] = slice(0, None, 2), slice(1, None, 2)
        f[tuple(ev)] = c
        f[tuple(od)] = c.dtype.type(0.5) * (c + np.roll(c, -1, ax))
        c = f
    return c


def transfer_matrix(fn, n_in, dim, dtype=np.float64):
    """dense matrix of a transfer operator on a grid with extents n_in (columns = unit vectors)"""
    shp = grid_shape(n_in)
    N = int(np.prod(shp))
    cols = []
    for j in range(N):
        e = np.zeros(N, dtype=dtype)
        e[j] = 1
        cols.append(fn(e.reshape((1,) + shp), dim).reshape(-1))
    return np.stack(cols, axis=1)


# ---- the frozen Jacobian action ------------------------------------------------------------------------------------------------------
def d1(f, a, h):
    ax, t = _ax(a), f.dtype.type
    return (t(8) * (np.roll(f, -1, ax) - np.roll(f, 1, ax)) - (np.roll(f, -2, ax) - np.roll(f, 2, ax))) / (t(12) * t(h))


def d2(f, a, h):
    ax, t = _ax(a), f.dtype.type
    return (t(16) * (np.roll(f, -1, ax) + np.roll(f, 1, ax)) - (np.roll(f, -2, ax) + np.roll(f, 2, ax)) - t(30) * f) / (t(12) * t(h) * t(h))


def lap(f, h):
    return sum(d2(f, a, h[a]) for a in range(len(h)))


def star_symbol(theta, h):
    """symbol of the 4th-order Laplacian star on the mode with phase advance theta[a] per point along axis a"""
    return sum((32.0 * np.cos(t) - 2.0 * np.cos(2.0 * t) - 30.0) / (12.0 * ha * ha) for t, ha in zip(theta, h))


def jac_apply(C, v, h, lig):
    """J v at the frozen planes C = [rho, G, G_rho, G_U1..] ((3 + nlig, *grid)); v (F, *grid); lig = dict(s, gamma, D) of sequences"""
    t = v.dtype.type
    dim, nl = len(h), v.shape[0] - 1
    rho, G = C[0], C[1]
    e = C[2] * v[0]
    for l in range(nl):
        e = e + C[3 + l] * v[1 + l]
    out = np.empty_like(v)
    acc = v[0] * lap(G, h) + rho * lap(e, h)
    for a in range(dim):
        acc = acc + d1(v[0], a, h[a]) * d1(G, a, h[a]) + d1(rho, a, h[a]) * d1(e, a, h[a])
    out[0] = acc
    for l in range(nl):
        out[1 + l] = -t(lig['gamma'][l]) * v[1 + l] + t(lig['s'][l]) * v[0] + t(lig['D'][l]) * lap(v[1 + l], h)
    return out


def op_apply(C, v, h, lig, shift):
    """(shift I - J) v"""
    return v.dtype.type(shift) * v - jac_apply(C, v, h, lig)


def dense_operator(C, h, lig, shift, F):
    """dense shift I - J on one level (small levels only), unknowns in SoA order"""
    shp = C.shape[1:]
    N = F * int(np.prod(shp))
    A = np.empty((N, N), dtype=C.dtype)
    e = np.zeros(N, dtype=C.dtype)
    for j in range(N):
        e[j] = 1
        A[:, j] = op_apply(C, e.reshape((F,) + shp), h, lig, shift).reshape(-1)
        e[j] = 0
    return A


# ---- point-block diagonal -----------------------------------------------------------------------------------------------------------
def block_diag(C, h, lig, shift):
    """the F x F point blocks of shift I - J, (*grid, F, F):
       D_rr = shift - (lap G + rho G_rho c2), D_rUl = -rho G_Ul c2, D_Ulr = -s_l, D_UlUl = shift + gamma_l - D_l c2, c2 = sum_a -30/(12 h_a^2)"""
    t = C.dtype.type
    nl = C.shape[0] - 3
    c2 = sum(t(-30) / (t(12) * t(ha) * t(ha)) for ha in h)
    M = np.zeros(C.shape[1:] + (nl + 1, nl + 1), dtype=C.dtype)
    M[..., 0, 0] = t(shift) - (lap(C[1], h) + C[0] * C[2] * c2)
    for l in range(nl):
        M[..., 0, 1 + l] = -C[0] * C[3 + l] * c2
        M[..., 1 + l, 0] = -t(lig['s'][l])
        M[..., 1 + l, 1 + l] = t(shift) + t(lig['gamma'][l]) - t(lig['D'][l]) * c2
    return M


def block_inverse(M):
    """inverse of every point block in the dtype of M (numpy.linalg in float64, then Newton steps X <- X (2 I - M X) in the dtype)"""
    X = np.linalg.inv(M.astype(np.float64)).astype(M.dtype)
    if M.dtype != np.float64:
        I2 = 2 * np.eye(M.shape[-1], dtype=M.dtype)
        for _ in range(2):
            X = np.einsum('...ij,...jk->...ik', X, I2 - np.einsum('...ij,...jk->...ik', M, X))
    return X


def planes_to_blocks(P, F):
    """(F*F, *grid) row-major planes -> (*grid, F, F)"""
    return np.moveaxis(P.reshape((F, F) + P.shape[1:]), (0, 1), (-2, -1))


def blocks_to_planes(B):
    F = B.shape[-1]
    return np.moveaxis(B, (-2, -1), (0, 1)).reshape((F * F,) + B.shape[:-2])


def dinv_apply(Dinv, r):
    """Dinv (*grid, F, F) times r (F, *grid)"""
    return np.einsum('...ac,c...->a...', Dinv, r)


# ---- Chebyshev smoother, textbook three-term form ---------------------------------------------------------------------------------------
def cheb_smooth(A, Dinv, b, x0, nu, lam_max, ratio, store=None):
    """nu steps of the Chebyshev iteration for Dinv A x = Dinv b on the interval [lam_max / ratio, lam_max] (Saad, Iterative Methods,
    Alg. 12.1): theta = centre, delta = half width, sigma = theta / delta; x0 = None: zero guess.  store: rounding applied to r, d and x
    wherever they are formed (the level vectors of the fp32 cycle)."""
    t = b.dtype.type
    st = store if store is not None else (lambda a: a)
    lmax, lmin = t(lam_max), t(lam_max) / t(ratio)
    theta, delta = (lmax + lmin) / t(2), (lmax - lmin) / t(2)
    sigma = theta / delta
    rho = t(1) / sigma
    if x0 is None:
        x, r = np.zeros_like(b), st(b)
    else:
        x = x0
        r = st(b - A(x))
    d = st(dinv_apply(Dinv, r) / theta)
    for k in range(nu):
        x = st(x + d)
        if k == nu - 1:
            break
        r = st(r - A(d))
        rho_new = t(1) / (t(2) * sigma - rho)
        d = st(rho_new * rho * d + (t(2) * rho_new / delta) * dinv_apply(Dinv, r))
        rho = rho_new
    return x


def cheb_residual_polynomial(nu, lam_max, ratio):
    """the residual polynomial of cheb_smooth as a numpy Chebyshev series in the mapped variable s = (theta - lambda) / delta:
    T_nu(s) / T_nu(sigma)"""
    from numpy.polynomial import chebyshev as Ch
    lmin = lam_max / ratio
    theta, delta = 0.5 * (lam_max + lmin), 0.5 * (lam_max - lmin)
    c = np.zeros(nu + 1)
    c[nu] = 1.0
    return lambda lam: Ch.chebval((theta - lam) / delta, c) / Ch.chebval(theta / delta, c)


# ---- the V cycle ------------------------------------------------------------------------------------------------------------------------
class Level:
    """one level: coefficient planes C, spacings h, inverse point blocks Dinv (*grid, F, F), Chebyshev bound lam_max, and on the level
    the cycle ends on the coarse interval ratio and sweep count"""

    def __init__(self, C, h, Dinv=None, lam_max=None, ratio=None, sweeps=None):
        self.C, self.h, self.Dinv, self.lam_max, self.ratio, self.sweeps = C, tuple(h), Dinv, lam_max, ratio, sweeps

    def astype(self, dt):
        return Level(self.C.astype(dt), self.h, None if self.Dinv is None else self.Dinv.astype(dt), self.lam_max, self.ratio, self.sweeps)


def vcycle(levels, lig, shift, b, nu, mg_ratio, l=0, end=None, exact=False, store=None, nstore=0):
    """recursive V(nu, nu) cycle from a zero guess.  The cycle ends on level `end` (default: the last) with sweeps Chebyshev steps over
    [lam_max / ratio, lam_max], or with an exact solve (dense, small levels).  store / nstore: rounding of x, b, r, d on levels
    0 .. nstore - 1 (the fp32 cycle); below them nothing is rounded."""
    end = len(levels) - 1 if end is None else end
    L = levels[l]
    dim = len(L.h)
    A = lambda v: op_apply(L.C, v, L.h, lig, shift)
    st = store if (store is not None and l < nstore) else None
    rnd = st if st is not None else (lambda a: a)
    if l == end:
        if exact:
            F = b.shape[0]
            key = (float(shift), b.dtype.str)
            if getattr(L, 'dense', None) is None or L.dense[0] != key:       # assembled and factored once per level, shift and dtype
                from scipy.linalg import lu_factor
                M = dense_operator(L.C, L.h, lig, shift, F)
                L.dense = (key, M, lu_factor(M.astype(np.float64)))
            from scipy.linalg import lu_solve
            _, M, lu = L.dense
            x = lu_solve(lu, b.reshape(-1).astype(np.float64)).astype(b.dtype)
            for _ in range(2):      # refinement in the working dtype
                x = x + lu_solve(lu, (b.reshape(-1) - M @ x).astype(np.float64)).astype(b.dtype)
            return x.reshape(b.shape)
        return cheb_smooth(A, L.Dinv, b, None, L.sweeps, L.lam_max, L.ratio)
    b = rnd(b)
    x = cheb_smooth(A, L.Dinv, b, None, nu, L.lam_max, mg_ratio, st)
    r = rnd(b - A(x))
    nxt = store if (store is not None and l + 1 < nstore) else (lambda a: a)
    xc = vcycle(levels, lig, shift, nxt(restrict(r, dim)), nu, mg_ratio, l + 1, end, exact, store, nstore)
    x = rnd(x + prolong(xc, dim))
    # the last smoothing step of level 0 leaves its result in the caller's precision
    x = cheb_smooth(A, L.Dinv, b, x, nu, L.lam_max, mg_ratio, st if l > 0 else _last_exact(st, nu))
    return x


def _last_exact(st, nu):
    """store for the post-smoothing of level 0: every rounding but the one of the last x"""
    if st is None:
        return None
    # cheb_smooth calls store for r, d, then per step for x and (all steps but the last) for r, d: the last call is the last x
    calls, total = {'n': 0}, 2 + nu + 2 * (nu - 1)

    def g(a):
        calls['n'] += 1
        return a if calls['n'] == total else st(a)
    return g


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).reshape(-1).astype(np.longdouble)) / np.linalg.norm(b.reshape(-1).astype(np.longdouble)))


def store_f32(a):
    """round to float32, keep the dtype"""
    return a.astype(np.float32).astype(a.dtype)
