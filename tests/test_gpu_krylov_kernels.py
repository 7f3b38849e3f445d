"""GPU: the Krylov vector kernels (ksfd_amd/csrc/pointwise.hip.h: k_lincomb, k_multidot, k_multidot_gram, k_reduce_rows, k_gs_update,
k_basis_axpy, k_gs_update_dev, k_gmres_coef) one by one through the test entry ksfd_krylov_op -- which runs the launch wrappers the stage
solvers run (basis-size ladder 4 | 8 | 16 | 32, chunks of 32 above that, the block-partial reduction) -- against plain numpy in
np.longdouble, and the solver paths these kernels feed: the pipelined GMRES with a restart longer than its kernels hold and synchronous
GMRES beyond 32 basis vectors, against the oracle's LU step.

No tolerance here is tuned.  With u = 2^-53 and gamma(n) = n u / (1 - n u), every bound is the standard forward bound of the operation,
valid for any order of summation and with or without fused multiply-adds (Higham, Accuracy and Stability of Numerical Algorithms, 3.1):
  dots and norms     |d - d_ref| <= gamma(n + 2) * sum_i |w_i| |v_i|,   n = F * nloc terms
  elementwise        |x - x_ref| <= gamma(k + 3) * (|beta x| + sum_i |c_i| |V_i|) * |scale|   per element (k + 1 terms, one product each,
                     the scaling: at most k + 3 roundings on any path)
  norm epilogues     the dot bound against the sum of squares of the vector the device returned
A dropped element, lane or vector misses these by many orders of magnitude while n^2 u << 1: every vector carries its own power of ten.
Each test prints 'KRATIO <operation> ... <largest error / bound>' before it asserts."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from ksfd_amd import lib as klib
from ksfd_amd.config import ProblemConfig
from oracle import ko

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53
STEP_TOL = 1e-10                      # the constant of test_gpu_step.py


def gamma(n):
    return LD(n) * U / (LD(1) - LD(n) * U)


# ---- handles: one per grid for the whole module ---------------------------------------------------------------------------------------
# (24,10): 240 points, even, 16-byte accesses, less than one block;  (25,9): 225 points, odd, 8-byte accesses;  (34,30) / (33,31): several
# blocks with a ragged last one, one per access width;  (6,5,7) x 3 fields: 3-D;  (166,): 1-D;  (16,10) x 13 fields: blockIdx.y and the
# loop over the field planes;  'ring': (24,10) as a ring of one over the host transport -- ghost rows, so the owned points do not start at 0
SUB_BLOCK = [('24x10', (24, 10), 1), ('25x9', (25, 9), 1)]
MULTI_BLOCK = [('34x30', (34, 30), 1), ('33x31', (33, 31), 1)]
OTHER = [('6x5x7', (6, 5, 7), 2), ('166', (166,), 1), ('16x10x13', (16, 10), 12), ('ring', (24, 10), 1)]
# the blocks of a vector launch are capped at 2048, so the grid-stride loop first runs a second trip above 2048 * 256 = 524288 points:
# the smallest even and odd shapes that get there
STRIDE = [('1026x512', (1026, 512), 1), ('1025x513', (1025, 513), 1)]
GRIDS = {name: (shape, nlig) for name, shape, nlig in SUB_BLOCK + MULTI_BLOCK + OTHER + STRIDE}

_HANDLES = {}


def _config(shape, nlig):
    L = tuple(0.01 * n for n in shape)
    if nlig <= 2:
        return ProblemConfig.standard(len(shape), shape, L=L, nlig=nlig)
    return ProblemConfig(dim=len(shape), n=shape, L=L, lig_group=np.arange(nlig) % 3, lig_w=np.full(nlig, 1.0), lig_s=np.full(nlig, 0.01),
                         lig_gamma=np.full(nlig, 0.01), lig_D=np.full(nlig, 1e-6), grp_alpha=np.full(3, 1500.0), grp_beta=[5.56e-4, -5.56e-4, 2e-4])


def handle(name):
    if name not in _HANDLES:
        shape, nlig = GRIDS[name]
        cfg = _config(shape, nlig)
        if name == 'ring':
            from ksfd_amd.dist import open_self_ring
            k, keep = open_self_ring(cfg, 0, 'host')
            k._keep_ring = keep
        else:
            k = klib.KSFDHip(cfg)
        _HANDLES[name] = k
    return _HANDLES[name]


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for k in _HANDLES.values():
        k.close()
    _HANDLES.clear()


# both sides of every ladder edge, the chunk edges, the whole basis (None = ksfd_basis_capacity - 1)
K_LADDER = [1, 4, 5, 8, 9, 16, 17, 30, 32, 33, 64, 65, None]
K_SHORT = [5, 17, 33]
GRID_K = [(g[0], k) for g in SUB_BLOCK + MULTI_BLOCK for k in K_LADDER] + [(g[0], k) for g in OTHER for k in K_SHORT]
GRID_K_DEV = [(g, k) for g, k in GRID_K if k is not None and k <= klib.ASYNC_MAXK]


def _ids(v):
    return 'cap-1' if v is None else str(v)


def _k(h, k):
    return h.basis_capacity() - 1 if k is None else k


@functools.lru_cache(maxsize=None)
def data(name, k):
    """k + 1 vectors of standard normal entries, each scaled by its own power of ten in 1e-3 .. 1e3, and k coefficients of mixed sign
    (read-only, shared by the tests of a case)"""
    h = handle(name)
    rng = np.random.default_rng(k * 104729 + h.nlocal * 131 + h.F)
    scales = 10.0 ** rng.permutation(np.linspace(-3.0, 3.0, k + 1))
    vecs = rng.standard_normal((k + 1, h.nlocal)) * scales[:, None]
    coef = rng.uniform(0.5, 2.0, size=max(k, 1)) * rng.choice([-1.0, 1.0], size=max(k, 1))
    coef[:2] = np.abs(coef[:2]) * np.array([1.0, -1.0])[:coef[:2].size]       # both signs at every k >= 2
    vecs.setflags(write=False)
    coef.setflags(write=False)
    return vecs, coef


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def dot_ref(w, v):
    """<w, v> and sum |w_i| |v_i| in longdouble"""
    p = w.astype(LD) * v.astype(LD)
    return p.sum(), np.abs(p).sum()


def check_dots(tag, got, w, vs):
    """got[i] against <w, vs[i]> under the dot bound; returns the largest error / bound"""
    n = w.size
    worst = 0.0
    for i, v in enumerate(vs):
        ref, mag = dot_ref(w, v)
        bound = gamma(n + 2) * mag
        ratio = float(abs(LD(got[i]) - ref) / bound)
        worst = max(worst, ratio)
    print('KRATIO %s %.3e' % (tag, worst))
    return worst


def check_elementwise(tag, got, terms, nround, scale=1.0):
    """got against sum(terms) * scale per element; terms = the products c_i * V_i (longdouble arrays); nround = roundings on the longest
    path"""
    ref = LD(scale) * sum(terms)
    mag = abs(LD(scale)) * sum(np.abs(t) for t in terms)
    bound = gamma(nround) * mag
    assert np.all(np.isfinite(got))
    err = np.abs(got.astype(LD) - ref)
    ok = bound > 0
    worst = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    assert np.all(err[~ok] == 0)
    print('KRATIO %s %.3e' % (tag, worst))
    return worst


def check_norm(tag, got, out):
    ref, mag = dot_ref(out, out)
    ratio = float(abs(LD(got) - ref) / (gamma(out.size + 2) * mag))
    print('KRATIO %s %.3e' % (tag, ratio))
    return ratio


# ---- k_lincomb ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('want_norm', [False, True])
@pytest.mark.parametrize('name', [g[0] for g in SUB_BLOCK + MULTI_BLOCK + OTHER])
def test_lincomb_vs_longdouble(name, want_norm):
    """out = sum_t a_t x_t for 1 .. 6 terms with the output aliasing input 0, with and without the norm epilogue"""
    h = handle(name)
    vecs, coef = data(name, 5)
    for nt in range(1, 7):
        a = np.append(coef[:5], 0.75)[:nt]
        out, sc = h.krylov_op(klib.KOP_LINCOMB, nt, vecs[:nt], a, want_norm=want_norm)
        terms = [LD(a[t]) * vecs[t].astype(LD) for t in range(nt)]
        assert check_elementwise('lincomb %s nt=%d' % (name, nt), out[0], terms, nt + 2) <= 1.0
        assert same_bits(out[1:], vecs[1:nt])                      # the inputs that are not the output
        if want_norm:
            assert check_norm('lincomb-norm %s nt=%d' % (name, nt), sc[0], out[0]) <= 1.0
        else:
            assert sc.size == 0


# ---- k_multidot + k_reduce_rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,k', [(g[0], 0) for g in SUB_BLOCK + MULTI_BLOCK + OTHER] + GRID_K, ids=_ids)
def test_multidot_vs_longdouble(name, k):
    """d_i = <w, V_i>, i < k, and <w, w> behind them: every row of every ladder step and chunk, twice with the same bits"""
    h = handle(name)
    k = _k(h, k)
    vecs, _ = data(name, k)
    out, sc = h.krylov_op(klib.KOP_MULTIDOT, k, vecs)
    assert sc.shape == (k + 1,)
    assert check_dots('multidot %s k=%d' % (name, k), sc, vecs[k], list(vecs[:k]) + [vecs[k]]) <= 1.0
    assert same_bits(out, vecs)
    out2, sc2 = h.krylov_op(klib.KOP_MULTIDOT, k, vecs)
    assert same_bits(sc, sc2)                                      # fixed order of the partial sums: reproducible to the bit


# ---- k_multidot_gram -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,k', GRID_K_DEV, ids=_ids)
def test_multidot_gram_vs_longdouble(name, k):
    """rows 0 .. k-1 <w, V_i>, rows k .. 2k-1 <V_{k-1}, V_i>, row 2k <w, w> -- in that order"""
    h = handle(name)
    vecs, _ = data(name, k)
    out, sc = h.krylov_op(klib.KOP_MULTIDOT_GRAM, k, vecs)
    assert sc.shape == (2 * k + 1,)
    tag = 'multidot_gram %s k=%d' % (name, k)
    assert check_dots(tag + ' d', sc[:k], vecs[k], vecs[:k]) <= 1.0
    assert check_dots(tag + ' gram', sc[k:2 * k], vecs[k - 1], vecs[:k]) <= 1.0
    assert check_dots(tag + ' ww', sc[2 * k:], vecs[k], [vecs[k]]) <= 1.0
    assert same_bits(out, vecs)
    out2, sc2 = h.krylov_op(klib.KOP_MULTIDOT_GRAM, k, vecs)
    assert same_bits(sc, sc2)
    # the Gram row is the multi-dot of V_{k-1} against the same basis: both are within the dot bound of the exact value, so within
    # twice the bound of each other
    _, md = h.krylov_op(klib.KOP_MULTIDOT, k, np.concatenate([vecs[:k], vecs[k - 1:k]]))
    for i in range(k):
        _, mag = dot_ref(vecs[k - 1], vecs[i])
        assert abs(LD(sc[k + i]) - LD(md[i])) <= 2 * gamma(vecs.shape[1] + 2) * mag
    _, mag = dot_ref(vecs[k - 1], vecs[k - 1])
    assert abs(LD(sc[2 * k - 1]) - LD(md[k])) <= 2 * gamma(vecs.shape[1] + 2) * mag


# ---- k_gs_update / k_gs_update_dev -----------------------------------------------------------------------------------------------------
def _gs_case(h, name, k, op):
    vecs, coef = data(name, k)
    scale = -0.37
    out, sc = h.krylov_op(op, k, vecs, coef[:k], alpha=scale)
    terms = [vecs[k].astype(LD)] + [-LD(coef[i]) * vecs[i].astype(LD) for i in range(k)]
    tag = '%s %s k=%d' % ('gs_update' if op == klib.KOP_GS_UPDATE else 'gs_update_dev', name, k)
    assert check_elementwise(tag, out[k], terms, k + 3, scale) <= 1.0
    assert same_bits(out[:k], vecs[:k])                            # the basis comes back as it went in


@pytest.mark.parametrize('name,k', GRID_K, ids=_ids)
def test_gs_update_vs_longdouble(name, k):
    """w = (w - sum_i h_i V_i) * scale with the coefficients passed by value, in chunks of 32 above 32 vectors"""
    h = handle(name)
    _gs_case(h, name, _k(h, k), klib.KOP_GS_UPDATE)


@pytest.mark.parametrize('name,k', GRID_K_DEV, ids=_ids)
def test_gs_update_dev_vs_longdouble(name, k):
    """the pipelined solver's update: coefficients and scale read from the device block its small-algebra kernel writes"""
    _gs_case(handle(name), name, k, klib.KOP_GS_UPDATE_DEV)


# ---- k_basis_axpy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('want_norm', [False, True])
@pytest.mark.parametrize('beta', [0.0, -1.75])
@pytest.mark.parametrize('name,k', GRID_K, ids=_ids)
def test_basis_axpy_vs_longdouble(name, k, beta, want_norm):
    """x = beta x + sum_i y_i V_i.  By the kernel's contract a zero coefficient costs no load and beta = 0 does not read x: every third
    coefficient is an exact zero with its V_i filled with NaN, and with beta = 0 the incoming x is NaN -- the result must be clean."""
    h = handle(name)
    k = _k(h, k)
    vecs0, coef0 = data(name, k)
    vecs, coef = vecs0.copy(), coef0[:k].copy()
    zero = np.arange(k) % 3 == 2
    coef[zero] = 0.0
    vecs[:k][zero] = np.nan
    if beta == 0.0:
        vecs[k] = np.nan
    out, sc = h.krylov_op(klib.KOP_BASIS_AXPY, k, vecs, coef, beta=beta, want_norm=want_norm)
    terms = [LD(coef[i]) * vecs[i].astype(LD) for i in range(k) if not zero[i]]
    if beta != 0.0:
        terms.append(LD(beta) * vecs[k].astype(LD))
    tag = 'basis_axpy %s k=%d beta=%g' % (name, k, beta)
    assert check_elementwise(tag, out[k], terms, k + 3) <= 1.0
    assert same_bits(out[:k], vecs[:k])
    if want_norm:
        assert check_norm('basis_axpy-norm %s k=%d beta=%g' % (name, k, beta), sc[0], out[k]) <= 1.0


# ---- the grid-stride loop ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def stride_data(name):
    h = handle(name)
    rng = np.random.default_rng(h.nlocal)
    scales = 10.0 ** rng.permutation(np.linspace(-3.0, 3.0, 34))
    vecs = rng.standard_normal((34, h.nlocal))
    vecs *= scales[:, None]
    coef = rng.uniform(0.5, 2.0, size=33) * np.where(np.arange(33) % 2, -1.0, 1.0)
    vecs.setflags(write=False)
    return vecs, coef


@pytest.mark.parametrize('name,case', [(g[0], c) for g in STRIDE for c in ('multidot3', 'multidot33', 'basis_axpy33', 'lincomb3')])
def test_grid_stride_loop(name, case):
    """more points than 2048 blocks cover in one trip: the second trip of the stride loop, and its ragged end, for both access widths"""
    h = handle(name)
    assert h.nlocal // h.F > 2048 * 256
    vecs, coef = stride_data(name)
    if case.startswith('multidot'):
        k = int(case[8:])
        v = np.concatenate([vecs[:k], vecs[33:]])
        out, sc = h.krylov_op(klib.KOP_MULTIDOT, k, v)
        assert check_dots('multidot %s k=%d' % (name, k), sc, v[k], list(v[:k]) + [v[k]]) <= 1.0
        assert same_bits(out, v)
    elif case == 'basis_axpy33':
        out, sc = h.krylov_op(klib.KOP_BASIS_AXPY, 33, vecs, coef, beta=0.5, want_norm=True)
        ref = LD(0.5) * vecs[33].astype(LD)
        mag = np.abs(ref)
        for i in range(33):
            t = LD(coef[i]) * vecs[i].astype(LD)
            ref += t
            mag += np.abs(t)
        ratio = float((np.abs(out[33].astype(LD) - ref) / (gamma(36) * mag)).max())
        print('KRATIO basis_axpy %s k=33 %.3e' % (name, ratio))
        assert ratio <= 1.0
        assert same_bits(out[:33], vecs[:33])
        assert check_norm('basis_axpy-norm %s k=33' % name, sc[0], out[33]) <= 1.0
    else:
        out, sc = h.krylov_op(klib.KOP_LINCOMB, 3, vecs[:3], coef[:3], want_norm=True)
        terms = [LD(coef[t]) * vecs[t].astype(LD) for t in range(3)]
        assert check_elementwise('lincomb %s nt=3' % name, out[0], terms, 5) <= 1.0
        assert same_bits(out[1:], vecs[1:3])
        assert check_norm('lincomb-norm %s nt=3' % name, sc[0], out[0]) <= 1.0


# ---- k_gmres_coef --------------------------------------------------------------------------------------------------------------------
# The kernel (header comment in pointwise.hip.h): from the reduced rows of column j (k = j + 1 vectors) d = V^T w, Gram row g, ww = |w|^2
#     c = d + (I - G) d,   hn^2 = ww - 2 c.d + c^T G c,   column [c; hn] -> earlier Givens rotations -> new rotation -> g.
# The reference evaluates the same formulas in longdouble and carries a first-order running error bound e(.) for every quantity next to its
# value; products of two error terms are added explicitly where they arise.  With A_i = |d_i| + sum_l |delta_il - G_il| |d_l|:
#   c_i      k + 1 terms, each (delta - G) d one subtraction and one product, the sum, the final addition:      e(c_i) = gamma(k + 3) A_i
#   hn^2     evaluated at the kernel's own c:  rounding  gamma(2k + 4) (|ww| + 2 sum |c_i d_i| + sum_il |c_i| |G_il| |c_l|)
#            (longest path: inner product k + 1, product with c_i, outer sum k, last addition)  plus the propagated
#            sum_i e(c_i) (2 |d_i| + 2 sum_l |G_il| |c_l|) + sum_il e(c_i) |G_il| e(c_l)
#   hn       sqrt is correctly rounded and |sqrt(a + e) - sqrt(a)| <= |e| / sqrt(a):            e(hn) = e(hn^2) / hn + u hn
#   scale    1 / hn:                                                   e(scale) = e(hn) / (hn (hn - e(hn))) + u / (hn - e(hn))
#   rotation of (a, b) by (cs, sn):  t = cs a + sn b:  e(t) = |cs| e(a) + |sn| e(b) + e(cs) |a| + e(sn) |b| + e(cs) e(a) + e(sn) e(b)
#            + gamma(3) (|cs a| + |sn b|), the same for the second row
#   den      hypot (within 1 ulp, taken as 2 u) of (a, b):  e(den) = e(a) + e(b) + 2 u den   (|a|, |b| <= den)
#   cs, sn   a / den:  e(cs) = e(a) / dl + |a| e(den) / (den dl) + u |cs|,  dl = den - e(den)
#   g        g_j+1 = -sn g_j, g_j = cs g_j:  e = e(sn) |g_j| + |sn| e(g_j) + e(sn) e(g_j) + u |sn g_j|;  |g_j| <= beta, so every bound on
#            g and on the residual estimate is a multiple of u beta plus what the column's own errors carry in.
def gmres_coef_reference(rows, k, beta):
    G = np.zeros((k, k), dtype=LD)
    H, eH = np.zeros((k + 1, k), dtype=LD), np.zeros((k + 1, k), dtype=LD)
    Hraw = np.zeros((k + 1, k), dtype=LD)
    cs, sn, ecs, esn = (np.zeros(k, dtype=LD) for _ in range(4))
    g, eg = np.zeros(k + 1, dtype=LD), np.zeros(k + 1, dtype=LD)
    g[0] = LD(beta)
    per_col = []
    pos = 0
    for j in range(k):
        kk = j + 1
        row = np.asarray(rows[pos:pos + 2 * kk + 1], dtype=LD)
        pos += 2 * kk + 1
        d, gr, ww = row[:kk], row[kk:2 * kk], row[2 * kk]
        G[:kk, j] = gr
        G[j, :kk] = gr
        Gk = G[:kk, :kk]
        IG = np.eye(kk, dtype=LD) - Gk
        c = d + IG @ d
        ec = gamma(kk + 3) * (np.abs(d) + np.abs(IG) @ np.abs(d))
        hn2 = ww - 2 * (c @ d) + c @ (Gk @ c)
        ca = np.abs(c) + ec                                         # magnitude of the kernel's own c
        ehn2 = (gamma(2 * kk + 4) * (abs(ww) + 2 * (ca @ np.abs(d)) + ca @ (np.abs(Gk) @ ca))
                + ec @ (2 * np.abs(d) + 2 * (np.abs(Gk) @ np.abs(c))) + ec @ (np.abs(Gk) @ ec))
        assert hn2 > ehn2, 'test data: the new vector must not vanish'
        hn = np.sqrt(hn2)
        ehn = ehn2 / hn + U * hn
        scale = 1 / hn
        escale = ehn / (hn * (hn - ehn)) + U / (hn - ehn)
        col, ecol = np.append(c, hn), np.append(ec, ehn)
        Hraw[:kk + 1, j] = col
        for i in range(j):
            a, b, ea, eb = col[i], col[i + 1], ecol[i], ecol[i + 1]
            rnd = gamma(3) * (abs(cs[i] * a) + abs(sn[i] * b))
            t = cs[i] * a + sn[i] * b
            et = abs(cs[i]) * ea + abs(sn[i]) * eb + ecs[i] * abs(a) + esn[i] * abs(b) + ecs[i] * ea + esn[i] * eb + rnd
            b2 = -sn[i] * a + cs[i] * b
            eb2 = abs(sn[i]) * ea + abs(cs[i]) * eb + esn[i] * abs(a) + ecs[i] * abs(b) + esn[i] * ea + ecs[i] * eb + rnd
            col[i], col[i + 1], ecol[i], ecol[i + 1] = t, b2, et, eb2
        a, b, ea, eb = col[j], col[j + 1], ecol[j], ecol[j + 1]
        den = np.hypot(a, b)
        eden = ea + eb + 2 * U * den
        dl = den - eden
        assert dl > 0
        cs[j], sn[j] = a / den, b / den
        ecs[j] = ea / dl + abs(a) * eden / (den * dl) + U * abs(cs[j])
        esn[j] = eb / dl + abs(b) * eden / (den * dl) + U * abs(sn[j])
        col[j], ecol[j], col[j + 1], ecol[j + 1] = den, eden, LD(0), LD(0)
        H[:kk + 1, j], eH[:kk + 1, j] = col, ecol
        gj, egj = g[j], eg[j]
        g[j + 1] = -sn[j] * gj
        eg[j + 1] = esn[j] * abs(gj) + abs(sn[j]) * egj + esn[j] * egj + U * abs(sn[j] * gj)
        g[j] = cs[j] * gj
        eg[j] = ecs[j] * abs(gj) + abs(cs[j]) * egj + ecs[j] * egj + U * abs(cs[j] * gj)
        per_col.append(dict(c=c, ec=ec, hn=hn, ehn=ehn, scale=scale, escale=escale, res=abs(g[j + 1]), eres=eg[j + 1]))
    return per_col, H, eH, g.copy(), eg.copy(), Hraw


@functools.lru_cache(maxsize=None)
def arnoldi_rows(k, skew):
    """the reduced rows [d, Gram row, ww] of k Arnoldi columns on a random 40 x 40 matrix, from a run in numpy that orthogonalises the way
    the pipelined solver does.  skew = 0: G = I to rounding, as in production; skew > 0: every new basis vector is pushed off by that
    much in a random direction, so ||I - G|| ~ skew and the algebraic second projection carries weight."""
    rng = np.random.default_rng(40 + k + int(skew * 1e6))
    n = 40
    A = rng.standard_normal((n, n)) / np.sqrt(n) + 2.0 * np.eye(n)
    b = rng.standard_normal(n)
    beta = float(np.linalg.norm(b))
    V = np.zeros((k + 1, n))
    V[0] = b / beta
    rows = []
    for j in range(k):
        kk = j + 1
        w = A @ V[j]
        d, gr, ww = V[:kk] @ w, V[:kk] @ V[j], w @ w
        rows += [d, gr, [ww]]
        Gk = V[:kk] @ V[:kk].T
        c = d + (np.eye(kk) - Gk) @ d
        w = w - V[:kk].T @ c
        w /= np.linalg.norm(w)
        if skew:
            p = rng.standard_normal(n)
            w = w + skew * p / np.linalg.norm(p)
        V[j + 1] = w
    rows = np.concatenate([np.ravel(r) for r in rows])
    rows.setflags(write=False)
    return rows, beta


def _backsolve(R, g, k):
    y = np.zeros(k, dtype=LD)
    for i in range(k - 1, -1, -1):
        y[i] = (g[i] - R[i, i + 1:k] @ y[i + 1:]) / R[i, i]
    return y


@pytest.mark.parametrize('skew', [0.0, 1e-3], ids=['orthonormal', 'skewed'])
@pytest.mark.parametrize('k', [1, 2, 5, 17, 30, 32])
def test_gmres_coef_vs_longdouble(k, skew):
    h = handle('24x10')
    rows, beta = arnoldi_rows(k, skew)
    _, sc = h.krylov_op(klib.KOP_GMRES_COEF, k, coef=rows, beta=beta)
    per_col, H, eH, g, eg, Hraw = gmres_coef_reference(rows, k, beta)
    worst = dict(coef=0.0, scale=0.0, res=0.0, hn=0.0, H=0.0, g=0.0)

    def ratio(key, got, ref, bound):
        r = float(abs(LD(got) - ref) / bound) if bound > 0 else (0.0 if LD(got) == ref else np.inf)
        worst[key] = max(worst[key], r)

    for j, col in enumerate(per_col):
        blk = sc[j * (k + 3):(j + 1) * (k + 3)]
        for i in range(j + 1):
            ratio('coef', blk[i], col['c'][i], col['ec'][i])
        ratio('scale', blk[k], col['scale'], col['escale'])
        ratio('res', blk[k + 1], col['res'], col['eres'])
        ratio('hn', blk[k + 2], col['hn'], col['ehn'])
    Hk = sc[k * (k + 3):k * (k + 3) + k * (k + 1)].reshape(k, k + 1).T            # column c of the kernel's H in column c
    gk = sc[k * (k + 3) + k * (k + 1):]
    assert gk.shape == (k + 1,)
    for c in range(k):
        for i in range(c + 1):
            ratio('H', Hk[i, c], H[i, c], eH[i, c])
        assert Hk[c + 1, c] == 0.0                                  # rotated away
    for i in range(k + 1):
        ratio('g', gk[i], g[i], eg[i])
    print('KRATIO gmres_coef k=%d skew=%g %s' % (k, skew, ' '.join('%s %.3e' % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0
    if skew and k >= 2:                                            # (V_0 is the normalised start residual: nothing skewed at k = 1)
        G = np.eye(k)
        pos = 0
        for j in range(k):
            G[:j + 1, j] = G[j, :j + 1] = rows[pos + j + 1:pos + 2 * j + 2]
            pos += 2 * j + 3
        assert 1e-4 < np.linalg.norm(np.eye(k) - G, 2) < 1e-1      # the second projection is not a no-op in this set
    # H and g solve the least-squares problem of the raw Hessenberg matrix: y from the kernel's triangular factor against numpy's lstsq.
    #   kernel side: (R + dR) y = g + dg with |dR| <= eH, |dg| <= eg  =>  |y - y_exact| <= ||R^-1|| (||eH||_F ||y|| + ||eg||)
    #   lstsq side:  backward stable with a modest constant, taken as 10 k u; first-order perturbation bound of the least-squares problem
    #                (Higham, Theorem 20.1): 10 k u (cond ||y|| + cond^2 ||r|| / ||H||)
    Hr = Hraw.astype(np.float64)
    rhs = np.zeros(k + 1)
    rhs[0] = beta
    y_ls = np.linalg.lstsq(Hr, rhs, rcond=None)[0]
    y_k = _backsolve(Hk.astype(LD), gk.astype(LD), k)
    s = np.linalg.svd(Hr, compute_uv=False)
    cond, rnorm = s[0] / s[-1], np.linalg.norm(rhs - Hr @ y_ls)
    rinv = 1.0 / np.linalg.svd(Hk[:k, :k], compute_uv=False)[-1]
    ynorm = float(np.linalg.norm(y_ls))
    bound = (rinv * (float(np.linalg.norm(eH.astype(np.float64))) * ynorm + float(np.linalg.norm(eg[:k].astype(np.float64))))
             + 10 * k * float(U) * (cond * ynorm + cond * cond * rnorm / s[0]))
    err = float(np.linalg.norm((y_k - y_ls.astype(LD)).astype(np.float64)))
    print('KRATIO gmres_coef-lstsq k=%d skew=%g %.3e' % (k, skew, err / bound))
    assert err <= bound


# ---- guards --------------------------------------------------------------------------------------------------------------------------
def test_guards_reject_and_leave_the_stepper_alone():
    """sizes outside the limits are KSFD_EINVAL before anything is touched, and neither they nor a successful operation change what a
    step computes: the same step on a fresh handle gives the same bits"""
    cfg = _config((24, 10), 1)
    rng = np.random.default_rng(5)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)
    u = np.concatenate([rho, rho * (1 + 0.01 * rng.standard_normal(cfg.N))])
    a, b = klib.KSFDHip(cfg), klib.KSFDHip(cfg)
    try:
        a.set_state(u), b.set_state(u)
        cap = a.basis_capacity()
        vecs, coef = data('24x10', 5)
        a.krylov_op(klib.KOP_MULTIDOT, 5, vecs)
        a.krylov_op(klib.KOP_GS_UPDATE_DEV, 5, vecs, coef)
        two = np.zeros((2, a.nlocal))
        bad = [(klib.KOP_MULTIDOT_GRAM, 33), (klib.KOP_MULTIDOT_GRAM, 0), (klib.KOP_GS_UPDATE_DEV, klib.ASYNC_MAXK + 1),
               (klib.KOP_MULTIDOT, cap), (klib.KOP_GS_UPDATE, cap), (klib.KOP_BASIS_AXPY, cap), (klib.KOP_BASIS_AXPY, cap + 7),
               (klib.KOP_LINCOMB, 7), (klib.KOP_LINCOMB, 0), (klib.KOP_MULTIDOT, -1), (7, 3)]
        for op, k in bad:
            with pytest.raises(klib.KSFDError) as e:
                a.krylov_op(op, k, two, np.zeros(max(k, 1)))
            assert e.value.code == klib.EINVAL, (op, k)
        with pytest.raises(klib.KSFDError) as e:
            a.krylov_op(klib.KOP_GMRES_COEF, 33, coef=np.zeros(33 * 33 + 66), beta=1.0)
        assert e.value.code == klib.EINVAL
        with pytest.raises(klib.KSFDError) as e:
            a.krylov_op(klib.KOP_MULTIDOT, 1, two, want_norm=True)
        assert e.value.code == klib.EINVAL
        assert same_bits(a.get_state(), b.get_state())
        opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, pc_type=0, ksp_rtol=1e-10)
        ra, rb = a.step(0.0, 0.05, opts), b.step(0.0, 0.05, opts)
        assert ra[2].linear_its == rb[2].linear_its > 0
        assert same_bits(a.get_state(), b.get_state())
    finally:
        a.close()
        b.close()


# ---- the solver paths these kernels feed -------------------------------------------------------------------------------------------------
LONG_SHAPE, LONG_H = (32, 24), 0.5


@functools.lru_cache(maxsize=None)
def long_case():
    """A fixed step whose four unpreconditioned stage systems need more than 32 iterations each at ksp_rtol = 1e-12, chosen with the
    oracle's GMRES on the CPU: 355 iterations for the four stages at restart 64, 368 at restart 32, both 1e-13 from the oracle's LU
    step, which is the answer here (dense LU of 1536 unknowns: a second)."""
    cfg = ProblemConfig.standard(2, LONG_SHAPE, L=(0.1, 0.1), nlig=1)
    rng = np.random.default_rng(11)
    rho = 9000 + 90 * rng.standard_normal(cfg.N)
    u = np.concatenate([rho, rho * cfg.lig_s[0] / cfg.lig_gamma[0]])
    un, err, wr, _ = ko.Oracle(cfg).rosw_step(u, LONG_H, 0.01, 1e-6, solver='lu')
    un.setflags(write=False)
    return cfg, u, un


def long_opts(**kw):
    return klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, pc_type=0, ksp_restart=64, ksp_rtol=1e-12, ksp_max_it=20000, **kw)


@functools.lru_cache(maxsize=None)
def long_run(tuning, reserved=0):
    cfg, u, un = long_case()
    k = klib.KSFDHip(cfg)
    k.set_tuning(use_fused=tuning)
    k.set_state(u)
    t, hn, st, rc = k.step(0.0, LONG_H, long_opts(reserved=reserved), raise_on_error=False)
    state, msg = k.get_state(), k.last_error()
    assert k.basis_capacity() > 64 + 16                           # room for a cycle of 64 behind the vectors kept for recycling
    k.close()
    state.setflags(write=False)
    return rc, state, st.linear_its, st.pc_used, msg


def test_pipelined_gmres_with_a_restart_beyond_its_kernels():
    """ksp_restart = 64 under the pipelined solver: its kernels hold 32 vectors, so the solve runs as cycles of 32 (before the clamp the
    kernels ignored the vectors past 32 and the small-algebra kernel wrote past its coefficient array).  Precondition, so that the test
    cannot pass without getting there: the synchronous solver with the restart kept at 64 needs at least 4 * 40 iterations."""
    cfg, u, un = long_case()
    rc_s, sync, its_s, pc_s, msg_s = long_run(klib.TUNE_FUSED | klib.TUNE_NO_RESTART_GROWTH)
    assert rc_s == 0, msg_s
    print('long restart: synchronous %d iterations, rel-L2 vs LU %.3e' % (its_s, rel_l2(sync, un)))
    assert its_s >= 4 * 40
    rc_a, asyn, its_a, pc_a, msg_a = long_run(klib.TUNE_FUSED | klib.TUNE_ASYNC_GMRES | klib.TUNE_NO_RESTART_GROWTH)
    assert rc_a == 0, msg_a
    print('long restart: pipelined %d iterations, rel-L2 vs LU %.3e, vs synchronous %.3e' % (its_a, rel_l2(asyn, un), rel_l2(asyn, sync)))
    assert pc_a == klib.PC_NONE
    assert rel_l2(asyn, un) < STEP_TOL
    assert rel_l2(asyn, sync) < STEP_TOL


@pytest.mark.parametrize('reserved', [0, 1], ids=['algebraic', 'classic'])
def test_synchronous_gmres_beyond_32_vectors(reserved):
    """Restart kept at 64: columns 33 .. 64 of a cycle go through the chunked multi-dot / update wrappers (31 and 32 through the top of
    the ladder).  The stats hold no per-cycle count; what they allow: at least 4 * 40 iterations over four stage solves means one solve of
    at least 40, and a cycle of a solve ends before its 64th column only on convergence -- so that solve's first cycle ran past 32 columns."""
    cfg, u, un = long_case()
    rc, state, its, pc, msg = long_run(klib.TUNE_FUSED | klib.TUNE_NO_RESTART_GROWTH, reserved)
    assert rc == 0, msg
    print('beyond 32 vectors (reserved %d): %d iterations, rel-L2 vs LU %.3e' % (reserved, its, rel_l2(state, un)))
    assert its >= 4 * 40
    assert rel_l2(state, un) < STEP_TOL
