"""GPU: every part of the geometric multigrid V cycle (csrc/mg.hip.h, mg_host.hip.h, the smoother epilogues of the Jacobian-action
kernels) in isolation against the numpy reference of tests/mg_reference.py, through the test entry ksfd_mg_part -- which runs the wrappers
the cycle calls.  The reference of each part is fed the DOWNLOADED results of the parts before it (coefficient planes, inverse point
blocks, Chebyshev bounds), so an error is charged to the part that makes it and every link has its own test.  Inputs: random normal
vectors and unit impulses at the first and the last owned point (the impulses catch index errors at the wrap).

Tolerances (none tuned on the kernels):
  transfers, coefficient restriction, fp64: elementwise (m + 2) eps |W| |v| against longdouble, m = terms of the weighted sum
  fp32 transfers, DINV: one float32 ulp from the float32-rounded reference
  OPERATOR fp64: rel-L2 per field 1e-12, the tolerance tests/test_gpu_operators.py applies to the Jacobian action
  SMOOTH, CYCLE fp64: 32 x max(d_ref, 1e-12), d_ref = rel-L2 between the reference's own float64 and longdouble evaluations
  CYCLE, OPERATOR fp32: 4 x d32, d32 = rel-L2 between the reference with float32-rounded level vectors and without; d32 < 1e-5
Measured distances and head-room: profiles/mg_parts_runs.log (the lines this file prints)."""
import os
import socket

import numpy as np
import pytest

import mg_reference as mr
from ksfd_amd.config import ProblemConfig
from ksfd_amd import lib as klib
from test_gpu_mg_coarse import _cfg, _state

pytestmark = pytest.mark.gpu
GAMMA = 0.43586652150845900
EPS = np.finfo(float).eps
LD = np.longdouble
TOL_OP = 1e-12                                # tests/test_gpu_operators.py: TOL of the Jacobian action
MARGIN = 32.0
S_MILD, S_STIFF = 1.0 / (GAMMA * 0.05), 1.0 / (GAMMA * 50.0)      # shifts of the DINV test
S_CYCLE = 1.0 / (GAMMA * 5.0)                 # shift of the SMOOTH and CYCLE tests: a stiff step
MG_RATIO = 6.0                                # the handle's default smoothing interval (mg_ratio)

#         name        shape       ligands  extents per level                          path per level (0 strip 2-D, 2 strip 3-D, 3 generic)
CASES = {'32x32': ((32, 32), 1, [(32, 32), (16, 16), (8, 8)], [0, 0, 3]),
         '64x48': ((64, 48), 2, [(64, 48), (32, 24), (16, 12)], [0, 0, 0]),
         '256x16': ((256, 16), 1, [(256, 16), (128, 8)], [0, 0]),
         '36x36': ((36, 36), 2, [(36, 36), (18, 18), (9, 9)], [0, 0, 3]),
         '40x24': ((40, 24), 3, [(40, 24), (20, 12)], [0, 0]),
         '16x16x16': ((16, 16, 16), 1, [(16, 16, 16), (8, 8, 8)], [None, 3]),
         '32x16x16': ((32, 16, 16), 2, [(32, 16, 16), (16, 8, 8)], [None, None]),
         '96': ((96,), 1, [(96,), (48,), (24,), (12,)], [3, 3, 3, 3]),
         '130': ((130,), 2, [(130,), (65,)], [3, 3])}
RING_CASES = {'ring-64x48': ((64, 48), 1), 'ring-16x16x16': ((16, 16, 16), 1), 'ring-96': ((96,), 2)}
SMOOTH_CASES = ['32x32', '64x48', '256x16', '16x16x16', '96']
FIRST_2D = ['32x32', '64x48', '256x16']


class Case:
    """one handle at the state of tests/test_gpu_mg_coarse.py::test_coarse_solve_against_numpy, with what the tests download once"""

    def __init__(self, name):
        ring = name.startswith('ring-')
        twin = name.startswith('twin-')                      # shape and ligands of a ring case on an ordinary handle (wrap-index arms)
        shape, nlig = RING_CASES[name] if ring else RING_CASES[name[5:]] if twin else CASES[name][:2]
        self.name, self.shape, self.nlig, self.dim = name, shape, nlig, len(shape)
        self.cfg = _cfg(shape, nlig, tuple((0.01 if len(shape) == 3 else 0.0025) * n for n in shape))
        if ring:
            from ksfd_amd.dist import open_self_ring
            self.k, self._keep = open_self_ring(self.cfg, 0, 'host')
        else:
            self.k = klib.KSFDHip(self.cfg)
        self.u = _state(self.cfg, 3, amp=0.05)
        self.k.set_state(self.u)
        self.F = self.cfg.F
        self.lig = dict(s=list(self.cfg.lig_s), gamma=list(self.cfg.lig_gamma), D=list(self.cfg.lig_D))
        self.h0 = [self.cfg.L[a] / shape[a] for a in range(self.dim)]
        self.nlev = self.k.mg_level_info(0)['nlevels']
        self.info = [self.k.mg_level_info(l) for l in range(self.nlev)]
        self._coef, self._setup = {}, {}

    def grid(self, l):
        return mr.grid_shape(self.info[l]['n'][:self.dim])

    def h(self, l):
        return [x * 2 ** l for x in self.h0]

    def field(self, a, l, planes=None):
        return np.asarray(a).reshape((planes or self.F,) + self.grid(l))

    def coef(self, l, tune=0):
        """(fp64 planes, fp32 copy or None) of level l as downloaded, (3 + nlig, *grid)"""
        if (l, tune) not in self._coef:
            c, c32 = self.k.mg_part(klib.MGP_COEF, l)
            self._coef[(l, tune)] = (self.field(c, l, 3 + self.nlig), None if c32 is None else self.field(c32, l, 3 + self.nlig))
        return self._coef[(l, tune)]

    def planes(self, l, tune=0):
        """the planes the operator of the fp64 cycle reads on level l"""
        c, c32 = self.coef(l, tune)
        return c32 if (self.k.mg_level_info(l)['coef32'] & 1) else c

    def setup(self, shift, tune=0):
        """per level of the cycle: downloaded inverse blocks (*grid, F, F), lam_max, ratio, coarse sweeps after a cold set-up at shift"""
        key = (shift, tune, self.k.mg_coarse_info()['kind'])
        if key not in self._setup:
            out = []
            for l in range(self.nlev):
                inf = self.k.mg_level_info(l, shift)
                if not inf['have_setup']:
                    out.append((inf, None))
                    continue
                D = self.k.mg_part(klib.MGP_DINV, l, shift=shift)
                out.append((inf, mr.planes_to_blocks(self.field(D, l, self.F * self.F), self.F)))
            self._setup[key] = out
        return self._setup[key]

    def levels(self, shift, tune=0, dtype=np.float64, copies=0):
        """reference levels from the downloaded planes, blocks and bounds.  copies: levels 0 .. copies - 1 on their fp32 coefficient copy,
        the planes the cycle with fp32 level vectors reads there (mg_op<float>)"""
        out = []
        for l, (inf, D) in enumerate(self.setup(shift, tune)):
            C = self.coef(l, tune)[1] if (l < copies and self.coef(l, tune)[1] is not None) else self.planes(l, tune)
            out.append(mr.Level(C.astype(dtype), self.h(l), None if D is None else D.astype(dtype), inf['lam_max'], inf['ratio'], inf['coarse_sweeps']))
        return out

    def inputs(self, l, seed, planes=None):
        """random normal vector, unit impulse at point 0 of field 0, unit impulse at the last owned point of the last field"""
        P = planes or self.F
        shp = (P,) + self.grid(l)
        v = np.random.default_rng(seed).standard_normal(shp)
        e0, e1 = np.zeros(shp), np.zeros(shp)
        e0.reshape(-1)[0] = 1.0
        e1.reshape(-1)[-1] = 1.0
        return [('random', v), ('impulse-first', e0), ('impulse-last', e1)]


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for c in _CASES.values():
        c.k.close()
    _CASES.clear()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def per_field(got, ref):
    """largest rel-L2 distance of a field; a field the reference leaves zero must be zero"""
    return max((mr.rel_l2(got[c], ref[c]) if np.any(ref[c]) else (np.inf if np.any(got[c]) else 0.0)) for c in range(ref.shape[0]))


# ---- 0. the levels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_level_info(name):
    c = case(name)
    shape, nlig, extents, paths = CASES[name]
    assert c.nlev == len(extents)
    for l, inf in enumerate(c.info):
        assert inf['n'][:c.dim] == extents[l] and inf['F'] == nlig + 1 and inf['points'] == int(np.prod(extents[l])) and inf['sloc'] == extents[l][-1]
        if paths[l] is not None:
            assert inf['path'] == paths[l], (l, inf)
        else:
            assert inf['path'] in (klib.MG_PATH_STRIP3D, klib.MG_PATH_GENERIC)
        strip2d = inf['path'] == klib.MG_PATH_STRIP2D
        assert inf['f32'] == (strip2d and l + 1 < c.nlev and all(c.info[q]['path'] == klib.MG_PATH_STRIP2D for q in range(l)))
        assert inf['can_fuse'] == (inf['path'] != klib.MG_PATH_STRIP3D)
        assert (inf['coef32'] & 1) == (1 if (l == 0 and strip2d) else 0)
        assert not inf['have_setup']
    if c.dim == 3:
        assert c.info[0]['path'] == klib.MG_PATH_STRIP3D and not c.info[0]['can_fuse']
    after = [c.k.mg_level_info(l, S_CYCLE) for l in range(c.nlev)]
    again = [c.k.mg_level_info(l, S_CYCLE) for l in range(c.nlev)]
    assert after == again                                   # cold set-ups: bit for bit
    for l, inf in enumerate(after):
        assert inf['have_setup'] and 0.5 < inf['lam_max'] < 4.0
        assert inf['coarse_sweeps'] == (0 if l + 1 < c.nlev else int(min(max(np.ceil(0.5 * np.sqrt(inf['ratio']) * np.log(2.0 / 0.3)), 4), 400)))


def test_level_zero_reads_fp64_planes_with_tuning_bit_9():
    c = case('32x32')
    try:
        c.k.set_tuning(use_fused=klib.TUNE_FUSED | klib.TUNE_POLY_FP64)
        assert c.k.mg_level_info(0)['coef32'] & 1 == 0
    finally:
        c.k.set_tuning(use_fused=klib.TUNE_FUSED)
    assert c.k.mg_level_info(0)['coef32'] & 1 == 1


# ---- 1. anchor of the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_reference_jacobian_equals_the_assembled_export(name):
    """the reference action at level 0 from the downloaded fp64 planes against ksfd_jacobian_csr (tied to the oracle and to the reference's
    entries by tests/test_gpu_operators.py), on impulses and a random vector"""
    import scipy.sparse as sp
    c = case(name)
    rp, col, val = c.k.jacobian_csr()
    N = c.cfg.N
    A = sp.csr_matrix((val, col, rp), shape=(c.F * N, c.F * N))
    C = c.coef(0)[0]
    for what, v in c.inputs(0, 11):
        want = (A @ v.reshape(c.F, N).T.reshape(-1)).reshape(N, c.F).T.reshape(v.shape)
        got = mr.jac_apply(C, v, c.h(0), c.lig)
        assert per_field(got, want) < TOL_OP, (what, per_field(got, want))


# ---- 2. coefficient planes and transfers ---------------------------------------------------------------------------------------------
def _transfer_bound(c, fn, v, m, extra=0):
    """(reference in longdouble, elementwise bound (m + 2) eps |W| |v|)"""
    ref = fn(v.astype(LD))
    return ref, (m + extra + 2) * EPS * fn(np.abs(v).astype(LD)).astype(np.float64)


@pytest.mark.parametrize('name', list(CASES) + list(RING_CASES))
def test_coefficient_planes_are_restricted_level_by_level(name):
    c = case(name)
    for l in range(c.nlev - 1):
        fine, (coarse, coarse32) = c.coef(l)[0], c.coef(l + 1)
        ref, bound = _transfer_bound(c, lambda a: mr.restrict(a, c.dim), fine, 3 ** c.dim)
        err = np.abs(coarse - ref.astype(np.float64))
        assert np.all(err <= bound), (l, float((err / np.maximum(bound, 1e-300)).max()))
        assert (coarse32 is not None) == (c.info[l + 1]['f32'])
        if coarse32 is not None:
            r32 = f32(ref)
            assert np.all(np.abs(coarse32 - r32) <= ulp32(r32)), l
    c0, c32 = c.coef(0)
    if c32 is not None:
        assert np.all(np.abs(c32 - f32(c0)) <= ulp32(c0))


@pytest.mark.parametrize('name', list(CASES) + list(RING_CASES))
def test_restriction_fp64(name):
    c = case(name)
    for l in range(c.nlev - 1):
        for what, v in c.inputs(l, 21 + l):
            got = c.field(c.k.mg_part(klib.MGP_RESTRICT, l, v), l + 1)
            ref, bound = _transfer_bound(c, lambda a: mr.restrict(a, c.dim), v, 3 ** c.dim)
            err = np.abs(got - ref.astype(np.float64))
            assert np.all(err <= bound), ('RESTRICT', l, what, float(err.max()))
            assert np.array_equal(got != 0, ref != 0), ('RESTRICT', l, what)      # an impulse reaches 1 (even point) or 2^dim (odd, at the wrap) coarse points
    if name.startswith('ring-'):
        one = case('twin-' + name)
        for l in range(c.nlev - 1):
            for what, v in c.inputs(l, 21 + l):
                assert np.array_equal(c.k.mg_part(klib.MGP_RESTRICT, l, v), one.k.mg_part(klib.MGP_RESTRICT, l, v))


@pytest.mark.parametrize('name', list(CASES) + list(RING_CASES))
def test_prolongation_fp64(name):
    c = case(name)
    for l in range(c.nlev - 1):
        fine = np.random.default_rng(31 + l).standard_normal((c.F,) + c.grid(l))
        for what, v in c.inputs(l + 1, 41 + l):
            got = c.field(c.k.mg_part(klib.MGP_PROLONG_ADD, l, fine, v), l)
            ref = fine.astype(LD) + mr.prolong(v.astype(LD), c.dim)
            bound = (2 ** c.dim + 1 + 2) * EPS * (np.abs(fine) + mr.prolong(np.abs(v), c.dim))
            err = np.abs(got - ref.astype(np.float64))
            assert np.all(err <= bound), ('PROLONG_ADD', l, what, float(err.max()))
    if name.startswith('ring-'):
        one = case('twin-' + name)
        for l in range(c.nlev - 1):
            fine = np.random.default_rng(31 + l).standard_normal((c.F,) + c.grid(l))
            for what, v in c.inputs(l + 1, 41 + l):
                assert np.array_equal(c.k.mg_part(klib.MGP_PROLONG_ADD, l, fine, v), one.k.mg_part(klib.MGP_PROLONG_ADD, l, fine, v))


@pytest.mark.parametrize('name', ['32x32', '64x48', '256x16', '36x36', '40x24', 'ring-64x48'])
def test_transfers_with_fp32_level_vectors(name):
    """the storage-type variants the fp32 cycle launches: k_restrict2d<float, float> / <float, double> / <double, float>,
    k_prolong_add2d<float, float> / <double, float>; one float32 ulp from the float32-rounded reference (fp64 results: the fp64 bound)"""
    c = case(name)
    ran = set()
    for l in range(c.nlev - 1):
        if not c.info[l]['f32']:
            continue
        coarse32 = c.info[l + 1]['f32']
        for what, v in c.inputs(l, 51 + l):
            got = c.field(c.k.mg_part(klib.MGP_RESTRICT, l, v, variant=1), l + 1)
            ref, bound = _transfer_bound(c, lambda a: mr.restrict(a, c.dim), f32(v), 9)
            if coarse32:
                assert np.all(np.abs(got - f32(ref)) <= ulp32(f32(ref))), ('RESTRICT<float,float>', l, what)
            else:
                assert np.all(np.abs(got - ref.astype(np.float64)) <= bound), ('RESTRICT<float,double>', l, what)
            ran.add('rff' if coarse32 else 'rfd')
            if coarse32:
                got = c.field(c.k.mg_part(klib.MGP_RESTRICT, l, v, variant=2), l + 1)
                ref = mr.restrict(v.astype(LD), c.dim)
                assert np.all(np.abs(got - f32(ref)) <= ulp32(f32(ref))), ('RESTRICT<double,float>', l, what)
                ran.add('rdf')
        fine = np.random.default_rng(61 + l).standard_normal((c.F,) + c.grid(l))
        for what, v in c.inputs(l + 1, 71 + l):
            got = c.field(c.k.mg_part(klib.MGP_PROLONG_ADD, l, fine, v, variant=1), l)
            ref = f32(f32(fine).astype(LD) + mr.prolong((f32(v) if coarse32 else v).astype(LD), c.dim))
            assert np.all(np.abs(got - ref) <= ulp32(ref)), ('PROLONG_ADD fp32', l, what, coarse32)
            ran.add('pff' if coarse32 else 'pdf')
    want = {'rfd', 'pdf'} | ({'rff', 'rdf', 'pff'} if sum(i['f32'] for i in c.info) >= 2 else set())
    assert ran == want, ran


# ---- 3. inverse point blocks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_inverse_point_blocks(name):
    c = case(name)
    for shift in (S_MILD, S_STIFF):
        for l, (inf, D) in enumerate(c.setup(shift)):
            M = mr.block_diag(c.coef(l)[0], c.h(l), c.lig, shift)
            cond = np.linalg.cond(M)
            assert cond.max() <= 1e6, (l, shift, float(cond.max()))
            ref = np.linalg.inv(M).astype(np.float32)
            err = np.abs(D - ref.astype(np.float64))
            assert np.all(err <= ulp32(ref)), ('DINV', l, shift, float((err / ulp32(ref)).max()))


@pytest.mark.parametrize('name', ['32x32', '40x24', '16x16x16', '130'])
def test_dinv_apply(name):
    c = case(name)
    for l, (inf, D) in enumerate(c.setup(S_MILD)):
        for what, r in c.inputs(l, 81 + l):
            variants = [0, 1] if c.info[l]['f32'] else [0]
            for variant in variants:
                z, z2, rcopy = (c.field(a, l) for a in c.k.mg_part(klib.MGP_DINV_APPLY, l, r, variant=variant, nu=3, shift=S_MILD))
                ref = mr.dinv_apply(D.astype(LD), r.astype(LD)) / LD(3)
                bound = (c.F + 3) * EPS * mr.dinv_apply(np.abs(D), np.abs(r)) / 3.0
                if variant == 0:
                    assert np.all(np.abs(z - ref.astype(np.float64)) <= bound), ('DINV_APPLY', l, what)
                    assert np.array_equal(rcopy, r)
                else:
                    assert np.all(np.abs(z - f32(ref)) <= ulp32(f32(ref))), ('DINV_APPLY fp32', l, what)
                    assert np.array_equal(rcopy, f32(r))
                assert np.array_equal(z2, z)


# ---- 4. the level operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES) + list(RING_CASES))
def test_level_operator(name):
    c = case(name)
    for l in range(c.nlev):
        C = c.planes(l).astype(LD)
        y = np.random.default_rng(91 + l).standard_normal((c.F,) + c.grid(l))
        for what, v in c.inputs(l, 95 + l):
            ref = mr.op_apply(C, v.astype(LD), c.h(l), c.lig, S_CYCLE)
            got1 = c.field(c.k.mg_part(klib.MGP_OPERATOR, l, v, variant=1, shift=S_CYCLE), l)
            got2 = c.field(c.k.mg_part(klib.MGP_OPERATOR, l, v, y, variant=2, shift=S_CYCLE), l)
            d1, d2 = per_field(got1, ref), per_field(got2, y.astype(LD) - ref)
            assert d1 < TOL_OP and d2 < TOL_OP, ('OPERATOR', l, what, d1, d2)
            if what != 'random':
                # two shifts: the difference is the shift on the diagonal and nothing else
                got0 = c.field(c.k.mg_part(klib.MGP_OPERATOR, l, v, variant=1, shift=S_MILD), l)
                D = got0 - got1
                j = int(np.flatnonzero(v.reshape(-1))[0])
                d = D.reshape(-1)[j]
                D.reshape(-1)[j] = 0.0
                assert not D.any(), ('OPERATOR two shifts', l, what)
                hu = lambda a: 0.5 * np.spacing(abs(a))
                assert abs(d - (S_MILD - S_CYCLE)) <= hu(got0.reshape(-1)[j]) + hu(got1.reshape(-1)[j]) + hu(d)
    if name.startswith('ring-'):
        one = case('twin-' + name)
        for l in range(c.nlev):
            for what, v in c.inputs(l, 95 + l):
                a, b = (x.k.mg_part(klib.MGP_OPERATOR, l, v, variant=1, shift=S_CYCLE) for x in (c, one))
                assert per_field(c.field(a, l), c.field(b, l)) < TOL_OP


def test_level_zero_operator_on_fp64_planes():
    """TUNE_POLY_FP64: level 0 reads the fp64 planes, and is compared on them"""
    c = case('64x48')
    try:
        c.k.set_tuning(use_fused=klib.TUNE_FUSED | klib.TUNE_POLY_FP64)
        C = c.coef(0)[0].astype(LD)
        for what, v in c.inputs(0, 97):
            ref = mr.op_apply(C, v.astype(LD), c.h(0), c.lig, S_CYCLE)
            got = c.field(c.k.mg_part(klib.MGP_OPERATOR, 0, v, variant=1, shift=S_CYCLE), 0)
            assert per_field(got, ref) < TOL_OP, what
            # ... and the planes matter: the default copy is a different operator at float32 size
            ref32 = mr.op_apply(c.coef(0)[1].astype(LD), v.astype(LD), c.h(0), c.lig, S_CYCLE)
            if what == 'random':
                assert per_field(got, ref32) > 100 * TOL_OP
    finally:
        c.k.set_tuning(use_fused=klib.TUNE_FUSED)


@pytest.mark.parametrize('name', FIRST_2D + ['ring-64x48'])
def test_level_operator_fp32(name):
    c = case(name)
    ran = 0
    for l in range(c.nlev):
        if not c.info[l]['f32']:
            continue
        C = c.coef(l)[1].astype(LD)                          # mg_op<float> reads the fp32 copy on every level that has one
        y = np.random.default_rng(101 + l).standard_normal((c.F,) + c.grid(l))
        v = c.inputs(l, 105 + l)[0][1]
        ref = y.astype(LD) - mr.op_apply(C, v.astype(LD), c.h(l), c.lig, S_CYCLE)
        ref32 = mr.store_f32(mr.store_f32(y.astype(LD)) - mr.op_apply(C, mr.store_f32(v.astype(LD)), c.h(l), c.lig, S_CYCLE))
        d32 = mr.rel_l2(ref32, ref)
        got = c.field(c.k.mg_part(klib.MGP_OPERATOR, l, v, y, variant=32, shift=S_CYCLE), l)
        d = mr.rel_l2(got, ref)
        print('mg_parts OPERATOR fp32 %s level %d: d32 %.3e distance %.3e head-room %.2f' % (name, l, d32, d, 4 * d32 / d))
        assert d32 < 1e-5 and d <= 4 * d32, (l, d, d32)
        ran += 1
    assert ran


# ---- 5. Chebyshev bounds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_chebyshev_bound_is_a_power_iteration_quotient(name):
    c = case(name)
    for shift in (S_MILD, S_CYCLE):
        for l, (inf, D) in enumerate(c.setup(shift)):
            if c.F * inf['points'] > 1024:
                continue
            A = mr.dense_operator(c.planes(l), c.h(l), c.lig, shift, c.F)
            N = inf['points']
            DA = np.empty_like(A)
            for j in range(A.shape[1]):
                DA[:, j] = mr.dinv_apply(D, A[:, j].reshape((c.F,) + c.grid(l))).reshape(-1)
            norm2 = np.linalg.norm(DA, 2)
            rho = np.abs(np.linalg.eigvals(DA)).max()
            print('mg_parts lam_max %s level %d shift %.4g: lam_max %.6f |DinvA|_2 %.6f rho %.6f lam_max/rho %.4f' %
                  (name, l, shift, inf['lam_max'], norm2, rho, inf['lam_max'] / rho))
            assert inf['lam_max'] / 1.15 <= norm2 * (1 + 1e-6), (l, shift, inf['lam_max'], norm2)


# ---- 6. the smoother ---------------------------------------------------------------------------------------------------------------------
SMOOTH_RUNS = [(1, True), (2, False), (2, True), (3, False), (5, False)]         # (nu, nonzero guess)


@pytest.mark.parametrize('tune', [0, klib.TUNE_UNFUSED_SMOOTHER])
@pytest.mark.parametrize('name', SMOOTH_CASES)
def test_smoother(name, tune):
    c = case(name)
    try:
        c.k.set_tuning(use_fused=klib.TUNE_FUSED | tune)
        lv64, lvld = c.levels(S_CYCLE, tune), c.levels(S_CYCLE, tune, LD)
        for l in range(c.nlev):
            b = np.random.default_rng(111 + l).standard_normal((c.F,) + c.grid(l))
            x0 = np.random.default_rng(115 + l).standard_normal((c.F,) + c.grid(l))
            b.reshape(-1)[0] += 1.0
            b.reshape(-1)[-1] += 1.0
            for ratio in (MG_RATIO, lv64[l].ratio):
                for nu, guess in SMOOTH_RUNS:
                    ref = {}
                    for key, L in (('f64', lv64[l]), ('ld', lvld[l])):
                        dt = L.C.dtype
                        A = lambda v, L=L: mr.op_apply(L.C, v, L.h, c.lig, S_CYCLE)
                        ref[key] = mr.cheb_smooth(A, L.Dinv, b.astype(dt), x0.astype(dt) if guess else None, nu, L.lam_max, ratio)
                    d_ref = mr.rel_l2(ref['f64'], ref['ld'])
                    got = c.field(c.k.mg_part(klib.MGP_SMOOTH, l, b, x0 if guess else None, nu=nu, shift=S_CYCLE, ratio=ratio), l)
                    d, bound = mr.rel_l2(got, ref['ld']), MARGIN * max(d_ref, TOL_OP)
                    print('mg_parts SMOOTH %s level %d %s nu %d %s ratio %.4g: d_ref %.3e distance %.3e head-room %.1f' %
                          (name, l, 'unfused' if tune else 'fused', nu, 'guess' if guess else 'zero', ratio, d_ref, d, bound / max(d, 1e-300)))
                    assert d <= bound, ('SMOOTH', l, nu, guess, ratio, d, d_ref)
    finally:
        c.k.set_tuning(use_fused=klib.TUNE_FUSED)


# ---- 7. the cycle ------------------------------------------------------------------------------------------------------------------------
def _cycle_refs(c, exact, b, lv):
    """lv: the reference levels, made once per test (an exact coarse solve keeps its dense matrix in them)"""
    end = c.k.mg_coarse_info()['level']
    if not lv:
        lv['f64'], lv['ld'] = c.levels(S_CYCLE), c.levels(S_CYCLE, 0, LD)
    lv64, lvld = lv['f64'], lv['ld']
    x64 = mr.vcycle(lv64, c.lig, S_CYCLE, b, 2, MG_RATIO, end=end, exact=exact)
    xld = mr.vcycle(lvld, c.lig, S_CYCLE, b.astype(LD), 2, MG_RATIO, end=end, exact=exact)
    nstore = sum(1 for l in range(c.nlev) if c.info[l]['f32'] and not (exact and l == end))
    if not nstore:
        return x64, xld, None, None
    # the cycle with fp32 level vectors reads the fp32 coefficient copy on every level it keeps in fp32 (the fp64 cycle: on level 0 alone):
    # its reference pair runs on those planes, as every part is compared on the planes it really reads
    if 'copies' not in lv:
        lv['copies'] = c.levels(S_CYCLE, copies=nstore)
    lvc = lv['copies']
    x64c = mr.vcycle(lvc, c.lig, S_CYCLE, b, 2, MG_RATIO, end=end, exact=exact)
    x32c = mr.vcycle(lvc, c.lig, S_CYCLE, b, 2, MG_RATIO, end=end, exact=exact, store=mr.store_f32, nstore=nstore)
    return x64, xld, x64c, x32c


@pytest.mark.parametrize('coarse', ['cheb', 'lu'])
@pytest.mark.parametrize('name', list(CASES) + list(RING_CASES))
def test_cycle(name, coarse):
    c = case(name)
    exact = coarse == 'lu'
    if exact and name not in FIRST_2D:
        return                                              # the exact coarse solve: the first three 2-D cases
    ring = name.startswith('ring-')
    try:
        if exact:
            c.k.set_mg_coarse(1)
        lv = {}
        for what, b in c.inputs(0, 121)[:2 if exact else 3]:
            if what == 'impulse-first':
                b = b + c.inputs(0, 0)[2][1]                   # both impulses in one right-hand side
            x64, xld, x64c, x32 = _cycle_refs(c, exact, b, lv)
            d_ref = mr.rel_l2(x64, xld)
            got = {}
            for eager in ([True] if ring else [False, True]):  # a handle with a halo transport always launches eagerly
                c.k.set_mg_params(power_its=klib.MG_EAGER if eager else 0)
                g = c.field(c.k.mg_part(klib.MGP_CYCLE, 0, b, variant=0, shift=S_CYCLE), 0)
                d, bound = mr.rel_l2(g, xld), MARGIN * max(d_ref, TOL_OP)
                print('mg_parts CYCLE fp64 %s %s %s %s: d_ref %.3e distance %.3e head-room %.1f' %
                      (name, coarse, 'eager' if eager else 'graph', what, d_ref, d, bound / max(d, 1e-300)))
                assert d <= bound, ('CYCLE', eager, d, d_ref)
                got[eager] = g
                if x32 is not None and (not ring or c.dim == 2):
                    g32 = c.field(c.k.mg_part(klib.MGP_CYCLE, 0, b, variant=1, shift=S_CYCLE), 0)
                    d32, dg = mr.rel_l2(x32, x64c), mr.rel_l2(g32, x64c)
                    print('mg_parts CYCLE fp32 %s %s %s %s: d32 %.3e distance %.3e head-room %.2f (effect of the coarse fp32 coefficient copies on the fp64 reference: %.3e)' %
                          (name, coarse, 'eager' if eager else 'graph', what, d32, dg, 4 * d32 / max(dg, 1e-300), mr.rel_l2(x64c, x64)))
                    assert d32 < 1e-5 and dg <= 4 * d32, ('CYCLE fp32', eager, dg, d32)
                    got[(eager, 32)] = g32
            if not ring:
                assert np.array_equal(got[False], got[True])
                if (False, 32) in got:
                    assert np.array_equal(got[(False, 32)], got[(True, 32)])
            else:
                # the wrap-index twin runs ANOTHER cycle: its power iteration starts from a hash fill of the plane without ghost rows, so its
                # Chebyshev bounds differ in the third digit.  Both meet the bound above on their own bounds; the parts that have no set-up
                # (RESTRICT, PROLONG_ADD, OPERATOR) are compared between the two handles in their tests
                one = case('twin-' + name)
                lam = [[x[0]['lam_max'] for x in h.setup(S_CYCLE)] for h in (c, one)]
                print('mg_parts CYCLE %s: lam_max per level with ghost rows %s, with wrapped indices %s' % (name, lam[0], lam[1]))
    finally:
        c.k.set_mg_params(power_its=0)
        if exact:
            c.k.set_mg_coarse(0)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def _einval(fn, word=None):
    with pytest.raises(klib.KSFDError) as e:
        fn()
    assert e.value.code == klib.EINVAL, str(e.value)
    if word:
        assert word in str(e.value), str(e.value)


def test_refused_calls():
    c = case('32x32')
    v0, v2 = np.ones((2, 32, 32)), np.ones((2, 8, 8))
    one = lambda **kw: c.k.L.ksfd_mg_part(c.k.h, kw.get('part', klib.MGP_SMOOTH), kw.get('level', 0), kw.get('variant', 0), kw.get('nu', 2),
                                          S_CYCLE, kw.get('ratio', 6.0), klib._dp(v0), None, klib._dp(np.empty_like(v0)), None)
    for kw in (dict(level=-1), dict(level=3), dict(nu=0), dict(nu=6), dict(ratio=1.0), dict(part=8), dict(part=klib.MGP_CYCLE, level=1),
               dict(part=klib.MGP_OPERATOR, variant=32, level=2), dict(part=klib.MGP_RESTRICT, level=2), dict(part=klib.MGP_RESTRICT, level=1, variant=2),
               dict(part=klib.MGP_PROLONG_ADD, level=0), dict(part=klib.MGP_OPERATOR, variant=2)):
        assert one(**kw) == klib.EINVAL, kw
    _einval(lambda: c.k.mg_level_info(3), 'level')
    c3 = case('16x16x16')
    _einval(lambda: c3.k.mg_part(klib.MGP_CYCLE, 0, np.ones((2, 16, 16, 16)), variant=1, shift=S_CYCLE), 'fp32')
    _einval(lambda: c3.k.mg_part(klib.MGP_RESTRICT, 0, np.ones((2, 16, 16, 16)), variant=1))


def _steps(k, n=2):
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, pc_type=1)
    t, h, out = 0.0, 5.0, []
    for _ in range(n):
        t, h, st, rc = k.step(t, h, opts)
        out.append((t, h, st.linear_its, st.rejections, st.pc_used, k.get_state()))
    return out


def test_handle_without_a_hierarchy_refuses_and_stays_as_it_was():
    cfg = _cfg((33, 20), 1, (0.0825, 0.05))
    u = _state(cfg, 3, amp=0.05)
    out = []
    for attempt in (False, True):
        k = klib.KSFDHip(cfg)
        k.set_state(u)
        first = _steps(k, 1)
        if attempt:
            _einval(lambda: k.mg_level_info(0), 'hierarchy')
            v = np.ones(2 * 33 * 20)
            for part in range(8):
                assert k.L.ksfd_mg_part(k.h, part, 0, 0, 2, S_CYCLE, 6.0, klib._dp(v), klib._dp(v), klib._dp(v.copy()), klib._dp(np.empty(4 * v.size))) == klib.EINVAL
            assert 'hierarchy' in k.last_error()
        k.set_state(u)
        out.append((first, _steps(k, 1)))
        k.close()
    for a, b in zip(out[0], out[1]):
        assert a[0][:5] == b[0][:5] and np.array_equal(a[0][5], b[0][5])


def test_steps_after_the_entry_equal_steps_on_a_fresh_handle():
    """default tuning, 2-D: every part once (both cycles, graph captured and dropped), then the same steps as a handle that never saw the entry"""
    cfg = _cfg((64, 48), 2, (0.16, 0.12))
    u = _state(cfg, 3, amp=0.05)
    out = []
    for touch in (False, True):
        k = klib.KSFDHip(cfg)
        k.set_state(u)
        if touch:
            rng = np.random.default_rng(1)
            v0, v1 = rng.standard_normal((3, 48, 64)), rng.standard_normal((3, 24, 32))
            k.mg_level_info(1, S_CYCLE)
            k.mg_part(klib.MGP_COEF, 1)
            for variant in (0, 1, 2):
                k.mg_part(klib.MGP_RESTRICT, 0, v0, variant=variant)
            for variant in (0, 1):
                k.mg_part(klib.MGP_PROLONG_ADD, 0, v0, v1, variant=variant)
                k.mg_part(klib.MGP_CYCLE, 0, v0, variant=variant, shift=S_CYCLE)
                k.mg_part(klib.MGP_DINV_APPLY, 0, v0, variant=variant, shift=S_MILD)
            k.mg_part(klib.MGP_OPERATOR, 0, v0, v0, variant=32, shift=S_MILD)
            k.mg_part(klib.MGP_OPERATOR, 1, v1, v1, variant=2, shift=S_MILD)
            k.mg_part(klib.MGP_DINV, 2, shift=S_STIFF)
            for nu in (2, 3):
                k.mg_part(klib.MGP_SMOOTH, 1, v1, v1, nu=nu, shift=S_STIFF, ratio=6.0)
            assert np.array_equal(k.get_state(), u)
        out.append(_steps(k, 3))
        k.close()
    for a, b in zip(*out):
        assert a[4] & klib.PC_MULTIGRID
        assert a[:5] == b[:5] and np.array_equal(a[5], b[5])


# ---- 9. two slab ranks ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _pair_worker(rank, size, port, outdir):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    try:
        from ksfd_amd.dist import open_handle, local_slab
        shape, nlig = (64, 48), 1
        cfg = _cfg(shape, nlig, (0.16, 0.12))
        u = _state(cfg, 3, amp=0.05)
        ks, keep = open_handle(cfg, rank, size, 0, transport='host')
        ks.set_state(local_slab(u, cfg, rank, size))
        F = cfg.F
        info = [ks.mg_level_info(l) for l in range(ks.mg_level_info(0)['nlevels'])]
        rng = np.random.default_rng(7)
        res = {'nlev': len(info), 'sloc': np.array([i['sloc'] for i in info]), 'nx': np.array([i['n'][0] for i in info])}

        def mine(a, l):                                    # rows of this rank on level l
            s = info[l]['sloc']
            return np.ascontiguousarray(a[:, rank * s:(rank + 1) * s, :])
        glob = lambda l: (F, info[l]['sloc'] * size, info[l]['n'][0])
        for l in range(len(info) - 1):
            v, w = rng.standard_normal(glob(l)), rng.standard_normal(glob(l + 1))
            for a in (v, w):
                a[0, 0, 0] += 1.0
                a[-1, -1, -1] += 1.0
            res['rin%d' % l], res['pin%d' % l] = v, w
            res['r%d' % l] = ks.mg_part(klib.MGP_RESTRICT, l, mine(v, l))
            res['p%d' % l] = ks.mg_part(klib.MGP_PROLONG_ADD, l, mine(v, l), mine(w, l + 1))
        b = rng.standard_normal(glob(0))
        b[0, 0, 0] += 1.0
        b[-1, -1, -1] += 1.0
        res['b'] = b
        res['cycle'] = ks.mg_part(klib.MGP_CYCLE, 0, mine(b, 0), variant=0, shift=S_CYCLE)
        for l in range(len(info)):
            inf = ks.mg_level_info(l, S_CYCLE)
            res['coef%d' % l] = ks.mg_part(klib.MGP_COEF, l)[0]
            c32 = ks.mg_part(klib.MGP_COEF, l)[1]
            if l == 0 and c32 is not None:
                res['coef32'] = c32
            res['dinv%d' % l] = ks.mg_part(klib.MGP_DINV, l, shift=S_CYCLE)
            res['set%d' % l] = np.array([inf['lam_max'], inf['ratio'], inf['coarse_sweeps']])
        ks.close()
        np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **res)
    finally:
        dist.destroy_process_group()


def test_two_slab_ranks(tmp_path):
    """(64, 48) on 2 ranks: the only place a slab that does not start at row 0 is checked.  RESTRICT, PROLONG_ADD and the fp64 CYCLE,
    assembled from the slabs and compared with the reference (fed the assembled planes, blocks and bounds of the two ranks)"""
    import torch.multiprocessing as mp
    mp.spawn(_pair_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    z = [np.load(str(tmp_path / ('rank%d.npz' % r))) for r in range(2)]
    nlev, F = int(z[0]['nlev']), 2
    sloc, nx = z[0]['sloc'], z[0]['nx']
    assert nlev >= 2 and sloc[0] == 24

    def whole(key, l, planes=F):
        return np.concatenate([zz[key].reshape(planes, sloc[l], nx[l]) for zz in z], axis=1)
    for l in range(nlev - 1):
        v, w = z[0]['rin%d' % l], z[0]['pin%d' % l]
        ref = mr.restrict(v.astype(LD), 2)
        bound = 11 * EPS * mr.restrict(np.abs(v), 2)
        assert np.all(np.abs(whole('r%d' % l, l + 1) - ref.astype(np.float64)) <= bound), ('RESTRICT', l)
        ref = v.astype(LD) + mr.prolong(w.astype(LD), 2)
        bound = 7 * EPS * (np.abs(v) + mr.prolong(np.abs(w), 2))
        assert np.all(np.abs(whole('p%d' % l, l) - ref.astype(np.float64)) <= bound), ('PROLONG_ADD', l)
    cfg = _cfg((64, 48), 1, (0.16, 0.12))
    lig = dict(s=list(cfg.lig_s), gamma=list(cfg.lig_gamma), D=list(cfg.lig_D))
    levels = []
    for l in range(nlev):
        C = whole('coef32', 0, 3 + 1) if (l == 0 and 'coef32' in z[0]) else whole('coef%d' % l, l, 3 + 1)
        lam, ratio, sweeps = z[0]['set%d' % l]
        assert np.array_equal(z[0]['set%d' % l], z[1]['set%d' % l])
        levels.append(mr.Level(C, [0.0025 * 2 ** l] * 2, mr.planes_to_blocks(whole('dinv%d' % l, l, F * F), F), float(lam), float(ratio), int(sweeps)))
    b = z[0]['b']
    x64 = mr.vcycle(levels, lig, S_CYCLE, b, 2, MG_RATIO)
    xld = mr.vcycle([L.astype(LD) for L in levels], lig, S_CYCLE, b.astype(LD), 2, MG_RATIO)
    d_ref, d = mr.rel_l2(x64, xld), mr.rel_l2(whole('cycle', 0), xld)
    print('mg_parts CYCLE fp64 2 ranks 64x48: d_ref %.3e distance %.3e head-room %.1f' % (d_ref, d, MARGIN * max(d_ref, TOL_OP) / d))
    assert d <= MARGIN * max(d_ref, TOL_OP)
