"""GPU: the stage right-hand sides and the frozen Jacobian action of ksfd_step in every launch mode, through the test entries
ksfd_stage_rhs and ksfd_stage_jvp -- which run the functions the step calls (stage_rhs, stage_gram_guess, step_finish, err_materialize,
op_jvp_frozen_halo, op_residual32, poly_apply) and launch nothing of their own.

References (never the library):
  RHS        ko.Oracle.rhs (sources of stage 2, stage parameters of stage 1 from a second Oracle) at u + sum At[i][j] Y_j, minus
             sum Ginv[i][j]/h Y_j in longdouble; the tableau is ko.tableau()
  action     tests/mg_reference.op_apply in longdouble on the level-0 planes downloaded with MGP_COEF where the handle has a hierarchy,
             else shift*v - Oracle.jvp
  sums, norms, wrms, completion: longdouble numpy
Which kernel variant ran is pinned by the bytes and launches ksfd_get_profile books (op_rhs charges carry, non-carry, GPLANE and the dG
pass differently), and by the launch geometry the entries report against a Python copy of strips_for / k3d_for.

Tolerances (none tuned on the kernels):
  b_i per field        max|got - ref| <= 1e-12 max(|f(z)| + sum |a_out,j| |Y_j|)        (TOL of tests/test_gpu_operators.py)
  ||b||^2, <b_i, b_j>  n eps sum|terms| against longdouble sums over the downloaded b (a lost wave partial is >= 1/nwaves of the sum)
  completion           new state, error vector: 1e-14 sum|terms| per element (sums of five terms; the plain relative form where nothing
                       cancels); wrms^2 n eps; the count under the floor exact
  action fp64          rel-L2 per field 1e-12, (deg + 1) 1e-12 for the polynomial
  fp32 residual        |got - ref| <= 2^-24 |ref| + 1e-12 scale per element; ||r||^2 is the sum of the UNROUNDED fp64 values (every
                       kernel accumulates a*a before the store converts), asserted at n eps sum against the fp64 residual of the same
                       launch mode (op 0, mode 2) and, with the fp64 tolerance propagated, against the longdouble reference
  fp32 polynomial      d <= max(4 d32, (deg + 1) 1e-12): d32 = distance of the Horner recurrence with float32-stored temporaries
                       (mr.store_f32) from the exact one, both on the downloaded fp32 planes (degree 1 has no fp32 temporary)
The long-segment child test prints its figures; duration of the file on an MI355X: profiles/stage_ops_runs.log."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mg_reference as mr
from conftest import ROOT
from ksfd_amd.config import ProblemConfig
from ksfd_amd import lib as klib
from oracle import ko

pytestmark = pytest.mark.gpu
GAMMA = 0.43586652150845900
EPS = np.finfo(float).eps
LD = np.longdouble
TOL = 1e-12                                   # tests/test_gpu_operators.py
TOL_OP = 1e-12
HSTEP = 0.05
S_A, S_B = 1.0 / (GAMMA * 0.05), 1.0 / (GAMMA * 5.0)
STRIP_OUT, WAVES_RHS, WAVES_JVP, YSEG_RHS, YSEG_JVP, ZSEG, BLOCKS3D = 124, 6144, 4096, 48, 16, 32, 1024
AT, GINV, BT, B2T, _ = ko.tableau()

#        name          shape, ligands, ring, path of the action
CASES = {'6x5': ((6, 5), 1, False, klib.JP_STRIP2D),                  # smallest grid the strip kernel gets: ksfd_create takes no axis under 5 points
         '8x5': ((8, 5), 2, False, klib.JP_STRIP2D),                  # last segment of one row
         '124x6': ((124, 6), 1, False, klib.JP_STRIP2D),              # exactly one full strip
         '126x8': ((126, 8), 3, False, klib.JP_STRIP2D),              # two unequal strips
         '250x9': ((250, 9), 4, False, klib.JP_STRIP2D),              # three strips
         '64x48': ((64, 48), 2, False, klib.JP_STRIP2D),              # a hierarchy: stored right-hand sides, fp32 planes to download
         '40x24': ((40, 24), 3, False, klib.JP_STRIP2D),              # ... three ligands
         '32x16': ((32, 16), 4, False, klib.JP_STRIP2D),              # ... four
         '37x21': ((37, 21), 1, False, klib.JP_GENERIC),              # odd nx
         '24x20': ((24, 20), 9, False, klib.JP_GENERIC),              # more than four ligands
         '96': ((96,), 1, False, klib.JP_GENERIC),                    # 1-D
         '16x16x12': ((16, 16, 12), 2, False, klib.JP_LDS3D),
         '16x12x10': ((16, 12, 10), 1, False, klib.JP_STRIP3D),
         '16x10x9': ((16, 10, 9), 1, False, klib.JP_STRIP3D),         # ragged y group, no plane barrier
         '24x9x40': ((24, 9, 40), 3, False, klib.JP_STRIP3D),
         'ring-36x20': ((36, 20), 1, True, klib.JP_STRIP2D),          # >= 3 segments: interior + boundary launches, split partials
         'ring-64x8': ((64, 8), 2, True, klib.JP_STRIP2D),            # four segments of two rows (strips_for leaves no grid of >= 5 rows fewer than 3
                                                                      # segments): one launch only with TUNE_NO_OVERLAP, or in the long-segment child
         'ring-64x48': ((64, 48), 1, True, klib.JP_STRIP2D),          # ... with a hierarchy: the inner products in split partials
         # the long-segment cases (child process / 3-D test only)
         '130x37': ((130, 37), 2, False, klib.JP_STRIP2D),
         '130x40': ((130, 40), 2, False, klib.JP_STRIP2D),
         'ring-130x40': ((130, 40), 2, True, klib.JP_STRIP2D),
         '8x64x512': ((8, 64, 512), 1, False, klib.JP_LDS3D),
         '8x60x512': ((8, 60, 512), 1, False, klib.JP_STRIP3D)}
SMALL = [n for n in CASES if n not in ('130x37', '130x40', 'ring-130x40', '8x64x512', '8x60x512')]
WITH_PLANES = ['64x48', '40x24', '32x16', 'ring-64x48']               # strip path and a hierarchy: fp32 planes can be downloaded


def _cfg(shape, nlig, L):
    """configuration of the multigrid parity tests (tests/test_gpu_mg_coarse.py): attractant, repellent of options84, one more attractant"""
    dim = len(shape)
    if nlig <= 2:
        return ProblemConfig.standard(dim, shape, L=L, nlig=nlig)
    return ProblemConfig(dim=dim, n=shape, L=L, lig_group=[0, 1, 0][:nlig], lig_w=[1.0, 1.0, 0.5][:nlig], lig_s=[0.01, 0.001, 0.003][:nlig],
                         lig_gamma=[0.01, 0.001, 0.004][:nlig], lig_D=[1e-6, 1e-5, 3e-6][:nlig], grp_alpha=[1500.0, 1500.0],
                         grp_beta=[5.56e-4, -5.56e-4])


def _state(cfg, seed, amp=0.01):
    """the near-uniform state of the existing parity tests: rho = 9000 (1 + amp N(0,1)), ligands at their equilibrium with rho"""
    rng = np.random.default_rng(seed)
    rho = 9000.0 * (1.0 + amp * rng.standard_normal(cfg.N))
    return np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] for l in range(cfg.nlig)])


def make_cfg(shape, nlig, tweak=False):
    """the configurations of the existing parity tests; tweak: other parameters of the same problem (stage parameters)"""
    dim = len(shape)
    L = tuple((0.01 if dim == 3 else 0.0025) * n for n in shape)
    f = 1.07 if tweak else 1.0
    if nlig <= 3:
        c = _cfg(shape, nlig, L)
        if not tweak:
            return c
        return ProblemConfig(dim=dim, n=shape, L=L, lig_group=list(c.lig_group), lig_w=list(c.lig_w), lig_s=[f * x for x in c.lig_s],
                             lig_gamma=[x / f for x in c.lig_gamma], lig_D=list(c.lig_D), grp_alpha=[f * x for x in c.grp_alpha],
                             grp_beta=list(c.grp_beta))
    rng = np.random.default_rng(21)           # tests/test_gpu_operators.py: nine ligands in three groups
    return ProblemConfig(dim=dim, n=shape, L=L, lig_group=[l % 3 for l in range(nlig)], lig_w=0.5 + rng.random(nlig),
                         lig_s=f * (0.005 + 0.01 * rng.random(nlig)), lig_gamma=(0.005 + 0.01 * rng.random(nlig)) / f,
                         lig_D=1e-6 * (1 + rng.random(nlig)), grp_alpha=[f * 1500.0, 1200.0, 1800.0], grp_beta=[5.56e-4, -3e-4, 2e-4])


def strips(nx, sloc, yseg, target):
    """ops.hip.h: strips_for"""
    nstrips = -(-nx // STRIP_OUT)
    seg = min(yseg, max(nstrips * sloc // target, 2))
    return dict(seg=seg, nseg=-(-sloc // seg), nstrips=nstrips)


def k3d(shape, rows, zseg=ZSEG, target=BLOCKS3D):
    """ops.hip.h: k3d_for"""
    nx, ny, nz = shape
    nstrips, nygrp = -(-nx // STRIP_OUT), -(-ny // rows)
    seg = min(zseg, max(nstrips * nygrp * nz // target, 2))
    return dict(seg=seg, nseg=-(-nz // seg), nstrips=nstrips, rows=rows)


class Case:
    """one handle at the near-uniform state of the existing tests, clean or with what the groom would touch, and the references"""

    def __init__(self, name, waves=(WAVES_RHS, WAVES_JVP)):
        self.name = name
        self.shape, self.nlig, self.ring, self.path = CASES[name]
        self.dim, self.waves = len(self.shape), waves
        self.cfg, self.cfg2 = make_cfg(self.shape, self.nlig), make_cfg(self.shape, self.nlig, tweak=True)
        self.F, self.N = self.cfg.F, self.cfg.N
        self.n = self.F * self.N
        self.o, self.o2 = ko.Oracle(self.cfg), ko.Oracle(self.cfg2)
        if self.ring:
            from ksfd_amd.dist import open_self_ring
            self.k, self._keep = open_self_ring(self.cfg, 0, 'host')
        else:
            self.k = klib.KSFDHip(self.cfg)
        self.plane = int(self.k.L.ksfd_device_plane_stride(self.k.h))
        rng = np.random.default_rng(17)
        self.clean = _state(self.cfg, 3, amp=0.05)
        N = self.N
        # what the groom would touch: one NaN, one negative value; points under the floor come with the stage vectors
        self.dirty = self.clean.copy()
        self.dirty[N // 3] = np.nan
        self.dirty[self.n - 1 - N // 5] = -3.0
        # stage vectors: random, an impulse at the first owned point of field 0 and one at the last owned point of the last field
        self.Y = 30.0 * rng.standard_normal((4, self.n))
        self.Y[:, 0] += 300.0 * np.array([1.0, -0.5, 0.25, 2.0])
        self.Y[:, -1] += 300.0 * np.array([-1.0, 0.5, 2.0, 0.25])
        # ... and two points where u + sum a Y falls under its floor in every stage (At[i][0] >= 1.4) and in the completion (bt[0] = 4.2)
        self.Yd = self.Y.copy()
        for p in (N // 2 + 1, self.n - 1 - N // 2):
            self.Yd[:, p] = 0.0
            self.Yd[0, p] = -2.0 * self.clean[p]
        self.src = [rng.standard_normal(N) * 50.0 for _ in range(self.F)]
        for c in range(self.F):
            self.k.set_source(c, self.src[c], stage=2)
        self.k.set_stage_params(1, self.cfg2)
        self.state = None
        self._ref, self._planes = {}, {}
        self.h = [self.cfg.L[a] / self.shape[a] for a in range(self.dim)]
        self.lig = dict(s=list(self.cfg.lig_s), gamma=list(self.cfg.lig_gamma), D=list(self.cfg.lig_D))
        self.grid = mr.grid_shape(self.shape)

    def use(self, kind):
        if self.state != kind:
            self.k.set_state(self.clean if kind == 'clean' else self.dirty)
            self.state = kind
        return self.clean if kind == 'clean' else self.dirty

    def inputs(self, kind):
        return (self.clean, self.Y) if kind == 'clean' else (self.dirty, self.Yd)

    # ---- geometry the handle must report
    def rhs_geometry(self, yseg=YSEG_RHS, tune=0):
        if self.path == klib.JP_STRIP2D:
            return dict(strips(self.shape[0], self.shape[1], yseg, self.waves[0]), rows=0)
        if self.path in (klib.JP_LDS3D, klib.JP_STRIP3D) and not tune & klib.TUNE_GENERIC_RHS3D:
            return k3d(self.shape, 4)
        return dict(seg=0, nseg=0, nstrips=0, rows=0)

    def jvp_geometry(self, yseg=YSEG_JVP):
        if self.path == klib.JP_STRIP2D:
            return dict(strips(self.shape[0], self.shape[1], yseg, self.waves[1]), rows=0)
        if self.path == klib.JP_LDS3D:
            return k3d(self.shape, 8)
        if self.path == klib.JP_STRIP3D:
            return k3d(self.shape, 4)
        return dict(seg=0, nseg=0, nstrips=0, rows=0)

    # ---- references
    def rhs_ref(self, kind):
        """per stage: (reference b_i in longdouble, scale |f(z)| + sum |a_out| |Y_j|)"""
        if kind not in self._ref:
            u, Y = self.inputs(kind)
            out = []
            for i in range(4):
                z = u.astype(LD)
                add, scale = np.zeros(self.n, dtype=LD), np.zeros(self.n, dtype=LD)
                for j in range(i):
                    z = z + LD(AT[i][j]) * Y[j]
                    aout = -GINV[i][j] / HSTEP
                    add = add + LD(aout) * Y[j]
                    scale = scale + abs(LD(aout)) * np.abs(Y[j])
                f = (self.o2 if i == 1 else self.o).rhs(z.astype(np.float64), self.src if i == 2 else None)
                assert np.isfinite(f).all()
                out.append((f.astype(LD) + add, np.abs(f).astype(LD) + scale))
            self._ref[kind] = out
        return self._ref[kind]

    def planes(self, kind):
        """(fp64 planes, fp32 copy) of level 0 in longdouble as downloaded, or (None, None) on a handle without a hierarchy"""
        if kind not in self._planes:
            self.use(kind)
            try:
                c, c32 = self.k.mg_part(klib.MGP_COEF, 0)
                shp = (3 + self.nlig,) + self.grid
                self._planes[kind] = (c.reshape(shp).astype(LD), None if c32 is None else c32.reshape(shp).astype(LD))
            except klib.KSFDError as e:
                assert e.code == klib.EINVAL
                self._planes[kind] = (None, None)
        return self._planes[kind]

    def A(self, kind, v, shift, fp32_planes=False):
        """(shift I - J) v in longdouble, (F, *grid)"""
        C, C32 = self.planes(kind)
        v = np.asarray(v).reshape((self.F,) + self.grid)
        if fp32_planes:
            assert C32 is not None
            return mr.op_apply(C32, v.astype(LD), self.h, self.lig, shift)
        if C is not None:
            return mr.op_apply(C, v.astype(LD), self.h, self.lig, shift)
        u = self.clean if kind == 'clean' else self.dirty
        return LD(shift) * v.astype(LD) - self.o.jvp(u, v.reshape(-1)).reshape(v.shape).astype(LD)

    def vectors(self, seed):
        """random with an impulse at the first owned point of field 0 and one at the last owned point of the last field, and the two impulses alone"""
        rng = np.random.default_rng(seed)
        v = rng.standard_normal(self.n)
        v[0] += 40.0
        v[-1] -= 40.0
        e0, e1 = np.zeros(self.n), np.zeros(self.n)
        e0[0], e1[-1] = 1.0, 1.0
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


def per_field(got, ref, F):
    """largest rel-L2 distance of a field; a field the reference leaves zero must be zero"""
    got, ref = np.asarray(got).reshape(F, -1), np.asarray(ref).reshape(F, -1)
    return max((mr.rel_l2(got[c], ref[c]) if np.any(ref[c]) else (np.inf if np.any(got[c]) else 0.0)) for c in range(F))


def fields_within(got, ref, scale, F, tol):
    """largest max|got - ref| / (tol max scale) of a field"""
    got, ref, scale = (np.asarray(a).reshape(F, -1) for a in (got, ref, scale))
    return max(float(np.abs(got[c].astype(LD) - ref[c]).max() / (LD(tol) * scale[c].max())) for c in range(F))


def dot_ld(a, b):
    t = a.astype(LD) * b.astype(LD)
    return t.sum(), np.abs(t).sum()


# ---- what op_rhs books for the four stages of one call (ops.hip.h: the Scopes of op_rhs) -----------------------------------------------------
def expected_books(c, tune, info):
    """{class: (launches, implementation bytes)} of rhs, gfield, lincomb, multidot for four stages, and the arms the call must have taken"""
    F, N, P = c.F, c.N, c.plane
    vb = lambda k: k * 8.0 * F * N
    nin = [0, 1, 2, 3]                                     # nonzeros of At[i][:i] and of Ginv[i][:i]: every earlier stage, both sides
    rhs_l = rhs_b = gf_l = gf_b = lin_l = 0
    arms = set()
    fused = info['fuse_stage']
    for i in range(4):
        nd = min(i, 2) if info['dots_done'][i] else 0
        halo_split = info['overlap'] and i > 0 and fused          # the newest stage vector's ghost rows travel behind the interior rows
        if c.path == klib.JP_STRIP2D:
            if fused:
                gplane = i == 0 and not tune & klib.TUNE_NO_GPLANE
                carry = i > 0 and not tune & klib.TUNE_NO_RHS_CARRY
                rhs_b += vb(2 + nin[i] + (0 if carry or i == 0 else nin[i]) + nd) + (8.0 * N if gplane else 0.0)
                arms.add('gplane' if gplane else 'carry' if carry else 'plain' if i == 0 else 'yout')
            else:
                gplane = i == 0 and not tune & klib.TUNE_NO_GPLANE
                rhs_b += vb(2) + (8.0 * N if gplane else 0.0)
                lin_l += 2 if i > 0 else 0
                arms.add('unfused2d')
            rhs_l += 2 if halo_split else 1
            if nd:
                arms.add('dots-epilogue')
        elif c.path in (klib.JP_LDS3D, klib.JP_STRIP3D) and not tune & klib.TUNE_GENERIC_RHS3D:
            ni, no = (nin[i], nin[i]) if fused else (0, 0)
            if i > 0:                                              # stage 0 takes G from the coefficient planes: no pass
                gf_l += 1
                gf_b += 8.0 * ((1 + ni) * F + (F if ni else 0) + 1) * P
                lin_l += 0 if fused else 2
            rhs_l += 1
            rhs_b += 8.0 * (2.0 * F + 1 + no * F) * N
            arms.add('strip3d-comb' if fused and i > 0 else 'strip3d')
        else:
            gf_l += 1
            gf_b += 8.0 * (F + 1) * P
            rhs_l += 1
            rhs_b += vb(2) + 8.0 * N
            lin_l += 2 if i > 0 else 0
            arms.add('generic')
    return dict(rhs=(rhs_l, rhs_b), gfield=(gf_l, gf_b), lincomb=lin_l), arms


def check_rhs(c, kind, regime, tune, yseg=None, say=None):
    """one call of four stages: every b_i, the epilogue scalars, the geometry and the books.  Returns (info, b, arms)"""
    u, Y = c.inputs(kind)
    c.use(kind)
    k = c.k
    k.set_tuning(use_fused=klib.TUNE_FUSED | tune, **({} if yseg is None else dict(yseg=yseg)))
    k.velocity_max()                                       # the CFL check makes the planes, as before a step: the call books the stages alone
    k.profile(reset=True)
    b, info, _ = k.stage_rhs(regime, HSTEP, Y[:3])
    prof = k.profile()
    tag = (c.name, kind, regime, hex(tune), yseg)
    # geometry
    geo = c.rhs_geometry(yseg or YSEG_RHS, tune)
    assert {q: info[q] for q in geo} == geo, (tag, info, geo)
    assert info['path'] == c.path and info['rhs_strip'] == (geo['nseg'] > 0)
    assert info['overlap'] == (c.ring and c.path == klib.JP_STRIP2D and geo['nseg'] >= 3 and not tune & klib.TUNE_NO_OVERLAP)
    strip_ok = c.path in (klib.JP_STRIP2D, klib.JP_STRIP3D, klib.JP_LDS3D) and c.nlig <= 4 and not (c.dim == 3 and tune & klib.TUNE_GENERIC_RHS3D)
    assert info['fuse_stage'] == (strip_ok and not tune & klib.TUNE_UNFUSED_STAGE), tag
    # every right-hand side
    worst = 0.0
    for i, (ref, scale) in enumerate(c.rhs_ref(kind)):
        assert np.isfinite(b[i]).all(), (tag, i)
        r = fields_within(b[i], ref, scale, c.F, TOL)
        worst = max(worst, r)
        assert r <= 1.0, ('b_%d' % i, tag, r)
    # epilogue scalars against longdouble sums over the downloaded vectors
    n = c.n
    norm_on = regime == 1 and c.path == klib.JP_STRIP2D and info['fuse_stage']
    for i in range(4):
        if not norm_on and not info['guess_on']:
            assert info['bnorm2'][i] == -1.0 and not info['dots_done'][i], (tag, i, info)
        if not norm_on:
            assert not info['dots_done'][i]
        if info['bnorm2'][i] != -1.0:
            s, sa = dot_ld(b[i], b[i])
            assert abs(LD(info['bnorm2'][i]) - s) <= n * EPS * sa, ('bnorm2', tag, i, float(abs(LD(info['bnorm2'][i]) - s) / sa))
        if info['guess_on']:
            for j in range(max(0, i - 2), i + 1):
                s, sa = dot_ld(b[i], b[j])
                assert abs(LD(info['gb'][i][j]) - s) <= n * EPS * sa, ('gb', tag, i, j, float(abs(LD(info['gb'][i][j]) - s) / sa))
                assert info['gb'][j][i] == info['gb'][i][j]
            assert info['dots_done'][i] == (norm_on and i > 0 and not tune & klib.TUNE_OWN_DOTS), (tag, i)
            assert info['bnorm2'][i] == info['gb'][i][i]
            check_guess(info, i, tag)
    if norm_on:
        assert all(x >= 0.0 for x in info['bnorm2']), (tag, info['bnorm2'])
    # the books
    want, arms = expected_books(c, tune, info)
    for cls, w in want.items():
        got = prof[cls]
        if cls == 'lincomb':
            assert got['launches'] == w, (cls, tag, got, w)
        else:
            assert got['launches'] == w[0] and abs(got['bytes'] - w[1]) <= 1e-9 * max(w[1], 1.0), (cls, tag, got, w)
    ndot = sum(1 for i in range(4) if info['guess_on'] and not info['dots_done'][i] and not (i == 0 and norm_on))
    assert prof['multidot']['launches'] == ndot, (tag, prof['multidot'], ndot)
    if ndot and any(not info['dots_done'][i] for i in range(1, 4)):
        arms.add('dots-own-pass')
    if say:
        say('stage_ops RHS %-10s %-5s regime %d tune %#9x yseg %s: seg %d x %d strips %d  worst b %.3f of the bound  arms %s'
            % (c.name, kind, regime, tune, yseg, info['seg'], info['nseg'], info['nstrips'], worst, ','.join(sorted(arms))))
    return info, b, arms


def check_guess(info, i, tag):
    """the guess coefficients against the Gram matrix the entry returned (ksfd_ctl::stage_guess: least squares on the regularised Gram
    system, taken when the predicted residual ||b_i - sum c_j b_j||^2 is below 0.09 ||b_i||^2).  The right-hand sides of a step are
    nearly dependent, so the coefficients are compared by the residual they predict, not one by one"""
    got = info['guess_c'][i]
    if i == 0:
        assert info['guess_n'][0] == 0 and not got.any()
        return
    j0 = max(0, i - 2)
    G, g, gii = info['gb'][j0:i, j0:i].astype(LD), info['gb'][i, j0:i].astype(LD), LD(info['gb'][i][i])
    pred = lambda cf: gii - 2 * (cf @ g) + cf @ G @ cf
    try:
        best = pred(np.linalg.solve(info['gb'][j0:i, j0:i] * (1.0 + 1e-13 * np.eye(i - j0)), info['gb'][i, j0:i]).astype(LD))
    except np.linalg.LinAlgError:
        best = None
    assert not got[:j0].any() and not got[i:].any(), (tag, i, got)
    assert info['guess_n'][i] == np.count_nonzero(got)
    if info['guess_n'][i]:
        mine = pred(got[j0:i].astype(LD))
        assert mine < 0.09 * gii * (1 + 1e-9), (tag, i, float(mine / gii))
        assert best is None or mine <= best + 1e-9 * gii, (tag, i, float(mine / gii), float(best / gii))
    else:
        assert best is None or not best < 0.08 * gii, (tag, i, float(best / gii))


def rhs_variants(c):
    v = [0, klib.TUNE_NO_RHS_CARRY, klib.TUNE_NO_GPLANE, klib.TUNE_UNFUSED_STAGE, klib.TUNE_OWN_DOTS]
    return v + ([klib.TUNE_GENERIC_RHS3D] if c.dim == 3 else [])


def test_four_by_four_is_refused_at_create():
    """jvp_path would give a 4 x 4 grid to the strip kernel, but no handle has one: the width-2 periodic star needs five points per axis.
    (6, 5) is the smallest grid the strip kernels see"""
    with pytest.raises(klib.KSFDError) as e:
        klib.KSFDHip(make_cfg((4, 4), 1))
    assert e.value.code == klib.EINVAL
    assert case('6x5').rhs_geometry() == dict(seg=2, nseg=3, nstrips=1, rows=0)


# ---- 1. the stage right-hand sides -----------------------------------------------------------------------------------------------------------
ALL_ARMS = {}


@pytest.mark.parametrize('name', SMALL)
def test_stage_rhs_every_variant(name):
    c = case(name)
    seen = set()
    by_variant = {}
    for tune in rhs_variants(c):
        for regime in (0, 1, 2):
            for kind in (('clean', 'dirty') if tune == 0 else ('clean',)):
                info, b, arms = check_rhs(c, kind, regime, tune, say=print)
                seen |= arms
                by_variant[(tune, regime, kind)] = (info, b)
    # epilogue and own-pass inner products: the same numbers within the summation bound, of the same right-hand sides
    a, b = by_variant[(0, 1, 'clean')], by_variant[(klib.TUNE_OWN_DOTS, 1, 'clean')]
    assert np.array_equal(a[1], b[1])
    if a[0]['guess_on'] and c.path == klib.JP_STRIP2D:
        assert any(a[0]['dots_done']) and not any(b[0]['dots_done'])
        for i in range(4):
            for j in range(max(0, i - 2), i + 1):
                sa = dot_ld(a[1][i], a[1][j])[1]
                assert abs(a[0]['gb'][i][j] - b[0]['gb'][i][j]) <= 2 * c.n * EPS * sa, (i, j)
    # the variants never change what is computed beyond rounding; GPLANE may differ in the last bit of G (ksfd_hip.h, KSFD_TUNE_NO_GPLANE)
    for tune in (klib.TUNE_NO_RHS_CARRY, klib.TUNE_UNFUSED_STAGE):
        assert np.array_equal(by_variant[(tune, 0, 'clean')][1][0], by_variant[(0, 0, 'clean')][1][0])
    ALL_ARMS[name] = seen
    want = {klib.JP_STRIP2D: {'gplane', 'carry', 'plain', 'yout', 'unfused2d'}, klib.JP_LDS3D: {'strip3d', 'strip3d-comb', 'generic'},
            klib.JP_STRIP3D: {'strip3d', 'strip3d-comb', 'generic'}, klib.JP_GENERIC: {'generic'}}[c.path]
    if c.nlig > 4:
        want = {'generic'}
    if c.path == klib.JP_STRIP2D and by_variant[(0, 1, 'clean')][0]['guess_on']:
        want |= {'dots-epilogue', 'dots-own-pass'}
    assert seen >= want, (name, seen, want)


def test_stage_rhs_arms_all_seen():
    """the shapes together reach every arm, the split partials of the halo-overlap launches included"""
    for name in ('64x48', 'ring-36x20', 'ring-64x8', 'ring-64x48', '16x16x12', '37x21'):
        if name not in ALL_ARMS:
            test_stage_rhs_every_variant(name)
    seen = set().union(*ALL_ARMS.values())
    assert seen >= {'gplane', 'carry', 'plain', 'yout', 'unfused2d', 'dots-epilogue', 'dots-own-pass', 'strip3d', 'strip3d-comb', 'generic'}
    for name, guess in (('ring-36x20', None), ('ring-64x48', True)):
        c = case(name)
        c.use('clean')
        c.k.set_tuning(use_fused=klib.TUNE_FUSED)
        info = c.k.stage_rhs(1, HSTEP, c.Y[:3])[1]
        assert info['overlap'] and info['nseg'] >= 3 and all(x >= 0 for x in info['bnorm2'])
        if guess:
            assert info['guess_on'] and all(info['dots_done'][1:])
    # one launch on a ring: with the overlap switched off (TUNE_NO_OVERLAP); with fewer than 3 segments in the long-segment child
    c = case('ring-64x8')
    info = check_rhs(c, 'clean', 1, 0)[0]
    assert info['overlap'] and info['nseg'] == 4
    info = check_rhs(c, 'clean', 1, klib.TUNE_NO_OVERLAP)[0]
    assert not info['overlap'] and all(x >= 0 for x in info['bnorm2'])
    assert case('8x5').rhs_geometry() == dict(seg=2, nseg=3, nstrips=1, rows=0)
    assert case('126x8').rhs_geometry()['nstrips'] == 2 and case('250x9').rhs_geometry()['nstrips'] == 3


def test_stage_guess_from_coherent_stage_vectors():
    """stage vectors that are small multiples of f(u), as a step's are to first order: the right-hand sides are nearly dependent, the
    guess is taken in the spectral and in the multigrid regime, and its coefficients reach the least-squares residual of the Gram system"""
    cfg = make_cfg((64, 48), 2)
    u = _state(cfg, 3, amp=0.05)
    n = cfg.F * cfg.N
    f = ko.Oracle(cfg).rhs(u)
    rng = np.random.default_rng(5)
    Y = np.stack([t * f * (1.0 + 1e-3 * rng.standard_normal(n)) for t in (2e-5, 3e-5, 1e-5)])
    k = klib.KSFDHip(cfg)
    k.set_state(u)
    try:
        for regime in (1, 2):
            b, info, _ = k.stage_rhs(regime, HSTEP, Y)
            assert info['guess_on'] and all(info['guess_n'][i] >= 1 for i in (1, 2, 3)), info
            for i in range(4):
                check_guess(info, i, ('coherent', regime))
                for j in range(max(0, i - 2), i + 1):
                    s, sa = dot_ld(b[i], b[j])
                    assert abs(LD(info['gb'][i][j]) - s) <= n * EPS * sa
    finally:
        k.close()


# ---- 2. the completion -----------------------------------------------------------------------------------------------------------------------
def check_finish(c, tune=0, atol=0.01, rtol=1e-6):
    """state with a negative value (no NaN: the norm must be a number), stage vectors that push two points under their floor"""
    u = c.clean.copy()
    u[c.n - 1 - c.N // 5] = -3.0
    c.k.set_state(u)
    c.state = None
    c.k.set_tuning(use_fused=klib.TUNE_FUSED | tune)
    Y = c.Yd
    b, info, (unew, err) = c.k.stage_rhs(0, HSTEP, Y, finish=(atol, rtol))
    terms_u = np.abs(u).astype(LD)
    ref_u, ref_e, terms_e = u.astype(LD), np.zeros(c.n, dtype=LD), np.zeros(c.n, dtype=LD)
    for j in range(4):
        ref_u = ref_u + LD(BT[j]) * Y[j]
        terms_u = terms_u + abs(LD(BT[j])) * np.abs(Y[j])
        ej = np.float64(B2T[j] - BT[j])
        ref_e = ref_e + LD(ej) * Y[j]
        terms_e = terms_e + abs(LD(ej)) * np.abs(Y[j])
    assert np.all(np.abs(unew.astype(LD) - ref_u) <= 1e-14 * terms_u), float((np.abs(unew - ref_u) / terms_u).max())
    assert np.all(np.abs(err.astype(LD) - ref_e) <= 1e-14 * terms_e), float((np.abs(err - ref_e) / terms_e).max())
    # ... and in the plain relative form wherever the five terms do not cancel by more than a factor of four (1e-14 |result| is then
    # still >= 2.5e-15 sum|terms|, above the 5 eps/2 a sum of five terms can lose); most elements of both vectors
    for got, ref, terms in ((unew, ref_u, terms_u), (err, ref_e, terms_e)):
        plain = terms <= 4 * np.abs(ref)
        assert np.count_nonzero(plain) > c.n // 4
        assert np.all(np.abs(got.astype(LD) - ref)[plain] <= 1e-14 * np.abs(ref)[plain])
    q = (ref_e / (LD(atol) + LD(rtol) * np.maximum(np.abs(ref_u), np.abs(ref_u + ref_e)))) ** 2
    got = LD(info['wrms']) ** 2 * c.n
    assert abs(got - q.sum()) <= (c.n + 8) * EPS * q.sum(), float(abs(got - q.sum()) / q.sum())
    assert abs(info['wrms'] - ko.wrms(unew, err, atol, rtol)) <= 1e-12 * info['wrms']
    lo = np.concatenate([np.full(c.N, c.cfg.rhomin)] + [np.full(c.N, c.cfg.Umin)] * c.nlig)
    below = int(np.count_nonzero(~(ref_u.astype(np.float64) >= lo)))
    assert below >= 2 and info['below'] == below, (info['below'], below)
    # the state is as it was, and the error vector of the entry's own completion is not handed out as a step's
    assert np.array_equal(c.k.get_state(), u, equal_nan=True)
    with pytest.raises(klib.KSFDError) as e:
        c.k.last_error_vector()
    assert e.value.code == klib.EINVAL
    return info


@pytest.mark.parametrize('name', ['8x5', '250x9', '24x20', '96', '16x10x9', 'ring-36x20'])
def test_completion_norm_and_count(name):
    c = case(name)
    check_finish(c)
    check_finish(c, tune=klib.TUNE_OLD_BOUNDARY)                          # the old step boundary: the completion stores the error vector itself


# ---- 3. the frozen action ---------------------------------------------------------------------------------------------------------------------
def check_action(c, kind, yseg=None, tune=0, say=None):
    c.use(kind)
    k = c.k
    k.set_tuning(use_fused=klib.TUNE_FUSED | tune, **({} if yseg is None else dict(yseg=yseg)))
    F = c.F
    geo = c.jvp_geometry(yseg or YSEG_JVP)
    y = np.random.default_rng(23).standard_normal(c.n)
    y[0], y[-1] = y[0] + 25.0, y[-1] - 25.0
    alpha, beta = 0.75, -1.0 / 3.0
    worst = 0.0
    for what, v in c.vectors(29):
        Av = c.A(kind, v, S_A).reshape(-1)
        vl, yl = v.astype(LD), y.astype(LD)
        refs = {0: LD(S_A) * vl - Av, 1: Av, 2: yl - Av, 3: LD(alpha) * yl + LD(beta) * Av, 4: LD(alpha) * vl + LD(beta) * Av}
        for mode, ref in refs.items():
            got, sc = k.stage_jvp(klib.SJ_ACTION, v, y if mode in (2, 3) else None, mode=mode, shift=S_A, alpha=alpha, beta=beta)
            assert sc['path'] == c.path and {q: sc[q] for q in geo} == geo, (c.name, sc, geo)
            assert sc['overlap'] == (c.ring and c.path == klib.JP_STRIP2D and geo['nseg'] >= 3)
            d = per_field(got, ref, F)
            worst = max(worst, d)
            assert d < TOL_OP, ('action', c.name, kind, what, mode, d)
        if what != 'random':
            # two shifts: the difference is the shift on the diagonal and nothing else
            g0 = k.stage_jvp(klib.SJ_ACTION, v, mode=1, shift=S_A)[0]
            g1 = k.stage_jvp(klib.SJ_ACTION, v, mode=1, shift=S_B)[0]
            D = g0 - g1
            j = int(np.flatnonzero(v)[0])
            d = D[j]
            D[j] = 0.0
            assert not D.any(), ('two shifts', c.name, what)
            hu = lambda a: 0.5 * np.spacing(abs(a))
            assert abs(d - (S_A - S_B)) <= hu(g0[j]) + hu(g1[j]) + hu(d)
    if say:
        say('stage_ops action %-10s %-5s yseg %s: seg %d x %d  worst rel-L2 %.2e' % (c.name, kind, yseg, geo['seg'], geo['nseg'], worst))


@pytest.mark.parametrize('name', SMALL)
def test_action_modes(name):
    c = case(name)
    check_action(c, 'clean', say=print)
    check_action(c, 'dirty', say=print)


def check_residual(c, kind, yseg=None, say=None):
    c.use(kind)
    k = c.k
    k.set_tuning(use_fused=klib.TUNE_FUSED, **({} if yseg is None else dict(yseg=yseg)))
    b = np.random.default_rng(31).standard_normal(c.n) * 50.0
    for what, x in c.vectors(37):
        Ax = c.A(kind, x, S_A).reshape(-1)
        ref = b.astype(LD) - Ax
        got, sc = k.stage_jvp(klib.SJ_RESIDUAL32, x, b, shift=S_A)
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))        # fp32 values
        rf, gf, bf, af = (a.reshape(c.F, -1) for a in (ref, got, np.abs(b), np.abs(Ax)))
        for f in range(c.F):
            scale = bf[f].max() + af[f].max()
            assert np.all(np.abs(gf[f].astype(LD) - rf[f]) <= LD(2.0) ** -24 * np.abs(rf[f]) + TOL_OP * scale), ('residual32', c.name, what, f)
        # ||r||^2 sums the unrounded fp64 values: the fp64 residual of the same launch mode gives them
        r64 = k.stage_jvp(klib.SJ_ACTION, x, b, mode=2, shift=S_A)[0]
        s, sa = dot_ld(r64, r64)
        assert abs(LD(sc['norm2']) - s) <= c.n * EPS * sa, ('norm2', c.name, what, float(abs(LD(sc['norm2']) - s) / sa))
        s_ref = (ref * ref).sum()
        dn = TOL_OP * np.sqrt(LD(c.n)) * (np.abs(b).max() + np.abs(Ax).max())      # norm of the fp64 tolerance over all elements
        assert abs(LD(sc['norm2']) - s_ref) <= c.n * EPS * s_ref + 2.0 * np.sqrt(s_ref) * dn + dn * dn
        s32 = dot_ld(got, got)[0]
        if say:
            say('stage_ops residual32 %-10s %-5s %-13s yseg %s: norm2 off the fp64 sum by %.2e, off the sum of the rounded values by %.2e (bound %.2e)'
                % (c.name, kind, what, yseg, float(abs(LD(sc['norm2']) - s) / sa), float(abs(LD(sc['norm2']) - s32) / sa), c.n * EPS))


@pytest.mark.parametrize('name', [n for n in SMALL if CASES[n][3] != klib.JP_GENERIC])
def test_residual32(name):
    c = case(name)
    check_residual(c, 'clean', say=print)
    check_residual(c, 'dirty')


@pytest.mark.parametrize('name', [n for n in SMALL if CASES[n][3] == klib.JP_GENERIC])
def test_residual32_refused_without_a_strip_kernel(name):
    c = case(name)
    c.use('clean')
    c.k.set_tuning(use_fused=klib.TUNE_FUSED)
    v = np.ones(c.n)
    with pytest.raises(klib.KSFDError) as e:
        c.k.stage_jvp(klib.SJ_RESIDUAL32, v, v, shift=S_A)
    assert e.value.code == klib.EINVAL


# ---- 4. the polynomial ----------------------------------------------------------------------------------------------------------------------
def horner(c, kind, v, coef, shift, fp32_planes=False, store=None):
    """sum_i coef[i] (A/shift)^i v the way poly_apply runs it: t = coef[d-1] v + coef[d]/shift A v, then t <- coef[i] v + A t / shift"""
    d = len(coef) - 1
    vl = v.astype(LD)
    st = store or (lambda a: a)
    t = LD(coef[d - 1]) * vl + LD(coef[d] / shift) * c.A(kind, v.astype(LD), shift, fp32_planes).reshape(-1)
    for i in range(d - 2, -1, -1):
        t = st(t)
        t = LD(coef[i]) * vl + LD(1.0 / shift) * c.A(kind, t, shift, fp32_planes).reshape(-1)
    return t


def check_poly(c, kind, fp32, yseg=None, say=None):
    c.use(kind)
    k = c.k
    k.set_tuning(use_fused=klib.TUNE_FUSED | (0 if fp32 else klib.TUNE_POLY_FP64), **({} if yseg is None else dict(yseg=yseg)))
    rng = np.random.default_rng(41)
    v = c.vectors(43)[0][1]
    for deg in (1, 2, 3, 7):
        coef = rng.uniform(0.3, 1.0, deg + 1) * (-1.0) ** np.arange(deg + 1)
        got, sc = k.stage_jvp(klib.SJ_POLY, v, shift=S_A, coef=coef)
        assert sc['fp32'] == fp32, (c.name, sc)
        if not fp32:
            d = per_field(got, horner(c, kind, v, coef, S_A), c.F)
            assert d < TOL_OP * (deg + 1), ('poly fp64', c.name, deg, d)
            line = 'fp64 rel-L2 %.2e' % d
        else:
            ref = horner(c, kind, v, coef, S_A, fp32_planes=True)
            d32 = mr.rel_l2(horner(c, kind, v, coef, S_A, fp32_planes=True, store=mr.store_f32), ref)
            d = mr.rel_l2(got, ref)
            bound = max(4 * d32, TOL_OP * (deg + 1))
            assert d32 < 1e-5 and d <= bound, ('poly fp32', c.name, deg, d, d32)
            line = 'fp32 d32 %.3e distance %.3e head-room %.2f' % (d32, d, bound / max(d, 1e-300))
        if say:
            say('stage_ops poly %-10s %-5s yseg %s degree %d: %s' % (c.name, kind, yseg, deg, line))


@pytest.mark.parametrize('name', SMALL)
def test_polynomial_fp64(name):
    check_poly(case(name), 'clean', False, say=print)


@pytest.mark.parametrize('name', WITH_PLANES)
def test_polynomial_fp32(name):
    c = case(name)
    assert c.planes('clean')[1] is not None
    check_poly(c, 'clean', True, say=print)
    check_poly(c, 'dirty', True)


def test_polynomial_steps_are_unchanged_by_the_polynomial_entry():
    """polynomial-preconditioned steps with the entry called between them equal those of a handle that never saw it: iterations, launches,
    states bit for bit -- the eigenvalue estimate and its schedule (StepMemo), the planes and their fp32 copy are undisturbed.  It does
    NOT show that poly_deg / poly_alpha are put back: every step sets the polynomial up again (step_begins) before it is read, so
    no entry of the library can observe them between steps; that part of the entry is four lines to read (ksfd_stage_jvp, op 2)"""
    cfg = make_cfg((64, 64), 1)
    u = _state(cfg, 3, amp=0.01)
    out = []
    for touch in (False, True):
        k = klib.KSFDHip(cfg)
        k.set_state(u)
        opts = klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6, pc_type=3)
        t, h, res = 0.0, 0.05, []
        for s in range(3):
            if touch and s > 0:
                k.stage_jvp(klib.SJ_POLY, np.ones(cfg.F * cfg.N), shift=2.0, coef=[1.0, -0.5, 0.25])
            t, h, st, rc = k.step(t, h, opts)
            res.append((t, h, st.linear_its, st.pc_used, st.launches, k.get_state()))
        out.append(res)
        k.close()
    for a, b in zip(*out):
        assert a[3] & klib.PC_POLYNOMIAL
        assert a[:5] == b[:5] and np.array_equal(a[5], b[5])


# ---- 5. long segments -------------------------------------------------------------------------------------------------------------------------
def run_long_2d():
    """in a child with KSFD_WAVES_RHS = KSFD_WAVES_JVP = 1: the handle's yseg is the segment length"""
    for name in ('130x37', '130x40', 'ring-130x40'):
        c = Case(name, waves=(1, 1))
        for yseg in (5, 32):
            geo = strips(c.shape[0], c.shape[1], yseg, 1)
            assert geo['seg'] == yseg and geo['nstrips'] == 2
            if c.ring:
                # 8 segments: interior + boundary launches with split partials; 2 segments: the single launch of a ring
                for regime in (1, 2):
                    info = check_rhs(c, 'clean', regime, 0, yseg=yseg, say=print)[0]
                    assert info['overlap'] == (yseg == 5) and info['guess_on']
                check_action(c, 'clean', yseg=yseg, say=print)
                check_residual(c, 'clean', yseg=yseg, say=print)
                check_poly(c, 'clean', True, yseg=yseg, say=print)
                continue
            seen = set()
            for tune in rhs_variants(c):
                for regime in (0, 1, 2):
                    seen |= check_rhs(c, 'clean', regime, tune, yseg=yseg, say=print)[2]
            check_rhs(c, 'dirty', 1, 0, yseg=yseg, say=print)
            assert seen >= {'gplane', 'carry', 'plain', 'yout', 'unfused2d'}
            if name == '130x40':
                assert seen >= {'dots-epilogue', 'dots-own-pass'}
            check_action(c, 'clean', yseg=yseg, say=print)
            check_residual(c, 'clean', yseg=yseg, say=print)
            check_poly(c, 'clean', False, yseg=yseg, say=print)
            if name == '130x40':
                check_poly(c, 'clean', True, yseg=yseg, say=print)
        c.k.close()


def test_long_segments_2d_in_a_fresh_process():
    """KSFD_WAVES_RHS / KSFD_WAVES_JVP are read once per process: a fresh child with both at 1 runs (130,37) x 2 (the RHS stage modes, action
    modes 0-4, the residual, the fp64 polynomial) and (130,40) x 2 (the same with stored right-hand sides, so the inner products of the
    epilogue, and the fp32 polynomial; once more as a ring of one rank) at segments of 5 and of 32 rows: prefetch, window shift and ring
    wrap in their steady state"""
    env = dict(os.environ, KSFD_WAVES_RHS='1', KSFD_WAVES_JVP='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'long2d'], env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'long2d done' in r.stdout


@pytest.mark.parametrize('name', ['8x64x512', '8x60x512'])
def test_long_segments_3d(name):
    """k3d_for leaves segments of >= 4 planes on these shapes: the z march in its steady state, in the RHS and in every action mode"""
    c = Case(name)
    try:
        assert c.jvp_geometry()['seg'] >= 4 and c.rhs_geometry()['seg'] >= 4
        for tune in (0, klib.TUNE_UNFUSED_STAGE):
            check_rhs(c, 'clean', 0, tune, say=print)
        check_rhs(c, 'dirty', 2, 0, say=print)
        check_action(c, 'clean', say=print)
        check_residual(c, 'clean', say=print)
    finally:
        c.k.close()


# ---- 6. refusals and hygiene -------------------------------------------------------------------------------------------------------------------
def _three_steps(k, pc_type, h0):
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, pc_type=pc_type)
    t, h, out = 0.0, h0, []
    for _ in range(3):
        t, h, st, rc = k.step(t, h, opts)
        out.append((t, h, st.linear_its, st.rejections, st.pc_used, st.launches, k.get_state()))
    return out


HYGIENE = {'2-D spectral': ((64, 64), 1, 4, 0.05, klib.PC_SPECTRAL), '2-D multigrid': ((64, 48), 2, 1, 5.0, klib.PC_MULTIGRID),
           '3-D': ((16, 16, 16), 1, 2, 0.05, 0)}


def _mixed_calls(k, n, rng):
    Y = 30.0 * rng.standard_normal((4, n))
    v, y = rng.standard_normal(n), rng.standard_normal(n)
    for regime in (0, 1, 2):
        k.stage_rhs(regime, HSTEP, Y[:3])
    k.stage_rhs(1, 0.3, Y, finish=(0.01, 1e-6))
    for mode in range(5):
        k.stage_jvp(klib.SJ_ACTION, v, y, mode=mode, shift=S_A, alpha=0.5, beta=2.0)
    k.stage_jvp(klib.SJ_RESIDUAL32, v, y, shift=S_B)
    k.stage_jvp(klib.SJ_POLY, v, shift=S_A, coef=[1.0, -0.5, 0.25, 0.1])


def _refused(k, n):
    """every bad argument: KSFD_EINVAL"""
    Y, v = np.zeros((4, n)), np.ones(n)
    bad = [lambda: k.stage_rhs(0, HSTEP, Y[:3], nstages=5), lambda: k.stage_rhs(0, HSTEP, None, nstages=0), lambda: k.stage_rhs(3, HSTEP, Y[:3]),
           lambda: k.stage_rhs(0, 0.0, Y[:3]), lambda: k.stage_rhs(0, HSTEP, None, nstages=4), lambda: k.stage_rhs(0, HSTEP, Y, nstages=3, finish=(0.01, 1e-6)),
           lambda: k.stage_rhs(0, HSTEP, Y, finish=(0.0, 0.0)),
           lambda: k.stage_jvp(klib.SJ_ACTION, v, mode=5), lambda: k.stage_jvp(klib.SJ_ACTION, v, mode=-1), lambda: k.stage_jvp(klib.SJ_ACTION, v, mode=2),
           lambda: k.stage_jvp(klib.SJ_ACTION, v, v, mode=3, shift=np.inf), lambda: k.stage_jvp(3, v), lambda: k.stage_jvp(klib.SJ_RESIDUAL32, v),
           lambda: k.stage_jvp(klib.SJ_POLY, v, coef=[1.0]), lambda: k.stage_jvp(klib.SJ_POLY, v, coef=np.ones(9)), lambda: k.stage_jvp(klib.SJ_POLY, v)]
    for i, call in enumerate(bad):
        with pytest.raises(klib.KSFDError) as e:
            call()
        assert e.value.code == klib.EINVAL, i


@pytest.mark.parametrize('what', list(HYGIENE))
def test_steps_after_the_entries_equal_steps_on_a_fresh_handle(what):
    """a mix of calls to both entries, refused ones included, before the first step and between the steps: three adaptive steps are bit for
    bit those of a handle that never saw the entries -- states, step sizes, iterations and launches"""
    shape, nlig, pc_type, h0, pc_bit = HYGIENE[what]
    cfg = make_cfg(shape, nlig)
    u = _state(cfg, 3, amp=0.05)
    n = cfg.F * cfg.N
    out = []
    for touch in (False, True):
        k = klib.KSFDHip(cfg)
        k.set_state(u)
        if touch:
            _refused(k, n)
            _mixed_calls(k, n, np.random.default_rng(1))
            assert np.array_equal(k.get_state(), u)
            with pytest.raises(klib.KSFDError):
                k.last_error_vector()
        opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, pc_type=pc_type)
        t, h, res = 0.0, h0, []
        for s in range(3):
            t, h, st, rc = k.step(t, h, opts)
            res.append((t, h, st.linear_its, st.rejections, st.pc_used, st.launches, k.get_state()))
            if touch and s < 2:
                before = k.get_state()
                _mixed_calls(k, n, np.random.default_rng(2 + s))
                _refused(k, n)
                assert np.array_equal(k.get_state(), before)
        out.append(res)
        k.close()
    for a, b in zip(*out):
        assert pc_bit == 0 or a[4] & pc_bit
        assert a[:6] == b[:6] and np.array_equal(a[6], b[6])


def test_error_vector_of_a_step_survives_the_stages_alone_but_not_the_completion():
    """as after a step that completed no attempt: stages without a completion leave a vector that was already formed, the entry's own
    completion overwrites its buffer and nothing is handed out"""
    cfg = make_cfg((64, 48), 1)
    k = klib.KSFDHip(cfg)
    k.set_state(_state(cfg, 3, amp=0.05))
    n = cfg.F * cfg.N
    Y = np.random.default_rng(3).standard_normal((4, n))
    k.step(0.0, 0.05, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6))
    k.stage_rhs(0, HSTEP, Y[:3])                          # the pending vector lived in Y
    with pytest.raises(klib.KSFDError):
        k.last_error_vector()
    k.step(0.05, 0.05, klib.default_step_opts(adapt=0, atol=0.01, rtol=1e-6))
    e = k.last_error_vector()                             # formed: in its own buffer
    k.stage_rhs(0, HSTEP, Y[:3])
    assert np.array_equal(k.last_error_vector(), e)
    k.stage_rhs(0, HSTEP, Y, finish=(0.01, 1e-6))
    with pytest.raises(klib.KSFDError):
        k.last_error_vector()
    k.close()


if __name__ == '__main__':
    if sys.argv[1:] == ['long2d']:
        run_long_2d()
        print('long2d done')
