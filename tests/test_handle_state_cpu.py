"""CPU: the handle's record of what is current (ksfd_amd/csrc/handle_state.h) on its own.  The header is plain C++ without device code
and without the handle -- that the small driver below compiles with the host compiler alone, warnings as errors, is the proof -- so the
driver replays scripts of the very events the library calls and prints the whole record after each one.
(a) every event alone, from a record with everything current, against the table of what it ends written out by hand below;
(b) seeded random sequences of events and setters against a model that keeps true generation numbers of the state, the parameters and
    every product, and remembers what each product was built from: whatever the record reports current was built from inputs that are
    all current in the model;
(c) the same driver built with the address and undefined-behaviour sanitizers, as a stand-alone program, over the scripts of (a)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

DRIVER = r'''
#include "handle_state.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
using namespace ksfd_ctl;
static FILE *f;
static double rd() { double v; if (fscanf(f, "%lf", &v) != 1) exit(3); return v; }
static const void *key(double id) { return (const void *)(uintptr_t)(long long)id; }
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    f = fopen(argv[1], "r");
    if (!f) return 2;
    const int n = (int)rd();
    Current c;
    for (int r = 0; r < n; r++) {
        const int op = (int)rd();
        const double a = rd(), b = rd(), d = rd();
        int q = -1;
        switch (op) {
        case 0:                                  /* the test's own start: everything current, set-up / graph / polynomial at shift a */
            c = Current();
            c.coef_fresh = c.coef32_fresh = c.floor_ok = c.ckpt_floor_ok = c.means_valid = c.mg_coef_valid = c.mgc_ready = true;
            c.mg_shift = c.mg_graph_shift = c.poly_shift = a; c.mg_graph_x = key(1); c.mg_graph_f32 = false;
            c.dr_valid = true; for (bool &v : c.rec_valid) v = true; c.rec_vtop = 5; c.rec_ztop = 3;
            c.have_err = c.err_pending = true;
            break;
        case 1: state_written(c, a != 0); break;
        case 2: state_handed_out(c); break;
        case 3: state_groomed(c); break;
        case 4: params_changed(c); break;
        case 5: planes_recomputed(c, a != 0, b != 0); break;
        case 6: coef32_made(c); break;
        case 7: means_computed(c); break;
        case 8: coarse_planes_restricted(c); break;
        case 9: shift_setup_done(c, a); break;
        case 10: coarse_factors_ready(c); break;
        case 11: coarse_factors_ended(c); break;
        case 12: graph_captured(c, a, key(b), d != 0); break;
        case 13: vcycle_config_changed(c); break;
        case 14: hierarchy_freed(c); break;
        case 15: hierarchy_borrowed(c); break;
        case 16: poly_set_up(c, a); break;
        case 17: poly_config_changed(c); break;
        case 18: krylov_basis_overwritten(c, a != 0); break;
        case 19: recycled_spaces_dropped(c); break;
        case 20: recycled_space_kept(c, (int)a, (int)b, (int)d); break;
        case 21: dr_relation_kept(c); break;
        case 22: step_begins(c); break;
        case 23: attempt_begins(c); break;
        case 24: completion_done(c, a != 0); break;
        case 25: error_vector_formed(c); break;
        case 26: checkpoint_saved(c); break;
        case 27: checkpoint_restored(c); break;
        case 28: q = graph_current(c, a, key(b), d != 0) ? 1 : 0; break;
        case 29: c = Current(); break;           /* a new handle */
        case 30: stage_vectors_borrowed(c, a != 0); break;
        case 31: { Current was; was.coef_fresh = ((int)a & 1) != 0; was.coef32_fresh = ((int)a & 2) != 0; was.means_valid = ((int)a & 4) != 0;
                   derived_given_back(c, was); } break;
        default: return 4;
        }
        printf("%d %d %d %d %d %d %.17g %d %.17g %lld %d %.17g %d %d %d %d %d %d %d %d %d %d\n", c.coef_fresh, c.coef32_fresh, c.floor_ok, c.ckpt_floor_ok,
               c.means_valid, c.mg_coef_valid, c.mg_shift, c.mgc_ready, c.mg_graph_shift, (long long)(uintptr_t)c.mg_graph_x, c.mg_graph_f32,
               c.poly_shift, c.dr_valid, c.rec_valid[0], c.rec_valid[1], c.rec_valid[2], c.rec_valid[3], c.rec_vtop, c.rec_ztop, c.have_err, c.err_pending, q);
    }
    return 0;
}
'''

FIELDS = ('coef_fresh', 'coef32_fresh', 'floor_ok', 'ckpt_floor_ok', 'means_valid', 'mg_coef_valid', 'mg_shift', 'mgc_ready', 'mg_graph_shift',
          'mg_graph_x', 'mg_graph_f32', 'poly_shift', 'dr_valid', 'rec0', 'rec1', 'rec2', 'rec3', 'rec_vtop', 'rec_ztop', 'have_err', 'err_pending', 'query')
(START, STATE_WRITTEN, STATE_HANDED_OUT, STATE_GROOMED, PARAMS_CHANGED, PLANES_RECOMPUTED, COEF32_MADE, MEANS_COMPUTED, COARSE_PLANES_RESTRICTED,
 SHIFT_SETUP_DONE, COARSE_FACTORS_READY, COARSE_FACTORS_ENDED, GRAPH_CAPTURED, VCYCLE_CONFIG_CHANGED, HIERARCHY_FREED, HIERARCHY_BORROWED, POLY_SET_UP,
 POLY_CONFIG_CHANGED, KRYLOV_BASIS_OVERWRITTEN, RECYCLED_SPACES_DROPPED, RECYCLED_SPACE_KEPT, DR_RELATION_KEPT, STEP_BEGINS, ATTEMPT_BEGINS,
 COMPLETION_DONE, ERROR_VECTOR_FORMED, CHECKPOINT_SAVED, CHECKPOINT_RESTORED, GRAPH_CURRENT, NEW_HANDLE, STAGE_VECTORS_BORROWED, DERIVED_GIVEN_BACK) = range(32)


def _cxx():
    # the host compiler, else the compiler the library itself is built with (the header is plain C++ either way)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('hipcc') or (hipcc if os.path.exists(hipcc) else None)
    if not cxx:
        pytest.fail('no C++ compiler found (g++, c++, hipcc): the library cannot have been built either')
    return cxx


def _build(d, name, extra):
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / name
    subprocess.run([_cxx(), '-x', 'c++', '-O1', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + extra +
                   ['-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(rows, tag='script'):
        inp = d / (name + '_' + tag + '.txt')
        with open(inp, 'w') as f:
            f.write('%d\n' % len(rows))
            f.write('\n'.join(' '.join(repr(float(x)) for x in (list(row) + [0, 0, 0])[:4]) for row in rows) + '\n')
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = [dict(zip(FIELDS, (float(x) for x in line.split()))) for line in r.stdout.splitlines()]
        assert len(out) == len(rows)
        return out
    return run


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('handle_state'), 'drv', [])


# ---- (a) every event alone ----------------------------------------------------------------------------------------------------------
S0 = 2.5                                  # the shift everything is set up for at the start
ALL_CURRENT = dict(coef_fresh=1, coef32_fresh=1, floor_ok=1, ckpt_floor_ok=1, means_valid=1, mg_coef_valid=1, mg_shift=S0, mgc_ready=1, mg_graph_shift=S0,
                   mg_graph_x=1, mg_graph_f32=0, poly_shift=S0, dr_valid=1, rec0=1, rec1=1, rec2=1, rec3=1, rec_vtop=5, rec_ztop=3, have_err=1,
                   err_pending=1, query=-1)
NO_REC = dict(rec0=0, rec1=0, rec2=0, rec3=0, rec_vtop=0, rec_ztop=0)
# event (with its arguments) -> what differs from ALL_CURRENT afterwards.  Written out by hand from the list of events in DESIGN.md, not derived from the header
TABLE = [
    ((STATE_WRITTEN, 0), dict(coef_fresh=0, floor_ok=0)),                       # set_state, set_state_random, scale_rho, mul_rho
    ((STATE_WRITTEN, 1), dict(coef_fresh=0)),                                   # accepted step that counted no value below its floor
    ((STATE_HANDED_OUT,), dict(floor_ok=0)),                                    # the planes deliberately stay
    ((STATE_GROOMED,), dict()),
    ((PARAMS_CHANGED,), dict(coef_fresh=0, floor_ok=0, ckpt_floor_ok=0)),
    ((PLANES_RECOMPUTED, 0, 0), dict(coef32_fresh=0, means_valid=0, mg_coef_valid=0, mg_shift=-1, mgc_ready=0)),
    ((PLANES_RECOMPUTED, 1, 0), dict(means_valid=0, mg_coef_valid=0, mg_shift=-1, mgc_ready=0)),
    ((PLANES_RECOMPUTED, 0, 1), dict(coef32_fresh=0, mg_coef_valid=0, mg_shift=-1, mgc_ready=0)),
    ((COEF32_MADE,), dict()),
    ((MEANS_COMPUTED,), dict()),
    ((COARSE_PLANES_RESTRICTED,), dict()),
    ((SHIFT_SETUP_DONE, 4.0), dict(mg_shift=4.0, mg_graph_shift=-1)),
    ((SHIFT_SETUP_DONE, S0), dict(mg_graph_shift=-1)),                          # the same shift again: new bounds all the same, the captured cycle ends
    ((COARSE_FACTORS_READY,), dict()),
    ((COARSE_FACTORS_ENDED,), dict(mgc_ready=0)),
    ((GRAPH_CAPTURED, 4.0, 7, 1), dict(mg_graph_shift=4.0, mg_graph_x=7, mg_graph_f32=1)),
    ((VCYCLE_CONFIG_CHANGED,), dict(mg_shift=-1, mgc_ready=0)),                 # the coarse planes stay
    ((HIERARCHY_FREED,), dict(mg_coef_valid=0, mg_shift=-1, mgc_ready=0, mg_graph_shift=-1)),
    ((HIERARCHY_BORROWED,), dict(mg_shift=-1, mgc_ready=0)),
    ((POLY_SET_UP, 4.0), dict(poly_shift=4.0)),
    ((POLY_CONFIG_CHANGED,), dict(poly_shift=-1)),
    ((KRYLOV_BASIS_OVERWRITTEN, 0), dict(dr_valid=0, **NO_REC)),
    ((KRYLOV_BASIS_OVERWRITTEN, 1), dict(dr_valid=0)),                          # gmres() building behind the spaces it keeps
    ((RECYCLED_SPACES_DROPPED,), dict(**NO_REC)),
    ((RECYCLED_SPACE_KEPT, 2, 9, 4), dict(rec_vtop=9, rec_ztop=4)),
    ((DR_RELATION_KEPT,), dict()),
    ((STEP_BEGINS,), dict(poly_shift=-1)),
    ((ATTEMPT_BEGINS,), dict(dr_valid=0, have_err=0, err_pending=0)),           # the pending error vector goes with Y
    ((COMPLETION_DONE, 0), dict()),
    ((COMPLETION_DONE, 1), dict(err_pending=0)),
    ((ERROR_VECTOR_FORMED,), dict(err_pending=0)),
    ((CHECKPOINT_SAVED,), dict()),
    ((CHECKPOINT_RESTORED,), dict(coef_fresh=0, have_err=0, err_pending=0)),    # floor_ok: the checkpoint's proof, true here
    ((STAGE_VECTORS_BORROWED, 0), dict(dr_valid=0, have_err=0, err_pending=0)), # ksfd_stage_rhs: as an attempt that begins
    ((STAGE_VECTORS_BORROWED, 1), dict(dr_valid=0, have_err=0, err_pending=0)), # ... with its own completion: no vector, stored or pending
    ((DERIVED_GIVEN_BACK, 7), dict()),                                          # ksfd_stage_rhs / ksfd_stage_jvp found everything current: it stays
    ((DERIVED_GIVEN_BACK, 6), dict(coef_fresh=0)),                              # ... found no planes: the ones it made are not the next step's
    ((DERIVED_GIVEN_BACK, 1), dict(coef32_fresh=0, means_valid=0)),
    ((GRAPH_CURRENT, S0, 1, 0), dict(query=1)),
    ((GRAPH_CURRENT, 4.0, 1, 0), dict(query=0)),
    ((GRAPH_CURRENT, S0, 2, 0), dict(query=0)),
    ((GRAPH_CURRENT, S0, 1, 1), dict(query=0)),
]


def _table_rows():
    rows = []
    for ev, _ in TABLE:
        rows += [(START, S0), ev]
    return rows


def _check_table(out):
    assert {ev[0] for ev, _ in TABLE} == set(range(1, 29)) | {STAGE_VECTORS_BORROWED, DERIVED_GIVEN_BACK}, 'an event has no row in the table'
    for k, (ev, diff) in enumerate(TABLE):
        assert out[2 * k] == ALL_CURRENT, ev
        assert out[2 * k + 1] == {**ALL_CURRENT, **diff}, (ev, {f: v for f, v in out[2 * k + 1].items() if ALL_CURRENT[f] != v})


def test_each_event_alone_ends_what_the_table_says(driver):
    _check_table(driver(_table_rows(), 'table'))


def test_events_that_depend_on_what_the_record_held(driver):
    out = driver([
        (NEW_HANDLE,),                                      # 0: nothing current, no set-up, no key, no error vector
        (START, S0), (COMPLETION_DONE, 1), (ATTEMPT_BEGINS,),                      # 3: a vector that is stored stays through the next attempt
        (START, S0), (STATE_WRITTEN, 0), (CHECKPOINT_SAVED,), (STATE_GROOMED,), (CHECKPOINT_RESTORED,),     # 8: the proof of the saved state, not of the groomed one
        (START, S0), (CHECKPOINT_SAVED,), (PARAMS_CHANGED,), (STATE_GROOMED,), (CHECKPOINT_RESTORED,),      # 13: moved floors end the proof in the slot
        (START, S0), (STATE_HANDED_OUT,), (PLANES_RECOMPUTED, 0, 1),               # 16: pins the exception: the hand-out alone never makes ensure_coef run
        (START, S0), (COMPLETION_DONE, 1), (STAGE_VECTORS_BORROWED, 0),            # 19: the test entry's stages alone leave a stored vector, as an attempt does
        (START, S0), (COMPLETION_DONE, 1), (STAGE_VECTORS_BORROWED, 1),            # 22: its completion overwrote the stored vector: nothing to hand out
    ], 'cases')
    assert out[0] == {**{f: 0 for f in FIELDS}, 'mg_shift': -1, 'mg_graph_shift': -1, 'poly_shift': -1, 'query': -1}
    assert (out[3]['have_err'], out[3]['err_pending'], out[3]['dr_valid']) == (1, 0, 0)
    assert (out[6]['ckpt_floor_ok'], out[7]['floor_ok'], out[8]['floor_ok'], out[8]['coef_fresh']) == (0, 1, 0, 0)
    assert (out[11]['ckpt_floor_ok'], out[12]['floor_ok'], out[13]['floor_ok']) == (0, 1, 0)
    assert (out[15]['coef_fresh'], out[15]['floor_ok']) == (1, 0)
    assert (out[19]['have_err'], out[19]['err_pending'], out[19]['dr_valid']) == (1, 0, 0)
    assert (out[22]['have_err'], out[22]['err_pending'], out[22]['dr_valid']) == (0, 0, 0)


# ---- (b) the model ------------------------------------------------------------------------------------------------------------------
class Model:
    """True generation numbers of everything a product is made from, and for every product the generations it was built from.  The
    products hang on each other in the order the code makes them (ensure_coef before everything; mg_precond: coarse planes, then the
    set-up, then the captured cycle), so `current` follows the same chain: a product counts only while everything before it does."""

    def __init__(self):
        self.gen = dict(state=0, params=0, planes=0, coarse=0, setup=0, config=0, levels=0, step=0, polycfg=0, basis=0, front=0, attempt=0)
        self.built = {}                    # product -> the generations it was built from

    def bump(self, *names):
        for n in names:
            self.gen[n] += 1

    def build(self, product, *names, **extra):
        self.built[product] = dict({n: self.gen[n] for n in names}, **extra)

    def is_current(self, product, **extra):
        b = self.built.get(product)
        return b is not None and all(self.gen.get(n, extra.get(n)) == v for n, v in b.items())


def _sequence(rng, nev):
    """one sequence: the rows for the driver and, per row, a copy of the model after it.  Events come at random; a setter comes only
    where the code calls it, behind the products it reads (mg_restrict_coefs behind ensure_coef, mg_setup_shift behind the coarse
    planes, the capture behind the set-up).  Whether those are current is decided by the model alone, never by the record under test.
    "State handed out" is left out: it deliberately keeps the planes (test_events_that_depend_on_what_the_record_held pins it)."""
    m = Model()
    rows, checks = [(NEW_HANDLE,)], [None]
    shifts = [0.5, 2.0, 8.0]
    keys = [(1, 0), (1, 1), (2, 0)]

    def emit(row, fn=None, inside=False):
        """inside: the row is not the last of the calls one function of the library makes (mg_setup_shift, ksfd_mg_coarse_apply): the
        record is looked at when the function returns"""
        if fn:
            fn()
        rows.append(row)
        checks.append('inside' if inside else {k: dict(v) for k, v in m.built.items()} | {'_gen': dict(m.gen)})

    planes_ok = lambda: m.is_current('planes')
    coarse_ok = lambda: planes_ok() and m.is_current('coarse')
    setup_ok = lambda: coarse_ok() and 'setup' in m.built and m.is_current('setup', shift=m.built['setup']['shift'])
    for _ in range(nev):
        k = int(rng.integers(0, 28))
        if k == 0:
            emit((STATE_WRITTEN, int(rng.integers(0, 2))), lambda: m.bump('state'))
        elif k == 1:
            emit((PARAMS_CHANGED,), lambda: m.bump('params'))
        elif k == 2:
            emit((STATE_GROOMED,))
        elif k == 3:                                                         # ensure_coef (the code runs it only when the planes have ended; any time is legal)
            c32, means = int(rng.integers(0, 2)), int(rng.integers(0, 2))

            def f():
                m.bump('planes')
                m.build('planes', 'state', 'params')
                if c32:
                    m.build('coef32', 'planes')
                if means:
                    m.build('means', 'planes')
            emit((PLANES_RECOMPUTED, c32, means), f)
        elif k == 4 and planes_ok():
            emit((COEF32_MADE,), lambda: m.build('coef32', 'planes'))
        elif k == 5 and planes_ok():
            emit((MEANS_COMPUTED,), lambda: m.build('means', 'planes'))
        elif k == 6 and planes_ok() and not coarse_ok():                     # mg_restrict_coefs runs only when the coarse planes have ended
            emit((COARSE_PLANES_RESTRICTED,), lambda: (m.bump('coarse'), m.build('coarse', 'planes', 'levels')))
        elif k in (7, 8) and coarse_ok():                                    # mg_setup_shift, with the exact coarse solve going through or not
            s, exact = float(rng.choice(shifts)), int(rng.integers(0, 3))
            emit((COARSE_FACTORS_ENDED,), inside=True)
            if exact == 1:
                emit((COARSE_FACTORS_READY,), lambda: m.build('factors', 'coarse', 'config', 'levels', nextsetup=m.gen['setup'] + 1), inside=True)
            emit((SHIFT_SETUP_DONE, s), lambda: (m.bump('setup'), m.build('setup', 'coarse', 'config', 'levels', 'setup', shift=s)))
        elif k == 9 and setup_ok():                                          # mg_coarse_graph after a key mismatch
            x, f32 = keys[int(rng.integers(0, len(keys)))]
            s = m.built['setup']['shift']
            emit((GRAPH_CAPTURED, s, x, f32), lambda: m.build('graph', 'setup', 'levels', key=(s, x, f32)))
        elif k == 10:
            emit((VCYCLE_CONFIG_CHANGED,), lambda: m.bump('config'))
        elif k == 11:
            emit((HIERARCHY_FREED,), lambda: m.bump('levels'))
        elif k == 12 and coarse_ok():                                        # mg_coarse_apply op 1: the factors at a shift of the entry's own
            emit((HIERARCHY_BORROWED,), lambda: m.bump('config'), inside=True)
            emit((COARSE_FACTORS_ENDED,), inside=True)
            emit((COARSE_FACTORS_READY,), inside=True)
            emit((HIERARCHY_BORROWED,))
        elif k == 13:
            emit((HIERARCHY_BORROWED,), lambda: m.bump('config'))
        elif k == 14:
            emit((STEP_BEGINS,), lambda: m.bump('step'))
        elif k == 15:
            s = float(rng.choice(shifts))
            emit((POLY_SET_UP, s), lambda: m.build('poly', 'step', 'polycfg', shift=s))
        elif k == 16:
            emit((POLY_CONFIG_CHANGED,), lambda: m.bump('polycfg'))
        elif k == 17:
            emit((ATTEMPT_BEGINS,), lambda: m.bump('attempt'))
        elif k == 18:
            behind = int(rng.integers(0, 2))
            emit((KRYLOV_BASIS_OVERWRITTEN, behind), lambda: m.bump('basis') if behind else m.bump('basis', 'front'))
        elif k == 19:
            emit((RECYCLED_SPACES_DROPPED,), lambda: m.bump('front'))      # the spaces are given up: whatever is kept later is new
        elif k == 20:
            q = int(rng.integers(0, 4))
            emit((RECYCLED_SPACE_KEPT, q, int(rng.integers(1, 30)), int(rng.integers(0, 30))), lambda: m.build('rec%d' % q, 'front'))
        elif k == 21:
            emit((DR_RELATION_KEPT,), lambda: m.build('dr', 'basis', 'attempt'))
        elif k == 22:
            stored = int(rng.integers(0, 2))
            emit((COMPLETION_DONE, stored))
        elif k == 23:
            emit((CHECKPOINT_SAVED,))
        elif k == 24:
            emit((CHECKPOINT_RESTORED,), lambda: m.bump('state'))
        elif k == 25:
            emit((ERROR_VECTOR_FORMED,))
        elif k == 26:                                                        # ksfd_stage_rhs: an attempt of the entry's own
            emit((STAGE_VECTORS_BORROWED, int(rng.integers(0, 2))), lambda: m.bump('attempt'))
        elif k == 27:                                                        # ... which only ends what it made for itself
            emit((DERIVED_GIVEN_BACK, int(rng.integers(0, 8))))
    return rows, checks


def _check_invariant(rec, snap):
    """rec: the record as the driver printed it; snap: the model after the same event"""
    m = Model()
    m.gen, m.built = snap['_gen'], {k: v for k, v in snap.items() if k != '_gen'}
    planes = bool(rec['coef_fresh'])
    if planes:
        assert m.is_current('planes'), 'planes'
    if planes and rec['coef32_fresh']:
        assert m.is_current('coef32'), 'coef32'
    if planes and rec['means_valid']:
        assert m.is_current('means'), 'means'
    coarse = planes and bool(rec['mg_coef_valid'])
    if coarse:
        assert m.is_current('coarse'), 'coarse planes'
    setup = coarse and rec['mg_shift'] != -1.0
    if setup:
        assert m.is_current('setup', shift=rec['mg_shift']), 'shift set-up'
        assert m.built['setup']['shift'] == rec['mg_shift']
    if setup and rec['mgc_ready']:
        assert m.is_current('factors', nextsetup=m.gen['setup']), 'coarse factors'
    if setup and rec['mg_graph_shift'] == rec['mg_shift']:
        assert m.is_current('graph', key=m.built['graph']['key']), 'captured cycle'
        assert m.built['graph']['key'] == (rec['mg_graph_shift'], rec['mg_graph_x'], rec['mg_graph_f32'])
    if rec['poly_shift'] != -1.0:
        assert m.is_current('poly', shift=rec['poly_shift']) and m.built['poly']['shift'] == rec['poly_shift'], 'polynomial'
    if rec['dr_valid']:
        assert m.is_current('dr'), 'deflated relation'
    for q in range(4):
        if rec['rec%d' % q]:
            assert m.is_current('rec%d' % q), 'recycled space %d' % q


def test_random_sequences_against_the_generation_model(driver):
    rng = np.random.default_rng(20261021)
    rows, checks = [], []
    for _ in range(2000):
        r, c = _sequence(rng, 40)
        rows += r
        checks += c
    out = driver(rows, 'model')
    seen = set()
    for k, (rec, snap) in enumerate(zip(out, checks)):
        if snap is None or snap == 'inside':
            continue
        try:
            _check_invariant(rec, snap)
        except AssertionError as e:
            first = max(j for j in range(k + 1) if checks[j] is None)
            raise AssertionError('%s stale after %r' % (e, rows[first:k + 1]))
        planes = rec['coef_fresh']
        seen |= {n for n, on in (('planes', planes), ('coef32', planes and rec['coef32_fresh']), ('means', planes and rec['means_valid']),
                                 ('coarse', planes and rec['mg_coef_valid']), ('setup', planes and rec['mg_coef_valid'] and rec['mg_shift'] != -1),
                                 ('factors', planes and rec['mg_coef_valid'] and rec['mg_shift'] != -1 and rec['mgc_ready']),
                                 ('graph', planes and rec['mg_coef_valid'] and rec['mg_shift'] != -1 and rec['mg_graph_shift'] == rec['mg_shift']),
                                 ('poly', rec['poly_shift'] != -1), ('dr', rec['dr_valid']), ('rec', rec['rec2'])) if on}
    # the sequences are long enough for every product to be reported current somewhere: the check is not vacuous
    assert seen == {'planes', 'coef32', 'means', 'coarse', 'setup', 'factors', 'graph', 'poly', 'dr', 'rec'}


# ---- (c) sanitizers -----------------------------------------------------------------------------------------------------------------
def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    run = _build(tmp_path, 'drv_san', ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    _check_table(run(_table_rows(), 'table'))
