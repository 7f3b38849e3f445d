"""Bitwise digest of the spectral stage solver of one libksfd_hip.so: one line per item with the SHA-256 of the output bytes.

    python tools/spec_digest.py path/to/libksfd_hip.so > digest.txt

Two builds that make the same launches with the same arguments in the same order print the same file; run it once per library (one
library per process) and diff.  Items, all on seeded inputs at the state and the two shifts of tests/test_gpu_spectral.py:
  apply    ksfd_spectral_apply on one rank: 2-D with 1, 2, 3 and 5 ligands (template and run-time pair counts), 3 * 2^k on either axis,
           both split column kernels (KSFD_SPEC_SPLIT set before the handle is created); 3-D with 1, 2 and 4 ligands, 3 * 2^k on each axis
  ring     the same through the ring of one rank (RCCL transport, own-piece all-to-alls): (48, 96) split columns in three chunks,
           (48, 32, 48) z planes in three chunks -- left out with a note where a single process cannot open that transport
  steps    the state after 3 steps solved by the spectral defect correction (pc_type 4) on 64x64 at ksp_rtol 1e-6 (fp32 residual input, x
           update, stage guesses) and 1e-11, and with each the launches and bytes of every kernel class (ksfd_get_profile)"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ksfd_amd import lib as klib                     # noqa: E402
from ksfd_amd.config import ProblemConfig            # noqa: E402

GAMMA = 4.3586652150845900e-01
SHIFTS = tuple(1.0 / (GAMMA * h) for h in (0.02, 5.0))

# (shape, ligands, KSFD_SPEC_SPLIT)
APPLY = [((64, 32), 1, None), ((32, 128), 2, None), ((64, 64), 3, None), ((32, 64), 5, None), ((96, 48), 1, None), ((48, 96), 2, None),
         ((64, 128), 2, '1'), ((128, 64), 1, '2'),
         ((32, 32, 32), 1, None), ((64, 32, 128), 2, None), ((32, 32, 32), 4, None), ((48, 32, 32), 1, None), ((32, 48, 32), 1, None),
         ((32, 32, 48), 1, None)]
RING = [((48, 96), 2, '1'), ((48, 32, 48), 1, None)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def config(shape, nlig):
    """the configurations of tests/test_gpu_spectral.py: standard ligands, three in two groups, many in three groups"""
    dim, L = len(shape), tuple(n * 4.0 / 1536 for n in shape)
    if nlig == 3:
        return ProblemConfig(dim=dim, n=shape, L=L, lig_group=[0, 0, 1], lig_w=[1.0, 0.5, 1.0], lig_s=[0.01, 0.02, 0.001],
                             lig_gamma=[0.01, 0.03, 0.001], lig_D=[1e-6, 3e-6, 1e-5], grp_alpha=[1500.0, 1500.0], grp_beta=[5.56e-4, -5.56e-4])
    if nlig > 3:
        rng = np.random.default_rng(100 + nlig)
        return ProblemConfig(dim=dim, n=shape, L=L, lig_group=[l % 3 for l in range(nlig)], lig_w=0.5 + rng.random(nlig),
                             lig_s=0.005 + 0.01 * rng.random(nlig), lig_gamma=0.005 + 0.01 * rng.random(nlig), lig_D=1e-6 * (1 + rng.random(nlig)),
                             grp_alpha=[1500.0, 1200.0, 1800.0], grp_beta=[5.56e-4, -3e-4, 2e-4])
    return ProblemConfig.standard(dim, shape, L=L, nlig=nlig)


def state(cfg, seed=3, amp=90.0):
    rng = np.random.default_rng(seed)
    rho = 9000.0 + amp * rng.standard_normal(cfg.N)
    return np.concatenate([rho] + [rho * cfg.lig_s[l] / cfg.lig_gamma[l] * (1 + 0.01 * rng.standard_normal(cfg.N)) for l in range(cfg.nlig)])


def apply_item(kind, shape, nlig, split, opener):
    name = '%s %s ligands %d split %s' % (kind, 'x'.join(str(n) for n in shape), nlig, split or '-')
    if split:
        os.environ['KSFD_SPEC_SPLIT'] = split        # read when the handle is created
    try:
        cfg = config(shape, nlig)
        k = opener(cfg)
    except Exception as e:                           # the ring of one needs the RCCL transport in this process
        print('%s not run: %s' % (name, type(e).__name__))
        return
    finally:
        os.environ.pop('KSFD_SPEC_SPLIT', None)
    k.set_state(state(cfg))
    v = np.random.default_rng(4).standard_normal(cfg.F * cfg.N)
    for shift in SHIFTS:
        print('%s shift %s %s' % (name, float(shift).hex(), sha(k.spectral_apply(shift, v))))
    k.close()


KEEP = []                                            # the communicator ids outlive their handles


def ring_of_one(cfg):
    from ksfd_amd.dist import open_self_ring
    ks, keep = open_self_ring(cfg, 0, 'rccl')
    KEEP.append(keep)
    return ks


def steps(ksp_rtol):
    cfg = config((64, 64), 1)
    k = klib.KSFDHip(cfg)
    k.set_state(state(cfg))
    k.set_profiling(True)
    k.profile(reset=True)
    opts = klib.default_step_opts(adapt=1, atol=0.01, rtol=1e-6, ksp_rtol=ksp_rtol, pc_type=4)
    t, h, its, used = 0.0, 0.3, 0, 0
    for _ in range(3):
        t, h, st, rc = k.step(t, h, opts)
        its += st.linear_its
        used |= st.pc_used
    print('steps 64x64 ksp_rtol %g t %s h %s its %d pc_used %d state %s' % (ksp_rtol, float(t).hex(), float(h).hex(), its, used, sha(k.get_state())))
    for cls, p in sorted(k.profile().items()):
        print('steps 64x64 ksp_rtol %g class %s launches %d bytes %r alg_bytes %r' % (ksp_rtol, cls, p['launches'], float(p['bytes']), float(p['alg_bytes'])))
    k.close()


def main():
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    klib.LIB_PATH = os.path.abspath(sys.argv[1])     # before the first handle loads the library
    for shape, nlig, split in APPLY:
        apply_item('apply', shape, nlig, split, klib.KSFDHip)
    for shape, nlig, split in RING:
        apply_item('ring', shape, nlig, split, ring_of_one)
    for ksp_rtol in (1e-6, 1e-11):
        steps(ksp_rtol)


if __name__ == '__main__':
    main()
