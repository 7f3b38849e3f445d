"""In-place basis rotation of the deflated restart (k_basis_rotate, 31 -> 11 vectors in one pass) against its composition from 11 basis
combinations (op_basis_axpy, out of place, copy-back not counted), HIP events after warm-up.
usage: python tools/rotate_bench.py [n=4096] [nlig=1] [reps=20]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
from ksfd_amd import lib as klib
from ksfd_amd.config import ProblemConfig
from ksfd_amd.initial import start_values

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
nlig = int(sys.argv[2]) if len(sys.argv) > 2 else 1
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
cfg = ProblemConfig.standard(2, (n, n), L=(n / 384.0,) * 2, nlig=nlig)
ks = klib.KSFDHip(cfg)
ks.set_state(start_values(cfg))
vec = 8.0 * cfg.F * n * n
for name, cls, moved in (('one pass', klib.BENCH_ROTATE, (31 + 11) * vec), ('11 combinations', klib.BENCH_ROTATE_COMPOSED, 11 * (31 + 1) * vec)):
    for trial in range(3):
        ms, by = ks.bench_kernel(cls, reps)
        print('%d^2 x %d fields, 31 -> 11 vectors, %-16s trial %d: %.3f ms, %.2f TB/s of the %.2f GB it moves (%.2f TB/s of the rotation\'s own %.2f GB)'
              % (n, cfg.F, name, trial, ms, moved / ms / 1e9, moved / 1e9, (31 + 11) * vec / ms / 1e9, (31 + 11) * vec / 1e9), flush=True)
ks.close()
