"""CPU: the host algebra of the deflated restart (ksfd_amd/csrc/dense_small.h) against numpy.  The header is plain C++ without device
code, so a small driver compiled with the host compiler exercises exactly what the library runs: the real-arithmetic eigen-solver
(Hessenberg reduction, Francis QR, back substitution), the dense least squares, and the GMRES-DR restart plan built from them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

DRIVER = r'''
#include "dense_small.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
using namespace ksfd_dense;
static std::vector<double> rd(FILE *f, size_t n) { std::vector<double> v(n); for (size_t i = 0; i < n; i++) if (fscanf(f, "%lf", &v[i]) != 1) exit(3); return v; }
static void pr(const std::vector<double> &v) { for (double x : v) printf("%.17g\n", x); }
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[2], "r");
    if (!f) return 2;
    if (!strcmp(argv[1], "eig")) {
        int n; if (fscanf(f, "%d", &n) != 1) return 3;
        std::vector<double> A = rd(f, (size_t)n * n), wr, wi, V;
        const bool ok = dense_eig(n, A, wr, wi, V);
        printf("%d\n", ok ? 1 : 0);
        if (ok) { pr(wr); pr(wi); pr(V); }
    } else if (!strcmp(argv[1], "lsq")) {
        int nr, n; if (fscanf(f, "%d %d", &nr, &n) != 2) return 3;
        std::vector<double> H = rd(f, (size_t)nr * n), c = rd(f, nr), y(n), rho(nr);
        const bool ok = dense_lsq(nr, n, H.data(), nr, c.data(), y.data(), rho.data());
        printf("%d\n", ok ? 1 : 0);
        if (ok) { pr(y); pr(rho); }
    } else {
        int nr, n, keep; if (fscanf(f, "%d %d %d", &nr, &n, &keep) != 3) return 3;
        std::vector<double> H = rd(f, (size_t)nr * n), rho = rd(f, nr);         /* H column-major, ld = nr */
        DrPlan p;
        const bool ok = dr_plan(nr, n, H.data(), nr, rho.data(), keep, 18, p);
        printf("%d\n", ok ? p.kk : -1);
        if (ok) { pr(p.P); pr(p.Hnew); pr(p.cnew); pr(p.theta_r); pr(p.theta_i); }
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    # the host compiler, else the compiler the library itself is built with (the header is plain C++ either way); none at all is a
    # broken build environment, not a reason to skip the only direct test of the eigen-solver and the restart plan
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('hipcc') or (hipcc if os.path.exists(hipcc) else None)
    if not cxx:
        pytest.fail('no C++ compiler found (g++, c++, hipcc): the library cannot have been built either')
    d = tmp_path_factory.mktemp('dense')
    (d / 'drv.cpp').write_text(DRIVER)
    exe = d / 'drv'
    subprocess.run([cxx, '-x', 'c++', '-O1', '-std=c++17', '-I', ROOT + '/ksfd_amd/csrc', str(d / 'drv.cpp'), '-o', str(exe)], check=True)

    def run(mode, head, *arrays):
        inp = d / 'in.txt'
        with open(inp, 'w') as f:
            f.write(' '.join(str(int(x)) for x in head) + '\n')
            for a in arrays:
                f.write('\n'.join(repr(float(x)) for x in np.asarray(a).ravel()) + '\n')
        r = subprocess.run([str(exe), mode, str(inp)], capture_output=True, text=True, check=True, timeout=60)
        return np.array([float(x) for x in r.stdout.split()])
    return run


def _check_eig(run, A):
    n = A.shape[0]
    out = run('eig', [n], A)
    assert out[0] == 1
    wr, wi, V = out[1:1 + n], out[1 + n:1 + 2 * n], out[1 + 2 * n:].reshape(n, n)
    lam = wr + 1j * wi
    ref = np.linalg.eigvals(A)
    scale = max(np.abs(ref).max(), 1e-300)
    # same spectrum: every computed value has a reference value next to it and the other way round
    assert max(np.abs(ref - l).min() for l in lam) < 1e-9 * scale
    assert max(np.abs(lam - l).min() for l in ref) < 1e-9 * scale
    j = 0
    while j < n:
        if wi[j] == 0:
            v = V[:, j].astype(complex); step = 1
        else:
            assert wi[j] > 0 and wi[j + 1] == -wi[j] and wr[j + 1] == wr[j]          # a pair: real part, imaginary part
            v = V[:, j] + 1j * V[:, j + 1]; step = 2
        assert np.linalg.norm(v) > 0
        assert np.linalg.norm(A @ v - lam[j] * v) < 1e-10 * np.linalg.norm(A, 2) * np.linalg.norm(v), (n, j)
        j += step


@pytest.mark.parametrize('n', [1, 2, 3, 7, 30, 120])
def test_eigen_solver_matches_numpy(driver, n):
    rng = np.random.default_rng(n)
    _check_eig(driver, rng.standard_normal((n, n)))                                  # complex pairs throughout
    S = rng.standard_normal((n, n))
    _check_eig(driver, S + S.T)                                                      # real spectrum
    H = np.triu(rng.standard_normal((n, n)), -1)
    _check_eig(driver, H)                                                            # already Hessenberg, as in the first cycle
    if n >= 3:
        H[n // 2, n // 2 - 1] = 0.0
        _check_eig(driver, H)                                                        # decoupled blocks (a breakdown inside the cycle)


def test_least_squares_matches_numpy(driver):
    rng = np.random.default_rng(5)
    for nr, n in [(2, 1), (31, 30), (32, 30), (13, 7)]:
        H, c = rng.standard_normal((nr, n)), rng.standard_normal(nr)
        out = driver('lsq', [nr, n], H.T, c)                                          # column-major
        assert out[0] == 1
        y, rho = out[1:1 + n], out[1 + n:]
        yr = np.linalg.lstsq(H, c, rcond=None)[0]
        assert np.linalg.norm(y - yr) < 1e-12 * max(1.0, np.linalg.norm(yr))
        assert np.linalg.norm(rho - (c - H @ yr)) < 1e-12 * np.linalg.norm(c)
    assert driver('lsq', [3, 2], np.zeros((2, 3)), np.ones(3))[0] == 0              # rank deficient: refused


def _arnoldi(A, b, m, V0=None):
    n = b.size
    V = np.zeros((n, m + 1)); H = np.zeros((m + 1, m))
    V[:, 0] = b / np.linalg.norm(b)
    for j in range(m):
        w = A @ V[:, j]
        for _ in range(2):
            d = V[:, :j + 1].T @ w
            w -= V[:, :j + 1] @ d
            H[:j + 1, j] += d
        H[j + 1, j] = np.linalg.norm(w)
        V[:, j + 1] = w / H[j + 1, j]
    return V, H


@pytest.mark.parametrize('keep', [1, 4, 10, 16])
def test_restart_plan_is_a_deflated_arnoldi_relation(driver, keep):
    """an indefinite matrix with a few eigenvalues left of the origin: the plan keeps the harmonic Ritz values of smallest modulus, P is
    orthonormal, contains the residual direction, and Hb P_k lies in span(P_k+1) -- which is what makes A V_k' = V_k+1' Hnew a relation"""
    rng = np.random.default_rng(100 + keep)
    N, m = 150, 30
    Q = np.linalg.qr(rng.standard_normal((N, N)))[0]
    ev = np.concatenate([-rng.uniform(0.05, 0.5, 4), rng.uniform(0.02, 3.0, N - 4)])
    A = Q @ np.diag(ev) @ Q.T + 0.05 * rng.standard_normal((N, N)) / np.sqrt(N)      # nonsymmetric part: complex harmonic Ritz pairs occur
    b = rng.standard_normal(N)
    V, H = _arnoldi(A, b, m)
    c = np.zeros(m + 1); c[0] = np.linalg.norm(b)
    y = np.linalg.lstsq(H, c, rcond=None)[0]
    rho = c - H @ y
    out = driver('plan', [m + 1, m, keep], H.T, rho)
    kk = int(out[0])
    assert kk in (keep, keep + 1)
    o = 1
    P = out[o:o + (m + 1) * 18].reshape(m + 1, 18)[:, :kk + 1]; o += (m + 1) * 18
    Hn = out[o:o + (kk + 1) * kk].reshape(kk, kk + 1).T; o += (kk + 1) * kk
    cn = out[o:o + kk + 1]; o += kk + 1
    th = out[o:o + kk] + 1j * out[o + kk:o + 2 * kk]
    assert np.abs(P.T @ P - np.eye(kk + 1)).max() < 1e-13
    assert np.abs(P[m, :kk]).max() == 0.0                                            # kept vectors live in V_m, only the residual reaches v_m+1
    HP = H @ P[:m, :kk]
    assert np.linalg.norm(HP - P @ Hn) < 1e-10 * np.linalg.norm(HP)
    assert np.linalg.norm(P @ cn - rho) < 1e-12 * np.linalg.norm(rho)               # the residual is in the new basis
    Hm = H[:m]
    em = np.zeros(m); em[-1] = 1.0
    ref = np.linalg.eigvals(Hm + H[m, m - 1] ** 2 * np.outer(np.linalg.solve(Hm.T, em), em))
    ref = ref[np.argsort(np.abs(ref))]
    assert max(np.abs(ref[:kk] - t).min() for t in th) < 1e-8 * np.abs(ref).max()
    assert np.abs(th).max() <= np.abs(ref[kk - 1]) * (1 + 1e-8)                       # the smallest ones
    # the rotated full-size relation holds: A (V_m P_k) = (V_m+1 P_k+1) Hnew
    Vn = V @ P
    assert np.linalg.norm(A @ Vn[:, :kk] - Vn @ Hn) < 1e-9 * np.linalg.norm(A, 2)


def test_restart_plan_refuses_what_it_cannot_deflate(driver):
    rng = np.random.default_rng(9)
    m = 12
    H = np.triu(rng.standard_normal((m + 1, m)), -1)
    res = lambda Hx: (lambda c: c - Hx @ np.linalg.lstsq(Hx, c, rcond=None)[0])(rng.standard_normal(Hx.shape[0]))
    rho = res(H)                                                                     # a least-squares residual, as in the solver
    assert driver('plan', [m + 1, m, 4], H.T, rho)[0] in (4, 5)
    assert driver('plan', [m + 1, m, 4], H.T, rng.standard_normal(m + 1))[0] == -1  # not one: the relation would not close
    Hs = H.copy(); Hs[:m, 0] = 0.0; Hs[1, 0] = 0.0                                   # singular H_m
    assert driver('plan', [m + 1, m, 4], Hs.T, rho)[0] == -1
    assert driver('plan', [m + 1, m, 11], H.T, rho)[0] == -1                         # keep > n - 2
    assert driver('plan', [m + 1, m, 4], H.T, np.zeros(m + 1))[0] == -1             # zero residual (happy breakdown): nothing to restart from
    # a cycle that started from a kept space has two trailing rows
    H2 = rng.standard_normal((m + 2, m))
    out = driver('plan', [m + 2, m, 3], H2.T, res(H2))
    kk = int(out[0])
    assert kk in (3, 4)
    P = out[1:1 + (m + 2) * 18].reshape(m + 2, 18)[:, :kk + 2]                       # the complement of range(H2) has two dimensions
    Hn = out[1 + (m + 2) * 18:1 + (m + 2) * 18 + (kk + 2) * kk].reshape(kk, kk + 2).T
    HP = H2 @ P[:m, :kk]
    assert np.abs(P.T @ P - np.eye(kk + 2)).max() < 1e-13
    N = np.linalg.svd(H2, full_matrices=True)[0][:, m:]                               # range(H2)^perp lies in span(P)
    assert np.linalg.norm(N - P @ (P.T @ N)) < 1e-12
    assert np.linalg.norm(HP - P @ Hn) < 1e-10 * np.linalg.norm(HP)
