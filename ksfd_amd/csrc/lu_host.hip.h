// libksfd_hip.so -- dense direct stage solver (pc_type 5): assembly of shift*I - J(u), LU factorization and triangular solves on the
// device (kernels in lu.hip.h), iterative refinement against the frozen-coefficient Jacobian action
// (part of the single translation unit ksfd_hip.hip; included after krylov.hip.h)
#pragma once

// Checked before anything is allocated or the state is touched: the dense factors of F*nloc unknowns take 8 (F*nloc)^2 bytes
static int direct_guard(ksfd_handle *h)
{
    const double n = (double)h->G.F * (double)h->G.nloc;
    if (n > (double)KSFD_DIRECT_MAX)
        return fail(h, KSFD_EINVAL, "direct solver (pc_type 5): %.0f unknowns exceed KSFD_DIRECT_MAX = %d (%.1f GB of dense factors); "
                                    "use pc_type 2", n, KSFD_DIRECT_MAX, 8.0 * n * n / 1e9);
    if (h->ring) return fail(h, KSFD_EINVAL, "direct solver (pc_type 5): single rank only (this handle has a halo transport)");
    return KSFD_OK;
}

// The factorization is a function of (geometry, physics, coefficient planes, LUState): pc_type 5 runs it on the handle's own grid,
// the exact coarse solve of the V cycle (mgc_setup) on a level of the hierarchy with that level's restricted planes.
struct LUSys {
    const KGeom *G;
    const KPhys *P;
    const double *coef;                      // [rho, G, G_rho, G_U..] planes of that grid
    long long gslow, slow0;                  // global extent of the slow axis, first owned slow index (k_jac_csr)
    int cls;                                 // kernel class the launches are booked under
};

static void lu_free(LUState &S)
{
    void *bufs[] = { S.A, S.piv, S.perm, S.info, S.col, S.val, S.y, S.z };
    for (void *b : bufs) if (b) hipFree(b);
    S = LUState();
}
static void direct_free(ksfd_handle *h) { lu_free(h->lu); }

// Jacobian entries k_jac_csr writes for a grid of nloc points
static int64_t lu_nnz(const KGeom &G, int nlig)
{
    const int64_t npts = 4 * G.dim + 1;
    return G.nloc * ((int64_t)G.F * npts + (int64_t)nlig * (npts + 1));
}

// solve_vectors: y, z of the triangular solves and the host copies of the pivots (pc_type 5); the coarse solve inverts instead
static int lu_alloc(ksfd_handle *h, LUState &S, int64_t n, int64_t nnz, bool solve_vectors)
{
    if (S.A) return KSFD_OK;
    bool ok = hipMalloc((void **)&S.A, sizeof(double) * (size_t)n * (size_t)n) == hipSuccess;
    ok = ok && hipMalloc((void **)&S.piv, sizeof(int) * (size_t)n) == hipSuccess;
    ok = ok && (!solve_vectors || hipMalloc((void **)&S.perm, sizeof(int) * (size_t)n) == hipSuccess);
    ok = ok && hipMalloc((void **)&S.info, sizeof(int)) == hipSuccess;
    ok = ok && hipMalloc((void **)&S.col, sizeof(long long) * (size_t)nnz) == hipSuccess;
    ok = ok && hipMalloc((void **)&S.val, sizeof(double) * (size_t)nnz) == hipSuccess;
    ok = ok && (!solve_vectors || hipMalloc((void **)&S.y, sizeof(double) * (size_t)n) == hipSuccess);
    ok = ok && (!solve_vectors || hipMalloc((void **)&S.z, sizeof(double) * (size_t)n) == hipSuccess);
    if (!ok) {
        (void)hipGetLastError();
        lu_free(S);
        return fail(h, KSFD_ENOMEM, "direct solver: hipMalloc of the %.2f GB of dense factors failed", 8.0 * (double)n * (double)n / 1e9);
    }
    S.n = n;
    S.nnz = nnz;
    if (solve_vectors) {
        S.piv_h.assign((size_t)n, 0);
        S.perm_h.assign((size_t)n, 0);
    }
    return KSFD_OK;
}

static int direct_alloc(ksfd_handle *h)
{
    return lu_alloc(h, h->lu, (int64_t)h->G.F * h->G.nloc, lu_nnz(h->G, h->P.nlig), true);
}

// S.A = shift*I - J of the system Y (dense, column-major), *S.info = 0
static int lu_assemble(ksfd_handle *h, LUState &S, const LUSys &Y, double shift)
{
    const KGeom &G = *Y.G;
    const long long n = S.n;
    const double dn = (double)n;
    S.valid = false;
    const int nbp = (int)std::min<long long>((G.nloc + KSFD_BLOCK - 1) / KSFD_BLOCK, 65535);
    {
        Scope sc(h, Y.cls, 16.0 * (double)S.nnz + 8.0 * (3 + h->P.nlig) * (double)G.nloc);
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_jac_csr<NL>), dim3(nbp), dim3(KSFD_BLOCK), 0, h->st, G, *Y.P, Y.coef,
                                                  Y.gslow, Y.slow0, S.col, S.val));
    }
    HIPCHK(h, hipGetLastError());
    {
        Scope sc(h, Y.cls, 8.0 * dn * dn);
        HIPCHK(h, hipMemsetAsync(S.A, 0, sizeof(double) * (size_t)n * (size_t)n, h->st));
    }
    {
        Scope sc(h, Y.cls, 4.0);
        HIPCHK(h, hipMemsetAsync(S.info, 0, sizeof(int), h->st));
    }
    {
        Scope sc(h, Y.cls, 32.0 * (double)S.nnz + 16.0 * dn);     // entries read, A entries read and written (strided)
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_lu_scatter<NL>), dim3(nbp), dim3(KSFD_BLOCK), 0, h->st, (long long)G.nloc, G.dim,
                                                  (const long long *)S.col, (const double *)S.val, shift, S.A));
    }
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

// Blocked right-looking LU of S.A in place.  one_launch_panels false: two launches per column (k_lu_pivot, k_lu_panel_col), any n;
// true: k_lu_panel, one launch per 64-column panel (n <= KSFD_MG_DIRECT_MAX).  The interchanges, the U12 solve and the trailing update
// follow per panel either way.  Asynchronous: the caller reads S.info.
static int lu_factor_blocks(ksfd_handle *h, LUState &S, int cls, bool one_launch_panels)
{
    const long long n = S.n;
    constexpr int NB = KSFD_LU_NB;
    for (long long k0 = 0; k0 < n; k0 += NB) {
        const long long k1 = std::min<long long>(k0 + NB, n), kw = k1 - k0;
        if (one_launch_panels) {
            Scope sc(h, cls, 8.0 * (double)(n - k0) * (double)kw * (1.0 + (double)kw));
            hipLaunchKernelGGL(k_lu_panel, dim3(1), dim3(KSFD_LU_PANT), 0, h->st, S.A, n, k0, k1, S.piv, S.info);
        } else
        for (long long j = k0; j < k1; j++) {
            {
                Scope sc(h, cls, 8.0 * (double)(n - j) + 32.0 * (double)kw);
                hipLaunchKernelGGL(k_lu_pivot, dim3(1), dim3(KSFD_LU_PIVT), 0, h->st, S.A, n, j, k0, k1, S.piv, S.info);
            }
            if (j + 1 < n) {
                const long long rows = n - j - 1;
                Scope sc(h, cls, 8.0 * (double)rows * (1.0 + 2.0 * (double)(k1 - j - 1)));
                hipLaunchKernelGGL(k_lu_panel_col, dim3((unsigned)((rows + KSFD_LU_ROWS - 1) / KSFD_LU_ROWS)), dim3(KSFD_LU_ROWS), 0, h->st,
                                   S.A, n, j, k1, (const int *)S.info);
            }
        }
        if (n > kw) {
            Scope sc(h, cls, 32.0 * (double)kw * (double)(n - kw));
            hipLaunchKernelGGL(k_lu_laswp, dim3((unsigned)((n - kw + KSFD_BLOCK - 1) / KSFD_BLOCK)), dim3(KSFD_BLOCK), 0, h->st,
                               S.A, n, k0, k1, (const int *)S.piv, (const int *)S.info);
        }
        const long long m = n - k1;
        if (m > 0) {
            const int tiles = (int)((m + NB - 1) / NB);
            {
                Scope sc(h, cls, 8.0 * NB * NB * tiles + 16.0 * NB * (double)m);
                hipLaunchKernelGGL(k_lu_trsm, dim3(tiles), dim3(KSFD_BLOCK), 0, h->st, S.A, n, k0, (const int *)S.info);
            }
            {
                Scope sc(h, cls, 16.0 * (double)m * (double)m + 16.0 * NB * (double)m);   // A22 read + written, L21 and U12 read
                hipLaunchKernelGGL(k_lu_gemm, dim3((unsigned)tiles * (unsigned)tiles), dim3(KSFD_BLOCK), 0, h->st, S.A, n, k0, tiles, (const int *)S.info);
            }
        }
        HIPCHK(h, hipGetLastError());
    }
    return KSFD_OK;
}

// A = shift*I - J at the resident coefficient planes (ensure_coef first), factored in place: P A = L U
static int direct_factor(ksfd_handle *h, double shift)
{
    int rc;
    if ((rc = direct_alloc(h))) return rc;
    LUState &S = h->lu;
    const long long n = S.n;
    const LUSys Y{ &h->G, &h->P, h->coef, (long long)h->cfg.n[h->G.dim - 1], (long long)h->slow0, KC_MISC };
    if ((rc = lu_assemble(h, S, Y, shift)) || (rc = lu_factor_blocks(h, S, KC_MISC, false))) return rc;
    int info = 0;
    HIPCHK(h, hipMemcpyAsync(S.piv_h.data(), S.piv, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipMemcpyAsync(&info, S.info, sizeof(int), hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    h->n_host_sync++;
    if (info) return fail(h, KSFD_ELINEAR, "direct solve: zero or non-finite pivot in column %d of shift*I - J (shift %.6g, %lld unknowns)", info - 1, shift, n);
    // P b = the interchanges in order; as a gather: (P b)_i = b[perm[i]]
    for (long long i = 0; i < n; i++) S.perm_h[i] = (int)i;
    for (long long j = 0; j < n; j++) std::swap(S.perm_h[j], S.perm_h[S.piv_h[j]]);
    HIPCHK(h, hipMemcpyAsync(S.perm, S.perm_h.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    S.valid = true;
    S.shift = shift;
    return KSFD_OK;
}

// x = U^-1 L^-1 P b; b and x in the ghosted SoA layout (distinct vectors)
static int direct_solve(ksfd_handle *h, const double *b, double *x)
{
    LUState &S = h->lu;
    if (!S.valid) return fail(h, KSFD_EINVAL, "direct solve without a factorization");
    const KGeom &G = h->G;
    const long long n = S.n;
    constexpr int NB = KSFD_LU_NB;
    const KLUVec V{ G.nloc, G.plane, (long long)G.ng * G.inner };
    const long long nbk = (n + NB - 1) / NB;
    for (long long kb = 0; kb < nbk; kb++) {
        const long long k0 = kb * NB, kw = std::min<long long>(NB, n - k0), rows = n - k0 - kw;
        const unsigned nblk = (unsigned)std::max<long long>(1, (rows + KSFD_LU_ROWS - 1) / KSFD_LU_ROWS);
        Scope sc(h, KC_MISC, 8.0 * (double)(rows + kw) * (double)kw + 16.0 * (double)(rows + kw));
        hipLaunchKernelGGL(k_lu_fwd, dim3(nblk), dim3(KSFD_LU_ROWS), 0, h->st, (const double *)S.A, n, k0, kb == 0 ? 1 : 0, V, b,
                           (const int *)S.perm, S.y, S.z);
    }
    for (long long kb = nbk - 1; kb >= 0; kb--) {
        const long long k0 = kb * NB, kw = std::min<long long>(NB, n - k0);
        const unsigned nblk = (unsigned)std::max<long long>(1, (k0 + KSFD_LU_ROWS - 1) / KSFD_LU_ROWS);
        Scope sc(h, KC_MISC, 8.0 * (double)(k0 + kw) * (double)kw + 16.0 * (double)(k0 + kw));
        hipLaunchKernelGGL(k_lu_bwd, dim3(nblk), dim3(KSFD_LU_ROWS), 0, h->st, (const double *)S.A, n, k0, V, S.z, x);
    }
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

// One stage system (shift*I - J) x = b of ksfd_step: solve, then the true residual b - A x from the frozen-coefficient Jacobian action
// against max(ksp_rtol*||b||, ksp_atol) -- the test of every other solver -- with at most two refinement steps x += A^-1 r.
// ls->its counts the solves (refinements included), ls->rel is the last true relative residual.
// solve: the factored solver the stage runs on (direct_solve, banded_solve); what: its name in the error message.
static int exact_stage(ksfd_handle *h, double shift, const double *b, double *x, const ksfd_step_opts *opts, LinStats *ls,
                       int (*solve)(ksfd_handle *, const double *, double *), const char *what)
{
    int rc;
    ls->its = 0;
    ls->rel = 0.0;
    if ((rc = op_multidot(h, b, b, 0))) return rc;
    const double bn = sqrt(h->hres[0]);
    const double tol = std::max(opts->ksp_rtol * bn, opts->ksp_atol);
    if ((rc = solve(h, b, x))) return rc;
    ls->its = 1;
    for (int ref = 0;; ref++) {
        if ((rc = halo(h, x)) || (rc = op_jvp_frozen(h, x, 2, shift, h->t3, b)) || (rc = op_multidot(h, h->t3, h->t3, 0))) return rc;
        h->n_residual++;
        const double rn = sqrt(h->hres[0]);
        ls->rel = bn > 0.0 ? rn / bn : rn;
        if (rn <= tol) return KSFD_OK;
        if (ref == 2) return fail(h, KSFD_ELINEAR, "%s solve: true residual %.3e above %.3e after two refinement steps", what, rn, tol);
        if ((rc = solve(h, h->t3, h->t2))) return rc;
        const double *xs[2] = { x, h->t2 };
        const double a[2] = { 1.0, 1.0 };
        if ((rc = op_lincomb(h, 2, xs, a, x))) return rc;
        ls->its++;
    }
}

static int direct_stage(ksfd_handle *h, double shift, const double *b, double *x, const ksfd_step_opts *opts, LinStats *ls)
{
    return exact_stage(h, shift, b, x, opts, ls, direct_solve, "direct");
}

// ------------------------------------------------------------------------------------------------
// Exact solve on the level the V cycle ends on (ksfd_set_mg_coarse kind 1; declared in mg_host.hip.h)
// ------------------------------------------------------------------------------------------------
static void mgc_free(ksfd_handle *h)
{
    MGCoarse &C = h->mgc;
    lu_free(C.lu);
    if (C.inv) hipFree(C.inv);
    C.inv = nullptr;
    ksfd_ctl::coarse_factors_ended(h->cur);
}

// buffers of the exact solve on level `level`: factors, Jacobian staging, inverse
static int mgc_alloc(ksfd_handle *h, int level)
{
    MGCoarse &C = h->mgc;
    const MGLevel &L = h->mg[level];
    const int64_t n = (int64_t)L.G.F * L.G.nloc;
    if (C.lu.A && C.lu.n == n && C.inv) return KSFD_OK;
    mgc_free(h);
    int rc;
    if ((rc = lu_alloc(h, C.lu, n, lu_nnz(L.G, h->P.nlig), false))) return rc;
    if (hipMalloc((void **)&C.inv, sizeof(double) * (size_t)n * (size_t)n) != hipSuccess) {
        (void)hipGetLastError();
        mgc_free(h);
        return fail(h, KSFD_ENOMEM, "coarse solve: hipMalloc of the %.1f MB inverse failed", 8.0 * (double)n * (double)n / 1e6);
    }
    return KSFD_OK;
}

// Set-up for this shift on level L (the one the cycle ends on): assemble shift*I - J_c from the level's planes, factor it with one launch
// per panel, invert.  One host wait, for the factorization's flag.  *ok false: zero or non-finite pivot, the caller falls back.
static int mgc_setup(ksfd_handle *h, MGLevel &L, double shift, bool *ok)
{
    int rc;
    MGCoarse &C = h->mgc;
    LUState &S = C.lu;
    *ok = false;
    ksfd_ctl::coarse_factors_ended(h->cur);
    if (!S.A || !C.inv || S.n != (int64_t)L.G.F * L.G.nloc) return fail(h, KSFD_EINVAL, "coarse solve: no buffers for this level");
    // single rank (ksfd_set_mg_coarse refuses a halo transport): the level is the whole grid, its slow extent the global one
    const LUSys Y{ &L.G, &L.P, L.coef, (long long)L.G.sloc, 0, KC_MG };
    if ((rc = lu_assemble(h, S, Y, shift)) || (rc = lu_factor_blocks(h, S, KC_MG, true))) return rc;
    const long long n = S.n;
    const double dn = (double)n;
    {
        // a flagged factorization leaves garbage here that nobody reads: the inversion needs no flag
        Scope sc(h, KC_MG, 8.0 * dn * dn * (2.0 + dn / KSFD_MGC_COLS));
        hipLaunchKernelGGL(k_lu_invert, dim3((unsigned)((n + KSFD_MGC_COLS - 1) / KSFD_MGC_COLS)), dim3(KSFD_BLOCK), 0, h->st,
                           (const double *)S.A, n, (const int *)S.piv, C.inv);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&C.info_h, S.info, sizeof(int), hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    h->n_host_sync++;
    C.factorizations++;
    if (C.info_h) return KSFD_OK;
    S.valid = true;
    S.shift = shift;
    ksfd_ctl::coarse_factors_ready(h->cur);
    *ok = true;
    return KSFD_OK;
}

// x = (shift*I - J_c)^-1 b on level L, both in the level's ghosted SoA layout (distinct vectors): one launch, fixed buffers, no host
// wait -- legal inside the captured part of the cycle
static int mgc_apply(ksfd_handle *h, MGLevel &L, const double *b, double *x)
{
    MGCoarse &C = h->mgc;
    if (!h->cur.mgc_ready) return fail(h, KSFD_EINVAL, "coarse solve without a set-up");
    const int n = (int)C.lu.n;
    const KLUVec V{ L.G.nloc, L.G.plane, L.kv.off };
    {
        Scope sc(h, KC_MG, 8.0 * (double)n * (double)n + 16.0 * (double)n);
        hipLaunchKernelGGL(k_mgc_gemv, dim3((unsigned)((n + KSFD_MGC_ROWS - 1) / KSFD_MGC_ROWS)), dim3(KSFD_BLOCK), 0, h->st,
                           (const double *)C.inv, n, V, b, x);
    }
    HIPCHK(h, hipGetLastError());
    C.solves++;
    return KSFD_OK;
}
