// libksfd_hip.so -- banded direct stage solver for 1-D grids (pc_type 6): assembly of shift*I - J(u) into band storage in the folded
// unknown order, LU factorization and the two sweeps of a solve on the device (kernels in banded.hip.h, indices in banded_plan.h);
// the stage wrapper is the dense solver's (exact_stage in lu_host.hip.h)
// (part of the single translation unit ksfd_hip.hip; included after lu_host.hip.h)
#pragma once

// Checked before anything is allocated or the state is touched
static int banded_guard(ksfd_handle *h)
{
    if (h->G.dim != 1)
        return fail(h, KSFD_EINVAL, "banded solver (pc_type 6): 1-D grids only (this handle has %d dimensions, the band would be thousands wide); "
                                    "use pc_type 2, or pc_type 5 up to KSFD_DIRECT_MAX = %d unknowns", h->G.dim, KSFD_DIRECT_MAX);
    if (h->ring) return fail(h, KSFD_EINVAL, "banded solver (pc_type 6): single rank only (this handle has a halo transport)");
    if ((double)h->G.F * (double)h->G.nloc > 1.0e9 || h->G.F > KSFD_BAND_FMAX)
        return fail(h, KSFD_EINVAL, "banded solver (pc_type 6): %.0f unknowns in blocks of %d are outside its 32-bit column index; use pc_type 2",
                    (double)h->G.F * (double)h->G.nloc, h->G.F);
    return KSFD_OK;
}

static void banded_free(ksfd_handle *h)
{
    BandState &S = h->band;
    void *bufs[] = { S.AB, S.piv, S.info, S.col, S.val, S.z };
    for (void *b : bufs) if (b) hipFree(b);
    S = BandState();
}

template <int NT>
static hipError_t banded_factor_attr(size_t lds)
{
    return hipFuncSetAttribute((const void *)k_band_factor<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

static int banded_alloc(ksfd_handle *h)
{
    BandState &S = h->band;
    if (S.AB) return KSFD_OK;
    const BandPlan B = band_plan(h->G.nloc, h->G.F);
    int64_t nr, nnz;
    ksfd_jacobian_nnz(h, &nr, &nnz);
    bool ok = hipMalloc((void **)&S.AB, sizeof(double) * (size_t)band_size(B)) == hipSuccess;
    ok = ok && hipMalloc((void **)&S.piv, sizeof(int) * (size_t)B.n) == hipSuccess;
    ok = ok && hipMalloc((void **)&S.info, sizeof(int)) == hipSuccess;
    ok = ok && hipMalloc((void **)&S.col, sizeof(long long) * (size_t)nnz) == hipSuccess;
    ok = ok && hipMalloc((void **)&S.val, sizeof(double) * (size_t)nnz) == hipSuccess;
    ok = ok && hipMalloc((void **)&S.z, sizeof(double) * (size_t)B.n) == hipSuccess;
    // one wave up to three fields (no barrier between the phases of a column), four waves above; KSFD_BAND_THREADS: timing knob
    const int nt = env_knobs().band_threads ? env_knobs().band_threads : (B.F <= 3 ? 64 : 256);
    const size_t lds = sizeof(double) * (size_t)band_factor_lds(B);
    ok = ok && (nt == 64 ? banded_factor_attr<64>(lds) : banded_factor_attr<256>(lds)) == hipSuccess;
    if (!ok) {
        hipGetLastError();
        banded_free(h);
        return fail(h, KSFD_ENOMEM, "banded solver: allocation of the %.1f MB of band factors (or of %zu bytes of LDS) failed", 8e-6 * (double)band_size(B), lds);
    }
    S.B = B;
    S.nnz = nnz;
    S.threads = nt;
    return KSFD_OK;
}

// A = shift*I - J at the resident coefficient planes (ensure_coef first), factored in place: P A = L U.  Five launches and one read-back.
static int banded_factor(ksfd_handle *h, double shift)
{
    int rc;
    if ((rc = banded_alloc(h))) return rc;
    BandState &S = h->band;
    const KGeom &G = h->G;
    const BandPlan &B = S.B;
    S.valid = false;
    const int nbp = (int)std::min<long long>((G.nloc + KSFD_BLOCK - 1) / KSFD_BLOCK, 65535);
    {
        Scope sc(h, KC_MISC, 16.0 * (double)S.nnz + 8.0 * (3 + h->P.nlig) * (double)G.nloc);
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_jac_csr<NL>), dim3(nbp), dim3(KSFD_BLOCK), 0, h->st, G, h->P, (const double *)h->coef,
                                                  (long long)h->cfg.n[G.dim - 1], (long long)h->slow0, S.col, S.val));
    }
    HIPCHK(h, hipGetLastError());
    {
        Scope sc(h, KC_MISC, 8.0 * (double)band_size(B));
        HIPCHK(h, hipMemsetAsync(S.AB, 0, sizeof(double) * (size_t)band_size(B), h->st));
    }
    {
        Scope sc(h, KC_MISC, 4.0);
        HIPCHK(h, hipMemsetAsync(S.info, 0, sizeof(int), h->st));
    }
    {
        Scope sc(h, KC_MISC, 32.0 * (double)S.nnz + 16.0 * (double)B.n);
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_band_scatter<NL>), dim3(nbp), dim3(KSFD_BLOCK), 0, h->st, B, (const long long *)S.col,
                                                  (const double *)S.val, shift, S.AB, S.info));
    }
    HIPCHK(h, hipGetLastError());
    {
        // every band entry read once and written once, the pivot indices written
        Scope sc(h, KC_MISC, 16.0 * (double)band_size(B) + 4.0 * (double)B.n);
        const size_t lds = sizeof(double) * (size_t)band_factor_lds(B);
        if (S.threads == 64) hipLaunchKernelGGL((k_band_factor<64>), dim3(1), dim3(64), lds, h->st, B, S.AB, S.piv, S.info);
        else hipLaunchKernelGGL((k_band_factor<256>), dim3(1), dim3(256), lds, h->st, B, S.AB, S.piv, S.info);
    }
    HIPCHK(h, hipGetLastError());
    int info = 0;
    HIPCHK(h, hipMemcpyAsync(&info, S.info, sizeof(int), hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    h->n_host_sync++;
    if (info < 0) return fail(h, KSFD_EINVAL, "banded solve: a Jacobian entry lies outside the band (kl = ku = %d, %lld unknowns)", B.kl, B.n);
    if (info) return fail(h, KSFD_ELINEAR, "banded solve: zero or non-finite pivot in column %d of shift*I - J (shift %.6g, %lld unknowns)", info - 1, shift, B.n);
    S.valid = true;
    S.shift = shift;
    return KSFD_OK;
}

// x = U^-1 L^-1 P b; b and x in the ghosted SoA layout (distinct vectors).  One launch.
static int banded_solve(ksfd_handle *h, const double *b, double *x)
{
    BandState &S = h->band;
    if (!S.valid) return fail(h, KSFD_EINVAL, "banded solve without a factorization");
    const KGeom &G = h->G;
    const BandPlan &B = S.B;
    const KBandVec V{ G.plane, (long long)G.ng * G.inner };
    {
        // L and U band read once, the vector read and written, z written and read
        Scope sc(h, KC_MISC, 8.0 * (double)(2 * B.kl + B.ku + 1) * (double)B.n + 32.0 * (double)B.n);
        hipLaunchKernelGGL(k_band_solve, dim3(1), dim3(KSFD_BAND_SOLVE_T), 0, h->st, B, (const double *)S.AB, (const int *)S.piv, V, b, S.z, x);
    }
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

static int banded_stage(ksfd_handle *h, double shift, const double *b, double *x, const ksfd_step_opts *opts, LinStats *ls)
{
    return exact_stage(h, shift, b, x, opts, ls, banded_solve, "banded");
}
