// libksfd_hip.so -- host side of the spectral preconditioner (kernels and rationale: spectral.hip.h; every shape decision: spec_shape in
// spectral_plan.h).  spec_build turns the planner's answer into device tables, kernel instances and all-to-all lists; spec_apply is a
// sequence of launches through them
// (part of the single translation unit ksfd_hip.hip; included after ops.hip.h)
#pragma once
#include "spectral_plan.h"

static void spec_free(ksfd_handle *h)
{
    SpecState &S = h->spec;
    void *bufs[] = { S.W, S.W2, S.twx, S.twy, S.twz, S.spos, S.skof, S.ytab, S.pairtab, S.lx, S.ly, S.lz };
    for (void *b : bufs) if (b) hipFree(b);
    S = SpecState();
}

template <typename T> static bool spec_upload(T **dev, const std::vector<T> &host)
{
    return hipMalloc((void **)dev, sizeof(T) * host.size()) == hipSuccess &&
           hipMemcpy(*dev, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice) == hipSuccess;
}

// The KSFD_SPEC_* environment knobs, read here and nowhere else: per handle (tests set KSFD_SPEC_SPLIT before they create one), except
// DIAG, FUSE and FUSE3, which are read once per process.
//   DIAG   timing-only diagnostics (wrong results): bit0/1/2 = skip the FFT stages of the rows-fwd / cols / rows-inv kernel
//   FUSE   KFFTPlan.flags of the 2-D kernels; FUSE3: fused edge stages of the y and z kernels (bit 0: first forward stage on the loaded
//          values, bit 1: last inverse stage into the store)
static SpecKnobs spec_knobs()
{
    auto num = [](const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; };
    static const int diag = num("KSFD_SPEC_DIAG", 0), fuse = num("KSFD_SPEC_FUSE", 7), fuse3 = num("KSFD_SPEC_FUSE3", 3);
    SpecKnobs K;
    K.no3d = getenv("KSFD_SPEC_NO3D");
    K.single = getenv("KSFD_SPEC_SINGLE");
    K.transposed = getenv("KSFD_SPEC_TRANSPOSED");
    K.cz = num("KSFD_SPEC_CZ", K.cz); K.pb = num("KSFD_SPEC_PB", K.pb); K.rb = num("KSFD_SPEC_RB", K.rb);
    K.split = num("KSFD_SPEC_SPLIT", 0);
    K.lgw = num("KSFD_SPEC_LGW", -1);
    K.thr_rows = num("KSFD_SPEC_THRR", 0); K.thr_cols = num("KSFD_SPEC_THRC", 0); K.thr_z = num("KSFD_SPEC_THRZ", 0);
    K.diag = diag; K.fuse = fuse; K.fuse3 = fuse3;
    return K;
}

template <bool R3, bool ONEPIECE> static decltype(&k_spec3_z<0, false>) spec_z_instance(int npair)
{
    return npair == 1 ? k_spec3_z<1, R3, ONEPIECE> : npair == 2 ? k_spec3_z<2, R3, ONEPIECE> : k_spec3_z<0, R3, ONEPIECE>;    // 0: run-time pair count
}

// Builds the shape, the kernel instances, the tables and the work arrays if this handle can use the spectral solver; leaves spec.ok =
// false otherwise.
static void spec_build(ksfd_handle *h)
{
    SpecState &S = h->spec;
    SpecShape &Z = S.shape;
    const KGeom &G = h->G;
    const int P = h->size;
    S.ok = false;
    const SpecKnobs K = spec_knobs();
    if (h->ring && (!h->tr || !h->tr->has_alltoall() || (P != 1 && P != 2 && P != 4 && P != 8) || K.single)) return;
    const SpecGrid I = { G.dim, { h->cfg.n[0], h->cfg.n[1], h->cfg.n[2] }, G.F, P, h->rank, h->ring, G.sloc, G.ng };
    SpecTables T;
    if (!spec_shape(I, K, Z, T)) return;
    const bool d3 = Z.dim == 3;
    // the kernel instances, chosen here and nowhere else: R3 = that axis is 3 * 2^k; a column of three chunks is never one piece
    S.k_rows_fwd64 = k_spec_rows_fwd<double>;
    S.k_rows_fwd32 = k_spec_rows_fwd<float>;
    S.k_rows_inv = k_spec_rows_inv;
    if (d3) {
        S.k_y_fwd = Z.py.m == 3 ? k_spec3_y_fwd<true> : k_spec3_y_fwd<false>;
        S.k_y_inv = Z.py.m == 3 ? k_spec3_y_inv<true> : k_spec3_y_inv<false>;
        S.k_z = Z.nch == 3 ? spec_z_instance<true, false>(Z.npair) : Z.pz.m == 3 ? spec_z_instance<true, true>(Z.npair) : spec_z_instance<false, false>(Z.npair);
    } else if (Z.cols_split) S.k_cols_split = Z.py.m == 3 ? k_spec_cols_split<true> : k_spec_cols_split<false>;
    else S.k_cols = Z.npair == 1 ? k_spec_cols<1> : Z.npair == 2 ? k_spec_cols<2> : k_spec_cols<0>;
    const struct { const void *kernel; size_t lds; } limits[] = {
        { (const void *)S.k_rows_fwd64, Z.lds_rows }, { (const void *)S.k_rows_fwd32, Z.lds_rows }, { (const void *)S.k_rows_inv, Z.lds_rows },
        { (const void *)S.k_y_fwd, Z.lds_y3 }, { (const void *)S.k_y_inv, Z.lds_y3 }, { (const void *)S.k_z, Z.lds_z3 },
        { (const void *)S.k_cols_split, Z.lds_cols }, { (const void *)S.k_cols, Z.lds_cols } };
    for (const auto &l : limits)
        if (l.kernel && hipFuncSetAttribute(l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds) != hipSuccess) { hipGetLastError(); return; }
    const KFFTPlan &ps = d3 ? Z.pz : Z.py;                           // the slow axis: its tables feed the symbol stage of the column (z) kernel
    const double *ih2 = h->P.inv_h2;
    const size_t wbytes = sizeof(kcf) * Z.welems;
    if (hipMalloc((void **)&S.W, wbytes) != hipSuccess || (Z.need_w2 && hipMalloc((void **)&S.W2, wbytes) != hipSuccess) ||
        !spec_upload(&S.twx, spec_twiddles(Z.px)) || !spec_upload(&S.twy, spec_twiddles(Z.py)) || (d3 && !spec_upload(&S.twz, spec_twiddles(Z.pz))) ||
        !spec_upload(&S.spos, spec_positions(ps)) || !spec_upload(&S.skof, spec_inverse(spec_positions(ps))) || !spec_upload(&S.pairtab, T.pairtab) ||
        !spec_upload(&S.lx, spec_symbol_table(Z.px.n, ih2[0])) || !spec_upload(&S.ly, spec_symbol_table(Z.py.n, ih2[1])) ||
        (d3 && !spec_upload(&S.lz, spec_symbol_table(Z.pz.n, ih2[2]))) ||
        !spec_upload(&S.ytab, spec_partner_table(ps, spec_symbol_table(ps.n, ih2[Z.dim - 1])))) { hipGetLastError(); spec_free(h); return; }
    kcf *back_s = Z.a2a_back_from_w ? S.W : S.W2, *back_r = Z.a2a_back_from_w ? S.W2 : S.W;
    for (const SpecBlock &b : T.a2a_fwd) { S.a2a_fwd_s.push_back({ b.peer, S.W + b.src, b.bytes }); S.a2a_fwd_r.push_back({ b.peer, S.W2 + b.dst, b.bytes }); }
    for (const SpecBlock &b : T.a2a_back) { S.a2a_back_s.push_back({ b.peer, back_s + b.src, b.bytes }); S.a2a_back_r.push_back({ b.peer, back_r + b.dst, b.bytes }); }
    S.ok = true;
}

// means of rho*G_rho, rho*G_Ul over the frozen coefficient planes (call after op_jcoef, once per step)
static int spec_means(ksfd_handle *h)
{
    SpecState &S = h->spec;
    const KGeom &G = h->G;
    const int nb = (int)std::min<long long>((G.nloc + KSFD_BLOCK - 1) / KSFD_BLOCK, 2048);
    {
        Scope sc(h, KC_SPECTRAL, 8.0 * (2 + h->P.nlig) * (double)G.nloc);
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_spec_means<NL>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, G, (const double *)h->coef, h->part));
    }
    HIPCHK(h, hipGetLastError());
    int rc = reduce_rows(h, 1 + h->P.nlig, nb, 0);
    if (rc) return rc;
    const double ntot = (double)h->cfg.n[0] * (double)h->cfg.n[1] * (double)h->cfg.n[2];
    S.a_rr = h->hres[0] / ntot;
    for (int l = 0; l < h->P.nlig; l++) S.a_rU[l] = h->hres[1 + l] / ntot;
    ksfd_ctl::means_computed(h->cur);
    return KSFD_OK;
}

// z = M^-1 v, M = shift*I - J0 (constant-coefficient part of the frozen Jacobian)
// xadd != NULL: z = xadd + M^-1 v (one Richardson update without a vector pass of its own)
// v32 != NULL: the input is that fp32 copy (F planes of floats, same geometry) instead of v
// guess != NULL (with v): z = sum_j c_j Y_j + M^-1 (v - sum_j c_j b_j), the first sweep from an initial guess in span{Y_j}
struct SpecGuess { int n; const double *Y[3], *b[3]; double c[3]; };

// what one application hands to its launches.  Slab ranks with 3 * 2^j rows (3-D: z planes): the row kernels, and the y kernels in 3-D,
// run once per chunk of 2^j rows (planes), on that chunk's part of the vectors and of the chunk-major work arrays (spec_shape);
// everywhere else nch = 1 and their loops are one launch
struct SpecRun {
    KSpecSym Y;
    KSpecLin ex, add;                // the transform is taken of v + ex; z = add + the result
    KFFTPlan px_f, py_c, px_i, py3, pz3;
    long long goff, rows_off, w_off; // the row kernels address owned rows only; a chunk's rows in a plane (inner = nx in 2-D, nx * ny in 3-D) / in W
    double fn, pn;                   // elements of a vector / bytes of a work array
    const double *v; const float *v32; double *z;
};

static void spec_rows_fwd(ksfd_handle *h, const SpecRun &R)
{
    const SpecState &S = h->spec;
    const SpecShape &Z = S.shape;
    const KGeom &G = h->G;
    Scope sc(h, KC_SPECTRAL, (R.v32 ? 4.0 : 8.0) * R.fn + 8.0 * R.ex.n * R.fn + R.pn, 8.0 * (1 + R.ex.n) * R.fn);      // read v (+ guess vectors) | write W
    const int nt = Z.tile_major ? -Z.ntiles : Z.ntiles;
    for (int c = 0; c < Z.nch; c++) {
        const long long ro = c * R.rows_off;
        kcf *Wf = (Z.tile_major ? S.W2 : S.W) + c * R.w_off;
        KSpecLin exc = R.ex;
        for (int j = 0; j < exc.n; j++) exc.p[j] += ro;
        if (R.v32) hipLaunchKernelGGL(S.k_rows_fwd32, dim3(Z.ntiles, Z.npair), dim3(Z.thr_rows), Z.lds_rows, h->st, R.px_f, Z.nyp, Z.rb, nt, G.F, R.v32 + R.goff + ro, G.plane, Wf, (const kcf *)S.twx, exc);
        else hipLaunchKernelGGL(S.k_rows_fwd64, dim3(Z.ntiles, Z.npair), dim3(Z.thr_rows), Z.lds_rows, h->st, R.px_f, Z.nyp, Z.rb, nt, G.F, R.v + R.goff + ro, G.plane, Wf, (const kcf *)S.twx, exc);
    }
}

// slab ranks, forward: rows (3-D: z planes) of everybody's columns -> whole columns of mine; and back
static int spec_transpose(ksfd_handle *h, const SpecRun &R, bool back)
{
    SpecState &S = h->spec;
    Scope sc(h, KC_HALO, R.pn);
    if (h->tr->alltoall(back ? S.a2a_back_s : S.a2a_fwd_s, back ? S.a2a_back_r : S.a2a_fwd_r, h->st)) return fail(h, KSFD_ECOMM, "spectral all-to-all failed: %s", h->tr->error().c_str());
    return KSFD_OK;
}

static void spec_cols(ksfd_handle *h, const SpecRun &R)
{
    const SpecState &S = h->spec;
    const SpecShape &Z = S.shape;
    // work array in place (split: 2 + (npair + 2) passes; by column: 2 + (2 npair + 1))
    Scope sc(h, KC_SPECTRAL, Z.cols_split == 2 ? (3.0 + 2.0 * Z.npair) * R.pn : Z.cols_split ? (4.0 + Z.npair) * R.pn : 2.0 * R.pn, 0.0);
    const long long pstride = (long long)Z.npair * Z.nxl << Z.lg_pl;
    const kcf *Wt = Z.tile_major ? S.W2 : nullptr;
    const int lg_rb = Z.tile_major ? Z.lg_rb : -1;
    if (!Z.cols_split) {
        hipLaunchKernelGGL(S.k_cols, dim3((unsigned)Z.nblk_cols), dim3(Z.thr_cols), Z.lds_cols, h->st, R.py_c, Z.nxl, Z.lg_pl, pstride, h->ring ? S.W2 : S.W, Wt, lg_rb, (const kcf *)S.twy,
                           (const int4 *)S.pairtab, (const int *)S.spos, (const int *)S.skof, (const float *)S.lx, (const float *)S.ly, (const int2 *)S.ytab, R.Y);
        return;
    }
    // one rank: tiles (W2) -> spectrum (W) -> result (W2); slab ranks: in place in W2, then result into W as scratch
    kcf *spec = h->ring ? S.W2 : S.W, *res = h->ring ? S.W : S.W2;
    for (int phase = 1; phase <= 2; phase++)
        hipLaunchKernelGGL(S.k_cols_split, dim3((unsigned)Z.nblk_cols, (unsigned)Z.npair, Z.cols_split == 2 ? 2u : 1u), dim3(Z.thr_cols), Z.lds_cols, h->st, phase, R.py_c, Z.nxl, Z.lg_pl, pstride, spec,
                           Wt, lg_rb, res, (const kcf *)S.twy, (const int4 *)S.pairtab, (const int *)S.spos, (const int *)S.skof, (const float *)S.lx, (const float *)S.ly, R.Y);
}

static void spec3_y(ksfd_handle *h, const SpecRun &R, bool inv)
{
    const SpecState &S = h->spec;
    const SpecShape &Z = S.shape;
    const KGeom &G = h->G;
    Scope sc(h, KC_SPECTRAL, 2.0 * R.pn, 0.0);
    const int nzc = (int)(G.sloc / Z.nch);                           // planes of a chunk
    const dim3 grid((unsigned)(nzc >> Z.lg_cz), (unsigned)G.nx);
    for (int c = 0; c < Z.nch; c++) {
        if (inv) hipLaunchKernelGGL(S.k_y_inv, grid, dim3(Z.thr_y), Z.lds_y3, h->st, R.py3, (int)G.nx, nzc, Z.lg_cz, Z.npair, (const kcf *)S.W + c * R.w_off, S.W2 + c * R.w_off, (const kcf *)S.twy);
        else hipLaunchKernelGGL(S.k_y_fwd, grid, dim3(Z.thr_y), Z.lds_y3, h->st, R.py3, (int)G.nx, nzc, Z.lg_cz, Z.npair, Z.lg_rb, (const kcf *)S.W2 + c * R.w_off, S.W + c * R.w_off, (const kcf *)S.twy);
    }
}

static void spec3_z(ksfd_handle *h, const SpecRun &R)
{
    const SpecState &S = h->spec;
    const SpecShape &Z = S.shape;
    Scope sc(h, KC_SPECTRAL, 2.0 * R.pn, 0.0);
    const long long ncol = (long long)Z.nxl * Z.py.n, pstride = (long long)Z.npair * ncol << Z.lg_pl;
    hipLaunchKernelGGL(S.k_z, dim3((unsigned)((Z.nent + Z.pb - 1) / Z.pb)), dim3(Z.thr_z), Z.lds_z3, h->st, R.pz3, Z.nent, Z.pb, ncol, Z.lg_pl, pstride, h->ring ? S.W2 : S.W,
                       (const kcf *)S.twz, (const int4 *)S.pairtab, (const int *)S.spos, (const int *)S.skof, (const float *)S.lx, (const float *)S.ly, (const float *)S.lz, (const int2 *)S.ytab, R.Y);
}

static void spec_rows_inv(ksfd_handle *h, const SpecRun &R)
{
    const SpecState &S = h->spec;
    const SpecShape &Z = S.shape;
    const KGeom &G = h->G;
    Scope sc(h, KC_SPECTRAL, R.pn + 8.0 * (1 + R.add.n) * R.fn, 8.0 * (1 + R.add.n) * R.fn);     // read W (+ x / guess vectors) | write z
    const kcf *Wi = (Z.dim == 3 || Z.cols_split) ? S.W2 : S.W;      // 3-D: [chunk][pair][pos_x][z*ny + y], the y inverse's store
    for (int c = 0; c < Z.nch; c++) {
        const long long ro = c * R.rows_off;
        KSpecLin addc = R.add;
        for (int j = 0; j < addc.n; j++) addc.p[j] += ro;
        hipLaunchKernelGGL(S.k_rows_inv, dim3(Z.ntiles, Z.npair), dim3(Z.thr_rows), Z.lds_rows, h->st, R.px_i, Z.nyp, Z.rb, Z.ntiles, G.F, Wi + c * R.w_off, R.z + R.goff + ro, G.plane, (const kcf *)S.twx, addc);
    }
}

static int spec_apply(ksfd_handle *h, double shift, const double *v, double *z, const double *xadd = nullptr, const float *v32 = nullptr, const SpecGuess *guess = nullptr)
{
    SpecState &S = h->spec;
    const SpecShape &Z = S.shape;
    const KGeom &G = h->G;
    if (!S.ok || !h->cur.means_valid) return fail(h, KSFD_EINVAL, "spectral preconditioner not available for this handle");
    SpecRun R;
    memset(&R, 0, sizeof R);
    R.v = v; R.v32 = v32; R.z = z;
    R.Y.nlig = h->P.nlig;
    R.Y.shift = (float)shift; R.Y.a_rr = (float)S.a_rr;
    R.Y.scale = (float)(1.0 / ((double)G.nx * (double)h->cfg.n[1] * (double)h->cfg.n[2]));
    R.Y.den_floor = (float)(0.02 * shift);
    for (int l = 0; l < h->P.nlig; l++) { R.Y.a_rU[l] = (float)S.a_rU[l]; R.Y.s[l] = (float)h->P.lig_s[l]; R.Y.gam[l] = (float)h->P.lig_gamma[l]; R.Y.D[l] = (float)h->P.lig_D[l]; }
    R.goff = (long long)G.ng * G.inner;
    R.rows_off = G.sloc / Z.nch * G.inner;
    R.w_off = (long long)Z.npair * G.nx * Z.nyp;
    if (xadd) { R.add.n = 1; R.add.p[0] = xadd + R.goff; R.add.a[0] = 1.0; }
    if (guess && !v32) {
        for (int j = 0; j < guess->n && j < 3; j++) {
            R.ex.p[R.ex.n] = guess->b[j] + R.goff; R.ex.a[R.ex.n++] = -guess->c[j];
            R.add.p[R.add.n] = guess->Y[j] + R.goff; R.add.a[R.add.n++] = guess->c[j];
        }
    }
    R.px_f = R.px_i = Z.px; R.py_c = R.py3 = Z.py; R.pz3 = Z.pz;
    if (Z.diag & 1) R.px_f.nstage = 0;
    if (Z.diag & 2) R.py_c.nstage = 0;
    if (Z.diag & 4) R.px_i.nstage = 0;
    R.px_f.flags = R.py_c.flags = R.px_i.flags = Z.fuse;
    R.px_f.lgw = R.py_c.lgw = Z.lgw;
    R.py3.flags = R.pz3.flags = Z.fuse3;
    R.fn = (double)G.F * (double)G.nloc; R.pn = 8.0 * Z.npair * (double)G.nloc;
    const bool d3 = Z.dim == 3;
    int rc;
    spec_rows_fwd(h, R);
    if (d3) spec3_y(h, R, false);
    if (h->ring && (rc = spec_transpose(h, R, false))) return rc;
    if (d3) spec3_z(h, R); else spec_cols(h, R);
    if (h->ring && (rc = spec_transpose(h, R, true))) return rc;
    if (d3) spec3_y(h, R, true);
    spec_rows_inv(h, R);
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}
