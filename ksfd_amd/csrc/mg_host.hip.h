// libksfd_hip.so -- host side of the geometric multigrid preconditioner (kernels and rationale: mg.hip.h)
// (part of the single translation unit ksfd_hip.hip, after ops.hip.h: the include list there gives the order)
#pragma once
// exact solve on the level the cycle ends on (lu_host.hip.h, after the dense LU it is built from)
static void mgc_free(ksfd_handle *h);
static int mgc_setup(ksfd_handle *h, MGLevel &L, double shift, bool *ok);
static int mgc_apply(ksfd_handle *h, MGLevel &L, const double *b, double *x);

// level the V cycle ends on: the coarsest one unless ksfd_set_mg_coarse chose a finer one for the exact solve
static inline size_t mg_end(const ksfd_handle *h) { return h->mgc.kind == 1 ? (size_t)h->mgc.level : h->mg.size() - 1; }
// level l keeps fp32 vectors in the cycle with fp32 level vectors (the level of an exact coarse solve stays in fp64, like the coarsest
// level of the Chebyshev cycle)
static inline bool mg_f32(const ksfd_handle *h, size_t l)
{
    return h->mg[l].f32 && !(h->mgc.kind == 1 && l == (size_t)h->mgc.level) && !(h->mgt.level >= 1 && l >= (size_t)h->mgt.level);   // the tail's levels: fp64, in the LDS
}

// The frozen Jacobian action on level L (ops.hip.h: JvpSys, jvp_path).  Level 0 is the handle's grid: booked as its Jacobian actions are,
// and its fp32 coefficient copy is the handle's (made on demand: ensure_coef32 before the first launch).  The levels have no launch of the second-generation 3-D kernel: the strip kernel serves
static JvpSys mg_sys(const ksfd_handle *h, const MGLevel &L)
{
    const bool l0 = &L == &h->mg[0];
    return { &L.G, &L.P, L.coef, l0 ? (coef32_on(h) ? h->coef32 : nullptr) : L.coef32, L.dG, l0 ? KC_JVP : KC_MG };
}
static JvpPath mg_path(const ksfd_handle *h, const MGLevel &L) { const JvpPath p = jvp_path(h, L.G, h->P.nlig, JVP_NX_LEVEL); return p == JP_LDS3D ? JP_STRIP3D : p; }

static void mg_free(ksfd_handle *h)
{
    mgc_free(h);
    h->mgc = MGCoarse();
    h->mgt.level = -1; h->mgt.nlev = 0; h->mgt.lds = 0;      // max_points stays: mg_build plans the tail again
    if (h->mg_graph) { hipGraphExecDestroy(h->mg_graph); h->mg_graph = nullptr; }      // it recorded the buffers freed below
    ksfd_ctl::hierarchy_freed(h->cur);
    for (size_t l = 0; l < h->mg.size(); l++) {
        MGLevel &L = h->mg[l];
        void *bufs[] = { L.dinv, l ? L.coef : nullptr, L.coef32, L.Ad, L.dG, L.pv, L.v64.x, L.v64.b, L.v64.r, L.v64.d, L.v32.x, L.v32.b, L.v32.r, L.v32.d };
        for (void *b : bufs) if (b) hipFree(b);
    }
    h->mg.clear();
    h->mg_ok = false;
}

// one level of `rows` slow units by nx (by ny in 3-D) with the physics P: geometry, buffers, and onto the list.  rep: the whole level
// on every slab rank (rows = the global slow extent): no ghost units, the slow axis wraps in the kernels
static int mg_push_level(ksfd_handle *h, long long nx, long long ny, long long rows, const KPhys &P, bool rep)
{
    const int dim = h->G.dim, nl = h->P.nlig, F = h->G.F;
    const bool l0 = h->mg.empty();
    MGLevel L;
    L.G = h->G; L.G.nx = nx;
    L.rep = rep;
    if (rep) { L.G.ng = 0; L.G.wrap_slow = 1; }
    if (dim == 1) { L.G.nx = rows; L.G.inner = 1; }                      // 1-D: the slab axis is x itself
    else if (dim == 2) { L.G.ny = rows; L.G.inner = nx; } else { L.G.ny = ny; L.G.nz = rows; L.G.inner = nx * ny; }
    L.G.sloc = rows;
    L.G.plane = (rows + 2 * L.G.ng) * L.G.inner; L.G.nloc = rows * L.G.inner;
    L.P = P;
    L.kv.plane = L.G.plane; L.kv.off = (long long)L.G.ng * L.G.inner; L.kv.nloc = L.G.nloc; L.kv.nf = F;
    L.vlen = (int64_t)F * L.G.plane;
    L.nblk = (int)std::min<long long>((L.G.nloc + KSFD_BLOCK - 1) / KSFD_BLOCK, 2048);
    h->mg.push_back(L);                                                  // first: mg_free releases whatever the allocations below leave
    MGLevel &M = h->mg.back();
    if (l0) M.coef = h->coef;
    else if (alloc_d(h, &M.coef, (int64_t)(3 + nl) * M.G.plane) || alloc_d(h, &M.v64.x, M.vlen) || alloc_d(h, &M.v64.b, M.vlen)) return KSFD_ENOMEM;
    if (hipMalloc((void **)&M.dinv, sizeof(float) * (size_t)F * F * M.G.plane) != hipSuccess || alloc_d(h, &M.v64.r, M.vlen) || alloc_d(h, &M.v64.d, M.vlen) ||
        alloc_d(h, &M.Ad, M.vlen) || alloc_d(h, &M.dG, M.G.plane) || alloc_d(h, &M.pv, M.vlen)) return KSFD_ENOMEM;
    double *zero[] = { M.v64.x, M.v64.b, M.v64.r, M.v64.d, M.Ad, M.pv };
    for (double *z : zero) if (z) hipMemsetAsync(z, 0, sizeof(double) * (size_t)M.vlen, h->st);
    return KSFD_OK;
}

// The coarse tail (ksfd_set_mg_tail): which levels run as one workgroup launch, from the stored max_points (mg_tail_plan.h), and the
// dynamic LDS size of the kernel instance this handle launches.  max_points = 0: nothing is touched, no HIP call is made.
static int mg_tail_replan(ksfd_handle *h)
{
    MGTail &M = h->mgt;
    M.level = -1; M.nlev = 0; M.lds = 0;
    if (M.max_points <= 0 || !h->mg_ok) return KSFD_OK;
    std::vector<long long> points;
    std::vector<int> local;
    for (const MGLevel &L : h->mg) {
        points.push_back(L.G.nloc);
        local.push_back((!h->ring || L.rep) && L.G.ng == 0 && L.G.plane == L.G.nloc ? 1 : 0);
    }
    const int end = (int)mg_end(h);
    long long lds = 0;
    const int t = ksfd_ctl::mg_tail_first_level(points.data(), local.data(), end, h->G.F, M.max_points, ksfd_ctl::MG_TAIL_LDS_BUDGET, &lds);
    if (t < 1) return KSFD_OK;
    hipError_t e = hipSuccess;
    NL_DISPATCH(h->P.nlig, e = hipFuncSetAttribute((const void *)k_mg_tail<NL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, KSFD_EHIP, "mg_tail: %lld bytes of dynamic LDS refused: %s", lds, hipGetErrorString(e)); }
    M.level = t; M.nlev = end - t + 1; M.lds = lds;
    return KSFD_OK;
}

static int mg_build(ksfd_handle *h)
{
    const int dim = h->G.dim, nl = h->P.nlig;
    // The level list is the plan's (mg_agglomerate_plan.h: a pure function of the global extents, the rank count and the ring, so every
    // rank builds the same hierarchy; h->mg_agg = 0 gives the plain slab rule).  sloc: this rank's slow units (y rows in 2-D, z planes
    // in 3-D) on a distributed level, the global slow extent on a replicated one
    constexpr int cap = 64;
    ksfd_ctl::MGPlanLevel plan[cap];
    const long long slow = h->G.sloc * h->size;
    const long long nglob[3] = { dim == 1 ? slow : h->G.nx, dim == 2 ? slow : dim == 3 ? h->G.ny : 1, dim == 3 ? slow : 1 };
    const int nplan = ksfd_ctl::mg_agglomerate_plan(dim, nglob, h->size, h->ring ? 1 : 0, h->mg_agg, plan, cap);
    if (nplan < 1) return fail(h, KSFD_EINVAL, "multigrid: the level plan describes no grid");
    if (nplan == cap) return fail(h, KSFD_EINVAL, "multigrid: more than %d levels", cap - 1);
    KPhys P = h->P;
    for (int l = 0; l < nplan; l++) {
        if (l) for (int a = 0; a < 3; a++) { P.inv_h[a] *= 0.5; P.inv_h2[a] *= 0.25; }
        int rc = mg_push_level(h, plan[l].n[0], plan[l].n[1], plan[l].sloc, P, plan[l].rep != 0);
        if (rc) return rc;
    }
    h->mg_ok = h->mg.size() >= 2;
    h->mgc.level = (int)h->mg.size() - 1;
    // fp32 level vectors (mg_vcycle<float>): 2-D, levels the strip kernel serves, never the coarsest one (its many Chebyshev sweeps
    // stay in fp64 with the kernels they have)
    if (h->mg_ok) {
        for (size_t l = 0; l + 1 < h->mg.size(); l++) {
            MGLevel &L = h->mg[l];
            if (L.rep || mg_path(h, L) != JP_STRIP2D) break;                 // replicated levels keep fp64 vectors and planes
            const size_t nb = sizeof(float) * (size_t)L.vlen;
            MGVecs<float> &V = L.v32;
            if (hipMalloc((void **)&V.x, nb) != hipSuccess || hipMalloc((void **)&V.b, nb) != hipSuccess ||
                hipMalloc((void **)&V.r, nb) != hipSuccess || hipMalloc((void **)&V.d, nb) != hipSuccess) { (void)hipGetLastError(); break; }
            for (float *z : { V.x, V.b, V.r, V.d }) hipMemsetAsync(z, 0, nb, h->st);
            if (l > 0 && hipMalloc((void **)&L.coef32, sizeof(float) * (size_t)(3 + nl) * L.G.plane) != hipSuccess) { (void)hipGetLastError(); L.coef32 = nullptr; }
            L.f32 = true;
        }
    }
    return mg_tail_replan(h);
}

// transfer operators for the storage types of the fine and the coarse vector.  fp64 on both sides: 1-D, 2-D or 3-D by the level geometry;
// any other pair exists in 2-D only (levels with fp32 vectors, the fp32 coefficient copy)
// Across the border from the last distributed level Lf to the first replicated one Lc (mg.hip.h: KMGSlow, k_mg_restrict) the restriction
// is a launch (here) and one all-reduce of the whole coarse vector (mg_border_reduce, which the caller runs behind the launch and
// outside the launch's Scope: the all-reduce is booked as communication, once), the prolongation a launch; the coarse side is fp64
static inline bool mg_border(const MGLevel &Lf, const MGLevel &Lc) { return Lc.rep && !Lf.rep; }
// sum over the ranks of the slices the border restriction left in `coarse` (np planes of Lc); a no-op anywhere but at the border
static int mg_border_reduce(ksfd_handle *h, const MGLevel &Lf, const MGLevel &Lc, int np, double *coarse)
{
    if (!mg_border(Lf, Lc)) return KSFD_OK;
    Scope sc(h, KC_HALO, 8.0 * np * (double)Lc.G.plane);
    if (h->tr->allreduce_vec(coarse, (long long)np * Lc.G.plane, h->st)) return fail(h, KSFD_ECOMM, "allreduce failed: %s", h->tr->error().c_str());
    return KSFD_OK;
}
template <typename T> static int mg_border_reduce(ksfd_handle *h, const MGLevel &Lf, const MGLevel &Lc, int, T *)
{
    return mg_border(Lf, Lc) ? fail(h, KSFD_EINVAL, "multigrid: a replicated level has fp64 vectors") : KSFD_OK;
}
// the slow axis of the transfers between Lf and Lc on this rank (mg.hip.h: KMGSlow).  Lc.G.sloc is the slow extent of the coarse array
// on either side of the border: half the rank's fine units, or the whole replicated level
static KMGSlow mg_slow(const ksfd_handle *h, const MGLevel &Lf, const MGLevel &Lc, bool restriction)
{
    const bool border = mg_border(Lf, Lc);
    const long long u0f = border ? (long long)h->rank * Lf.G.sloc : 0;       // first fine slow unit of this rank's slab
    // across the border (the kernels' BORDER instances) the fine side has ghost units (no wrap) and the coarse side is whole (wrap)
    return { Lf.G.sloc, restriction ? u0f / 2 : u0f, Lc.G.sloc, border ? (restriction ? 0 : 1) : (int)Lf.G.wrap_slow };
}
// what no transfer exists for
template <typename TF, typename TK>
static int mg_transfer_refused(ksfd_handle *h, const MGLevel &Lf, const MGLevel &Lc)
{
    constexpr bool f64 = std::is_same<TF, double>::value && std::is_same<TK, double>::value;
    if (mg_border(Lf, Lc) && !std::is_same<TK, double>::value) return fail(h, KSFD_EINVAL, "multigrid: a replicated level has fp64 vectors");
    if (!f64 && Lf.G.dim != 2) return fail(h, KSFD_EINVAL, "multigrid: fp32 level vectors exist in 2-D only");
    if (mg_border(Lf, Lc) && Lf.G.dim == 1) return fail(h, KSFD_EINVAL, "multigrid: no replicated levels on a 1-D grid");
    return KSFD_OK;
}
template <typename TF, typename TK>
static int mg_launch_restrict(ksfd_handle *h, MGLevel &Lf, MGLevel &Lc, int np, const TF *fine, TK *coarse)
{
    constexpr bool f64 = std::is_same<TF, double>::value && std::is_same<TK, double>::value;
    if (int rc = mg_transfer_refused<TF, TK>(h, Lf, Lc)) return rc;
    const KMGSlow Z = mg_slow(h, Lf, Lc, true);
    auto launch = [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(point_blocks(Lc.G)), dim3(KSFD_BLOCK), 0, h->st, np, Lf.G.nx, Lf.G.ny, Z,
                               fine, Lf.G.plane, Lf.kv.off, coarse, Lc.G.plane, Lc.kv.off);
        };
        if constexpr (D > 1 && std::is_same<TK, double>::value) if (mg_border(Lf, Lc)) return go(k_mg_restrict<D, true, TF, TK>);
        go(k_mg_restrict<D, false, TF, TK>);
    };
    if (Lf.G.dim == 2) launch(std::integral_constant<int, 2>());
    if constexpr (f64) {
        if (Lf.G.dim == 1) launch(std::integral_constant<int, 1>());
        if (Lf.G.dim == 3) launch(std::integral_constant<int, 3>());
    }
    return KSFD_OK;
}
template <typename TK, typename TF>
static int mg_launch_prolong(ksfd_handle *h, MGLevel &Lf, MGLevel &Lc, int np, const TK *coarse, TF *fine)
{
    constexpr bool f64 = std::is_same<TF, double>::value && std::is_same<TK, double>::value;
    if (int rc = mg_transfer_refused<TF, TK>(h, Lf, Lc)) return rc;
    const KMGSlow Z = mg_slow(h, Lf, Lc, false);
    auto launch = [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(point_blocks(Lf.G)), dim3(KSFD_BLOCK), 0, h->st, np, Lf.G.nx, Lf.G.ny, Z,
                               coarse, Lc.G.plane, Lc.kv.off, fine, Lf.G.plane, Lf.kv.off);
        };
        if constexpr (D > 1 && std::is_same<TK, double>::value) if (mg_border(Lf, Lc)) return go(k_mg_prolong_add<D, true, TK, TF>);
        go(k_mg_prolong_add<D, false, TK, TF>);
    };
    if (Lf.G.dim == 2) launch(std::integral_constant<int, 2>());
    if constexpr (f64) {
        if (Lf.G.dim == 1) launch(std::integral_constant<int, 1>());
        if (Lf.G.dim == 3) launch(std::integral_constant<int, 3>());
    }
    return KSFD_OK;
}

// ghost rows of a level vector (np field planes) from the ring neighbours.  An fp32 vector travels through the double-typed transport as
// half as many doubles (nx is even on the levels that have one).  A replicated level has no ghost rows
template <typename T>
static int mg_halo(ksfd_handle *h, MGLevel &L, T *v, int np)
{
    if (!h->ring || L.rep) return KSFD_OK;
    const long long scale = sizeof(double) / sizeof(T);
    Scope sc(h, KC_HALO, 4.0 * sizeof(T) * np * (double)L.G.inner * 2.0);
    if (h->tr->exchange(reinterpret_cast<double *>(v), np, L.G.plane / scale, L.G.inner / scale, L.G.sloc, L.G.ng, h->st)) return fail(h, KSFD_ECOMM, "halo exchange failed: %s", h->tr->error().c_str());
    return KSFD_OK;
}

// smoother algebra in the epilogue of the Jacobian action: the 2-D strip kernel and the generic kernel have it
static bool mg_can_fuse(const ksfd_handle *h, const MGLevel &L) { return h->tune.mg_fuse && mg_path(h, L) != JP_STRIP3D; }

// Which coefficient planes the strip kernel reads on the level of Y when the level vectors are stored in T.  fp64 vectors: the fp32 copy
// on level 0 only (the V cycle is a preconditioner: see poly_apply; the coarse levels keep their fp64 planes).  fp32 vectors: the fp32
// copy on every level that has one.  NULL: the fp64 planes
template <typename T>
static const float *mg_strip_coef32(const JvpSys &Y) { return (std::is_same<T, float>::value || Y.cls == KC_JVP) ? Y.coef32 : nullptr; }

// out = J v | shift v - J v | yadd - (shift v - J v) on level L, vectors stored in T (float: levels of the 2-D strip kernel only)
// sm != NULL: modes 5 / 6, smoother algebra in the epilogue (2-D strip kernel and generic kernel only: see mg_can_fuse)
template <typename T>
static int mg_op(ksfd_handle *h, MGLevel &L, const T *v, int mode, double shift, T *out, const T *yadd, const KSmoothT<T> *sm = nullptr)
{
    const KGeom &G = L.G;
    if (h->ring) { int rch = mg_halo(h, L, const_cast<T *>(v), G.F); if (rch) return rch; }
    const JvpSys Y = mg_sys(h, L);
    // path: fp32 vectors exist only where mg_build found the 2-D strip kernel, the one kernel that takes them; the 3-D strip kernel and
    // the generic kernel are reached with fp64 vectors alone
    const JvpPath path = std::is_same<T, float>::value ? JP_STRIP2D : mg_path(h, L);
    const float *c32 = path == JP_STRIP2D ? mg_strip_coef32<T>(Y) : nullptr;
    // bytes per point: coefficient planes, v and per mode 1: out; 2: yadd, out; 5: yadd, r, d; 6: rr, x in and out; Dinv in modes 5 and 6;
    // a mode 6 that writes the fp64 result (x64) stores 8 bytes in place of sizeof(T)
    const double s = sizeof(T);
    const double by = ((c32 ? 4.0 : 8.0) * (3 + h->P.nlig) + s * G.F * (1 + (mode == 1 ? 1 : mode == 2 ? 2 : 3)) + (mode >= 5 ? 4.0 * G.F * G.F : 0.0) +
                       ((mode == 6 && sm && sm->x64) ? (8.0 - s) * G.F : 0.0)) * (double)G.nloc;
    if (path == JP_STRIP2D) {
        const KStrips K = strips_for(G, h->tune.yseg_jvp, 4096);       // the levels do not follow KSFD_WAVES_JVP
        Scope sc(h, Y.cls, by);
        auto launch = [&](auto *C) { sm ? jvp2d_launch<true>(h, Y, K, C, v, mode, shift, out, yadd, 0.0, 0.0, *sm, nullptr) : jvp2d_launch<false>(h, Y, K, C, v, mode, shift, out, yadd, 0.0, 0.0, KSmooth{}, nullptr); };
        if (c32) launch(c32); else launch(Y.coef);
    } else if constexpr (std::is_same<T, double>::value) {
        Scope sc(h, Y.cls, by + 8.0 * G.plane);
        dg_pass(h, Y, v, -1);
        if (path == JP_STRIP3D) jvp3d_launch<double>(h, Y, k3d_for(G, 4, 0, h->tune.zseg, 1024), v, mode, shift, out, yadd, 0.0, 0.0, nullptr);
        else jvpgen_launch(h, Y, plane_blocks(G), v, mode, shift, out, yadd, 0.0, 0.0, sm ? *sm : KSmooth{});
    }
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

static int mg_norm(ksfd_handle *h, MGLevel &L, const double *v, double *nrm)
{
    const bool v2 = (L.G.nloc % 2 == 0);
    const int nb = v2 ? (L.nblk + 1) / 2 : L.nblk;
    {
        Scope sc(h, KC_MG, 8.0 * L.vlen);
        if (v2) hipLaunchKernelGGL((k_multidot<4, 2>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, L.kv, v, v, L.vlen, 0, h->part);
        else hipLaunchKernelGGL((k_multidot<4, 1>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, L.kv, v, v, L.vlen, 0, h->part);
    }
    HIPCHK(h, hipGetLastError());
    int rc = reduce_rows(h, 1, nb, 0, L.rep);                 // a replicated level: the local sum is the whole one
    if (rc) return rc;
    *nrm = sqrt(h->hres[0]);
    return KSFD_OK;
}

// restrict coefficient planes down the hierarchy (once per frozen state)
static int mg_restrict_coefs(ksfd_handle *h)
{
    const int np = 3 + h->P.nlig;
    int rc;
    for (size_t l = 0; l + 1 < h->mg.size(); l++) {
        MGLevel &Lf = h->mg[l], &Lc = h->mg[l + 1];
        {
            Scope sc(h, KC_MG, 8.0 * np * (Lf.G.nloc + Lc.G.nloc));
            if ((rc = mg_launch_restrict(h, Lf, Lc, np, (const double *)Lf.coef, Lc.coef))) return rc;
        }
        if ((rc = mg_border_reduce(h, Lf, Lc, np, Lc.coef))) return rc;
        if ((rc = mg_halo(h, Lc, Lc.coef, np))) return rc;       // fine ghosts were valid; now the coarse ones are too
        if (Lc.coef32) {
            // the fp32 cycle reads an fp32 copy (the same full weighting of the fine fp64 planes, rounded once)
            {
                Scope sc(h, KC_MG, np * (8.0 * Lf.G.nloc + 4.0 * Lc.G.nloc));
                if ((rc = mg_launch_restrict(h, Lf, Lc, np, (const double *)Lf.coef, Lc.coef32))) return rc;
            }
            if ((rc = mg_halo(h, Lc, Lc.coef32, np))) return rc;
        }
    }
    HIPCHK(h, hipGetLastError());
    ksfd_ctl::coarse_planes_restricted(h->cur);
    return KSFD_OK;
}

// z = scale * Dinv r on the owned points of level L (z2, rcopy: k_dinv_apply); vectors in the level's ghosted layout, bytes = what the launch moves
template <typename TR, typename TZ>
static void mg_dinv_apply(ksfd_handle *h, MGLevel &L, double bytes, const TR *r, double scale, TZ *z, TZ *z2 = nullptr, TZ *rcopy = nullptr)
{
    const long long off = L.kv.off;     // owned rows start here inside a (ghosted) plane
    Scope sc(h, KC_MG, bytes);
    NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_dinv_apply<NL, TR, TZ>), dim3(point_blocks(L.G)), dim3(KSFD_BLOCK), 0, h->st, L.G.nloc, L.G.plane, (const float *)(L.dinv + off), r + off, scale, z + off, z2 ? z2 + off : (TZ *)nullptr, rcopy ? rcopy + off : (TZ *)nullptr));
}

// the next set-up starts the power iteration of every level cold, from the hash fill (a checkpoint save and restore, so that replays are
// bitwise; the test entries, so that what they return does not depend on the steps before)
static void mg_setup_cold(ksfd_handle *h) { for (MGLevel &L : h->mg) L.pv_norm = 0.0; }

// block-diagonal inverses and Chebyshev upper bounds for this shift
static int mg_setup_shift(ksfd_handle *h, double shift)
{
    int rc;
    const size_t end = mg_end(h);           // levels below it are not part of the cycle
    for (size_t l = 0; l <= end; l++) {
        MGLevel &L = h->mg[l];
        const int F = L.G.F;
        int nb = point_blocks(L.G);
        if (l == end && h->mgc.kind == 1) {
            // exact solve: no smoother on this level, so no block diagonal, power iteration or ratio estimate -- unless the
            // factorization is flagged, then this set-up runs the Chebyshev solve here like the default cycle on its coarsest level
            bool ok = false;
            if ((rc = mgc_setup(h, L, shift, &ok))) return rc;
            if (ok) break;
            h->mgc.fallbacks++;
        }
        {
            Scope sc(h, KC_MG, 8.0 * (3 + h->P.nlig + F * F) * L.G.nloc);
            NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_blockdiag_inv<NL>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, L.G, L.P, (const double *)L.coef, shift, L.dinv));
        }
        HIPCHK(h, hipGetLastError());
        // power iteration on Dinv*A: v and w = Dinv A v / |v| alternate between L.pv and L.v64.r, A v in L.Ad.  The vector is kept
        // from one set-up to the next (L.pv): the shift and the frozen state move a little from step to step and the dominant
        // vector with them, so a warm start needs 2-3 iterations where the cold one from a hash fill takes mg_power_its
        // (4096^2 x 3 fields: 9.4 -> 2.9 ms of set-up per step).
        double *v = L.pv, *w = L.v64.r;
        double nv = L.pv_norm, lam = 2.0, lam_prev = 0.0;
        const bool warm = nv > 0.0 && h->tune.mg_warm_power;
        if (!warm) {
            hipLaunchKernelGGL(k_hash_fill, dim3(nb), dim3(KSFD_BLOCK), 0, h->st, (long long)L.vlen, v);
            if ((rc = mg_norm(h, L, v, &nv))) return rc;
        }
        const int its = warm ? std::min(h->mg_power_its, 3) : h->mg_power_its;
        for (int it = 0; it < its; it++) {
            if (!(nv > 0.0) || nv != nv) break;
            if ((rc = mg_op<double>(h, L, v, 1, shift, L.Ad, nullptr))) return rc;
            mg_dinv_apply(h, L, 8.0 * (2 * F + 0.5 * F * F) * L.G.nloc, (const double *)L.Ad, 1.0 / nv, w);
            double nw;
            if ((rc = mg_norm(h, L, w, &nw))) return rc;
            if (!(nw > 0.0)) break;
            lam_prev = lam; lam = nw;                              // |Dinv A v| / |v|
            std::swap(v, w); nv = nw;
            if (warm && it >= 1 && fabs(lam - lam_prev) <= 0.01 * lam) break;
        }
        if (v != L.pv) HIPCHK(h, hipMemcpyAsync(L.pv, v, sizeof(double) * (size_t)L.vlen, hipMemcpyDeviceToDevice, h->st));
        L.pv_norm = (nv > 0.0 && nv == nv) ? nv : 0.0;
        L.lam_max = 1.15 * lam;
        if (l == end) {
            int nbr = (int)std::min<long long>((L.G.nloc + KSFD_BLOCK - 1) / KSFD_BLOCK, 256);
            hipLaunchKernelGGL(k_ratio_est, dim3(nbr), dim3(KSFD_BLOCK), 0, h->st, (long long)L.G.nloc, (const float *)(L.dinv + L.kv.off), shift, h->part);
            if ((rc = reduce_rows(h, 1, nbr, 1, L.rep))) return rc;
            L.ratio = std::max(30.0, 1.5 * L.lam_max * h->hres[0]);
        }
    }
    ksfd_ctl::shift_setup_done(h->cur, shift);
    return KSFD_OK;
}

// Chebyshev iteration on the eigen-interval [lam_max/ratio, lam_max] in the "direction" form: d_0 = Dinv r_0 / theta, then
// d_{k+1} = c1 d_k + c2 Dinv r with c1 = rho_{k+1} rho_k, c2 = 2 rho_{k+1} / delta, rho_0 = 1/sig1, rho_{k+1} = 1/(2 sig1 - rho_k)
struct MGCheb {
    double theta, delta, sig1, rho0, rhon;                      // rhon = rho_1
    double next(double rho) const { return 1.0 / (2.0 * sig1 - rho); }
};
static inline MGCheb mg_cheb(double lam_max, double ratio)
{
    const double lmax = lam_max, lmin = lmax / ratio;
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sig1 = theta / delta;
    MGCheb C = { theta, delta, sig1, 1.0 / sig1, 0.0 };
    C.rhon = C.next(C.rho0);
    return C;
}

// The V(2,2) smoother pair with the algebra in the Jacobian-action epilogues (modes 5 and 6, KSmoothT), level vectors stored in T: 2 launches
// instead of 3 (zero guess) or 4 (correction), and the residual / A d round trips through memory disappear.
//   zero guess:  d0 = Dinv b / theta, then x = d0 + d1 in the epilogue of A d0 (mode 6)
//   correction:  r = b - A x and d0 = Dinv r / theta in one launch (mode 5), x += d0 + d1 in the next (mode 6)
// Level 0 of the fp32 cycle works on the caller's fp64 vectors: b64 (zero guess) is the right-hand side, read once, k_dinv_apply leaves its
// copy of type T in b; x64: the last kernel writes the result there in fp64 instead of back to x
template <typename T>
static int mg_smooth_fused(ksfd_handle *h, MGLevel &L, double shift, const T *b, T *x, bool zero_init, double ratio, const double *b64 = nullptr, double *x64 = nullptr)
{
    int rc;
    const int F = L.G.F;
    MGVecs<T> &V = L.vecs<T>();
    const MGCheb C = mg_cheb(L.lam_max, ratio);
    KSmoothT<T> S = KSmoothT<T>{};
    S.dinv = L.dinv; S.x = x; S.c1 = C.rhon * C.rho0; S.c2 = 2.0 * C.rhon / C.delta;
    if (zero_init) {
        const double by = ((b64 ? 8.0 + sizeof(T) : sizeof(T)) * F + sizeof(T) * F + 4.0 * F * F) * (double)L.G.nloc;
        if (b64) mg_dinv_apply(h, L, by, b64, 1.0 / C.theta, V.d, (T *)nullptr, const_cast<T *>(b));
        else mg_dinv_apply(h, L, by, b, 1.0 / C.theta, V.d);
        S.rr = b; S.x_has_d = 1;
    } else {
        S.out2 = V.d; S.scale = 1.0 / C.theta;
        if ((rc = mg_op<T>(h, L, x, 5, shift, V.r, b, &S))) return rc;
        S.rr = V.r; S.x_has_d = 0;
    }
    S.x64 = x64;
    return mg_op<T>(h, L, V.d, 6, shift, nullptr, nullptr, &S);
}

// Chebyshev smoothing of A x = b on level L with Dinv; nu sweeps; eigen-interval [lmax/ratio, lmax]
static int mg_smooth(ksfd_handle *h, MGLevel &L, double shift, const double *b, double *x, int nu, bool zero_init, double ratio)
{
    // Chebyshev iteration in the "direction" form:  d_0 = Dinv r_0 / theta ; x += d_k ; r -= A d_k ;
    // d_{k+1} = c1 d_k + c2 Dinv r.   nu sweeps = nu updates of x = nu-1 operator applications (+1 for a nonzero guess).
    // Fusions: a zero guess writes x = d_0 directly; the last sweep folds "x += d_old + d_new" into one kernel.
    if (nu == 2 && mg_can_fuse(h, L)) return mg_smooth_fused(h, L, shift, b, x, zero_init, ratio);    // the default V(2,2) sweeps
    int rc;
    const int F = L.G.F;
    const int nb = point_blocks(L.G);
    const MGCheb C = mg_cheb(L.lam_max, ratio);
    const long long off = L.kv.off;     // owned rows start here inside a (ghosted) plane
    double *const r = L.v64.r, *const d = L.v64.d;
    const double *res = b;
    if (!zero_init) {
        if ((rc = mg_op(h, L, x, 2, shift, r, b))) return rc;        // r = b - A x
        res = r;
    }
    mg_dinv_apply(h, L, 8.0 * ((zero_init ? 3 : 2) * F + 0.5 * F * F) * L.G.nloc, res, 1.0 / C.theta, d, zero_init ? x : (double *)nullptr);
    bool x_has_d = zero_init;          // x == d_0 already
    double rho = C.rho0;
    for (int k = 1; k < nu; k++) {
        if ((rc = mg_op<double>(h, L, d, 1, shift, L.Ad, nullptr))) return rc;
        const double rhon = C.next(rho);
        const double *rsrc = (zero_init && k == 1) ? b : r;             // first sweep from a zero guess: r_0 = b, never copied
        if (k == nu - 1) {
            Scope sc(h, KC_MG, 8.0 * (5 * F + 0.5 * F * F) * L.G.nloc);
            NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_cheb_last<NL>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, L.G.nloc, L.G.plane, (const float *)(L.dinv + off), x + off, rsrc + off, (const double *)(d + off), (const double *)(L.Ad + off), rhon * rho, 2.0 * rhon / C.delta, x_has_d ? 1 : 0));
            x_has_d = true;
        } else {
            if (rsrc != r) HIPCHK(h, hipMemcpyAsync(r, b, sizeof(double) * (size_t)L.vlen, hipMemcpyDeviceToDevice, h->st));
            if (x_has_d && k == 1) { /* x already holds d_0: the step kernel adds d to x, so undo by starting x at 0 */
                HIPCHK(h, hipMemsetAsync(x, 0, sizeof(double) * (size_t)L.vlen, h->st));
            }
            Scope sc(h, KC_MG, 8.0 * (7 * F + 0.5 * F * F) * L.G.nloc);
            NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_cheb_step<NL>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, L.G.nloc, L.G.plane, (const float *)(L.dinv + off), x + off, r + off, d + off, (const double *)(L.Ad + off), rhon * rho, 2.0 * rhon / C.delta));
            x_has_d = false;
        }
        rho = rhon;
    }
    if (!x_has_d) {
        // x += d (only reached when nu == 1 with a nonzero guess, or after k_cheb_step sweeps)
        const double *xs[2] = { x, d };
        KLin LL;
        for (int t = 0; t < 6; t++) { LL.x[t] = t < 2 ? xs[t] : nullptr; LL.a[t] = t < 2 ? 1.0 : 0.0; }
        Scope sc(h, KC_MG, 24.0 * L.vlen);
        hipLaunchKernelGGL((k_lincomb<2, 1>), dim3(L.nblk, F), dim3(KSFD_BLOCK), 0, h->st, L.kv, LL, x);
    }
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

template <typename T>
static int mg_vcycle(ksfd_handle *h, size_t l, double shift, const T *b, T *x, const double *b64 = nullptr, double *x64 = nullptr);

// Chebyshev sweeps of the coarse solve on the level the cycle ends on: over the whole spectrum, enough for the reduction mg_coarse_tol
static int mg_coarse_sweeps(const ksfd_handle *h, const MGLevel &L)
{
    const int sweeps = (int)ceil(0.5 * sqrt(L.ratio) * log(2.0 / h->mg_coarse_tol));
    return std::min(std::max(sweeps, 4), h->mg_ncoarse);
}

// The tail of the cycle in ONE launch (k_mg_tail in mg.hip.h; ksfd_set_mg_tail): x = mg_vcycle<double>(t) b for the first tail level
// t = h->mgt.level, b and x the fp64 vectors of that level (whole, no ghost units).  By-value level descriptors from what mg_setup_shift
// left on the levels (dinv, lam_max, ratio) and the handle's smoothing parameters; one node of the captured graph on graph handles.
// Booked under KC_MG with the bytes the launch moves through global memory: per level the coefficient planes and the fp32 blocks once,
// plus b in and x out -- everything else stays in the LDS.
static double mg_tail_bytes(const ksfd_handle *h)
{
    const int F = h->G.F;
    double by = 0.0;
    for (int q = 0; q < h->mgt.nlev; q++) by += (8.0 * (3 + h->P.nlig) + 4.0 * F * F) * (double)h->mg[h->mgt.level + q].G.nloc;
    return by + 16.0 * F * (double)h->mg[h->mgt.level].G.nloc;
}
static int mg_tail_apply(ksfd_handle *h, double shift, const double *b, double *x)
{
    const MGTail &M = h->mgt;
    if (M.level < 1 || M.nlev < 1 || M.nlev > ksfd_ctl::MG_TAIL_MAX_LEVELS || (size_t)(M.level + M.nlev) != mg_end(h) + 1)
        return fail(h, KSFD_EINVAL, "mg_tail: this handle has no tail planned");
    KMGTail T;
    memset(&T, 0, sizeof T);
    T.nlev = M.nlev; T.dim = h->G.dim; T.shift = shift;
    long long lds = 0;
    for (int q = 0; q < M.nlev; q++) {
        const MGLevel &L = h->mg[M.level + q];
        const bool last = q == M.nlev - 1;
        // what the kernel's indexing rests on: a whole level with wrapped indices, few enough points for the threads' point loops
        if (L.G.ng != 0 || L.G.plane != L.G.nloc || L.G.nloc > ksfd_ctl::mg_tail_max_points(L.G.F) || !L.coef || !L.dinv)
            return fail(h, KSFD_EINVAL, "mg_tail: level %d is not a whole local level", M.level + q);
        KMGTailLevel &D = T.L[q];
        D.coef = L.coef; D.dinv = L.dinv;
        D.n[0] = (int)L.G.nx; D.n[1] = L.G.dim >= 2 ? (int)L.G.ny : 1; D.n[2] = L.G.dim >= 3 ? (int)L.G.nz : 1;
        D.np = (int)L.G.nloc;
        if ((long long)D.n[0] * D.n[1] * D.n[2] != L.G.nloc) return fail(h, KSFD_EINVAL, "mg_tail: level %d: extents and point count disagree", M.level + q);
        D.sweeps = last ? mg_coarse_sweeps(h, L) : h->mg_nu;
        const MGCheb C = mg_cheb(L.lam_max, last ? L.ratio : h->mg_ratio);
        D.theta = C.theta; D.delta = C.delta; D.sig1 = C.sig1; D.rho0 = C.rho0;
        for (int a = 0; a < 3; a++) { D.inv_h[a] = L.P.inv_h[a]; D.inv_h2[a] = L.P.inv_h2[a]; }
        lds += ksfd_ctl::mg_tail_level_bytes(L.G.nloc, L.G.F);
    }
    if (lds != M.lds || lds > ksfd_ctl::MG_TAIL_LDS_BUDGET) return fail(h, KSFD_EINVAL, "mg_tail: the levels need %lld bytes of LDS, the plan has %lld", lds, M.lds);
    {
        Scope sc(h, KC_MG, mg_tail_bytes(h));
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_mg_tail<NL>), dim3(1), dim3(ksfd_ctl::MG_TAIL_THREADS), (size_t)lds, h->st, T, h->mg[M.level].P, b, x));
    }
    HIPCHK(h, hipGetLastError());
    h->mgt.launches++;
    return KSFD_OK;
}

// coarse-grid correction of level l, vectors stored in T and those of level l + 1 in TC: restrict r, recurse, prolong-add into x
template <typename T, typename TC>
static int mg_coarse_correction_in(ksfd_handle *h, size_t l, double shift, T *x)
{
    int rc;
    MGLevel &L = h->mg[l], &Lc = h->mg[l + 1];
    MGVecs<T> &V = L.vecs<T>();
    MGVecs<TC> &Vc = Lc.vecs<TC>();
    const int F = L.G.F;
    const double sf = sizeof(T), sk = sizeof(TC);
    if ((rc = mg_halo(h, L, V.r, F))) return rc;                      // restriction reads fine rows -1 and sloc
    {
        Scope sc(h, KC_MG, F * (sf * L.G.nloc + sk * Lc.G.nloc));
        if ((rc = mg_launch_restrict(h, L, Lc, F, (const T *)V.r, Vc.b))) return rc;
    }
    if ((rc = mg_border_reduce(h, L, Lc, F, Vc.b))) return rc;
    // the rest of the cycle in one launch where the tail begins (its levels are fp64: mg_f32)
    if constexpr (std::is_same<TC, double>::value) rc = (int)l + 1 == h->mgt.level ? mg_tail_apply(h, shift, Vc.b, Vc.x) : mg_vcycle<TC>(h, l + 1, shift, Vc.b, Vc.x);
    else rc = mg_vcycle<TC>(h, l + 1, shift, Vc.b, Vc.x);
    if (rc) return rc;
    if ((rc = mg_halo(h, Lc, Vc.x, F))) return rc;                    // prolongation reads coarse row sloc_c
    {
        Scope sc(h, KC_MG, F * (2.0 * sf * L.G.nloc + sk * Lc.G.nloc));
        if ((rc = mg_launch_prolong(h, L, Lc, F, (const TC *)Vc.x, x))) return rc;
    }
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}
// ... in the storage type of the next level: below fp32 vectors it keeps fp32 ones where it can (mg_f32) and the transfer kernels convert
// at the border to fp64; below fp64 vectors everything is fp64
template <typename T>
static int mg_coarse_correction(ksfd_handle *h, size_t l, double shift, T *x)
{
    if constexpr (std::is_same<T, float>::value) if (mg_f32(h, l + 1)) return mg_coarse_correction_in<T, float>(h, l, shift, x);
    return mg_coarse_correction_in<T, double>(h, l, shift, x);
}

// everything below level 0 touches only fixed buffers: capture it once per shift into a hipGraph and replay it (a V cycle has ~15
// launches per level; on small grids they are pure launch latency).  body = the coarse-grid correction of level 0 in the precision in use.
template <typename Body>
static int mg_coarse_graph(ksfd_handle *h, double shift, const void *xkey, bool f32, Body body)
{
    int rc;
    if (!h->mg_graph || !ksfd_ctl::graph_current(h->cur, shift, xkey, f32)) {
        if (h->mg_graph) { hipGraphExecDestroy(h->mg_graph); h->mg_graph = nullptr; }
        hipGraph_t g = nullptr;
        const double b0 = h->bytes_acc;
        const int32_t s0 = h->mgc.solves;
        const int64_t t0 = h->mgt.launches;
        HIPCHK(h, hipStreamBeginCapture(h->st, hipStreamCaptureModeThreadLocal));
        h->capturing = true;
        rc = body();
        h->capturing = false;
        hipError_t e = hipStreamEndCapture(h->st, &g);
        if (rc) { if (g) hipGraphDestroy(g); return rc; }
        if (e != hipSuccess || !g) return fail(h, KSFD_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        e = hipGraphInstantiate(&h->mg_graph, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (e != hipSuccess) { h->mg_graph = nullptr; return fail(h, KSFD_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
        h->mg_graph_bytes = h->bytes_acc - b0;
        h->bytes_acc = b0;
        h->mgc.graph_solves = h->mgc.solves - s0;
        h->mgc.solves = s0;
        h->mgt.graph_launches = h->mgt.launches - t0;
        h->mgt.launches = t0;
        ksfd_ctl::graph_captured(h->cur, shift, xkey, f32);
    }
    Scope sc(h, KC_MG, h->mg_graph_bytes);
    HIPCHK(h, hipGraphLaunch(h->mg_graph, h->st));
    h->mgc.solves += h->mgc.graph_solves;
    h->mgt.launches += h->mgt.graph_launches;
    return KSFD_OK;
}

// ------------------------------------------------------------------------------------------------
// Level l of the V cycle, level vectors (x, b, r, d) stored in T; the arithmetic inside the kernels is fp64 either way.
// Why fp32 LEVEL VECTORS are legitimate: a V cycle is a preconditioner: GMRES sees the true fp64 residual of the real system whatever
// the cycle returns, and the cycle is bandwidth-bound -- at 4096^2 x 3 fields an iteration moves ~82 planes of 134 MB through level 0
// alone, two thirds of them level vectors.  Used when the step's ksp_rtol >= 1e-7 (ksfd_step; the parity tests at 1e-11 keep the fp64
// cycle), 2-D, one rank or slab ranks (a float plane travels through the double-typed transport as half as many doubles), V(2,2) with
// the fused smoother (mg_cycle32_ok).  The fp64 right-hand side is read once (k_dinv_apply leaves its fp32 copy), the last smoothing
// kernel writes the result in fp64 (KSmoothT::x64); levels below the last f32 one run with T = double, the transfer kernels convert
// at that border.
// b -> x are the level's own vectors of type T, except on level 0: T = double: the caller's vectors; T = float: the level's, with the
// caller's fp64 right-hand side in b64 and the result going to x64.
// ------------------------------------------------------------------------------------------------
template <typename T>
static int mg_vcycle(ksfd_handle *h, size_t l, double shift, const T *b, T *x, const double *b64, double *x64)
{
    int rc;
    constexpr bool f32 = std::is_same<T, float>::value;
    MGLevel &L = h->mg[l];
    // the level the cycle ends on has fp64 vectors (mg_f32): the exact solve, or Chebyshev sweeps over the whole spectrum
    if constexpr (!f32) if (l == mg_end(h)) {
        if (h->mgc.kind == 1 && h->cur.mgc_ready) return mgc_apply(h, L, b, x);
        return mg_smooth(h, L, shift, b, x, mg_coarse_sweeps(h, L), true, L.ratio);
    }
    // nu sweeps before and after the correction; fp32 vectors have the fused V(2,2) pair only
    auto smooth = [&](bool zero_init) {
        if constexpr (f32) return mg_smooth_fused(h, L, shift, b, x, zero_init, h->mg_ratio, zero_init ? b64 : nullptr, zero_init ? nullptr : x64);
        else return mg_smooth(h, L, shift, b, x, h->mg_nu, zero_init, h->mg_ratio);
    };
    if ((rc = smooth(true))) return rc;
    if ((rc = mg_op<T>(h, L, x, 2, shift, L.vecs<T>().r, b))) return rc;
    if (l == 0 && mg_graph_on(h) && !h->capturing) {
        if ((rc = mg_coarse_graph(h, shift, x, f32, [&]() { return mg_coarse_correction(h, 0, shift, x); }))) return rc;
    } else if ((rc = mg_coarse_correction(h, l, shift, x))) return rc;
    return smooth(false);
}

// this handle has a cycle with fp32 level vectors: they exist on level 0, and the V(2,2) pair with the fused smoother is what runs on them
static bool mg_cycle32_ok(const ksfd_handle *h) { return h->tune.mg_fp32 && h->mg[0].f32 && h->mg_nu == 2 && mg_can_fuse(h, h->mg[0]); }

// out = M^-1 in  (one V cycle)
static int mg_precond(ksfd_handle *h, double shift, const double *in, double *out)
{
    int rc;
    if ((rc = ensure_coef32(h))) return rc;                  // level 0 reads the fp32 copy of the planes (mg_sys)
    if (!h->cur.mg_coef_valid && (rc = mg_restrict_coefs(h))) return rc;
    if (h->cur.mg_shift != shift && (rc = mg_setup_shift(h, shift))) return rc;
    MGVecs<float> &V = h->mg[0].v32;
    if (h->mg_use32 && mg_cycle32_ok(h)) return mg_vcycle<float>(h, 0, shift, V.b, V.x, in, out);
    return mg_vcycle<double>(h, 0, shift, in, out);
}
