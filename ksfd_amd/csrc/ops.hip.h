// libksfd_hip.so -- halo exchange, host-visible reductions, launch geometry, launch wrappers of every kernel class, host<->device layouts
// (part of the single translation unit ksfd_hip.hip, after handle.hip.h: the include list there gives the order)
#pragma once
// ---- halo exchange (DMDA globalToLocal stand-in, KSFD/ksfdsym.py:919-920) -----------------------
static int halo(ksfd_handle *h, double *vec)
{
    if (!h->ring) return KSFD_OK;
    Scope sc(h, KC_HALO, 4.0 * 2.0 * 8.0 * h->G.F * (double)h->G.inner * 2.0);
    int rc = h->tr->exchange(vec, h->G.F, h->G.plane, h->G.inner, h->G.sloc, h->G.ng, h->st);
    if (rc) return fail(h, KSFD_ECOMM, "halo exchange failed: %s", h->tr->error().c_str());
    return KSFD_OK;
}

// ---- reductions to the host ------------------------------------------------------------------
// host side of the zero-copy hand-over: spin until the kernel has raised the flag (with a look at the stream now and then,
// so that a faulted launch turns into an error instead of a hang)
static int spin_for(ksfd_handle *h, unsigned long long seq)
{
    for (unsigned long long spins = 1;; spins++) {
        if (__atomic_load_n(h->pub_flag, __ATOMIC_ACQUIRE) == seq) return KSFD_OK;
        if ((spins & 0xffff) == 0) {
            hipError_t e = hipStreamQuery(h->st);
            if (e == hipSuccess) {
                if (__atomic_load_n(h->pub_flag, __ATOMIC_ACQUIRE) == seq) return KSFD_OK;
                return fail(h, KSFD_EHIP, "reduction finished without publishing its result");
            }
            if (e != hipErrorNotReady) return fail(h, KSFD_EHIP, "stream error while waiting for a reduction: %s", hipGetErrorString(e));
        }
    }
}

// part holds `rows` rows of `nblk` partials; result lands in h->hres[0..rows).  local: the partials already cover the whole quantity on
// every rank (a replicated multigrid level), so slab ranks skip the all-reduce
static int reduce_rows(ksfd_handle *h, int rows, int nblk, int op, bool local = false)
{
    // several ranks with a device-side all-reduce (RCCL): a one-block k_publish behind the all-reduce hands the result over
    // the same way; ksfd_amd.dist.open_handle checks that path end to end on a new handle and clears zero_copy if it fails
    const bool zc = zero_copy_on(h) && !h->capturing && rows <= 128 && (!h->ring || (h->tr->device_allreduce() && !local));
    const bool zc_here = zc && !h->ring;
    h->n_host_sync++;
    const unsigned long long seq = zc ? ++h->pub_seq : 0;
    {
        Scope sc(h, KC_REDUCE, 8.0 * rows * (double)nblk);
        if (zc_here) hipLaunchKernelGGL(k_reduce_rows, dim3(rows), dim3(KSFD_BLOCK), 0, h->st, h->part, nblk, op, h->dres, h->hres_dev, h->pub_count, h->pub_flag_dev, seq);
        else hipLaunchKernelGGL(k_reduce_rows, dim3(rows), dim3(KSFD_BLOCK), 0, h->st, h->part, nblk, op, h->dres);
    }
    if (zc_here) { HIPCHK(h, hipGetLastError()); return spin_for(h, seq); }
    if (h->ring && !local) {
        int rc = h->tr->allreduce(h->dres, rows, op, h->st);
        if (rc) return fail(h, KSFD_ECOMM, "allreduce failed: %s", h->tr->error().c_str());
        if (h->tr->result_on_host()) { memcpy(h->hres, h->tr->host_result(), sizeof(double) * rows); return KSFD_OK; }
        if (zc) {
            hipLaunchKernelGGL(k_publish, dim3(1), dim3(128), 0, h->st, (const double *)h->dres, rows, h->hres_dev, h->pub_flag_dev, seq);
            HIPCHK(h, hipGetLastError());
            return spin_for(h, seq);
        }
    }
    HIPCHK(h, hipMemcpyAsync(h->hres, h->dres, sizeof(double) * rows, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return KSFD_OK;
}

// ---- kernel wrappers ----------------------------------------------------------------------------
#define NL_DISPATCH(nl, CALL)                                                                      \
    switch (nl) {                                                                                  \
    case 1: { constexpr int NL = 1; CALL; } break;                                                 \
    case 2: { constexpr int NL = 2; CALL; } break;                                                 \
    case 3: { constexpr int NL = 3; CALL; } break;                                                 \
    case 4: { constexpr int NL = 4; CALL; } break;                                                 \
    case 5: { constexpr int NL = 5; CALL; } break;                                                 \
    case 6: { constexpr int NL = 6; CALL; } break;                                                 \
    case 7: { constexpr int NL = 7; CALL; } break;                                                 \
    case 8: { constexpr int NL = 8; CALL; } break;                                                 \
    case 9: { constexpr int NL = 9; CALL; } break;                                                 \
    case 10: { constexpr int NL = 10; CALL; } break;                                               \
    case 11: { constexpr int NL = 11; CALL; } break;                                               \
    default: { constexpr int NL = 12; CALL; } break;                                               \
    }

// ---- launch geometry (of a KGeom, not of the handle: the multigrid levels have their own) -------
// grid of a grid-stride launch over n items / the points of a plane with its ghost rows / the owned points
static inline int blocks_for(long long n) { return (int)std::min<long long>((n + KSFD_BLOCK - 1) / KSFD_BLOCK, 4096); }
static inline int plane_blocks(const KGeom &G) { return blocks_for(G.plane); }
static inline int point_blocks(const KGeom &G) { return blocks_for(G.nloc); }
// strip launches: whole rounds over the 8 XCDs (ksfd_xcd_remap)
static inline int round8(long long nb) { return (int)((nb + 7) / 8 * 8); }

// segments seg0, seg0 + seg_stride, ... (nseg of them) of the strips K: four waves to a block
static KStrips strips_sub(KStrips K, int seg0, int seg_stride, int nseg)
{
    K.seg0 = seg0; K.seg_stride = seg_stride; K.nseg = nseg;
    K.nblocks = round8(((long long)K.nstrips * nseg + 3) / 4);
    return K;
}
// all row segments of G in strips of at most yseg rows.  Small grids: shorter segments so that there are about wave_target waves
// to fill 256 CUs (a wave costs ~1 us per row it marches; the 4 halo rows per segment are L2 hits at these sizes)
static KStrips strips_for(const KGeom &G, int yseg, long long wave_target)
{
    KStrips S;
    S.nstrips = (int)((G.nx + KSFD_STRIP_OUT - 1) / KSFD_STRIP_OUT);
    const long long fit = std::max<long long>((long long)S.nstrips * G.sloc / wave_target, 2);
    S.yseg = (int)std::min<long long>(yseg, fit);
    return strips_sub(S, 0, 1, (int)((G.sloc + S.yseg - 1) / S.yseg));
}
static KStrips make_strips(const ksfd_handle *h, bool jvp = false)
{
    return strips_for(h->G, jvp ? h->tune.yseg_jvp : h->tune.yseg, jvp ? env_knobs().waves_jvp : env_knobs().waves_rhs);
}

// launch geometry of the 3-D z-marching strip kernels: blocks of `rows` y rows, z segments of at most zseg planes, shorter when that
// is what it takes to have about block_target blocks for 256 CUs
static K3D k3d_for(const KGeom &G, int rows, int sync, int zseg, long long block_target)
{
    K3D K;
    K.rows = rows; K.sync = sync;
    K.nstrips = (int)((G.nx + KSFD_STRIP_OUT - 1) / KSFD_STRIP_OUT);
    K.nygrp = (int)((G.ny + rows - 1) / rows);
    const long long fit = std::max<long long>((long long)K.nstrips * K.nygrp * G.sloc / block_target, 2);
    K.zseg = (int)std::min<long long>(zseg, fit);
    K.nzseg = (int)((G.sloc + K.zseg - 1) / K.zseg);
    K.nblocks = round8((long long)K.nstrips * K.nygrp * K.nzseg);
    return K;
}
// rows of y per block of the 3-D strip kernels (K3D).  Measured at 512^3 (bench.py --dim 3, ms per step): 4 rows 110.6, 4 rows with a
// barrier per plane 107.8, 8 rows 111.9, 8 rows + barrier 115.5 -- so 4 rows marching in step; KSFD_ROWS3D=8 / KSFD_SYNC3D=0 for measurements
static int rows3d(const ksfd_handle *h)
{
    return (env_knobs().rows3d == 8 && h->P.nlig == 1) ? 8 : 4;
}
static K3D make_k3d(const ksfd_handle *h)
{
    const int rows = rows3d(h);
    return k3d_for(h->G, rows, env_knobs().sync3d && (h->G.ny % rows == 0), h->tune.zseg, rows == 8 ? 512 : 1024);
}

// ---- frozen Jacobian action shift*v - J v: where it runs and which kernel serves it ---------------
// The action is a function of (geometry, physics, coefficient planes, dG scratch plane): the handle's grid and every level of the
// multigrid hierarchy (mg_host.hip.h: mg_sys) describe themselves this way and share the launch helpers below
struct JvpSys {
    const KGeom *G; const KPhys *P;
    const double *coef;                      // [rho, G, G_rho, G_U..] planes of that grid
    const float *coef32;                     // their fp32 copy, NULL where there is none
    double *dG;                              // scratch plane of the dG pass (3-D strip and generic kernels)
    int cls;                                 // kernel class the launches are booked under
};
static JvpSys jvp_sys(const ksfd_handle *h) { return { &h->G, &h->P, h->coef, coef32_on(h) ? h->coef32 : nullptr, h->dGb, KC_JVP }; }

enum JvpPath { JP_STRIP2D, JP_LDS3D, JP_STRIP3D, JP_GENERIC };     // k_jvp2d_frozen, k_jvp3d_lds, dG pass + k_jvp3d_frozen, dG pass + k_jvp_generic
// fewest columns the strip kernels serve
static const int JVP_NX_GRID = 4;         // the handle's grid: what the five-point window of a periodic row needs
static const int JVP_NX_LEVEL = 16;       // multigrid levels: coarse levels of 8..14 columns should not march 124-column strips
// The one rule.  tune.use_fused off, an odd nx, fewer than min_nx columns, more than 4 ligands or a 1-D grid: generic.  2-D: the strip kernel
// (4 slow units at least: every level of a hierarchy has them, mg_build).  3-D: the second generation for one or two ligands where ny is
// a multiple of its 8 rows per block (KSFD_J3L=0 keeps the first generation), else the first-generation strip kernel
static JvpPath jvp_path(const ksfd_handle *h, const KGeom &G, int nlig, int min_nx)
{
    if (!h->tune.use_fused || G.dim < 2 || (G.nx % 2) || G.nx < min_nx || nlig > 4) return JP_GENERIC;
    if (G.dim == 2) return G.sloc >= 4 ? JP_STRIP2D : JP_GENERIC;
    return (env_knobs().j3l && nlig <= 2 && G.ny % KSFD_J3L_ROWS == 0) ? JP_LDS3D : JP_STRIP3D;
}
// the handle's own grid: strip kernels of the RHS and of the Jacobian action alike (k_rhs2d_fused / k_rhs3d_strip follow the same rule)
static bool fused_ok(const ksfd_handle *h) { return jvp_path(h, h->G, h->P.nlig, JVP_NX_GRID) == JP_STRIP2D; }
static bool strip3d_ok(const ksfd_handle *h) { const JvpPath p = jvp_path(h, h->G, h->P.nlig, JVP_NX_GRID); return p == JP_LDS3D || p == JP_STRIP3D; }

// path of the handle's grid.  k_jvp3d_lds (y-neighbours through the LDS, dG on the fly) needs its dynamic LDS size registered, once per
// handle; where that fails the first generation serves the grid
static JvpPath grid_path(ksfd_handle *h)
{
    const JvpPath p = jvp_path(h, h->G, h->P.nlig, JVP_NX_GRID);
    if (p == JP_LDS3D && !h->j3l_attr_set) {
        auto reg = [](const void *k, size_t lds) { return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess; };
        h->j3l_usable = h->P.nlig == 1 ? reg((const void *)k_jvp3d_lds<1, double>, ksfd_j3l_lds_bytes<1>()) && reg((const void *)k_jvp3d_lds<1, float>, ksfd_j3l_lds_bytes<1>())
                                       : reg((const void *)k_jvp3d_lds<2, double>, ksfd_j3l_lds_bytes<2>()) && reg((const void *)k_jvp3d_lds<2, float>, ksfd_j3l_lds_bytes<2>());
        h->j3l_attr_set = true;
        if (!h->j3l_usable) hipGetLastError();
    }
    return (p == JP_LDS3D && !h->j3l_usable) ? JP_STRIP3D : p;
}
static bool j3l_ok(ksfd_handle *h) { return grid_path(h) == JP_LDS3D; }
// (one block per CU: four rounds of blocks at least)
static K3D make_k3d_lds(const ksfd_handle *h) { return k3d_for(h->G, KSFD_J3L_ROWS, 0, h->tune.zseg, 1024); }

// wave counts of the strip launches: the fused norms leave one partial per wave in h->part
static inline long long part_capacity() { return (long long)(2 * KSFD_MAXDOT + 4) * 4096; }      // of h->part in doubles (ksfd_create)
static long long strip_waves(const ksfd_handle *h, bool jvp = false) { const KStrips K = make_strips(h, jvp); return (long long)K.nstrips * K.nseg; }
static long long k3d_waves(ksfd_handle *h) { const K3D K = j3l_ok(h) ? make_k3d_lds(h) : make_k3d(h); return (long long)K.nblocks * K.rows; }

// launch of k_jvp3d_lds for 1 or 2 ligands and the storage type of the output
template <typename TO>
static void j3l_launch(ksfd_handle *h, const K3D &K, const double *v, int mode, double shift, TO *out, const double *yadd, double alpha, double beta, double *normpart)
{
    const KGeom &G = h->G;
    if (h->P.nlig == 1) hipLaunchKernelGGL((k_jvp3d_lds<1, TO>), dim3(K.nblocks), dim3(KSFD_J3L_ROWS * KSFD_WAVE), ksfd_j3l_lds_bytes<1>(), h->st, G, h->P, K, (const double *)h->coef, v, mode, shift, out, yadd, alpha, beta, normpart);
    else hipLaunchKernelGGL((k_jvp3d_lds<2, TO>), dim3(K.nblocks), dim3(KSFD_J3L_ROWS * KSFD_WAVE), ksfd_j3l_lds_bytes<2>(), h->st, G, h->P, K, (const double *)h->coef, v, mode, shift, out, yadd, alpha, beta, normpart);
}

static KSrc src_of(const ksfd_handle *h, int stage)
{
    KSrc s;
    for (int c = 0; c <= KSFD_MAXL; c++) s.p[c] = (stage >= 0 && c < h->G.F) ? h->src[stage][c] : nullptr;
    return s;
}

// dG plane of the direction v from the frozen coefficient planes of Y: the pass in front of the 3-D (first generation) and generic
// Jacobian-action kernels.  cls < 0: the launch rides in the caller's Scope (multigrid levels charge both kernels as one)
static void dg_pass(ksfd_handle *h, const JvpSys &Y, const double *v, int cls = KC_GFIELD)
{
    const KGeom &G = *Y.G;
    auto launch = [&] { NL_DISPATCH(Y.P->nlig, hipLaunchKernelGGL((k_dg_frozen<NL>), dim3(plane_blocks(G)), dim3(KSFD_BLOCK), 0, h->st, G, Y.coef, v, Y.dG)); };
    if (cls < 0) return launch();
    Scope sc(h, cls, 8.0 * (2 + Y.P->nlig + G.F) * (double)G.plane);
    launch();
}

// The one launch of each kernel of the frozen action, on the system Y, inside the caller's Scope.  k_jvp2d_frozen on the strips K.  The storage types of C, v, yadd and out come from the pointers.  Every (types, SMOOTH) combination is a
// kernel of its own, so the coefficient type and SMOOTH are compile-time choices of the caller (a run-time flag in here would build
// smoother kernels for the type combinations of the polynomial preconditioner).  sm: KSmooth{} without a smoother
template <bool SMOOTH, typename TC, typename TV, typename TY, typename TO, typename TS>
static void jvp2d_launch(ksfd_handle *h, const JvpSys &Y, const KStrips &K, const TC *C, const TV *v, int mode, double shift, TO *out, const TY *yadd, double alpha, double beta, const KSmoothT<TS> &sm, double *normpart)
{
    static_assert(SMOOTH || std::is_same<TS, double>::value, "no smoother: pass KSmooth{}");
    NL_DISPATCH(Y.P->nlig, if constexpr (NL <= 4) hipLaunchKernelGGL((k_jvp2d_frozen<NL, TC, TV, TY, TO, 1, SMOOTH, TS>), dim3(K.nblocks), dim3(KSFD_BLOCK), 0, h->st,
                                                                     *Y.G, *Y.P, K, C, v, mode, shift, out, yadd, alpha, beta, sm, normpart));
}
// k_jvp3d_frozen on the blocks K, behind a dg_pass; TO: storage type of out.  8 rows per block exist for one ligand only (rows3d)
template <typename TO>
static void jvp3d_launch(ksfd_handle *h, const JvpSys &Y, const K3D &K, const double *v, int mode, double shift, TO *out, const double *yadd, double alpha, double beta, double *normpart)
{
    if (K.rows == 8) hipLaunchKernelGGL((k_jvp3d_frozen<1, TO, 8>), dim3(K.nblocks), dim3(8 * KSFD_WAVE), 0, h->st, *Y.G, *Y.P, K, Y.coef, v, (const double *)Y.dG, mode, shift, out, yadd, alpha, beta, normpart);
    else NL_DISPATCH(Y.P->nlig, if constexpr (NL <= 4) hipLaunchKernelGGL((k_jvp3d_frozen<NL, TO>), dim3(K.nblocks), dim3(KSFD_BLOCK), 0, h->st, *Y.G, *Y.P, K, Y.coef, v, (const double *)Y.dG, mode, shift, out, yadd, alpha, beta, normpart));
}
// k_jvp_generic behind a dg_pass, as a grid-stride launch of nblocks blocks (point_blocks on the handle's grid, plane_blocks on the
// multigrid levels).  The kernel reads rho from plane 0 of its `u` argument (already clamped in the coefficient planes) and G from plane 1
static void jvpgen_launch(ksfd_handle *h, const JvpSys &Y, int nblocks, const double *v, int mode, double shift, double *out, const double *yadd, double alpha, double beta, const KSmooth &sm)
{
    NL_DISPATCH(Y.P->nlig, hipLaunchKernelGGL((k_jvp_generic<NL>), dim3(nblocks), dim3(KSFD_BLOCK), 0, h->st, *Y.G, *Y.P, Y.coef, v, Y.coef + Y.G->plane, (const double *)Y.dG, mode, shift, out, yadd, alpha, beta, sm));
}

// Bytes per point a Jacobian action moves, by the storage types of its operands: impl = ncoef coefficient planes + v + out (+ yadd in
// modes 2 and 3) + extra, alg = SURVEY.md 8d: read u, v, write out (+ the fused vector operand) in fp64.  ncoef is 3 + nlig where the
// kernel reads the coefficient planes, 3 on the paths where a dG plane pass stands in for them.
struct JvpBytes { double impl, alg; };
template <typename TC = double, typename TV = double, typename TY = double, typename TO = double>
static JvpBytes jvp_bytes(const KGeom &G, int mode, double ncoef, double extra = 0.0)
{
    const double y = (mode == 2 || mode == 3) ? G.F : 0;
    return { ncoef * sizeof(TC) + G.F * (double)(sizeof(TV) + sizeof(TO)) + y * (double)sizeof(TY) + extra, 8.0 * (3.0 * G.F + y) };
}

// A strip launch whose input needs its ghost rows exchanged first (slab ranks), with the exchange hidden behind the interior rows:
//   compute stream: [interior segments]                      [two boundary segments]
//   comm stream   :   wait(input ready) -> ghost rows <- ring neighbours -> signal
// Interior segments read owned rows only; the first and last segment are the only readers of ghost rows.  Without h->tune.overlap or
// with fewer than 3 segments: exchange on the compute stream, then one launch of everything.
// exchange(stream) -> nonzero on failure; launch(strips, share of the work, normpart) -> KSFD error code.  normpart: per-wave
// partials numbered over ALL segments of K (interior launch first, then the two boundary segments)
template <typename Exchange, typename Launch>
static int with_halo_overlap(ksfd_handle *h, const KStrips &K, double *normpart, Exchange exchange, Launch launch)
{
    int rc;
    const bool ovl = h->tune.overlap && K.nseg >= 3;
    if (ovl) {
        HIPCHK(h, hipEventRecord(h->ev_ready, h->st));
        if ((rc = launch(strips_sub(K, 1, 1, K.nseg - 2), (double)(K.nseg - 2) / K.nseg, normpart))) return rc;
        HIPCHK(h, hipStreamWaitEvent(h->st_comm, h->ev_ready, 0));
    }
    if (exchange(ovl ? h->st_comm : h->st)) return fail(h, KSFD_ECOMM, "halo exchange failed: %s", h->tr->error().c_str());
    if (!ovl) return launch(K, 1.0, normpart);
    HIPCHK(h, hipEventRecord(h->ev_halo, h->st_comm));
    HIPCHK(h, hipStreamWaitEvent(h->st, h->ev_halo, 0));
    return launch(strips_sub(K, 0, K.nseg - 1, 2), 2.0 / K.nseg, normpart ? normpart + (long long)K.nstrips * (K.nseg - 2) : nullptr);
}

// out = f(u) (+sources of `stage`); u must have valid ghosts when size>1
// want_norm (fused 2-D path only): ||out||^2 lands in h->hres[0] without a pass of its own (per-wave partials in the store epilogue)
// halo_vec (slab ranks): a vector among the inputs whose ghost rows have NOT been exchanged yet (the newest stage vector).  On the
// 2-D strip path they travel on the communication stream while the interior segments are computed (with_halo_overlap); elsewhere
// they are exchanged first.
// ndots (with want_norm, fused 2-D path): <out, dotv + q*vlen>, q < ndots <= 2, land in h->hres[1 + q] beside ||out||^2 in h->hres[0]
static int op_rhs(ksfd_handle *h, const double *u, int stage, double *out, const KComb *cmb = nullptr, bool want_norm = false, double *halo_vec = nullptr,
                  int ndots = 0, const double *dotv = nullptr)
{
    const KGeom &G = h->G;
    KSrc S = src_of(h, stage);
    // time-dependent parameters: the reference evaluates ps.values(t) at the STAGE time of every RHS call
    const KPhys &PP = (stage >= 0 && stage < 4 && h->Pst_valid[stage]) ? h->Pst[stage] : h->P;
    if (!h->ring) halo_vec = nullptr;
    if (fused_ok(h)) {
        KStrips K = make_strips(h);
        KComb C = cmb ? *cmb : KComb{};
        const long long nwaves = strip_waves(h);
        const bool fused_norm = want_norm && nwaves * (1 + ndots) <= part_capacity();
        KDots D = KDots{};
        if (fused_norm && ndots > 0) { D.n = std::min(ndots, 2); D.stride = nwaves; for (int q = 0; q < D.n; q++) D.v[q] = dotv + (int64_t)q * h->vlen; }
        // the vectors added at the store are the ones the stage argument is formed from: one read serves both (k_rhs2d_fused<NL, true>)
        bool carry = h->tune.rhs_carry && C.nout > 0 && C.nout == C.nin;
        for (int j = 0; j < C.nout && carry; j++) carry = C.yin[j] == C.yout[j];
        // first stage of a step: the argument is the resident state itself and G(u) is plane 1 of the frozen coefficients the step has
        // just made of it (same parameters, same clamped inputs): loaded, not evaluated (the rule of the 3-D path below)
        const bool reuse_G = h->tune.rhs_gplane && C.nin == 0 && C.nout == 0 && u == h->u && h->cur.coef_fresh && h->tune.use_frozen && h->coef && &PP == &h->P;
        auto launch = [&](const KStrips &Kx, double frac, double *np) -> int {
            Scope sc(h, KC_RHS, (vbytes(h, 2 + C.nin + (carry ? 0 : C.nout) + D.n) + (reuse_G ? 8.0 * (double)G.nloc : 0.0)) * frac, vbytes(h, 2 + C.nin + C.nout + D.n) * frac);
            if (reuse_G) { NL_DISPATCH(h->P.nlig, if constexpr (NL <= 4) hipLaunchKernelGGL((k_rhs2d_fused<NL, false, true>), dim3(Kx.nblocks), dim3(KSFD_BLOCK), 0, h->st, G, PP, Kx, u, S, out, C, np, D, (const double *)(h->coef + G.plane))); }
            else if (carry) { NL_DISPATCH(h->P.nlig, if constexpr (NL <= 4) hipLaunchKernelGGL((k_rhs2d_fused<NL, true>), dim3(Kx.nblocks), dim3(KSFD_BLOCK), 0, h->st, G, PP, Kx, u, S, out, C, np, D)); }
            else { NL_DISPATCH(h->P.nlig, if constexpr (NL <= 4) hipLaunchKernelGGL((k_rhs2d_fused<NL>), dim3(Kx.nblocks), dim3(KSFD_BLOCK), 0, h->st, G, PP, Kx, u, S, out, C, np, D)); }
            return KSFD_OK;
        };
        double *np = fused_norm ? h->part : (double *)nullptr;
        int rc = !halo_vec ? launch(K, 1.0, np) : with_halo_overlap(h, K, np, [&](hipStream_t st) {
            Scope sc(h, KC_HALO, 4.0 * 2.0 * 8.0 * G.F * (double)G.inner * 2.0);
            return h->tr->exchange(halo_vec, G.F, G.plane, G.inner, G.sloc, G.ng, st);
        }, launch);
        if (rc) return rc;
        HIPCHK(h, hipGetLastError());
        if (fused_norm) return reduce_rows(h, 1 + D.n, (int)nwaves, 0);
        if (want_norm) return fail(h, KSFD_EINVAL, "op_rhs: fused norm needs the strip kernels");
        return KSFD_OK;
    }
    if (halo_vec) { int rc = halo(h, halo_vec); if (rc) return rc; }
    if (strip3d_ok(h) && h->tune.rhs3d_strip) {
        // 3-D: G plane (+ the stage argument, when the stage algebra rides along), then the z-marching 13-point star
        if (want_norm) return fail(h, KSFD_EINVAL, "op_rhs: fused norm is a 2-D feature");
        KComb C = cmb ? *cmb : KComb{};
        const double *uin = u;
        const double *Gplane = h->Gb;
        // first stage of a step: the argument is the resident state itself and G(u) is plane 1 of the frozen coefficients the step has
        // just made of it (same parameters): nothing to form, no pass
        const bool reuse_G = C.nin == 0 && u == h->u && h->cur.coef_fresh && h->tune.use_frozen && h->coef && &PP == &h->P;
        if (reuse_G) Gplane = h->coef + G.plane;
        else {
            Scope sc(h, KC_GFIELD, 8.0 * ((1 + C.nin) * G.F + (C.nin ? G.F : 0) + 1) * (double)G.plane, C.nin ? vbytes(h, 2 + C.nin) : 0.0);
            NL_DISPATCH(h->P.nlig, if constexpr (NL <= 4) hipLaunchKernelGGL((k_gfield_comb<NL>), dim3(plane_blocks(G)), dim3(KSFD_BLOCK), 0, h->st, G, PP, u, C, C.nin ? h->Z : (double *)nullptr, h->Gb));
        }
        if (C.nin) uin = h->Z;
        K3D K = make_k3d(h);
        Scope sc(h, KC_RHS, 8.0 * (2.0 * G.F + 1 + C.nout * G.F) * (double)G.nloc, vbytes(h, 2 + C.nout));
        if (K.rows == 8) hipLaunchKernelGGL((k_rhs3d_strip<1, 8>), dim3(K.nblocks), dim3(8 * KSFD_WAVE), 0, h->st, G, PP, K, uin, Gplane, S, out, C);
        else NL_DISPATCH(h->P.nlig, if constexpr (NL <= 4) hipLaunchKernelGGL((k_rhs3d_strip<NL>), dim3(K.nblocks), dim3(KSFD_BLOCK), 0, h->st, G, PP, K, uin, Gplane, S, out, C));
    } else {
        {
            Scope sc(h, KC_GFIELD, 8.0 * (G.F + 1) * (double)G.plane);
            NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_gfield<NL, false>), dim3(plane_blocks(G)), dim3(KSFD_BLOCK), 0, h->st, G, PP, u, (const double *)nullptr, h->Gb, (double *)nullptr));
        }
        Scope sc(h, KC_RHS, vbytes(h, 2) + 8.0 * (double)G.nloc, vbytes(h, 2));
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_rhs_generic<NL>), dim3(point_blocks(G)), dim3(KSFD_BLOCK), 0, h->st, G, PP, u, h->Gb, S, out));
    }
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

// out = J(u) v (mode 0) or shift*v - J(u) v (mode 1); u and v need valid ghosts when size>1
static int op_jvp(ksfd_handle *h, const double *u, const double *v, int mode, double shift, double *out)
{
    const KGeom &G = h->G;
    if (fused_ok(h)) {
        KStrips K = make_strips(h, true);
        Scope sc(h, KC_JVP, vbytes(h, 3));
        NL_DISPATCH(h->P.nlig, if constexpr (NL <= 4) hipLaunchKernelGGL((k_jvp2d_fused<NL>), dim3(K.nblocks), dim3(KSFD_BLOCK), 0, h->st, G, h->P, K, u, v, mode, shift, out));
    } else {
        {
            Scope sc(h, KC_GFIELD, 8.0 * (2 * G.F + 2) * (double)G.plane);
            NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_gfield<NL, true>), dim3(plane_blocks(G)), dim3(KSFD_BLOCK), 0, h->st, G, h->P, u, v, h->Gb, h->dGb));
        }
        Scope sc(h, KC_JVP, vbytes(h, 3) + 16.0 * (double)G.nloc, vbytes(h, 3));
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_jvp_generic<NL>), dim3(point_blocks(G)), dim3(KSFD_BLOCK), 0, h->st, G, h->P, u, v, h->Gb, h->dGb, mode, shift, out));
    }
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

// The buffer of the fp32 coefficient copy, allocated when first wanted (2-D strip path only).  false: no copy on this handle (poly_fp32
// off, another kernel path, or no memory: coef32_failed keeps the allocation from being tried at every call)
static bool coef32_alloc(ksfd_handle *h)
{
    const KGeom &G = h->G;
    if (!h->coef32 && !h->coef32_failed && h->tune.poly_fp32 && fused_ok(h) && h->P.nlig <= 4 && G.plane % 2 == 0 && G.inner % 2 == 0 &&
        hipMalloc((void **)&h->coef32, sizeof(float) * (size_t)(3 + h->P.nlig) * G.plane) != hipSuccess) { h->coef32 = nullptr; h->coef32_failed = true; (void)hipGetLastError(); }
    return coef32_on(h);
}

// Once per step: C = [rho, G, G_rho, G_U..] of the (ghost-filled) state u
// c32: where the launch stores the fp32 copy of the planes, or NULL.  want_means: the grid means of the spectral preconditioner come out
// of the same launch (resident state only; the caller has checked that the block partials fit)
static int op_jcoef(ksfd_handle *h, const double *u, float *c32, bool want_means)
{
    const KGeom &G = h->G;
    const int nbp = plane_blocks(G);
    {
    Scope sc(h, KC_GFIELD, (8.0 * (G.F + 3 + h->P.nlig) + (c32 ? 4.0 * (3 + h->P.nlig) : 0.0)) * (double)G.plane);
    NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_jcoef<NL>), dim3(nbp), dim3(KSFD_BLOCK), 0, h->st, G, h->P, u, h->coef, c32, want_means ? h->part : (double *)nullptr));
    }
    HIPCHK(h, hipGetLastError());
    if (want_means) {
        int rc = reduce_rows(h, 1 + h->P.nlig, nbp, 0);
        if (rc) return rc;
        const double ntot = (double)h->cfg.n[0] * (double)h->cfg.n[1] * (double)h->cfg.n[2];
        h->spec.a_rr = h->hres[0] / ntot;
        for (int l = 0; l < h->P.nlig; l++) h->spec.a_rU[l] = h->hres[1 + l] / ntot;
    }
    return KSFD_OK;
}

// Coefficient planes of the RESIDENT state, computed once per state: the CFL check after a step and the next step's
// Jacobian need the same planes (the reference evaluates G twice there: velocity, KSFD/ksfdsym.py:1188-1209, and Jacobian).
// Every event that gives h->u or the parameters new values ends cur.coef_fresh (handle_state.h: state_written, params_changed).
static int ensure_coef(ksfd_handle *h, bool ghosts_done = false)
{
    if (h->cur.coef_fresh) return KSFD_OK;
    int rc;
    if (!ghosts_done && (rc = halo(h, h->u))) return rc;
    // the fp32 copy is made when a consumer asks for it (ensure_coef32); only the old step boundary has k_jcoef store it
    float *c32 = h->tune.old_boundary && coef32_alloc(h) ? h->coef32 : nullptr;
    const bool means = h->spec.ok && (long long)(1 + h->P.nlig) * plane_blocks(h->G) <= part_capacity();
    if ((rc = op_jcoef(h, h->u, c32, means))) return rc;
    ksfd_ctl::planes_recomputed(h->cur, c32 != nullptr, means);
    return KSFD_OK;
}

// fp32 copy of the coefficient planes as they are now, for the readers that take it: the Horner path of the polynomial preconditioner
// (poly_apply) and level 0 of the V cycle (mg_sys).  The spectral regime never asks.  (float) of the stored double is what k_jcoef's
// own store rounds, so the readers see the same bits either way.
static int ensure_coef32(ksfd_handle *h)
{
    if (!coef32_alloc(h) || h->cur.coef32_fresh) return KSFD_OK;
    const long long n = (long long)(3 + h->P.nlig) * h->G.plane;
    {
        Scope sc(h, KC_GFIELD, 12.0 * (double)n);
        hipLaunchKernelGGL(k_coef32, dim3(blocks_for(n / 2)), dim3(KSFD_BLOCK), 0, h->st, n, (const double *)h->coef, h->coef32);
    }
    HIPCHK(h, hipGetLastError());
    ksfd_ctl::coef32_made(h->cur);
    return KSFD_OK;
}

// The 2-D strip kernel of the frozen Jacobian action on `frac` of the segments, for any storage types of its operands (fp32
// coefficient copy / Horner temporaries of the polynomial preconditioner, fp32 residual of the spectral solver)
template <typename TC, typename TV, typename TY, typename TO>
static int jvp2d_launch_t(ksfd_handle *h, const KStrips &K, double frac, const TC *C, const TV *v, int mode, double shift, TO *out, const TY *yadd, double alpha, double beta, double *normpart = nullptr)
{
    const KGeom &G = h->G;
    const JvpBytes B = jvp_bytes<TC, TV, TY, TO>(G, mode, 3 + h->P.nlig);
    Scope sc(h, KC_JVP, B.impl * (double)G.nloc * frac, B.alg * (double)G.nloc * frac);
    jvp2d_launch<false>(h, jvp_sys(h), K, C, v, mode, shift, out, yadd, alpha, beta, KSmooth{}, normpart);
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

// ... with the halo exchange of v hidden behind the interior rows on slab ranks (with_halo_overlap; the caller has NOT exchanged the
// ghost rows of v).  A float vector travels through the double-typed transport as half as many doubles (inner and plane are even
// on this path).  normpart != NULL: per-wave partials of ||out||^2
template <typename TC, typename TV, typename TY, typename TO>
static int jvp2d_halo_t(ksfd_handle *h, const TC *C, TV *v, int mode, double shift, TO *out, const TY *yadd, double alpha, double beta, double *normpart = nullptr)
{
    const KGeom &G = h->G;
    auto launch = [&](const KStrips &Kx, double frac, double *np) { return jvp2d_launch_t(h, Kx, frac, C, v, mode, shift, out, yadd, alpha, beta, np); };
    if (!h->ring) return launch(make_strips(h, true), 1.0, normpart);
    const long long scale = sizeof(double) / sizeof(TV);            // 1 for double, 2 for float
    return with_halo_overlap(h, make_strips(h, true), normpart, [&](hipStream_t st) {
        Scope sc(h, KC_HALO, 4.0 * 2.0 * sizeof(TV) * G.F * (double)G.inner * 2.0);
        return h->tr->exchange(reinterpret_cast<double *>(v), G.F, G.plane / scale, G.inner / scale, G.sloc, G.ng, st);
    }, launch);
}

// Jacobian action from the frozen coefficients (see stencil.hip.h, "Frozen-Jacobian path")
static int op_jvp_frozen(ksfd_handle *h, const double *v, int mode, double shift, double *out, const double *yadd = nullptr, double alpha = 0.0, double beta = 0.0)
{
    const KGeom &G = h->G;
    const JvpSys Y = jvp_sys(h);
    const JvpBytes B = jvp_bytes(G, mode, 3 + h->P.nlig), Bdg = jvp_bytes(G, mode, 3);
    const JvpPath path = grid_path(h);
    if (path == JP_STRIP2D) return jvp2d_launch_t(h, make_strips(h, true), 1.0, Y.coef, v, mode, shift, out, yadd, alpha, beta);
    if (path == JP_LDS3D) {
        Scope sc(h, KC_JVP, B.impl * (double)G.nloc, B.alg * (double)G.nloc);
        j3l_launch<double>(h, make_k3d_lds(h), v, mode, shift, out, yadd, alpha, beta, nullptr);
    } else {
        dg_pass(h, Y, v);
        Scope sc(h, KC_JVP, Bdg.impl * (double)G.nloc, Bdg.alg * (double)G.nloc);
        if (path == JP_STRIP3D) jvp3d_launch<double>(h, Y, make_k3d(h), v, mode, shift, out, yadd, alpha, beta, nullptr);
        else jvpgen_launch(h, Y, point_blocks(G), v, mode, shift, out, yadd, alpha, beta, KSmooth{});
    }
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

// Jacobian action on a vector whose ghost rows have NOT been exchanged yet: behind the interior rows where the 2-D strip kernel
// runs with at least 3 segments, else exchange first and op_jvp_frozen (which also serves the 3-D and generic kernels)
static int op_jvp_frozen_halo(ksfd_handle *h, double *v, int mode, double shift, double *out, const double *yadd = nullptr, double alpha = 0.0, double beta = 0.0)
{
    if (!h->ring) return op_jvp_frozen(h, v, mode, shift, out, yadd, alpha, beta);
    if (!h->tune.overlap || !fused_ok(h) || make_strips(h, true).nseg < 3 || h->P.nlig > 4) {
        const int rc = halo(h, v);
        return rc ? rc : op_jvp_frozen(h, v, mode, shift, out, yadd, alpha, beta);
    }
    return jvp2d_halo_t<double, double, double, double>(h, (const double *)h->coef, v, mode, shift, out, yadd, alpha, beta);
}

// r32 = b - A x stored in fp32 (its only reader is the spectral preconditioner, which works in fp32 anyway) with ||r||^2 in
// fp64 from the store epilogue -> h->hres[0].  Single rank or slab ranks (2-D: the ghost rows of x travel while the interior segments are
// computed, the caller has NOT exchanged them), strip kernels.
static int op_residual32(ksfd_handle *h, const double *x, double shift, const double *b, float *r32)
{
    const KGeom &G = h->G;
    const long long nwaves = G.dim == 3 ? k3d_waves(h) : strip_waves(h, true);
    if (nwaves > part_capacity()) return fail(h, KSFD_EINVAL, "op_residual32: too many waves for the fused norm");
    if (G.dim == 3) {
        // second generation, or: dG plane, then the z-marching Jacobian action in residual mode; fp32 output and the norm in the epilogue
        const JvpSys Y = jvp_sys(h);
        const bool j3l = j3l_ok(h);
        if (!j3l) dg_pass(h, Y, x);
        // (the second generation charges one more fp64 vector than its operands: kept as it has always been reported)
        const JvpBytes B = j3l ? jvp_bytes<double, double, double, float>(G, 2, 3 + h->P.nlig, 8.0 * G.F) : jvp_bytes<double, double, double, float>(G, 2, 3);
        Scope sc(h, KC_JVP, B.impl * (double)G.nloc, B.alg * (double)G.nloc);
        if (j3l) j3l_launch<float>(h, make_k3d_lds(h), x, 2, shift, r32, b, 0.0, 0.0, h->part);
        else jvp3d_launch<float>(h, Y, make_k3d(h), x, 2, shift, r32, b, 0.0, 0.0, h->part);
    } else if (int rc = jvp2d_halo_t(h, h->coef, const_cast<double *>(x), 2, shift, r32, b, 0.0, 0.0, h->part)) return rc;
    HIPCHK(h, hipGetLastError());
    return reduce_rows(h, 1, (int)nwaves, 0);
}

// VW = 2 when every plane/offset/length is even (all accesses 16-byte aligned double2)
static inline bool vec2(const ksfd_handle *h) { return (h->G.nloc % 2 == 0) && (h->kv.off % 2 == 0) && (h->G.plane % 2 == 0); }
static inline dim3 vgridw(const ksfd_handle *h, int vw) { return dim3((h->nblk_vec + vw - 1) / vw, h->G.F); }
#define VW_DISPATCH(h, CALL) do { if (vec2(h)) { constexpr int VW = 2; CALL; } else { constexpr int VW = 1; CALL; } } while (0)
// basis-size ladder of the Krylov kernels: KB = 4 | 8 | 16 | 32 >= k
#define KB_DISPATCH(k, CALL)                                                                       \
    do {                                                                                           \
        if ((k) <= 4) { constexpr int KB = 4; CALL; }                                              \
        else if ((k) <= 8) { constexpr int KB = 8; CALL; }                                         \
        else if ((k) <= 16) { constexpr int KB = 16; CALL; }                                       \
        else { constexpr int KB = 32; CALL; }                                                      \
    } while (0)
// number of terms of k_lincomb: NT = 1..6
#define NT_DISPATCH(nt, CALL)                                                                      \
    switch (nt) {                                                                                  \
    case 1: { constexpr int NT = 1; CALL; } break;                                                 \
    case 2: { constexpr int NT = 2; CALL; } break;                                                 \
    case 3: { constexpr int NT = 3; CALL; } break;                                                 \
    case 4: { constexpr int NT = 4; CALL; } break;                                                 \
    case 5: { constexpr int NT = 5; CALL; } break;                                                 \
    default: { constexpr int NT = 6; CALL; } break;                                                \
    }

// want_norm: ||out||^2 lands in h->hres[0] (one reduction instead of a pass of its own)
static int op_lincomb(ksfd_handle *h, int nt, const double *const *x, const double *a, double *out, bool want_norm = false)
{
    double *part = want_norm ? h->part : nullptr;
    KLin L;
    for (int t = 0; t < 6; t++) { L.x[t] = t < nt ? x[t] : nullptr; L.a[t] = t < nt ? a[t] : 0.0; }
    Scope sc(h, KC_LINCOMB, vbytes(h, nt + 1));
    NT_DISPATCH(nt, VW_DISPATCH(h, hipLaunchKernelGGL((k_lincomb<NT, VW>), vgridw(h, VW), dim3(KSFD_BLOCK), 0, h->st, h->kv, L, out, part)));
    HIPCHK(h, hipGetLastError());
    if (want_norm) { const dim3 gr = vgridw(h, vec2(h) ? 2 : 1); return reduce_rows(h, 1, (int)(gr.x * gr.y), 0); }
    return KSFD_OK;
}

// d[0..k) = <w,V_i>, d[k] = <w,w>  -> h->hres
static int op_multidot(ksfd_handle *h, const double *w, const double *V, int k)
{
    if (k > 32) {
        // more basis vectors than one launch takes (restart lengths beyond 32: gmres() grows the restart when a cycle stagnates): chunks
        // of 32, each with its own reduction; <w,w> from the last one
        std::vector<double> acc((size_t)k + 1);
        for (int c0 = 0; c0 < k; c0 += 32) {
            const int kc = std::min(32, k - c0);
            int rc = op_multidot(h, w, V + (int64_t)c0 * h->vlen, kc);
            if (rc) return rc;
            for (int i = 0; i < kc; i++) acc[c0 + i] = h->hres[i];
            acc[k] = h->hres[kc];
        }
        if (k + 1 > 128) return fail(h, KSFD_EINVAL, "op_multidot: %d vectors exceed the result buffer", k);
        for (int i = 0; i <= k; i++) h->hres[i] = acc[i];
        return KSFD_OK;
    }
    const int nb = vec2(h) ? (h->nblk_vec + 1) / 2 : h->nblk_vec;
    {
        Scope sc(h, KC_MULTIDOT, vbytes(h, k + 1));
        KB_DISPATCH(k, VW_DISPATCH(h, hipLaunchKernelGGL((k_multidot<KB, VW>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, h->kv, w, V, h->vlen, k, h->part)));
    }
    HIPCHK(h, hipGetLastError());
    return reduce_rows(h, k + 1, nb, 0);
}

// d[0..k) = <w,V_i>, g[0..k) = <V_{k-1},V_i>, ww  -> h->hres[0..2k]
static int op_multidot_gram(ksfd_handle *h, const double *w, const double *V, int k)
{
    const int nb = vec2(h) ? (h->nblk_vec + 1) / 2 : h->nblk_vec;
    {
        Scope sc(h, KC_MULTIDOT, vbytes(h, k + 1));
        KB_DISPATCH(k, VW_DISPATCH(h, hipLaunchKernelGGL((k_multidot_gram<KB, VW>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, h->kv, w, V, h->vlen, k, h->part)));
    }
    HIPCHK(h, hipGetLastError());
    return reduce_rows(h, 2 * k + 1, nb, 0);
}

static int op_gs_update(ksfd_handle *h, double *w, const double *V, int k, const double *coef, double scale)
{
    if (k > 32) {                        // chunks of 32 basis vectors; the scaling rides in the last one
        for (int c0 = 0; c0 < k; c0 += 32) {
            const int kc = std::min(32, k - c0);
            int rc = op_gs_update(h, w, V + (int64_t)c0 * h->vlen, kc, coef + c0, c0 + kc == k ? scale : 1.0);
            if (rc) return rc;
        }
        return KSFD_OK;
    }
    KCoef C;
    for (int i = 0; i < KSFD_MAXDOT; i++) C.h[i] = i < k ? coef[i] : 0.0;
    Scope sc(h, KC_GSUPDATE, vbytes(h, k + 2));
    KB_DISPATCH(k, VW_DISPATCH(h, hipLaunchKernelGGL((k_gs_update<KB, VW>), vgridw(h, VW), dim3(KSFD_BLOCK), 0, h->st, h->kv, w, V, h->vlen, k, C, scale)));
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

static int op_basis_axpy(ksfd_handle *h, double *x, const double *V, int k, const double *coef, double beta, bool want_norm = false)
{
    if (k > 32) {                        // chunks of 32 basis vectors: beta applies to the first, the norm comes with the last
        for (int c0 = 0; c0 < k; c0 += 32) {
            const int kc = std::min(32, k - c0);
            int rc = op_basis_axpy(h, x, V + (int64_t)c0 * h->vlen, kc, coef + c0, c0 == 0 ? beta : 1.0, want_norm && c0 + kc == k);
            if (rc) return rc;
        }
        return KSFD_OK;
    }
    double *part = want_norm ? h->part : nullptr;
    KCoef C;
    int nread = 0;                                      // vectors with a zero coefficient are not loaded
    for (int i = 0; i < KSFD_MAXDOT; i++) { C.h[i] = i < k ? coef[i] : 0.0; nread += C.h[i] != 0.0; }
    Scope sc(h, KC_BASISAXPY, vbytes(h, nread + 1 + (beta != 0.0)));
    KB_DISPATCH(k, VW_DISPATCH(h, hipLaunchKernelGGL((k_basis_axpy<KB, VW>), vgridw(h, VW), dim3(KSFD_BLOCK), 0, h->st, h->kv, x, V, h->vlen, k, C, beta, part)));
    HIPCHK(h, hipGetLastError());
    if (want_norm) { const dim3 gr = vgridw(h, vec2(h) ? 2 : 1); return reduce_rows(h, 1, (int)(gr.x * gr.y), 0); }
    return KSFD_OK;
}

// V[:, 0:nout] <- V[:, 0:nin] * P in place (k_basis_rotate): P row-major on the host, nin x nout with row stride ldp.  Same index range
// as op_basis_axpy (owned points; ghost rows untouched), booked with the Gram-Schmidt updates.  The coefficients travel through a pinned
// staging buffer of the handle: every caller has waited on the stream (a reduction result, a download) since the previous rotation.
static int op_basis_rotate(ksfd_handle *h, double *V, int nin, int nout, const double *P, int ldp)
{
    if (nin < 1 || nout < 1 || nout > nin || nin > KSFD_ROT_MAXIN || nout > KSFD_ROT_MAXOUT || ldp < nout || ldp > KSFD_ROT_MAXOUT)
        return fail(h, KSFD_EINVAL, "basis rotation %d -> %d vectors (row stride %d) outside 1 <= nout <= %d, nout <= nin <= %d", nin, nout, ldp, KSFD_ROT_MAXOUT, KSFD_ROT_MAXIN);
    const size_t nP = (size_t)KSFD_ROT_MAXIN * KSFD_ROT_MAXOUT;
    if (!h->dr_P && hipMalloc((void **)&h->dr_P, sizeof(double) * nP) != hipSuccess) { h->dr_P = nullptr; return fail(h, KSFD_ENOMEM, "hipMalloc of the rotation matrix failed"); }
    if (!h->dr_Phost && hipHostMalloc((void **)&h->dr_Phost, sizeof(double) * nP, hipHostMallocDefault) != hipSuccess) { h->dr_Phost = nullptr; return fail(h, KSFD_ENOMEM, "hipHostMalloc of the rotation matrix failed"); }
    if (P) {                                            // NULL: the matrix of the previous call is still on the device (Zb follows V)
        memcpy(h->dr_Phost, P, sizeof(double) * (size_t)nin * ldp);
        HIPCHK(h, hipMemcpyAsync(h->dr_P, h->dr_Phost, sizeof(double) * (size_t)nin * ldp, hipMemcpyHostToDevice, h->st));
    }
    Scope sc(h, KC_GSUPDATE, vbytes(h, nin + nout));
#define ROT_LAUNCH(NO) VW_DISPATCH(h, hipLaunchKernelGGL((k_basis_rotate<NO, VW>), vgridw(h, VW), dim3(KSFD_BLOCK), 0, h->st, h->kv, V, (long long)h->vlen, nin, nout, (const double *)h->dr_P, ldp))
    if (nout <= 4) ROT_LAUNCH(4);
    else if (nout <= 8) ROT_LAUNCH(8);
    else if (nout <= 12) ROT_LAUNCH(12);
    else ROT_LAUNCH(KSFD_ROT_MAXOUT);
#undef ROT_LAUNCH
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

static int op_copy(ksfd_handle *h, double *dst, const double *src)
{
    Scope sc(h, KC_MISC, vbytes(h, 2));
    HIPCHK(h, hipMemcpyAsync(dst, src, sizeof(double) * (size_t)h->vlen, hipMemcpyDeviceToDevice, h->st));
    return KSFD_OK;
}

// ---- host <-> device vectors -------------------------------------------------------------------
static int upload(ksfd_handle *h, const double *host, int layout, double *dev)
{
    const KGeom &G = h->G;
    if (layout < 0 || layout > 2) return fail(h, KSFD_EINVAL, "bad layout %d", layout);
    HIPCHK(h, hipMemcpyAsync(h->flat, host, sizeof(double) * (size_t)G.F * G.nloc, hipMemcpyHostToDevice, h->st));
    Scope sc(h, KC_MISC, vbytes(h, 2));
    hipLaunchKernelGGL(k_from_host_layout, vgrid(h), dim3(KSFD_BLOCK), 0, h->st, G, layout, h->flat, dev, G.plane,
                       (long long)G.ng * G.inner);
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}
static int download(ksfd_handle *h, const double *dev, int layout, double *host)
{
    const KGeom &G = h->G;
    if (layout < 0 || layout > 2) return fail(h, KSFD_EINVAL, "bad layout %d", layout);
    {
        Scope sc(h, KC_MISC, vbytes(h, 2));
        hipLaunchKernelGGL(k_to_host_layout, vgrid(h), dim3(KSFD_BLOCK), 0, h->st, G, layout, dev, G.plane,
                           (long long)G.ng * G.inner, h->flat);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(host, h->flat, sizeof(double) * (size_t)G.F * G.nloc, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return KSFD_OK;
}
