// libksfd_hip.so -- C ABI (include/ksfd_hip.h) and the attempt loop of the Rosenbrock-W step (ksfd_step); handle, launch wrappers,
// multigrid and Krylov solvers live in handle.hip.h / ops.hip.h / mg_host.hip.h / krylov.hip.h, the parts of a step attempt in
// step.hip.h (one translation unit), the step's decisions and its step-to-step memory (StepMemo) as plain C++ in step_control.h, the
// record of which derived data is current (h->cur) and the events that write it in handle_state.h.
// Together they stand in for petsc4py TS.step() in the reference (KSFD/ksfdts.py:211).
// gfx950 only.  No CPU fallback: every entry point runs HIP kernels or fails.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/ksfd_hip.h"
#include "stencil.hip.h"
#include "mg.hip.h"
#include "spectral.hip.h"
#include "lu.hip.h"
#include "banded.hip.h"
#include "transport.h"
#include "step_control.h"
#include "mg_coarse_plan.h"
#include "mg_agglomerate_plan.h"
#include "mg_tail_plan.h"

#include "handle.hip.h"
#include "ops.hip.h"
#include "spectral_host.hip.h"
#include "mg_host.hip.h"
#include "krylov.hip.h"
#include "krylov_dr.hip.h"
#include "lu_host.hip.h"
#include "banded_host.hip.h"
#include "step.hip.h"

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" const char *ksfd_last_error(const ksfd_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

extern "C" void ksfd_destroy(ksfd_handle *h)
{
    if (!h) return;
    hipSetDevice(h->device);
    if (h->st) hipStreamSynchronize(h->st);
    double *bufs[] = { h->bstore, h->ckpt, h->Zb, h->pvec, h->coef, h->u, h->usave, h->Z, h->bvec, h->Y, h->V, h->t1, h->t2, h->t3, h->errv, h->Gb, h->dGb, h->flat, h->part, h->dres };
    for (double *b : bufs) if (b) hipFree(b);
    for (int s = 0; s < 4; s++) for (int c = 0; c <= KSFD_MAXL; c++) if (h->src[s][c]) hipFree(h->src[s][c]);
    if (h->coef32) hipFree(h->coef32);
    if (h->hres) hipHostFree(h->hres);
    if (h->pub_count) hipFree(h->pub_count);
    if (h->gm_host) hipHostFree(h->gm_host);
    if (h->gm_dev) hipFree(h->gm_dev);
    if (h->dr_P) hipFree(h->dr_P);
    if (h->dr_Phost) hipHostFree(h->dr_Phost);
    for (auto e : h->gm_ev) if (e) hipEventDestroy(e);
    for (auto &p : h->pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (auto e : h->pool) hipEventDestroy(e);
    if (h->st_io) { hipStreamSynchronize(h->st_io); hipStreamDestroy(h->st_io); }
    for (int q = 0; q < 2; q++) {
        if (h->snap_dev[q]) hipFree(h->snap_dev[q]);
        if (h->snap_host[q]) hipHostFree(h->snap_host[q]);
        if (h->snap_ready[q]) hipEventDestroy(h->snap_ready[q]);
        if (h->snap_done[q]) hipEventDestroy(h->snap_done[q]);
    }
    mg_free(h);
    spec_free(h);
    direct_free(h);
    banded_free(h);
    delete h->tr;
    if (h->ev_ready) hipEventDestroy(h->ev_ready);
    if (h->ev_halo) hipEventDestroy(h->ev_halo);
    if (h->st_comm) hipStreamDestroy(h->st_comm);
    if (h->st) hipStreamDestroy(h->st);
    delete h;
}

extern "C" int ksfd_create(const ksfd_config *cfg, const ksfd_dist *dist, ksfd_handle **out)
{
    if (!cfg || !out) return fail(nullptr, KSFD_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->dim < 1 || cfg->dim > 3) return fail(nullptr, KSFD_EINVAL, "dim must be 1, 2 or 3");
    for (int a = 0; a < cfg->dim; a++)
        if (cfg->n[a] < 5) return fail(nullptr, KSFD_EINVAL, "n[%d]=%lld < 5: the width-2 periodic star needs >= 5 points", a, (long long)cfg->n[a]);
    ksfd_handle *h = new ksfd_handle();
    memset(h->src, 0, sizeof h->src);
    memset(&h->prof, 0, sizeof h->prof);
    h->cfg = *cfg;
    // the caller keeps ownership of the tables: the handle holds numeric copies (fill_phys), never these pointers
    h->cfg.lig_group = nullptr; h->cfg.lig_w = h->cfg.lig_s = h->cfg.lig_gamma = h->cfg.lig_D = nullptr;
    h->cfg.grp_alpha = h->cfg.grp_beta = nullptr;
    int rc = fill_phys(h, cfg);
    if (rc) { g_create_error = h->err; delete h; return rc; }
    h->rank = dist ? dist->rank : 0;
    h->size = dist ? dist->size : 1;
    h->device = dist ? dist->device : 0;
    if (h->size < 1 || h->rank < 0 || h->rank >= h->size) { delete h; return fail(nullptr, KSFD_EINVAL, "bad rank/size"); }
    // one rank WITH a transport = a ring of one: ghost units, halo exchange with itself, all-reduce over one rank, the own-piece path of
    // the all-to-alls -- the whole multi-rank code path on a single GPU (how the RCCL transport is exercised on a one-GPU box)
    h->ring = h->size > 1 || (dist && dist->transport != 0);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { delete h; return fail(nullptr, KSFD_EHIP, "no HIP device available (libksfd_hip has no CPU path)"); }
    if (h->device < 0 || h->device >= ndev) { delete h; return fail(nullptr, KSFD_EINVAL, "device %d of %d", h->device, ndev); }
#define CFAIL(code, ...) do { int rc_ = fail(nullptr, code, __VA_ARGS__); ksfd_destroy(h); return rc_; } while (0)
    if (hipSetDevice(h->device) != hipSuccess) CFAIL(KSFD_EHIP, "hipSetDevice(%d) failed", h->device);
    if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess) CFAIL(KSFD_EHIP, "hipStreamCreate failed");
    if (h->ring && (hipStreamCreateWithFlags(&h->st_comm, hipStreamNonBlocking) != hipSuccess ||
                        hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming) != hipSuccess ||
                        hipEventCreateWithFlags(&h->ev_halo, hipEventDisableTiming) != hipSuccess)) CFAIL(KSFD_EHIP, "comm stream/event creation failed");

    KGeom &G = h->G;
    G.dim = cfg->dim; G.F = cfg->nlig + 1;
    const int slow = cfg->dim - 1;
    int64_t nglob = cfg->n[slow];
    if (h->size > 1 && (nglob % h->size != 0 || nglob / h->size < 4))
        CFAIL(KSFD_EINVAL, "slab axis extent %lld must be divisible by %d ranks with >= 4 units each", (long long)nglob, h->size);
    int64_t sloc = nglob / h->size;
    h->slow0 = sloc * h->rank;
    G.ng = h->ring ? 2 : 0;
    G.wrap_slow = !h->ring;
    G.nx = cfg->n[0]; G.ny = cfg->dim >= 2 ? cfg->n[1] : 1; G.nz = cfg->dim >= 3 ? cfg->n[2] : 1;
    if (slow == 0) G.nx = sloc; else if (slow == 1) G.ny = sloc; else G.nz = sloc;
    G.inner = slow == 0 ? 1 : (slow == 1 ? G.nx : G.nx * G.ny);
    G.sloc = sloc;
    G.plane = (sloc + 2 * G.ng) * G.inner;
    G.nloc = sloc * G.inner;
    h->kv.plane = G.plane; h->kv.off = (long long)G.ng * G.inner; h->kv.nloc = G.nloc; h->kv.nf = G.F;
    h->vlen = (int64_t)G.F * G.plane;
    h->nblk_vec = (int)std::min<long long>((G.nloc + KSFD_BLOCK - 1) / KSFD_BLOCK, 2048);
    build_tableau(h);

    // Krylov storage (V: m+1 vectors, Zb: m) is sized to the HBM that is free (ksfd_krylov::restart_fit): m = 30 on anything up to
    // ~12k^2 x 2 fields on a 288 GB MI355X, up to 120 where HBM is plentiful; larger grids run with a shorter restart.
    h->restart_alloc = ksfd_krylov::RESTART_DEFAULT;
    int fit_local = ksfd_krylov::RESTART_DEFAULT;
    {
        size_t mfree = 0, mtotal = 0;
        if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess && mfree > 0) {
            fit_local = ksfd_krylov::restart_fit((double)mfree, 8.0 * (double)h->vlen, env_knobs().restart_cap);
        }
    }
    if (alloc_d(h, &h->dres, 128)) CFAIL(KSFD_ENOMEM, "%s", h->err.c_str());
    if (h->ring) {
        std::string terr;
        h->tr = make_transport(dist, G.F, G.inner, terr);
        if (!h->tr) CFAIL(KSFD_ECOMM, "transport %d: %s", dist->transport, terr.c_str());
        // every rank must run with the SAME restart length (the multi-dot row counts and restart points are part of the
        // collective pattern): take the minimum over the ranks of what each one's free HBM allows
        double v = -(double)fit_local;
        if (hipMemcpyAsync(h->dres, &v, sizeof v, hipMemcpyHostToDevice, h->st) != hipSuccess || h->tr->allreduce(h->dres, 1, 1, h->st))
            CFAIL(KSFD_ECOMM, "agreeing on the restart length failed: %s", h->tr->error().c_str());
        if (h->tr->result_on_host()) v = h->tr->host_result()[0];
        else if (hipMemcpyAsync(&v, h->dres, sizeof v, hipMemcpyDeviceToHost, h->st) != hipSuccess || hipStreamSynchronize(h->st) != hipSuccess)
            CFAIL(KSFD_EHIP, "reading the agreed restart length failed");
        fit_local = (int)(-v + 0.5);
    }
    if (fit_local != ksfd_krylov::RESTART_DEFAULT) {
        if (fit_local < ksfd_krylov::RESTART_MIN) CFAIL(KSFD_ENOMEM, "grid too large for this device: a vector is %.2f GB, the solver needs ~47 of them (restart length that fits: %d)", 8.0 * (double)h->vlen / 1e9, fit_local);
        h->restart_alloc = fit_local;
    }
    double **vecs[] = { &h->u, &h->usave, &h->Z, &h->bvec, &h->t1, &h->t2, &h->t3, &h->errv };
    for (double **v : vecs) {
        if (alloc_d(h, v, h->vlen)) CFAIL(KSFD_ENOMEM, "%s", h->err.c_str());
        hipMemsetAsync(*v, 0, sizeof(double) * (size_t)h->vlen, h->st);
    }
    if (alloc_d(h, &h->Y, 4 * h->vlen) || alloc_d(h, &h->V, (int64_t)(h->restart_alloc + 1) * h->vlen) ||
        alloc_d(h, &h->Gb, G.plane) || alloc_d(h, &h->dGb, G.plane) || alloc_d(h, &h->coef, (int64_t)(3 + cfg->nlig) * G.plane) ||
        alloc_d(h, &h->flat, (int64_t)std::max(G.F, 3) * G.nloc) ||
        alloc_d(h, &h->part, (int64_t)(2 * KSFD_MAXDOT + 4) * 4096))
        CFAIL(KSFD_ENOMEM, "%s", h->err.c_str());
    // flexible-GMRES / spectral-fallback basis: allocated here when the device has room (the sizing above counted it), so that no step
    // pays a multi-GB hipMalloc; if it does not fit now it is tried again on first use
    if (hipMalloc((void **)&h->Zb, sizeof(double) * (size_t)h->restart_alloc * (size_t)h->vlen) != hipSuccess) { h->Zb = nullptr; hipGetLastError(); }
    hipMemsetAsync(h->Y, 0, sizeof(double) * (size_t)(4 * h->vlen), h->st);
    hipMemsetAsync(h->V, 0, sizeof(double) * (size_t)((h->restart_alloc + 1) * h->vlen), h->st);
    if (hipHostMalloc((void **)&h->hres, sizeof(double) * 128 + 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) CFAIL(KSFD_ENOMEM, "hipHostMalloc failed");
    h->pub_flag = reinterpret_cast<unsigned long long *>(h->hres + 128);
    *h->pub_flag = 0;
    if (hipHostGetDevicePointer((void **)&h->hres_dev, h->hres, 0) != hipSuccess || hipMalloc((void **)&h->pub_count, sizeof(unsigned int)) != hipSuccess ||
        hipMemset(h->pub_count, 0, sizeof(unsigned int)) != hipSuccess) h->hres_dev = nullptr;          // zero_copy_on is false from here on
    else h->pub_flag_dev = reinterpret_cast<unsigned long long *>(h->hres_dev + 128);
    {
        const int m = h->restart_alloc;
        const size_t ndev = (size_t)(m + 1) * (m + 1) + (size_t)(m + 1) * m + 2 * m + (m + 1) + KSFD_MAXDOT + 1 + 2 * (m + 1);
        const size_t nhost = 2 * (m + 1) + (size_t)(m + 1) * m + (m + 1);
        if (alloc_d(h, &h->gm_dev, (int64_t)ndev)) CFAIL(KSFD_ENOMEM, "%s", h->err.c_str());
        if (hipHostMalloc((void **)&h->gm_host, sizeof(double) * nhost, hipHostMallocDefault) != hipSuccess) CFAIL(KSFD_ENOMEM, "hipHostMalloc failed");
        h->gm_ev.resize(m + 1);
        for (auto &e : h->gm_ev) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) CFAIL(KSFD_EHIP, "hipEventCreate failed");
    }

    spec_build(h);                                            // leaves spec.ok = false where it does not apply (1-D, extents other than 2^k or 3 * 2^k, other rank counts, ...)
    if (mg_build(h)) { mg_free(h); h->mg_ok = false; }        // out of memory for the hierarchy: run without the multigrid preconditioner
    if ((h->spec.ok || h->mg_ok) && alloc_d(h, &h->bstore, 3 * h->vlen)) { h->bstore = nullptr; h->err.clear(); }     // no stage guesses (plan_stage_forms asks for the buffer)
    if (h->ring) {
        // which solvers exist decides the sequence of collectives of every step: all ranks must agree (an allocation that failed
        // on one rank only would otherwise leave the others waiting in an all-reduce)
        double flags[3] = { h->spec.ok ? 1.0 : 0.0, h->mg_ok ? 1.0 : 0.0, h->bstore ? 1.0 : 0.0 };
        for (double &f : flags) f = -f;                       // MIN through the transport's MAX
        if (hipMemcpyAsync(h->dres, flags, sizeof flags, hipMemcpyHostToDevice, h->st) != hipSuccess || h->tr->allreduce(h->dres, 3, 1, h->st))
            CFAIL(KSFD_ECOMM, "agreeing on the available solvers failed: %s", h->tr->error().c_str());
        if (h->tr->result_on_host()) memcpy(flags, h->tr->host_result(), sizeof flags);
        else if (hipMemcpyAsync(flags, h->dres, sizeof flags, hipMemcpyDeviceToHost, h->st) != hipSuccess || hipStreamSynchronize(h->st) != hipSuccess)
            CFAIL(KSFD_EHIP, "reading the agreed solver flags failed");
        if (flags[0] > -0.5 && h->spec.ok) spec_free(h);
        if (flags[1] > -0.5 && h->mg_ok) { mg_free(h); h->mg_ok = false; }
        if (flags[2] > -0.5 && h->bstore) { hipFree(h->bstore); h->bstore = nullptr; }
    }
    if (hipStreamSynchronize(h->st) != hipSuccess) CFAIL(KSFD_EHIP, "stream sync failed in create");
#undef CFAIL
    *out = h;
    return KSFD_OK;
}

extern "C" int ksfd_rccl_unique_id(void *out128)
{
    if (!out128) return KSFD_EINVAL;
    std::string err;
    RcclApi api;
    if (!api.load(err)) return fail(nullptr, KSFD_ECOMM, "%s", err.c_str());
    auto getid = (decltype(&ncclGetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
    if (!getid) return fail(nullptr, KSFD_ECOMM, "librccl lacks ncclGetUniqueId");
    ncclUniqueId id;
    ncclResult_t r = getid(&id);
    if (r != ncclSuccess) return fail(nullptr, KSFD_ECOMM, "ncclGetUniqueId: %s", api.GetErrorString(r));
    memcpy(out128, &id, sizeof id);
    return KSFD_OK;
}

extern "C" int ksfd_update_params(ksfd_handle *h, const ksfd_config *cfg)
{
    if (!h || !cfg) return KSFD_EINVAL;
    if (cfg->dim != h->cfg.dim || cfg->nlig != h->cfg.nlig) return fail(h, KSFD_EINVAL, "update_params cannot change dim/nlig");
    for (int a = 0; a < 3; a++) if (cfg->n[a] != h->cfg.n[a]) return fail(h, KSFD_EINVAL, "update_params cannot change the grid");
    h->cfg = *cfg;
    h->cfg.lig_group = nullptr; h->cfg.lig_w = h->cfg.lig_s = h->cfg.lig_gamma = h->cfg.lig_D = nullptr;
    h->cfg.grp_alpha = h->cfg.grp_beta = nullptr;
    ksfd_ctl::params_changed(h->cur);
    return fill_phys(h, cfg);
}

extern "C" int ksfd_set_stage_params(ksfd_handle *h, int32_t stage, const ksfd_config *cfg)
{
    if (!h || stage < -1 || stage > 3) return KSFD_EINVAL;
    if (!cfg) {                                            // clear: the stages use the handle's parameters again
        for (int s = 0; s < 4; s++) if (stage == -1 || s == stage) h->Pst_valid[s] = false;
        return KSFD_OK;
    }
    if (cfg->dim != h->cfg.dim || cfg->nlig != h->cfg.nlig) return fail(h, KSFD_EINVAL, "set_stage_params cannot change dim/nlig");
    for (int a = 0; a < 3; a++) if (cfg->n[a] != h->cfg.n[a] || cfg->L[a] != h->cfg.L[a]) return fail(h, KSFD_EINVAL, "set_stage_params cannot change the grid");
    for (int s = 0; s < 4; s++) {
        if (stage != -1 && s != stage) continue;
        int rc = fill_phys(h, cfg, &h->Pst[s]);
        if (rc) return rc;
        h->Pst_valid[s] = true;
    }
    return KSFD_OK;
}

extern "C" int ksfd_local_range(const ksfd_handle *h, int64_t *b, int64_t *e)
{
    if (!h) return KSFD_EINVAL;
    if (b) *b = h->slow0;
    if (e) *e = h->slow0 + h->G.sloc;
    return KSFD_OK;
}
extern "C" int64_t ksfd_local_size(const ksfd_handle *h) { return h ? (int64_t)h->G.F * h->G.nloc : 0; }
// the pointer is good until the next ksfd_step (an accepted step moves the state to the handle's other buffer); handing it out ends the
// floor proof of the values it points at, and only that (handle_state.h: state_handed_out)
extern "C" double *ksfd_device_state(ksfd_handle *h) { if (h) ksfd_ctl::state_handed_out(h->cur); return h ? h->u : nullptr; }
extern "C" int64_t ksfd_device_plane_stride(const ksfd_handle *h) { return h ? h->G.plane : 0; }
extern "C" int64_t ksfd_device_interior_offset(const ksfd_handle *h) { return h ? (int64_t)h->G.ng * h->G.inner : 0; }

extern "C" int ksfd_set_state(ksfd_handle *h, const double *u, int32_t layout)
{
    if (!h || !u) return KSFD_EINVAL;
    hipSetDevice(h->device);
    int rc = upload(h, u, layout, h->u);
    ksfd_ctl::state_written(h->cur);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->st));
    return KSFD_OK;
}
// Asynchronous read-out of the resident state for writers ("next" row f2: TimeSeries fed from the device without
// stalling the stepper).  _begin: the layout transform runs on the compute stream (ordered after everything issued so
// far, ~0.1 ms at 4096^2) into one of two device staging slots; the D2H copy into pinned memory runs on a third stream.
// _wait: blocks until that copy has landed and hands out the pinned buffer (F*nlocal doubles), valid until the slot is
// used again, i.e. until the second-next _begin.  A slot whose data nobody waited for is simply overwritten.
extern "C" int ksfd_snapshot_begin(ksfd_handle *h, int32_t layout, int32_t *slot)
{
    if (!h || !slot) return KSFD_EINVAL;
    if (layout < 0 || layout > 2) return fail(h, KSFD_EINVAL, "bad layout %d", layout);
    hipSetDevice(h->device);
    const KGeom &G = h->G;
    const size_t bytes = sizeof(double) * (size_t)G.F * G.nloc;
    if (!h->st_io) {
        if (hipStreamCreateWithFlags(&h->st_io, hipStreamNonBlocking) != hipSuccess) return fail(h, KSFD_EHIP, "hipStreamCreate (io) failed");
        for (int q = 0; q < 2; q++) {
            if (hipMalloc((void **)&h->snap_dev[q], bytes) != hipSuccess || hipHostMalloc((void **)&h->snap_host[q], bytes, hipHostMallocDefault) != hipSuccess)
                return fail(h, KSFD_ENOMEM, "snapshot staging buffers (%zu bytes each) could not be allocated", bytes);
            if (hipEventCreateWithFlags(&h->snap_ready[q], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&h->snap_done[q], hipEventDisableTiming) != hipSuccess) return fail(h, KSFD_EHIP, "hipEventCreate failed");
        }
    }
    const int q = h->snap_next;
    h->snap_next ^= 1;
    if (h->snap_busy[q]) HIPCHK(h, hipEventSynchronize(h->snap_done[q]));      // its previous copy must have left the staging slot
    {
        Scope sc(h, KC_MISC, vbytes(h, 2));
        hipLaunchKernelGGL(k_to_host_layout, vgrid(h), dim3(KSFD_BLOCK), 0, h->st, G, layout, (const double *)h->u, G.plane,
                           (long long)G.ng * G.inner, h->snap_dev[q]);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->snap_ready[q], h->st));
    HIPCHK(h, hipStreamWaitEvent(h->st_io, h->snap_ready[q], 0));
    HIPCHK(h, hipMemcpyAsync(h->snap_host[q], h->snap_dev[q], bytes, hipMemcpyDeviceToHost, h->st_io));
    HIPCHK(h, hipEventRecord(h->snap_done[q], h->st_io));
    h->snap_busy[q] = true;
    *slot = q;
    return KSFD_OK;
}

extern "C" int ksfd_snapshot_wait(ksfd_handle *h, int32_t slot, const double **host)
{
    if (!h || !host || slot < 0 || slot > 1) return KSFD_EINVAL;
    if (!h->snap_busy[slot]) return fail(h, KSFD_EINVAL, "snapshot slot %d holds nothing", slot);
    hipSetDevice(h->device);
    HIPCHK(h, hipEventSynchronize(h->snap_done[slot]));
    *host = h->snap_host[slot];
    return KSFD_OK;
}

extern "C" int ksfd_checkpoint(ksfd_handle *h, int32_t op)
{
    if (!h || op < 0 || op > 1) return KSFD_EINVAL;
    hipSetDevice(h->device);
    if (op == 0) {
        if (!h->ckpt && alloc_d(h, &h->ckpt, h->vlen)) return KSFD_ENOMEM;
        HIPCHK(h, hipMemcpyAsync(h->ckpt, h->u, sizeof(double) * (size_t)h->vlen, hipMemcpyDeviceToDevice, h->st));
        h->ckpt_memo = h->memo;
        ksfd_ctl::checkpoint_saved(h->cur);
        mg_setup_cold(h);                                // the step after a save and the step after a restore both set the hierarchy up cold: replays stay bitwise
        h->ckpt_valid = true;
        return KSFD_OK;
    }
    if (!h->ckpt_valid) return fail(h, KSFD_EINVAL, "no checkpoint has been saved");
    HIPCHK(h, hipMemcpyAsync(h->u, h->ckpt, sizeof(double) * (size_t)h->vlen, hipMemcpyDeviceToDevice, h->st));
    h->memo = h->ckpt_memo;
    ksfd_ctl::checkpoint_restored(h->cur);
    mg_setup_cold(h);
    return KSFD_OK;
}

extern "C" int ksfd_set_state_random(ksfd_handle *h, const int64_t *nc, const double *z, double rho0)
{
    if (!h || !nc || !z) return KSFD_EINVAL;
    hipSetDevice(h->device);
    int64_t n = 1;
    for (int a = 0; a < 3; a++) {
        if (a < h->G.dim ? nc[a] < 1 : nc[a] != 1) return fail(h, KSFD_EINVAL, "coarse grid must be >= 1 per used axis and 1 elsewhere");
        n *= nc[a];
    }
    double *dz = nullptr;
    ksfd_ctl::state_written(h->cur);
    if (hipMalloc((void **)&dz, sizeof(double) * (size_t)n) != hipSuccess) return fail(h, KSFD_ENOMEM, "hipMalloc of the coarse samples failed");
    hipError_t e = hipMemcpyAsync(dz, z, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->st);
    const KGeom &G = h->G;
    int nb = (int)std::min<long long>((G.nloc + KSFD_BLOCK - 1) / KSFD_BLOCK, 65535);
    if (e == hipSuccess) {
        Scope sc(h, KC_MISC, vbytes(h, 1));
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_random_start<NL>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, G, h->P, (long long)h->cfg.n[G.dim - 1],
                                                  (long long)h->slow0, (long long)nc[0], (long long)nc[1], (long long)nc[2], (const double *)dz, rho0, h->u));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->st);
    hipFree(dz);
    if (e != hipSuccess) return fail(h, KSFD_EHIP, "random start: %s", hipGetErrorString(e));
    return KSFD_OK;
}
extern "C" int ksfd_get_state(ksfd_handle *h, double *u, int32_t layout)
{
    if (!h || !u) return KSFD_EINVAL;
    hipSetDevice(h->device);
    return download(h, h->u, layout, u);
}

extern "C" int ksfd_set_source(ksfd_handle *h, int32_t stage, int32_t field, const double *srch, int32_t layout)
{
    if (!h || field < 0 || field >= h->G.F || stage < -1 || stage > 3) return h ? fail(h, KSFD_EINVAL, "bad stage/field") : KSFD_EINVAL;
    if (layout != KSFD_LAYOUT_SOA) return fail(h, KSFD_EINVAL, "sources are single dense planes: pass layout SOA");
    hipSetDevice(h->device);
    for (int s = 0; s < 4; s++) {
        if (stage != -1 && s != stage) continue;
        if (!srch) {
            if (h->src[s][field]) { HIPCHK(h, hipStreamSynchronize(h->st)); hipFree(h->src[s][field]); h->src[s][field] = nullptr; }
            continue;
        }
        if (!h->src[s][field] && alloc_d(h, &h->src[s][field], h->G.nloc)) return KSFD_ENOMEM;
        HIPCHK(h, hipMemcpyAsync(h->src[s][field], srch, sizeof(double) * (size_t)h->G.nloc, hipMemcpyHostToDevice, h->st));
    }
    HIPCHK(h, hipStreamSynchronize(h->st));
    return KSFD_OK;
}

extern "C" int ksfd_rhs(ksfd_handle *h, double t, const double *uh, double *outh, int32_t layout)
{
    (void)t;   // sources(t) are uploaded by the caller (ksfd_set_source); constants via ksfd_update_params
    if (!h || !outh) return KSFD_EINVAL;
    hipSetDevice(h->device);
    int rc;
    double *uin = h->u;
    if (uh) { if ((rc = upload(h, uh, layout, h->t1))) return rc; uin = h->t1; }
    if ((rc = halo(h, uin))) return rc;
    if ((rc = op_rhs(h, uin, 0, h->t3))) return rc;
    return download(h, h->t3, layout, outh);
}

extern "C" int ksfd_jvp(ksfd_handle *h, const double *uh, const double *vh, double *outh, int32_t layout)
{
    if (!h || !vh || !outh) return KSFD_EINVAL;
    hipSetDevice(h->device);
    int rc;
    double *uin = h->u;
    if (uh) { if ((rc = upload(h, uh, layout, h->t1))) return rc; uin = h->t1; }
    if ((rc = upload(h, vh, layout, h->t2))) return rc;
    if ((rc = halo(h, uin)) || (rc = halo(h, h->t2))) return rc;
    if (!uh && h->tune.use_frozen) {
        // the path the stepper uses: coefficients of the stored state once, then the frozen-coefficient kernels
        if ((rc = ensure_coef(h, true))) return rc;
        if ((rc = op_jvp_frozen(h, h->t2, 0, 0.0, h->t3))) return rc;
    } else if ((rc = op_jvp(h, uin, h->t2, 0, 0.0, h->t3))) return rc;
    return download(h, h->t3, layout, outh);
}

static int velocity_common(ksfd_handle *h, const double *uin, double *vel_dev, double vmax[3])
{
    const KGeom &G = h->G;
    int rc;
    const double *Gplane = h->Gb;
    if (uin == h->u && h->tune.use_frozen) {
        // the G plane of the resident state is plane 1 of the frozen coefficient planes; the next step reuses them
        if ((rc = ensure_coef(h))) return rc;
        Gplane = h->coef + G.plane;
    } else {
        if ((rc = halo(h, (double *)uin))) return rc;
        Scope sc(h, KC_GFIELD, 8.0 * (G.F + 1) * (double)G.plane);
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_gfield<NL, false>), dim3(plane_blocks(G)), dim3(KSFD_BLOCK), 0, h->st, G, h->P, uin, (const double *)nullptr, h->Gb, (double *)nullptr));
    }
    int nb = (int)std::min<long long>((G.nloc + KSFD_BLOCK - 1) / KSFD_BLOCK, 1024);
    if (vmax && !vel_dev && G.dim == 2 && (G.nx % 2 == 0) && G.nx >= 4) {
        // CFL check: max|dG/dx|, max|dG/dy| only -- row-structured kernel, 16-B loads, no 64-bit divisions
        const int bx = (int)((G.nx / 2 + KSFD_BLOCK - 1) / KSFD_BLOCK), by = (int)std::min<long long>(G.sloc, std::max(1, 2048 / bx));
        nb = bx * by;
        Scope sc(h, KC_VELOCITY, 8.0 * (double)G.nloc);
        hipLaunchKernelGGL(k_velmax2d, dim3(bx, by), dim3(KSFD_BLOCK), 0, h->st, G, h->P, Gplane, h->part);
    } else if (vmax && !vel_dev && G.dim == 3 && (G.nx % 2 == 0) && G.nx >= 4 && G.ny >= 4 && G.nx * G.ny < (1LL << 30)) {
        const int bx = (int)((G.nx / 2 * G.ny + KSFD_BLOCK - 1) / KSFD_BLOCK);
        int zseg = (int)G.sloc;                               // enough blocks to fill the chip, segments of >= 8 planes (4 extra loads each)
        while (zseg >= 32 && (long long)bx * ((G.sloc + zseg - 1) / zseg) < 8192) zseg = (zseg + 1) / 2;
        const int by = (int)((G.sloc + zseg - 1) / zseg);
        nb = bx * by;
        if (3LL * nb > part_capacity()) return fail(h, KSFD_EINVAL, "velocity_max: grid too large for the partial-result buffer");
        Scope sc(h, KC_VELOCITY, 8.0 * (double)G.nloc);
        hipLaunchKernelGGL(k_velmax3d, dim3(bx, by), dim3(KSFD_BLOCK), 0, h->st, G, h->P, zseg, Gplane, h->part);
    } else {
        Scope sc(h, KC_VELOCITY, 8.0 * (double)G.nloc * (1 + (vel_dev ? G.dim : 0)));
        hipLaunchKernelGGL(k_velocity, dim3(nb), dim3(KSFD_BLOCK), 0, h->st, G, h->P, Gplane, vel_dev, vmax ? h->part : (double *)nullptr);
    }
    HIPCHK(h, hipGetLastError());
    if (vmax) {
        if ((rc = reduce_rows(h, 3, nb, 1))) return rc;
        for (int a = 0; a < 3; a++) vmax[a] = a < G.dim ? h->hres[a] : 0.0;
    }
    return KSFD_OK;
}

extern "C" int ksfd_velocity(ksfd_handle *h, const double *uh, double *velh, int32_t layout)
{
    if (!h || !velh) return KSFD_EINVAL;
    if (layout != KSFD_LAYOUT_SOA) return fail(h, KSFD_EINVAL, "velocity output is dim dense SoA planes: pass layout SOA for it");
    hipSetDevice(h->device);
    int rc;
    double *uin = h->u;
    if (uh) { if ((rc = upload(h, uh, layout, h->t1))) return rc; uin = h->t1; }
    if ((rc = velocity_common(h, uin, h->flat, nullptr))) return rc;
    HIPCHK(h, hipMemcpyAsync(velh, h->flat, sizeof(double) * (size_t)h->G.dim * h->G.nloc, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return KSFD_OK;
}

extern "C" int ksfd_velocity_max(ksfd_handle *h, double vmax[3])
{
    if (!h || !vmax) return KSFD_EINVAL;
    hipSetDevice(h->device);
    return velocity_common(h, h->u, nullptr, vmax);
}

extern "C" int ksfd_groom(ksfd_handle *h)
{
    if (!h) return KSFD_EINVAL;
    hipSetDevice(h->device);
    Scope sc(h, KC_MISC, vbytes(h, 2));
    hipLaunchKernelGGL(k_groom, vgrid(h), dim3(KSFD_BLOCK), 0, h->st, h->kv, h->u, h->P.rhomin, h->P.Umin);
    HIPCHK(h, hipGetLastError());
    ksfd_ctl::state_groomed(h->cur);
    return KSFD_OK;
}

extern "C" int ksfd_count_worms(ksfd_handle *h, double *total)
{
    if (!h || !total) return KSFD_EINVAL;
    hipSetDevice(h->device);
    {
        Scope sc(h, KC_MISC, 8.0 * (double)h->G.nloc);
        hipLaunchKernelGGL(k_sum_rho, dim3(h->nblk_vec), dim3(KSFD_BLOCK), 0, h->st, h->kv, h->u, h->part);
    }
    HIPCHK(h, hipGetLastError());
    int rc = reduce_rows(h, 1, h->nblk_vec, 0);
    if (rc) return rc;
    *total = h->hres[0];
    return KSFD_OK;
}

extern "C" int ksfd_scale_rho(ksfd_handle *h, double factor)
{
    if (!h) return KSFD_EINVAL;
    hipSetDevice(h->device);
    ksfd_ctl::state_written(h->cur);
    Scope sc(h, KC_MISC, 16.0 * (double)h->G.nloc);
    hipLaunchKernelGGL(k_mul_rho, dim3(h->nblk_vec), dim3(KSFD_BLOCK), 0, h->st, h->kv, h->u, (const double *)nullptr, factor);
    HIPCHK(h, hipGetLastError());
    return KSFD_OK;
}

extern "C" int ksfd_mul_rho(ksfd_handle *h, const double *fh)
{
    if (!h || !fh) return KSFD_EINVAL;
    hipSetDevice(h->device);
    HIPCHK(h, hipMemcpyAsync(h->flat, fh, sizeof(double) * (size_t)h->G.nloc, hipMemcpyHostToDevice, h->st));
    ksfd_ctl::state_written(h->cur);
    Scope sc(h, KC_MISC, 24.0 * (double)h->G.nloc);
    hipLaunchKernelGGL(k_mul_rho, dim3(h->nblk_vec), dim3(KSFD_BLOCK), 0, h->st, h->kv, h->u, (const double *)h->flat, 1.0);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->st));
    return KSFD_OK;
}

// Assembled Jacobian export (row f4 of the scope table; kernel k_jac_csr in stencil.hip.h)
extern "C" int ksfd_jacobian_nnz(ksfd_handle *h, int64_t *nrows, int64_t *nnz)
{
    if (!h) return KSFD_EINVAL;
    const int64_t npts = 4 * h->G.dim + 1;
    if (nrows) *nrows = (int64_t)h->G.F * h->G.nloc;
    if (nnz) *nnz = h->G.nloc * ((int64_t)h->G.F * npts + (int64_t)h->P.nlig * (npts + 1));
    return KSFD_OK;
}

extern "C" int ksfd_jacobian_csr(ksfd_handle *h, int64_t *rowptr, int64_t *col, double *val)
{
    if (!h || !rowptr || !col || !val) return KSFD_EINVAL;
    hipSetDevice(h->device);
    int64_t nrows, nnz;
    ksfd_jacobian_nnz(h, &nrows, &nnz);
    int rc;
    if ((rc = ensure_coef(h))) return rc;                    // clamps like groom
    long long *dcol = nullptr;
    double *dval = nullptr;
    if (hipMalloc((void **)&dcol, sizeof(long long) * (size_t)nnz) != hipSuccess ||
        hipMalloc((void **)&dval, sizeof(double) * (size_t)nnz) != hipSuccess) {
        if (dcol) hipFree(dcol);
        return fail(h, KSFD_ENOMEM, "hipMalloc of the CSR staging buffers failed");
    }
    const KGeom &G = h->G;
    int nb = (int)std::min<long long>((G.nloc + KSFD_BLOCK - 1) / KSFD_BLOCK, 65535);
    {
        Scope sc(h, KC_MISC, 16.0 * (double)nnz + 8.0 * (3 + h->P.nlig) * (double)G.nloc);
        NL_DISPATCH(h->P.nlig, hipLaunchKernelGGL((k_jac_csr<NL>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, G, h->P, (const double *)h->coef,
                                                  (long long)h->cfg.n[G.dim - 1], (long long)h->slow0, dcol, dval));
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(col, dcol, sizeof(long long) * (size_t)nnz, hipMemcpyDeviceToHost, h->st);
    if (e == hipSuccess) e = hipMemcpyAsync(val, dval, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, h->st);
    if (e == hipSuccess) e = hipStreamSynchronize(h->st);
    hipFree(dcol);
    hipFree(dval);
    if (e != hipSuccess) return fail(h, KSFD_EHIP, "jacobian export: %s", hipGetErrorString(e));
    // row pointers are a fixed pattern: rho row F*npts entries, each U row npts+1
    const int64_t npts = 4 * G.dim + 1, F = G.F, per = F * npts + (F - 1) * (npts + 1);
    for (int64_t p = 0; p < G.nloc; p++) {
        rowptr[p * F] = p * per;
        for (int64_t l = 1; l < F; l++) rowptr[p * F + l] = p * per + F * npts + (l - 1) * (npts + 1);
    }
    rowptr[nrows] = nnz;
    return KSFD_OK;
}


// ------------------------------------------------------------------------------------------------
extern "C" void ksfd_default_step_opts(ksfd_step_opts *o)
{
    memset(o, 0, sizeof *o);
    o->rtol = 1e-5; o->atol = 1e-5;           // KSFD/ksfdts.py:66-67 defaults
    o->adapt = 1; o->max_reject = 10;
    o->clip_lo = 0.1; o->clip_hi = 5.0;       // -ts_adapt_clip 0.1,5
    o->dt_min = 1e-20; o->dt_max = 1e4;       // -ts_adapt_dt_min/-ts_adapt_dt_max
    o->safety = 0.9; o->reject_safety = 0.5;  // PETSc TSAdaptBasic defaults
    // relative residual 1e-6: the fields then agree with a 1e-12 solve to ~1e-10 rel-L2 over several steps
    // (tools/acc_vs_ksp.py); the north-star tolerance is 1e-8.  PETSc's own KSP default is 1e-5.
    o->ksp_rtol = 1e-6; o->ksp_atol = 1e-50;
    o->ksp_restart = 30; o->ksp_max_it = 2000;
    o->pc_type = 2;    // 0 none, 1 multigrid always, 2 multigrid when the step is stiff (2-D, single rank)
}

// One TSStep_RosW attempt loop (PETSc rosw.c restated; tableau/derivation in oracle/ksfd_oracle.c) over the parts in step.hip.h.
// Grooms the state where that can change it, then tries step sizes until the controller accepts one: plan, four stages, the solvers' own
// adaptation, completion with the embedded error norm, TSAdaptChoose_Basic.  The stages only read h->u and the completion writes the new
// state into h->usave, so an attempt that fails or is rejected has nothing to roll back; acceptance swaps the two pointers.
static int step_run(ksfd_handle *h, double *t, double *hstep, const ksfd_step_opts *opts, bool direct, bool dr_on, ksfd_step_stats &st)
{
    int rc;
    StepMemo &m = h->memo;
    double hh = *hstep;
    bool prev_accept = !(opts->reserved & 4);           // bit 2: the caller's previous attempt of this step was rejected
    bool lam_done = false;
    int rejects = 0;
    const int max_rej = opts->max_reject < 0 ? 0x7fffffff : opts->max_reject;      // PETSc: -ts_max_reject -1 = unlimited
    const bool single = (opts->reserved & 2) != 0;                                   // one attempt per call (the caller owns the reject loop)
    // KSFDTS.solve grooms the global vector before every TS.step (KSFD/ksfdts.py:210)
    // cur.floor_ok: every owned value is at or above its floor already (the last completion counted none below and nothing has written u
    // or moved the floors since), so the groom would store the bits it loads and is left out
    if (!h->cur.floor_ok || h->tune.old_boundary) {
        Scope sc(h, KC_MISC, vbytes(h, 2));
        hipLaunchKernelGGL(k_groom, vgrid(h), dim3(KSFD_BLOCK), 0, h->st, h->kv, h->u, h->P.rhomin, h->P.Umin);
        if (hipGetLastError() != hipSuccess) return fail(h, KSFD_EHIP, "k_groom launch failed");
        ksfd_ctl::state_groomed(h->cur);
    }
    if ((rc = halo(h, h->u))) return rc;
    if (h->tune.use_frozen && (rc = ensure_coef(h, true))) return rc;      // usually already there: the CFL check after the last step made them
    ksfd_ctl::step_begins(h->cur);
    m.nsteps++;
    ksfd_ctl::spec_rho_roll(m);                      // contraction memory of the spectral sweeps
    while (true) {
        AttemptPlan p;
        if ((rc = plan_attempt(h, opts, hh, direct, dr_on, lam_done, p))) return rc;
        const int its_before = st.linear_its;
        bool spec_failed = false;
        ksfd_ctl::attempt_begins(h->cur);
        rc = step_attempt(h, opts, p, spec_failed, st);
        const int its = st.linear_its - its_before;
        if (p.use_spec && opts->pc_type == 2) ksfd_ctl::spec_backoff_update(m, spec_failed, its, m.nsteps);
        if (!rc && p.use_pc && !env_knobs().pc_sigma_set)      // online search for the shift floor, unless KSFD_PC_SIGMA fixes it
            ksfd_ctl::shift_floor_update(m, (double)its, p.shift);
        if (rc == KSFD_ELINEAR && opts->adapt && !single && rejects < max_rej && hh * 0.25 >= opts->dt_min) {
            // PETSc's -ts_adapt_scale_solve_failed (0.25): a failed solve rejects the step and quarters it.  The
            // reference disables that by setMaxSNESFailures(1) (KSFD/ksfdts.py:135) because its LU cannot fail this
            // way; an iterative solve can, and aborting a long run for it would not be a service.
            rejects++;
            st.rejections = rejects;
            prev_accept = false;
            hh *= 0.25;
            *hstep = hh;
            continue;
        }
        if (rc) { hipStreamSynchronize(h->st); return rc; }
        double below = 0.0;
        if ((rc = step_finish(h, opts, &st.wrms, &below))) return rc;
        if (!(st.wrms == st.wrms) || isinf(st.wrms)) {
            hipStreamSynchronize(h->st);
            return fail(h, KSFD_ENAN, "non-finite error norm at t=%g h=%g", *t, hh);
        }
        ksfd_ctl::AdaptChoice next = { true, hh };
        if (opts->adapt) next = ksfd_ctl::adapt_basic(hh, st.wrms, prev_accept, opts->safety, opts->reject_safety, opts->clip_lo, opts->clip_hi, opts->dt_min, opts->dt_max);
        prev_accept = next.accept;
        if (next.accept) {
            std::swap(h->u, h->usave);                               // the new state; its ghost rows are stale until the next halo exchange
            ksfd_ctl::state_written(h->cur, below == 0.0);
            st.accepted = 1; st.h_used = hh;
            *t += hh;
            *hstep = next.hnext;
            return KSFD_OK;
        }
        rejects++;
        st.rejections = rejects;
        hh = next.hnext;                                         // h->u, its ghost rows and the coefficient planes made of it are untouched
        *hstep = next.hnext;
        if (single) return KSFD_OK;                              // single attempt: report the rejection
        if (rejects > max_rej) return fail(h, KSFD_EREJECT, "step rejected %d times at t=%g", rejects, *t);
    }
}

extern "C" int ksfd_step(ksfd_handle *h, double *t, double *hstep, const ksfd_step_opts *opts, ksfd_step_stats *stats)
{
    if (!h || !t || !hstep || !opts) return KSFD_EINVAL;
    hipSetDevice(h->device);
    // pc_type 5: dense LU of shift*I - J, factored once per attempt (lu_host.hip.h); no spectral / polynomial / multigrid / pipelined
    // solver, no stage guesses.  Its limits are checked before the state or the step-to-step memory is touched.
    // pc_type 6: the same with the banded LU of the folded 1-D ring (banded_host.hip.h) in its place.
    const bool direct = opts->pc_type == 5 || opts->pc_type == 6;
    if (direct) {
        const int g = opts->pc_type == 6 ? banded_guard(h) : direct_guard(h);
        if (g) return g;
    }
    // deflated restarting (krylov_dr.hip.h): the restart length is the caller's, fixed, and must leave room behind the kept vectors
    const bool dr_on = h->dr_keep > 0 && !direct;
    if (dr_on) {
        const int m_dr = std::min(opts->ksp_restart > 0 ? opts->ksp_restart : 30, h->restart_alloc);
        if (h->dr_keep > m_dr - 3) return fail(h, KSFD_EINVAL, "deflation: keep = %d needs a restart length of at least %d (ksp_restart %d, basis vectors allocated %d)", h->dr_keep, h->dr_keep + 3, (int)opts->ksp_restart, h->restart_alloc);
    }
    memset(&h->dr_stats, 0, sizeof h->dr_stats);
    if (env_knobs().pc_sigma_set) h->memo.mg_shift_floor = env_knobs().pc_sigma;      // experiment knob: fixed floor
    ksfd_step_stats st;
    memset(&st, 0, sizeof st);
    const StepCounters c0 = stats_begin(h);
    const int32_t coarse0 = h->mgc.solves;
    const int rc = step_run(h, t, hstep, opts, direct, dr_on, st);
    stats_end(h, c0, st);
    if (h->mgc.solves != coarse0) st.pc_used |= 64;
    if (stats) *stats = st;
    return rc;
}

extern "C" int ksfd_get_last_error_vector(ksfd_handle *h, double *eh, int32_t layout)
{
    if (!h || !eh) return KSFD_EINVAL;
    if (!h->cur.have_err) return fail(h, KSFD_EINVAL, "no step has been attempted yet");
    hipSetDevice(h->device);
    int rc = err_materialize(h);
    if (rc) return rc;
    return download(h, h->errv, layout, eh);
}

extern "C" int ksfd_set_profiling(ksfd_handle *h, int32_t on)
{
    if (!h) return KSFD_EINVAL;
    prof_resolve(h);
    if (on < 0 || on >= 2 + KSFD_NKCLASS) return KSFD_EINVAL;
    h->profiling = on != 0;
    h->prof_only = on >= 2 ? on - 2 : -1;
    return KSFD_OK;
}
extern "C" int ksfd_get_profile(ksfd_handle *h, ksfd_profile *p, int32_t reset)
{
    if (!h || !p) return KSFD_EINVAL;
    prof_resolve(h);
    *p = h->prof;
    if (reset) memset(&h->prof, 0, sizeof h->prof);
    return KSFD_OK;
}
extern "C" int ksfd_set_mg_params(ksfd_handle *h, int32_t nu, int32_t ncoarse_max, int32_t power_its, double ratio, double coarse_tol)
{
    if (!h) return KSFD_EINVAL;
    if (nu > 0) h->mg_nu = nu;
    if (ncoarse_max > 0) h->mg_ncoarse = ncoarse_max;
    if (power_its > 0) h->mg_power_its = power_its;
    if (ratio > 1.0) h->mg_ratio = ratio;
    if (coarse_tol > 0.0) h->mg_coarse_tol = coarse_tol;
    ksfd_ctl::tuning_mg_graph(h->tune, power_its);
    ksfd_ctl::vcycle_config_changed(h->cur);
    return KSFD_OK;
}
// level the cycle would end on for (kind, max_unknowns), or -1 (mg_coarse_plan.h)
static int mg_coarse_choice(const ksfd_handle *h, int32_t kind, int32_t max_unknowns)
{
    std::vector<long long> unk;
    for (const MGLevel &L : h->mg) unk.push_back((long long)L.G.F * L.G.nloc);
    return ksfd_ctl::mg_coarse_level(unk.data(), h->mg_ok ? (int)unk.size() : 0, kind, max_unknowns, KSFD_MG_DIRECT_MAX);
}
extern "C" int ksfd_set_mg_coarse(ksfd_handle *h, int32_t kind, int32_t max_unknowns)
{
    if (!h) return KSFD_EINVAL;
    if (kind != 0 && kind != 1) return fail(h, KSFD_EINVAL, "mg_coarse: kind %d is neither 0 (Chebyshev) nor 1 (exact solve)", (int)kind);
    if (kind == 1) {
        if (h->ring) return fail(h, KSFD_EINVAL, "mg_coarse: the exact coarse solve is single rank only (this handle has a halo transport)");
        if (!h->mg_ok) return fail(h, KSFD_EINVAL, "mg_coarse: this handle has no multigrid hierarchy");
        if (max_unknowns > KSFD_MG_DIRECT_MAX) return fail(h, KSFD_EINVAL, "mg_coarse: max_unknowns = %d above KSFD_MG_DIRECT_MAX = %d", (int)max_unknowns, KSFD_MG_DIRECT_MAX);
        if (h->mgt.max_points > 0) return fail(h, KSFD_EINVAL, "mg_coarse: the exact coarse solve and the coarse tail exclude each other (ksfd_set_mg_tail(%lld) is in force)", (long long)h->mgt.max_points);
    } else if (!h->mg_ok) return KSFD_OK;               // nothing to switch off
    const int level = mg_coarse_choice(h, kind, max_unknowns);
    if (level < 0) {
        const MGLevel &Lc = h->mg.back();
        return fail(h, KSFD_EINVAL, "mg_coarse: no level below level 0 has at most %d unknowns (the coarsest of %d levels has %lld)",
                    max_unknowns > 0 ? (int)max_unknowns : KSFD_MG_DIRECT_MAX, (int)h->mg.size(), (long long)Lc.G.F * Lc.G.nloc);
    }
    hipSetDevice(h->device);
    if (kind == 1) { int rc = mgc_alloc(h, level); if (rc) return rc; }      // before anything changes
    if (kind == h->mgc.kind && level == h->mgc.level) { h->mgc.max_unknowns = kind == 1 ? max_unknowns : 0; return KSFD_OK; }
    h->mgc.kind = kind; h->mgc.level = level; h->mgc.max_unknowns = kind == 1 ? max_unknowns : 0;
    ksfd_ctl::vcycle_config_changed(h->cur);             // the next V cycle sets the hierarchy up again, and with it captures its graph again
    return KSFD_OK;
}
extern "C" int ksfd_set_mg_agglomerate(ksfd_handle *h, int64_t max_points)
{
    if (!h) return KSFD_EINVAL;
    if (max_points < 0) return fail(h, KSFD_EINVAL, "mg_agglomerate: max_points = %lld is negative", (long long)max_points);
    if (!h->ring) return KSFD_OK;                        // one rank without a transport: every level is whole already
    if (h->G.dim == 1) return fail(h, KSFD_EINVAL, "mg_agglomerate: 2-D and 3-D slabs only (this handle is 1-D)");
    if (!h->mg_ok) return fail(h, KSFD_EINVAL, "mg_agglomerate: this handle has no multigrid hierarchy");
    hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize(h->st));
    // free and rebuild; every rank must come out with the same hierarchy (an allocation that failed on one rank only would leave the
    // others waiting in a collective), so the ranks agree on the outcome and fall back to the previous setting together
    const int64_t before = h->mg_agg;
    int own_rc = KSFD_OK;
    std::string own_err;
    bool failed = false;
    auto rebuild = [&](int64_t agg) -> int {
        mg_free(h);
        h->mg_agg = agg;
        own_rc = mg_build(h);
        own_err = h->err;
        if (!own_rc && !h->mg_ok) own_rc = fail(h, KSFD_EINVAL, "mg_agglomerate: the rebuilt hierarchy has fewer than two levels"), own_err = h->err;
        double bad = own_rc ? 1.0 : 0.0;
        if (hipMemcpyAsync(h->dres, &bad, sizeof bad, hipMemcpyHostToDevice, h->st) != hipSuccess || h->tr->allreduce(h->dres, 1, 1, h->st))
            return fail(h, KSFD_ECOMM, "mg_agglomerate: agreeing on the hierarchy failed: %s", h->tr->error().c_str());
        if (h->tr->result_on_host()) bad = h->tr->host_result()[0];
        else if (hipMemcpyAsync(&bad, h->dres, sizeof bad, hipMemcpyDeviceToHost, h->st) != hipSuccess || hipStreamSynchronize(h->st) != hipSuccess)
            return fail(h, KSFD_EHIP, "mg_agglomerate: reading the agreed outcome failed");
        HIPCHK(h, hipStreamSynchronize(h->st));
        failed = bad > 0.5;
        return KSFD_OK;
    };
    int rc = rebuild(max_points);
    if (rc || !failed) return rc;
    // this rank's own reason where it has one; a rank whose build went through learns that another's did not
    const int why_rc = own_rc;
    const std::string why = own_err;
    if (rebuild(before) != KSFD_OK || failed) { mg_free(h); h->mg_agg = 0; }
    if (why_rc) { h->err = why; return why_rc; }
    return fail(h, KSFD_ENOMEM, "mg_agglomerate: another rank could not build the hierarchy with max_points = %lld", (long long)max_points);
}
extern "C" int ksfd_get_mg_coarse_info(ksfd_handle *h, ksfd_mg_coarse_info *info)
{
    if (!h || !info) return KSFD_EINVAL;
    memset(info, 0, sizeof *info);
    if (!h->mg_ok) return fail(h, KSFD_EINVAL, "mg_coarse: this handle has no multigrid hierarchy");
    const MGLevel &L = h->mg[mg_end(h)];
    info->kind = h->mgc.kind; info->level = (int32_t)mg_end(h); info->nlevels = (int32_t)h->mg.size(); info->F = L.G.F;
    // extents per axis of that level (the 1-D level keeps its extent in nx)
    info->n[0] = L.G.nx; info->n[1] = L.G.dim >= 2 ? L.G.ny : 1; info->n[2] = L.G.dim >= 3 ? L.G.nz : 1;
    info->unknowns = (int64_t)L.G.F * L.G.nloc;
    info->factorizations = h->mgc.factorizations; info->solves = h->mgc.solves; info->fallbacks = h->mgc.fallbacks;
    return KSFD_OK;
}
extern "C" int ksfd_mg_coarse_apply(ksfd_handle *h, double shift, int32_t op, const double *vh, double *outh)
{
    if (!h || !vh || !outh) return KSFD_EINVAL;
    if (!isfinite(shift)) return fail(h, KSFD_EINVAL, "mg_coarse_apply: non-finite shift");
    if (op != 0 && op != 1) return fail(h, KSFD_EINVAL, "mg_coarse_apply: op %d is neither 0 (operator) nor 1 (solve)", (int)op);
    if (!h->mg_ok) return fail(h, KSFD_EINVAL, "mg_coarse: this handle has no multigrid hierarchy");
    if (op == 1 && h->mgc.kind != 1) return fail(h, KSFD_EINVAL, "mg_coarse_apply: op 1 needs ksfd_set_mg_coarse(kind 1)");
    if (h->ring) return fail(h, KSFD_EINVAL, "mg_coarse_apply: single rank only (this handle has a halo transport)");
    hipSetDevice(h->device);
    int rc;
    if ((rc = ensure_coef(h))) return rc;
    if (!h->cur.mg_coef_valid && (rc = mg_restrict_coefs(h))) return rc;
    MGLevel &L = h->mg[mg_end(h)];                        // never level 0: b and x are the level's own
    double *const lb = L.v64.b, *const lx = L.v64.x;
    const size_t nb = sizeof(double) * (size_t)L.G.nloc;
    for (int f = 0; f < L.G.F; f++)
        HIPCHK(h, hipMemcpyAsync(lb + (int64_t)f * L.G.plane + L.kv.off, vh + (int64_t)f * L.G.nloc, nb, hipMemcpyHostToDevice, h->st));
    if (op == 0) rc = mg_op<double>(h, L, lb, 1, shift, lx, nullptr);
    else {
        bool ok = false;
        ksfd_ctl::hierarchy_borrowed(h->cur);            // the coarse factors now belong to this shift: the next cycle sets up again
        if ((rc = mgc_setup(h, L, shift, &ok))) return rc;
        if (!ok) return fail(h, KSFD_ELINEAR, "coarse solve: zero or non-finite pivot in column %d of shift*I - J_c (shift %.6g, %lld unknowns)", h->mgc.info_h - 1, shift, (long long)h->mgc.lu.n);
        rc = mgc_apply(h, L, lb, lx);
        ksfd_ctl::hierarchy_borrowed(h->cur);
    }
    if (rc) return rc;
    for (int f = 0; f < L.G.F; f++)
        HIPCHK(h, hipMemcpyAsync(outh + (int64_t)f * L.G.nloc, lx + (int64_t)f * L.G.plane + L.kv.off, nb, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return KSFD_OK;
}
// ---- parity/test entry of the parts of the V cycle (include/ksfd_hip.h has the contract) ------------------------------------------------
// host vector (np planes of the level's owned points, SoA) -> a device vector in the level's ghosted layout; ghosts zero.  T = float:
// rounded on the host
template <typename T>
static int mgp_put(ksfd_handle *h, const MGLevel &L, int np, const double *host, T *dev)
{
    HIPCHK(h, hipMemsetAsync(dev, 0, sizeof(T) * (size_t)np * L.G.plane, h->st));
    std::vector<T> tmp((size_t)np * L.G.nloc);
    for (size_t i = 0; i < tmp.size(); i++) tmp[i] = (T)host[i];
    for (int f = 0; f < np; f++)
        HIPCHK(h, hipMemcpyAsync(dev + (int64_t)f * L.G.plane + L.kv.off, tmp.data() + (int64_t)f * L.G.nloc, sizeof(T) * (size_t)L.G.nloc, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return KSFD_OK;
}
template <typename T>
static int mgp_get(ksfd_handle *h, const MGLevel &L, int np, const T *dev, double *host)
{
    std::vector<T> tmp((size_t)np * L.G.nloc);
    for (int f = 0; f < np; f++)
        HIPCHK(h, hipMemcpyAsync(tmp.data() + (int64_t)f * L.G.nloc, dev + (int64_t)f * L.G.plane + L.kv.off, sizeof(T) * (size_t)L.G.nloc, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    for (size_t i = 0; i < tmp.size(); i++) host[i] = (double)tmp[i];
    return KSFD_OK;
}
// coefficient planes of every level at the resident state; setup: block diagonals and Chebyshev bounds at `shift` from a cold power iteration
static int mgp_begin(ksfd_handle *h, bool setup, double shift)
{
    int rc;
    if ((rc = ensure_coef(h)) || (rc = ensure_coef32(h))) return rc;      // level 0 reads the fp32 copy of the planes where the handle has one (mg_sys)
    if (!h->cur.mg_coef_valid && (rc = mg_restrict_coefs(h))) return rc;
    if (setup) {
        mg_setup_cold(h);
        ksfd_ctl::hierarchy_borrowed(h->cur);
        if ((rc = mg_setup_shift(h, shift))) return rc;
    }
    return KSFD_OK;
}
// the hierarchy counts as not set up afterwards: the next real set-up starts cold and captures its graph again
static void mgp_end(ksfd_handle *h)
{
    ksfd_ctl::hierarchy_borrowed(h->cur);
    mg_setup_cold(h);
}
// the level has a smoother after a set-up: it is part of the cycle, and not the level of an exact solve that succeeded
static bool mgp_smoothed(const ksfd_handle *h, size_t l) { return l <= mg_end(h) && !(l == mg_end(h) && h->mgc.kind == 1 && h->cur.mgc_ready); }

extern "C" int ksfd_mg_level_info(ksfd_handle *h, int32_t level, int32_t setup, double shift, ksfd_mg_level_info_t *info)
{
    if (!h || !info) return KSFD_EINVAL;
    memset(info, 0, sizeof *info);
    if (!h->mg_ok) return fail(h, KSFD_EINVAL, "mg_part: this handle has no multigrid hierarchy");
    if (level < 0 || level >= (int)h->mg.size()) return fail(h, KSFD_EINVAL, "mg_part: level %d outside 0 .. %d", (int)level, (int)h->mg.size() - 1);
    if (setup && !isfinite(shift)) return fail(h, KSFD_EINVAL, "mg_part: non-finite shift");
    hipSetDevice(h->device);
    const int rc = mgp_begin(h, setup != 0, shift);         // the planes first: the fp32 coefficient copy exists once they are made
    const MGLevel &L = h->mg[level];
    info->level = level; info->nlevels = (int32_t)h->mg.size(); info->F = L.G.F; info->end_level = (int32_t)mg_end(h);
    info->n[0] = L.G.nx; info->n[1] = L.G.dim >= 2 ? L.G.ny : 1; info->n[2] = L.G.dim >= 3 ? L.G.nz : 1;
    info->sloc = L.G.sloc; info->points = L.G.nloc;
    info->path = (int32_t)mg_path(h, L);
    info->f32 = L.f32 ? 1 : 0;
    const JvpSys Y = mg_sys(h, L);
    info->coef32 = (Y.coef32 ? 2 : 0) | ((Y.coef32 && Y.cls == KC_JVP && mg_path(h, L) == JP_STRIP2D) ? 1 : 0);
    info->can_fuse = mg_can_fuse(h, L) ? 1 : 0;
    if (setup && !rc) {
        info->have_setup = mgp_smoothed(h, (size_t)level) ? 1 : 0;
        if (info->have_setup) { info->lam_max = L.lam_max; info->ratio = L.ratio; }
        if ((size_t)level == mg_end(h) && info->have_setup) info->coarse_sweeps = mg_coarse_sweeps(h, L);
    }
    mgp_end(h);
    return rc;
}

extern "C" int ksfd_mg_part(ksfd_handle *h, int32_t part, int32_t level, int32_t variant, int32_t nu, double shift, double ratio,
                            const double *in0, const double *in1, double *out0, double *out1)
{
    if (!h) return KSFD_EINVAL;
    if (!h->mg_ok) return fail(h, KSFD_EINVAL, "mg_part: this handle has no multigrid hierarchy");
    const int nlev = (int)h->mg.size();
    if (level < 0 || level >= nlev) return fail(h, KSFD_EINVAL, "mg_part: level %d outside 0 .. %d", (int)level, nlev - 1);
    if (!isfinite(shift)) return fail(h, KSFD_EINVAL, "mg_part: non-finite shift");
    MGLevel &L = h->mg[level];
    const bool transfer = part == KSFD_MGP_RESTRICT || part == KSFD_MGP_PROLONG_ADD;
    if (transfer && level + 1 >= nlev) return fail(h, KSFD_EINVAL, "mg_part: level %d has no coarser level", (int)level);
    MGLevel &Lc = h->mg[transfer ? level + 1 : level];
    const bool cf32 = transfer && mg_f32(h, (size_t)level + 1);       // the fp32 cycle keeps the coarser level in fp32 too
    const int F = L.G.F, np = 3 + h->P.nlig;
    bool setup = false, ok = true, need1 = false, need_o1 = false;
    switch (part) {
    case KSFD_MGP_COEF: ok = variant == 0; break;
    case KSFD_MGP_RESTRICT: ok = variant == 0 || (variant == 1 && L.f32) || (variant == 2 && L.G.dim == 2 && Lc.f32); break;
    case KSFD_MGP_PROLONG_ADD: ok = variant == 0 || (variant == 1 && L.f32); need1 = true; break;
    case KSFD_MGP_OPERATOR: ok = variant == 1 || variant == 2 || (variant == 32 && L.f32); need1 = variant != 1; break;
    case KSFD_MGP_DINV: ok = variant == 0; setup = true; break;
    case KSFD_MGP_DINV_APPLY: ok = variant == 0 || (variant == 1 && L.f32); setup = true; need_o1 = true; break;
    case KSFD_MGP_SMOOTH: ok = variant == 0; setup = true; break;
    case KSFD_MGP_CYCLE: ok = level == 0 && (variant == 0 || variant == 1); setup = true; break;
    case KSFD_MGP_TAIL:
        if (level != h->mgt.level) return fail(h, KSFD_EINVAL, "mg_part: level %d is not the first level of the coarse tail (%d; -1: this handle has none)", (int)level, h->mgt.level);
        ok = variant == 0; setup = true; break;
    default: return fail(h, KSFD_EINVAL, "mg_part: unknown part %d", (int)part);
    }
    if (!ok) return fail(h, KSFD_EINVAL, "mg_part %d: level %d has no variant %d", (int)part, (int)level, (int)variant);
    if (part == KSFD_MGP_CYCLE && variant == 1 && !mg_cycle32_ok(h))
        return fail(h, KSFD_EINVAL, "mg_part: this handle has no cycle with fp32 level vectors (2-D strip kernel on level 0, nu = 2, fused smoother, KSFD_TUNE_MG_FP64 clear)");
    if (part == KSFD_MGP_SMOOTH && (nu < 1 || nu > 5)) return fail(h, KSFD_EINVAL, "mg_part: nu = %d outside 1 .. 5", (int)nu);
    if (part == KSFD_MGP_SMOOTH && !(ratio > 1.0)) return fail(h, KSFD_EINVAL, "mg_part: smoothing ratio %.6g not above 1", ratio);
    if ((part != KSFD_MGP_COEF && part != KSFD_MGP_DINV && !in0) || (need1 && !in1) || !out0 || (need_o1 && !out1))
        return fail(h, KSFD_EINVAL, "mg_part %d: missing buffer", (int)part);
    if (setup && part != KSFD_MGP_CYCLE && (size_t)level > mg_end(h)) return fail(h, KSFD_EINVAL, "mg_part %d: level %d lies below the level the cycle ends on", (int)part, (int)level);
    hipSetDevice(h->device);
    int rc;
    if ((rc = mgp_begin(h, setup, shift))) { mgp_end(h); return rc; }
    if (setup && part != KSFD_MGP_CYCLE && !mgp_smoothed(h, (size_t)level)) { mgp_end(h); return fail(h, KSFD_EINVAL, "mg_part %d: level %d is solved exactly and has no smoother", (int)part, (int)level); }
    // staging in the level's ghosted layout (no larger than the handle's vectors); a replicated level, which may be larger than this
    // rank's slab, lends its own vectors
    double *const a = L.rep ? L.v64.b : h->t1, *const b = L.rep ? L.v64.x : h->t2, *const c = L.rep ? L.v64.d : h->t3;
    auto run = [&]() -> int {
        int r;
        switch (part) {
        case KSFD_MGP_COEF: {
            if ((r = mgp_get(h, L, np, (const double *)L.coef, out0))) return r;
            const float *c32 = mg_sys(h, L).coef32;
            if (out1 && c32) return mgp_get(h, L, np, c32, out1);
            return KSFD_OK;
        }
        case KSFD_MGP_RESTRICT: {
            auto go = [&](auto *fine, auto *coarse) -> int {
                if ((r = mgp_put(h, L, F, in0, fine)) || (r = mg_halo(h, L, fine, F))) return r;
                if ((r = mg_launch_restrict(h, L, Lc, F, fine, coarse)) || (r = mg_border_reduce(h, L, Lc, F, coarse))) return r;
                return mgp_get(h, Lc, F, coarse, out0);
            };
            if (variant == 0) return Lc.rep ? go(a, Lc.v64.b) : go(a, b);
            if (variant == 2) return go(a, Lc.v32.b);       // what the fp32 coefficient copy of a level is made with
            return cf32 ? go(L.v32.r, Lc.v32.b) : go(L.v32.r, Lc.v64.b);
        }
        case KSFD_MGP_PROLONG_ADD: {
            auto go = [&](auto *fine, auto *coarse) -> int {
                if ((r = mgp_put(h, L, F, in0, fine)) || (r = mgp_put(h, Lc, F, in1, coarse)) || (r = mg_halo(h, Lc, coarse, F))) return r;
                if ((r = mg_launch_prolong(h, L, Lc, F, coarse, fine))) return r;
                return mgp_get(h, L, F, fine, out0);
            };
            if (variant == 0) return Lc.rep ? go(a, Lc.v64.x) : go(a, b);
            return cf32 ? go(L.v32.x, Lc.v32.x) : go(L.v32.x, Lc.v64.x);
        }
        case KSFD_MGP_OPERATOR: {
            auto go = [&](auto *v, auto *out, auto *y, int mode) -> int {
                if ((r = mgp_put(h, L, F, in0, v)) || (mode == 2 && (r = mgp_put(h, L, F, in1, y)))) return r;
                if ((r = mg_op(h, L, v, mode, shift, out, mode == 2 ? y : nullptr))) return r;
                return mgp_get(h, L, F, out, out0);
            };
            return variant == 32 ? go(L.v32.x, L.v32.r, L.v32.b, 2) : go(a, b, c, variant);
        }
        case KSFD_MGP_DINV: return mgp_get(h, L, F * F, (const float *)L.dinv, out0);
        case KSFD_MGP_DINV_APPLY: {
            const double scale = nu ? (double)nu : 1.0;        // any scale: nu stands in (0 = 1)
            auto go = [&](auto *z, auto *z2, auto *rcopy) -> int {
                if ((r = mgp_put(h, L, F, in0, a))) return r;
                mg_dinv_apply(h, L, 0.0, (const double *)a, 1.0 / scale, z, z2, rcopy);
                if ((r = mgp_get(h, L, F, z, out0)) || (r = mgp_get(h, L, F, z2, out1))) return r;
                return mgp_get(h, L, F, rcopy, out1 + (int64_t)F * L.G.nloc);
            };
            return variant == 0 ? go(b, c, L.Ad) : go(L.v32.d, L.v32.x, L.v32.b);
        }
        case KSFD_MGP_SMOOTH:
            if ((r = mgp_put(h, L, F, in0, a))) return r;
            if (in1) { if ((r = mgp_put(h, L, F, in1, b))) return r; }
            else HIPCHK(h, hipMemsetAsync(b, 0x7f, sizeof(double) * (size_t)L.vlen, h->st));      // zero guess: x is not to be read (1.4e306 if it is)
            if ((r = mg_smooth(h, L, shift, a, b, nu, !in1, ratio))) return r;
            return mgp_get(h, L, F, (const double *)b, out0);
        case KSFD_MGP_TAIL:                                    // b and x are the level's own, as in the cycle
            if ((r = mgp_put(h, L, F, in0, L.v64.b))) return r;
            HIPCHK(h, hipMemsetAsync(L.v64.x, 0x7f, sizeof(double) * (size_t)L.vlen, h->st));
            if ((r = mg_tail_apply(h, shift, L.v64.b, L.v64.x))) return r;
            return mgp_get(h, L, F, (const double *)L.v64.x, out0);
        default: {                                             // KSFD_MGP_CYCLE
            if ((r = mgp_put(h, L, F, in0, a))) return r;
            HIPCHK(h, hipMemsetAsync(b, 0x7f, sizeof(double) * (size_t)L.vlen, h->st));
            const bool was = h->mg_use32;
            h->mg_use32 = variant == 1;
            r = mg_precond(h, shift, a, b);
            h->mg_use32 = was;
            if (r) return r;
            return mgp_get(h, L, F, (const double *)b, out0);
        }
        }
    };
    rc = run();
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(h, KSFD_EHIP, "mg_part %d: launch failed", (int)part);
    mgp_end(h);
    return rc;
}
extern "C" int ksfd_set_mg_tail(ksfd_handle *h, int64_t max_points)
{
    if (!h) return KSFD_EINVAL;
    if (max_points < 0) return fail(h, KSFD_EINVAL, "mg_tail: max_points = %lld is negative", (long long)max_points);
    if (max_points == h->mgt.max_points) return KSFD_OK;
    if (max_points > 0) {
        if (!h->mg_ok) return fail(h, KSFD_EINVAL, "mg_tail: this handle has no multigrid hierarchy");
        if (h->mgc.kind == 1) return fail(h, KSFD_EINVAL, "mg_tail: the coarse tail and the exact coarse solve exclude each other (ksfd_set_mg_coarse kind 1 is in force)");
    }
    hipSetDevice(h->device);
    const MGTail before = h->mgt;
    h->mgt.max_points = max_points;
    const int rc = mg_tail_replan(h);
    if (rc) { h->mgt = before; return rc; }
    ksfd_ctl::vcycle_config_changed(h->cur);             // another cycle: the next one sets the hierarchy up again and captures its graph again
    mg_setup_cold(h);                                    // ... from a cold power iteration, as after this entry it always has
    return KSFD_OK;
}
extern "C" int ksfd_get_mg_tail_info(ksfd_handle *h, ksfd_mg_tail_info *info)
{
    if (!h || !info) return KSFD_EINVAL;
    memset(info, 0, sizeof *info);
    info->level = -1;
    if (!h->mg_ok) return fail(h, KSFD_EINVAL, "mg_tail: this handle has no multigrid hierarchy");
    const MGTail &M = h->mgt;
    info->level = M.level; info->nlevels = M.nlev; info->max_points = M.max_points; info->lds_bytes = M.lds; info->launches = M.launches;
    for (int q = 0; q < M.nlev && q < 8; q++) info->points[q] = h->mg[M.level + q].G.nloc;
    return KSFD_OK;
}
extern "C" int ksfd_set_poly_params(ksfd_handle *h, int32_t max_degree, double target, double mg_threshold)
{
    if (!h || max_degree < 0 || max_degree > ksfd_krylov::CHEB_MAX_DEG) return KSFD_EINVAL;
    if (mg_threshold > 0.0) h->mg_threshold = mg_threshold;
    h->poly_max_deg = max_degree;           // 0 disables the polynomial preconditioner
    if (target > 0.0 && target < 1.0) h->poly_target = target;
    ksfd_ctl::poly_config_changed(h->cur);
    return KSFD_OK;
}
extern "C" int ksfd_spectral_apply(ksfd_handle *h, double shift, const double *vh, double *outh, int32_t layout)
{
    if (!h || !vh || !outh || !(shift > 0.0)) return KSFD_EINVAL;
    hipSetDevice(h->device);
    if (!h->spec.ok) return fail(h, KSFD_EINVAL, "spectral preconditioner not available for this handle (needs a 2-D or 3-D grid with every extent 2^k, 32 ... 16384, or 3*2^k, 48 ... 12288; on slab ranks 1, 2, 4 or 8 of them, an all-to-all transport, at least 4 local rows or 2 local planes)");
    int rc;
    if ((rc = upload(h, vh, layout, h->t2))) return rc;
    if ((rc = ensure_coef(h))) return rc;
    if ((rc = spec_means(h)) || (rc = spec_apply(h, shift, h->t2, h->t3))) return rc;
    return download(h, h->t3, layout, outh);
}
extern "C" int ksfd_direct_apply(ksfd_handle *h, double shift, const double *vh, double *outh, int32_t layout)
{
    if (!h || !vh || !outh) return KSFD_EINVAL;
    if (!isfinite(shift)) return fail(h, KSFD_EINVAL, "direct_apply: non-finite shift");
    if (layout < 0 || layout > 2) return fail(h, KSFD_EINVAL, "bad layout %d", layout);
    hipSetDevice(h->device);
    int rc;
    if ((rc = direct_guard(h))) return rc;
    if ((rc = ensure_coef(h)) || (rc = direct_factor(h, shift))) return rc;
    if ((rc = upload(h, vh, layout, h->t2)) || (rc = direct_solve(h, h->t2, h->t3))) return rc;
    return download(h, h->t3, layout, outh);
}
extern "C" int ksfd_banded_apply(ksfd_handle *h, double shift, const double *vh, double *outh, int32_t layout)
{
    if (!h || !vh || !outh) return KSFD_EINVAL;
    if (!isfinite(shift)) return fail(h, KSFD_EINVAL, "banded_apply: non-finite shift");
    if (layout < 0 || layout > 2) return fail(h, KSFD_EINVAL, "bad layout %d", layout);
    hipSetDevice(h->device);
    int rc;
    if ((rc = banded_guard(h))) return rc;
    if ((rc = ensure_coef(h)) || (rc = banded_factor(h, shift))) return rc;
    if ((rc = upload(h, vh, layout, h->t2)) || (rc = banded_solve(h, h->t2, h->t3))) return rc;
    return download(h, h->t3, layout, outh);
}
extern "C" int ksfd_set_deflation(ksfd_handle *h, int32_t keep, int32_t carry_stages)
{
    if (!h) return KSFD_EINVAL;
    if (keep < 0 || keep > 16) return fail(h, KSFD_EINVAL, "deflation: keep = %d outside 0 (off) .. 16", (int)keep);
    h->dr_keep = keep;
    h->dr_carry = carry_stages != 0;
    return KSFD_OK;
}
extern "C" int ksfd_get_deflation_stats(ksfd_handle *h, ksfd_deflation_stats *s)
{
    if (!h || !s) return KSFD_EINVAL;
    *s = h->dr_stats;
    return KSFD_OK;
}
extern "C" int32_t ksfd_basis_capacity(const ksfd_handle *h) { return h ? h->restart_alloc + 1 : 0; }
extern "C" int ksfd_basis_rotate(ksfd_handle *h, int32_t nin, int32_t nout, const double *P, const double *vin, double *vout, int32_t layout)
{
    if (!h || !P || !vin || !vout) return KSFD_EINVAL;
    if (layout < 0 || layout > 2) return fail(h, KSFD_EINVAL, "bad layout %d", layout);
    if (nin < 1 || nout < 1 || nout > nin || nout > KSFD_ROT_MAXOUT || nin > KSFD_ROT_MAXIN || nin > h->restart_alloc + 1)
        return fail(h, KSFD_EINVAL, "basis_rotate: %d -> %d vectors outside 1 <= nout <= %d, nout <= nin <= min(%d, %d)", (int)nin, (int)nout, KSFD_ROT_MAXOUT, KSFD_ROT_MAXIN, h->restart_alloc + 1);
    hipSetDevice(h->device);
    ksfd_ctl::krylov_basis_overwritten(h->cur);
    int rc;
    const int64_t nl = (int64_t)h->G.F * h->G.nloc;
    for (int i = 0; i < nin; i++) {
        if ((rc = upload(h, vin + (int64_t)i * nl, layout, h->V + (int64_t)i * h->vlen))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->st));            // the staging buffer of upload() is reused by the next vector
    }
    std::vector<double> Pp((size_t)nin * KSFD_ROT_MAXOUT, 0.0);
    for (int i = 0; i < nin; i++) for (int j = 0; j < nout; j++) Pp[(size_t)i * KSFD_ROT_MAXOUT + j] = P[(size_t)i * nout + j];
    if ((rc = op_basis_rotate(h, h->V, nin, nout, Pp.data(), KSFD_ROT_MAXOUT))) return rc;
    for (int i = 0; i < nin; i++)                          // all nin slots come back: the first nout rotated, the rest as uploaded
        if ((rc = download(h, h->V + (int64_t)i * h->vlen, layout, vout + (int64_t)i * nl))) return rc;
    return KSFD_OK;
}
// Parity/test entry of the Krylov vector kernels (include/ksfd_hip.h has the contract of every op).  Everything goes through the
// wrappers the solvers call (op_lincomb, op_multidot, op_multidot_gram, op_gs_update, op_basis_axpy, launch_gs_update_dev,
// launch_gmres_coef), in the Krylov basis V and the pipelined solver's device block, so dispatch, chunking and reduce_rows are what a
// stage solve runs.
extern "C" int ksfd_krylov_op(ksfd_handle *h, int32_t op, int32_t k, int32_t want_norm, const double *coef, double alpha, double beta,
                              const double *vecs, double *out_vecs, double *scalars, int32_t layout)
{
    if (!h) return KSFD_EINVAL;
    if (layout < 0 || layout > 2) return fail(h, KSFD_EINVAL, "bad layout %d", layout);
    const int cap = h->restart_alloc + 1;                  // ksfd_basis_capacity
    const int kdev = std::min(KSFD_ASYNC_MAXK, h->restart_alloc);
    int kmin = 1, kmax = 0, nvec = 0, nscal = 0;
    bool need_coef = true;
    switch (op) {
    case KSFD_KOP_LINCOMB: kmax = std::min(6, cap); nvec = k; nscal = want_norm ? 1 : 0; break;
    case KSFD_KOP_MULTIDOT: kmin = 0; kmax = cap - 1; nvec = k + 1; nscal = k + 1; need_coef = false; break;
    case KSFD_KOP_MULTIDOT_GRAM: kmax = std::min(32, cap - 1); nvec = k + 1; nscal = 2 * k + 1; need_coef = false; break;
    case KSFD_KOP_GS_UPDATE: kmax = cap - 1; nvec = k + 1; break;
    case KSFD_KOP_BASIS_AXPY: kmax = cap - 1; nvec = k + 1; nscal = want_norm ? 1 : 0; break;
    case KSFD_KOP_GS_UPDATE_DEV: kmax = kdev; nvec = k + 1; break;
    case KSFD_KOP_GMRES_COEF: kmax = kdev; nvec = 0; nscal = 1; break;
    default: return fail(h, KSFD_EINVAL, "krylov_op: unknown operation %d", (int)op);
    }
    if (k < kmin || k > kmax) return fail(h, KSFD_EINVAL, "krylov_op %d: k = %d outside %d .. %d (basis capacity %d)", (int)op, (int)k, kmin, kmax, cap);
    if ((need_coef && !coef) || (nvec && (!vecs || !out_vecs)) || (nscal && !scalars)) return fail(h, KSFD_EINVAL, "krylov_op %d: missing buffer", (int)op);
    if (want_norm && op != KSFD_KOP_LINCOMB && op != KSFD_KOP_BASIS_AXPY) return fail(h, KSFD_EINVAL, "krylov_op %d has no norm epilogue", (int)op);
    hipSetDevice(h->device);
    ksfd_ctl::krylov_basis_overwritten(h->cur);
    int rc;
    const GmDev D = gm_dev_block(h);
    if (op == KSFD_KOP_GMRES_COEF) {
        // columns j = 0 .. k-1 in sequence; the caller's rows stand in for what k_reduce_rows leaves in h->dres
        const double *row = coef;
        double *so = scalars;
        HIPCHK(h, hipMemsetAsync(D.coef, 0, sizeof(double) * KSFD_MAXDOT, h->st));        // what no column writes comes back as zero
        HIPCHK(h, hipMemsetAsync(D.H, 0, sizeof(double) * (size_t)D.ld * k, h->st));
        for (int j = 0; j < k; j++) {
            const int nrow = 2 * (j + 1) + 1;
            HIPCHK(h, hipMemcpyAsync(h->dres, row, sizeof(double) * nrow, hipMemcpyHostToDevice, h->st));
            launch_gmres_coef(h, D, j, beta);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipMemcpyAsync(so, D.coef, sizeof(double) * k, hipMemcpyDeviceToHost, h->st));
            HIPCHK(h, hipMemcpyAsync(so + k, D.scale, sizeof(double), hipMemcpyDeviceToHost, h->st));
            HIPCHK(h, hipMemcpyAsync(so + k + 1, D.mon + 2 * j, 2 * sizeof(double), hipMemcpyDeviceToHost, h->st));
            HIPCHK(h, hipStreamSynchronize(h->st));
            row += nrow; so += k + 3;
        }
        for (int c = 0; c < k; c++) HIPCHK(h, hipMemcpyAsync(so + (size_t)c * (k + 1), D.H + (size_t)D.ld * c, sizeof(double) * (k + 1), hipMemcpyDeviceToHost, h->st));
        HIPCHK(h, hipMemcpyAsync(so + (size_t)k * (k + 1), D.g, sizeof(double) * (k + 1), hipMemcpyDeviceToHost, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));
        return KSFD_OK;
    }
    const int64_t nl = (int64_t)h->G.F * h->G.nloc, vs = h->vlen;
    for (int i = 0; i < nvec; i++) {
        if ((rc = upload(h, vecs + (int64_t)i * nl, layout, h->V + (int64_t)i * vs))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->st));            // the staging buffer of upload() is reused by the next vector
    }
    double *const w = h->V + (int64_t)k * vs;              // where the solvers have the new vector: behind the k basis vectors
    switch (op) {
    case KSFD_KOP_LINCOMB: {
        const double *xs[6];
        for (int t = 0; t < k; t++) xs[t] = h->V + (int64_t)t * vs;
        rc = op_lincomb(h, k, xs, coef, h->V, want_norm != 0);       // out aliases input 0
    } break;
    case KSFD_KOP_MULTIDOT: rc = op_multidot(h, w, h->V, k); break;
    case KSFD_KOP_MULTIDOT_GRAM: rc = op_multidot_gram(h, w, h->V, k); break;
    case KSFD_KOP_GS_UPDATE: rc = op_gs_update(h, w, h->V, k, coef, alpha); break;
    case KSFD_KOP_BASIS_AXPY: rc = op_basis_axpy(h, w, h->V, k, coef, beta, want_norm != 0); break;
    default: {                                             // KSFD_KOP_GS_UPDATE_DEV: coefficients and scale where k_gmres_coef leaves them
        HIPCHK(h, hipMemcpyAsync(D.coef, coef, sizeof(double) * k, hipMemcpyHostToDevice, h->st));
        HIPCHK(h, hipMemcpyAsync(D.scale, &alpha, sizeof(double), hipMemcpyHostToDevice, h->st));
        launch_gs_update_dev(h, w, h->V, k, D.coef, D.scale);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(h->st));            // coef / alpha are the caller's pageable memory
        rc = KSFD_OK;
    } break;
    }
    if (rc) return rc;
    for (int i = 0; i < nscal; i++) scalars[i] = h->hres[i];
    for (int i = 0; i < nvec; i++)                         // every uploaded slot comes back: what the operation does not write, as uploaded
        if ((rc = download(h, h->V + (int64_t)i * vs, layout, out_vecs + (int64_t)i * nl))) return rc;
    return KSFD_OK;
}
// ---- parity/test entries of the stage right-hand sides and the frozen Jacobian action (include/ksfd_hip.h has the contract) -------------
// Everything goes through the functions the step calls, on the vectors the step uses; the entries only upload, download and report.
static int stage_rhs_run(ksfd_handle *h, int regime, int nstages, int ny, double hstep, double atol, double rtol, const double *y_host,
                         double *b_host, double *fin_host, ksfd_stage_info *info, int layout)
{
    int rc;
    const int64_t nl = (int64_t)h->G.F * h->G.nloc, vs = h->vlen;
    // head of step_run without the groom: the kernels clamp on load and the state must stay as it is
    if ((rc = halo(h, h->u))) return rc;
    if (h->tune.use_frozen && (rc = ensure_coef(h, true))) return rc;
    for (int j = 0; j < ny; j++) {
        if ((rc = upload(h, y_host + (int64_t)j * nl, layout, h->Y + (int64_t)j * vs))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->st));            // the staging buffer of upload() is reused by the next vector
    }
    AttemptPlan p = AttemptPlan{};
    p.hh = hstep;
    p.shift = 1.0 / (GAMMA_RA * hstep);
    p.use_spec = regime == 1;
    p.use_pc = regime == 2;
    plan_stage_forms(h, p);
    info->fuse_stage = p.fuse_stage; info->guess_on = p.guess_on;
    info->path = (int32_t)grid_path(h);
    if (fused_ok(h)) {
        const KStrips K = make_strips(h);
        info->rhs_strip = 1; info->seg = K.yseg; info->nseg = K.nseg; info->nstrips = K.nstrips;
        info->overlap = h->ring && h->tune.overlap && K.nseg >= 3;
    } else if (strip3d_ok(h) && h->tune.rhs3d_strip) {
        const K3D K = make_k3d(h);
        info->rhs_strip = 1; info->seg = K.zseg; info->nseg = K.nzseg; info->nstrips = K.nstrips; info->rows = K.rows;
    }
    double gb[4][4];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) gb[i][j] = NAN;
    for (int i = 0; i < nstages; i++) {
        StageRhs r;
        SpecGuess sg;
        sg.n = 0;
        if ((rc = stage_rhs(h, p, i, r))) return rc;
        if (p.guess_on && (rc = stage_gram_guess(h, i, r, gb, sg))) return rc;
        info->bnorm2[i] = r.bnorm2;
        info->dots_done[i] = r.dots_done ? 1 : 0;
        info->guess_n[i] = sg.n;
        for (int q = 0; q < sg.n; q++) info->guess_c[4 * i + (int)((sg.Y[q] - h->Y) / vs)] = sg.c[q];
        if ((rc = download(h, r.b, layout, b_host + (int64_t)i * nl))) return rc;
    }
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) info->gb[4 * i + j] = gb[i][j];
    if (fin_host) {
        ksfd_step_opts o;
        ksfd_default_step_opts(&o);
        o.atol = atol; o.rtol = rtol;
        if ((rc = step_finish(h, &o, &info->wrms, &info->below))) return rc;
        if ((rc = download(h, h->usave, layout, fin_host))) return rc;       // the new state; h->u is as it was (nothing swaps)
        if ((rc = err_materialize(h)) || (rc = download(h, h->errv, layout, fin_host + nl))) return rc;
    }
    return KSFD_OK;
}
extern "C" int ksfd_stage_rhs(ksfd_handle *h, int32_t regime, int32_t nstages, double hstep, double atol, double rtol, const double *y_host,
                              double *b_host, double *fin_host, ksfd_stage_info *info, int32_t layout)
{
    if (!h || !b_host || !info) return KSFD_EINVAL;
    if (layout < 0 || layout > 2) return fail(h, KSFD_EINVAL, "bad layout %d", layout);
    if (regime < 0 || regime > 2) return fail(h, KSFD_EINVAL, "stage_rhs: regime %d is none of 0 (plain), 1 (spectral), 2 (multigrid)", (int)regime);
    if (nstages < 1 || nstages > 4) return fail(h, KSFD_EINVAL, "stage_rhs: %d stages outside 1 .. 4", (int)nstages);
    if (!(hstep > 0.0) || !isfinite(hstep)) return fail(h, KSFD_EINVAL, "stage_rhs: step size %.6g is not positive and finite", hstep);
    if (fin_host && nstages != 4) return fail(h, KSFD_EINVAL, "stage_rhs: the completion needs all four stages (got %d)", (int)nstages);
    if (fin_host && !(atol >= 0.0 && rtol >= 0.0 && atol + rtol > 0.0 && isfinite(atol + rtol)))
        return fail(h, KSFD_EINVAL, "stage_rhs: tolerances atol %.6g, rtol %.6g of the completion are not usable", atol, rtol);
    const int ny = fin_host ? 4 : nstages - 1;
    if (ny > 0 && !y_host) return fail(h, KSFD_EINVAL, "stage_rhs: missing buffer");
    hipSetDevice(h->device);
    memset(info, 0, sizeof *info);
    for (int i = 0; i < 4; i++) info->bnorm2[i] = -1.0;
    const ksfd_ctl::Current before = h->cur;
    ksfd_ctl::stage_vectors_borrowed(h->cur, false);       // Y and bstore are about to hold the caller's vectors
    const int rc = stage_rhs_run(h, regime, nstages, ny, hstep, atol, rtol, y_host, b_host, fin_host, info, layout);
    if (fin_host) ksfd_ctl::stage_vectors_borrowed(h->cur, true);     // ... and the error vector, if the completion got that far, is no step's
    ksfd_ctl::derived_given_back(h->cur, before);          // planes made here only: the next step makes its own, launch for launch
    return rc;
}
// the fused fp32 residual as spec_solve decides it
static bool residual32_ok(ksfd_handle *h) { return fused_ok(h) || (strip3d_ok(h) && k3d_waves(h) <= part_capacity()); }
static int stage_jvp_run(ksfd_handle *h, int op, int mode, double shift, double alpha, double beta, int deg, const double *coef,
                         const double *v_host, const double *y_host, double *out_host, double *scalars, int layout);
extern "C" int ksfd_stage_jvp(ksfd_handle *h, int32_t op, int32_t mode, double shift, double alpha, double beta, int32_t deg, const double *coef,
                              const double *v_host, const double *y_host, double *out_host, double *scalars, int32_t layout)
{
    if (!h) return KSFD_EINVAL;
    if (layout < 0 || layout > 2) return fail(h, KSFD_EINVAL, "bad layout %d", layout);
    if (op < 0 || op > 2) return fail(h, KSFD_EINVAL, "stage_jvp: unknown operation %d", (int)op);
    if (!isfinite(shift) || !isfinite(alpha) || !isfinite(beta)) return fail(h, KSFD_EINVAL, "stage_jvp: non-finite shift, alpha or beta");
    if (op == 0 && (mode < 0 || mode > 4)) return fail(h, KSFD_EINVAL, "stage_jvp: mode %d outside 0 .. 4", (int)mode);
    if (op == 2 && (deg < 1 || deg > ksfd_krylov::CHEB_MAX_DEG)) return fail(h, KSFD_EINVAL, "stage_jvp: degree %d outside 1 .. %d", (int)deg, ksfd_krylov::CHEB_MAX_DEG);
    if (op == 2 && !(shift != 0.0)) return fail(h, KSFD_EINVAL, "stage_jvp: the polynomial needs a shift other than zero");
    const bool need_y = op == 1 || (op == 0 && (mode == 2 || mode == 3));
    if (!v_host || !out_host || !scalars || (need_y && !y_host) || (op == 2 && !coef)) return fail(h, KSFD_EINVAL, "stage_jvp %d: missing buffer", (int)op);
    if (!h->tune.use_frozen) return fail(h, KSFD_EINVAL, "stage_jvp: the frozen Jacobian action is switched off (KSFD_TUNE_RECOMPUTE_JVP)");
    hipSetDevice(h->device);
    if (op == 1 && !residual32_ok(h)) return fail(h, KSFD_EINVAL, "stage_jvp: no fused fp32 residual on this handle (it needs a strip kernel)");
    const ksfd_ctl::Current before = h->cur;
    const int rc = stage_jvp_run(h, op, mode, shift, alpha, beta, deg, coef, v_host, y_host, out_host, scalars, layout);
    ksfd_ctl::derived_given_back(h->cur, before);          // planes and fp32 copy made here only: the next step makes its own
    return rc;
}
static int stage_jvp_run(ksfd_handle *h, int op, int mode, double shift, double alpha, double beta, int deg, const double *coef,
                         const double *v_host, const double *y_host, double *out_host, double *scalars, int layout)
{
    int rc;
    if ((rc = ensure_coef(h))) return rc;
    // operands where the solvers have theirs: x in a work vector, b in bvec, the residual (fp32 or fp64) in Z; t1 and t2 are poly_apply's
    double *const v = h->t3, *const y = h->bvec, *const out = h->Z;
    if ((rc = upload(h, v_host, layout, v))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->st));
    if (y_host) {
        if ((rc = upload(h, y_host, layout, y))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->st));
    }
    for (int i = 0; i < 8; i++) scalars[i] = 0.0;
    const JvpPath path = grid_path(h);
    scalars[1] = (double)path;
    if (path == JP_STRIP2D) {
        const KStrips K = make_strips(h, true);
        scalars[2] = K.yseg; scalars[3] = K.nseg; scalars[4] = K.nstrips;
        scalars[6] = (h->ring && h->tune.overlap && K.nseg >= 3) ? 1.0 : 0.0;
    } else if (path == JP_LDS3D || path == JP_STRIP3D) {
        const K3D K = path == JP_LDS3D ? make_k3d_lds(h) : make_k3d(h);
        scalars[2] = K.zseg; scalars[3] = K.nzseg; scalars[4] = K.nstrips; scalars[7] = K.rows;
    }
    if (op == 0) {
        if ((rc = op_jvp_frozen_halo(h, v, mode, shift, out, y_host ? y : nullptr, alpha, beta))) return rc;
        return download(h, out, layout, out_host);
    }
    if (op == 1) {
        // as spec_residual: the 2-D fused residual exchanges the ghost rows of x itself, behind its interior rows
        if (h->ring && h->G.dim != 2 && (rc = halo(h, v))) return rc;
        float *const r32 = reinterpret_cast<float *>(out);
        if ((rc = op_residual32(h, v, shift, y, r32))) return rc;
        scalars[0] = h->hres[0];
        // widened on the host, then through the layout kernel like every other vector
        std::vector<float> f((size_t)h->vlen);
        std::vector<double> d((size_t)h->vlen);
        HIPCHK(h, hipMemcpyAsync(f.data(), r32, sizeof(float) * f.size(), hipMemcpyDeviceToHost, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));
        for (size_t i = 0; i < f.size(); i++) d[i] = (double)f[i];
        HIPCHK(h, hipMemcpyAsync(h->t1, d.data(), sizeof(double) * d.size(), hipMemcpyHostToDevice, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));
        return download(h, h->t1, layout, out_host);
    }
    // op 2: the caller's polynomial in place of the handle's for this one application.  poly_apply reads poly_deg and poly_alpha only; the
    // record of which shift they were made for (cur.poly_shift) is not touched and holds again once they are back
    const int deg0 = h->poly_deg;
    double alpha0[8];
    memcpy(alpha0, h->poly_alpha, sizeof alpha0);
    h->poly_deg = deg;
    for (int i = 0; i < 8; i++) h->poly_alpha[i] = i <= deg ? coef[i] : 0.0;
    rc = poly_apply(h, shift, v, out);
    h->poly_deg = deg0;
    memcpy(h->poly_alpha, alpha0, sizeof alpha0);
    if (rc) return rc;
    scalars[5] = (coef32_on(h) && fused_ok(h)) ? 1.0 : 0.0;
    return download(h, out, layout, out_host);
}
extern "C" int ksfd_set_spectral_params(ksfd_handle *h, double from_stiffness, int32_t enable)
{
    if (!h) return KSFD_EINVAL;
    if (from_stiffness > 0.0) h->spec_from = from_stiffness;
    if (enable == 0) h->spec.user_off = true;
    else if (enable > 0) { h->spec.user_off = false; h->memo.spec_bad_until = 0; h->memo.spec_backoff = 8; }
    return KSFD_OK;
}
extern "C" int ksfd_synchronize(ksfd_handle *h)
{
    if (!h) return KSFD_EINVAL;
    hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize(h->st));
    return KSFD_OK;
}
extern "C" int ksfd_set_tuning(ksfd_handle *h, int32_t word, int32_t yseg, int32_t yseg_jvp)
{
    if (!h) return KSFD_EINVAL;
    const bool mg_fuse = h->tune.mg_fuse;
    ksfd_ctl::tuning_apply(h->tune, word, yseg, yseg_jvp);
    if (word >= 0) h->coef32_failed = false;               // a word that asks for the fp32 copy has its allocation tried once more
    if (h->tune.mg_fuse != mg_fuse) ksfd_ctl::vcycle_config_changed(h->cur);       // the only switch a set-up depends on ("Switches")
    return KSFD_OK;
}

// Raw timing of one kernel class on the current state, HIP events on the compute stream.
// cls: KC_RHS, KC_JVP, KC_MULTIDOT (k = 8 basis vectors), KC_GSUPDATE (k = 8), KC_LINCOMB (3 inputs).
extern "C" int ksfd_bench_kernel(ksfd_handle *h, int32_t cls, int32_t reps, double *avg_ms, double *bytes_per_launch)
{
    if (!h || reps < 1 || !avg_ms) return KSFD_EINVAL;
    hipSetDevice(h->device);
    hipEvent_t a, b;
    HIPCHK(h, hipEventCreate(&a));
    HIPCHK(h, hipEventCreate(&b));
    const bool was = h->profiling;
    h->profiling = false;
    int rc = KSFD_OK;
    double by = 0.0;
    auto one = [&]() -> int {
        const double b0 = h->bytes_acc;
        int r = KSFD_OK;
        double coef[KSFD_MAXDOT] = { 0 };
        switch (cls) {
        case KC_RHS: r = op_rhs(h, h->u, -1, h->t3); break;
        case KC_JVP: r = h->tune.use_frozen ? op_jvp_frozen(h, h->Y, 1, 1.0, h->t3) : op_jvp(h, h->u, h->Y, 1, 1.0, h->t3); break;
        case KC_MULTIDOT: {
            Scope sc(h, KC_MULTIDOT, vbytes(h, 9));
            VW_DISPATCH(h, hipLaunchKernelGGL((k_multidot<8, VW>), dim3(vec2(h) ? (h->nblk_vec + 1) / 2 : h->nblk_vec), dim3(KSFD_BLOCK), 0, h->st, h->kv, (const double *)h->t3, (const double *)h->V, h->vlen, 8, h->part));
        } break;
        case KC_GSUPDATE: r = op_gs_update(h, h->t3, h->V, 8, coef, 1.0); break;
        case KC_SPECTRAL: r = spec_apply(h, 10.0, h->Y, h->t3); break;
        case KC_LINCOMB: { const double *xs[3] = { h->u, h->Y, h->Y + h->vlen }; double aa[3] = { 1.0, 0.5, 0.25 }; r = op_lincomb(h, 3, xs, aa, h->t3); } break;
        case KSFD_BENCH_ROTATE: {                                      // basis rotation 31 -> 11 vectors in one pass (k_basis_rotate)
            std::vector<double> Pb((size_t)31 * KSFD_ROT_MAXOUT, 0.0);
            for (int j = 0; j < 11; j++) Pb[(size_t)j * KSFD_ROT_MAXOUT + j] = 1.0;
            r = op_basis_rotate(h, h->V, 31, 11, Pb.data(), KSFD_ROT_MAXOUT);
        } break;
        case KSFD_BENCH_ROTATE_COMPOSED: {                                      // the same rotation as 11 combinations of 31 vectors each (out of place, into Zb)
            for (int i = 0; i < 31; i++) coef[i] = 1.0 / 31.0;
            for (int j = 0; j < 11 && !r; j++) r = op_basis_axpy(h, h->Zb + (int64_t)j * h->vlen, h->V, 31, coef, 0.0);
        } break;
        case KSFD_BENCH_BAND_FACTOR: r = banded_factor(h, h->band.shift); break;
        case KSFD_BENCH_BAND_SOLVE: r = banded_solve(h, h->Y, h->t3); break;
        case KSFD_BENCH_MGC_SETUP: { bool ok = false; MGLevel &L = h->mg[mg_end(h)]; r = mgc_setup(h, L, 1.0, &ok); if (!r && !ok) r = fail(h, KSFD_ELINEAR, "bench_kernel: the coarse factorization is flagged"); } break;
        case KSFD_BENCH_MGC_APPLY: { MGLevel &L = h->mg[mg_end(h)]; r = mgc_apply(h, L, L.v64.b, L.v64.x); } break;
        case KSFD_BENCH_MGC_FACTOR_COLUMNS: {
            MGLevel &L = h->mg[mg_end(h)];
            const LUSys Y{ &L.G, &L.P, L.coef, (long long)L.G.sloc, 0, KC_MG };
            if (!(r = lu_assemble(h, h->mgc.lu, Y, 1.0))) r = lu_factor_blocks(h, h->mgc.lu, KC_MG, false);
        } break;
        default: r = fail(h, KSFD_EINVAL, "bench_kernel: class %d not benchable", cls);
        }
        by = h->bytes_acc - b0;
        return r;
    };
    if ((cls == KSFD_BENCH_ROTATE || cls == KSFD_BENCH_ROTATE_COMPOSED) && (h->restart_alloc < 30 || !h->Zb)) { rc = fail(h, KSFD_EINVAL, "bench_kernel: the rotation benchmark needs 31 basis vectors and the flexible basis"); goto done; }
    if (cls == KSFD_BENCH_ROTATE || cls == KSFD_BENCH_ROTATE_COMPOSED) ksfd_ctl::krylov_basis_overwritten(h->cur);
    if (cls == KSFD_BENCH_BAND_FACTOR || cls == KSFD_BENCH_BAND_SOLVE) {
        if ((rc = banded_guard(h))) goto done;
        if (!h->band.valid) { rc = fail(h, KSFD_EINVAL, "bench_kernel: the banded benchmark needs a factorization (ksfd_banded_apply first)"); goto done; }
        if ((rc = ensure_coef(h, true))) goto done;
    }
    if (cls >= KSFD_BENCH_MGC_SETUP && cls <= KSFD_BENCH_MGC_FACTOR_COLUMNS) {
        if (h->mgc.kind != 1 || !h->mg_ok) { rc = fail(h, KSFD_EINVAL, "bench_kernel: the coarse-solve benchmark needs ksfd_set_mg_coarse(kind 1)"); goto done; }
        if ((rc = ensure_coef(h)) || (!h->cur.mg_coef_valid && (rc = mg_restrict_coefs(h)))) goto done;
        ksfd_ctl::hierarchy_borrowed(h->cur);                // the coarse factors no longer belong to the hierarchy's set-up
        if (cls == KSFD_BENCH_MGC_APPLY) { bool ok = false; if ((rc = mgc_setup(h, h->mg[mg_end(h)], 1.0, &ok))) goto done; if (!ok) { rc = fail(h, KSFD_ELINEAR, "bench_kernel: the coarse factorization is flagged"); goto done; } }
    }
    if ((rc = halo(h, h->u))) goto done;
    if (h->tune.use_frozen && (cls == KC_JVP || cls == KC_SPECTRAL) && (rc = ensure_coef(h, true))) goto done;
    if (cls == KC_SPECTRAL && (rc = spec_means(h))) goto done;
    for (int i = 0; i < 3 && !rc; i++) rc = one();
    if (rc) goto done;
    hipEventRecord(a, h->st);
    for (int i = 0; i < reps && !rc; i++) rc = one();
    hipEventRecord(b, h->st);
    if (hipEventSynchronize(b) != hipSuccess) rc = fail(h, KSFD_EHIP, "event sync failed");
    if (!rc) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, a, b);
        *avg_ms = ms / reps;
        if (bytes_per_launch) *bytes_per_launch = by;
    }
done:
    h->profiling = was;
    hipEventDestroy(a);
    hipEventDestroy(b);
    return rc;
}
