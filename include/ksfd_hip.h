/*
 * ksfd_hip.h -- C ABI of libksfd_hip.so, the MI355X (gfx950) implementation of the hot path of
 * leonavery/KSFD: RHS stencil, analytic Jacobian action, CFL velocity and the implicit
 * (PETSc "TS ROSW ra34pw2"-equivalent) time step, for the periodic 4th-order finite-difference
 * Keller-Segel system in 1, 2 or 3 dimensions.
 *
 * The reference has no FFI for this path: the seam is the Python object
 * `implicitTS(derivs, t0, dt, tmax, maxsteps, rtol, atol)` (KSFD/ksfdts.py:500-561) whose
 * TS.step() calls back into Derivatives.dfdt / Derivatives.Jacobian (KSFD/ksfdsym.py:902-940,
 * 814-886).  Each entry point below names the reference code it stands in for.  The ctypes
 * binding a maintainer would add is shown in INTEGRATION.md; ksfd_amd/lib.py is that binding.
 *
 * Conventions: every function returns 0 on success or a KSFD_E* code; ksfd_last_error() gives
 * the message (mirrors the CHKERR -> RuntimeError convention of cython/ksfdMat/ksfdMat.pyx:17-20).
 * One host thread per handle.  The handle owns all device memory, streams and events; callers
 * own host buffers.  No callbacks into the host language except the optional halo transport.
 */
#ifndef KSFD_HIP_H
#define KSFD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSFD_DIRECT_MAX 32768  /* largest F * local points the direct solver (pc_type 5) takes: 8 * 32768^2 B = 8.6 GB of dense factors */
#define KSFD_MG_DIRECT_MAX 2048   /* largest F * points of a level the direct coarse solver of the V cycle takes (32 MB inverse) */
#define KSFD_MAX_LIG 12  /* ligand fields after the reference's fourier_series() expansion (KSFD/ksfdligand.py:315-388 has no cap;
                          * 12 = the dispatch width of the kernels, params.h: KSFD_MAXL) */

enum {
    KSFD_OK = 0,
    KSFD_EINVAL = 1,      /* bad argument / unsupported configuration */
    KSFD_EHIP = 2,        /* a HIP runtime call failed */
    KSFD_ENOMEM = 3,
    KSFD_ELINEAR = 4,     /* linear solve did not converge (the reference's SNES failure, ksfdts.py:135) */
    KSFD_ENAN = 5,        /* non-finite error norm */
    KSFD_EREJECT = 6,     /* step rejected more than max_reject times (PETSc TS_DIVERGED_STEP_REJECTED) */
    KSFD_ECOMM = 7        /* halo / reduction transport failed */
};

/* Host-buffer layouts of an (F fields x local grid) state.  F = nlig + 1, field 0 = rho. */
enum {
    KSFD_LAYOUT_PETSC = 0, /* dof fastest: c + F*(i + nx*(j + ny*k))   KSFD/ksfdgrid.py:9-58 */
    KSFD_LAYOUT_SOA = 1,   /* device order, x fastest: i + nx*(j + ny*(k + nz*c)) */
    KSFD_LAYOUT_HDF5 = 2   /* (c,x,y[,z]) C order, last axis fastest  KSFD/ksfdtimeseries.py:497-505 */
};

/* Numeric problem description = what ps.values(t) and ps.Vgroups.ligands() give the reference's
 * operators (KSFD/ksfdsoln.py:104-161, KSFD/ksfdligand.py:306-388, 527-547). */
typedef struct ksfd_config {
    int32_t dim;            /* 1, 2, 3 */
    int32_t nlig;           /* <= KSFD_MAX_LIG */
    int32_t ngroups;
    int32_t cap_kind;       /* 0 tophat, 1 witch   (KSFD/ksfdsoln.py:150-157) */
    int64_t n[3];           /* GLOBAL grid points per axis, unused axes = 1 */
    double L[3];            /* box lengths; spacing = L/n, periodic (KSFD/ksfdgrid.py:138-149) */
    double s2, rhomax, cushion, maxscale, rhomin, Umin;
    const int32_t *lig_group;      /* [nlig] 0-based group of each ligand */
    const double *lig_w, *lig_s, *lig_gamma, *lig_D;   /* [nlig] */
    const double *grp_alpha, *grp_beta;                /* [ngroups] */
} ksfd_config;

/* Slab decomposition along the slowest spatial axis (y in 2-D, z in 3-D) -- the build's stand-in for
 * the PETSc DMDA ghost exchange of width 2 (KSFD/ksfdgrid.py:388-411; globalToLocal at
 * KSFD/ksfdsym.py:704,787,920,1203).  rank r owns slow-axis indices [r*n/size, (r+1)*n/size).
 * transport: 0 none (size must be 1), 1 RCCL (ncclSend/ncclRecv + ncclAllReduce inside the library;
 * nccl_id = the 128-byte ncclUniqueId broadcast by the launcher), 2 host callbacks (exchange /
 * allreduce run by the caller, e.g. mpi4py or torch.distributed; buffers are HOST pointers). */
typedef int (*ksfd_exchange_fn)(void *ctx, const double *send_lo, const double *send_hi,
                                double *recv_lo, double *recv_hi, int64_t count);
typedef int (*ksfd_allreduce_fn)(void *ctx, double *buf, int32_t count, int32_t op /*0 sum, 1 max*/);
/* uniform all-to-all on host buffers: block q of `send` (bytes_per_peer bytes) goes to rank q, block r of `recv` comes from
 * rank r (the own block included).  Optional: without it the spectral solver stays single-rank under transport 2.  With it (and
 * under transport 1) 1, 2, 4 or 8 slab ranks have the solver for the same extents as one rank, 2^k or 3*2^k per axis: see
 * ksfd_spectral_apply; other rank counts do not. */
typedef int (*ksfd_alltoall_fn)(void *ctx, const void *send, void *recv, int64_t bytes_per_peer);
typedef struct ksfd_dist {
    int32_t rank, size;
    int32_t transport;
    int32_t device;                /* HIP device ordinal for this rank */
    const void *nccl_id;           /* transport 1 */
    ksfd_exchange_fn exchange;     /* transport 2 */
    ksfd_allreduce_fn allreduce;   /* transport 2 */
    void *ctx;
    ksfd_alltoall_fn alltoall;     /* transport 2, may be NULL */
} ksfd_dist;

/* Time-step controls = the PETSc options every shipped options file passes
 * (options84:47-67: -ts_type rosw -ts_adapt_type basic -ts_adapt_clip 0.1,5 -ts_adapt_dt_min/max)
 * plus the Krylov knobs that replace -ksp_type preonly -pc_type lu. */
typedef struct ksfd_step_opts {
    double rtol, atol;          /* TSSetTolerances (KSFD/ksfdts.py:136) */
    int32_t adapt;              /* 1 = TSAdaptBasic, 0 = -ts_adapt_type none */
    int32_t max_reject;         /* rejections tolerated inside one call (PETSc default 10); < 0: unlimited (-ts_max_reject -1) */
    double clip_lo, clip_hi;    /* 0.1, 5 */
    double dt_min, dt_max;      /* 1e-20, 1e4 */
    double safety, reject_safety; /* 0.9, 0.5 */
    double ksp_rtol, ksp_atol;  /* GMRES: stop at ||r|| <= max(ksp_rtol*||b||, ksp_atol) */
    int32_t ksp_restart, ksp_max_it;
    int32_t pc_type;            /* 0 none; 1 geometric multigrid V cycle always; 2 automatic (default): the spectral defect correction
                                 * (constant-coefficient part of shift*I - J inverted by FFT; 2-D and 3-D, extents 2^k or 3*2^k, on one
                                 * rank and on 1, 2, 4 or 8 slab ranks: see ksfd_spectral_apply) while it converges in a few sweeps, else multigrid when the step is stiff,
                                 * Chebyshev polynomial + flexible GMRES when mildly stiff, none when not; 3 polynomial only;
                                 * 4 spectral always; 5 direct: dense LU of shift*I - J on the device, factored once per step attempt, every
                                 * stage solve checked by its true residual against max(ksp_rtol*||b||, ksp_atol) with at most two refinement
                                 * steps (single rank, at most KSFD_DIRECT_MAX unknowns, else KSFD_EINVAL before anything is touched);
                                 * 6 banded: the same for 1-D grids of any size at O(N F^3) cost -- the periodic ring is folded (0, N-1, 1, N-2, ...)
                                 * so that shift*I - J is banded with kl = ku = 5F - 1, and factored with partial pivoting inside the band
                                 * by one workgroup; a handful of launches per step attempt (single rank, 1-D, else KSFD_EINVAL before
                                 * anything is touched) */
    int32_t reserved;           /* flags.  bit 0: classic two-pass CGS2 instead of CGS2 with the algebraic second projection;
                                 * bit 1: single attempt per call -- a rejected step returns with accepted = 0 and *hstep = the
                                 * controller's proposal (callers that must refresh stage-time data per attempt);
                                 * bit 2: the previous attempt of this step was rejected (TSAdaptBasic then applies reject_safety);
                                 * bit 3: the spectral defect correction verifies EVERY solve with a final residual evaluation (no
                                 * predicted last sweep) */
} ksfd_step_opts;

typedef struct ksfd_step_stats {
    int32_t accepted;           /* 1 if the state advanced */
    int32_t rejections;
    int32_t linear_its;         /* linear iterations over all stages and attempts: GMRES iterations, or applications of the spectral
                                 * inverse (sweeps of the defect correction) where pc_used has bit 8 */
    int32_t rhs_evals, jvp_evals;
    int32_t pc_used;            /* preconditioners the stage solves of this call ran with, OR of: 1 none, 2 multigrid V cycle,
                                 * 4 Chebyshev polynomial, 8 spectral (constant-coefficient FFT), 16 direct (dense LU, pc_type 5), 32 banded direct
                                 * (banded LU of the folded 1-D ring, pc_type 6), 64 a V cycle of this call ended in a direct coarse
                                 * solve (ksfd_set_mg_coarse kind 1; set together with 2) */
    double wrms;                /* error norm of the last attempt */
    double h_used;              /* step actually taken (valid when accepted) */
    double ksp_resid;           /* last relative residual */
    double bytes;               /* algorithmic HBM bytes of all kernels launched by the call */
    int32_t launches;           /* kernels / device copies the call enqueued on the compute stream */
    int32_t host_syncs;         /* times the host waited for a device result inside the call (reduction hand-overs, stream
                                 * synchronisations): the latency-bound part of a step on many slab ranks */
    int32_t residual_evals;     /* true residuals b - A x evaluated by the spectral defect correction or the direct solver (one Jacobian
                                 * action each) */
    int32_t predicted_final;    /* stage solves whose LAST sweep was applied on the measured contraction of the earlier sweeps
                                 * instead of a residual evaluation (ksp_rtol >= 1e-8 only; opts.reserved bit 3 switches it off) */
} ksfd_step_stats;

/* Per-kernel-class timing gathered with HIP events on the library's compute stream. */
#define KSFD_NKCLASS 14
typedef struct ksfd_profile {
    double ms[KSFD_NKCLASS];       /* accumulated device time */
    double bytes[KSFD_NKCLASS];    /* accumulated bytes the IMPLEMENTATION must move (e.g. frozen-coefficient planes included) */
    int64_t launches[KSFD_NKCLASS];
    double alg_bytes[KSFD_NKCLASS];/* accumulated ALGORITHMIC bytes of the same launches (RHS 16*F*N,
                                    * Jacobian action 24*F*N, vector passes = operands * 8*F*N) */
} ksfd_profile;
const char *ksfd_kernel_class_name(int32_t cls);

typedef struct ksfd_handle ksfd_handle;

/* 128-byte ncclUniqueId from the same librccl the library resolves (rank 0 calls, the launcher broadcasts it) */
int ksfd_rccl_unique_id(void *out128);

/* -- lifetime.  dist == NULL: single GPU (device 0 or HIP_VISIBLE_DEVICES), in-kernel periodic wrap. */
int ksfd_create(const ksfd_config *cfg, const ksfd_dist *dist, ksfd_handle **out);
void ksfd_destroy(ksfd_handle *h);
const char *ksfd_last_error(const ksfd_handle *h);          /* h may be NULL: error of a failed create */
int ksfd_update_params(ksfd_handle *h, const ksfd_config *cfg);   /* time-dependent ps.values(t): Jacobian / operators at t */
/* Time-dependent parameters inside a step: the reference hands ps.values(t) at the STAGE time t_n + ASum_i*h to every RHS
 * evaluation (KSFD/ksfdsym.py:1303-1312, 1430-1439 via implicitIF, KSFD/ksfdts.py:563-596) while the Jacobian uses
 * ps.values(t_n).  stage 0..3 sets the table the i-th stage RHS of ksfd_step uses, -1 all four; cfg == NULL clears (the
 * stages then use the ksfd_update_params table).  Grid and ligand count must match the handle's. */
int ksfd_set_stage_params(ksfd_handle *h, int32_t stage, const ksfd_config *cfg);
int ksfd_local_range(const ksfd_handle *h, int64_t *slow_begin, int64_t *slow_end); /* Grid._ranges on the slab axis */
int64_t ksfd_local_size(const ksfd_handle *h);               /* F * local points: length of every host buffer */

/* -- state (the TS solution Vec u; KSFD/ksfdts.py:141-152).  Host buffers hold the LOCAL slab. */
int ksfd_set_state(ksfd_handle *h, const double *u_host, int32_t layout);
int ksfd_get_state(ksfd_handle *h, double *u_host, int32_t layout);
/* "next" row f2: asynchronous read-out for writers (TimeSeries.store / makeSaveMonitor, KSFD/ksfdtimeseries.py:484-509,
 * KSFD/ksfdts.py:466-497) -- the layout transform is ordered on the compute stream, the D2H copy runs on a third stream
 * into one of two pinned buffers owned by the handle while the stepper carries on.  _wait blocks until the copy has landed
 * and returns the buffer (ksfd_local_size doubles), valid until the second-next _begin.  Thread rule: _begin from the
 * stepping thread; _wait may be called from a writer thread. */
int ksfd_snapshot_begin(ksfd_handle *h, int32_t layout, int32_t *slot);
int ksfd_snapshot_wait(ksfd_handle *h, int32_t slot, const double **host);
/* "next" row f3: the reference's start_values (ksfdsolver2.py:580-639) evaluated on the device for this rank's slab:
 * rho = rho0 + smoothstep interpolation (KSFD/ksfdrandom.py:116,194-214) of the coarse samples z (GLOBAL coarse grid
 * nc[0..2], x fastest, periodic; the caller draws them from numpy's default_rng so the stream matches ksfdrandom.py:44-49),
 * U_l = rho*s_l/gamma_l (:636-637). */
int ksfd_set_state_random(ksfd_handle *h, const int64_t nc[3], const double *z_coarse_host, double rho0);
/* Device-side checkpoint of the state together with what the solver remembers from step to step (spectral-radius estimate,
 * preconditioner adaptation): op 0 = save, op 1 = restore.  One slot, allocated on first use.  Used by bench.py to time a
 * pinned window of steps repeatedly and by callers that want to retry from a known state without a host round trip. */
int ksfd_checkpoint(ksfd_handle *h, int32_t op);
/* device pointer, SoA with ghost rows; plane stride below.  Good until the next ksfd_step: an accepted step leaves the new state in the
 * handle's other buffer (the completion is out of place), so ask again after every step */
double *ksfd_device_state(ksfd_handle *h);
int64_t ksfd_device_plane_stride(const ksfd_handle *h);
int64_t ksfd_device_interior_offset(const ksfd_handle *h);

/* -- sources(t) added by Derivatives.dfdt (KSFD/ksfdsym.py:930-936).  stage -1 sets all four stage
 *    slots; stage 0..3 sets the field used at stage time t + ASum[stage]*h.  NULL clears. */
int ksfd_set_source(ksfd_handle *h, int32_t stage, int32_t field, const double *src_host, int32_t layout);

/* -- operators on host vectors (parity tests and host-driven integrators).
 *    u_host == NULL: use the handle's state.  Inputs are clamped the way Derivatives.groom does
 *    (KSFD/ksfdsym.py:888-900) on the fly; the stored state is not modified. */
int ksfd_rhs(ksfd_handle *h, double t, const double *u_host, double *out_host, int32_t layout);   /* Derivatives.dfdt */
int ksfd_jvp(ksfd_handle *h, const double *u_host, const double *v_host, double *out_host,
             int32_t layout);                                    /* action of Derivatives.Jacobian(u) on v */
int ksfd_velocity(ksfd_handle *h, const double *u_host, double *vel_host, int32_t layout); /* Derivatives.velocity: dim planes */
int ksfd_velocity_max(ksfd_handle *h, double vmax[3]);           /* per-axis max|grad G| of the state; CFL_step, ksfdts.py:302-319 */

/* -- outer-loop helpers of KSFDTS.solve (KSFD/ksfdts.py:202-284) acting on the device state */
int ksfd_groom(ksfd_handle *h);                                  /* KSFDTS.groom :231-237 */
int ksfd_count_worms(ksfd_handle *h, double *total);             /* sum(rho) over all ranks :239-246 */
int ksfd_scale_rho(ksfd_handle *h, double factor);               /* conserve_worms :248-256 */
int ksfd_mul_rho(ksfd_handle *h, const double *factor_host);     /* add_variance: rho *= exp(sd*N(0,1)) :268-284; local SoA plane */

/* -- assembled Jacobian export ("next" row f4): the matrix Derivatives.Jacobian + ksfdMat.setValuesJacobian assemble
 *    (KSFD/ksfdsym.py:814-886, cython/ksfdMat/ksfdMat.pyx:55-180), evaluated at the resident (clamped) state, as CSR over
 *    this rank's rows.  Ordering = the reference's PETSc Vec: unknown F*point + dof, point x-fastest; rows are numbered
 *    from this rank's first owned point (rowptr starts at 0), columns are GLOBAL unknown indices (periodic wrap applied),
 *    not sorted within a row.  Row of rho: F*(4*dim+1) entries; row of U_l: 4*dim+2.  Caller allocates from _nnz. */
int ksfd_jacobian_nnz(ksfd_handle *h, int64_t *nrows_local, int64_t *nnz_local);
int ksfd_jacobian_csr(ksfd_handle *h, int64_t *rowptr /* nrows+1 */, int64_t *col /* nnz */, double *val /* nnz */);

/* -- the implicit step that replaces petsc4py TS.step() (KSFD/ksfdts.py:211):
 *    4-stage Rosenbrock-W RA34PW2 with frozen Jacobian J(t_n,u_n), shift 1/(gamma h), each stage
 *    solved matrix-free by restarted GMRES on the device; TSAdaptBasic error control.
 *    in: *t, *hstep (step to try).  out: *t advanced when accepted, *hstep = next proposed step. */
void ksfd_default_step_opts(ksfd_step_opts *o);
int ksfd_step(ksfd_handle *h, double *t, double *hstep, const ksfd_step_opts *opts, ksfd_step_stats *stats);
/* embedded-minus-main of the last completed attempt, accepted or rejected.  Formed on this call from the stage vectors of that attempt,
 * which stay in place until the stage solves of the next attempt begin; a ksfd_step that fails before it completes an attempt (a stage
 * solve that returns an error) therefore leaves no vector, and the call fails with KSFD_EINVAL until an attempt completes again */
int ksfd_get_last_error_vector(ksfd_handle *h, double *err_host, int32_t layout);

/* -- measurement
 * on: 0 off; 1 HIP-event pair around every launch (costs ~8 us of device time per launch); 2+c events only around
 * launches of kernel class c (launch and byte counters of the other classes keep running) */
int ksfd_set_profiling(ksfd_handle *h, int32_t on);
int ksfd_get_profile(ksfd_handle *h, ksfd_profile *p, int32_t reset);
int ksfd_synchronize(ksfd_handle *h);
/* raw kernel benchmark used by bench.py/profiles: run `reps` launches of one kernel class on the state,
 * timed with HIP events on the compute stream; returns average ms per launch. */
int ksfd_bench_kernel(ksfd_handle *h, int32_t cls, int32_t reps, double *avg_ms, double *bytes_per_launch);
/* -- the tuning word of ksfd_set_tuning: one macro per bit or field, in bit order.  The encoding is frozen (callers pass stored words).
 * Defaults: KSFD_TUNE_FUSED set, every other bit clear, three vectors kept per stage. */
#define KSFD_TUNE_FUSED (1 << 0)             /* fused 2-D / strip kernels */
#define KSFD_TUNE_RECOMPUTE_JVP (1 << 1)     /* recompute (non-frozen) Jacobian action */
#define KSFD_TUNE_NO_OVERLAP (1 << 2)        /* no halo/compute overlap */
#define KSFD_TUNE_ASYNC_GMRES (1 << 3)       /* pipelined GMRES with device-resident Hessenberg/Givens state; its cycles are at most 32 iterations
                                              * long, which is what its kernels hold: a longer ksp_restart (and restart growth) runs as cycles of 32 */
#define KSFD_TUNE_NO_RECYCLE (1 << 4)        /* no Krylov recycling across the four stage systems of a step (wins over the next bit) */
#define KSFD_TUNE_RECYCLE_ALL (1 << 5)       /* recycle from every earlier stage (default: from the stages measured to matter: 1 for 2 and 3,
                                              * 1 and 3 for 4) */
#define KSFD_TUNE_REC_KEEP_MASK (7 << 6)     /* field: leading Arnoldi vectors kept per stage, KSFD_TUNE_REC_KEEP(1..4); 5..7 give 4; 0 keeps the
                                              * count in force (3 on a new handle), unlike every other bit, which a word always replaces */
#define KSFD_TUNE_REC_KEEP(v) (((v) & 7) << 6)
#define KSFD_TUNE_POLY_FP64 (1 << 9)         /* the polynomial preconditioner's temporaries and coefficient copy in fp64 (default: fp32 storage
                                              * inside p(A) only; the Krylov vectors, A z_j and the solution are fp64 always) */
#define KSFD_TUNE_UNFUSED_STAGE (1 << 10)    /* stage vectors formed with separate passes instead of inside the RHS kernel */
#define KSFD_TUNE_NO_ZERO_COPY (1 << 11)     /* reduction results fetched with a stream synchronisation + copy instead of spinning on a flag the
                                              * reduction kernel raises in mapped host memory */
#define KSFD_TUNE_UNFUSED_SMOOTHER (1 << 12) /* multigrid smoother as separate kernels instead of inside the Jacobian-action epilogues */
#define KSFD_TUNE_GENERIC_RHS3D (1 << 13)    /* 3-D RHS through the generic one-thread-per-point stencil pass instead of the z-marching strip kernel */
#define KSFD_TUNE_NO_SPEC_GUESS (1 << 14)    /* spectral stage solves start from zero instead of from the span of the earlier stage solutions */
#define KSFD_TUNE_NO_RHS_CARRY (1 << 15)     /* the stage RHS kernel re-reads the stage vectors it adds at the store instead of carrying their
                                              * combination along from the window load */
#define KSFD_TUNE_NO_SPEC_PREDICT (1 << 16)  /* the spectral defect correction verifies every solve with a residual evaluation (no predicted last sweep) */
#define KSFD_TUNE_NO_RESTART_GROWTH (1 << 17) /* GMRES keeps the restart length it was given (default: a cycle that ends without convergence is
                                              * followed by one of twice the length, up to the 30 ... 120 basis vectors ksfd_create found room for) */
#define KSFD_TUNE_COLD_POWER (1 << 18)       /* every multigrid set-up estimates the Chebyshev bound of a level by a cold power iteration (default:
                                              * warm start from the vector of the previous set-up, at most three iterations) */
#define KSFD_TUNE_MG_FP64 (1 << 19)          /* the V cycle keeps its level vectors in fp64 at every tolerance (default: fp32 level vectors when
                                              * ksp_rtol >= 1e-7, 2-D) */
#define KSFD_TUNE_REC_MG (1 << 20)           /* multigrid-preconditioned stage solves keep the whole first GMRES cycle of every stage and project the
                                              * later stages of the step on it first (experiment, measured slower: krylov.hip.h) */
#define KSFD_TUNE_OWN_DOTS (1 << 21)         /* the inner products of a new stage right-hand side with the earlier ones (stage guesses) are a pass of
                                              * their own instead of part of the RHS kernel's store epilogue */
#define KSFD_TUNE_OLD_BOUNDARY (1 << 22)     /* the step boundary as it was before the passes nobody reads were taken out: groom at the head of every
                                              * step (default: only when a value can be under its floor), the embedded error vector stored by every
                                              * completion (default: formed from the stage vectors when ksfd_get_last_error_vector asks), the fp32
                                              * coefficient copy stored with the fp64 planes (default: converted when the polynomial preconditioner or
                                              * the V cycle first reads it).  Same results bit for bit; for tests and A/B timing */
#define KSFD_TUNE_NO_GPLANE (1 << 23)        /* the first stage's right-hand side evaluates G(u) itself (default, 2-D strip path: it loads G from the
                                              * coefficient planes the step has just made of the same state, which may differ in the last bit) */
/* word < 0 changes no switch.  Any other word replaces EVERY switch above: a clear bit means its default, not "keep" -- except the
 * KSFD_TUNE_REC_KEEP field, where 0 keeps.  A word that toggles KSFD_TUNE_UNFUSED_SMOOTHER ends the multigrid shift set-up; no other bit
 * invalidates anything.  KSFD_TUNE_NO_ZERO_COPY clear has an effect only where the handle could map its result buffer.
 * yseg_*: rows per wave segment; <= 0 keeps */
int ksfd_set_tuning(ksfd_handle *h, int32_t word, int32_t yseg_rhs, int32_t yseg_jvp);
/* multigrid knobs (<=0 keeps): smoothing sweeps per side, cap on coarsest-grid sweeps, power iterations for the
 * Chebyshev bound, smoothing interval ratio lambda_max/lambda_min, coarsest-grid reduction target.
 * power_its = KSFD_MG_EAGER keeps the count and launches the coarse part of the V cycle kernel by kernel (debug / A-B timing); EVERY other
 * call of this entry, whatever it sets, goes back to replaying the captured graph (handles with a halo transport never capture) */
#define KSFD_MG_EAGER (-7)
int ksfd_set_mg_params(ksfd_handle *h, int32_t nu, int32_t ncoarse_max, int32_t power_its, double ratio, double coarse_tol);
/* Coarse solve of the multigrid V cycle.
 * kind 0: Chebyshev on the coarsest level (default, bit-for-bit the cycle without this call; max_unknowns is ignored);
 * kind 1: exact solve: shift*I - J_c assembled from the level's restricted coefficient planes, dense LU, explicit inverse, rebuilt
 *         once per set-up of the hierarchy and applied in one launch inside the cycle.  A set-up whose factorization meets a zero or
 *         non-finite pivot runs the Chebyshev solve on that level instead (counted in fallbacks); the step does not fail.
 * max_unknowns <= 0: the cycle ends on the hierarchy's own coarsest level; > 0: it ends on the FINEST level below level 0
 * whose F * points <= max_unknowns (levels below it stay allocated and unused).
 * KSFD_EINVAL, nothing changed: kind 1 on a handle with a halo transport, without a hierarchy, when the chosen level has more than
 * KSFD_MG_DIRECT_MAX unknowns or no level qualifies, max_unknowns > KSFD_MG_DIRECT_MAX. */
int ksfd_set_mg_coarse(ksfd_handle *h, int32_t kind, int32_t max_unknowns);
/* Coarse-level agglomeration of the multigrid hierarchy on slab ranks (handles with a halo transport, 2-D and 3-D).  Without it the
 * hierarchy ends where a rank would keep fewer than 4 slow units (4096^2 on 8 ranks: 32^2 instead of 8^2), and the Chebyshev solve on
 * that level needs many sweeps, each with a halo exchange.  With it the coarse levels are REPLICATED: every rank holds the whole level
 * and computes it redundantly with the wrap-index kernels of a single rank -- no ghost units, no halo exchange, no all-reduce in its
 * norms -- and coarsening goes on by the single-rank rule (even extents, >= 8 points per axis after halving).
 * max_points = 0: off (default): level list and every bit are those of a handle that never made the call.
 * max_points > 0: every level below level 0 whose GLOBAL point count is <= max_points is replicated, and, whatever max_points says,
 * the level the 4-units rule refuses is replicated instead of ending the hierarchy (1 = "replicate only where the slab rule forces it").
 * Across the border the restriction is a launch into this rank's slice of a zeroed whole-level vector and one all-reduce (sum) of that
 * vector -- the same bits on every rank; the prolongation reads the whole coarse vector with wrapped global indices, without
 * communication; the coefficient planes cross the same way, one all-reduce of 3 + nlig planes per set-up.  Replicated levels keep fp64
 * vectors and planes.  Launches stay eager, nothing joins the checkpoint.  What the all-reduce costs between devices against the halo
 * exchanges and sweeps it saves has NOT been measured: no timing claim is made.
 * The call is collective, every rank passes the same value.  It frees and rebuilds the hierarchy, so the hierarchy counts as not set up
 * afterwards (as after ksfd_mg_part).  On a handle without a halo transport: KSFD_OK, nothing changes.
 * KSFD_EINVAL, nothing changed: a negative value, a 1-D handle with a transport, a handle without a hierarchy.
 * ksfd_set_mg_coarse kind 1 stays refused on handles with a transport. */
int ksfd_set_mg_agglomerate(ksfd_handle *h, int64_t max_points);
/* The coarse TAIL of the V cycle in one workgroup launch (opt-in).  The last levels of every hierarchy hold 64 .. ~1500 points; a
 * V cycle spends tens of dependent tiny launches on them.  With the tail the sub-cycle from a level t down to the level the cycle ends on
 * and back -- pre-smoothing, residual, restriction, the Chebyshev sweeps of the end level, prolongation, post-smoothing: mathematically
 * the same operator -- is ONE launch of one workgroup that keeps every level vector of those levels in the LDS (k_mg_tail); inside
 * the captured graph it is one node, on handles with a halo transport one eager launch.
 * max_points = 0: off (the default): every bit is that of a handle that never made the call.
 * max_points > 0: t = the smallest level >= 1 for which every level t .. end is whole on this rank (a handle without a halo transport,
 * or a replicated level of ksfd_set_mg_agglomerate; a distributed level never qualifies), has at most max_points points, and the levels
 * together fit the LDS a workgroup may have (160 KB; 8 * points * (4 F + 1) bytes per level), in at most 8 levels.  Level 0 is never
 * part of the tail.  The tail's levels keep fp64 vectors in the cycle with fp32 level vectors.  If no level qualifies the call returns
 * KSFD_OK and the cycle is the one without it (info.level = -1).  The plan is remade whenever the hierarchy is rebuilt
 * (ksfd_set_mg_agglomerate).  The call is collective on handles with a transport (every rank passes the same value) and leaves the
 * hierarchy "not set up", as ksfd_mg_part does.  Nothing joins the checkpoint.
 * KSFD_EINVAL, nothing changed: a negative value, a handle without a hierarchy (max_points > 0), an exact coarse solve in force
 * (ksfd_set_mg_coarse kind 1) -- the two exclude each other: ksfd_set_mg_coarse kind 1 is refused while max_points > 0.
 * ksfd_get_mg_tail_info: level = t or -1, nlevels and points of the tail's levels, the LDS bytes of the launch, and the launches of the
 * tail over the life of the handle (replays of the captured graph counted). */
typedef struct ksfd_mg_tail_info { int32_t level, nlevels; int64_t max_points; int64_t points[8]; int64_t lds_bytes, launches; } ksfd_mg_tail_info;
int ksfd_set_mg_tail(ksfd_handle *h, int64_t max_points);
int ksfd_get_mg_tail_info(ksfd_handle *h, ksfd_mg_tail_info *info);
typedef struct ksfd_mg_coarse_info { int32_t kind, level, nlevels, F; int64_t n[3]; int64_t unknowns;
                                     int32_t factorizations, solves, fallbacks, reserved; } ksfd_mg_coarse_info;
/* valid with kind 0 too: describes the level the cycle ends on; the counters run over the life of the handle */
int ksfd_get_mg_coarse_info(ksfd_handle *h, ksfd_mg_coarse_info *info);
/* parity/test entry on the level the cycle ends on, at the resident state (single rank).  Host vectors of F * points doubles, SoA of
 * that level (x fastest, field slowest, no ghosts).  op 0: out = (shift*I - J_c) v by the level's own operator kernels (what the
 * smoother applies); op 1 (kind 1 only): out = the direct coarse solve of v, through the same set-up and apply wrappers the cycle
 * calls (KSFD_ELINEAR on a zero or non-finite pivot).  State and step memory untouched. */
int ksfd_mg_coarse_apply(ksfd_handle *h, double shift, int32_t op, const double *v_host, double *out_host);
/* Parity/test entry of the PARTS of the V cycle, the twin of ksfd_mg_coarse_apply and ksfd_krylov_op: one part of the cycle runs on
 * host vectors through the wrappers the cycle itself calls (mg_restrict_coefs, mg_setup_shift, mg_launch_restrict / _prolong in
 * every storage-type pair, mg_halo, mg_op in both storage types, mg_dinv_apply, mg_smooth, mg_precond), never through a kernel launch of its own, so a
 * wrong launch argument shows.  Host vectors are SoA of the level (x fastest, field slowest), OWNED points only: F * points doubles,
 * points = ksfd_mg_level_info_t.points.  fp32 operands are rounded to float on the host before upload and come back as doubles.
 * Handles with a halo transport: every call is collective, each rank passes its slab of the level (sloc slow units).  A REPLICATED level
 * (ksfd_set_mg_agglomerate) is taken and returned WHOLE on every rank: ksfd_mg_level_info reports sloc = the global slow extent and
 * points = the whole level there, nlevels / end_level count the replicated levels, and RESTRICT / PROLONG_ADD across the border run
 * slab <-> whole level (RESTRICT returns the gathered coarse vector, the same bits on every rank).
 * Both calls work at the resident state (its coefficient planes are made and restricted if they are not current) and leave the state and
 * what the stepper remembers from step to step untouched.  After either call the hierarchy counts as NOT set up: shift forgotten, captured
 * graph dropped, power-iteration vectors forgotten -- so the next real set-up starts its power iteration cold, as on a fresh handle, and so
 * does every set-up these calls run themselves: two calls with the same arguments agree bit for bit.
 * KSFD_EINVAL, nothing touched: no hierarchy, level out of range, a part or variant the level does not have, nu outside 1 .. 5, ratio <= 1,
 * a missing buffer, a non-finite shift.
 *
 * ksfd_mg_level_info: geometry and kernel choice of one level; setup != 0: after a cold set-up at `shift` also lam_max, ratio and the
 * Chebyshev sweeps mg_vcycle runs on the level the cycle ends on (have_setup = 0 and zeros on a level below the end of the cycle or on
 * the level of an exact coarse solve).
 *   path: 0 2-D strip kernel, 2 3-D strip kernel, 3 generic kernel (what mg_path picks)
 *   f32: the level has fp32 level vectors;  coef32: bit 0 = the operator of the fp64 cycle reads an fp32 coefficient copy (level 0, unless
 *   KSFD_TUNE_POLY_FP64 is set), bit 1 = the level has such a copy (the fp32 cycle reads it);  can_fuse: mg_can_fuse holds
 *
 * ksfd_mg_part: `level` is the level the part runs on; transfers run between `level` (fine) and level + 1.
 *   COEF         out0 = the 3 + nlig coefficient planes the level's operator reads, after ensure_coef + mg_restrict_coefs; out1 (may be
 *                NULL) = the fp32 copy where info.coef32 bit 1 is set
 *   RESTRICT     out0 (level + 1) = R in0 (level).  variant 0: fp64 (mg_launch_restrict); 1 (f32 levels): the launch of the fp32 cycle, fine
 *                fp32 and coarse fp32 where level + 1 runs in fp32, else fp64; 2 (2-D, level + 1 an f32 level): fine fp64, coarse fp32 (the
 *                launch that makes the fp32 coefficient copy)
 *   PROLONG_ADD  out0 = in0 (level) + P in1 (level + 1).  variant 0: fp64 (mg_launch_prolong); 1 (f32 levels): fine fp32, coarse as above
 *   OPERATOR     variant 1: out0 = (shift*I - J_l) in0; 2: out0 = in1 - (shift*I - J_l) in0 (mg_op modes 1, 2); 32 (f32 levels): mode 2 of
 *                mg_op on fp32 vectors
 *   DINV         out0 = the F*F planes k_blockdiag_inv leaves after mg_setup_shift(shift) (row-major blocks, fp32 values)
 *   DINV_APPLY   k_dinv_apply with scale 1/nu (nu = 0: 1): out0 = z, out1 = [z2 | rcopy] (2 F points).  variant 0: fp64 in and out;
 *                1 (f32 levels): fp64 in, fp32 out (entry of the fp32 cycle)
 *   SMOOTH       out0 = mg_smooth(level, shift, b = in0, x0 = in1 or NULL for the zero guess, nu = 1 .. 5, ratio) after a set-up at shift
 *   CYCLE        level 0: out0 = mg_precond(shift, in0); variant 0: fp64 level vectors, 1: fp32 level vectors (what ksp_rtol >= 1e-7
 *                selects in ksfd_step; KSFD_EINVAL where the handle would not run that cycle).  Captured graph or eager launches as the
 *                handle is set (ksfd_set_mg_params).
 *   TAIL         level = the first tail level of ksfd_set_mg_tail (any other level: KSFD_EINVAL): out0 = the tail applied to in0 after a
 *                set-up at shift, through the wrapper the cycle calls (mg_tail_apply), with the handle's nu and smoothing ratio */
typedef struct ksfd_mg_level_info_t { int32_t level, nlevels, end_level, F; int64_t n[3]; int64_t sloc, points;
                                      int32_t path, f32, coef32, can_fuse, have_setup, coarse_sweeps; double lam_max, ratio; } ksfd_mg_level_info_t;
enum { KSFD_MGP_COEF = 0, KSFD_MGP_RESTRICT = 1, KSFD_MGP_PROLONG_ADD = 2, KSFD_MGP_OPERATOR = 3, KSFD_MGP_DINV = 4, KSFD_MGP_DINV_APPLY = 5,
       KSFD_MGP_SMOOTH = 6, KSFD_MGP_CYCLE = 7, KSFD_MGP_TAIL = 8 };
int ksfd_mg_level_info(ksfd_handle *h, int32_t level, int32_t setup, double shift, ksfd_mg_level_info_t *info);
int ksfd_mg_part(ksfd_handle *h, int32_t part, int32_t level, int32_t variant, int32_t nu, double shift, double ratio,
                 const double *in0, const double *in1, double *out0, double *out1);
/* The hierarchy is built for max(shift, floor)*I - J; the floor is searched online by ksfd_step when 1/(gamma h) has fallen
 * below the growth rate of the instability and the iteration count explodes.  Environment KSFD_PC_SIGMA=<x> fixes it
 * instead (0 = no floor) -- an experiment knob, not part of the ABI. */
/* Chebyshev polynomial preconditioner: highest degree (default 6, at most 7; 0 = off), the residual reduction per
 * outer iteration that picks the degree (default 0.02; <= 0 keeps), and the stiffness h*gamma*lambda_max(diffusion)
 * above which pc_type 2 hands over to multigrid (default 75; <= 0 keeps) */
int ksfd_set_poly_params(ksfd_handle *h, int32_t max_degree, double target, double mg_threshold);
/* Spectral preconditioner: z = (shift*I - J0)^-1 v with J0 the constant-coefficient part of the Jacobian at the resident state
 * (grid means of rho*G_rho, rho*G_Ul; the 4th-order star's exact symbol), three hand-written FFT kernels (csrc/spectral.hip.h).
 * Handles that have it: on one rank without a halo transport, every 2-D and 3-D grid whose extents are each 2^k (32..16384) or
 * 3*2^k (48..12288), through every column path (the two-phase column kernel for columns that do not fit the LDS included); the
 * same grids on P = 1 (ring of one), 2, 4 or 8 slab ranks over a transport with an all-to-all: 2-D with ny/P >= 4 local rows, 3-D
 * with nz/P >= 2 local planes (3*2^j local rows or planes travel as three chunks of 2^j, which every valid extent allows).
 * Handles that do not: 1-D, other extents, rank counts other than 1, 2, 4, 8, a transport without an all-to-all.  Timing between
 * different devices is unmeasured for all of them.
 * _apply is the parity/test entry (host vectors; KSFD_EINVAL where the handle has no spectral solver).  _params: stiffness
 * h*gamma*lambda_max(diffusion) from which pc_type 2 prefers it (default 0.1 where the fused 2-D residual kernel runs, 0.3
 * elsewhere; <= 0 keeps) and enable (0 = never pick it automatically, 1 = default, < 0 keeps). */
int ksfd_spectral_apply(ksfd_handle *h, double shift, const double *v_host, double *out_host, int32_t layout);
int ksfd_set_spectral_params(ksfd_handle *h, double from_stiffness, int32_t enable);
/* Direct solver (pc_type 5): out = (shift*I - J)^-1 v with J the assembled Jacobian at the resident state, by the same assembly, LU
 * factorization with partial pivoting and triangular solves ksfd_step uses (no refinement here).  Parity/test entry like
 * ksfd_spectral_apply; KSFD_EINVAL on a handle with a halo transport or more than KSFD_DIRECT_MAX unknowns, KSFD_ELINEAR on a zero or
 * non-finite pivot.  The state and what the stepper remembers are not changed. */
int ksfd_direct_apply(ksfd_handle *h, double shift, const double *v, double *out, int32_t layout);
/* Banded direct solver (pc_type 6), the twin of ksfd_direct_apply for 1-D handles: any finite shift, all three layouts.  KSFD_EINVAL
 * on a handle that is not 1-D or has a halo transport, KSFD_ELINEAR on a zero or non-finite pivot. */
int ksfd_banded_apply(ksfd_handle *h, double shift, const double *v, double *out, int32_t layout);


/* -- GMRES with deflated restarting (GMRES-DR; Morgan, SIAM J. Sci. Comput. 24, 2002) as the Krylov solver of the stage systems.
 * Off by default.  keep = 0 switches it off, 1..16 = harmonic Ritz vectors of smallest modulus kept in the basis across a restart (one
 * more when the last one is half of a complex pair); above 16: KSFD_EINVAL.  ksfd_step returns KSFD_EINVAL, state untouched, while
 * keep > ksp_restart - 3.  carry_stages != 0: the relation kept at the end of a stage solve also serves the later stage systems of the
 * same step attempt (same matrix); it never crosses an attempt, a step or ksfd_checkpoint.
 * With deflation on, the solves pc_type selects as plain, multigrid-preconditioned or polynomial-preconditioned GMRES run deflated: the
 * restart length is ksp_restart and stays fixed (no restart growth), Krylov recycling across stages and the pipelined solver (the tuning
 * word's KSFD_TUNE_ASYNC_GMRES ... KSFD_TUNE_REC_KEEP_MASK and KSFD_TUNE_REC_MG) are bypassed, the V cycle preconditions flexibly like the polynomial (z_j kept: the cycle is not a linear operator), and a
 * solve returns KSFD_OK only on the TRUE residual b - A x, never on the recurrence alone: it must meet the tolerance, or -- unpreconditioned
 * solves only -- exceed it by no more than an estimate of the rounding error of evaluating it, nnz_row * u * ||A|| ||x||, and by no more than
 * a quarter of the tolerance; such solves are counted in rounding_passes and report their residual in ksp_resid.  The spectral defect correction with its fallbacks and the direct solver (pc_type 5) are untouched. */
int ksfd_set_deflation(ksfd_handle *h, int32_t keep, int32_t carry_stages);
typedef struct ksfd_deflation_stats {   /* of the last ksfd_step call, all its attempts together */
    int32_t restarts;           /* deflated restarts */
    int32_t kept;               /* vectors kept at the last of them */
    int32_t stage_its[4];       /* iterations per stage system */
    int32_t true_resid_fail;    /* solves whose recurrence residual met the tolerance while the true residual did not: continued */
    int32_t projections;        /* residuals projected on a kept relation (carry_stages, and continuations after a failed check) */
    int32_t rounding_passes;    /* solves accepted with a true residual above the tolerance (by < 25 %) within the rounding error of b - A x */
    int32_t reserved;
} ksfd_deflation_stats;
int ksfd_get_deflation_stats(ksfd_handle *h, ksfd_deflation_stats *stats);
/* Vectors the Krylov basis of this handle holds (restart length that fits + 1): 9 ... 121 by the memory free at ksfd_create.  The upper
 * limit of nin below; a caller of the test entry cannot know it otherwise. */
int32_t ksfd_basis_capacity(const ksfd_handle *h);
/* Parity/test entry of the basis rotation kernel: uploads nin host vectors (each ksfd_local_size doubles) into the Krylov basis and runs
 * V[:, 0:nout] <- V[:, 0:nin] * P in place (P nin x nout, row-major; nout <= 18, nin <= min(121, ksfd_basis_capacity)).  vout_host
 * receives ALL nin slots, not only the first nout: the first nout rotated, slots nout .. nin-1 as the kernel left them, which is
 * untouched -- so that a test can assert exactly that. */
int ksfd_basis_rotate(ksfd_handle *h, int32_t nin, int32_t nout, const double *P_host, const double *vin_host, double *vout_host,
                      int32_t layout);
/* Parity/test entry of the Krylov vector kernels, the twin of ksfd_basis_rotate: host vectors of ksfd_local_size doubles in `layout` are
 * uploaded into the leading slots of the Krylov basis, ONE operation runs through the launch wrappers the stage solvers call (basis-size
 * ladder 4 | 8 | 16 | 32, chunks of 32 vectors above that, the block-partial reduction), and results are downloaded.  The k basis vectors
 * are slots 0 .. k-1 and the vector w the operation measures or updates is slot k, as in the solvers; vecs_host holds all nvec slots in
 * that order and out_vecs_host receives ALL of them back, so a test can assert that what an operation does not write is untouched.
 * cap = ksfd_basis_capacity.  KSFD_EINVAL for a k outside the limits, before anything is touched; the state and what the stepper
 * remembers from step to step are unchanged.
 *   LINCOMB        nvec = k = 1..6: slot 0 <- sum_t coef[t] * slot t (output aliasing input 0); want_norm: scalars[0] = ||result||^2
 *   MULTIDOT       k = 0..cap-1, nvec = k+1: scalars[i] = <w, V_i>, i < k; scalars[k] = <w, w>
 *   MULTIDOT_GRAM  k = 1..min(32, cap-1), nvec = k+1: scalars[i] = <w, V_i>; scalars[k+i] = <V_{k-1}, V_i>, i < k; scalars[2k] = <w, w>
 *   GS_UPDATE      k = 1..cap-1, nvec = k+1: w <- (w - sum_i coef[i] V_i) * alpha
 *   BASIS_AXPY     k = 1..cap-1, nvec = k+1: w <- beta * w + sum_i coef[i] V_i (beta = 0: w is not read; coef[i] = 0: V_i is not read);
 *                  want_norm: scalars[0] = ||result||^2
 *   GS_UPDATE_DEV  k = 1..min(32, cap-1), nvec = k+1: GS_UPDATE by the pipelined solver's kernel; coef and alpha are first put where its
 *                  small-algebra kernel leaves coefficients and scale on the device
 *   GMRES_COEF     k = 1..min(32, cap-1), no vectors: the pipelined solver's small-algebra kernel for columns j = 0..k-1 in sequence on the
 *                  handle's device block.  coef_host = the reduced rows of every column one after the other, column j in the order of
 *                  MULTIDOT_GRAM with j+1 vectors (2j+3 numbers); beta = norm of the start residual.  scalars: per column k+3 numbers
 *                  [coef[0..k) (the first j+1 are the column's), scale = 1/hn, residual estimate, hn], then the triangular factor the Givens
 *                  rotations have made of the Hessenberg matrix, column c at [c*(k+1), (c+1)*(k+1)), then the rotated right-hand side
 *                  g[0..k]: k*(k+3) + k*(k+1) + k+1 numbers in all.
 * want_norm != 0 on another operation: KSFD_EINVAL. */
enum { KSFD_KOP_LINCOMB = 0, KSFD_KOP_MULTIDOT = 1, KSFD_KOP_MULTIDOT_GRAM = 2, KSFD_KOP_GS_UPDATE = 3, KSFD_KOP_BASIS_AXPY = 4,
       KSFD_KOP_GS_UPDATE_DEV = 5, KSFD_KOP_GMRES_COEF = 6 };
int ksfd_krylov_op(ksfd_handle *h, int32_t op, int32_t k, int32_t want_norm, const double *coef_host, double alpha, double beta,
                   const double *vecs_host, double *out_vecs_host, double *scalars_out, int32_t layout);
/* Parity/test entries of the stage right-hand sides and of the frozen Jacobian action, the twins of ksfd_krylov_op and ksfd_mg_part: the
 * functions the step itself calls (stage_rhs, stage_gram_guess, step_finish, err_materialize, op_jvp_frozen_halo, op_residual32,
 * poly_apply) run on host vectors, never a kernel launch of the entries' own, so every launch mode, its geometry and its epilogue show.
 * Both work at the resident state (ghost rows exchanged and coefficient planes made as at the head of a step, but NO groom: the kernels
 * clamp on load) and leave the state and what the stepper remembers from step to step untouched.  Host vectors: ksfd_local_size doubles
 * in `layout`.  KSFD_EINVAL before anything is touched on a bad argument.
 *
 * ksfd_stage_rhs: the right-hand sides b_0 .. b_{nstages-1} (nstages 1..4) of one attempt with step size hstep whose stage vectors
 * Y_0 .. Y_{nstages-2} are the caller's (y_host, one after the other; with fin_host: four), formed in order exactly as step_attempt forms
 * them, with the stage guesses' Gram bookkeeping wherever the attempt would keep it.  regime 0: plain (no norm, no guess); 1: spectral
 * (||b_i||^2 and, with guesses, <b_i, b_j> from the store epilogue of the 2-D strip kernel); 2: multigrid (guesses, inner products by
 * a multi-dot).  Whether the stage algebra is fused and whether guesses are on follows the rules of the step (KSFD_TUNE_UNFUSED_STAGE,
 * _GENERIC_RHS3D, _NO_SPEC_GUESS, _NO_RHS_CARRY, _OWN_DOTS, _NO_GPLANE and the handle's solvers).  b_host receives nstages vectors.  fin_host != NULL (nstages = 4, four Y vectors): step_finish with
 * atol / rtol, then err_materialize; fin_host receives the new state (from the completion's output buffer; the state is not advanced) and
 * the embedded error vector, info wrms and below.  The stage vectors, the stored right-hand sides and the error vector buffer are
 * overwritten: ksfd_get_last_error_vector afterwards answers as after a step that completed no attempt. */
typedef struct ksfd_stage_info {
    int32_t fuse_stage, guess_on;      /* AttemptPlan of the run */
    int32_t path;                      /* kernel path of the grid: 0 2-D strip, 1 3-D second generation (k_jvp3d_lds), 2 3-D first generation, 3 generic */
    int32_t rhs_strip;                 /* the RHS ran on a strip kernel (2-D: k_rhs2d_fused, 3-D: k_rhs3d_strip) */
    int32_t seg, nseg, nstrips, rows;  /* RHS launch geometry: rows (2-D) or planes (3-D) per segment, segments, strips, y rows per block (3-D) */
    int32_t overlap;                   /* launches with a stage vector whose ghost rows travel: interior + boundary launches with split partials */
    int32_t dots_done[4];              /* per stage: <b_i, b_j> came from the RHS epilogue */
    int32_t guess_n[4];                /* per stage: vectors of the stage guess */
    double bnorm2[4];                  /* per stage: ||b_i||^2 as the stage solve would get it, -1 where none */
    double gb[16];                     /* Gram matrix of the right-hand sides, row-major 4 x 4; NaN where the attempt never forms the entry */
    double guess_c[16];                /* [4 i + j]: coefficient of Y_j in the guess of stage i */
    double wrms, below;                /* of the completion (fin_host) */
} ksfd_stage_info;
int ksfd_stage_rhs(ksfd_handle *h, int32_t regime, int32_t nstages, double hstep, double atol, double rtol, const double *y_host,
                   double *b_host, double *fin_host, ksfd_stage_info *info, int32_t layout);
/* ksfd_stage_jvp: one frozen Jacobian action at the resident state.
 *   op 0: out = op_jvp_frozen_halo(v, mode, shift, yadd = y, alpha, beta); mode 0: J v, 1: A v = shift v - J v, 2: y - A v,
 *         3: alpha y + beta A v, 4: alpha v + beta A v (y_host needed for modes 2 and 3)
 *   op 1: op_residual32(x = v, shift, b = y): out = the fp32 values of b - A x widened to double, scalars[0] = ||r||^2 from the store
 *         epilogue; KSFD_EINVAL where the spectral solver would not take the fused residual (no strip kernel on the grid)
 *   op 2: out = poly_apply(v) with the polynomial sum_i coef[i] (A/shift)^i, i = 0 .. deg (deg 1..7), installed for the call and put back
 *         afterwards; fp32 or fp64 Horner temporaries exactly as the handle would take them (KSFD_TUNE_POLY_FP64)
 * scalars (8 doubles): [0] see op 1; [1] path as in ksfd_stage_info; [2] rows (2-D) or planes (3-D) per segment of the launch, [3] segments,
 * [4] strips, [5] 1 where op 2 took the fp32 path, [6] 1 where the launches were interior + boundary (ghost rows of v travelling), [7] y rows
 * per block (3-D).  Needs the frozen action (KSFD_TUNE_RECOMPUTE_JVP clear), else KSFD_EINVAL. */
int ksfd_stage_jvp(ksfd_handle *h, int32_t op, int32_t mode, double shift, double alpha, double beta, int32_t deg, const double *coef,
                   const double *v_host, const double *y_host, double *out_host, double *scalars, int32_t layout);
/* ksfd_bench_kernel classes beyond the profile's kernel classes: the rotation kernel on 31 -> 11 vectors in one pass, and the same
 * rotation composed from 11 basis combinations of 31 vectors (out of place); one factorization of the banded direct solver (assembly
 * and the read-back of info included, at the shift of the last ksfd_banded_apply or pc_type 6 attempt) and one of its solves */
#define KSFD_BENCH_ROTATE 100
#define KSFD_BENCH_ROTATE_COMPOSED 101
#define KSFD_BENCH_BAND_FACTOR 102
#define KSFD_BENCH_BAND_SOLVE 103
/* exact coarse solve of the V cycle (ksfd_set_mg_coarse kind 1 first), at a shift of 1: one set-up (assembly, factorization with one launch
 * per panel, inversion, the host wait for the flag), one apply, and for comparison assembly + the two-launches-per-column factorization
 * of pc_type 5 on the same matrix */
#define KSFD_BENCH_MGC_SETUP 104
#define KSFD_BENCH_MGC_APPLY 105
#define KSFD_BENCH_MGC_FACTOR_COLUMNS 106

#ifdef __cplusplus
}
#endif
#endif /* KSFD_HIP_H */
