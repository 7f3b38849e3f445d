// libksfd_hip.so -- the handle: device buffers, solver state, error reporting, HIP-event profiling scopes, tableau and physics tables
// (part of the single translation unit ksfd_hip.hip, first of its host-side headers: the include list there gives the order)
#pragma once
#include "spectral_plan.h"
#include "handle_state.h"
#include "tuning.h"
#include "krylov_small.h"
// ------------------------------------------------------------------------------------------------
// kernel classes for the profile
enum { KC_RHS = 0, KC_JVP, KC_MULTIDOT, KC_GSUPDATE, KC_LINCOMB, KC_BASISAXPY, KC_FINISH, KC_REDUCE,
       KC_GFIELD, KC_VELOCITY, KC_MISC, KC_HALO, KC_MG, KC_SPECTRAL };
static const char *kc_names[KSFD_NKCLASS] = { "rhs", "jvp", "multidot", "gs_update", "lincomb", "basis_axpy",
                                              "rosw_finish", "reduce", "gfield", "velocity", "misc", "halo", "mg", "spectral" };
extern "C" const char *ksfd_kernel_class_name(int32_t c) { return (c >= 0 && c < KSFD_NKCLASS) ? kc_names[c] : "?"; }

static thread_local std::string g_create_error;

struct EvPair { hipEvent_t a, b; int cls; };

// level vectors of the V cycle in the storage type T: solution, right-hand side, residual, Chebyshev direction
template <typename T>
struct MGVecs { T *x = nullptr, *b = nullptr, *r = nullptr, *d = nullptr; };

// one grid of the multigrid hierarchy (level 0 = the solver's own grid; see mg.hip.h)
struct MGLevel {
    KGeom G;
    KPhys P;
    KVec kv;
    int64_t vlen = 0;
    int nblk = 1;
    double *coef = nullptr;    // [rho, G, G_rho, G_U..] planes (level 0 aliases the handle's)
    float *dinv = nullptr;     // F*F planes (fp32)
    MGVecs<double> v64;        // level 0 has no x and b: they are the caller's vectors
    MGVecs<float> v32;         // f32 levels only
    template <typename T> MGVecs<T> &vecs() { if constexpr (std::is_same<T, float>::value) return v32; else return v64; }
    double *Ad = nullptr, *dG = nullptr;
    float *coef32 = nullptr;   // fp32 copy of the coefficient planes of a coarse f32 level (level 0 uses the handle's)
    bool f32 = false;          // this level can run the fp32 cycle (2-D strip kernel, not the coarsest level)
    bool rep = false;          // slab ranks: every rank holds this WHOLE level and computes it redundantly (ksfd_set_mg_agglomerate): no ghost
                               // units, no halo exchange, the slow axis wraps in the kernels, norms are local
    double *pv = nullptr;      // power-iteration vector of Dinv*A, kept from one set-up to the next (warm start)
    double pv_norm = 0.0;      // its norm; 0 = no vector yet
    double lam_max = 2.3;
    double ratio = 60.0;       // lambda_max/lambda_min estimate (used on the coarsest grid)
};

// spectral preconditioner (spectral.hip.h / spectral_plan.h / spectral_host.hip.h): what spec_build makes of the planner's shape
struct SpecState {
    bool ok = false;
    SpecShape shape;
    // work arrays W: [pair][pos_x][y_local]; W2: after the all-to-all, [rank][pair][own pos][y_local] (nch = 3: [chunk] in front of [pair] in both)
    kcf *W = nullptr, *W2 = nullptr, *twx = nullptr, *twy = nullptr, *twz = nullptr;
    int *spos = nullptr, *skof = nullptr;    // slow axis (2-D: y, 3-D: z): position of a wavenumber, wavenumber at a position
    int2 *ytab = nullptr;                    // per position of the slow axis: (position of -k, bits of its symbol) -- symbol stage of k_spec_cols / k_spec3_z
    int4 *pairtab = nullptr;                 // SpecTables.pairtab
    float *lx = nullptr, *ly = nullptr, *lz = nullptr;
    // the kernel instances this handle launches, chosen once (spec_build raises the dynamic-LDS limit of exactly these)
    decltype(&k_spec_rows_fwd<double>) k_rows_fwd64 = nullptr;
    decltype(&k_spec_rows_fwd<float>) k_rows_fwd32 = nullptr;
    decltype(&k_spec_rows_inv) k_rows_inv = nullptr;
    decltype(&k_spec_cols<0>) k_cols = nullptr;
    decltype(&k_spec_cols_split<false>) k_cols_split = nullptr;
    decltype(&k_spec3_y_fwd<false>) k_y_fwd = nullptr;
    decltype(&k_spec3_y_inv<false>) k_y_inv = nullptr;
    decltype(&k_spec3_z<0, false>) k_z = nullptr;
    std::vector<A2APiece> a2a_fwd_s, a2a_fwd_r, a2a_back_s, a2a_back_r;
    double a_rr = 0.0, a_rU[KSFD_MAXL] = { 0 };       // means of rho*G_rho, rho*G_Ul (spec_means)
    bool user_off = false;                   // ksfd_set_spectral_params(enable = 0): off until enabled again; a checkpoint restore does not bring it back
};

// dense direct solver, pc_type 5 (lu.hip.h / lu_host.hip.h): buffers allocated on first use, factors rebuilt every step attempt
struct LUState {
    int64_t n = 0, nnz = 0;
    double *A = nullptr;                     // n x n factors, column-major (L unit-lower below the diagonal, U on and above)
    int *piv = nullptr, *perm = nullptr, *info = nullptr;
    long long *col = nullptr;                // Jacobian entries staged by k_jac_csr
    double *val = nullptr;
    double *y = nullptr, *z = nullptr;       // triangular-solve work vectors
    std::vector<int> piv_h, perm_h;
    bool valid = false;                      // a factorization exists: A holds the factors of shift*I - J for `shift`, at the planes as they were when
                                             // it was made (every step attempt and every apply entry factors before it solves; nothing ends this)
    double shift = 0.0;
};

// exact solve on the level the V cycle ends on (ksfd_set_mg_coarse; mg_coarse_plan.h, lu.hip.h, mgc_* in lu_host.hip.h).  The buffers are
// allocated when kind 1 is set and live as long as the handle does; the factors and the inverse are rebuilt by every mg_setup_shift
// from the level's restricted coefficient planes, so nothing of this joins a checkpoint.
struct MGCoarse {
    int kind = 0;                            // 0 Chebyshev on the coarsest level, 1 exact solve
    int max_unknowns = 0;
    int level = -1;                          // level the cycle ends on (mg_build: the coarsest)
    LUState lu;                              // shift*I - J_c and its factors
    double *inv = nullptr;                   // (shift*I - J_c)^-1, row-major
    int info_h = 0;
    int32_t factorizations = 0, solves = 0, fallbacks = 0;
    int32_t graph_solves = 0;                // coarse solves inside the captured part of the cycle, counted at every replay
};

// the coarse tail of the V cycle in one workgroup launch (ksfd_set_mg_tail; mg_tail_plan.h, k_mg_tail in mg.hip.h, mg_tail_* in
// mg_host.hip.h).  The plan is remade by every mg_build from max_points; nothing of this joins a checkpoint.
struct MGTail {
    int64_t max_points = 0;                  // 0: off (the default)
    int level = -1;                          // first tail level t >= 1, or -1: no level qualifies, the cycle is the one without the call
    int nlev = 0;                            // levels t .. the level the cycle ends on
    long long lds = 0;                       // dynamic LDS bytes of the launch (the plan's sum)
    int64_t launches = 0;                    // over the handle's life
    int64_t graph_launches = 0;              // launches inside the captured part of the cycle, counted at every replay
};

// banded direct solver for 1-D grids, pc_type 6 (banded_plan.h / banded.hip.h / banded_host.hip.h): allocated on first use, factors
// rebuilt every step attempt; the pivot indices never leave the device
struct BandState {
    BandPlan B = {};
    int64_t nnz = 0;
    double *AB = nullptr;                    // band storage of the factors (LAPACK gbtrf layout, ldab = 2 kl + ku + 1)
    int *piv = nullptr, *info = nullptr;
    long long *col = nullptr;                // Jacobian entries staged by k_jac_csr
    double *val = nullptr;
    double *z = nullptr;                     // L^-1 P b between the two sweeps of a solve
    int threads = 0;                         // workgroup of k_band_factor (64 or 256)
    bool valid = false;                      // a factorization exists (as LUState::valid)
    double shift = 0.0;
};

struct ksfd_handle {
    ksfd_config cfg;
    int32_t lig_group[KSFD_MAXL];
    double lig_w[KSFD_MAXL], lig_s[KSFD_MAXL], lig_gamma[KSFD_MAXL], lig_D[KSFD_MAXL];
    double grp_alpha[KSFD_MAXL], grp_beta[KSFD_MAXL];
    KGeom G;
    KPhys P;
    KPhys Pst[4];                    // ps.values(t_stage) for the four stage RHS evaluations (ksfd_set_stage_params)
    bool Pst_valid[4] = { false, false, false, false };
    KVec kv;
    int rank = 0, size = 1, device = 0;
    bool ring = false;               // ghost units + transport in use: size > 1, or ONE rank that is its own ring neighbour (ksfd_dist.size = 1 with a
                                     // transport: the RCCL path executed end to end on a single GPU)
    int64_t slow0 = 0;               // first owned global slow index
    hipStream_t st = nullptr;
    hipStream_t st_comm = nullptr;            // halo exchange stream (overlapped with interior rows)
    hipEvent_t ev_ready = nullptr, ev_halo = nullptr;
    Transport *tr = nullptr;
    std::string err;

    // device vectors (each F*plane doubles)
    int64_t vlen = 0;
    double *u = nullptr, *usave = nullptr, *Z = nullptr, *bvec = nullptr, *Y = nullptr, *V = nullptr;
    double *t1 = nullptr, *t2 = nullptr, *t3 = nullptr, *errv = nullptr;
    // u and usave trade places at every accepted step (step_run): the completion writes the new state into usave.  Nothing may keep
    // either pointer across a step
    double *ckpt = nullptr;                 // ksfd_checkpoint slot (allocated on first save)
    double *bstore = nullptr;               // right-hand sides of stages 0..2 of the current step (initial guesses of the spectral solves)
    long long n_predicted = 0;              // spectral solves that ended with a predicted last sweep (spec_solve)
    long long n_residual = 0;               // true residuals evaluated by the spectral defect correction
    long long n_host_sync = 0;              // host waits on the device so far (reduction results, stream synchronisations)
    SpecState spec;
    // what the solvers remember from one step to the next (step_control.h), and the copy a checkpoint holds: besides the state vector
    // this is all that ksfd_checkpoint saves and restores
    ksfd_ctl::StepMemo memo, ckpt_memo;
    double spec_from = 0.1;                 // stiffness above which pc_type 2 prefers the spectral solver (below: plain GMRES; measured at 4096^2, X = 0.19: 6 sweeps = 7.3 ms against 5 GMRES iterations = 7.9 ms per step)
    bool ckpt_valid = false;
    double *Gb = nullptr, *dGb = nullptr;   // generic-path scratch planes
    double *coef = nullptr;                 // frozen-Jacobian coefficient planes [rho, G, G_rho, G_U..]
    // which of the derived data below still belongs to the state and the configuration as they are now: handle_state.h, whose events
    // are the only writers
    ksfd_ctl::Current cur;
    double *flat = nullptr;                 // staging for host layouts: max(F,dim)*nloc
    double *src[4][KSFD_MAXL + 1];          // dense source planes per stage (lazy)
    double *part = nullptr;                 // block partials
    double *dres = nullptr;                 // reduced results (device)
    double *hres = nullptr;                 // pinned host mirror
    // zero-copy hand-over of reduction results: the kernel stores into hres through its device alias and raises pub_flag
    double *hres_dev = nullptr;             // NULL: the buffer could not be mapped (zero_copy_on)
    unsigned long long *pub_flag = nullptr, *pub_flag_dev = nullptr, pub_seq = 0;
    unsigned int *pub_count = nullptr;
    int restart_alloc = 0;                  // basis vectors V / Zb hold (ksfd_create: 30 ... 120 by the free HBM)
    int nblk_vec = 0;                       // grid.x of the BLAS-1 kernels

    // the switches between code paths (tuning.h): ksfd_set_tuning and ksfd_set_mg_params write them, through tuning_apply / tuning_mg_graph only
    ksfd_ctl::Tuning tune;

    // profile
    bool profiling = false;
    int prof_only = -1;             // >= 0: HIP events only around launches of this kernel class
    std::vector<EvPair> pending;
    std::vector<hipEvent_t> pool;
    ksfd_profile prof;
    double bytes_acc = 0.0;

    // pipelined GMRES (device-resident Hessenberg / Givens state, see gmres_async)
    double *gm_dev = nullptr;       // [G (m+1)^2 | H (m+1)m | cs m | sn m | g m+1 | coef MAXDOT | scale 1 | mon 2(m+1)]
    double *gm_host = nullptr;      // pinned: [mon 2(m+1) | H (m+1)m | g m+1]
    std::vector<hipEvent_t> gm_ev;

    // polynomial (Chebyshev) preconditioner + flexible GMRES (see poly_setup / gmres)
    double *Zb = nullptr;           // preconditioned basis z_j = p(A) v_j (allocated on first use)
    double *pvec = nullptr;         // power-iteration vector for lambda_max(A)
    int poly_deg = 0;
    double poly_alpha[8];           // z = sum_i alpha_i (A/shift)^i v
    int poly_max_deg = 6;
    double mg_threshold = 75.0;      // stiffness above which pc_type 2 switches from the polynomial to multigrid
    double poly_target = 0.02;      // wanted reduction per outer iteration (picks the degree)
    float *coef32 = nullptr;        // fp32 copy of the frozen coefficient planes (2-D strip path only)
    bool coef32_failed = false;     // its allocation failed: coef32_alloc does not try again until ksfd_set_tuning passes a word
    bool j3l_attr_set = false, j3l_usable = false;   // k_jvp3d_lds: dynamic LDS size registered / usable (ops.hip.h: j3l_ok)

    // asynchronous snapshots for writers (ksfd_snapshot_begin / _wait): layout transform on the compute stream into a
    // device staging slot, D2H on a third stream into pinned memory while the stepper carries on
    hipStream_t st_io = nullptr;
    double *snap_dev[2] = { nullptr, nullptr }, *snap_host[2] = { nullptr, nullptr };
    hipEvent_t snap_ready[2] = { nullptr, nullptr }, snap_done[2] = { nullptr, nullptr };
    bool snap_busy[2] = { false, false };
    int snap_next = 0;

    // Krylov recycling across the four stage systems of one step (same matrix): see gmres()
    struct RecSpace { int vb = 0, zb = 0, k = 0, pc = 0; std::vector<double> H; };   // leading (k+1) x k raw Hessenberg, ld = k+1; in force while cur.rec_valid[stage]
    RecSpace rec[4];

    // Deflated restart of GMRES (krylov_dr.hip.h; ksfd_set_deflation).  keep = 0: off, every other solver path is as without it.
    int dr_keep = 0;                 // harmonic Ritz vectors kept across a restart (1..16)
    bool dr_carry = false;           // the kept relation also serves the later stage systems of a step attempt
    double *dr_P = nullptr, *dr_Phost = nullptr;      // rotation matrix of op_basis_rotate: device copy and pinned staging (KSFD_ROT_MAXIN x KSFD_ROT_MAXOUT)
    // A M^-1 V_kk = V_kk+1 H (H (kk+1) x kk column-major) in the leading slots of V (and Zb) while cur.dr_valid: for this matrix, shift and preconditioner only
    struct DrKept { int kk = 0, pc = -1; double shift = 0.0, shift_pc = 0.0; std::vector<double> H; };
    DrKept dr;
    ksfd_deflation_stats dr_stats = {};

    LUState lu;
    BandState band;
    MGCoarse mgc;
    MGTail mgt;

    // multigrid preconditioner
    std::vector<MGLevel> mg;
    bool mg_use32 = false;       // V cycle with fp32 level vectors: decided per step by ksfd_step (tune.mg_fp32 and ksp_rtol >= 1e-7)
    bool mg_ok = false;          // hierarchy exists (2-D, single rank, >= 2 levels)
    int64_t mg_agg = 0;          // slab ranks: 0 = every level distributed; > 0: coarse levels replicated (mg_agglomerate_plan.h)
    hipGraphExec_t mg_graph = nullptr;   // captured coarse part of the V cycle (levels >= 1) under the key in cur (graph_current)
    double mg_graph_bytes = 0.0;
    bool capturing = false;
    int mg_nu = 2, mg_ncoarse = 400, mg_power_its = 8;   // smoothing sweeps, cap on coarsest-grid sweeps, power iterations
    double mg_ratio = 6.0, mg_coarse_tol = 0.3;    // coarsest-grid reduction target: 0.3 is enough (tools/mg_longrun_tune.py: 24.3 -> 19.9 ms/step at 384^2, same iterations)

    // ROSW tableau (PETSc transformed form)
    double At[4][4], Ginv[4][4], bt[4], b2t[4], asum[4];
};

#define GAMMA_RA 4.3586652150845900e-01

// a switch of tune that also takes a fact about the handle.  Reduction results through the mapped flag: the buffer is mapped
static inline bool zero_copy_on(const ksfd_handle *h) { return h->tune.zero_copy && h->hres_dev; }
// fp32 copy of the coefficient planes read by the polynomial and by level 0 of the V cycle: the buffer exists (ops.hip.h: coef32_alloc)
static inline bool coef32_on(const ksfd_handle *h) { return h->tune.poly_fp32 && h->coef32; }
// coarse part of the V cycle from a captured graph: not on slab ranks, whose cycle has collectives inside
static inline bool mg_graph_on(const ksfd_handle *h) { return h->tune.mg_use_graph && !h->ring; }

// The environment knobs outside the spectral planner's (spec_knobs, spectral_host.hip.h) and the transport's KSFD_VRED_MAX (transport.h,
// per transport), read here and nowhere else, once per process at first use.  All are experiment or diagnostic knobs
struct EnvKnobs {
    long long waves_jvp = 4096, waves_rhs = 6144;   // KSFD_WAVES_JVP / _RHS: wave target of the 2-D strip launches (tools/yseg_sweep.py)
    int rows3d = 0;                 // KSFD_ROWS3D = 8: eight y rows per block of the 3-D strip kernels (one ligand), else four
    int sync3d = 1;                 // KSFD_SYNC3D = 0: no barrier per plane in the 3-D strip kernels
    int j3l = 1;                    // KSFD_J3L = 0: the first-generation 3-D Jacobian action where k_jvp3d_lds would serve
    int spec_verify = 0;            // KSFD_SPEC_VERIFY: 1 checks the predicted sweeps, 2 switches them off (step_control.h: spec_predict_on)
    bool spec_trace = false;        // KSFD_SPEC_TRACE: residual history of the defect correction on stderr
    bool stage_trace = false;       // KSFD_STAGE_TRACE: iterations per stage system on stderr
    int restart_cap = ksfd_krylov::RESTART_MAX;     // KSFD_RESTART_MAX: cap on the basis vectors ksfd_create sizes V / Zb for
    // KSFD_GUESS_MAX (1..3): earlier stages a stage guess is built from (the most recent ones).  Measured on the pinned window at 4096^2: 3 vectors 9.80 ms
    // per step, 2 vectors 9.67 (same sweep counts, two full-vector reads and a multi-dot operand less for stage 4), 1 vector 9.75 (one more sweep)
    int guess_max = 2;
    bool pc_sigma_set = false;      // KSFD_PC_SIGMA: fixed shift floor of the multigrid preconditioner instead of the online search
    double pc_sigma = 0.0;
    int band_threads = 0;           // KSFD_BAND_THREADS: workgroup of k_band_factor, 256 (>= 256) or 64; 0: banded_factor's own choice
};
static const EnvKnobs &env_knobs()
{
    static const EnvKnobs K = [] {
        EnvKnobs E;
        if (const char *v = getenv("KSFD_WAVES_JVP")) E.waves_jvp = atoll(v);
        if (const char *v = getenv("KSFD_WAVES_RHS")) E.waves_rhs = atoll(v);
        if (const char *v = getenv("KSFD_ROWS3D")) E.rows3d = atoi(v);
        if (const char *v = getenv("KSFD_SYNC3D")) E.sync3d = atoi(v);
        if (const char *v = getenv("KSFD_J3L")) E.j3l = atoi(v);
        if (const char *v = getenv("KSFD_SPEC_VERIFY")) E.spec_verify = atoi(v);
        E.spec_trace = getenv("KSFD_SPEC_TRACE") != nullptr;
        E.stage_trace = getenv("KSFD_STAGE_TRACE") != nullptr;
        if (const char *v = getenv("KSFD_RESTART_MAX")) E.restart_cap = ksfd_krylov::restart_cap(atoi(v));
        if (const char *v = getenv("KSFD_GUESS_MAX")) E.guess_max = std::max(1, std::min(atoi(v), 3));
        if (const char *v = getenv("KSFD_PC_SIGMA")) { E.pc_sigma_set = true; E.pc_sigma = atof(v); }
        if (const char *v = getenv("KSFD_BAND_THREADS")) E.band_threads = atoi(v) >= 256 ? 256 : 64;
        return E;
    }();
    return K;
}

static int fail(ksfd_handle *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}
#define HIPCHK(h, call)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return fail(h, KSFD_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ---- profiling helpers -------------------------------------------------------------------------
static hipEvent_t ev_get(ksfd_handle *h)
{
    if (!h->pool.empty()) { hipEvent_t e = h->pool.back(); h->pool.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}
struct Scope {
    ksfd_handle *h; EvPair p; bool on;
    // alg < 0: the implementation moves exactly the algorithmic bytes
    Scope(ksfd_handle *h_, int cls, double bytes, double alg = -1.0) : h(h_), on(h_->profiling && !h_->capturing && (h_->prof_only < 0 || h_->prof_only == cls))
    {
        h->bytes_acc += bytes;
        h->prof.bytes[cls] += bytes;
        h->prof.alg_bytes[cls] += alg < 0.0 ? bytes : alg;
        h->prof.launches[cls] += 1;
        if (on) { p.a = ev_get(h); p.b = ev_get(h); p.cls = cls; hipEventRecord(p.a, h->st); }
    }
    ~Scope() { if (on) { hipEventRecord(p.b, h->st); h->pending.push_back(p); } }
};
static void prof_resolve(ksfd_handle *h)
{
    if (h->pending.empty()) return;
    hipStreamSynchronize(h->st);
    for (auto &p : h->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) h->prof.ms[p.cls] += ms;
        h->pool.push_back(p.a);
        h->pool.push_back(p.b);
    }
    h->pending.clear();
}

// ---- small utilities ---------------------------------------------------------------------------
static inline dim3 vgrid(const ksfd_handle *h) { return dim3(h->nblk_vec, h->G.F); }
static inline double vbytes(const ksfd_handle *h, double nvec) { return nvec * 8.0 * (double)h->G.F * (double)h->G.nloc; }

static void build_tableau(ksfd_handle *h)
{
    static const double A[4][4] = { { 0, 0, 0, 0 }, { 8.7173304301691801e-01, 0, 0, 0 },
                                    { 8.4457060015369423e-01, -1.1299064236484185e-01, 0, 0 }, { 0, 0, 1., 0 } };
    static const double Gm[4][4] = { { GAMMA_RA, 0, 0, 0 }, { -8.7173304301691801e-01, GAMMA_RA, 0, 0 },
                                     { -9.0338057013044082e-01, 5.4180672388095326e-02, GAMMA_RA, 0 },
                                     { 2.4212380706095346e-01, -1.2232505839045147e+00, 5.4526025533510214e-01, GAMMA_RA } };
    static const double b[4] = { 2.4212380706095346e-01, -1.2232505839045147e+00, 1.5452602553351020e+00, GAMMA_RA };
    static const double b2[4] = { 3.7810903145819369e-01, -9.6042292212423178e-02, 0.5, 2.1793326075422950e-01 };
    memset(h->Ginv, 0, sizeof h->Ginv);
    for (int col = 0; col < 4; col++)
        for (int i = col; i < 4; i++) {
            double s = (i == col) ? 1.0 : 0.0;
            for (int k = col; k < i; k++) s -= Gm[i][k] * h->Ginv[k][col];
            h->Ginv[i][col] = s / Gm[i][i];
        }
    for (int i = 0; i < 4; i++) {
        h->asum[i] = 0.0;
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += A[i][k] * h->Ginv[k][j];
            h->At[i][j] = s;
            h->asum[i] += A[i][j];
        }
    }
    for (int j = 0; j < 4; j++) {
        double s = 0.0, s2 = 0.0;
        for (int k = 0; k < 4; k++) { s += b[k] * h->Ginv[k][j]; s2 += b2[k] * h->Ginv[k][j]; }
        h->bt[j] = s;
        h->b2t[j] = s2;
    }
}

static int fill_phys(ksfd_handle *h, const ksfd_config *c, KPhys *dst = nullptr)
{
    if (c->nlig < 1 || c->nlig > KSFD_MAXL || c->ngroups < 1 || c->ngroups > KSFD_MAXL)
        return fail(h, KSFD_EINVAL, "nlig=%d ngroups=%d outside 1..%d", c->nlig, c->ngroups, KSFD_MAXL);
    KPhys &P = dst ? *dst : h->P;
    memset(&P, 0, sizeof P);
    P.nlig = c->nlig; P.ngroups = c->ngroups; P.cap_kind = c->cap_kind;
    for (int a = 0; a < 3; a++) {
        double sp = c->L[a] / (double)c->n[a];
        P.inv_h[a] = 1.0 / sp;
        P.inv_h2[a] = 1.0 / (sp * sp);
    }
    P.s2 = c->s2; P.rhomax = c->rhomax; P.inv_cushion = 1.0 / c->cushion; P.ms = c->maxscale * c->s2;
    P.rhomin = c->rhomin; P.Umin = c->Umin; P.inv_rhomax = 1.0 / c->rhomax;
    for (int l = 0; l < c->nlig; l++) {
        if (c->lig_group[l] < 0 || c->lig_group[l] >= c->ngroups) return fail(h, KSFD_EINVAL, "lig_group[%d] out of range", l);
        P.lig_group[l] = h->lig_group[l] = c->lig_group[l];
        P.lig_w[l] = h->lig_w[l] = c->lig_w[l];
        P.lig_s[l] = h->lig_s[l] = c->lig_s[l];
        P.lig_gamma[l] = h->lig_gamma[l] = c->lig_gamma[l];
        P.lig_D[l] = h->lig_D[l] = c->lig_D[l];
    }
    for (int l = c->nlig; l < KSFD_MAXL; l++) P.lig_group[l] = -1;
    for (int q = 0; q < c->ngroups; q++) {
        P.grp_alpha[q] = h->grp_alpha[q] = c->grp_alpha[q];
        P.grp_beta[q] = h->grp_beta[q] = c->grp_beta[q];
    }
    return KSFD_OK;
}

static int alloc_d(ksfd_handle *h, double **p, int64_t n)
{
    if (hipMalloc((void **)p, sizeof(double) * (size_t)n) != hipSuccess) return fail(h, KSFD_ENOMEM, "hipMalloc of %lld doubles failed", (long long)n);
    return KSFD_OK;
}
