// libksfd_hip.so -- the Rosenbrock-W step driver: what one attempt of a step is made of.  The decisions (which solver, which guess, how the
// solvers' step-to-step memory and the step size move) are host arithmetic in step_control.h; here are the parts that launch:
//   plan_attempt          regime of this attempt (choose_regime) and what it needs on the device before the stages start
//   stage_rhs             right-hand side b_i of stage i, fused (KComb inside the RHS kernel, norm and dots from its epilogue) or unfused
//   stage_gram_guess      Gram matrix of the right-hand sides of the attempt -> coefficients of the stage guess (stage_guess)
//   stage_solve           direct (dense or banded) / spectral with its fallbacks / V cycle from a guess / the GMRES variants, and the multigrid retry
//   step_attempt          the four stages
//   step_finish           completion u_new = u + sum bt_i Y_i (out of place), the WRMS norm of the embedded error, the count of values under their floor
//   err_materialize       the embedded error vector itself, when somebody asks for it
//   stats_begin / _end    the ksfd_step_stats counters
// ksfd_step (ksfd_hip.hip) is the attempt loop of TSStep_RosW over them.
// (part of the single translation unit ksfd_hip.hip; included last)
#pragma once
using ksfd_ctl::StepMemo;

// what plan_attempt decides for one attempt
struct AttemptPlan {
    double hh, shift, stiff;
    bool direct, dr_on;                       // pc_type 5 or 6 / deflated restarting (decided once per step)
    bool banded;                              // ... the direct solver is the banded one (pc_type 6)
    bool use_spec, use_pc, use_poly, use_async;
    bool fuse_stage;                          // stage argument and Zdot term folded into the RHS kernel
    bool guess_on;                            // stage guesses from the earlier stages of the attempt
};

// right-hand side of a stage as stage_rhs leaves it
struct StageRhs {
    double *b;
    double bnorm2 = -1.0;                     // ||b||^2 when the RHS kernel's epilogue delivered it (or the Gram bookkeeping since)
    bool dots_done = false;                   // ... and <b_i, b_j> for the stage guess with it
    double dot[2] = { 0.0, 0.0 };
};

struct StepCounters { double bytes; int64_t rhs, jvp, launches; long long sync, pred, resid; };

static int64_t launches_total(const ksfd_handle *h)
{
    int64_t n = 0;
    for (int c = 0; c < KSFD_NKCLASS; c++) n += h->prof.launches[c];
    return n;
}
static StepCounters stats_begin(const ksfd_handle *h)
{
    return { h->bytes_acc, h->prof.launches[KC_RHS], h->prof.launches[KC_JVP], launches_total(h), h->n_host_sync, h->n_predicted, h->n_residual };
}
static void stats_end(ksfd_handle *h, const StepCounters &c0, ksfd_step_stats &st)
{
    prof_resolve(h);
    st.bytes = h->bytes_acc - c0.bytes;
    st.rhs_evals = (int32_t)(h->prof.launches[KC_RHS] - c0.rhs);
    st.jvp_evals = (int32_t)(h->prof.launches[KC_JVP] - c0.jvp);
    st.launches = (int32_t)(launches_total(h) - c0.launches);
    st.host_syncs = (int32_t)(h->n_host_sync - c0.sync);
    st.predicted_final = (int32_t)(h->n_predicted - c0.pred);
    st.residual_evals = (int32_t)(h->n_residual - c0.resid);
}

// How the stages of an attempt are formed once its regime (use_spec, use_pc) is known; shared with the test entry ksfd_stage_rhs
static void plan_stage_forms(const ksfd_handle *h, AttemptPlan &p)
{
    p.fuse_stage = (fused_ok(h) || (strip3d_ok(h) && h->tune.rhs3d_strip)) && h->P.nlig <= 4 && h->tune.fuse_stage;
    // Initial guesses for the spectral stage solves from the earlier stages of the step (A Y_j = b_j is known): the right-hand
    // sides of a step are nearly dependent -- b_1 = c b_0 to ~1e-3, later ones to a few per cent (CPU experiment with the oracle)
    // -- so x0 = sum c_j Y_j, c = argmin ||b_i - sum c_j b_j||, starts the defect correction 1-3 digits ahead for one small
    // multi-dot.  The b_j are kept in bstore (three vectors); stage_gram_guess keeps their Gram matrix.
    p.guess_on = (p.use_spec || p.use_pc) && p.fuse_stage && h->tune.spec_guess && h->bstore;
}

// Regime of one attempt with step size hh.  lam_done: the eigenvalue estimate of the polynomial is looked at once per step, not per attempt.
static int plan_attempt(ksfd_handle *h, const ksfd_step_opts *opts, double hh, bool direct, bool dr_on, bool &lam_done, AttemptPlan &p)
{
    int rc;
    StepMemo &m = h->memo;
    p.hh = hh; p.direct = direct; p.dr_on = dr_on;
    p.banded = direct && opts->pc_type == 6;
    p.shift = 1.0 / (GAMMA_RA * hh);
    p.stiff = ksfd_ctl::stiffness(h->P.s2, h->P.lig_D, h->P.nlig, h->P.inv_h2, h->G.dim, p.shift);
    ksfd_ctl::RegimeIn in;
    in.pc_type = opts->pc_type; in.reserved = opts->reserved; in.stiff = p.stiff;
    in.direct = direct; in.dr_on = dr_on;
    in.spec_ok = h->spec.ok; in.user_off = h->spec.user_off;
    in.use_frozen = h->tune.use_frozen; in.fused2d = fused_ok(h);
    in.mg_ok = h->mg_ok; in.mg_threshold = h->mg_threshold; in.spec_from = h->spec_from;
    in.nsteps = m.nsteps; in.bad_until = m.spec_bad_until;
    in.unknowns = (double)h->G.F * (double)h->G.nloc;
    in.ring = h->ring; in.device_allreduce = h->ring && h->tr->device_allreduce();
    in.async_mode = h->tune.async_mode;
    const ksfd_ctl::Regime r = ksfd_ctl::choose_regime(in);
    p.use_spec = r.spec; p.use_pc = r.mg;
    if (p.use_spec) {
        if (!h->Zb && alloc_d(h, &h->Zb, (int64_t)h->restart_alloc * h->vlen)) return KSFD_ENOMEM;
        if (!h->cur.means_valid && (rc = spec_means(h))) return rc;
    }
    p.use_poly = false;
    if (r.poly_wanted) {
        if (!h->Zb && alloc_d(h, &h->Zb, (int64_t)h->restart_alloc * h->vlen)) return KSFD_ENOMEM;
        if (!lam_done) {
            if (ksfd_ctl::lam_due(m)) {
                const double before = m.lamJ;
                if ((rc = est_lambda_max(h, p.shift, ksfd_ctl::lam_power_its(before)))) return rc;
                ksfd_ctl::lam_estimated(m, before);
            }
            lam_done = true;
        }
        if (h->cur.poly_shift != p.shift) poly_setup(h, p.shift);
        p.use_poly = h->poly_deg >= 1 && h->poly_max_deg >= 1;
    }
    p.use_async = ksfd_ctl::pipelined_allowed(in, r, p.use_poly);
    h->mg_use32 = opts->ksp_rtol >= 1e-7;          // fp32 level vectors inside the V cycle (mg_vcycle<float>); tight tolerances keep fp64
    plan_stage_forms(h, p);
    return KSFD_OK;
}

static int stage_rhs(ksfd_handle *h, const AttemptPlan &p, int i, StageRhs &r)
{
    int rc;
    const int64_t vs = h->vlen;
    r.b = (p.guess_on && i < 3) ? h->bstore + (int64_t)i * vs : h->bvec;
    if (p.fuse_stage) {
        // stage argument and Zdot term folded into the RHS kernel (no Z vector, no separate passes)
        KComb cmb = KComb{};
        for (int j = 0; j < i; j++) {
            if (h->At[i][j] != 0.0) { cmb.yin[cmb.nin] = h->Y + (int64_t)j * vs; cmb.ain[cmb.nin++] = h->At[i][j]; }
            if (h->Ginv[i][j] != 0.0) { cmb.yout[cmb.nout] = h->Y + (int64_t)j * vs; cmb.aout[cmb.nout++] = -h->Ginv[i][j] / p.hh; }
        }
        // ||b||^2 from the store epilogue (2-D strip kernel), and with it the inner products of b_i with the right-hand sides the stage
        // guess is built from (the multi-dot of stage_gram_guess would read all of them again)
        const int gdot_j0 = std::max(0, i - env_knobs().guess_max), gdot_n = (p.guess_on && i > 0 && h->tune.rhs_dots) ? i - gdot_j0 : 0;
        const bool rhs_norm = p.use_spec && fused_ok(h) && (!(p.guess_on && i > 0) || (gdot_n > 0 && gdot_n <= 2 && strip_waves(h) * (1 + gdot_n) <= part_capacity()));
        r.dots_done = rhs_norm && gdot_n > 0;
        // ghosts of the newest stage vector (earlier ones done): exchanged behind the interior rows of the RHS (op_rhs)
        if ((rc = op_rhs(h, h->u, i, r.b, &cmb, rhs_norm, i > 0 ? h->Y + (int64_t)(i - 1) * vs : nullptr, r.dots_done ? gdot_n : 0,
                         r.dots_done ? h->bstore + (int64_t)gdot_j0 * vs : nullptr))) return rc;
        if (rhs_norm) r.bnorm2 = h->hres[0];
        if (r.dots_done) for (int j = 0; j < gdot_n; j++) r.dot[j] = h->hres[1 + j];
        return KSFD_OK;
    }
    const double *zin = h->u;
    if (i > 0) {
        const double *xs[5]; double a[5]; int nt = 0;
        xs[nt] = h->u; a[nt++] = 1.0;
        for (int j = 0; j < i; j++) if (h->At[i][j] != 0.0) { xs[nt] = h->Y + (int64_t)j * vs; a[nt++] = h->At[i][j]; }
        if (nt > 1) {
            if ((rc = op_lincomb(h, nt, xs, a, h->Z))) return rc;
            if ((rc = halo(h, h->Z))) return rc;
            zin = h->Z;
        }
    }
    if ((rc = op_rhs(h, zin, i, h->bvec))) return rc;
    if (i > 0) {
        const double *xs[5]; double a[5]; int nt = 0;
        xs[nt] = h->bvec; a[nt++] = 1.0;
        for (int j = 0; j < i; j++) if (h->Ginv[i][j] != 0.0) { xs[nt] = h->Y + (int64_t)j * vs; a[nt++] = -h->Ginv[i][j] / p.hh; }
        if (nt > 1 && (rc = op_lincomb(h, nt, xs, a, h->bvec))) return rc;
    }
    return KSFD_OK;
}

// Row and column i of the Gram matrix gb of the attempt's right-hand sides, from the RHS epilogue or one multi-dot, and the guess built on it.
static int stage_gram_guess(ksfd_handle *h, int i, StageRhs &r, double gb[4][4], SpecGuess &sg)
{
    int rc;
    const int64_t vs = h->vlen;
    if (i == 0) {
        if (r.bnorm2 < 0.0) { if ((rc = op_multidot(h, r.b, r.b, 0))) return rc; r.bnorm2 = h->hres[0]; }
        gb[0][0] = r.bnorm2;
        return KSFD_OK;
    }
    // <b_i, b_j> (j0 <= j < i) and <b_i, b_i> in one pass.
    // j0 > 0 (env_knobs().guess_max): only the most recent stages enter -- every vector of the guess costs two more full-vector
    // reads in the first sweep (b_j in the forward row kernel, Y_j in the inverse one) and one in this multi-dot
    const int j0 = std::max(0, i - env_knobs().guess_max), ng = i - j0;
    if (r.dots_done) {
        for (int j = 0; j < ng; j++) gb[i][j0 + j] = gb[j0 + j][i] = r.dot[j];
        gb[i][i] = r.bnorm2;
    } else {
        if ((rc = op_multidot(h, r.b, h->bstore + (int64_t)j0 * vs, ng))) return rc;
        for (int j = 0; j < ng; j++) gb[i][j0 + j] = gb[j0 + j][i] = h->hres[j];
        gb[i][i] = r.bnorm2 = h->hres[ng];
    }
    double cf[3];
    if (ksfd_ctl::stage_guess(gb, i, j0, ng, cf))
        for (int j = 0; j < ng; j++) if (cf[j] != 0.0) { sg.Y[sg.n] = h->Y + (int64_t)(j0 + j) * vs; sg.b[sg.n] = h->bstore + (int64_t)(j0 + j) * vs; sg.c[sg.n++] = cf[j]; }
    return KSFD_OK;
}

// Solves stage system i for Y_i.  spec_failed: the spectral solver has failed a stage of this attempt (pc_type 2).
static int stage_solve(ksfd_handle *h, const ksfd_step_opts *opts, const AttemptPlan &p, int i, const StageRhs &r, const SpecGuess &sg,
                       bool &spec_failed, ksfd_step_stats &st)
{
    int rc;
    const double shift = p.shift;
    double *xi = h->Y + (int64_t)i * h->vlen;
    LinStats ls;
    if (p.direct) {
        rc = p.banded ? banded_stage(h, shift, r.b, xi, opts, &ls) : direct_stage(h, shift, r.b, xi, opts, &ls);
        st.pc_used |= p.banded ? 32 : 16;
    } else if (p.use_spec) {
        // defect correction with M^-1 (no Krylov vectors), flexible GMRES for the rest if it contracts slowly; the attempt
        // is capped so that a state it does not suit costs little, then the V cycle / plain GMRES takes over
        // (automatic choice: once a stage of this step has failed, the remaining stages go straight to the fallback, and a
        //  re-trial after a back-off period gets a short leash -- a state the preconditioner does not suit then costs one
        //  cheap attempt instead of four expensive ones: 440 -> 176 ms for such a step at 4096^2 x 3 fields)
        const bool skip = spec_failed && opts->pc_type == 2;
        if (!skip) {
            rc = spec_solve(h, shift, r.b, xi, opts, &ls, r.bnorm2, ksfd_ctl::spec_gmres_cap(opts->pc_type, h->memo.spec_backoff), sg.n ? &sg : nullptr);
            st.pc_used |= 8;
        }
        if (skip || (rc == KSFD_ELINEAR && opts->pc_type == 2)) {
            if (!skip) st.linear_its += ls.its;
            spec_failed = true;
            const bool mg_here = ksfd_ctl::spec_fallback_mg(h->mg_ok, p.stiff);
            rc = gmres(h, h->u, shift, r.b, xi, opts, &ls, mg_here ? 1 : 0);
            st.pc_used |= mg_here ? 2 : 1;
        }
    } else if (p.use_pc && sg.n) {
        // multigrid regime, same initial guess: x0 = sum c_j Y_j, TRUE residual r0 = b - A x0 (one Jacobian action), then the
        // correction A d = r0 to the tolerance of the original system and x = x0 + d
        const double *xs[3]; double a[3];
        for (int j = 0; j < sg.n; j++) { xs[j] = sg.Y[j]; a[j] = sg.c[j]; }
        if ((rc = op_lincomb(h, sg.n, xs, a, xi)) || (rc = halo(h, xi)) || (rc = op_jvp_frozen(h, xi, 2, shift, h->Z, r.b))) return rc;
        const double tol = std::max(opts->ksp_rtol * sqrt(r.bnorm2), opts->ksp_atol);
        rc = p.dr_on ? gmres_dr(h, h->u, shift, h->Z, h->t3, opts, &ls, 1, i, tol)
                     : gmres(h, h->u, shift, h->Z, h->t3, opts, &ls, 1, i, tol);        // stage index: the Krylov spaces of the earlier stages are projected out first
        if (!rc) { const double *x2[2] = { xi, h->t3 }; double a2[2] = { 1.0, 1.0 }; rc = op_lincomb(h, 2, x2, a2, xi); }
        st.pc_used |= 2;
    } else {
        const int pc = p.use_pc ? 1 : (p.use_poly ? 2 : 0);
        rc = p.use_async ? gmres_async(h, shift, r.b, xi, opts, &ls)
             : p.dr_on ? gmres_dr(h, h->u, shift, r.b, xi, opts, &ls, pc, i)
                       : gmres(h, h->u, shift, r.b, xi, opts, &ls, pc, i);
        st.pc_used |= p.use_pc ? 2 : (p.use_poly ? 4 : 1);
    }
    st.linear_its += ls.its;
    st.ksp_resid = ls.rel;
    {
        const bool stage_trace = env_knobs().stage_trace;          // iterations per stage system (diagnostics)
        if (stage_trace) fprintf(stderr, "[stage %d] its %d rel %.2e guess %d\n", i, ls.its, ls.rel, sg.n);
    }
    if (rc == KSFD_ELINEAR && !p.direct && !p.use_pc && h->mg_ok && h->tune.use_frozen && opts->pc_type) {
        // unpreconditioned GMRES ran out of iterations: the multigrid-preconditioned solve of the same system
        // is the remedy (the stiffness estimate only knows the diffusion part of J)
        rc = gmres(h, h->u, shift, r.b, xi, opts, &ls, 1);
        st.pc_used |= 2;
        st.linear_its += ls.its;
        st.ksp_resid = ls.rel;
    }
    return rc;
}

// The four stages of one attempt: Y_0..Y_3 from the state in h->u.  A failed stage ends the attempt with its code.
static int step_attempt(ksfd_handle *h, const ksfd_step_opts *opts, const AttemptPlan &p, bool &spec_failed, ksfd_step_stats &st)
{
    int rc = KSFD_OK;
    double gb[4][4];
    // direct: the factors of shift*I - J(u_n) serve the four stages of this attempt (the coefficient planes are those of u_n here
    // also with use_frozen off: ensure_coef)
    if (p.direct && !(rc = ensure_coef(h, true))) rc = p.banded ? banded_factor(h, p.shift) : direct_factor(h, p.shift);
    for (int i = 0; i < 4 && !rc; i++) {
        StageRhs r;
        SpecGuess sg;
        sg.n = 0;
        if ((rc = stage_rhs(h, p, i, r))) break;
        if (p.guess_on && (rc = stage_gram_guess(h, i, r, gb, sg))) break;
        rc = stage_solve(h, opts, p, i, r, sg, spec_failed, st);
    }
    return rc;
}

// The embedded error vector of the last completed attempt into h->errv, if the completion left it in the stage vectors.  Nothing
// outside a step attempt writes the owned points of Y (halo exchanges fill ghost rows only); the next attempt's first stage solve does.
static int err_materialize(ksfd_handle *h)
{
    if (!h->cur.err_pending) return KSFD_OK;
    {
        Scope sc(h, KC_FINISH, vbytes(h, 5));
        hipLaunchKernelGGL(k_rosw_error, vgrid(h), dim3(KSFD_BLOCK), 0, h->st, h->kv, (const double *)h->Y, h->vlen, h->b2t[0] - h->bt[0],
                           h->b2t[1] - h->bt[1], h->b2t[2] - h->bt[2], h->b2t[3] - h->bt[3], h->errv);
    }
    HIPCHK(h, hipGetLastError());
    ksfd_ctl::error_vector_formed(h->cur);
    return KSFD_OK;
}

// completion + embedded error norm.  The new state goes to h->usave: h->u is as it was until the caller accepts (step_run swaps).
// *below: owned values of the new state under their floor (exact: a count carried in doubles; summed over the ranks of a ring)
static int step_finish(ksfd_handle *h, const ksfd_step_opts *opts, double *wrms, double *below)
{
    int rc;
    {
        Scope sc(h, KC_FINISH, vbytes(h, h->tune.old_boundary ? 7 : 6));
        hipLaunchKernelGGL(k_rosw_finish, dim3(h->nblk_vec), dim3(KSFD_BLOCK), 0, h->st, h->kv, (const double *)h->u, h->usave, h->Y, h->vlen,
                           h->bt[0], h->bt[1], h->bt[2], h->bt[3], h->b2t[0] - h->bt[0], h->b2t[1] - h->bt[1],
                           h->b2t[2] - h->bt[2], h->b2t[3] - h->bt[3], opts->atol, opts->rtol, h->P.rhomin, h->P.Umin,
                           h->tune.old_boundary ? h->errv : (double *)nullptr, h->part);
    }
    ksfd_ctl::completion_done(h->cur, h->tune.old_boundary);
    if ((rc = reduce_rows(h, 2, h->nblk_vec, 0))) return rc;
    const double ntot = (double)h->G.F * (double)h->cfg.n[0] * (double)h->cfg.n[1] * (double)h->cfg.n[2];
    *wrms = sqrt(h->hres[0] / ntot);
    *below = h->hres[1];
    return KSFD_OK;
}
