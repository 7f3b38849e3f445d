// libksfd_hip.so -- Chebyshev polynomial preconditioner, flexible/recycled GMRES(m), pipelined GMRES
// (part of the single translation unit ksfd_hip.hip; included from there in this order:
//  handle.hip.h, ops.hip.h, spectral_host.hip.h, mg_host.hip.h, krylov.hip.h, krylov_dr.hip.h, lu_host.hip.h, banded_host.hip.h,
//  step.hip.h)
#pragma once
#include "krylov_small.h"
// ------------------------------------------------------------------------------------------------
// Polynomial preconditioner.  In the non-stiff regime (h*gamma*lambda_max(J) of order 1..10, the regime of the
// headline benchmark) plain GMRES needs ~7 iterations per stage and spends most of its time in Gram-Schmidt, whose
// traffic grows with the square of the iteration count.  z = p(A) v with p the degree-d Chebyshev approximation of
// 1/lambda on [a, b] (spectrum of A/shift: a ~ 1, b = 1 + lambda_max(-J)/shift) costs d Jacobian actions with a fused
// Horner epilogue (out = alpha*v + beta*A t, no extra pass) and cuts the outer iterations to 2-3: same number of
// Jacobian actions, a fraction of the Gram-Schmidt passes.  Used through flexible GMRES (Z basis kept), so the
// solution update needs no extra preconditioner application.
// ------------------------------------------------------------------------------------------------
static int est_lambda_max(ksfd_handle *h, double shift, int nits)
{
    int rc;
    if (!h->pvec) {
        if (alloc_d(h, &h->pvec, h->vlen)) return KSFD_ENOMEM;
        const int nb = blocks_for(h->vlen);
        hipLaunchKernelGGL(k_hash_fill, dim3(nb), dim3(KSFD_BLOCK), 0, h->st, (long long)h->vlen, h->pvec);
        if ((rc = op_multidot(h, h->pvec, h->pvec, 0))) return rc;
        const double n0 = sqrt(h->hres[0]);
        const double *xs[1] = { h->pvec }; double a[1] = { 1.0 / n0 };
        if ((rc = op_lincomb(h, 1, xs, a, h->pvec))) return rc;
    }
    double lamA = 0.0;
    for (int it = 0; it < nits; it++) {
        if ((rc = op_jvp_frozen_halo(h, h->pvec, 1, shift, h->t3))) return rc;
        if ((rc = op_multidot(h, h->t3, h->t3, 0))) return rc;
        lamA = sqrt(h->hres[0]);
        if (!(lamA > 0.0) || lamA != lamA) return fail(h, KSFD_ENAN, "power iteration on the Jacobian broke down");
        const double *xs[1] = { h->t3 }; double a[1] = { 1.0 / lamA };
        if ((rc = op_lincomb(h, 1, xs, a, h->pvec))) return rc;
    }
    const double est = lamA - shift;
    h->memo.lamJ = est > 0.0 ? est : 0.0;
    return KSFD_OK;
}

// coefficients of p for this shift (ksfd_krylov::cheb_setup); degree 0 = "do not precondition"
static void poly_setup(ksfd_handle *h, double shift)
{
    ksfd_ctl::poly_set_up(h->cur, shift);
    h->poly_deg = ksfd_krylov::cheb_setup(h->memo.lamJ, shift, h->poly_target, h->poly_max_deg, h->poly_alpha);
}

// z = sum_i alpha_i (A/shift)^i v  by Horner, one fused Jacobian action per degree
static int poly_apply(ksfd_handle *h, double shift, double *v, double *z)
{
    int rc;
    const int d = h->poly_deg;
    const double *al = h->poly_alpha;
    if ((rc = ensure_coef32(h))) return rc;                  // first application since the planes were made: the fp32 copy is formed here
    if (coef32_on(h) && fused_ok(h)) {
        // mixed precision: the Horner temporaries and the coefficient planes live in fp32 (half the traffic of every
        // application but the arithmetic stays fp64); v is read and z written in fp64.  p(A) becomes a slightly
        // different fixed linear operator, which flexible GMRES does not care about: w_j = A z_j is computed in fp64
        // from the stored z_j, so the Arnoldi relation and the solution keep full accuracy.
        const float *C = h->coef32;
        float *tf[2] = { reinterpret_cast<float *>(h->t1), reinterpret_cast<float *>(h->t2) };
        const double *nod = nullptr;
        if (d == 1) return jvp2d_halo_t<float, double, double, double>(h, C, v, 4, shift, z, nod, al[0], al[1] / shift);
        if ((rc = jvp2d_halo_t<float, double, double, float>(h, C, v, 4, shift, tf[0], nod, al[d - 1], al[d] / shift))) return rc;
        int cur32 = 0;
        for (int i = d - 2; i >= 1; i--) {
            if ((rc = jvp2d_halo_t<float, float, double, float>(h, C, tf[cur32], 3, shift, tf[cur32 ^ 1], (const double *)v, al[i], 1.0 / shift))) return rc;
            cur32 ^= 1;
        }
        return jvp2d_halo_t<float, float, double, double>(h, C, tf[cur32], 3, shift, z, (const double *)v, al[0], 1.0 / shift);
    }
    double *tmp[2] = { h->t1, h->t2 };
    // t_{d-1} = alpha_{d-1} v + (alpha_d/shift) A v
    double *cur = (d == 1) ? z : tmp[0];
    if ((rc = op_jvp_frozen_halo(h, v, 4, shift, cur, nullptr, al[d - 1], al[d] / shift))) return rc;
    int flip = 1;
    for (int i = d - 2; i >= 0; i--) {
        double *nxt = (i == 0) ? z : tmp[flip];
        if ((rc = op_jvp_frozen_halo(h, cur, 3, shift, nxt, v, al[i], 1.0 / shift))) return rc;
        cur = nxt;
        flip ^= 1;
    }
    return KSFD_OK;
}

// ------------------------------------------------------------------------------------------------
// matrix-free GMRES(m) for (shift I - J(u)) x = b, x0 = 0  -- replaces -ksp_type preonly -pc_type lu
// (options84:58-60).  Classical Gram-Schmidt applied twice (CGS2), one fused multi-dot + one fused
// update kernel per pass; the new vector's norm comes from the second pass by Pythagoras.
// The small host algebra (Hessenberg QR, algebraic second projection, recycling and cycle-length rules) is in krylov_small.h.
// ------------------------------------------------------------------------------------------------
struct LinStats { int its; double rel; };

// A right-hand side of norm bn with nothing to iterate on: zero (x = 0 is the solution) or not finite (nan_msg: the solver's own error
// text).  *empty: the solver returns what this returns.
static int rhs_empty(ksfd_handle *h, double bn, double *x, const char *nan_msg, bool *empty)
{
    *empty = !(bn > 0.0);
    if (!*empty) return KSFD_OK;
    if (bn != bn) return fail(h, KSFD_ENAN, "%s", nan_msg);
    HIPCHK(h, hipMemsetAsync(x, 0, sizeof(double) * (size_t)h->vlen, h->st));
    return KSFD_OK;
}

// w = A M^-1 v_j.  z != NULL: where M^-1 v_j lands (pcmode 1 one multigrid V cycle for shift_pc, 2 Chebyshev polynomial p(A), 3 spectral);
// NULL: no preconditioner.
static int apply_AMinv(ksfd_handle *h, const double *ustate, double shift, double shift_pc, int pcmode, double *vj, double *z, double *w)
{
    int rc;
    if (z) {
        if ((rc = pcmode == 1 ? mg_precond(h, shift_pc, vj, z) : pcmode == 3 ? spec_apply(h, shift, vj, z) : poly_apply(h, shift, vj, z))) return rc;
        return op_jvp_frozen_halo(h, z, 1, shift, w);
    }
    if (h->tune.use_frozen) return op_jvp_frozen_halo(h, vj, 1, shift, w);
    return (rc = halo(h, vj)) ? rc : op_jvp(h, ustate, vj, 1, shift, w);
}

// Second Gram-Schmidt pass of w (already projected once with hcol) against V_0..k-1: measure what is left, add it to hcol, project it
// out and normalise; *hn = the norm, from the pass's own <w,w> by Pythagoras.
static int cgs2_second_pass(ksfd_handle *h, double *w, const double *V, int k, double *hcol, double *d, double *hn)
{
    int rc;
    if ((rc = op_multidot(h, w, V, k))) return rc;
    double s2 = 0.0;
    for (int i = 0; i < k; i++) { d[i] = h->hres[i]; hcol[i] += d[i]; s2 += d[i] * d[i]; }
    double hn2 = h->hres[k] - s2;          // ||w''||^2 by Pythagoras; d is O(eps) so this is accurate
    if (hn2 < 0.0) hn2 = 0.0;
    *hn = sqrt(hn2);
    return op_gs_update(h, w, V, k, d, *hn > 0.0 ? 1.0 / *hn : 0.0);
}

// classic CGS2: two Gram-Schmidt passes, each = one fused multi-dot + one fused update.
// (One pass alone loses orthogonality like eps*(||r0||/||r_j||)^2 and stalls near 1e-8.)
// The caller has run the first multi-dot, op_multidot(h, w, V, k), and looked at <w,w>: its result is taken from h->hres.
static int cgs2_classic(ksfd_handle *h, double *w, const double *V, int k, double *hcol, double *d, double *hn)
{
    int rc;
    for (int i = 0; i < k; i++) hcol[i] = h->hres[i];
    if ((rc = op_gs_update(h, w, V, k, hcol, 1.0))) return rc;
    return cgs2_second_pass(h, w, V, k, hcol, d, hn);
}

// CGS2 of w = A M^-1 v_j against V_0..j with the second projection done algebraically (ksfd_krylov::cgs2_algebraic): one pass over V
// for the dots and the Gram row of v_j (kept in Gm, leading dimension ldg), one fused update.
static int cgs2_gram(ksfd_handle *h, double *w, const double *V, int j, double *Gm, int ldg, double *hcol, double *d, double *hn)
{
    int rc;
    const int k = j + 1;
    if ((rc = op_multidot_gram(h, w, V, k))) return rc;
    for (int i = 0; i < k; i++) { d[i] = h->hres[i]; Gm[(size_t)i * ldg + j] = Gm[(size_t)j * ldg + i] = h->hres[k + i]; }
    const double ww = h->hres[2 * k];
    if (!(ww == ww)) return fail(h, KSFD_ENAN, "GMRES: Krylov vector is not finite");
    double hn2;
    if (ksfd_krylov::cgs2_algebraic(Gm, ldg, k, d, ww, hcol, &hn2)) {
        *hn = sqrt(hn2);
        return op_gs_update(h, w, V, k, hcol, 1.0 / *hn);
    }
    // heavy cancellation (||w|| >> ||w - Vc||): apply c, then measure and project once more
    if ((rc = op_gs_update(h, w, V, k, hcol, 1.0))) return rc;
    return cgs2_second_pass(h, w, V, k, hcol, d, hn);
}

// what the parts of one gmres() call share
struct GmresRun {
    int pcmode, stage;
    bool use_pc, use_poly;      // multigrid, right preconditioning: w = A (M^-1 v_j), x = M^-1 (V y) / flexible GMRES (z_j = M^-1 v_j kept in Zb): 2 Chebyshev polynomial p(A), 3 spectral (spectral_host.hip.h)
    bool rec_on, rec_full;      // ksfd_krylov::recycle_decide
    double shift_pc;
    int vb, zb;                 // first slot of this solve's own vectors in V / Zb (behind the kept ones)
    double *V, *Zq;             // ... and the vectors themselves
    std::vector<int> spaces;    // earlier stages whose kept space this solve projects on
    std::vector<double> g_first;    // <b, V_i> over the first of them and <b,b>
    double bn, beta;            // ||b||, norm of the residual of the current x
    const double *rsrc;         // that residual, while it is at hand (first cycle)
    bool x_set = false;         // x holds an iterate (else it is taken as 0 and overwritten)
    // x0 from the recycled spaces is not written on its own: its coefficients wait (indexed by absolute slot of Zb / V) and
    // ride in the solution update of the first cycle -- one pass over x instead of two
    bool x0_pending = false;
    std::vector<double> xcoef;
};

// ||b||: with a recycled space to project on, the projection's multi-dot of b returns <b,b> as well -- one pass, one
// reduction and one host round trip less per stage
static int rhs_norm(ksfd_handle *h, GmresRun &R, const double *b)
{
    int rc;
    if (R.rec_on && R.stage > 0)
        for (int q = 0; q < R.stage; q++)
            if (ksfd_krylov::recycle_uses(R.stage, q, h->tune.rec_mode, R.rec_full) && h->cur.rec_valid[q] && h->rec[q].pc == R.pcmode) R.spaces.push_back(q);
    if (R.spaces.empty()) {
        if ((rc = op_multidot(h, b, R.V, 0))) return rc;
        R.bn = sqrt(h->hres[0]);
        return KSFD_OK;
    }
    const ksfd_handle::RecSpace &S = h->rec[R.spaces.front()];
    if ((rc = op_multidot(h, b, h->V + (int64_t)S.vb * h->vlen, S.k + 1))) return rc;
    R.g_first.assign(h->hres, h->hres + S.k + 2);
    R.bn = sqrt(R.g_first[S.k + 1]);
    return KSFD_OK;
}

// stage >= 0: Krylov recycling.  The four stage systems of a step share the matrix, and their right-hand sides are
// nearly linear images of one another (b_i = f(u + sum a_ij Y_j) - sum c_ij Y_j/h with f almost linear over a step), so
// the leading Arnoldi vectors of an earlier stage (A Z_s = V_s H_s, kept in place at the front of V / Zb) already span
// most of the new solution: x0 = Z_s y with y = argmin ||V_s^T r - H_s y||, r <- r - V_s H_s y, one space after the
// other, costs ~5 vector passes per kept vector and removes 1-2 of the 3-4 outer iterations of stages 2-4 (each
// (d+1) Jacobian actions + Gram-Schmidt).  The iteration then continues on the true residual with the same stopping
// test, so the result is the same to the solver tolerance.  stage < 0: plain solve from x0 = 0.
static int recycle_project(ksfd_handle *h, GmresRun &R, const double *b, double *x)
{
    if (R.spaces.empty()) return KSFD_OK;
    int rc;
    const int64_t vs = h->vlen;
    const bool defer_x0 = !R.use_pc;
    bool pc_x0_pending = false;
    double *const rbuf = (x == h->t3) ? R.V : h->t3;         // projected residual (a correction solve has its x in t3: this solve's slot 0 then, scaled in place below)
    const int first_space = R.spaces.front(), last_space = R.spaces.back();       // the last one's residual update also returns the norm of the result
    bool have_norm = false;
    for (int q : R.spaces) {
        const ksfd_handle::RecSpace &S = h->rec[q];
        const double *Vs = h->V + (int64_t)S.vb * vs;
        const double *Zs = R.use_poly ? h->Zb + (int64_t)S.zb * vs : Vs;
        std::vector<double> gq_((size_t)S.k + 2), yq_((size_t)S.k + 1), Hy_((size_t)S.k + 2), neg_((size_t)S.k + 2);
        double *gq = gq_.data(), *yq = yq_.data(), *Hy = Hy_.data(), *neg = neg_.data();
        if (q == first_space && R.rsrc == b) {
            for (int i = 0; i <= S.k; i++) gq[i] = R.g_first[i];                 // already computed together with ||b||
        } else {
            if ((rc = op_multidot(h, R.rsrc, Vs, S.k + 1))) return rc;
            for (int i = 0; i <= S.k; i++) gq[i] = h->hres[i];
        }
        ksfd_krylov::hess_lsq(S.H.data(), S.k, gq, yq, Hy);
        if (R.use_pc) {
            // x0 = M^-1 (sum over the spaces of V_s y_s): the combinations gather in t2, one V cycle behind the loop
            if ((rc = op_basis_axpy(h, h->t2, Vs, S.k, yq, pc_x0_pending ? 1.0 : 0.0))) return rc;
            pc_x0_pending = true;
        } else if (defer_x0) {
            for (int i = 0; i < S.k; i++) R.xcoef[(R.use_poly ? S.zb : S.vb) + i] += yq[i];
            R.x0_pending = true;
        } else {
            if ((rc = op_basis_axpy(h, x, Zs, S.k, yq, R.x_set ? 1.0 : 0.0))) return rc;
            R.x_set = true;
        }
        for (int i = 0; i <= S.k; i++) neg[i] = -Hy[i];
        if (R.rsrc == b && S.k + 2 <= 6) {
            const double *xs[6] = { b }; double a[6] = { 1.0 };
            for (int i = 0; i <= S.k; i++) { xs[i + 1] = Vs + (int64_t)i * vs; a[i + 1] = neg[i]; }
            if ((rc = op_lincomb(h, S.k + 2, xs, a, rbuf, q == last_space))) return rc;
            R.rsrc = rbuf;
            have_norm = q == last_space;
        } else {
            if (R.rsrc == b) { if ((rc = op_copy(h, rbuf, b))) return rc; R.rsrc = rbuf; }
            const bool nrm = q == last_space;
            if ((rc = op_basis_axpy(h, rbuf, Vs, S.k + 1, neg, 1.0, nrm))) return rc;
            have_norm = nrm;
        }
    }
    if (pc_x0_pending) {
        if ((rc = mg_precond(h, R.shift_pc, h->t2, h->t1)) || (rc = op_copy(h, x, h->t1))) return rc;
        R.x_set = true;
    }
    if (R.x_set || R.x0_pending) {
        if (!have_norm && (rc = op_multidot(h, R.rsrc, R.rsrc, 0))) return rc;
        R.beta = sqrt(h->hres[0]);
        if (!(R.beta == R.beta)) return fail(h, KSFD_ENAN, "GMRES: projected residual is not finite");
    }
    return KSFD_OK;
}

// x += (M^-1) V_j y at the end of a cycle; coefficients of a pending x0 ride along (j = 0: those alone)
static int update_x(ksfd_handle *h, GmresRun &R, double *x, int j, const double *y)
{
    int rc;
    if (R.use_pc) {
        if ((rc = op_basis_axpy(h, h->t2, R.V, j, y, 0.0)) || (rc = mg_precond(h, R.shift_pc, h->t2, h->t1))) return rc;
        if (!R.x_set) { if ((rc = op_copy(h, x, h->t1))) return rc; }
        else { const double *xs[2] = { x, h->t1 }; double a2[2] = { 1.0, 1.0 }; if ((rc = op_lincomb(h, 2, xs, a2, x))) return rc; }
    } else if (R.x0_pending) {
        const int xslot0 = R.use_poly ? R.zb : R.vb;            // first slot of this solve's own vectors in the basis the solution is expanded in
        for (int i = 0; i < j; i++) R.xcoef[xslot0 + i] = y[i];
        if ((rc = op_basis_axpy(h, x, R.use_poly ? h->Zb : h->V, xslot0 + j, R.xcoef.data(), R.x_set ? 1.0 : 0.0))) return rc;
        R.x0_pending = false;
    } else if ((rc = op_basis_axpy(h, x, R.use_poly ? R.Zq : R.V, j, y, R.x_set ? 1.0 : 0.0))) return rc;
    R.x_set = true;
    return KSFD_OK;
}

// keep the leading vectors of this stage's Arnoldi relation (j columns, raw Hessenberg Hraw with leading dimension ld) where they are;
// the next stage builds behind them
static void recycle_keep(ksfd_handle *h, const GmresRun &R, int j, const double *Hraw, int ld)
{
    ksfd_handle::RecSpace &S = h->rec[R.stage];
    S.k = R.rec_full ? j : std::min(j, std::min(h->tune.rec_keep, 4));
    S.vb = R.vb; S.zb = R.zb; S.pc = R.pcmode;
    S.H.assign((size_t)(S.k + 1) * S.k, 0.0);
    for (int c = 0; c < S.k; c++)
        for (int i = 0; i <= S.k; i++) S.H[c * (S.k + 1) + i] = Hraw[(size_t)ld * c + i];
    ksfd_ctl::recycled_space_kept(h->cur, R.stage, R.vb + S.k + 1, R.zb + (R.use_poly ? S.k : 0));
}

// resolve, project on the kept spaces (recycle_project), then per cycle { start vector, per column { w = A M^-1 v_j, orthogonalise,
// push the column }, solve, update x, keep }, restart growth, verdict
static int gmres(ksfd_handle *h, const double *ustate, double shift, const double *b, double *x,
                 const ksfd_step_opts *o, LinStats *ls, int pcmode, int stage = -1, double tol_abs = -1.0)
{
    // tol_abs > 0: stop at that absolute residual norm (the caller solves a correction equation A d = b - A x0 and wants the
    // tolerance of the original system)
    GmresRun R;
    R.pcmode = pcmode; R.stage = stage;
    R.use_pc = pcmode == 1;
    // the hierarchy may be built for a LARGER shift than the system's (h->memo.mg_shift_floor): when 1/(gamma h) falls below the growth
    // rate of the chemotactic instability, shift*I - J is indefinite and a V cycle of it is no contraction; the V cycle of the
    // positively shifted operator still is, and GMRES (true residual of the real system) takes care of the difference
    R.shift_pc = std::max(shift, h->memo.mg_shift_floor);
    R.use_poly = pcmode == 2 || pcmode == 3;
    const int m_opt = std::min(o->ksp_restart > 0 ? o->ksp_restart : 30, h->restart_alloc);
    const int maxit = o->ksp_max_it > 0 ? o->ksp_max_it : 2000;
    const int64_t vs = h->vlen;
    const ksfd_krylov::RecycleChoice rcy = ksfd_krylov::recycle_decide(pcmode, stage, h->tune.rec_mode, h->tune.rec_mg, h->tune.use_frozen, h->restart_alloc, h->cur.rec_vtop);
    // this solve builds in V: a relation kept by the deflated solver (krylov_dr.hip.h) is gone, the recycled spaces unless it builds behind them
    ksfd_ctl::krylov_basis_overwritten(h->cur, !rcy.reset);
    R.rec_on = rcy.rec_on; R.rec_full = rcy.rec_full;
    R.vb = R.rec_on ? h->cur.rec_vtop : 0; R.zb = R.rec_on ? h->cur.rec_ztop : 0;
    // restart length: ksfd_krylov::cycle_first / cycle_next.  Host arrays are sized for the longest cycle.
    const int m = ksfd_krylov::cycle_room(h->restart_alloc, R.vb);
    int m_cur = ksfd_krylov::cycle_first(m_opt, m, R.rec_on, R.rec_full);
    double *const V = R.V = h->V + (int64_t)R.vb * vs;
    R.Zq = R.use_poly ? h->Zb + (int64_t)R.zb * vs : nullptr;
    R.xcoef.assign((size_t)std::max(h->restart_alloc + 2, KSFD_MAXDOT), 0.0);
    int rc;
    ksfd_krylov::HessQR qr(m);
    std::vector<double> hcol(m + 2), d(m + 2), Gm((size_t)(m + 1) * (m + 1), 0.0);
    if ((rc = rhs_norm(h, R, b))) return rc;
    const double bn = R.bn;
    ls->its = 0; ls->rel = 0.0;
    bool empty;
    if ((rc = rhs_empty(h, bn, x, "GMRES: right-hand side is not finite", &empty)) || empty) return rc;
    const double tol = tol_abs > 0.0 ? tol_abs : std::max(o->ksp_rtol * bn, o->ksp_atol);
    R.beta = bn; R.rsrc = b;
    if ((rc = recycle_project(h, R, b, x))) return rc;
    double rn = R.beta;
    int total = 0;
    bool first = true;          // the residual of the current x is at hand (rsrc, norm beta): no A x needed
    bool restarted = false;
    while (true) {
        if (first && R.beta <= tol) {                          // the recycled spaces already hold the solution
            if (R.x0_pending && (rc = update_x(h, R, x, 0, nullptr))) return rc;
            break;
        }
        // V0 = r / beta
        if (first) { const double *xs[1] = { R.rsrc }; double a[1] = { 1.0 / R.beta }; if ((rc = op_lincomb(h, 1, xs, a, V))) return rc; }
        else {
            if ((rc = halo(h, x)) || (rc = h->tune.use_frozen ? op_jvp_frozen(h, x, 1, shift, V) : op_jvp(h, ustate, x, 1, shift, V))) return rc;     // V0 = A x
            const double *xs[2] = { b, V }; double a[2] = { 1.0, -1.0 };
            if ((rc = op_lincomb(h, 2, xs, a, V))) return rc;                                  // r = b - A x
            if ((rc = op_multidot(h, V, V, 0))) return rc;
            R.beta = rn = sqrt(h->hres[0]);
            if (!(rn == rn)) return fail(h, KSFD_ENAN, "GMRES: residual is not finite");
            if (rn <= tol) break;
            const double *x1[1] = { V }; double a1[1] = { 1.0 / rn };
            if ((rc = op_lincomb(h, 1, x1, a1, V))) return rc;
        }
        qr.reset(R.beta);
        int j = 0;
        bool done = false;
        for (; j < m_cur && total < maxit; j++) {
            double *vj = V + (int64_t)j * vs, *w = V + (int64_t)(j + 1) * vs;
            double *z = R.use_pc ? h->t1 : R.use_poly ? R.Zq + (int64_t)j * vs : nullptr;
            if ((rc = apply_AMinv(h, ustate, shift, R.shift_pc, pcmode, vj, z, w))) return rc;
            const int k = j + 1;
            double hn;
            if (ksfd_krylov::gs_classic(o->reserved, k)) {
                if ((rc = op_multidot(h, w, V, k))) return rc;
                if (!(h->hres[k] == h->hres[k])) return fail(h, KSFD_ENAN, "GMRES: Krylov vector is not finite");
                if ((rc = cgs2_classic(h, w, V, k, hcol.data(), d.data(), &hn))) return rc;
            } else if ((rc = cgs2_gram(h, w, V, j, Gm.data(), m + 1, hcol.data(), d.data(), &hn))) return rc;
            hcol[k] = hn;
            rn = qr.push_column(j, hcol.data());
            total++;
            if (rn <= tol || hcol[k] == 0.0) { j++; done = true; break; }
        }
        qr.solve(j);
        if ((rc = update_x(h, R, x, j, qr.y.data()))) return rc;
        if (R.rec_on && first && !restarted && done && j >= 1) recycle_keep(h, R, j, qr.Hraw.data(), qr.ld);
        if (!first) restarted = true;
        first = false;
        if (done || total >= maxit) break;
        restarted = true;
        m_cur = ksfd_krylov::cycle_next(m_cur, m, h->tune.restart_grow);
    }
    if (!R.x_set) HIPCHK(h, hipMemsetAsync(x, 0, sizeof(double) * (size_t)vs, h->st));
    ls->its = total;
    ls->rel = ksfd_krylov::rel_of(rn, bn, tol_abs, o->ksp_rtol);
    if (rn > tol) return fail(h, KSFD_ELINEAR, "GMRES did not converge: %d iterations, relative residual %.3e (tol %.3e)", total, rn / bn, tol / bn);
    return KSFD_OK;
}

// ------------------------------------------------------------------------------------------------
// Stage solve with the spectral preconditioner.  M = shift*I - J0 is so close to A = shift*I - J on near-uniform states
// (||I - A M^-1|| ~ 0.01: tests/experiments/fft_pc_experiment.py) that plain defect correction
//      x <- x + M^-1 (b - A x)
// converges as fast as GMRES would (3-4 iterations to 1e-6) and needs NO Krylov vectors: an iteration is one spectral
// application (its last kernel adds into x) and one Jacobian action in residual mode whose store epilogue also leaves
// ||r||^2 -- no BLAS-1 pass at all, where GMRES spends ~40 % of such a step in Gram-Schmidt.  Stops on the TRUE residual,
// ||b - A x|| <= max(ksp_rtol ||b||, ksp_atol), like every other solver here.  If the contraction is worse than 0.25 per
// sweep (coefficients vary too much for the constant-coefficient inverse), the remaining correction A d = r is handed to
// flexible GMRES with the same preconditioner, and if that fails too the caller falls back to the V cycle.
// bnorm2 >= 0: ||b||^2 if the caller already has it (RHS kernel epilogue), else it is computed here.
// ------------------------------------------------------------------------------------------------
// residual of the iterate a spectral application left in x: r32 (fp32, fused: the strip kernel whose store epilogue also leaves the norm)
// or r (fp64); ||r||^2 -> hres[0]
static int spec_residual(ksfd_handle *h, bool fused, double *x, double shift, const double *b, double *r, float *r32)
{
    int rc;
    // the spectral application wrote owned rows only; the 2-D fused residual exchanges the ghost rows itself, behind its interior rows
    if (h->ring && !(fused && h->G.dim == 2) && (rc = halo(h, x))) return rc;
    if (fused) return op_residual32(h, x, shift, b, r32);
    return (rc = op_jvp_frozen(h, x, 2, shift, r, b)) ? rc : op_multidot(h, r, r, 0);
}

// guess != NULL: the first sweep starts from x0 = sum_j c_j Y_j (earlier stage solutions of the same step, A Y_j = b_j):
//   x = x0 + M^-1 (b - sum_j c_j b_j)   -- no extra Jacobian action, the vectors ride in the row kernels of the application
static int spec_solve(ksfd_handle *h, double shift, const double *b, double *x, const ksfd_step_opts *o, LinStats *ls, double bnorm2, int gmres_cap,
                      const SpecGuess *guess = nullptr)
{
    int rc;
    ls->its = 0; ls->rel = 0.0;
    ksfd_ctl::recycled_spaces_dropped(h->cur);
    if (bnorm2 < 0.0) {
        if ((rc = op_multidot(h, b, b, 0))) return rc;
        bnorm2 = h->hres[0];
    }
    const double bn = sqrt(bnorm2);
    bool empty;
    if ((rc = rhs_empty(h, bn, x, "spectral solve: right-hand side is not finite", &empty)) || empty) return rc;
    const double tol = std::max(o->ksp_rtol * bn, o->ksp_atol);
    const int maxit = std::min(o->ksp_max_it > 0 ? o->ksp_max_it : 2000, ksfd_ctl::SPEC_SWEEP_CAP);
    double *r = h->Z;                              // residual (the fused-stage path leaves Z unused)
    float *r32 = reinterpret_cast<float *>(h->Z);  // ... kept in fp32 while only the preconditioner reads it
    double rn = bn, rprev = bn;
    // fp32 residual with the norm from the store epilogue: the 2-D strip kernel, or the 3-D one when its wave count fits the partial buffer
    const bool fused = fused_ok(h) || (strip3d_ok(h) && k3d_waves(h) <= part_capacity());
    // Predicted last sweep.  Every sweep multiplies the residual by (I - A M^-1); the four stage systems of a step share that
    // operator, so its contraction has been MEASURED by the time a solve is about to finish: rho_hat = the largest ratio
    // ||r_k+1|| / ||r_k|| of any sweep (but the first one from zero, see ksfd_ctl::spec_sweep) of this step and the previous one.  When
    // SAFETY * rho_hat * ||r_k|| <= tol the update x += M^-1 r_k is applied and the solve returns WITHOUT evaluating the residual of the
    // result (a Jacobian action, 40 % of a sweep, whose only purpose would be to confirm a number 1-2 decades below the tolerance).  Every
    // other residual is the true fp64 one, as before.  Off for tight tolerances (ksp_rtol < 1e-8: the parity tests verify every solve),
    // with opts.reserved bit 3, and with KSFD_SPEC_VERIFY=1, which also evaluates and reports the residual the prediction stood in for.
    const int verify_env = env_knobs().spec_verify;
    const bool predict = ksfd_ctl::spec_predict_on(h->tune.spec_predict, o->reserved, o->ksp_rtol, verify_env);
    bool final_sweep = false, slow = false;
    for (int k = 0; k < maxit && !slow; k++) {
        if (k == 0) rc = spec_apply(h, shift, b, x, nullptr, nullptr, guess);
        else rc = fused ? spec_apply(h, shift, nullptr, x, x, r32) : spec_apply(h, shift, r, x, x);
        if (rc) return rc;
        ls->its++;
        if (final_sweep) {
            ls->rel = ksfd_ctl::spec_pred_bound(h->memo, rn, bn);                  // the bound the decision was made on
            h->n_predicted++;
            if (verify_env == 1) {
                if ((rc = spec_residual(h, fused, x, shift, b, r, r32))) return rc;
                const double rv = sqrt(h->hres[0]);
                fprintf(stderr, "[spec] predicted final sweep %d: bound %.3e true %.3e tol %.3e%s\n", k, ls->rel, rv / bn, tol / bn, rv <= tol ? "" : "  <-- ABOVE TOLERANCE");
                if (!(rv <= tol)) return fail(h, KSFD_ELINEAR, "predicted final sweep missed the tolerance: true %.3e, bound %.3e, tol %.3e", rv / bn, ls->rel, tol / bn);
            }
            return KSFD_OK;
        }
        if ((rc = spec_residual(h, fused, x, shift, b, r, r32))) return rc;
        h->n_residual++;
        rn = sqrt(h->hres[0]);
        {
            if (env_knobs().spec_trace) fprintf(stderr, "[spec] sweep %d rel %.3e%s\n", k, rn / bn, (k == 0 && guess) ? " (guess)" : "");
        }
        switch (ksfd_ctl::spec_sweep(k, maxit, rn, rprev, tol, guess != nullptr, predict, h->memo)) {
        case ksfd_ctl::SPEC_NOT_FINITE: return fail(h, KSFD_ENAN, "spectral solve: residual is not finite");
        case ksfd_ctl::SPEC_CONVERGED: ls->rel = rn / bn; return KSFD_OK;
        case ksfd_ctl::SPEC_SLOW: slow = true; break;
        case ksfd_ctl::SPEC_CONTINUE_FINAL: final_sweep = true; rprev = rn; break;
        case ksfd_ctl::SPEC_CONTINUE: rprev = rn; break;
        }
    }
    if (fused && (rc = op_jvp_frozen(h, x, 2, shift, r, b))) return rc;       // the correction solve below wants the residual in fp64
    // slow, or out of sweeps: hand the correction equation A d = r to flexible GMRES with the same preconditioner (absolute tolerance = ours)
    ksfd_step_opts go = *o;
    go.ksp_rtol = 1e-30; go.ksp_atol = tol;
    if (gmres_cap > 0) go.ksp_max_it = gmres_cap;
    const bool restart_from_zero = ksfd_ctl::spec_handover(rn, bn);       // the sweeps made it worse: forget x
    LinStats g2;
    rc = gmres(h, h->u, shift, restart_from_zero ? b : r, h->t3, &go, &g2, 3);
    ls->its += g2.its;
    if (rc) { ls->rel = rn / bn; return rc; }
    if (restart_from_zero) { if ((rc = op_copy(h, x, h->t3))) return rc; }
    else { const double *xs[2] = { x, h->t3 }; double a2[2] = { 1.0, 1.0 }; if ((rc = op_lincomb(h, 2, xs, a2, x))) return rc; }
    ls->rel = ksfd_ctl::spec_handover_rel(g2.rel, restart_from_zero, rn, bn);
    return KSFD_OK;
}

// ------------------------------------------------------------------------------------------------
// Pipelined GMRES: same mathematics as gmres() (CGS2 with the algebraic second projection), but the small
// algebra of every iteration runs in a one-thread kernel on the device (k_gmres_coef) and the fused update reads its
// coefficients from device memory, so an iteration = [J action, multi-dot, reduce(+allreduce), coef, update] with NO
// host round trip.  The host polls the residual estimate one iteration behind (and exactly on time when the
// extrapolated estimate says "this one converges"), so the GPU never idles and at most one iteration is wasted.
// Pays when an iteration is latency-bound: small grids, many slab ranks.  Unpreconditioned, frozen Jacobian only.
// ------------------------------------------------------------------------------------------------
// the device block of the small algebra (h->gm_dev, sized by ksfd_create for restart_alloc columns; handle.hip.h has the layout)
struct GmDev { double *G, *H, *cs, *sn, *g, *coef, *scale, *mon; int ld; };
static GmDev gm_dev_block(const ksfd_handle *h)
{
    GmDev D;
    const int m = h->restart_alloc;
    D.ld = m + 1;
    D.G = h->gm_dev; D.H = D.G + (size_t)D.ld * D.ld; D.cs = D.H + (size_t)D.ld * m; D.sn = D.cs + m;
    D.g = D.sn + m; D.coef = D.g + D.ld; D.scale = D.coef + KSFD_MAXDOT; D.mon = D.scale + 1;
    return D;
}
// small algebra of column j on the device (k_gmres_coef): reads the reduced rows in h->dres
static void launch_gmres_coef(ksfd_handle *h, const GmDev &D, int j, double beta)
{
    hipLaunchKernelGGL(k_gmres_coef, dim3(1), dim3(64), 0, h->st, j, h->restart_alloc, beta, (const double *)h->dres, D.G, D.H, D.cs, D.sn, D.g, D.coef, D.scale, D.mon);
}
// w = (w - sum_{i<k} coef[i] V_i) * (*scale) with coefficients and scale in device memory (k <= KSFD_ASYNC_MAXK)
static void launch_gs_update_dev(ksfd_handle *h, double *w, const double *V, int k, const double *coef, const double *scale)
{
    Scope sc(h, KC_GSUPDATE, vbytes(h, k + 2));
    KB_DISPATCH(k, VW_DISPATCH(h, hipLaunchKernelGGL((k_gs_update_dev<KB, VW>), vgridw(h, VW), dim3(KSFD_BLOCK), 0, h->st, h->kv, w, V, h->vlen, k, coef, scale)));
}

static int gmres_async(ksfd_handle *h, double shift, const double *b, double *x, const ksfd_step_opts *o, LinStats *ls)
{
    ksfd_ctl::recycled_spaces_dropped(h->cur);
    // Cycle length: what the kernels of an iteration hold, whatever the basis has room for.  k_multidot_gram / k_gs_update_dev stop at the
    // top of the KB ladder (32 vectors), k_gmres_coef keeps its coefficients in KSFD_MAXDOT slots: a longer ksp_restart runs as cycles of
    // KSFD_ASYNC_MAXK (gmres() goes on classically and in chunks beyond that length; there is no such path here).
    const int m = ksfd_krylov::async_cycle(o->ksp_restart, h->restart_alloc, KSFD_ASYNC_MAXK);
    const int maxit = o->ksp_max_it > 0 ? o->ksp_max_it : 2000;
    const int64_t vs = h->vlen;
    const int ld = h->restart_alloc + 1;
    double *V = h->V;
    const GmDev D = gm_dev_block(h);
    double *dH = D.H, *dg = D.g, *dmon = D.mon;
    double *hmon = h->gm_host, *hH = hmon + 2 * ld, *hg = hH + (size_t)ld * h->restart_alloc;
    int rc;
    if ((rc = op_multidot(h, b, V, 0))) return rc;
    const double bn = sqrt(h->hres[0]);
    ls->its = 0; ls->rel = 0.0;
    bool empty;
    if ((rc = rhs_empty(h, bn, x, "GMRES: right-hand side is not finite", &empty)) || empty) return rc;
    const double tol = std::max(o->ksp_rtol * bn, o->ksp_atol);
    double beta = bn, rn = bn;
    int total = 0;
    bool first = true;
    std::vector<double> y(m);
    while (true) {
        if (first) { const double *xs[1] = { b }; double a[1] = { 1.0 / beta }; if ((rc = op_lincomb(h, 1, xs, a, V))) return rc; }
        else {
            if ((rc = op_jvp_frozen_halo(h, x, 1, shift, V))) return rc;
            const double *xs[2] = { b, V }; double a[2] = { 1.0, -1.0 };
            if ((rc = op_lincomb(h, 2, xs, a, V))) return rc;
            if ((rc = op_multidot(h, V, V, 0))) return rc;
            beta = sqrt(h->hres[0]);
            rn = beta;
            if (!(beta == beta)) return fail(h, KSFD_ENAN, "GMRES: residual is not finite");
            if (beta <= tol) break;
            const double *x1[1] = { V }; double a1[1] = { 1.0 / beta };
            if ((rc = op_lincomb(h, 1, x1, a1, V))) return rc;
        }
        int jc = -1, jlast = -1, checked = -1;
        double r1 = beta, r2 = -1.0;
        auto poll = [&](int upto) -> int {          // read monitors (checked, upto]; sets jc when converged
            for (int q = checked + 1; q <= upto; q++) {
                if (hipEventSynchronize(h->gm_ev[q]) != hipSuccess) return fail(h, KSFD_EHIP, "event sync failed");
                const double r = hmon[2 * q], hn = hmon[2 * q + 1];
                if (!(r == r)) return fail(h, KSFD_ENAN, "GMRES: Krylov vector is not finite");
                checked = q;
                r2 = r1; r1 = r;
                if (r <= tol || hn == 0.0) { jc = q; return KSFD_OK; }
            }
            return KSFD_OK;
        };
        for (int j = 0; j < m && total + j < maxit; j++) {
            double *vj = V + (int64_t)j * vs, *w = V + (int64_t)(j + 1) * vs;
            const int k = j + 1;
            if ((rc = op_jvp_frozen_halo(h, vj, 1, shift, w))) return rc;
            const int nb = vec2(h) ? (h->nblk_vec + 1) / 2 : h->nblk_vec;
            {
                Scope sc(h, KC_MULTIDOT, vbytes(h, k + 1));
                KB_DISPATCH(k, VW_DISPATCH(h, hipLaunchKernelGGL((k_multidot_gram<KB, VW>), dim3(nb), dim3(KSFD_BLOCK), 0, h->st, h->kv, (const double *)w, (const double *)V, h->vlen, k, h->part)));
            }
            {
                Scope sc(h, KC_REDUCE, 8.0 * (2 * k + 1) * (double)nb);
                hipLaunchKernelGGL(k_reduce_rows, dim3(2 * k + 1), dim3(KSFD_BLOCK), 0, h->st, (const double *)h->part, nb, 0, h->dres);
            }
            if (h->ring && h->tr->allreduce(h->dres, 2 * k + 1, 0, h->st)) return fail(h, KSFD_ECOMM, "allreduce failed: %s", h->tr->error().c_str());
            launch_gmres_coef(h, D, j, beta);
            launch_gs_update_dev(h, w, V, k, D.coef, D.scale);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipMemcpyAsync(hmon + 2 * j, dmon + 2 * j, 2 * sizeof(double), hipMemcpyDeviceToHost, h->st));
            HIPCHK(h, hipEventRecord(h->gm_ev[j], h->st));
            jlast = j;
            if ((rc = poll(j - 1))) return rc;                 // one iteration behind: the GPU already has iteration j queued
            if (jc >= 0) break;
            if (r2 > 0.0 && r1 * (r1 / r2) <= 1.5 * tol) {     // extrapolation says iteration j converges: look now, queue nothing more
                if ((rc = poll(j))) return rc;
                if (jc >= 0) break;
            }
        }
        if (jc < 0 && (rc = poll(jlast))) return rc;
        const int kused = jc >= 0 ? jc + 1 : jlast + 1;
        total += jlast + 1;
        HIPCHK(h, hipMemcpyAsync(hH, dH, sizeof(double) * (size_t)ld * h->restart_alloc, hipMemcpyDeviceToHost, h->st));
        HIPCHK(h, hipMemcpyAsync(hg, dg, sizeof(double) * ld, hipMemcpyDeviceToHost, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));
        ksfd_krylov::hess_backsolve(hH, ld, hg, kused, y.data());
        if ((rc = op_basis_axpy(h, x, V, kused, y.data(), first ? 0.0 : 1.0))) return rc;
        first = false;
        rn = hmon[2 * (kused - 1)];
        if (jc >= 0 || total >= maxit) break;
    }
    ls->its = total;
    ls->rel = rn / bn;
    if (rn > tol) return fail(h, KSFD_ELINEAR, "GMRES did not converge: %d iterations, relative residual %.3e (tol %.3e)", total, rn / bn, tol / bn);
    return KSFD_OK;
}
