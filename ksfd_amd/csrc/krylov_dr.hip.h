// libksfd_hip.so -- GMRES with deflated restarting (GMRES-DR; Morgan, SIAM J. Sci. Comput. 24, 2002), opt-in per handle
// (ksfd_set_deflation).  Part of the single translation unit ksfd_hip.hip, included behind krylov.hip.h.
//
// Restarted GMRES loses most where it needs many iterations: shift*I - J indefinite late in a run, a handful of eigenvalues of J
// above the shift.  Here a restart keeps the k harmonic Ritz vectors of smallest modulus in the basis.  A cycle works on a relation
//      A M^-1 V_n = V_n+1 Hb,   Hb (n + 1) x n.
// With P = orth[ harmonic Ritz vectors | c - Hb y ] (host: dense_small.h) the k + 1 vectors V_n+1 P satisfy a relation of the same
// form with the small DENSE matrix P^T Hb P_k, the residual of the iterate lies in their span, and Arnoldi carries on from vector k.  The basis is rotated
// in place by one pass over V (k_basis_rotate); in flexible mode Zb follows with P_k.  No extra vectors.
// The small least-squares problem is dense (no longer Hessenberg) and is solved by Householder QR on the host in every iteration:
// O(m^3) flops and one small allocation per iteration -- tens of microseconds at the default restart length of 30, next to an iteration
// of several hundred; about a millisecond at ksp_restart = 120, where an updating QR (O(m^2)) would be the thing to build.  The restart
// length is ksp_restart, fixed: no restart growth here.
//
// The four stage systems of a step attempt share the matrix, so the relation kept at the end of one solve is still one for the next
// right-hand side (carry_stages): the new residual is projected on it -- c = V_k+1^T r, y = argmin ||c - Hb y||, x0 = M^-1 V_k y,
// r <- r - V_k+1 Hb y -- which takes the slow modes the kept vectors hold out of it, and the deflated solve starts afresh from what is
// left.  (Running Arnoldi on BEHIND the kept block instead was built first and measured: the remainder of the new residual has to join
// the basis as a second trailing vector, the complement of range(Hb) gains a dimension with every right-hand side, every chain of the
// resulting block Krylov space advances only every e-th column, and stage 3 of case 100 of the indefinite sweep took 3282 iterations
// instead of 163.  dense_small.h still handles such relations.)  The same projection is used when the true residual b - A x, evaluated
// once before a solve returns, is still above the tolerance: the recurrence residual drifts over many deflated restarts, and this
// solver never reports convergence on the recurrence alone.
// Orthogonalisation is classical Gram-Schmidt applied twice, two fused passes each (the variant of gmres() with the algebraic second
// projection needs the Gram matrix of the basis, which a rotation would invalidate).
#pragma once
#include "dense_small.h"

static int gmres_dr(ksfd_handle *h, const double *ustate, double shift, const double *b, double *x,
                    const ksfd_step_opts *o, LinStats *ls, int pcmode, int stage, double tol_abs = -1.0)
{
    using namespace ksfd_dense;
    // Both preconditioned modes run FLEXIBLY here (z_j = M^-1 v_j kept in Zb, x = Z y).  For the polynomial that is what gmres() does
    // too.  For the V cycle it is what makes a verified residual affordable: the cycle is not a linear operator (fp32 level vectors, a
    // coarsest-grid iteration that stops on a tolerance), so x = M^-1 (V y) is not sum_j y_j M^-1 v_j, the recurrence residual of plain right
    // preconditioning misses the true one by more than the tolerance (measured: 107 failed checks in 30 steps of the 384^2 run at
    // ksp_rtol = 1e-6, every one answered with more iterations), and the update costs a V cycle of its own.
    const bool use_flex = pcmode == 1 || pcmode == 2;
    const double shift_pc = std::max(shift, h->memo.mg_shift_floor);
    const int m = std::min(o->ksp_restart > 0 ? o->ksp_restart : 30, h->restart_alloc);
    const int keep = h->dr_keep;
    const int maxit = o->ksp_max_it > 0 ? o->ksp_max_it : 2000;
    const int64_t vs = h->vlen;
    if (use_flex && !h->Zb && alloc_d(h, &h->Zb, (int64_t)h->restart_alloc * h->vlen)) return KSFD_ENOMEM;
    double *V = h->V, *Zq = use_flex ? h->Zb : nullptr;
    ksfd_handle::DrKept &K = h->dr;
    ksfd_deflation_stats &S = h->dr_stats;
    int rc;
    ls->its = 0; ls->rel = 0.0;
    if (keep < 1 || keep > m - 3) return fail(h, KSFD_EINVAL, "deflation: keep = %d needs 1 <= keep <= restart - 3 = %d", keep, m - 3);
    const int ld = m + 1;                                  // rows of Hb
    const int ldp = KSFD_ROT_MAXOUT;
    std::vector<double> Hb((size_t)ld * m, 0.0), c(ld, 0.0), y(m, 0.0), rho(ld, 0.0), hcol(ld + 1, 0.0), dcol(ld + 1, 0.0);
    const int e = 1;                                       // trailing vectors of the relation (dense_small.h handles more; this solver never has them)
    int kk = 0;                                            // the relation in front of the basis: kk columns, kk + 1 vectors
    if (h->cur.dr_valid && h->dr_carry && stage > 0 && stage < 4 && K.pc == pcmode && K.shift == shift && K.shift_pc == shift_pc && K.kk >= 1 && K.kk + 1 <= m) {
        kk = K.kk;
        for (int j = 0; j < kk; j++) for (int i = 0; i < kk + e; i++) Hb[(size_t)j * ld + i] = K.H[(size_t)j * (kk + e) + i];
    }
    ksfd_ctl::krylov_basis_overwritten(h->cur);            // V is about to change; dr_relation_kept where a relation is left behind

    auto true_residual = [&](double *r) -> int {           // r = b - A x
        int q;
        if ((q = halo(h, x))) return q;
        if (h->tune.use_frozen) return op_jvp_frozen(h, x, 2, shift, r, b);
        if ((q = op_jvp(h, ustate, x, 1, shift, r))) return q;
        const double *xs[2] = { b, r }; double a[2] = { 1.0, -1.0 };
        return op_lincomb(h, 2, xs, a, r);
    };
    std::vector<double> ytmp(m, 0.0), rhotmp(ld, 0.0);
    auto lsq = [&](int n, int ee, double *res) -> bool {   // y, rho and ||rho|| of the n-column problem; y and rho are kept on failure
        if (!dense_lsq(n + ee, n, Hb.data(), ld, c.data(), ytmp.data(), rhotmp.data())) return false;
        double s2 = 0.0;
        for (int i = 0; i < n + ee; i++) s2 += rhotmp[i] * rhotmp[i];
        if (!(s2 == s2)) return false;
        std::copy(ytmp.begin(), ytmp.begin() + n, y.begin());
        std::copy(rhotmp.begin(), rhotmp.begin() + n + ee, rho.begin());
        *res = sqrt(s2);
        return true;
    };
    bool x_set = false;
    auto update_x = [&](int n) -> int {                    // x += Z_n y (V_n y without a preconditioner)
        if (n < 1) return KSFD_OK;
        const int q = op_basis_axpy(h, x, use_flex ? Zq : V, n, y.data(), x_set ? 1.0 : 0.0);
        x_set = true;
        return q;
    };

    // ---- the residual of x = 0 is b: its norm, and with a kept space its projection, from one pass
    double *r0 = V + (int64_t)(kk ? kk + e : 0) * vs;
    if ((rc = op_copy(h, r0, b))) return rc;
    if ((rc = op_multidot(h, r0, V, kk ? kk + e : 0))) return rc;
    const double bn = sqrt(h->hres[kk ? kk + e : 0]);
    bool empty;
    if ((rc = rhs_empty(h, bn, x, "GMRES-DR: right-hand side is not finite", &empty)) || empty) return rc;
    const double tol = tol_abs > 0.0 ? tol_abs : std::max(o->ksp_rtol * bn, o->ksp_atol);
    const double rel_den = (tol_abs > 0.0 && o->ksp_rtol > 0.0) ? tol_abs / o->ksp_rtol : bn;
    int total = 0, stagnant = 0;
    double rn = bn, rnorm = bn, prev_fail = -1.0, tol_it = tol;
    bool accepted = false;                                 // the true residual met the tolerance (or missed it by less than its own rounding error)
    // Rounding of the verdict itself.  fl(b - A x) carries an error of about nnz_row * u * || |A| |x| ||, and where ||A|| ||x|| >> ||b||
    // (nearly singular stage matrices) that is of the size of a tight tolerance: a true residual within this allowance of the tolerance
    // cannot be told from one below it in fp64, and passes.  ||A|| is bounded from BELOW by the largest ||A v_j|| seen (unpreconditioned
    // solves only: the columns of Hb; with a preconditioner the allowance is zero), so the allowance errs on the strict side.
    double anorm = 0.0;
    const double nnz_row = (double)h->G.F * (4.0 * h->G.dim + 1.0);
    bool dots_ready = true;                                // hres holds <r0, V_i> (i < kk + e) and <r0, r0>

    while (true) {
        // ---- start of a solve from the residual in slot r0 (= b, or a true residual)
        std::fill(c.begin(), c.end(), 0.0);
        if (kk) {
            // a kept relation A M^-1 V_kk = V_kk+1 Hb: least squares over it gives x0 = M^-1 V_kk y, the residual loses V_kk+1 Hb y
            const int nk = kk + 1;
            if (!dots_ready && (rc = op_multidot(h, r0, V, nk))) return rc;
            for (int i = 0; i < nk; i++) c[i] = h->hres[i];
            if (lsq(kk, 1, &rn)) {
                if ((rc = update_x(kk))) return rc;
                for (int i = 0; i < nk; i++) { double t = 0.0; for (int l = 0; l < kk; l++) t += Hb[(size_t)l * ld + i] * y[l]; hcol[i] = t; }
                if ((rc = op_gs_update(h, r0, V, nk, hcol.data(), 1.0))) return rc;
                S.projections++;
            }
            kk = 0;                                        // the basis is rebuilt from the projected residual; deflation resumes with its first restart
            dots_ready = false;
            std::fill(c.begin(), c.end(), 0.0);
        }
        if (!dots_ready && (rc = op_multidot(h, r0, V, 0))) return rc;
        rnorm = sqrt(h->hres[0]);
        if (!(rnorm == rnorm)) return fail(h, KSFD_ENAN, "GMRES-DR: residual is not finite");
        if (rnorm > 0.0) { const double *xs[1] = { r0 }; double a[1] = { 1.0 / rnorm }; if ((rc = op_lincomb(h, 1, xs, a, V))) return rc; }
        c[0] = rnorm;
        dots_ready = false;
        rn = rnorm;
        bool converged = rnorm <= tol_it, broke = false;   // (the projection may have done it all)
        int n = kk;
        // ---- cycles of this start: Arnoldi behind the kept block, deflated restart, again
        while (true) {
            const int ncols = m;
            if (n > 0) {
                if (!lsq(n, e, &rn)) { broke = true; n = 0; }              // (nothing usable in the kept block: x stays, plain restart)
                converged = !broke && rn <= tol_it;
            }
            while (!converged && !broke && n < ncols && total < maxit) {
                const int j = n, nb = j + e;               // column j: w against the nb vectors in front of it
                double *w = V + (int64_t)nb * vs;
                if ((rc = apply_AMinv(h, ustate, shift, shift_pc, pcmode, V + (int64_t)j * vs, use_flex ? Zq + (int64_t)j * vs : nullptr, w))) return rc;     // w = A M^-1 v_j
                if ((rc = op_multidot(h, w, V, nb))) return rc;
                if (!(h->hres[nb] == h->hres[nb])) return fail(h, KSFD_ENAN, "GMRES-DR: Krylov vector is not finite");
                double hn;
                if ((rc = cgs2_classic(h, w, V, nb, hcol.data(), dcol.data(), &hn))) return rc;
                double *Hc = &Hb[(size_t)j * ld];
                for (int i = 0; i < ld; i++) Hc[i] = i < nb ? hcol[i] : 0.0;
                Hc[nb] = hn;
                if (pcmode == 0) { double cn2 = hn * hn; for (int i = 0; i < nb; i++) cn2 += hcol[i] * hcol[i]; anorm = std::max(anorm, sqrt(cn2)); }
                n = j + 1;
                total++;
                if (!lsq(n, e, &rn)) { broke = true; n = j; break; }       // y still solves the problem without this column
                if (rn <= tol_it) converged = true;
                else if (hn == 0.0) broke = true;          // breakdown without convergence: this space has nothing more to give
            }
            if ((rc = update_x(n))) return rc;
            // what this cycle leaves behind: the deflated relation in slots 0 .. kk + e - 1
            int kk_new = 0;
            if (!broke && n >= 1) {
                DrPlan plan;
                const int target = std::min(std::min(keep, n - 2), ldp - e - 1);          // (- 1: a complex pair may add one)
                if (converged && n <= keep) kk_new = n;    // short solve: the whole relation stays as it is
                else if (target >= 1 && dr_plan(n + e, n, Hb.data(), ld, rho.data(), target, ldp, plan)) {
                    if ((rc = op_basis_rotate(h, V, n + e, plan.kk + e, plan.P.data(), ldp))) return rc;
                    if (use_flex && (rc = op_basis_rotate(h, Zq, n, plan.kk, nullptr, ldp))) return rc;
                    kk_new = plan.kk;
                    std::fill(Hb.begin(), Hb.end(), 0.0);
                    for (int jc = 0; jc < kk_new; jc++) for (int i = 0; i < kk_new + e; i++) Hb[(size_t)jc * ld + i] = plan.Hnew[(size_t)jc * (kk_new + e) + i];
                    std::fill(c.begin(), c.end(), 0.0);
                    for (int i = 0; i < kk_new + e; i++) c[i] = plan.cnew[i];
                    if (!converged) {
                        S.restarts++; S.kept = kk_new;
                        // From the first deflated restart on the recurrence is iterated a digit below the tolerance: it is the restarts that
                        // let it drift from the true residual (measured: 5-10 % of the tolerance on the indefinite sweep), and a failed check
                        // costs far more than that digit -- the solve starts afresh and has to find its deflation space again.
                        tol_it = std::min(tol_it, 0.1 * tol);
                    }
                }
            }
            kk = kk_new;
            if (converged || total >= maxit || kk == 0) break;           // kk == 0: plain restart from the true residual below
            n = kk;
        }
        if (!converged && total >= maxit) break;
        // ---- true residual: the verdict when the recurrence says converged, the new start otherwise
        r0 = V + (int64_t)(kk ? kk + e : 0) * vs;
        if ((rc = true_residual(r0)) || (rc = op_multidot(h, r0, V, kk ? kk + e : 0))) return rc;
        dots_ready = true;
        const double rt = sqrt(h->hres[kk ? kk + e : 0]);
        if (!(rt == rt)) return fail(h, KSFD_ENAN, "GMRES-DR: residual is not finite");
        rn = rt;
        std::fill(c.begin(), c.end(), 0.0);
        if (kk) for (int i = 0; i <= kk; i++) c[i] = h->hres[i];          // V_kk+1^T r of the verified iterate
        accepted = rt <= tol;
        if (!accepted && converged && anorm > 0.0 && rt <= 1.25 * tol) {
            if ((rc = op_multidot(h, x, x, 0))) return rc;
            const double allow = nnz_row * 1.1102230246251565e-16 * anorm * sqrt(h->hres[0]);
            dots_ready = false;
            if (rt <= tol + allow) { S.rounding_passes++; accepted = true; }
        }
        if (accepted) {
            // Last touch: the verified residual is projected once on the relation that stays behind (the coefficients are at hand,
            // no operator application).  In exact arithmetic it is orthogonal to range(Hb) already; what the projection removes is the
            // DRIFT between recurrence and true residual inside A * span(kept vectors) -- the slow directions, where a residual of the
            // size of the tolerance is amplified most in the solution (near-singular stage matrices: 1/lambda_min).  The residual
            // norm cannot grow by it: y minimises ||r - V_kk+1 Hb y||.
            double rproj = rt;
            if (kk && lsq(kk, 1, &rproj) && rproj <= rt) { if ((rc = update_x(kk))) return rc; S.projections++; }
            break;
        }
        if (converged) {
            S.true_resid_fail++;
            tol_it = 0.1 * tol;                            // the correction is iterated a digit further, so that drift of that size cannot fail the next check
            // a true residual that no longer halves from one check to the next sits on the rounding floor of b - A x
            if (prev_fail > 0.0 && rt > 0.5 * prev_fail && ++stagnant >= 3) break;
            prev_fail = rt;
        }
    }
    if (!x_set) HIPCHK(h, hipMemsetAsync(x, 0, sizeof(double) * (size_t)vs, h->st));
    if (stage >= 0 && stage < 4) S.stage_its[stage] += total;
    ls->its = total;
    ls->rel = rn / rel_den;
    if (!accepted) return fail(h, KSFD_ELINEAR, "GMRES-DR did not converge: %d iterations, true relative residual %.3e (tol %.3e)", total, rn / bn, tol / bn);
    if (kk >= 1) {
        ksfd_ctl::dr_relation_kept(h->cur);
        K.kk = kk; K.pc = pcmode; K.shift = shift; K.shift_pc = shift_pc;
        K.H.assign((size_t)(kk + e) * kk, 0.0);
        for (int j = 0; j < kk; j++) for (int i = 0; i < kk + e; i++) K.H[(size_t)j * (kk + e) + i] = Hb[(size_t)j * ld + i];
    }
    return KSFD_OK;
}
