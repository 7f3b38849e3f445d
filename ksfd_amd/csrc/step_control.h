// libksfd_hip.so -- the decisions of the Rosenbrock-W step driver (step.hip.h), in plain C++: no device code, no handle, no library.
// Everything here is host arithmetic on a few scalars, so a small driver compiled with the host compiler exercises exactly what the
// library runs (tests/test_step_control_cpu.py).
//   StepMemo             what the solvers remember from one step to the next; a checkpoint carries it whole
//   stiffness            X = h*gamma*lambda_max of the diffusion part
//   choose_regime        which stage solver an attempt uses (spectral / V cycle / polynomial wanted) ...
//   pipelined_allowed    ... and, once the polynomial is confirmed or not, whether the pipelined GMRES may run
//   stage_guess          least-squares coefficients of a stage's right-hand side in the earlier ones (regularised Gram system)
//   shift_floor_update   online search for the shift floor of the multigrid hierarchy
//   spec_backoff_update  back-off of the automatic spectral choice after a step it suited badly
//   spec_gmres_cap, spec_fallback_mg   leash of a spectral attempt's GMRES / which solver takes over after it (stage_solve)
//   spec_predict_on, spec_sweep, spec_pred_bound, spec_rho_roll, spec_handover, spec_handover_rel
//                        the defect-correction sweeps of spec_solve: verdict after a sweep's true residual, contraction memory,
//                        predicted last sweep, hand-over of the rest to GMRES
//   lam_due, lam_power_its, lam_estimated   when the eigenvalue estimate of the polynomial preconditioner is refreshed (plan_attempt)
//   adapt_basic          PETSc's TSAdaptChoose_Basic
#pragma once
#include <math.h>
#include <algorithm>
#include <type_traits>

namespace ksfd_ctl {

struct StepMemo {
    // polynomial preconditioner (est_lambda_max / poly_setup)
    double lamJ = -1.0;                 // running estimate of lambda_max(-J) = lambda_max(A) - shift
    int lam_age = 0, lam_period = 1;    // steps since the last estimate / re-estimate every lam_period steps (1..8, grows while stable)
    // multigrid preconditioner: lower bound on the shift the hierarchy is built for (see gmres) and the online search for it
    // (shift_floor_update: hill climbing in log2(floor) on the iterations per step)
    double mg_shift_floor = 0.0;
    int sf_dir = 0, sf_hold = 0;        // +1 doubling, -1 halving, 0 settled (and steps to wait before the next probe)
    bool sf_tried_down = false;
    double sf_prev_its = 0.0, sf_prev_floor = 0.0;
    long long nsteps = 0;               // ksfd_step calls so far
    // spectral preconditioner: steps (counted by ksfd_step calls) before which the automatic choice leaves it alone after it converged badly
    long long spec_bad_until = 0;
    int spec_backoff = 8;
    // largest contraction ||r_k+1|| / ||r_k|| of a defect-correction sweep measured in the current / the previous step
    // (spec_solve: predicted last sweep)
    double spec_rho_step = 0.0, spec_rho_prev = 0.0;
};
static_assert(std::is_trivially_copyable<StepMemo>::value, "a checkpoint saves and restores StepMemo by assignment");

// stiffness estimate X = h*gamma*lambda_max of the diffusion part; the multigrid preconditioner pays off above ~60
static inline double stiffness(double s2, const double *lig_D, int nlig, const double *inv_h2, int dim, double shift)
{
    double dmax = s2, lap = 0.0;
    for (int l = 0; l < nlig; l++) dmax = std::max(dmax, lig_D[l]);
    for (int a = 0; a < dim; a++) lap += (16.0 / 3.0) * inv_h2[a];
    return dmax * lap / shift;
}

struct RegimeIn {
    int pc_type, reserved;              // ksfd_step_opts
    double stiff;                       // stiffness()
    bool direct, dr_on;                 // pc_type 5 / deflated restarting
    bool spec_ok, user_off;             // spectral solver exists / switched off by the caller
    bool use_frozen, fused2d;           // frozen-coefficient kernels / the fused 2-D strip path applies
    bool mg_ok;                         // multigrid hierarchy exists
    double mg_threshold, spec_from;
    long long nsteps, bad_until;
    double unknowns;                    // per rank: F * nloc
    bool ring, device_allreduce;        // slab transport in use / it reduces on the device
    int async_mode;                     // 0 off, 1 whenever legal, 2 when the local problem is small
};
struct Regime { bool spec, mg, poly_wanted; };

static inline Regime choose_regime(const RegimeIn &in)
{
    Regime r;
    // (measured crossover against the degree-6 polynomial: X ~ 80 on 4096^2, ~ 280 on 1024^2 where the V cycle is latency-bound)
    const double mg_from = in.mg_threshold * (in.unknowns < 8.0e6 ? 3.0 : 1.0);
    // spectral preconditioner (constant-coefficient part of shift*I - J inverted by FFT): nearly exact while the state is a
    // smooth perturbation of a uniform one, at any stiffness; pc_type 2 uses it until it converges badly (spec_backoff_update), 4 always
    // (without the fused 2-D residual kernel a sweep costs more: 3-D at X = 0.29, 80 ms plain GMRES against 83 ms)
    r.spec = !in.direct && in.spec_ok && in.use_frozen &&
             (in.pc_type == 4 || (in.pc_type == 2 && in.stiff >= (in.fused2d ? in.spec_from : std::max(in.spec_from, 0.3)) &&
                                  in.nsteps > in.bad_until && !in.user_off));
    r.mg = !in.direct && !r.spec && in.mg_ok && in.use_frozen && (in.pc_type == 1 || (in.pc_type == 2 && in.stiff > mg_from));
    // polynomial preconditioner in the mildly stiff regime (pc_type 2 = automatic, 3 = polynomial whenever useful); confirmed by the
    // caller once the eigenvalue estimate has given it a degree
    r.poly_wanted = !r.spec && !r.mg && in.use_frozen && (in.pc_type == 2 || in.pc_type == 3) && in.stiff >= 0.3;
    return r;
}

// pipelined solver: latency-bound iterations only (small local problem), not in the tiny-h regime where the
// Pythagorean norm update cancels heavily (|w|^2/h_n^2 ~ 1/stiff^2) and gmres() takes its explicit second pass
static inline bool pipelined_allowed(const RegimeIn &in, const Regime &r, bool use_poly)
{
    const bool small = in.unknowns <= 6.0e6;
    return !in.dr_on && !in.direct && !r.spec && !r.mg && !use_poly && in.use_frozen && !(in.reserved & 1) && in.stiff >= 1e-3 &&
           (!in.ring || in.device_allreduce) &&
           (in.async_mode == 1 || (in.async_mode == 2 && small));
}

// Stage guess: c = argmin ||b_i - sum_j c_j b_j|| over the ng right-hand sides j0 <= j < i, from their Gram matrix gb (least squares on
// the ill-conditioned but tiny Gram system, diagonal scaled by 1 + 1e-13).  false: no guess -- singular or non-finite system, or the
// predicted residual ||b_i - sum c_j b_j||^2 is not below 0.09 ||b_i||^2.
static inline bool stage_guess(const double gb[4][4], int i, int j0, int ng, double cf[3])
{
    double M[3][4];
    for (int a = 0; a < ng; a++) { for (int c = 0; c < ng; c++) M[a][c] = gb[j0 + a][j0 + c]; M[a][ng] = gb[i][j0 + a]; M[a][a] *= 1.0 + 1e-13; }
    bool okls = ng > 0;
    for (int c = 0; c < ng && okls; c++) {              // Gaussian elimination with partial pivoting
        int pv = c;
        for (int a = c + 1; a < ng; a++) if (fabs(M[a][c]) > fabs(M[pv][c])) pv = a;
        if (!(fabs(M[pv][c]) > 0.0)) { okls = false; break; }
        for (int q = 0; q <= ng; q++) std::swap(M[c][q], M[pv][q]);
        for (int a = c + 1; a < ng; a++) { const double f = M[a][c] / M[c][c]; for (int q = c; q <= ng; q++) M[a][q] -= f * M[c][q]; }
    }
    cf[0] = cf[1] = cf[2] = 0.0;
    for (int a = ng - 1; a >= 0 && okls; a--) { double t = M[a][ng]; for (int q = a + 1; q < ng; q++) t -= M[a][q] * cf[q]; cf[a] = t / M[a][a]; }
    double pred = gb[i][i];                                // ||b_i - sum c_j b_j||^2 = b.b - 2 c.g + c.G c
    for (int a = 0; a < ng; a++) { pred -= 2.0 * cf[a] * gb[i][j0 + a]; for (int c = 0; c < ng; c++) pred += cf[a] * cf[c] * gb[j0 + a][j0 + c]; }
    return okls && pred == pred && pred < 0.09 * gb[i][i];
}

// Shift floor of the multigrid hierarchy (gmres(): shift_pc = max(shift, floor)).  Once 1/(gamma h) has fallen below the
// growth rate of the chemotactic instability the V cycle of shift*I - J stops contracting and the iteration count explodes
// (options81 run, h ~ 350: 480 iterations per step; with a floor of 0.2: 120).  The right floor is a property of J we do
// not know, so it is searched online: when a step needs > 64 iterations, double the floor while that pays (> 5 % fewer
// iterations), else go back and try halving, else settle for 25 steps.
static inline void shift_floor_update(StepMemo &m, double its, double shift)
{
    if (m.sf_dir == 0) {
        if (m.sf_hold > 0) m.sf_hold--;
        else if (its > 64.0) {
            m.sf_prev_its = its; m.sf_prev_floor = m.mg_shift_floor;
            m.mg_shift_floor = 2.0 * std::max(m.mg_shift_floor, shift);
            m.sf_dir = 1; m.sf_tried_down = false;
        }
    } else if (its < 0.95 * m.sf_prev_its) {
        m.sf_prev_its = its; m.sf_prev_floor = m.mg_shift_floor;
        m.mg_shift_floor = m.sf_dir > 0 ? 2.0 * m.mg_shift_floor : 0.5 * m.mg_shift_floor;
        if (m.mg_shift_floor <= shift) { m.sf_dir = 0; m.sf_hold = 25; }          // floor no longer active
    } else {
        m.mg_shift_floor = m.sf_prev_floor;
        if (m.sf_dir > 0 && !m.sf_tried_down && 0.5 * m.sf_prev_floor > shift) {
            m.sf_dir = -1; m.sf_tried_down = true;
            m.mg_shift_floor = 0.5 * m.sf_prev_floor;
        } else { m.sf_dir = 0; m.sf_hold = 25; }
    }
}

// adaptation of the automatic spectral choice: > 12 iterations per stage system (or a failed attempt) means the coefficients vary too
// much for the constant-coefficient inverse; leave it alone for a while (doubling) and let the polynomial / V cycle work
static inline void spec_backoff_update(StepMemo &m, bool failed, int its, long long nsteps)
{
    if (failed || its > 48) {
        m.spec_bad_until = nsteps + m.spec_backoff;
        m.spec_backoff = std::min(2 * m.spec_backoff, 512);
    } else m.spec_backoff = 8;
}

// A spectral attempt of the automatic choice (pc_type 2) caps the GMRES that takes over from slow sweeps, so that a state the
// preconditioner does not suit costs little: 40 iterations, 8 on a re-trial after a back-off period (spec_backoff already doubled).
// 0: no cap (pc_type 4).
static inline int spec_gmres_cap(int pc_type, int backoff) { return pc_type == 2 ? (backoff > 8 ? 8 : 40) : 0; }
// ... and what solves the stage after a failed attempt: the V cycle where there is one and the step is stiff enough for it, else plain GMRES
static inline bool spec_fallback_mg(bool mg_ok, double stiff) { return mg_ok && stiff > 0.3; }

// ---- defect-correction sweeps of the spectral stage solver (spec_solve) ----
const int SPEC_SWEEP_CAP = 24;              // sweeps per solve before the rest goes to GMRES
const double SPEC_SLOW_RATIO = 0.25;        // a sweep that leaves more than this of the residual is slow: the coefficients vary too much
const double SPEC_PRED_SAFETY = 4.0;        // predicted last sweep: SAFETY * rho_hat * ||r_k|| <= tol
const double SPEC_PRED_MIN_RTOL = 1e-8;     // ... off below this ksp_rtol (the parity tests verify every solve)

// Predicted last sweep on?  spec_predict: the handle's switch (KSFD_TUNE_NO_SPEC_PREDICT); reserved bit 3: the caller's; verify_env: KSFD_SPEC_VERIFY
// (2 = off, 1 = on and every skipped residual evaluated anyway).
static inline bool spec_predict_on(bool spec_predict, int reserved, double ksp_rtol, int verify_env)
{
    return spec_predict && !(reserved & 8) && ksp_rtol >= SPEC_PRED_MIN_RTOL && verify_env != 2;
}

// rho_hat: the largest contraction measured in this step and the previous one
static inline double spec_rho_hat(const StepMemo &m) { return std::max(m.spec_rho_step, m.spec_rho_prev); }

// start of a step: this step's maximum replaces the last one's (a step that recorded none keeps it)
static inline void spec_rho_roll(StepMemo &m)
{
    if (m.spec_rho_step > 0.0) m.spec_rho_prev = m.spec_rho_step;
    m.spec_rho_step = 0.0;
}

enum SpecVerdict {
    SPEC_NOT_FINITE,        // the residual is NaN
    SPEC_CONVERGED,         // rn <= tol
    SPEC_SLOW,              // rn > SPEC_SLOW_RATIO * rprev: hand the rest to GMRES
    SPEC_CONTINUE,          // another sweep, its residual evaluated
    SPEC_CONTINUE_FINAL     // another sweep, predicted to be the last: return after it without evaluating the residual
};

// Verdict after sweep k (0-based, cap sweeps at most) left the true residual norm rn; rprev: the one before it (||b|| for k = 0).
// A contraction ratio enters the memory only between residuals of iterates that have been through a sweep (k >= 1), and only from a sweep
// that goes on.  The first sweep from zero is a class of its own and is neither recorded nor predicted from: b = f(u) is
// smooth, (I - A M^-1) b = dJ M^-1 b is several times larger relative to b (3-6 % on the bench window) than the same operator
// makes of the rough residuals that follow (0.6-1 %), and after one sweep a residual never is that smooth again.  With an initial guess
// (guess) the residual after sweep 0 is rough already, and a rho_prev left by the previous step may predict from it.
static inline SpecVerdict spec_sweep(int k, int cap, double rn, double rprev, double tol, bool guess, bool predict, StepMemo &m)
{
    if (!(rn == rn)) return SPEC_NOT_FINITE;
    if (rn <= tol) return SPEC_CONVERGED;
    if (rn > SPEC_SLOW_RATIO * rprev) return SPEC_SLOW;
    if (k >= 1) m.spec_rho_step = std::max(m.spec_rho_step, rn / rprev);
    const double rho_hat = spec_rho_hat(m);
    const bool final_next = predict && rho_hat > 0.0 && (k >= 1 || guess) && k + 1 < cap && SPEC_PRED_SAFETY * rho_hat * rn <= tol;
    return final_next ? SPEC_CONTINUE_FINAL : SPEC_CONTINUE;
}

// what a predicted exit reports as its relative residual: the bound the decision was made on (rn: the last residual evaluated)
static inline double spec_pred_bound(const StepMemo &m, double rn, double bn) { return SPEC_PRED_SAFETY * spec_rho_hat(m) * rn / bn; }

// Hand-over of the correction equation A d = r to GMRES.  true: the sweeps made it worse than x = 0 -- forget x and solve A x = b.
static inline bool spec_handover(double rn, double bn) { return !(rn < bn); }
// ... and the relative residual of the whole solve from that of the correction solve (relative to its own right-hand side, r or b)
static inline double spec_handover_rel(double gmres_rel, bool from_zero, double rn, double bn) { return gmres_rel * (from_zero ? 1.0 : rn / bn); }

// ---- eigenvalue estimate of the polynomial preconditioner (plan_attempt, once per step) ----
// Due on the first step (lamJ < 0) and every lam_period steps after an estimate; lam_age counts only once there is an estimate.
static inline bool lam_due(StepMemo &m) { return m.lamJ < 0.0 || ++m.lam_age >= m.lam_period; }
// power iterations: warm-started after the first estimate (before: lamJ as it was)
static inline int lam_power_its(double before) { return before < 0.0 ? 8 : 2; }
// J changes slowly from step to step: while the estimate moves by < 2 %, look less often (every 2, 4, 8 steps)
static inline void lam_estimated(StepMemo &m, double before)
{
    const bool stable = before > 0.0 && fabs(m.lamJ - before) <= 0.02 * before;
    m.lam_period = stable ? std::min(2 * m.lam_period, 8) : 1;
    m.lam_age = 0;
}

// TSAdaptChoose_Basic
struct AdaptChoice { bool accept; double hnext; };
static inline AdaptChoice adapt_basic(double hh, double wrms, bool prev_accept, double safety, double reject_safety,
                                      double clip_lo, double clip_hi, double dt_min, double dt_max)
{
    AdaptChoice r;
    r.accept = true;
    if (wrms > 1.0) {
        if (!prev_accept) safety *= reject_safety;
        r.accept = hh < (1.0 + 1.4901161193847656e-08) * dt_min;   // at minimum step: accept anyway
    }
    double hfac = wrms > 0.0 ? safety * pow(wrms, -1.0 / 3.0) : INFINITY;
    hfac = std::min(std::max(hfac, clip_lo), clip_hi);
    r.hnext = std::min(std::max(hh * hfac, dt_min), dt_max);
    return r;
}

}  // namespace ksfd_ctl
