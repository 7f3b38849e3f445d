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
