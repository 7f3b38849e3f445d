// libksfd_hip.so -- the small host algebra of the Krylov solvers (krylov.hip.h, krylov_dr.hip.h), in plain C++: no device code, no
// handle, no library.  Everything here works on a few numbers that a reduction brought back, so a small driver compiled with the host
// compiler exercises exactly what the library runs (tests/test_krylov_small_cpu.py).
//   hess_lsq         least squares on a kept (k+1) x k Hessenberg matrix (recycling: projection on an earlier stage's space)
//   hess_backsolve   back substitution on the triangular factor of a cycle
//   HessQR           incremental QR of a cycle's Hessenberg matrix by Givens rotations
//   cgs2_algebraic   second Gram-Schmidt projection and the norm of the result from the Gram row
//   recycle_uses     which earlier stages' spaces a stage projects on
//   recycle_decide   whether a solve recycles at all
//   cycle_room, cycle_first, cycle_next, gs_classic, async_cycle, rel_of   length of a GMRES cycle, which Gram-Schmidt it runs, what it reports
//   restart_fit, restart_cap   how many basis vectors ksfd_create allocates from the free device memory
//   cheb_setup       degree and monomial coefficients of the Chebyshev polynomial preconditioner
#pragma once
#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <vector>

namespace ksfd_krylov {

// Least squares min ||g - H y|| for a small upper-Hessenberg H ((k+1) x k, column-major, ld = k+1); also returns H y.
static inline void hess_lsq(const double *H, int k, const double *g, double *y, double *Hy)
{
    const int ld = k + 1;
    std::vector<double> R((size_t)ld * k), q((size_t)k + 1);
    for (int i = 0; i < ld * k; i++) R[i] = H[i];
    for (int i = 0; i <= k; i++) q[i] = g[i];
    for (int j = 0; j < k; j++) {
        const double a = R[j * ld + j], b = R[j * ld + j + 1], den = hypot(a, b);
        const double c = den > 0.0 ? a / den : 1.0, sn = den > 0.0 ? b / den : 0.0;
        for (int l = j; l < k; l++) {
            const double t = c * R[l * ld + j] + sn * R[l * ld + j + 1];
            R[l * ld + j + 1] = -sn * R[l * ld + j] + c * R[l * ld + j + 1];
            R[l * ld + j] = t;
        }
        const double t = c * q[j] + sn * q[j + 1];
        q[j + 1] = -sn * q[j] + c * q[j + 1];
        q[j] = t;
    }
    for (int i = k - 1; i >= 0; i--) {
        double t = q[i];
        for (int l = i + 1; l < k; l++) t -= R[l * ld + i] * y[l];
        y[i] = R[i * ld + i] != 0.0 ? t / R[i * ld + i] : 0.0;
    }
    for (int i = 0; i <= k; i++) {
        double t = 0.0;
        for (int l = 0; l < k; l++) t += H[l * ld + i] * y[l];
        Hy[i] = t;
    }
}

// R y = g for the leading k columns of the rotated Hessenberg matrix (upper triangular, column-major with leading dimension ld)
static inline void hess_backsolve(const double *R, int ld, const double *g, int k, double *y)
{
    for (int i = k - 1; i >= 0; i--) {
        double s = g[i];
        for (int q = i + 1; q < k; q++) s -= R[(size_t)ld * q + i] * y[q];
        y[i] = s / R[(size_t)ld * i + i];
    }
}

// Hessenberg matrix of one GMRES cycle of up to m columns, kept as it comes (Hraw: what recycling keeps) and rotated to triangular
// form column by column (H), with the right-hand side g = Q^T (beta e_0) whose next entry is the residual norm of the cycle so far.
struct HessQR {
    int ld;                             // m + 1
    std::vector<double> H, Hraw, cs, sn, g, y;
    explicit HessQR(int m) : ld(m + 1), H((size_t)(m + 1) * m, 0.0), Hraw((size_t)(m + 1) * m, 0.0), cs(m), sn(m), g(m + 1), y(m) {}
    void reset(double beta)
    {
        std::fill(g.begin(), g.end(), 0.0);
        g[0] = beta;
    }
    // column j = hcol[0 .. j+1]: apply the earlier rotations, form the new one; returns the residual estimate |g[j+1]|
    double push_column(int j, const double *hcol)
    {
        double *Hc = &H[(size_t)ld * j];
        for (int i = 0; i <= j + 1; i++) Hraw[(size_t)ld * j + i] = Hc[i] = hcol[i];
        for (int i = 0; i < j; i++) { double t = cs[i] * Hc[i] + sn[i] * Hc[i + 1]; Hc[i + 1] = -sn[i] * Hc[i] + cs[i] * Hc[i + 1]; Hc[i] = t; }
        const double den = hypot(Hc[j], Hc[j + 1]);
        cs[j] = den > 0.0 ? Hc[j] / den : 1.0;
        sn[j] = den > 0.0 ? Hc[j + 1] / den : 0.0;
        Hc[j] = den; Hc[j + 1] = 0.0;
        g[j + 1] = -sn[j] * g[j];
        g[j] = cs[j] * g[j];
        return fabs(g[j + 1]);
    }
    void solve(int j) { hess_backsolve(H.data(), ld, g.data(), j, y.data()); }     // y[0 .. j) of the first j columns
};

// CGS2 with the second projection done algebraically (halves the Gram-Schmidt traffic):
//   d = V^T w and the Gram row g = V^T v_j come from ONE pass over V; with G = V^T V,
//   the twice-projected coefficients are c = d + (I - G) d, and
//   ||w - V c||^2 = ww - 2 c.d + c.G c.   One fused update pass applies c and normalises.
// G: k x k in Gm with leading dimension ld; c -> hcol[0 .. k), ||w - V c||^2 -> *hn2.  Returns whether the caller may normalise with
// that norm; false: heavy cancellation (||w|| >> ||w - Vc||), apply c, then measure and project once more.
static inline bool cgs2_algebraic(const double *Gm, int ld, int k, const double *d, double ww, double *hcol, double *hn2)
{
    for (int i = 0; i < k; i++) {
        double s = 0.0;
        for (int l = 0; l < k; l++) s += ((i == l ? 1.0 : 0.0) - Gm[(size_t)i * ld + l]) * d[l];
        hcol[i] = d[i] + s;
    }
    double cd = 0.0, cGc = 0.0;
    for (int i = 0; i < k; i++) {
        cd += hcol[i] * d[i];
        double s = 0.0;
        for (int l = 0; l < k; l++) s += Gm[(size_t)i * ld + l] * hcol[l];
        cGc += hcol[i] * s;
    }
    *hn2 = ww - 2.0 * cd + cGc;
    return *hn2 > 1e-8 * ww;
}

// Does stage `stage` (0..3) of a step project its right-hand side on the space kept by the earlier stage q?  By default the selected
// ones below; every earlier one with rec_mode 2 or when whole cycles are kept (rec_full).  Callers ask for q < stage only.
static inline bool recycle_uses(int stage, int q, int rec_mode, bool rec_full)
{
    static const int sel[4][3] = { { -1, -1, -1 }, { 0, -1, -1 }, { 0, -1, -1 }, { 0, 2, -1 } };
    if (stage < 0 || stage > 3) return false;
    bool use = rec_mode == 2 || rec_full;
    for (int e = 0; e < 3; e++) use = use || sel[stage][e] == q;
    return use;
}

// With the multigrid preconditioner the LEADING vectors of an earlier stage buy nothing (measured on the 600-step 384^2 run:
// 20.4 s with, 18.9 s without).  Round 3 tried the other end (rec_full, KSFD_TUNE_REC_MG, off by default): keep the WHOLE first
// cycle of every stage -- the slow modes of shift*I - J that take the iterations late in a run sit in the tail of the Krylov
// space -- and project a later stage's right-hand side on A M^-1 V_k = V_k+1 H_k first (one multi-dot, one basis combination,
// ONE V cycle for all spaces together).  Measured: it does NOT pay -- aggregated state at 4096^2 x 3 (h = 4.4) 25 instead of 26
// iterations per step but 142 instead of 125 ms; indefinite tail of the 384^2 run (h = 400, tools/late_phase.py) 142 instead of
// 135 iterations per step.  What a later stage still has to resolve is not in the span of what an earlier one built.
struct RecycleChoice {
    bool rec_on;        // this solve projects on kept spaces and keeps its own
    bool rec_full;      // ... the whole first cycle of it (multigrid-preconditioned solves with rec_mg)
    bool reset;         // the kept spaces are dropped first: stage 0, no recycling, or too little room behind them
};
static inline RecycleChoice recycle_decide(int pcmode, int stage, int rec_mode, bool rec_mg, bool use_frozen, int restart_alloc, int rec_vtop)
{
    const bool use_pc = pcmode == 1;
    RecycleChoice c;
    c.rec_full = use_pc && rec_mg && stage >= 0 && stage < 4 && use_frozen && rec_mode > 0;
    c.rec_on = stage >= 0 && stage < 4 && rec_mode > 0 && use_frozen && (!use_pc || c.rec_full);
    c.reset = !c.rec_on || stage == 0 || restart_alloc - rec_vtop < (c.rec_full ? 16 : 6);
    if (c.reset && stage != 0) c.rec_on = false;
    return c;
}

// ---- cycle length ----
// Restart length.  The first cycle runs with ksp_restart (30: PETSc's default); a cycle that ends without convergence is followed by
// one of twice the length, up to what ksfd_create could allocate (restart_alloc, <= 120).  Restarted GMRES loses most on exactly the
// systems where it needs many iterations -- shift*I - J indefinite late in a run, 30-50 iterations per stage system -- and a longer
// basis costs little next to the V cycle and Jacobian actions of an iteration there.
// room: basis slots behind the kept spaces (vb: first slot of this solve's own vectors)
static inline int cycle_room(int restart_alloc, int vb) { return restart_alloc - vb; }
// m_opt: min(ksp_restart, restart_alloc).  rec_full: no restart inside the space that is going to be kept
static inline int cycle_first(int m_opt, int room, bool rec_on, bool rec_full) { return (rec_full && rec_on) ? room : std::min(m_opt, room); }
static inline int cycle_next(int m_cur, int room, bool restart_grow) { return restart_grow ? std::min(2 * m_cur, room) : m_cur; }
// Column k (= j + 1 vectors to project on) by classical CGS2 instead of the Gram-row variant: on request (opts.reserved bit 0), and beyond 30
// (the fused multi-dot + Gram-row kernel returns 2k + 1 numbers, sized for the 30 vectors of the default restart: longer cycles finish classically)
static inline bool gs_classic(int reserved, int k) { return (reserved & 1) || k > 30; }
// Pipelined solver: what the kernels of an iteration hold (maxk), whatever the basis has room for
static inline int async_cycle(int ksp_restart, int restart_alloc, int maxk) { return std::min(std::min(ksp_restart > 0 ? ksp_restart : 30, restart_alloc), maxk); }
// Relative residual a solve reports.  tol_abs > 0: a correction equation A d = b - A x0 solved to the absolute tolerance of the original
// system -- relative to the original right-hand side, whose norm is tol_abs / ksp_rtol
static inline double rel_of(double rn, double bn, double tol_abs, double ksp_rtol) { return rn / ((tol_abs > 0.0 && ksp_rtol > 0.0) ? tol_abs / ksp_rtol : bn); }

// ---- basis size ----
const int RESTART_DEFAULT = 30, RESTART_MAX = 120, RESTART_MIN = 8;     // below RESTART_MIN the grid does not fit the device
// KSFD_RESTART_MAX as the caller's environment gives it -> the cap on the basis
static inline int restart_cap(int env_value) { return std::max(RESTART_MIN, std::min(env_value, RESTART_MAX)); }
// Krylov storage is what scales with the restart length: V (m+1 vectors) + Zb (m).  Sized to the free device memory mfree (bytes):
// ~30 other full-size vectors of vecbytes (state, stage vectors, temporaries, coefficient planes, multigrid level 0 + coarse levels)
// must fit first.  Where memory is plentiful the basis may be longer than the first cycle's 30 vectors (cycle_next), up to cap and to
// 40 % of the free memory for V + Zb; where it is short, whatever fits (the caller refuses below RESTART_MIN).
static inline int restart_fit(double mfree, double vecbytes, int cap)
{
    const double room = 0.92 * mfree / vecbytes - 30.0;
    const int fit_room = (int)floor(std::min((room - 1.0) / 2.0, 1.0e6));
    const int fit_40 = (int)floor(std::min(0.4 * mfree / vecbytes / 2.0, 1.0e6));
    return std::max(std::min(std::min(cap, fit_room), fit_40), std::min(RESTART_DEFAULT, fit_room));
}

// ---- Chebyshev polynomial preconditioner ----
const int CHEB_MAX_DEG = 7;                     // largest degree ksfd_set_poly_params admits: alpha[0 .. CHEB_MAX_DEG]
const int CHEB_NCOEF = CHEB_MAX_DEG + 2;        // monomial coefficients of T_n(mu(l)), n = degree + 1 <= CHEB_MAX_DEG + 1
static_assert(CHEB_MAX_DEG + 1 == 8, "the handle keeps the coefficients in poly_alpha[8]");

// Coefficients of p, z = sum_i alpha_i (A/shift)^i v ~ A^-1 v, for the spectrum of A/shift in [a, b] = [0.97, 1 + 1.15 lamJ/shift] (power
// iteration converges from below: +15 %).  Returns the degree d (alpha[0 .. d] set); 0 = "do not precondition" (kappa = b/a < 1.3: GMRES
// alone needs <= 3 iterations).  target: wanted size of the residual polynomial r(l) = 1 - l p(l) on [a, b]; max_deg <= CHEB_MAX_DEG.
static inline int cheb_setup(double lamJ, double shift, double target, int max_deg, double alpha[8])
{
    const double a = 0.97, b = 1.0 + 1.15 * lamJ / shift;
    const double kappa = b / a;
    if (kappa < 1.3) return 0;
    const double rc_ = (sqrt(kappa) - 1.0) / (sqrt(kappa) + 1.0);
    int d = (int)ceil(log(target) / log(rc_)) - 1;                 // residual polynomial of degree d+1: ~2 rc^(d+1) <= 2*target
    d = std::min(std::max(d, 1), std::max(std::min(max_deg, CHEB_MAX_DEG), 1));
    // r(l) = T_{d+1}(mu(l)) / T_{d+1}(mu(0)), mu(l) = m0 + m1 l;  p(l) = (1 - r(l)) / l
    const int n = d + 1;
    double m0 = (b + a) / (b - a), m1 = -2.0 / (b - a);
    double Tp[CHEB_NCOEF] = { 1.0 }, Tc[CHEB_NCOEF] = { m0, m1 }, Tn[CHEB_NCOEF];
    int degc = 1;
    for (int k = 1; k < n; k++) {                                  // T_{k+1} = 2 mu T_k - T_{k-1} in the monomial basis; degc = k <= CHEB_MAX_DEG
        for (int i = 0; i < CHEB_NCOEF; i++) Tn[i] = 0.0;
        for (int i = 0; i <= degc; i++) { Tn[i] += 2.0 * m0 * Tc[i]; Tn[i + 1] += 2.0 * m1 * Tc[i]; }
        for (int i = 0; i <= degc - 1; i++) Tn[i] -= Tp[i];
        for (int i = 0; i < CHEB_NCOEF; i++) { Tp[i] = Tc[i]; Tc[i] = Tn[i]; }
        degc++;
    }
    const double t0 = Tc[0];                                       // T_n(mu(0))
    for (int i = 0; i <= d; i++) alpha[i] = -(Tc[i + 1] / t0) / shift;   // p_i = -r_{i+1}; the 1/shift turns p(A/shift) into ~A^-1
    return d;
}

}   // namespace ksfd_krylov
