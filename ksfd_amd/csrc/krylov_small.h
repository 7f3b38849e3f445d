// libksfd_hip.so -- the small host algebra of the Krylov solvers (krylov.hip.h, krylov_dr.hip.h), in plain C++: no device code, no
// handle, no library.  Everything here works on a few numbers that a reduction brought back, so a small driver compiled with the host
// compiler exercises exactly what the library runs (tests/test_krylov_small_cpu.py).
//   hess_lsq         least squares on a kept (k+1) x k Hessenberg matrix (recycling: projection on an earlier stage's space)
//   hess_backsolve   back substitution on the triangular factor of a cycle
//   HessQR           incremental QR of a cycle's Hessenberg matrix by Givens rotations
//   cgs2_algebraic   second Gram-Schmidt projection and the norm of the result from the Gram row
//   recycle_uses     which earlier stages' spaces a stage projects on
//   recycle_decide   whether a solve recycles at all
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
// 20.4 s with, 18.9 s without).  Round 3 tried the other end (rec_full, KSFD_TUNE bit 20, off by default): keep the WHOLE first
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

}   // namespace ksfd_krylov
