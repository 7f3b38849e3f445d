// libksfd_hip.so -- small dense real algebra on the host for the deflated restart of GMRES (krylov_dr.hip.h).
// Plain C++, no device code and no library: orders are at most the restart length (<= 120), so everything here runs in
// microseconds next to one Jacobian action.  Matrices are row-major n x n unless said otherwise.
//   dense_eig      eigenvalues and eigenvectors of a general real matrix in real arithmetic: Householder reduction to
//                  Hessenberg form, Francis double-shift QR with accumulated transformations, back substitution (the
//                  classical EISPACK orthes / hqr2 sequence).  A complex pair comes back as two columns: real and imaginary part.
//   dense_lu_solve Gaussian elimination with partial pivoting, several right-hand sides
//   dr_plan        the restart of GMRES-DR (Morgan, SIAM J. Sci. Comput. 24, 2002): harmonic Ritz vectors of smallest modulus ->
//                  orthonormal P_{k+e}, the deflated relation P_{k+e}^T Hbar P_k and the projected residual
#pragma once
#include <math.h>
#include <algorithm>
#include <vector>

namespace ksfd_dense {

static inline void cdiv(double xr, double xi, double yr, double yi, double &re, double &im)
{
    double r, d;
    if (fabs(yr) > fabs(yi)) { r = yi / yr; d = yr + r * yi; re = (xr + r * xi) / d; im = (xi - r * xr) / d; }
    else { r = yr / yi; d = yi + r * yr; re = (r * xr + xi) / d; im = (r * xi - xr) / d; }
}

// A (row-major, destroyed) = V diag(lambda) V^-1.  wr/wi: real and imaginary parts; for a pair wi[j] > 0, wi[j+1] < 0 the
// eigenvector of wr[j] + i wi[j] is V[:, j] + i V[:, j+1].  false: the QR iteration did not converge.
static bool dense_eig(int nn, std::vector<double> &Hm, std::vector<double> &d, std::vector<double> &e, std::vector<double> &Vm)
{
    d.assign(nn, 0.0); e.assign(nn, 0.0); Vm.assign((size_t)nn * nn, 0.0);
    if (nn <= 0) return true;
#define H_(i, j) Hm[(size_t)(i) * nn + (j)]
#define V_(i, j) Vm[(size_t)(i) * nn + (j)]
    const int low = 0, high = nn - 1;
    std::vector<double> ort(nn, 0.0);
    // ---- Householder reduction to Hessenberg form
    for (int m = low + 1; m <= high - 1; m++) {
        double scale = 0.0;
        for (int i = m; i <= high; i++) scale += fabs(H_(i, m - 1));
        if (scale == 0.0) continue;
        double h = 0.0;
        for (int i = high; i >= m; i--) { ort[i] = H_(i, m - 1) / scale; h += ort[i] * ort[i]; }
        double g = sqrt(h);
        if (ort[m] > 0) g = -g;
        h -= ort[m] * g;
        ort[m] -= g;
        for (int j = m; j < nn; j++) {
            double f = 0.0;
            for (int i = high; i >= m; i--) f += ort[i] * H_(i, j);
            f /= h;
            for (int i = m; i <= high; i++) H_(i, j) -= f * ort[i];
        }
        for (int i = 0; i <= high; i++) {
            double f = 0.0;
            for (int j = high; j >= m; j--) f += ort[j] * H_(i, j);
            f /= h;
            for (int j = m; j <= high; j++) H_(i, j) -= f * ort[j];
        }
        ort[m] = scale * ort[m];
        H_(m, m - 1) = scale * g;
    }
    for (int i = 0; i < nn; i++) V_(i, i) = 1.0;
    for (int m = high - 1; m >= low + 1; m--) {
        if (H_(m, m - 1) == 0.0) continue;
        for (int i = m + 1; i <= high; i++) ort[i] = H_(i, m - 1);
        for (int j = m; j <= high; j++) {
            double g = 0.0;
            for (int i = m; i <= high; i++) g += ort[i] * V_(i, j);
            g = (g / ort[m]) / H_(m, m - 1);
            for (int i = m; i <= high; i++) V_(i, j) += g * ort[i];
        }
    }
    for (int i = 2; i < nn; i++) for (int j = 0; j < i - 1; j++) H_(i, j) = 0.0;       // the reflectors were stored below the subdiagonal
    // ---- Francis QR to real Schur form, transformations accumulated in V
    int n = nn - 1;
    const double eps = ldexp(1.0, -52);
    double exshift = 0.0, p = 0, q = 0, r = 0, s = 0, z = 0, t, w, x, y;
    double norm = 0.0;
    for (int i = 0; i < nn; i++) for (int j = std::max(i - 1, 0); j < nn; j++) norm += fabs(H_(i, j));
    if (!(norm == norm) || isinf(norm)) return false;
    int iter = 0, total_iter = 0;
    while (n >= low) {
        int l = n;
        while (l > low) {
            s = fabs(H_(l - 1, l - 1)) + fabs(H_(l, l));
            if (s == 0.0) s = norm;
            if (fabs(H_(l, l - 1)) < eps * s) break;
            l--;
        }
        if (l == n) {                                   // one root
            H_(n, n) += exshift;
            d[n] = H_(n, n); e[n] = 0.0;
            n--; iter = 0;
        } else if (l == n - 1) {                        // two roots
            w = H_(n, n - 1) * H_(n - 1, n);
            p = (H_(n - 1, n - 1) - H_(n, n)) / 2.0;
            q = p * p + w;
            z = sqrt(fabs(q));
            H_(n, n) += exshift;
            H_(n - 1, n - 1) += exshift;
            x = H_(n, n);
            if (q >= 0) {                               // real pair
                z = p >= 0 ? p + z : p - z;
                d[n - 1] = x + z;
                d[n] = d[n - 1];
                if (z != 0.0) d[n] = x - w / z;
                e[n - 1] = 0.0; e[n] = 0.0;
                x = H_(n, n - 1);
                s = fabs(x) + fabs(z);
                p = x / s; q = z / s;
                r = sqrt(p * p + q * q);
                p /= r; q /= r;
                for (int j = n - 1; j < nn; j++) { z = H_(n - 1, j); H_(n - 1, j) = q * z + p * H_(n, j); H_(n, j) = q * H_(n, j) - p * z; }
                for (int i = 0; i <= n; i++) { z = H_(i, n - 1); H_(i, n - 1) = q * z + p * H_(i, n); H_(i, n) = q * H_(i, n) - p * z; }
                for (int i = low; i <= high; i++) { z = V_(i, n - 1); V_(i, n - 1) = q * z + p * V_(i, n); V_(i, n) = q * V_(i, n) - p * z; }
            } else {                                    // complex pair
                d[n - 1] = x + p; d[n] = x + p;
                e[n - 1] = z; e[n] = -z;
            }
            n -= 2; iter = 0;
        } else {
            x = H_(n, n); y = 0.0; w = 0.0;
            if (l < n) { y = H_(n - 1, n - 1); w = H_(n, n - 1) * H_(n - 1, n); }
            if (iter == 10) {                           // exceptional shifts
                exshift += x;
                for (int i = low; i <= n; i++) H_(i, i) -= x;
                s = fabs(H_(n, n - 1)) + fabs(H_(n - 1, n - 2));
                x = y = 0.75 * s;
                w = -0.4375 * s * s;
            }
            if (iter == 30) {
                s = (y - x) / 2.0;
                s = s * s + w;
                if (s > 0) {
                    s = sqrt(s);
                    if (y < x) s = -s;
                    s = x - w / ((y - x) / 2.0 + s);
                    for (int i = low; i <= n; i++) H_(i, i) -= s;
                    exshift += s;
                    x = y = w = 0.964;
                }
            }
            iter++;
            if (++total_iter > 60 * nn + 200 || iter > 120) return false;
            int m = n - 2;
            while (m >= l) {
                z = H_(m, m);
                r = x - z; s = y - z;
                p = (r * s - w) / H_(m + 1, m) + H_(m, m + 1);
                q = H_(m + 1, m + 1) - z - r - s;
                r = H_(m + 2, m + 1);
                s = fabs(p) + fabs(q) + fabs(r);
                p /= s; q /= s; r /= s;
                if (m == l) break;
                if (fabs(H_(m, m - 1)) * (fabs(q) + fabs(r)) < eps * (fabs(p) * (fabs(H_(m - 1, m - 1)) + fabs(z) + fabs(H_(m + 1, m + 1))))) break;
                m--;
            }
            for (int i = m + 2; i <= n; i++) { H_(i, i - 2) = 0.0; if (i > m + 2) H_(i, i - 3) = 0.0; }
            for (int k = m; k <= n - 1; k++) {          // double QR step on rows l..n, columns m..n
                const bool notlast = k != n - 1;
                if (k != m) {
                    p = H_(k, k - 1); q = H_(k + 1, k - 1); r = notlast ? H_(k + 2, k - 1) : 0.0;
                    x = fabs(p) + fabs(q) + fabs(r);
                    if (x == 0.0) continue;
                    p /= x; q /= x; r /= x;
                }
                s = sqrt(p * p + q * q + r * r);
                if (p < 0) s = -s;
                if (s == 0.0) continue;
                if (k != m) H_(k, k - 1) = -s * x;
                else if (l != m) H_(k, k - 1) = -H_(k, k - 1);
                p += s;
                x = p / s; y = q / s; z = r / s;
                q /= p; r /= p;
                for (int j = k; j < nn; j++) {
                    p = H_(k, j) + q * H_(k + 1, j);
                    if (notlast) { p += r * H_(k + 2, j); H_(k + 2, j) -= p * z; }
                    H_(k, j) -= p * x;
                    H_(k + 1, j) -= p * y;
                }
                for (int i = 0; i <= std::min(n, k + 3); i++) {
                    p = x * H_(i, k) + y * H_(i, k + 1);
                    if (notlast) { p += z * H_(i, k + 2); H_(i, k + 2) -= p * r; }
                    H_(i, k) -= p;
                    H_(i, k + 1) -= p * q;
                }
                for (int i = low; i <= high; i++) {
                    p = x * V_(i, k) + y * V_(i, k + 1);
                    if (notlast) { p += z * V_(i, k + 2); V_(i, k + 2) -= p * r; }
                    V_(i, k) -= p;
                    V_(i, k + 1) -= p * q;
                }
            }
        }
    }
    if (norm == 0.0) return true;
    // ---- eigenvectors of the quasi-triangular form by back substitution
    for (n = nn - 1; n >= 0; n--) {
        p = d[n]; q = e[n];
        if (q == 0) {                                   // real vector
            int l = n;
            H_(n, n) = 1.0;
            for (int i = n - 1; i >= 0; i--) {
                w = H_(i, i) - p;
                r = 0.0;
                for (int j = l; j <= n; j++) r += H_(i, j) * H_(j, n);
                if (e[i] < 0.0) { z = w; s = r; }
                else {
                    l = i;
                    if (e[i] == 0.0) H_(i, n) = w != 0.0 ? -r / w : -r / (eps * norm);
                    else {
                        x = H_(i, i + 1); y = H_(i + 1, i);
                        q = (d[i] - p) * (d[i] - p) + e[i] * e[i];
                        t = (x * s - z * r) / q;
                        H_(i, n) = t;
                        H_(i + 1, n) = fabs(x) > fabs(z) ? (-r - w * t) / x : (-s - y * t) / z;
                    }
                    t = fabs(H_(i, n));
                    if ((eps * t) * t > 1) for (int j = i; j <= n; j++) H_(j, n) /= t;
                }
            }
        } else if (q < 0) {                             // complex vector: columns n-1 (real part) and n (imaginary part)
            int l = n - 1;
            if (fabs(H_(n, n - 1)) > fabs(H_(n - 1, n))) {
                H_(n - 1, n - 1) = q / H_(n, n - 1);
                H_(n - 1, n) = -(H_(n, n) - p) / H_(n, n - 1);
            } else {
                double cr, ci;
                cdiv(0.0, -H_(n - 1, n), H_(n - 1, n - 1) - p, q, cr, ci);
                H_(n - 1, n - 1) = cr; H_(n - 1, n) = ci;
            }
            H_(n, n - 1) = 0.0; H_(n, n) = 1.0;
            for (int i = n - 2; i >= 0; i--) {
                double ra = 0.0, sa = 0.0, vr, vi, cr, ci;
                for (int j = l; j <= n; j++) { ra += H_(i, j) * H_(j, n - 1); sa += H_(i, j) * H_(j, n); }
                w = H_(i, i) - p;
                if (e[i] < 0.0) { z = w; r = ra; s = sa; }
                else {
                    l = i;
                    if (e[i] == 0) {
                        cdiv(-ra, -sa, w, q, cr, ci);
                        H_(i, n - 1) = cr; H_(i, n) = ci;
                    } else {
                        x = H_(i, i + 1); y = H_(i + 1, i);
                        vr = (d[i] - p) * (d[i] - p) + e[i] * e[i] - q * q;
                        vi = (d[i] - p) * 2.0 * q;
                        if (vr == 0.0 && vi == 0.0) vr = eps * norm * (fabs(w) + fabs(q) + fabs(x) + fabs(y) + fabs(z));
                        cdiv(x * r - z * ra + q * sa, x * s - z * sa - q * ra, vr, vi, cr, ci);
                        H_(i, n - 1) = cr; H_(i, n) = ci;
                        if (fabs(x) > (fabs(z) + fabs(q))) {
                            H_(i + 1, n - 1) = (-ra - w * H_(i, n - 1) + q * H_(i, n)) / x;
                            H_(i + 1, n) = (-sa - w * H_(i, n) - q * H_(i, n - 1)) / x;
                        } else {
                            cdiv(-r - y * H_(i, n - 1), -s - y * H_(i, n), z, q, cr, ci);
                            H_(i + 1, n - 1) = cr; H_(i + 1, n) = ci;
                        }
                    }
                    t = std::max(fabs(H_(i, n - 1)), fabs(H_(i, n)));
                    if ((eps * t) * t > 1) for (int j = i; j <= n; j++) { H_(j, n - 1) /= t; H_(j, n) /= t; }
                }
            }
        }
    }
    for (int j = nn - 1; j >= low; j--)                 // back to the original basis
        for (int i = low; i <= high; i++) {
            z = 0.0;
            for (int k = low; k <= std::min(j, high); k++) z += V_(i, k) * H_(k, j);
            V_(i, j) = z;
        }
#undef H_
#undef V_
    for (double v : Vm) if (!(v == v) || isinf(v)) return false;
    return true;
}

// A X = B in place (A n x n row-major, destroyed; B n x nrhs row-major).  false: a pivot below rcond_min * max|A|.
static bool dense_lu_solve(int n, std::vector<double> &A, int nrhs, std::vector<double> &B, double rcond_min = 1e-13)
{
    double amax = 0.0;
    for (double v : A) amax = std::max(amax, fabs(v));
    if (!(amax > 0.0) || isinf(amax)) return false;
    for (int c = 0; c < n; c++) {
        int pv = c;
        for (int i = c + 1; i < n; i++) if (fabs(A[(size_t)i * n + c]) > fabs(A[(size_t)pv * n + c])) pv = i;
        if (!(fabs(A[(size_t)pv * n + c]) > rcond_min * amax)) return false;
        if (pv != c) {
            for (int j = 0; j < n; j++) std::swap(A[(size_t)c * n + j], A[(size_t)pv * n + j]);
            for (int j = 0; j < nrhs; j++) std::swap(B[(size_t)c * nrhs + j], B[(size_t)pv * nrhs + j]);
        }
        for (int i = c + 1; i < n; i++) {
            const double f = A[(size_t)i * n + c] / A[(size_t)c * n + c];
            if (f == 0.0) continue;
            for (int j = c; j < n; j++) A[(size_t)i * n + j] -= f * A[(size_t)c * n + j];
            for (int j = 0; j < nrhs; j++) B[(size_t)i * nrhs + j] -= f * B[(size_t)c * nrhs + j];
        }
    }
    for (int i = n - 1; i >= 0; i--)
        for (int j = 0; j < nrhs; j++) {
            double t = B[(size_t)i * nrhs + j];
            for (int l = i + 1; l < n; l++) t -= A[(size_t)i * n + l] * B[(size_t)l * nrhs + j];
            B[(size_t)i * nrhs + j] = t / A[(size_t)i * n + i];
        }
    return true;
}

// Least squares min ||c - Hb y|| for a dense nr x n matrix (column-major, leading dimension ld), nr >= n, by Householder QR.
// Returns the residual vector rho = c - Hb y as well.  false: a zero column during the factorisation (rank deficient).
static bool dense_lsq(int nr, int n, const double *Hb, int ld, const double *c, double *y, double *rho)
{
    std::vector<double> R((size_t)nr * n), qc(c, c + nr);
    for (int j = 0; j < n; j++) for (int i = 0; i < nr; i++) R[(size_t)j * nr + i] = Hb[(size_t)j * ld + i];
    for (int j = 0; j < n; j++) {
        double *cj = &R[(size_t)j * nr];
        double nrm = 0.0;
        for (int i = j; i < nr; i++) nrm += cj[i] * cj[i];
        nrm = sqrt(nrm);
        if (!(nrm > 0.0) || isinf(nrm)) return false;
        const double alpha = cj[j] > 0 ? -nrm : nrm;
        cj[j] -= alpha;                                 // cj[j..] is the reflector v now; I - beta v v^T maps the column to alpha e_j
        const double beta = -1.0 / (alpha * cj[j]);
        for (int l = j + 1; l < n; l++) {
            double *cl = &R[(size_t)l * nr];
            double sdot = 0.0;
            for (int i = j; i < nr; i++) sdot += cj[i] * cl[i];
            sdot *= beta;
            for (int i = j; i < nr; i++) cl[i] -= sdot * cj[i];
        }
        double sdot = 0.0;
        for (int i = j; i < nr; i++) sdot += cj[i] * qc[i];
        sdot *= beta;
        for (int i = j; i < nr; i++) qc[i] -= sdot * cj[i];
        cj[j] = alpha;                                  // every column right of j and the right-hand side have seen this reflector
        for (int i = j + 1; i < nr; i++) cj[i] = 0.0;
    }
    for (int i = n - 1; i >= 0; i--) {
        double t = qc[i];
        for (int l = i + 1; l < n; l++) t -= R[(size_t)l * nr + i] * y[l];
        const double dgl = R[(size_t)i * nr + i];
        if (dgl == 0.0) return false;
        y[i] = t / dgl;
    }
    for (int i = 0; i < nr; i++) {
        double t = c[i];
        for (int l = 0; l < n; l++) t -= Hb[(size_t)l * ld + i] * y[l];
        rho[i] = t;
    }
    return true;
}

struct DrPlan {
    int kk = 0;                         // harmonic Ritz vectors kept (keep, or keep + 1 when the last one is half of a complex pair)
    int e = 1;                          // trailing vectors: nr - n of the relation that was deflated
    int ldp = 0;                        // row stride of P
    std::vector<double> P;              // nr x (kk + e), row-major: orthonormal columns, the last e span the complement of range(Hb)
    std::vector<double> Hnew;           // (kk + e) x kk, column-major, leading dimension kk + e
    std::vector<double> cnew;           // kk + e: the residual in the new basis
    std::vector<double> theta_r, theta_i;   // the kept harmonic Ritz values
};

// Restart of GMRES-DR.  In: the relation A M^-1 V_n = V_nr Hb (Hb nr x n column-major, nr = n + e; rows n.. are the trailing block B),
// the residual rho = c - Hb y of its least-squares problem, keep = how many harmonic Ritz vectors to keep.
// The harmonic Ritz pairs (theta, g) are the eigenpairs of H_n + H_n^-T B^T B; their residuals Hb g - theta [g; 0] are orthogonal to
// range(Hb), an e-dimensional space that also holds rho.  So P = orth[ [g_1 .. g_k; 0] | basis of range(Hb)^perp ] closes the relation:
// Hb P_k lies in span(P).  e = 1 is Morgan's restart (the basis is rho alone); e > 1 arises when a solve started from a kept space and
// added the remainder of its residual to the basis (krylov_dr.hip.h).  false: no usable deflated relation (singular H_n, breakdown,
// eigen-solver failure, dependent vectors, a relation that does not close) -- the caller restarts plainly for this cycle.
static bool dr_plan(int nr, int n, const double *Hb, int ld, const double *rho, int keep, int ldp, DrPlan &out)
{
    if (keep < 1 || n < keep + 2 || nr <= n) return false;
    const int e = nr - n;
    std::vector<double> HT((size_t)n * n), BtB((size_t)n * n, 0.0), G((size_t)n * n);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) HT[(size_t)i * n + j] = Hb[(size_t)i * ld + j];      // H_n^T, row-major
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
        double t = 0.0;
        for (int q = 0; q < e; q++) t += Hb[(size_t)i * ld + n + q] * Hb[(size_t)j * ld + n + q];
        BtB[(size_t)i * n + j] = t;
    }
    if (!dense_lu_solve(n, HT, n, BtB)) return false;                    // BtB <- H_n^-T B^T B
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) G[(size_t)i * n + j] = Hb[(size_t)j * ld + i] + BtB[(size_t)i * n + j];
    for (double v : G) if (!(v == v) || isinf(v)) return false;
    std::vector<double> wr, wi, Ev;
    if (!dense_eig(n, G, wr, wi, Ev)) return false;
    std::vector<int> ord(n);
    for (int i = 0; i < n; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return hypot(wr[a], wi[a]) < hypot(wr[b], wi[b]); });
    // columns to keep: both halves of a pair or neither
    std::vector<int> cols;
    std::vector<char> taken(n, 0);
    for (int q = 0; q < n && (int)cols.size() < keep; q++) {
        const int j = ord[q];
        if (taken[j]) continue;
        if (wi[j] == 0.0) { cols.push_back(j); taken[j] = 1; }
        else {
            const int j0 = wi[j] > 0.0 ? j : j - 1;
            if (j0 < 0 || j0 + 1 >= n) return false;
            cols.push_back(j0); cols.push_back(j0 + 1);
            taken[j0] = taken[j0 + 1] = 1;
        }
    }
    const int kk = (int)cols.size();
    if (kk < 1 || kk + e > ldp || kk > n - 2) return false;
    out.kk = kk; out.e = e; out.ldp = ldp;
    const int np = kk + e;
    // candidates for the complement of range(Hb): rho first, then the least-squares residuals of the trailing unit vectors
    std::vector<std::vector<double>> comp;
    comp.emplace_back(rho, rho + nr);
    if (e > 1) {
        std::vector<double> unit(nr), yy(n), rr(nr);
        for (int q = 0; q < e; q++) {
            std::fill(unit.begin(), unit.end(), 0.0);
            unit[n + q] = 1.0;
            if (!dense_lsq(nr, n, Hb, ld, unit.data(), yy.data(), rr.data())) return false;
            comp.push_back(rr);
        }
    }
    out.P.assign((size_t)nr * ldp, 0.0);
    out.theta_r.resize(kk); out.theta_i.resize(kk);
    auto Pm = [&](int i, int j) -> double & { return out.P[(size_t)i * ldp + j]; };
    size_t next_comp = 0;
    for (int c = 0; c < np; c++) {
        if (c < kk) { for (int i = 0; i < n; i++) Pm(i, c) = Ev[(size_t)i * n + cols[c]]; out.theta_r[c] = wr[cols[c]]; out.theta_i[c] = wi[cols[c]]; }
        else {
            if (next_comp >= comp.size()) return false;
            for (int i = 0; i < nr; i++) Pm(i, c) = comp[next_comp][i];
            next_comp++;
        }
        double n0 = 0.0;
        for (int i = 0; i < nr; i++) n0 += Pm(i, c) * Pm(i, c);
        n0 = sqrt(n0);
        if (!(n0 > 0.0) || isinf(n0)) { if (c > kk) { c--; continue; } return false; }
        for (int i = 0; i < nr; i++) Pm(i, c) /= n0;
        for (int pass = 0; pass < 2; pass++)            // modified Gram-Schmidt, twice
            for (int b = 0; b < c; b++) {
                double t = 0.0;
                for (int i = 0; i < nr; i++) t += Pm(i, b) * Pm(i, c);
                for (int i = 0; i < nr; i++) Pm(i, c) -= t * Pm(i, b);
            }
        double n1 = 0.0;
        for (int i = 0; i < nr; i++) n1 += Pm(i, c) * Pm(i, c);
        n1 = sqrt(n1);
        if (!(n1 > 1e-8)) {                             // dependent on the vectors before it
            if (c > kk) { c--; continue; }                // a complement candidate: try the next one (rho itself must not be dropped)
            return false;
        }
        for (int i = 0; i < nr; i++) Pm(i, c) /= n1;
    }
    // Hnew = P_{k+1}^T Hb P_k, and how well Hb P_k lies in span(P_{k+1}) (exactly, for exact harmonic Ritz vectors)
    std::vector<double> HP((size_t)nr * kk, 0.0);      // column-major nr x kk
    for (int c = 0; c < kk; c++) for (int j = 0; j < n; j++) {
        const double pj = Pm(j, c);
        if (pj == 0.0) continue;
        for (int i = 0; i < nr; i++) HP[(size_t)c * nr + i] += Hb[(size_t)j * ld + i] * pj;
    }
    out.Hnew.assign((size_t)np * kk, 0.0);
    double defect = 0.0, total = 0.0;
    for (int c = 0; c < kk; c++) {
        for (int a = 0; a < np; a++) {
            double t = 0.0;
            for (int i = 0; i < nr; i++) t += Pm(i, a) * HP[(size_t)c * nr + i];
            out.Hnew[(size_t)c * np + a] = t;
        }
        for (int i = 0; i < nr; i++) {
            double t = HP[(size_t)c * nr + i];
            total += t * t;
            for (int a = 0; a < np; a++) t -= Pm(i, a) * out.Hnew[(size_t)c * np + a];
            defect += t * t;
        }
    }
    if (!(defect <= 1e-18 * total)) return false;       // relative 1e-9: the relation would not close
    out.cnew.assign(np, 0.0);
    for (int a = 0; a < np; a++) {
        double t = 0.0;
        for (int i = 0; i < nr; i++) t += Pm(i, a) * rho[i];
        out.cnew[a] = t;
    }
    return true;
}

}   // namespace ksfd_dense
