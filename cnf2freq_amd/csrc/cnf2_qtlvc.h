// cnf2_qtlvc.h -- the variance-component QTL scan (cnf2_qtl_scan_vc, include/cnf2hip.h), shared by host and device code: the
// schedule and the rotation of the cyclic Jacobi iteration, the eigenvalue order and the rank rule, the grid tables of a marker,
// the search of one (marker, column) cell, one marker fitted serially on the CPU, and what the kernels of
// cnf2_qtlvc_kernels.hip read and write.  The design row, the mask and the gather list are cnf2_qtlhap.h's, the Cholesky
// factor of the null design cnf2_qtl.h's.
//
// The founder-allele effects are random: y = X0 b + Z u + e, u ~ N(0, s_u^2 I_H), e ~ N(0, s_e^2 I), one variance component per
// locus (the flexible intercross analysis of Ronnegard, Besnier and Carlborg 2008).  The inputs are cnf2_qtl_scan_hap's with
// H = 1 .. 64; c_i, n_c, Z[i][h], X0 = [1, centred cov], the centring, S11, b0, RSS0 and the conditions under which a chromosome
// is not scanned are that scan's (cnf2_qtlhap.h).  Per marker
//   W = Z'Z - S21 S11^-1 S21',  v = Z'y - S21 S11^-1 X0'y,  nu = n_c - 1 - K,
//   W = Q diag(d) Q' (eigenvalues below 0 count as 0),  rank = the number of d_k > 1e-10 d_max,  t = Q'v;
// only the terms of the rank enter the sums below.  The rows of Z add up to 2 c_i, so W always has null directions: they are
// the normal path.  The restricted likelihood is that of A'y with A A' = I - X0 (X0'X0)^-1 X0': log|I + g A'ZZ'A| = log|I_H + g W|
// and by Woodbury the quadratic form is RSS0 - g v'(I + g W)^-1 v.  With g = h / (1 - h), h in [0, 0.999]:
//   q(h) = RSS0 - sum_k g t_k^2 / (1 + g d_k)          clamped below at RSS0 2^-52
//   f(h) = ( nu log10(RSS0 / q(h)) - sum_k log10(1 + g d_k) ) / 2,   f(0) = 0.
// The search: 41 grid points h_j = 0.999 j / 40, j* the first arg-max, h^ the maximiser of f on [h_max(j*-1,0), h_min(j*+1,40)]
// by QTLVC_REFINE bisections on the sign of f'(h) (qtlvc_slope: no logarithm), which leaves it within 0.05 2^-21 < 1e-7;
// lod = max(f(h^), 0), and h^ = 0 wherever the LOD is 0.  sigma2 = q(h^) / nu, blup = Q diag(g / (1 + g d_k)) t (0 at h^ = 0).
// The grid pass compares without a logarithm or a division: f_a > f_b exactly when E_a q_b > E_b q_a with
// E_j = 10^(-sum_k log10(1 + g_j d_k) / nu), a table of the marker like g_j / (1 + g_j d_k).
// A marker with nu < 2 or rank = 0 reports lod 0, h 0, blup 0 and sigma2 = RSS0 / nu (0 where nu < 1).
//
// The Jacobi iteration is cyclic: a sweep is Hp - 1 rounds (Hp = H rounded up to even) of Hp / 2 disjoint pairs in the fixed
// round-robin order of qtlvc_pair; a pair with |W_pq| <= 2^-52 sqrt(|W_pp W_qq|) is left alone, the others are rotated (columns
// of every pair of the round first, then rows, then the pair's own 2 x 2 block from the closed form, W_pq = 0 exactly).  It stops
// after a sweep that rotated nothing, or after QTLVC_SWEEPS sweeps: a marker that has not converged reports rank -1 and lod 0.
// (|W_pp W_qq|: a null direction's diagonal entry is rounding noise of either sign.)
#ifndef CNF2_QTLVC_H
#define CNF2_QTLVC_H

#include "cnf2_qtlhap.h"

namespace cnf2 {

constexpr int    QTLVC_MAXH   = 64;        // model columns at most: 32 phased grandparents
constexpr int    QTLVC_GRID   = 41;        // grid points h_j = QTLVC_HMAX j / 40
constexpr double QTLVC_HMAX   = 0.999;
constexpr int    QTLVC_SWEEPS = 30;        // Jacobi sweeps at most
constexpr int    QTLVC_REFINE = 21;        // bisections of the bracket (two grid steps, 0.04995)
constexpr double QTLVC_RANK   = 1e-10;     // an eigenvalue counts when it is above this times the largest
constexpr double QTLVC_EPS    = 2.220446049250313e-16;

CNF2_HD constexpr int qtlvc_ld(int H) { return H | 1; }     // leading dimension of W in LDS: odd, a column walks all banks
// doubles of a marker's record: d[H], Qt[H][H] (row k the eigenvector of d_k, descending), G[H][nx], E[41], gtab[41][H]
CNF2_HD constexpr int qtlvc_o_qt(int H) { return H; }
CNF2_HD constexpr int qtlvc_o_g(int H) { return H + H * H; }
CNF2_HD constexpr int qtlvc_o_e(int H, int nx) { return H + H * H + H * nx; }
CNF2_HD constexpr int qtlvc_o_gtab(int H, int nx) { return qtlvc_o_e(H, nx) + QTLVC_GRID; }
CNF2_HD constexpr int qtlvc_rec_size(int H, int nx) { return qtlvc_o_gtab(H, nx) + QTLVC_GRID * H; }

CNF2_HD double qtlvc_grid_h(int j) { return QTLVC_HMAX * (double)j / (double)(QTLVC_GRID - 1); }
CNF2_HD double qtlvc_g(double h) { return h / (1.0 - h); }

// pair k (0 .. Hp/2 - 1) of round r (0 .. Hp - 2) of the round-robin schedule on Hp (even) indices: p < q
CNF2_HD void qtlvc_pair(int Hp, int r, int k, int* p, int* q)
{
    const int m = Hp - 1;
    const int a = k == 0 ? m : (r + k) % m, b = (r + m - k) % m;
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// The rotation of the pair: false (c = 1, s = 0) when the entry is small enough to stay.  t = tan of the angle: the closed
// form of the 2 x 2 block is W_pp - t W_pq, W_qq + t W_pq, 0.
CNF2_HD bool qtlvc_rotation(double app, double aqq, double apq, double* c, double* s, double* t)
{
    *c = 1.0, *s = 0.0, *t = 0.0;
    if (fabs(apq) <= QTLVC_EPS * sqrt(fabs(app * aqq))) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    const double tt    = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    *t = theta < 0.0 ? -tt : tt;
    *c = 1.0 / sqrt(*t * *t + 1.0);
    *s = *t * *c;
    return true;
}

// the position of eigenvalue k in descending order (ties by index)
CNF2_HD int qtlvc_position(const double* d, int H, int k)
{
    int pos = 0;
    for (int j = 0; j < H; j++) pos += (d[j] > d[k] || (d[j] == d[k] && j < k)) ? 1 : 0;
    return pos;
}

// the rank of sorted, clamped eigenvalues
CNF2_HD int qtlvc_rank(const double* d, int H)
{
    int r = 0;
    for (int k = 0; k < H; k++) r += d[k] > QTLVC_RANK * d[0] ? 1 : 0;
    return r;
}

// the tables of grid point j from the sorted eigenvalues: gtab[k] = g_j / (1 + g_j d_k), returns E_j
CNF2_HD double qtlvc_grid_tables(const double* d, int H, int rank, int nu, int j, double* gtab)
{
    const double g = qtlvc_g(qtlvc_grid_h(j));
    double       ls = 0.0;
    for (int k = 0; k < H; k++) {
        gtab[k] = g / (1.0 + g * d[k]);
        if (k < rank) ls += log10(1.0 + g * d[k]);
    }
    return pow(10.0, -ls / (double)nu);
}

// q(g), clamped, and the sign carrier of f'(h): nu sum t_k^2 / (1 + g d_k)^2 - q sum d_k / (1 + g d_k).  t at stride ts.
CNF2_HD double qtlvc_slope(const double* d, const double* t, size_t ts, int rank, double rss0, int nu, double g, double* q_out)
{
    double a = 0.0, b = 0.0, s = 0.0;
    for (int k = 0; k < rank; k++) {
        const double w = 1.0 / (1.0 + g * d[k]), tw = t[k * ts] * w;
        s += g * t[k * ts] * tw;
        a += tw * tw;
        b += d[k] * w;
    }
    double       q  = rss0 - s;
    const double lo = rss0 * QTLVC_EPS;
    q               = q > lo ? q : lo;
    *q_out          = q;
    return (double)nu * a - q * b;
}

struct QtlVcCell {
    double lod, h, sigma2, g;
};

// One (marker, column) cell from t = Q'v (stride ts), the marker's sorted eigenvalues and grid tables (E[41], gtab[41][H]).
// ok: the chromosome is scanned, the iteration converged, rank > 0 and nu >= 2.
CNF2_HD QtlVcCell qtlvc_cell(const double* d, const double* E, const double* gtab, int H, int rank, const double* t, size_t ts,
                             double rss0, int nu, bool ok)
{
    QtlVcCell r;
    r.lod = r.h = r.g = 0.0;
    r.sigma2 = (nu >= 1 && rss0 > 0.0) ? rss0 / (double)nu : 0.0;
    if (!ok || !(rss0 > 0.0)) return r;
    const double lo = rss0 * QTLVC_EPS;
    // the grid: the first arg-max of f, compared as E_j / q_j
    int    js = 0;
    double eb = 1.0, qb = rss0;
    for (int j = 1; j < QTLVC_GRID; j++) {
        const double* gt = gtab + (size_t)j * H;
        double        s  = 0.0;
        for (int k = 0; k < rank; k++) s += gt[k] * (t[k * ts] * t[k * ts]);
        double q = rss0 - s;
        q        = q > lo ? q : lo;
        if (E[j] * qb > eb * q) js = j, eb = E[j], qb = q;
    }
    // the bracket and the bisection on the sign of f'
    double h_lo = qtlvc_grid_h(js > 0 ? js - 1 : 0), h_hi = qtlvc_grid_h(js < QTLVC_GRID - 1 ? js + 1 : QTLVC_GRID - 1);
    // An end where f does not rise into the bracket is given up for the grid's own maximum h_js: what is reported is never
    // below the grid's maximum, also where f has two local maxima inside the bracket.
    double q, h;
    bool   up = qtlvc_slope(d, t, ts, rank, rss0, nu, qtlvc_g(h_lo), &q) > 0.0;
    bool   dn = qtlvc_slope(d, t, ts, rank, rss0, nu, qtlvc_g(h_hi), &q) < 0.0;
    if (!up && js > 0) {
        h_lo = qtlvc_grid_h(js);
        up   = qtlvc_slope(d, t, ts, rank, rss0, nu, qtlvc_g(h_lo), &q) > 0.0;
    }
    if (!dn && js < QTLVC_GRID - 1) {
        h_hi = qtlvc_grid_h(js);
        dn   = qtlvc_slope(d, t, ts, rank, rss0, nu, qtlvc_g(h_hi), &q) < 0.0;
    }
    if (!up) h = h_lo;
    else if (!dn) h = h_hi;
    else {
        for (int it = 0; it < QTLVC_REFINE; it++) {
            const double mid = 0.5 * (h_lo + h_hi);
            if (qtlvc_slope(d, t, ts, rank, rss0, nu, qtlvc_g(mid), &q) > 0.0) h_lo = mid;
            else h_hi = mid;
        }
        h = 0.5 * (h_lo + h_hi);
    }
    const double g = qtlvc_g(h);
    qtlvc_slope(d, t, ts, rank, rss0, nu, g, &q);
    double ls = 0.0;
    for (int k = 0; k < rank; k++) ls += log10(1.0 + g * d[k]);
    const double f = 0.5 * ((double)nu * log10(rss0 / q) - ls);
    if (f > 0.0 && h > 0.0) {
        r.lod    = f;
        r.h      = h;
        r.g      = g;
        r.sigma2 = q / (double)nu;
    }
    return r;
}

// ------------------------------------------------------------------------------------------------ one marker on the CPU
// W[H][ld] (symmetric, both triangles) -> eigenvalues on its diagonal and Qt[H][H] (row k the eigenvector of W[k][k]), by the
// kernels' steps.  false: not converged after QTLVC_SWEEPS sweeps.
inline bool qtlvc_jacobi_serial(double* W, int ld, double* Qt, int H)
{
    for (int k = 0; k < H; k++)
        for (int h = 0; h < H; h++) Qt[(size_t)k * H + h] = k == h ? 1.0 : 0.0;
    const int Hp = H + (H & 1), np = Hp / 2;
    double    c[QTLVC_MAXH / 2], s[QTLVC_MAXH / 2], t[QTLVC_MAXH / 2], app[QTLVC_MAXH / 2], aqq[QTLVC_MAXH / 2], apq[QTLVC_MAXH / 2];
    int       pp[QTLVC_MAXH / 2], qq[QTLVC_MAXH / 2];
    bool      on[QTLVC_MAXH / 2];
    for (int sweep = 0; sweep < QTLVC_SWEEPS; sweep++) {
        bool any = false;
        for (int r = 0; r < Hp - 1; r++) {
            for (int k = 0; k < np; k++) {
                qtlvc_pair(Hp, r, k, &pp[k], &qq[k]);
                on[k] = false;
                if (qq[k] >= H) continue;
                app[k] = W[(size_t)pp[k] * ld + pp[k]], aqq[k] = W[(size_t)qq[k] * ld + qq[k]], apq[k] = W[(size_t)pp[k] * ld + qq[k]];
                on[k]  = qtlvc_rotation(app[k], aqq[k], apq[k], &c[k], &s[k], &t[k]);
                any    = any || on[k];
            }
            for (int k = 0; k < np; k++) {      // columns of W, rows of Qt
                if (!on[k]) continue;
                for (int i = 0; i < H; i++) {
                    double *x = &W[(size_t)i * ld + pp[k]], *y = &W[(size_t)i * ld + qq[k]];
                    const double a = *x, b = *y;
                    *x = c[k] * a - s[k] * b, *y = s[k] * a + c[k] * b;
                    x = &Qt[(size_t)pp[k] * H + i], y = &Qt[(size_t)qq[k] * H + i];
                    const double e = *x, f = *y;
                    *x = c[k] * e - s[k] * f, *y = s[k] * e + c[k] * f;
                }
            }
            for (int k = 0; k < np; k++) {      // rows of W
                if (!on[k]) continue;
                for (int j = 0; j < H; j++) {
                    double *x = &W[(size_t)pp[k] * ld + j], *y = &W[(size_t)qq[k] * ld + j];
                    const double a = *x, b = *y;
                    *x = c[k] * a - s[k] * b, *y = s[k] * a + c[k] * b;
                }
            }
            for (int k = 0; k < np; k++) {      // the pair's own block
                if (!on[k]) continue;
                W[(size_t)pp[k] * ld + pp[k]] = app[k] - t[k] * apq[k];
                W[(size_t)qq[k] * ld + qq[k]] = aqq[k] + t[k] * apq[k];
                W[(size_t)pp[k] * ld + qq[k]] = W[(size_t)qq[k] * ld + pp[k]] = 0.0;
            }
        }
        if (!any) return true;
    }
    return false;
}

// One marker of the scan, serially, by the steps and in the order of the kernels: the arguments of qtlhap_marker_serial;
// lod[T], h[T], sigma2[T], blup[T][H] (may be null), eval[H] (may be null), *rank, rss0[T], *n_used.  false: an argument out
// of range.
inline bool qtlvc_marker_serial(int n, const double* descent, const int32_t* col, int H, int T, const double* y, int K,
                                const double* cov, const uint8_t* c, double* lod, double* h_out, double* sigma2, double* blup,
                                double* eval, int32_t* rank_out, double* rss0, int32_t* n_used)
{
    if (n < 1 || T < 1 || K < 0 || K > QTL_MAXK || H < 1 || H > QTLVC_MAXH) return false;
    std::vector<uint8_t> mask(n);
    if (qtlhap_mask(n, c, col, H, mask.data()) >= 0) return false;
    const int nx = K + 1, ld = qtlvc_ld(H);
    int       n_c = 0;
    for (int i = 0; i < n; i++) n_c += mask[i];
    *n_used = n_c;
    const int nu = n_c - 1 - K;
    auto x0 = [&](int i, int k) { return k == 0 ? 1.0 : cov[(size_t)i * K + (k - 1)]; };
    double S11[QTL_NX * QTL_NX] = {0.0};
    for (int j = 0; j < nx; j++)
        for (int k = 0; k <= j; k++) {
            double s = 0.0;
            for (int i = 0; i < n; i++)
                if (mask[i]) s += x0(i, j) * x0(i, k);
            S11[j * QTL_NX + k] = s;
        }
    const bool usable = qtl_cholesky(S11, nx) && n_c >= K + 4;
    // the design: S22, S21 over the individuals in ascending order, G, W, its decomposition and the tables
    std::vector<double> W((size_t)H * ld, 0.0), S21((size_t)H * QTL_NX, 0.0), G((size_t)H * QTL_NX, 0.0), z(H), Qt((size_t)H * H, 0.0);
    std::vector<double> d(H, 0.0), E(QTLVC_GRID, 1.0), gtab((size_t)QTLVC_GRID * H, 0.0);
    for (int i = 0; i < n; i++) {
        if (!mask[i]) continue;
        for (int h = 0; h < H; h++) z[h] = qtlhap_z(descent + (size_t)i * 8, col + (size_t)i * 8, h);
        for (int j = 0; j < H; j++) {
            for (int k = 0; k < H; k++) W[(size_t)j * ld + k] += z[j] * z[k];
            for (int k = 0; k < nx; k++) S21[(size_t)j * QTL_NX + k] += z[j] * x0(i, k);
        }
    }
    int rank = 0;
    if (usable) {
        for (int h = 0; h < H; h++) {
            double g[QTL_NX] = {0.0};
            for (int k = 0; k < nx; k++) g[k] = S21[(size_t)h * QTL_NX + k];
            qtl_chol_solve(S11, nx, g);
            for (int k = 0; k < nx; k++) G[(size_t)h * QTL_NX + k] = g[k];
        }
        for (int j = 0; j < H; j++)
            for (int k = 0; k <= j; k++) {
                double s = 0.0;
                for (int kk = 0; kk < nx; kk++) s += G[(size_t)j * QTL_NX + kk] * S21[(size_t)k * QTL_NX + kk];
                W[(size_t)j * ld + k] -= s;
                W[(size_t)k * ld + j] = W[(size_t)j * ld + k];
            }
        std::vector<double> Qraw((size_t)H * H), draw(H);
        if (qtlvc_jacobi_serial(W.data(), ld, Qraw.data(), H)) {
            for (int k = 0; k < H; k++) draw[k] = W[(size_t)k * ld + k] > 0.0 ? W[(size_t)k * ld + k] : 0.0;
            for (int k = 0; k < H; k++) {
                const int pos = qtlvc_position(draw.data(), H, k);
                d[pos]        = draw[k];
                for (int h = 0; h < H; h++) Qt[(size_t)pos * H + h] = Qraw[(size_t)k * H + h];
            }
            rank = qtlvc_rank(d.data(), H);
            if (nu >= 2)
                for (int j = 0; j < QTLVC_GRID; j++) E[j] = qtlvc_grid_tables(d.data(), H, rank, nu, j, &gtab[(size_t)j * H]);
        }
        else
            rank = -1;
    }
    *rank_out = rank;
    if (eval)
        for (int k = 0; k < H; k++) eval[k] = d[k];
    const bool ok = usable && rank > 0 && nu >= 2;
    QtlHapLayout lay;
    qtlhap_layout(n, mask.data(), col, &lay);
    for (int tr = 0; tr < T; tr++) {
        double b0[QTL_NX] = {0.0}, s0[QTL_NX] = {0.0}, yy = 0.0, e0 = 0.0;
        for (int i = 0; i < n; i++) {
            if (!mask[i]) continue;
            const double v = y[(size_t)i * T + tr];
            for (int k = 0; k < nx; k++) b0[k] += x0(i, k) * v;
            yy += v * v;
        }
        if (usable) {
            for (int k = 0; k < nx; k++) s0[k] = b0[k];
            qtl_chol_solve(S11, nx, s0);
            for (int k = 0; k < nx; k++) e0 += b0[k] * s0[k];
        }
        rss0[tr] = usable ? yy - e0 : 0.0;
        std::vector<double> v(H, 0.0), t(H, 0.0);
        double              part[8] = {0.0};
        for (size_t s = 0; s < lay.steppat.size(); s++) {
            for (int j = 0; j < 4; j++) {
                const int32_t i = lay.gidx[4 * s + j];
                if (i < 0) continue;
                for (int k = 0; k < 8; k++) part[k] += descent[(size_t)i * 8 + k] * y[(size_t)i * T + tr];
            }
            if (lay.stepend[s])
                for (int k = 0; k < 8; k++) {
                    v[lay.patcol[(size_t)lay.steppat[s] * 8 + k]] += part[k];
                    part[k] = 0.0;
                }
        }
        for (int h = 0; h < H; h++)
            for (int k = 0; k < nx; k++) v[h] -= G[(size_t)h * QTL_NX + k] * b0[k];
        if (ok)
            for (int k = 0; k < rank; k++) {
                double s = 0.0;
                for (int h = 0; h < H; h++) s += Qt[(size_t)k * H + h] * v[h];
                t[k] = s;
            }
        const QtlVcCell r = qtlvc_cell(d.data(), E.data(), gtab.data(), H, rank, t.data(), 1, rss0[tr], nu, ok);
        lod[tr] = r.lod, h_out[tr] = r.h, sigma2[tr] = r.sigma2;
        if (blup)
            for (int h = 0; h < H; h++) {
                double s = 0.0;
                if (r.lod > 0.0)
                    for (int k = 0; k < rank; k++) s += Qt[(size_t)k * H + h] * (r.g / (1.0 + r.g * d[k]) * t[k]);
                blup[(size_t)tr * H + h] = s;
            }
    }
    return true;
}

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlvc_kernels.hip read and write (device pointers).  The column image, the null quantities and
// the maxima of the permuted columns are cnf2_qtl_kernels.hip's (QtlParams: qtl_gather_kernel, qtl_null_kernel,
// qtl_finish_kernel), on tiles of two markers.
struct QtlVcParams {
    QtlParams      q;              // as in QtlHapParams
    int            H, S;           // model columns; slots of the gather list (a multiple of 4)
    const double*  descent;        // [n][M][8]
    const int32_t* col;            // [n][8]
    const int32_t* gidx;           // [S]
    const int32_t* steppat;        // [S / 4]
    const int32_t* stepend;        // [S / 4]
    const int32_t* patcol;         // [patterns][8]
    double*        rec;            // [M][qtlvc_rec_size(H, nx)]
    int32_t*       rank;           // [M]
    double *       h, *sigma2;     // [T][M]
    double*        blup;           // [T][M][H] or null
    double*        eval;           // [M][H] or null
};
void launch_qtlvc_chrom(const QtlVcParams& p, hipStream_t stream);
bool launch_qtlvc_design(const QtlVcParams& p, hipStream_t stream);      // false: the dynamic LDS was refused
bool launch_qtlvc_scan(const QtlVcParams& p, hipStream_t stream);
#endif

} // namespace cnf2
#endif
