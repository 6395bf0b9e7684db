// cnf2_qtlem.h -- the maximum-likelihood single-locus scan (cnf2_qtl_scan_em, include/cnf2hip.h), shared by host and device
// code: the rank rule on the prior means, one individual's E-step terms, the M-step by the Schur complement on the fixed
// factor of X0'X0, and the stopping rule.  The kernels of cnf2_qtlem_kernels.hip (and qtlem_fit_serial below, on the CPU) form
// the sums over the individuals; every decision that gives the result its meaning is taken here.
//
// Interval mapping (Lander and Botstein): under the mask c of a chromosome, with the classes g = 0 .. 3 = AA, BA, AB, BB of the
// marker's origin row o and the priors pi_g = o_g / sum_g o_g,
//   y_i | g ~ N(x0_i' gamma + e(g)' beta, sigma^2),   l(theta) = sum_i c_i log sum_g pi_ig phi(y_i; mu_ig, sigma^2)
// with the effect codes a = (-1, 0, 0, 1), d = (0, 1, 1, 0) (not with CNF2_QTL_ADDITIVE), i = (0, 1, -1, 0) (only with
// CNF2_QTL_IMPRINT), in that order.  A class with pi = 0 has weight 0 and never enters a logarithm; an individual whose row at
// the marker has no positive sum takes no part there.
//   rank rule  the prior means sum_g pi_g e(g) are factored against X0 in the order a, d, i; an effect is dropped (beta = 0
//              throughout, coefficient NaN) when its raw diagonal is 0 or its pivot is below QTL_PIVOT times the diagonal.
//              That is Haley-Knott's rule: a marker whose rows carry no linkage information is not fitted.
//   start      theta_0 = the null fit (gamma = S11^-1 b0, beta = 0, sigma^2 = RSS0 / n_c), so l(theta_0) = l0 =
//              -(n_c / 2)(log(2 pi RSS0 / n_c) + 1).  The start is fixed and a fit deterministic; EM may stop at a local maximum
//              of the likelihood, which belongs to the method.
//   pass       one walk over the individuals with theta_t gives l_t = l(theta_t) and, from the weights
//              w_g ~ pi_g exp(-(y - mu_g)^2 / (2 sigma^2)), the sums S21 = sum e_bar x0', S22 = sum E_w[e e'], r = sum e_bar y.
//   M-step     G = L^-1 S21', W = S22 - G'G, v = r - G'z0 (z0 = L^-1 b0): beta = W^-1 v, RSS = RSS0 - v'W^-1 v,
//              sigma^2 = RSS / n_c, gamma = L'^-1 (z0 - G beta).  A kept pivot of W that is not positive, or a sigma^2 that is
//              not positive and finite, is a breakdown (status 2): the last complete iterate is reported.
//   stop       after iteration t when (l_t - l_{t-1}) / ln 10 < tol (status 0) or t = max_iter (status 1).
// Every loop over the columns of X0 or the effects has a constant bound and a predicate, so that the device code keeps its
// vectors in registers.
#ifndef CNF2_QTLEM_H
#define CNF2_QTLEM_H

#include "cnf2_qtl.h"
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

namespace cnf2 {

constexpr int    QTLEM_NE       = 3;         // effects at most: a, d, i
constexpr int    QTLEM_MAX_ITER = 10000;
constexpr double QTLEM_LN10     = 2.302585092994045684;
constexpr double QTLEM_2PI      = 6.283185307179586477;

// the design: which effect sits at which place (QTLEM_A .. QTLEM_I), and how many there are
constexpr int QTLEM_A = 0, QTLEM_D = 1, QTLEM_I = 2;
struct QtlemDesign {
    int nx, ne, w;
    int eff[QTLEM_NE];      // the code at place e < ne
};
CNF2_HD QtlemDesign qtlem_design(int K, bool additive, bool imprint)
{
    QtlemDesign ds;
    ds.nx     = K + 1;
    ds.ne     = 1 + (additive ? 0 : 1) + (imprint ? 1 : 0);
    ds.eff[0] = QTLEM_A;
    ds.eff[1] = additive ? QTLEM_I : QTLEM_D;
    ds.eff[2] = QTLEM_I;
    ds.w      = ds.nx + ds.ne;
    return ds;
}

// the sums of one pass (or, for the rank rule, of the prior means), indexed by effect code, not by place
struct QtlemSums {
    double s21[QTLEM_NE][QTL_NX];    // sum e_bar x0'
    double saa, sdd, sii, sdi;       // S22: E[a d] = E[a i] = 0 in a pass; the rank rule has its own sad, sai
    double sad, sai;
    double r[QTLEM_NE];              // sum e_bar y
    double ll;                       // sum of the individuals' log-likelihood terms
};
CNF2_HD void qtlem_zero(QtlemSums& s)
{
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLEM_NE; e++) {
CNF2_QTL_UNROLL
        for (int k = 0; k < QTL_NX; k++) s.s21[e][k] = 0.0;
        s.r[e] = 0.0;
    }
    s.saa = s.sdd = s.sii = s.sdi = s.sad = s.sai = s.ll = 0.0;
}

// pi[4] of an origin row; false when the row has no positive sum
CNF2_HD bool qtlem_prior(double o0, double o1, double o2, double o3, double pi[4])
{
    const double t = (o0 + o1) + (o2 + o3);
    if (!(t > 0.0)) return false;
    pi[0] = o0 / t, pi[1] = o1 / t, pi[2] = o2 / t, pi[3] = o3 / t;
    return true;
}

// one individual's share of the rank rule's sums: the prior means as Haley-Knott columns
CNF2_HD void qtlem_prior_terms(QtlemSums& s, const double pi[4], const double x[QTL_NX], int nx)
{
    const double a = pi[3] - pi[0], d = pi[1] + pi[2], i = pi[1] - pi[2];
CNF2_QTL_UNROLL
    for (int k = 0; k < QTL_NX; k++)
        if (k < nx) {
            s.s21[QTLEM_A][k] += a * x[k];
            s.s21[QTLEM_D][k] += d * x[k];
            s.s21[QTLEM_I][k] += i * x[k];
        }
    s.saa += a * a, s.sdd += d * d, s.sii += i * i;
    s.sad += a * d, s.sai += a * i, s.sdi += d * i;
}

// S22 of the effect codes (e, f)
CNF2_HD double qtlem_s22(const QtlemSums& s, int e, int f)
{
    const int lo = e < f ? e : f, hi = e < f ? f : e;
    if (lo == QTLEM_A) return hi == QTLEM_A ? s.saa : (hi == QTLEM_D ? s.sad : s.sai);
    if (lo == QTLEM_D) return hi == QTLEM_D ? s.sdd : s.sdi;
    return s.sii;
}

// The Schur block of the kept effects against X0 and its sequential Cholesky factor.  L: the factor of S11 (stride QTL_NX).
// g[e] <- L^-1 s21[e] for every effect place e < ne with keep[e] (on entry: every effect that may be kept).
// decide = true (the rank rule): keep[e] is cleared where the raw diagonal is 0 or the pivot below QTL_PIVOT times it.
// decide = false (an M-step): a kept pivot that is not positive returns false.
// c[e][f] (f <= e) holds the factor of W over the kept places.
CNF2_HD bool qtlem_schur(const double* L, const QtlemDesign& ds, const QtlemSums& s, bool keep[QTLEM_NE],
                         double g[QTLEM_NE][QTL_NX], double c[QTLEM_NE][QTLEM_NE], bool decide)
{
    bool ok = true;
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLEM_NE; e++) {
        const int ce = ds.eff[e];
CNF2_QTL_UNROLL
        for (int j = 0; j < QTL_NX; j++) {
            double v = 0.0;
            if (e < ds.ne && keep[e] && j < ds.nx) {
                v = s.s21[ce][j];
CNF2_QTL_UNROLL
                for (int k = 0; k < QTL_NX; k++)
                    if (k < j) v -= L[j * QTL_NX + k] * g[e][k];
                v /= L[j * QTL_NX + j];
            }
            g[e][j] = v;
        }
CNF2_QTL_UNROLL
        for (int f = 0; f < QTLEM_NE; f++) c[e][f] = 0.0;
        if (!(e < ds.ne && keep[e])) {
            keep[e] = false;
            continue;
        }
        // row e of the factor: against X0, then against the kept places before e
        const double raw = qtlem_s22(s, ce, ce);
        double       d   = raw;
CNF2_QTL_UNROLL
        for (int k = 0; k < QTL_NX; k++) d -= g[e][k] * g[e][k];
CNF2_QTL_UNROLL
        for (int f = 0; f < QTLEM_NE; f++)
            if (f < e && keep[f]) {
                double w = qtlem_s22(s, ce, ds.eff[f]);
CNF2_QTL_UNROLL
                for (int k = 0; k < QTL_NX; k++) w -= g[e][k] * g[f][k];
CNF2_QTL_UNROLL
                for (int h = 0; h < QTLEM_NE; h++)
                    if (h < f && keep[h]) w -= c[e][h] * c[f][h];
                c[e][f] = w / c[f][f];
                d -= c[e][f] * c[e][f];
            }
        if (decide) {
            if (!(raw > 0.0 && d >= QTL_PIVOT * raw)) {
                keep[e] = false;
CNF2_QTL_UNROLL
                for (int f = 0; f < QTLEM_NE; f++) c[e][f] = 0.0;
                continue;
            }
        } else if (!(d > 0.0)) {
            ok = false;
            d  = 1.0;
        }
        c[e][e] = sqrt(d);
    }
    return ok;
}

// the rank rule: keep[e] per effect place from the sums of the prior means; the number of kept effects is returned.
// usable: the chromosome is scanned (qtlem_usable).
CNF2_HD int qtlem_rank(const double* L, const QtlemDesign& ds, bool usable, const QtlemSums& prior, bool keep[QTLEM_NE])
{
    double g[QTLEM_NE][QTL_NX], c[QTLEM_NE][QTLEM_NE];
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLEM_NE; e++) keep[e] = usable && e < ds.ne;
    if (!usable) return 0;
    qtlem_schur(L, ds, prior, keep, g, c, true);
    return (keep[0] ? 1 : 0) + (keep[1] ? 1 : 0) + (keep[2] ? 1 : 0);
}

// A chromosome is scanned when X0 has a Cholesky factor, the null fit of cnf2_qtl_scan exists (n_c >= K + 4: has_null is the
// flag qtl_chrom_kernel leaves behind its factor) and n_c >= W + 1.
CNF2_HD bool qtlem_usable(bool has_null, int n_c, const QtlemDesign& ds) { return has_null && n_c >= ds.w + 1; }

// the iterate of one fit
struct QtlemTheta {
    double gamma[QTL_NX], beta[QTLEM_NE], sigma2;      // beta by effect place
};

struct QtlemFit {
    QtlemTheta th;          // theta_t
    double     z0[QTL_NX];  // L^-1 b0
    double     rss0, ll0;   // of the null fit
    double     ll, ll_prev; // l_t once known, l_{t-1}
    int        n_c, iters, status, done;
};

// theta_0 and l0 from b0 = X0'y and RSS0 > 0
CNF2_HD void qtlem_start(QtlemFit& f, const double* L, int nx, const double b0[QTL_NX], double rss0, int n_c)
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_NX; j++) {
        double v = 0.0;
        if (j < nx) {
            v = b0[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTL_NX; k++)
                if (k < j) v -= L[j * QTL_NX + k] * f.z0[k];
            v /= L[j * QTL_NX + j];
        }
        f.z0[j] = v;
    }
CNF2_QTL_UNROLL
    for (int jj = 0; jj < QTL_NX; jj++) {
        const int j = QTL_NX - 1 - jj;
        double    v = 0.0;
        if (j < nx) {
            v = f.z0[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTL_NX; k++)
                if (k > j && k < nx) v -= L[k * QTL_NX + j] * f.th.gamma[k];
            v /= L[j * QTL_NX + j];
        }
        f.th.gamma[j] = v;
    }
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLEM_NE; e++) f.th.beta[e] = 0.0;
    f.th.sigma2 = rss0 / (double)n_c;
    f.rss0      = rss0;
    f.n_c       = n_c;
    f.ll0       = -0.5 * (double)n_c * (log(QTLEM_2PI * rss0 / (double)n_c) + 1.0);
    f.ll = f.ll_prev = f.ll0;
    f.iters = f.status = f.done = 0;
}

// One individual's terms of a pass at theta: its log-likelihood term and, from its weights, its share of S21, S22 and r.
// four: the imprinting effect is kept, so BA and AB have means of their own; otherwise they share one exponential.
// The largest exponent is taken out, so that a residual of many sigma gives a finite term.
CNF2_HD void qtlem_terms(QtlemSums& s, const QtlemDesign& ds, const bool keep[QTLEM_NE], const QtlemTheta& th, const double pi[4],
                         const double x[QTL_NX], double y)
{
    double mu0 = 0.0;
CNF2_QTL_UNROLL
    for (int k = 0; k < QTL_NX; k++)
        if (k < ds.nx) mu0 += x[k] * th.gamma[k];
    double ba = 0.0, bd = 0.0, bi = 0.0;
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLEM_NE; e++)
        if (e < ds.ne && keep[e]) {
            const int ce = ds.eff[e];
            ba += ce == QTLEM_A ? th.beta[e] : 0.0;
            bd += ce == QTLEM_D ? th.beta[e] : 0.0;
            bi += ce == QTLEM_I ? th.beta[e] : 0.0;
        }
    const bool   four = ds.eff[ds.ne - 1] == QTLEM_I && keep[ds.ne - 1];
    const double h = -0.5 / th.sigma2, res = y - mu0;
    const double r0 = res + ba, r3 = res - ba, r1 = res - bd - bi, r2 = res - bd + bi;
    const double t0 = h * r0 * r0, t3 = h * r3 * r3, t1 = h * r1 * r1, t2 = h * r2 * r2;
    const double p12 = pi[1] + pi[2];
    const double ninf = -INFINITY;
    double       m = ninf;
    m = pi[0] > 0.0 && t0 > m ? t0 : m;
    m = pi[3] > 0.0 && t3 > m ? t3 : m;
    if (four) {
        m = pi[1] > 0.0 && t1 > m ? t1 : m;
        m = pi[2] > 0.0 && t2 > m ? t2 : m;
    } else
        m = p12 > 0.0 && t1 > m ? t1 : m;
    double u0 = pi[0] > 0.0 ? pi[0] * exp(t0 - m) : 0.0;
    double u3 = pi[3] > 0.0 ? pi[3] * exp(t3 - m) : 0.0;
    double u1, u2;
    if (four) {
        u1 = pi[1] > 0.0 ? pi[1] * exp(t1 - m) : 0.0;
        u2 = pi[2] > 0.0 ? pi[2] * exp(t2 - m) : 0.0;
    } else {
        u1 = p12 > 0.0 ? p12 * exp(t1 - m) : 0.0;      // BA and AB together
        u2 = 0.0;
    }
    const double tot = (u0 + (u1 + u2)) + u3;
    s.ll += log(tot) + m;
    const double inv = 1.0 / tot;
    u0 *= inv, u1 *= inv, u2 *= inv, u3 *= inv;
    const double ea = u3 - u0, ed = u1 + u2, ei = u1 - u2;      // e_bar; ei is used only when four
CNF2_QTL_UNROLL
    for (int k = 0; k < QTL_NX; k++)
        if (k < ds.nx) {
            s.s21[QTLEM_A][k] += ea * x[k];
            s.s21[QTLEM_D][k] += ed * x[k];
            s.s21[QTLEM_I][k] += ei * x[k];
        }
    s.r[QTLEM_A] += ea * y, s.r[QTLEM_D] += ed * y, s.r[QTLEM_I] += ei * y;
    s.saa += u0 + u3;
    s.sdd += ed;
    s.sii += ed;
    s.sdi += ei;
}

// After a pass at theta_t (s.ll = the sum of its terms): l_t, the stopping rule, and unless the fit stops the M-step to
// theta_{t+1}.  Returns true when the fit is over; f.th, f.ll, f.iters and f.status are then what is reported.
CNF2_HD bool qtlem_step(QtlemFit& f, const double* L, const QtlemDesign& ds, const bool keep[QTLEM_NE], const QtlemSums& s,
                        int max_iter, double tol)
{
    // (l_0 is the closed form: the pass at theta_0 gives the same value up to rounding)
    const double ll = f.iters == 0 ? f.ll0 : s.ll - 0.5 * (double)f.n_c * log(QTLEM_2PI * f.th.sigma2);
    f.ll = ll;
    if (f.iters >= 1) {
        if ((ll - f.ll_prev) / QTLEM_LN10 < tol) {
            f.status = 0;
            return true;
        }
        if (f.iters >= max_iter) {
            f.status = 1;
            return true;
        }
    }
    bool   kk[QTLEM_NE];
    double g[QTLEM_NE][QTL_NX], c[QTLEM_NE][QTLEM_NE], v[QTLEM_NE], beta[QTLEM_NE];
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLEM_NE; e++) kk[e] = keep[e];
    bool   ok = qtlem_schur(L, ds, s, kk, g, c, false);
    double drss = 0.0;
    // c u = v forwards, then c' beta = u backwards, over the kept places
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLEM_NE; e++) {
        double w = 0.0;
        if (kk[e]) {
            w = s.r[ds.eff[e]];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTL_NX; k++) w -= g[e][k] * f.z0[k];
CNF2_QTL_UNROLL
            for (int h = 0; h < QTLEM_NE; h++)
                if (h < e && kk[h]) w -= c[e][h] * v[h];
            w /= c[e][e];
        }
        v[e] = w;
        drss += w * w;
    }
CNF2_QTL_UNROLL
    for (int ee = 0; ee < QTLEM_NE; ee++) {
        const int e = QTLEM_NE - 1 - ee;
        double    w = 0.0;
        if (kk[e]) {
            w = v[e];
CNF2_QTL_UNROLL
            for (int h = 0; h < QTLEM_NE; h++)
                if (h > e && kk[h]) w -= c[h][e] * beta[h];
            w /= c[e][e];
        }
        beta[e] = w;
    }
    const double sigma2 = (f.rss0 - drss) / (double)f.n_c;
    ok = ok && sigma2 > 0.0 && sigma2 <= 1.79769313486231570815e308;
    if (!ok) {
        f.status = 2;
        return true;
    }
    // gamma = L'^-1 (z0 - G beta)
    double z[QTL_NX];
CNF2_QTL_UNROLL
    for (int k = 0; k < QTL_NX; k++) {
        z[k] = f.z0[k];
CNF2_QTL_UNROLL
        for (int e = 0; e < QTLEM_NE; e++) z[k] -= g[e][k] * beta[e];
    }
CNF2_QTL_UNROLL
    for (int jj = 0; jj < QTL_NX; jj++) {
        const int j = QTL_NX - 1 - jj;
        double    w = 0.0;
        if (j < ds.nx) {
            w = z[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTL_NX; k++)
                if (k > j && k < ds.nx) w -= L[k * QTL_NX + j] * f.th.gamma[k];
            w /= L[j * QTL_NX + j];
        }
        f.th.gamma[j] = w;
    }
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLEM_NE; e++) f.th.beta[e] = beta[e];
    f.th.sigma2 = sigma2;
    f.ll_prev   = ll;
    f.iters++;
    return false;
}

// what a finished fit reports
CNF2_HD double qtlem_lod(const QtlemFit& f)
{
    const double l = (f.ll - f.ll0) / QTLEM_LN10;
    return l > 0.0 ? l : 0.0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One (marker, column) fit on the CPU, the individuals in ascending order: o[n][4] the marker's origin rows, y[n], x0 the
// covariates cov[n][K], c[n] the chromosome's mask.  Mirrors what the kernels do with the functions above.
// As the scans do, it works on y and the covariates minus their means over the individuals of c (qtl_column_mean).
// Returns false for bad arguments.  Outputs: lod, coef[ne] (NaN where dropped or not fitted), sigma2, iters, status, rank,
// rss0 (0 for a chromosome that is not scanned), n_c.
inline bool qtlem_fit_serial(int n, const double* o, const double* y_raw, int K, const double* cov_raw, const uint8_t* c,
                             bool additive, bool imprint, int max_iter, double tol, double* lod, double* coef, double* sigma2,
                             int32_t* iters, int32_t* status, int32_t* rank, double* rss0_out, int32_t* nc_out)
{
    if (n < 1 || !o || !y_raw || K < 0 || K > QTL_MAXK || (K > 0 && !cov_raw) || !c) return false;
    if (max_iter < 1 || max_iter > QTLEM_MAX_ITER || !(tol - tol == 0.0)) return false;
    std::vector<double> y(y_raw, y_raw + n), cov(cov_raw, cov_raw + (K > 0 ? (size_t)n * K : 0));
    for (int k = -1; k < K; k++) {
        double*      col    = k < 0 ? y.data() : cov.data() + k;
        const int    stride = k < 0 ? 1 : K;
        const double mean   = qtl_column_mean(col, n, stride, c);
        for (int i = 0; i < n; i++)
            if (c[i]) col[(size_t)i * stride] -= mean;
    }
    const QtlemDesign ds = qtlem_design(K, additive, imprint);
    const int         nx = ds.nx;
    double S[QTL_NX * QTL_NX], b0[QTL_NX], x[QTL_NX], pi[4], yy = 0.0;
    for (int t = 0; t < QTL_NX * QTL_NX; t++) S[t] = 0.0;
    for (int k = 0; k < QTL_NX; k++) b0[k] = x[k] = 0.0;
    int n_c = 0;
    x[0]    = 1.0;
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        n_c++;
        for (int k = 1; k < nx; k++) x[k] = cov[(size_t)i * K + (k - 1)];
        for (int j = 0; j < nx; j++) {
            for (int k = 0; k <= j; k++) S[j * QTL_NX + k] += x[j] * x[k];
            b0[j] += x[j] * y[i];
        }
        yy += y[i] * y[i];
    }
    const bool has_null = qtl_cholesky(S, nx) && n_c >= K + 4;
    const bool usable   = qtlem_usable(has_null, n_c, ds);
    double     rss0     = 0.0;
    if (has_null) {
        double z[QTL_NX];
        for (int k = 0; k < QTL_NX; k++) z[k] = b0[k];
        qtl_chol_solve(S, nx, z);
        double e = 0.0;
        for (int k = 0; k < nx; k++) e += b0[k] * z[k];
        rss0 = yy - e;
    }
    QtlemSums s;
    qtlem_zero(s);
    if (usable)
        for (int i = 0; i < n; i++) {
            if (!c[i] || !qtlem_prior(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3], pi)) continue;
            for (int k = 1; k < nx; k++) x[k] = cov[(size_t)i * K + (k - 1)];
            qtlem_prior_terms(s, pi, x, nx);
        }
    bool keep[QTLEM_NE];
    *rank     = qtlem_rank(S, ds, usable, s, keep);
    *rss0_out = usable ? rss0 : 0.0;
    *nc_out   = n_c;
    *lod      = 0.0;
    *sigma2   = (double)NAN;
    *iters = *status = 0;
    for (int e = 0; e < ds.ne; e++) coef[e] = (double)NAN;
    if (!usable || !(rss0 > 0.0)) return true;
    QtlemFit f;
    qtlem_start(f, S, nx, b0, rss0, n_c);
    *sigma2 = f.th.sigma2;
    if (*rank == 0) return true;
    for (;;) {
        qtlem_zero(s);
        for (int i = 0; i < n; i++) {
            if (!c[i] || !qtlem_prior(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3], pi)) continue;
            for (int k = 1; k < nx; k++) x[k] = cov[(size_t)i * K + (k - 1)];
            qtlem_terms(s, ds, keep, f.th, pi, x, y[i]);
        }
        if (qtlem_step(f, S, ds, keep, s, max_iter, tol)) break;
    }
    *lod    = qtlem_lod(f);
    *sigma2 = f.th.sigma2;
    *iters  = f.iters;
    *status = f.status;
    for (int e = 0; e < ds.ne; e++) coef[e] = keep[e] ? f.th.beta[e] : (double)NAN;
    return true;
}
#endif

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlem_kernels.hip read and write (device pointers); the masks, the factor of S11, the column image
// and the null fit come from the kernels of cnf2_qtl_kernels.hip through a QtlParams of the same buffers.
struct QtlemParams {
    int n, M, C, T, P, K, additive, imprint, max_iter;
    double         tol;
    const double*  origin;       // [n][M][4]
    const double*  cov;          // [n][K]
    const int32_t* cs;           // [C + 1] chromstarts
    const int32_t* mchrom;       // [M] chromosome of a marker
    const uint8_t* cmask;        // [C][n]
    const int32_t* nc;           // [C]
    const double*  chol;         // [C][QTL_CHOL]
    int32_t*       keep;         // [M] bit e: the effect at place e is kept
    int            r0, rn, rstride;
    const double*  Y;            // [n][rstride] the column image
    const double*  nullq;        // [C][nx + 1][rstride]: b0, then RSS0
    const int32_t* tiles;        // [n_tiles][4] chromosome, first marker, markers (<= QTLEM_TILE), 0
    const int32_t* tile_start;   // [C + 1]
    int            n_tiles;
    double*        tilemax;      // [n_tiles][rstride]
    double *       lod, *coef, *sigma2, *pmax;
    double*        rss0;         // [T][C] RSS0 of the observed columns, 0 for a chromosome that is not scanned
    int32_t *      iters, *status, *rank;
};
constexpr int QTLEM_TILE = 4;    // markers per block of the fit kernel: one per wave, all of one chromosome
void launch_qtlem_rank(const QtlemParams& q, hipStream_t stream);
void launch_qtlem_fit(const QtlemParams& q, hipStream_t stream);
void launch_qtlem_finish(const QtlemParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
