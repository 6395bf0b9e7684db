// cnf2_qtlbin.h -- the binary-trait single-locus scan (cnf2_qtl_scan_binary, include/cnf2hip.h), shared by host and device
// code: the design, the rank rule on the unweighted columns, one individual's terms of a pass, the Newton step on the packed
// normal matrix and the stopping rule.  The kernels of cnf2_qtlbin_kernels.hip (and qtlbin_fit_serial below, on the CPU) form
// the sums over the individuals; every decision that gives the result its meaning is taken here.
//
// Logistic regression of a 0/1 trait on the origin rows: under the mask c of a chromosome, with the marker's origin row o,
//   x_i = [1, z_1 .. z_K, a, d, i],  a = o[3] - o[0],  d = o[1] + o[2] (not with CNF2_QTL_ADDITIVE),  i = o[1] - o[2] (only with
//   CNF2_QTL_IMPRINT),  eta_i = x_i' theta,  l(theta) = sum_i c_i [ y_i eta_i - softplus(eta_i) ]
// which is the design of cnf2_qtl_scanx's models 0 and 1 (cnf2_qtlx.h).  The columns sit at fixed places: X0 at 0 .. K, the
// effects at QTL_NX + e; a place that is not part of the fit (past K, a dropped effect) has x = 0 and is not active.
//   rank rule  the unweighted normal matrix X'X is factored in the order X0, a, d, i; X0 must have a factor (else the chromosome
//              is not scanned), an effect is dropped (beta = 0 throughout, coefficient NaN) when its raw diagonal is 0 or its
//              pivot is below QTL_PIVOT times the diagonal.  That is qtlx_factor's rule.
//   softplus   max(eta, 0) + log1p(exp(-|eta|)); p and w = p (1 - p) come from the same exponential e = exp(-|eta|):
//              p = 1 / (1 + e) or e / (1 + e), w = e / (1 + e)^2.  No intermediate overflows for any finite eta.
//   null fit   per chromosome and column, on X0 alone, from gamma = (logit(n_1 / n_c), 0, ..): QTLBIN_NULL_ITER iterations at
//              most, stopped by QTLBIN_NULL_TOL.  A column with n_1 = 0 or n_1 = n_c, or whose null fit does not stop by its
//              tolerance or breaks down, is not scanned on that chromosome.
//   fit        from theta_0 = (gamma0, 0), so l_0 = l0 by definition (the pass at theta_0 is not asked for its value).  A pass
//              at theta_t gives l_t, G = X'WX and s = X'(y - p) over the active places.
//   stop       after the pass at theta_t, t >= 1: (l_t - l_{t-1}) / ln 10 < tol stops the fit (status 0), else t = max_iter does
//              (status 1).  What is reported is theta_t and l_t.
//   step       otherwise G is Cholesky-factored; a pivot that is not positive, or a theta_{t+1} that is not finite, is a breakdown
//              (status 2: this is what separation ends in) and theta_t, l_t are reported.  Else theta_{t+1} = theta_t + G^-1 s.
//   no step-halving   from the null start Newton's method did not lose likelihood on any shape of the tests (n from 17 to 130,
//              K from 0 to 8, soft and certain rows); a decrease is simply a gain below tol and stops the fit by the rule above.
// Every loop over the places has a constant bound and a predicate, so that the device code keeps its vectors in registers.
#ifndef CNF2_QTLBIN_H
#define CNF2_QTLBIN_H

#include "cnf2_qtlem.h"

namespace cnf2 {

constexpr int    QTLBIN_NE        = QTLEM_NE;              // effects at most: a, d, i
constexpr int    QTLBIN_W         = QTL_NX + QTLBIN_NE;    // places: X0 at 0 .. QTL_NX - 1, effect place e at QTL_NX + e
constexpr int    QTLBIN_TRI       = QTLBIN_W * (QTLBIN_W + 1) / 2;
constexpr int    QTLBIN_MAX_ITER  = 1000;
constexpr int    QTLBIN_NULL_ITER = 50;
constexpr double QTLBIN_NULL_TOL  = 1e-13;                 // LOD
constexpr double QTLBIN_DBL_MAX   = 1.79769313486231570815e308;

// the packed lower triangle: (j, k), k <= j
CNF2_HD constexpr int qtlbin_at(int j, int k) { return j * (j + 1) / 2 + k; }

// the sums of one pass: G = X'WX (or X'X for the rank rule), s = X'(y - p), the log-likelihood
struct QtlbinSums {
    double G[QTLBIN_TRI], s[QTLBIN_W], ll;
};
CNF2_HD void qtlbin_zero(QtlbinSums& u)
{
CNF2_QTL_UNROLL
    for (int t = 0; t < QTLBIN_TRI; t++) u.G[t] = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) u.s[j] = 0.0;
    u.ll = 0.0;
}

// which places take part: X0's columns, and the effect places with keep[e]
CNF2_HD void qtlbin_active(const QtlemDesign& ds, const bool keep[QTLBIN_NE], bool act[QTLBIN_W])
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_NX; j++) act[j] = j < ds.nx;
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLBIN_NE; e++) act[QTL_NX + e] = e < ds.ne && keep[e];
}

// x of one individual: x0[QTL_NX] is its row of X0 (zero past the design's columns), o its origin row at the marker; an
// effect place that is not active gets 0
CNF2_HD void qtlbin_row(const QtlemDesign& ds, const bool act[QTLBIN_W], const double x0[QTL_NX], double o0, double o1, double o2,
                        double o3, double x[QTLBIN_W])
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_NX; j++) x[j] = act[j] ? x0[j] : 0.0;
    const double a = o3 - o0, d = o1 + o2, i = o1 - o2;
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLBIN_NE; e++) {
        const int    ce = ds.eff[e];
        const double v  = ce == QTLEM_A ? a : (ce == QTLEM_D ? d : i);
        x[QTL_NX + e]   = act[QTL_NX + e] ? v : 0.0;
    }
}

// one individual's share of the unweighted normal matrix (the rank rule)
CNF2_HD void qtlbin_raw_terms(QtlbinSums& u, const bool act[QTLBIN_W], const double x[QTLBIN_W])
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) {
CNF2_QTL_UNROLL
            for (int k = 0; k < QTLBIN_W; k++)
                if (k <= j && act[k]) u.G[qtlbin_at(j, k)] += x[j] * x[k];
        }
}

// One individual's terms of a pass at theta: its log-likelihood term and its share of G and s.  y is 0 or 1.
CNF2_HD void qtlbin_terms(QtlbinSums& u, const bool act[QTLBIN_W], const double th[QTLBIN_W], const double x[QTLBIN_W], double y)
{
    double eta = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) eta += x[j] * th[j];
    const double e = exp(-fabs(eta)), q = 1.0 + e;
    u.ll += y * eta - ((eta > 0.0 ? eta : 0.0) + log1p(e));
    const double p = (eta >= 0.0 ? 1.0 : e) / q, w = e / (q * q), r = y - p;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) {
            const double wx = w * x[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTLBIN_W; k++)
                if (k <= j && act[k]) u.G[qtlbin_at(j, k)] += wx * x[k];
            u.s[j] += r * x[j];
        }
}

// G <- its sequential Cholesky factor over the active places, in place on the packed triangle.
// decide = true (the rank rule): a column of X0 whose pivot is not positive returns false (the chromosome is not scanned); an
// effect place is dropped (act cleared) when its raw diagonal is 0 or its pivot is below QTL_PIVOT times it.
// decide = false (a Newton step): an active pivot that is not positive returns false.
CNF2_HD bool qtlbin_factor(double G[QTLBIN_TRI], bool act[QTLBIN_W], bool decide)
{
    bool ok = true;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) {
        const double raw = G[qtlbin_at(j, j)];
        double       d   = raw;
CNF2_QTL_UNROLL
        for (int k = 0; k < QTLBIN_W; k++)
            if (k < j && act[k]) d -= G[qtlbin_at(j, k)] * G[qtlbin_at(j, k)];
        if (act[j]) {
            if (decide && j >= QTL_NX) {
                if (!(raw > 0.0 && d >= QTL_PIVOT * raw)) act[j] = false;
            } else if (!(d > 0.0))
                ok = false;
        }
        // (a pivot that ends the factorisation still gets a finite root: nothing below is reported then)
        d = act[j] && d > 0.0 ? sqrt(d) : 1.0;
        G[qtlbin_at(j, j)] = d;
CNF2_QTL_UNROLL
        for (int i = 0; i < QTLBIN_W; i++)
            if (i > j) {
                double v = G[qtlbin_at(i, j)];
CNF2_QTL_UNROLL
                for (int k = 0; k < QTLBIN_W; k++)
                    if (k < j && act[k]) v -= G[qtlbin_at(i, k)] * G[qtlbin_at(j, k)];
                G[qtlbin_at(i, j)] = act[j] ? v / d : 0.0;
            }
    }
    return ok;
}

// x <- (L L')^-1 x over the active places (0 elsewhere)
CNF2_HD void qtlbin_solve(const double L[QTLBIN_TRI], const bool act[QTLBIN_W], double x[QTLBIN_W])
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) {
        double v = x[j];
CNF2_QTL_UNROLL
        for (int k = 0; k < QTLBIN_W; k++)
            if (k < j && act[k]) v -= L[qtlbin_at(j, k)] * x[k];
        x[j] = act[j] ? v / L[qtlbin_at(j, j)] : 0.0;
    }
CNF2_QTL_UNROLL
    for (int jj = 0; jj < QTLBIN_W; jj++) {
        const int j = QTLBIN_W - 1 - jj;
        double    v = x[j];
CNF2_QTL_UNROLL
        for (int k = 0; k < QTLBIN_W; k++)
            if (k > j && act[k]) v -= L[qtlbin_at(k, j)] * x[k];
        x[j] = act[j] ? v / L[qtlbin_at(j, j)] : 0.0;
    }
}

// A chromosome is scanned when X0 has a Cholesky factor and n_c >= W + 1 (cnf2_qtl_scanx's rule).
// The rank rule on the sums of qtlbin_raw_terms over every place of the design: keep[e] per effect place and the number of
// kept effects (0 for a chromosome that is not scanned); *scanned says which.
CNF2_HD int qtlbin_rank(QtlbinSums& raw, const QtlemDesign& ds, int n_c, bool keep[QTLBIN_NE], bool* scanned)
{
    bool act[QTLBIN_W];
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLBIN_NE; e++) keep[e] = true;
    qtlbin_active(ds, keep, act);
    const bool ok = qtlbin_factor(raw.G, act, true) && n_c >= ds.w + 1;
    *scanned = ok;
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLBIN_NE; e++) keep[e] = ok && act[QTL_NX + e];
    return (keep[0] ? 1 : 0) + (keep[1] ? 1 : 0) + (keep[2] ? 1 : 0);
}

// the iterate of one fit (the null fit is a fit without effects)
struct QtlbinFit {
    double th[QTLBIN_W];     // theta_t by place
    double ll, ll_prev;      // l_t once known, l_{t-1}
    int    iters, status;
};

// theta_0 = (g0[0 .. nx), 0) with its log-likelihood ll0 where that is known (the fit; the null fit takes it from its pass)
CNF2_HD void qtlbin_start(QtlbinFit& f, const double g0[QTL_NX], int nx, double ll0)
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) f.th[j] = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_NX; j++)
        if (j < nx) f.th[j] = g0[j];
    f.ll = f.ll_prev = ll0;
    f.iters = f.status = 0;
}

// After a pass at theta_t (u.ll = the sum of its terms): l_t, the stopping rule, and unless the fit stops the Newton step to
// theta_{t+1}.  known0: l_0 is what qtlbin_start was given.  Returns true when the fit is over; f.th, f.ll, f.iters and f.status
// are then what is reported.  u.G is used up.
CNF2_HD bool qtlbin_step(QtlbinFit& f, const bool act_in[QTLBIN_W], QtlbinSums& u, int max_iter, double tol, bool known0)
{
    const double ll = (f.iters == 0 && known0) ? f.ll : u.ll;
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
    bool act[QTLBIN_W];
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) act[j] = act_in[j];
    bool ok = qtlbin_factor(u.G, act, false);
    qtlbin_solve(u.G, act, u.s);
    double th[QTLBIN_W];
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) {
        th[j] = act[j] ? f.th[j] + u.s[j] : 0.0;
        ok    = ok && th[j] - th[j] == 0.0 && fabs(th[j]) <= QTLBIN_DBL_MAX;
    }
    if (!ok) {
        f.status = 2;
        return true;
    }
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) f.th[j] = th[j];
    f.ll_prev = ll;
    f.iters++;
    return false;
}

// what a finished fit reports against the null fit's l0
CNF2_HD double qtlbin_lod(const QtlbinFit& f, double ll0)
{
    const double l = (f.ll - ll0) / QTLEM_LN10;
    return l > 0.0 ? l : 0.0;
}

// the null fit's start from n_1 of n_c; false when the trait is constant there
CNF2_HD bool qtlbin_null_start(QtlbinFit& f, int n_1, int n_c)
{
    double g0[QTL_NX];
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_NX; j++) g0[j] = 0.0;
    const bool both = n_1 > 0 && n_1 < n_c;
    if (both) g0[0] = log((double)n_1 / (double)(n_c - n_1));
    qtlbin_start(f, g0, 1, 0.0);
    return both;
}
// a finished null fit counts when it stopped by its tolerance
CNF2_HD bool qtlbin_null_ok(const QtlbinFit& f) { return f.status == 0 && f.iters >= 1 && f.ll < 0.0; }

#if !defined(__HIP_DEVICE_COMPILE__)
// One (marker, column) fit on the CPU, the individuals in ascending order: o[n][4] the marker's origin rows, y[n] (0 or 1 where
// c is set), the covariates cov[n][K], c[n] the chromosome's mask.  Mirrors what the kernels do with the functions above.
// As the scan does, it works on the covariates minus their means over the individuals of c, each difference rounded once
// (qtl_column_mean2, qtl_minus_mean2 of cnf2_qtl.h).
// Returns false for bad arguments.  Outputs: lod, coef[ne] (NaN where dropped or not fitted), iters, status, rank, ll0 (0 for
// a column that is not scanned), n_ones, n_c.
inline bool qtlbin_fit_serial(int n, const double* o, const double* y, int K, const double* cov_raw, const uint8_t* c, bool additive,
                              bool imprint, int max_iter, double tol, double* lod, double* coef, int32_t* iters, int32_t* status,
                              int32_t* rank, double* ll0_out, int32_t* n1_out, int32_t* nc_out)
{
    if (n < 1 || !o || !y || K < 0 || K > QTL_MAXK || (K > 0 && !cov_raw) || !c) return false;
    if (max_iter < 1 || max_iter > QTLBIN_MAX_ITER || !(tol - tol == 0.0)) return false;
    int n_c = 0, n_1 = 0;
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        if (!(y[i] == 0.0 || y[i] == 1.0)) return false;
        n_c++;
        n_1 += y[i] == 1.0 ? 1 : 0;
    }
    std::vector<double> cov(cov_raw, cov_raw + (K > 0 ? (size_t)n * K : 0));
    for (int k = 0; k < K; k++) {
        const QtlMean2 mean = qtl_column_mean2(cov.data() + k, n, K, c);
        for (int i = 0; i < n; i++)
            if (c[i]) cov[(size_t)i * K + k] = qtl_minus_mean2(cov[(size_t)i * K + k], mean);
    }
    const QtlemDesign ds = qtlem_design(K, additive, imprint);
    const int         nx = ds.nx;
    bool              keep[QTLBIN_NE] = {true, true, true}, act[QTLBIN_W], scanned = false;
    double            x0[QTL_NX], x[QTLBIN_W];
    for (int k = 0; k < QTL_NX; k++) x0[k] = 0.0;
    x0[0] = 1.0;
    auto row = [&](int i) {
        for (int k = 1; k < nx; k++) x0[k] = cov[(size_t)i * K + (k - 1)];
        qtlbin_row(ds, act, x0, o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3], x);
    };
    QtlbinSums u;
    qtlbin_zero(u);
    qtlbin_active(ds, keep, act);
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        row(i);
        qtlbin_raw_terms(u, act, x);
    }
    *rank    = qtlbin_rank(u, ds, n_c, keep, &scanned);
    *n1_out  = n_1;
    *nc_out  = n_c;
    *lod     = 0.0;
    *ll0_out = 0.0;
    *iters = *status = 0;
    for (int e = 0; e < ds.ne; e++) coef[e] = (double)NAN;
    if (!scanned) return true;
    // the null fit
    const bool none[QTLBIN_NE] = {false, false, false};
    QtlbinFit  f0;
    if (!qtlbin_null_start(f0, n_1, n_c)) return true;
    qtlbin_active(ds, none, act);
    for (;;) {
        qtlbin_zero(u);
        for (int i = 0; i < n; i++) {
            if (!c[i]) continue;
            row(i);
            qtlbin_terms(u, act, f0.th, x, y[i]);
        }
        if (qtlbin_step(f0, act, u, QTLBIN_NULL_ITER, QTLBIN_NULL_TOL, false)) break;
    }
    if (!qtlbin_null_ok(f0)) return true;
    *ll0_out = f0.ll;
    if (*rank == 0) return true;
    QtlbinFit f;
    qtlbin_start(f, f0.th, nx, f0.ll);
    qtlbin_active(ds, keep, act);
    for (;;) {
        qtlbin_zero(u);
        for (int i = 0; i < n; i++) {
            if (!c[i]) continue;
            row(i);
            qtlbin_terms(u, act, f.th, x, y[i]);
        }
        if (qtlbin_step(f, act, u, max_iter, tol, true)) break;
    }
    *lod    = qtlbin_lod(f, f0.ll);
    *iters  = f.iters;
    *status = f.status;
    for (int e = 0; e < ds.ne; e++) coef[e] = keep[e] ? f.th[QTL_NX + e] : (double)NAN;
    return true;
}
#endif

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlbin_kernels.hip read and write (device pointers); the masks and n_c come from qtl_chrom_kernel
// and the column image from qtl_gather_kernel of cnf2_qtl_kernels.hip through a QtlParams of the same buffers.  (That kernel
// also leaves cnf2_qtl_scan's factor of X0'X0 with cnf2_qtl_scan's own flag, which asks for n_c >= K + 4: this scan reads
// neither.  Whether a chromosome is scanned is qtlbin_rank's verdict alone, in `scan`.)
constexpr int QTLBIN_NULLQ = QTL_NX + 2;     // doubles per (chromosome, column) of the null fit: gamma0, l0, 1.0 = scanned
struct QtlbinParams {
    int n, M, C, T, P, K, additive, imprint, max_iter;
    double         tol;
    const double*  origin;       // [n][M][4]
    const double*  cov;          // [n][K]
    const int32_t* cs;           // [C + 1] chromstarts
    const int32_t* mchrom;       // [M] chromosome of a marker
    const uint8_t* cmask;        // [C][n]
    const int32_t* nc;           // [C]
    int32_t*       keep;         // [M] bit e: the effect at place e is kept
    int32_t*       scan;         // [C] 1: the chromosome is scanned.  The one place that says so: zeroed by the host, then
                                 // written by qtlbin_rank_kernel's thread of the chromosome's first marker (qtlbin_rank)
    int            r0, rn, rstride;
    const double*  Y;            // [n][rstride] the column image
    double*        nullq;        // [C][QTLBIN_NULLQ][rstride]
    const int32_t* tiles;        // [n_tiles][4] chromosome, first marker, markers (<= QTLBIN_TILE), 0
    const int32_t* tile_start;   // [C + 1]
    int            n_tiles;
    double*        tilemax;      // [n_tiles][rstride]
    double *       lod, *coef, *pmax;
    double*        ll0;          // [T][C] l0 of the observed columns, 0 where the column is not scanned
    int32_t*       n_ones;       // [T][C]
    int32_t *      iters, *status, *rank;
};
constexpr int QTLBIN_TILE = 4;   // markers per block of the fit kernel: one per wave, all of one chromosome
void launch_qtlbin_rank(const QtlbinParams& q, hipStream_t stream);
void launch_qtlbin_null(const QtlbinParams& q, hipStream_t stream);
void launch_qtlbin_fit(const QtlbinParams& q, hipStream_t stream);
void launch_qtlbin_finish(const QtlbinParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
