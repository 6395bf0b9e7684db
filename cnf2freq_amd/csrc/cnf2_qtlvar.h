// cnf2_qtlvar.h -- the variance-QTL single-locus scan (cnf2_qtl_scan_var, include/cnf2hip.h), shared by host and device code:
// the two designs, one individual's terms of each pass, the two solves of an iteration, the step-halving, the stopping rule
// and the three LODs.  The kernels of cnf2_qtlvar_kernels.hip (and qtlvar_fit_serial below, on the CPU) form the sums over the
// individuals; every decision that gives the result its meaning is taken here or in cnf2_qtlbin.h.
//
// The double generalised linear model of a quantitative trait on the origin rows: under the mask c of a chromosome, with the
// marker's origin row o,
//   x_i = [1, z_1 .. z_K, E]      mu_i  = x_i' beta
//   v_i = [1, z_1 .. z_nvar, E]   eta_i = v_i' gamma = log sigma_i^2          (n_var <= min(K, QTLVAR_MAXV))
//   E   = a, d, i as in cnf2_qtlbin.h
//   l(beta, gamma) = -1/2 sum_i c_i [ log 2pi + eta_i + (y_i - mu_i)^2 exp(-eta_i) ]
// Both designs sit at cnf2_qtlbin.h's places -- X0 at 0 .. K, the effects at QTL_NX + e -- and differ in which are active:
// V's columns are a subset of X's in the same order, so one row x serves both, and qtlbin_factor / qtlbin_solve serve as they are.
//   fits       null (X0, V0) per chromosome and column; per marker fit 0 mean-only (X0 + E, V0), fit 1 variance-only
//              (X0, V0 + E) and fit 2 full (X0 + E, V0 + E), each from (beta0, 0; gamma0, 0) with l_0 = l0.
//   LODs       lod[0] joint = l_full - l_null, lod[1] mean = l_full - l_variance-only, lod[2] variance = l_full - l_mean-only,
//              each over ln 10 and max(0, .).
//   iteration  from (beta_t, gamma_t, l_t):
//              1. w_i = exp(-v_i' gamma_t); beta_{t+1} = (X'WX)^-1 X'Wy by the Cholesky factor (the exact maximiser in beta)
//              2. r = y - X beta_{t+1}, q_i = w_i r_i^2; delta = (V' diag(q) V)^-1 V'(q - 1): Newton's step in gamma with the
//                 observed information, which is positive definite wherever it has a factor
//              3. gamma' = gamma_t + 2^-h delta for h = 0 .. QTLVAR_HALVINGS: the first h with
//                 (l_t - l(beta_{t+1}, gamma')) / ln 10 <= QTLVAR_LOSS is taken; gamma_{t+1} = gamma', l_{t+1} that value
//              4. (l_{t+1} - l_t) / ln 10 < tol stops the fit (status 0), else t + 1 = max_iter does (status 1)
//   breakdown  status 2, reporting (beta_t, gamma_t, l_t): a pivot of either factor that is not positive; a beta, gamma or l
//              that is not finite; an |eta_i| of a trial gamma' above QTLVAR_ETA_MAX; no h accepted.
//   rank rule  qtlbin_rank's on the mean design; an effect dropped there is dropped from V too (one keep mask per marker).  A
//              chromosome is scanned when X0 has a factor and n_c >= (1 + K + ne) + (1 + n_var + ne) + 1.
//   null fit   the same iteration on (X0, V0) from beta = 0, gamma = (log(sum c y^2 / n_c), 0, ..), whose
//              l_0 = -n_c / 2 (log 2pi + gamma_0 + 1): QTLVAR_NULL_ITER iterations at most, stopped by QTLVAR_NULL_TOL.  A column
//              that is constant on the chromosome, or whose null fit does not stop by its tolerance or breaks down, is not
//              scanned there.
// Every loop over the places has a constant bound and a predicate, so that the device code keeps its vectors in registers.
#ifndef CNF2_QTLVAR_H
#define CNF2_QTLVAR_H

#include "cnf2_qtlbin.h"

namespace cnf2 {

constexpr int    QTLVAR_MAXV      = 3;                     // variance covariates at most
constexpr int    QTLVAR_NV0       = QTLVAR_MAXV + 1;       // places of V0 at most
constexpr int    QTLVAR_NFIT      = 3;                     // fits, and LODs, per cell
constexpr int    QTLVAR_MAX_ITER  = QTLBIN_MAX_ITER;
constexpr int    QTLVAR_NULL_ITER = 50;
constexpr double QTLVAR_NULL_TOL  = 1e-13;                 // LOD
constexpr int    QTLVAR_HALVINGS  = 8;
constexpr double QTLVAR_LOSS      = 1e-9;                  // LOD a step may lose
constexpr double QTLVAR_ETA_MAX   = 700.0;

CNF2_HD bool qtlvar_finite(double v) { return v - v == 0.0 && fabs(v) <= QTLBIN_DBL_MAX; }

// the scan threshold on top of qtlbin_rank's
CNF2_HD int qtlvar_min_n(const QtlemDesign& ds, int n_var) { return ds.w + (1 + n_var + ds.ne) + 1; }

// which places take part in fit `which` (0 mean-only, 1 variance-only, 2 full; -1 the null fit): actx the mean design's,
// actv the variance design's
CNF2_HD void qtlvar_active(const QtlemDesign& ds, int n_var, const bool keep[QTLBIN_NE], int which, bool actx[QTLBIN_W],
                           bool actv[QTLBIN_W])
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_NX; j++) {
        actx[j] = j < ds.nx;
        actv[j] = j < QTLVAR_NV0 && j <= n_var;
    }
CNF2_QTL_UNROLL
    for (int e = 0; e < QTLBIN_NE; e++) {
        const bool k = e < ds.ne && keep[e];
        actx[QTL_NX + e] = k && (which == 0 || which == 2);
        actv[QTL_NX + e] = k && (which == 1 || which == 2);
    }
}

// the sums of the trial pass: sum_i [eta_i + r_i^2 exp(-eta_i)] and the largest |eta_i|
struct QtlvarTrial {
    double s, emax;
};

// eta_i = v_i' gamma (x holds every active place of either design)
CNF2_HD double qtlvar_eta(const bool actv[QTLBIN_W], const double ga[QTLBIN_W], const double x[QTLBIN_W])
{
    double eta = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (actv[j]) eta += x[j] * ga[j];
    return eta;
}
CNF2_HD double qtlvar_mu(const bool actx[QTLBIN_W], const double be[QTLBIN_W], const double x[QTLBIN_W])
{
    double mu = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (actx[j]) mu += x[j] * be[j];
    return mu;
}

// Step 1, one individual with w = exp(-eta_i): its share of G = X'WX and s = X'Wy
CNF2_HD void qtlvar_mean_terms(QtlbinSums& u, const bool actx[QTLBIN_W], const double x[QTLBIN_W], double w, double y)
{
    const double wy = w * y;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (actx[j]) {
            const double wx = w * x[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTLBIN_W; k++)
                if (k <= j && actx[k]) u.G[qtlbin_at(j, k)] += wx * x[k];
            u.s[j] += wy * x[j];
        }
}

// Step 2, one individual at (beta_{t+1}, gamma_t): q = w r^2, its share of G = V' diag(q) V and s = V'(q - 1)
CNF2_HD void qtlvar_var_terms(QtlbinSums& u, const bool actx[QTLBIN_W], const bool actv[QTLBIN_W], const double be[QTLBIN_W],
                              const double ga[QTLBIN_W], const double x[QTLBIN_W], double y)
{
    const double r = y - qtlvar_mu(actx, be, x), q = exp(-qtlvar_eta(actv, ga, x)) * r * r, q1 = q - 1.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (actv[j]) {
            const double qx = q * x[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTLBIN_W; k++)
                if (k <= j && actv[k]) u.G[qtlbin_at(j, k)] += qx * x[k];
            u.s[j] += q1 * x[j];
        }
}

// Step 3, one individual at (beta_{t+1}, gamma'): its term of l and its |eta|; returns w = exp(-eta), which is step 1's weight
// if gamma' is taken
CNF2_HD double qtlvar_trial_terms(QtlvarTrial& tr, const bool actx[QTLBIN_W], const bool actv[QTLBIN_W], const double be[QTLBIN_W],
                                  const double ga[QTLBIN_W], const double x[QTLBIN_W], double y)
{
    const double eta = qtlvar_eta(actv, ga, x), w = exp(-eta), r = y - qtlvar_mu(actx, be, x);
    tr.s += eta + r * r * w;
    tr.emax = fmax(tr.emax, fabs(eta));
    return w;
}
// l from the sum of those terms over the n_c individuals
CNF2_HD double qtlvar_ll(double s, int n_c) { return -0.5 * ((double)n_c * log(QTLEM_2PI) + s); }

// the iterate of one fit
struct QtlvarFit {
    double be[QTLBIN_W], ga[QTLBIN_W];   // beta_t, gamma_t by place
    double bn[QTLBIN_W];                 // beta_{t+1} of the iteration under way
    double de[QTLBIN_W], gt[QTLBIN_W];   // delta and the trial gamma' = gamma_t + 2^-h delta
    double ll;                           // l_t
    int    h, iters, status;
};

// (beta0[0 .. nx), 0; gamma0[0 .. n_var], 0) with l_0 = ll0
CNF2_HD void qtlvar_start(QtlvarFit& f, const double b0[QTL_NX], int nx, const double g0[QTLVAR_NV0], int n_var, double ll0)
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) f.be[j] = f.ga[j] = f.bn[j] = f.de[j] = f.gt[j] = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_NX; j++)
        if (j < nx) f.be[j] = b0[j];
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLVAR_NV0; j++)
        if (j <= n_var) f.ga[j] = f.gt[j] = g0[j];
    f.ll = ll0;
    f.h = f.iters = f.status = 0;
}

// After step 1's sums: beta_{t+1}.  False on a breakdown (the fit is over, status 2).  u is used up.
CNF2_HD bool qtlvar_beta(QtlvarFit& f, const bool actx[QTLBIN_W], QtlbinSums& u)
{
    bool act[QTLBIN_W];
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) act[j] = actx[j];
    bool ok = qtlbin_factor(u.G, act, false);
    qtlbin_solve(u.G, act, u.s);
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) {
        f.bn[j] = act[j] ? u.s[j] : 0.0;
        ok      = ok && qtlvar_finite(f.bn[j]);
    }
    if (!ok) f.status = 2;
    return ok;
}

// After step 2's sums: delta and the first trial gamma' (h = 0).  False on a breakdown.  u is used up.
CNF2_HD bool qtlvar_delta(QtlvarFit& f, const bool actv[QTLBIN_W], QtlbinSums& u)
{
    bool act[QTLBIN_W];
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) act[j] = actv[j];
    bool ok = qtlbin_factor(u.G, act, false);
    qtlbin_solve(u.G, act, u.s);
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) {
        f.de[j] = act[j] ? u.s[j] : 0.0;
        f.gt[j] = act[j] ? f.ga[j] + f.de[j] : 0.0;
        ok      = ok && qtlvar_finite(f.gt[j]);
    }
    f.h = 0;
    if (!ok) f.status = 2;
    return ok;
}

// After step 3's sums at gamma' (ll its l, emax its largest |eta|): what comes next
constexpr int QTLVAR_NEXT = 0, QTLVAR_OVER = 1, QTLVAR_HALVE = 2;
CNF2_HD int qtlvar_accept(QtlvarFit& f, const bool actv[QTLBIN_W], double ll, double emax, int max_iter, double tol)
{
    if (!qtlvar_finite(ll) || !(emax <= QTLVAR_ETA_MAX)) {
        f.status = 2;
        return QTLVAR_OVER;
    }
    if (!((f.ll - ll) / QTLEM_LN10 <= QTLVAR_LOSS)) {
        f.h++;
        if (f.h > QTLVAR_HALVINGS) {
            f.status = 2;
            return QTLVAR_OVER;
        }
        double sc = 1.0;
CNF2_QTL_UNROLL
        for (int k = 0; k < QTLVAR_HALVINGS; k++)
            if (k < f.h) sc *= 0.5;
CNF2_QTL_UNROLL
        for (int j = 0; j < QTLBIN_W; j++) f.gt[j] = actv[j] ? f.ga[j] + sc * f.de[j] : 0.0;
        return QTLVAR_HALVE;
    }
    const double gain = (ll - f.ll) / QTLEM_LN10;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) {
        f.be[j] = f.bn[j];
        f.ga[j] = f.gt[j];
    }
    f.ll = ll;
    f.iters++;
    if (gain < tol) {
        f.status = 0;
        return QTLVAR_OVER;
    }
    if (f.iters >= max_iter) {
        f.status = 1;
        return QTLVAR_OVER;
    }
    return QTLVAR_NEXT;
}

// the null fit's start from sum c y^2 and n_c (of a column that is not constant there)
CNF2_HD void qtlvar_null_start(QtlvarFit& f, double yy, int n_c)
{
    double b0[QTL_NX], g0[QTLVAR_NV0];
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_NX; j++) b0[j] = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLVAR_NV0; j++) g0[j] = 0.0;
    g0[0] = log(yy / (double)n_c);
    qtlvar_start(f, b0, 1, g0, 0, -0.5 * (double)n_c * (log(QTLEM_2PI) + g0[0] + 1.0));
}
// a finished null fit counts when it stopped by its tolerance
CNF2_HD bool qtlvar_null_ok(const QtlvarFit& f) { return f.status == 0 && f.iters >= 1 && qtlvar_finite(f.ll); }

// the three LODs from the three fits' l and the null fit's
CNF2_HD void qtlvar_lods(const double ll[QTLVAR_NFIT], double ll0, double lod[QTLVAR_NFIT])
{
    const double v[QTLVAR_NFIT] = {(ll[2] - ll0) / QTLEM_LN10, (ll[2] - ll[1]) / QTLEM_LN10, (ll[2] - ll[0]) / QTLEM_LN10};
CNF2_QTL_UNROLL
    for (int k = 0; k < QTLVAR_NFIT; k++) lod[k] = v[k] > 0.0 ? v[k] : 0.0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One (marker, column) cell on the CPU, the individuals in ascending order: o[n][4] the marker's origin rows, y[n], the
// covariates cov[n][K] of which the first n_var enter the variance design, c[n] the chromosome's mask.  Mirrors what the
// kernels do with the functions above, one pass per step.  As the scan does, it works on the trait and the covariates minus
// their means over the individuals of c, each difference rounded once.
// Returns false for bad arguments.  Outputs: lod[3], coef_mean[ne] and coef_var[ne] of the full fit (NaN where dropped or not
// fitted), iters[3] and status[3] by fit, rank, ll0 (0 for a column that is not scanned), n_c.
inline bool qtlvar_fit_serial(int n, const double* o, const double* y_raw, int K, const double* cov_raw, int n_var, const uint8_t* c,
                              bool additive, bool imprint, int max_iter, double tol, double* lod, double* coef_mean, double* coef_var,
                              int32_t* iters, int32_t* status, int32_t* rank, double* ll0_out, int32_t* nc_out)
{
    if (n < 1 || !o || !y_raw || K < 0 || K > QTL_MAXK || (K > 0 && !cov_raw) || !c) return false;
    if (n_var < 0 || n_var > K || n_var > QTLVAR_MAXV) return false;
    if (max_iter < 1 || max_iter > QTLVAR_MAX_ITER || !(tol - tol == 0.0)) return false;
    std::vector<double> y(y_raw, y_raw + n), cov(cov_raw, cov_raw + (K > 0 ? (size_t)n * K : 0));
    int n_c = 0;
    for (int i = 0; i < n; i++) n_c += c[i] ? 1 : 0;
    for (int k = -1; k < K; k++) {
        double*        col    = k < 0 ? y.data() : cov.data() + k;
        const int      stride = k < 0 ? 1 : K;
        const QtlMean2 mean   = qtl_column_mean2(col, n, stride, c);
        for (int i = 0; i < n; i++)
            if (c[i]) col[(size_t)i * stride] = qtl_minus_mean2(col[(size_t)i * stride], mean);
    }
    const QtlemDesign ds = qtlem_design(K, additive, imprint);
    const int         nx = ds.nx;
    bool              keep[QTLBIN_NE] = {true, true, true}, actx[QTLBIN_W], actv[QTLBIN_W], scanned = false;
    double            x0[QTL_NX], x[QTLBIN_W];
    for (int k = 0; k < QTL_NX; k++) x0[k] = 0.0;
    x0[0] = 1.0;
    bool all[QTLBIN_W];           // the row holds every place of the design; the active masks choose among them
    qtlbin_active(ds, keep, all);
    auto row = [&](int i) {
        for (int k = 1; k < nx; k++) x0[k] = cov[(size_t)i * K + (k - 1)];
        qtlbin_row(ds, all, x0, o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3], x);
    };
    QtlbinSums u;
    qtlbin_zero(u);
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        row(i);
        qtlbin_raw_terms(u, all, x);
    }
    *rank = qtlbin_rank(u, ds, n_c, keep, &scanned);
    if (n_c < qtlvar_min_n(ds, n_var)) {
        scanned = false;
        *rank   = 0;
        for (int e = 0; e < QTLBIN_NE; e++) keep[e] = false;
    }
    *nc_out  = n_c;
    *ll0_out = 0.0;
    for (int k = 0; k < QTLVAR_NFIT; k++) lod[k] = 0.0, iters[k] = status[k] = 0;
    for (int e = 0; e < ds.ne; e++) coef_mean[e] = coef_var[e] = (double)NAN;
    if (!scanned) return true;
    double yy = 0.0, lo = 0.0, hi = 0.0;
    bool   first = true;
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        yy += y[i] * y[i];
        lo = first ? y[i] : std::min(lo, y[i]);
        hi = first ? y[i] : std::max(hi, y[i]);
        first = false;
    }
    if (!(lo < hi)) return true;
    // one fit from its start to its stop
    auto run = [&](QtlvarFit& f, int mi, double tl) {
        for (;;) {
            qtlbin_zero(u);
            for (int i = 0; i < n; i++) {
                if (!c[i]) continue;
                row(i);
                qtlvar_mean_terms(u, actx, x, exp(-qtlvar_eta(actv, f.ga, x)), y[i]);
            }
            if (!qtlvar_beta(f, actx, u)) return;
            qtlbin_zero(u);
            for (int i = 0; i < n; i++) {
                if (!c[i]) continue;
                row(i);
                qtlvar_var_terms(u, actx, actv, f.bn, f.ga, x, y[i]);
            }
            if (!qtlvar_delta(f, actv, u)) return;
            int next;
            do {
                QtlvarTrial tr = {0.0, 0.0};
                for (int i = 0; i < n; i++) {
                    if (!c[i]) continue;
                    row(i);
                    qtlvar_trial_terms(tr, actx, actv, f.bn, f.gt, x, y[i]);
                }
                next = qtlvar_accept(f, actv, qtlvar_ll(tr.s, n_c), tr.emax, mi, tl);
            } while (next == QTLVAR_HALVE);
            if (next == QTLVAR_OVER) return;
        }
    };
    const bool none[QTLBIN_NE] = {false, false, false};
    QtlvarFit  f0;
    qtlvar_null_start(f0, yy, n_c);
    qtlvar_active(ds, n_var, none, -1, actx, actv);
    run(f0, QTLVAR_NULL_ITER, QTLVAR_NULL_TOL);
    if (!qtlvar_null_ok(f0)) return true;
    *ll0_out = f0.ll;
    if (*rank == 0) return true;
    double ll[QTLVAR_NFIT];
    for (int k = 0; k < QTLVAR_NFIT; k++) {
        QtlvarFit f;
        qtlvar_start(f, f0.be, nx, f0.ga, n_var, f0.ll);
        qtlvar_active(ds, n_var, keep, k, actx, actv);
        run(f, max_iter, tol);
        ll[k]     = f.ll;
        iters[k]  = f.iters;
        status[k] = f.status;
        if (k == 2)
            for (int e = 0; e < ds.ne; e++) {
                coef_mean[e] = keep[e] ? f.be[QTL_NX + e] : (double)NAN;
                coef_var[e]  = keep[e] ? f.ga[QTL_NX + e] : (double)NAN;
            }
    }
    qtlvar_lods(ll, f0.ll, lod);
    return true;
}
#endif

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlvar_kernels.hip read and write (device pointers).  `b` is the binary scan's record: the rank
// kernel is that scan's (launch_qtlbin_rank; launch_qtlvar_threshold then applies this scan's threshold to rank, keep and
// scan), the masks and n_c come from qtl_chrom_kernel and the column image from qtl_gather_kernel.  Of b's outputs lod, iters
// and status have QTLVAR_NFIT entries per cell and pmax per (permutation, trait, chromosome), coef is the mean part's, n_ones
// is not used; tilemax is [n_tiles][QTLVAR_NFIT][rstride] and nullq [C][QTLVAR_NULLQ][rstride].
constexpr int QTLVAR_NULLQ = QTL_NX + QTLVAR_NV0 + 2;    // doubles per (chromosome, column): beta0, gamma0, l0, 1.0 = scanned
struct QtlvarParams {
    QtlbinParams b;
    int          n_var;
    double*      coef_var;      // [T][M][ne]
};
void launch_qtlvar_threshold(const QtlvarParams& p, hipStream_t stream);
void launch_qtlvar_null(const QtlvarParams& p, hipStream_t stream);
void launch_qtlvar_fit(const QtlvarParams& p, hipStream_t stream);
void launch_qtlvar_finish(const QtlvarParams& p, hipStream_t stream);
#endif

} // namespace cnf2
#endif
