// cnf2_qtlsurv.h -- the survival-trait single-locus scan (cnf2_qtl_scan_surv, include/cnf2hip.h), shared by host and device
// code: the design, one position's terms of the forward and the backward pass, the group-end step, the Newton step and the
// stopping rule.  The kernels of cnf2_qtlsurv_kernels.hip (and qtlsurv_fit_serial below, on the CPU) form the running sums
// along the risk order; every decision that gives the result its meaning is taken here or in cnf2_qtlbin.h.
//
// Cox's proportional hazards regression of (time, status) on the origin rows, Breslow's partial likelihood for ties: under the
// mask c of a chromosome, with the marker's origin row o,
//   x_i = [z_1 .. z_K, a, d, i] (the effects as in cnf2_qtlbin.h),  w_j = exp(x_j' theta),  S0(t) = sum_{j: c_j, t_j >= t} w_j,
//   l(theta) = sum_{k: c_k, delta_k = 1} [ eta_k - log S0(t_k) ]
// There is no intercept (it is not identifiable).  The places are cnf2_qtlbin.h's -- X0 at 0 .. K, the effects at QTL_NX + e
// -- with place 0, the intercept, active in the rank rule only: so qtlbin_factor, qtlbin_solve and qtlbin_step serve as they
// are, and a fit pays nothing for the place it does not use.
//   rank rule  qtlbin_rank's, on the unweighted columns [1, z, a, d, i]: a column that is constant over the individuals of c
//              is dropped, a chromosome is scanned when X0 has a factor and n_c >= W + 1, W = 1 + K + ne.
//   risk order the individuals of a column by descending time; equal times form a tie group, inside it ascending index; the
//              individuals that are not used follow, each a group of its own (qtlsurv_order).  One word per position: the
//              individual, whether it has an event, whether it ends its group.
//   a pass     along that order with S0_r, S1_r the inclusive running sums of w and w x (a masked individual has w = 0 and
//              no event), at the end r of a group with ev_r unmasked events: c_r = ev_r / S0_r, m_r = S1_r / S0_r (a group
//              without events has c_r = 0 and adds nothing), and with A_q the inclusive suffix sum of c from q on:
//                l = sum_r delta_r eta_r - sum_ends ev_r log S0_r
//                s = sum_r delta_r x_r   - sum_q w_q A_q x_q
//                G = sum_q w_q A_q x_q x_q' - sum_ends ev_r m_r m_r'
//              (the forward pass gives the first sum of l and s, the group-end terms and c_r, w_r per position; the backward
//              pass the sums with A.)  Both terms of G go to the same packed triangle.
//   null fit   per chromosome and column on the covariates alone from theta = 0: QTLSURV_NULL_ITER iterations at most,
//              stopped by QTLSURV_NULL_TOL; without covariates the single pass at theta = 0, which gives
//              l0 = -sum_groups ev_g log(n at risk).  A column without an event among the n_c, or whose null fit does not
//              stop by its tolerance or breaks down, is not scanned on that chromosome.
//   fit        from (gamma0, 0), so l_0 = l0; the stopping rule, the step and its breakdown are qtlbin_step's.  In addition a
//              pass at theta_t, t >= 1, whose l is not finite (an S0 that overflowed) is a breakdown: the fit goes back to
//              theta_{t-1}, l_{t-1} with iters = t - 1 and status 2, so that what is reported is always finite.  This is
//              where a monotone likelihood ends if max_iter does not end it first.  There is no step-halving.
// Every loop over the places has a constant bound and a predicate, so that the device code keeps its vectors in registers.
#ifndef CNF2_QTLSURV_H
#define CNF2_QTLSURV_H

#include "cnf2_qtlbin.h"

#include <algorithm>
#include <vector>

namespace cnf2 {

constexpr int      QTLSURV_MAX_ITER  = QTLBIN_MAX_ITER;
constexpr int      QTLSURV_NULL_ITER = 50;
constexpr double   QTLSURV_NULL_TOL  = 1e-13;               // LOD
constexpr uint32_t QTLSURV_IND       = 0x3fffffffu;         // the order word: the individual,
constexpr uint32_t QTLSURV_EVENT     = 0x40000000u;         //   its status,
constexpr uint32_t QTLSURV_END       = 0x80000000u;         //   whether the position is the last of its tie group

// which places take part: the covariates and the kept effects, not the intercept
CNF2_HD void qtlsurv_active(const QtlemDesign& ds, const bool keep[QTLBIN_NE], bool act[QTLBIN_W])
{
    qtlbin_active(ds, keep, act);
    act[0] = false;
}

CNF2_HD double qtlsurv_eta(const bool act[QTLBIN_W], const double th[QTLBIN_W], const double x[QTLBIN_W])
{
    double eta = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) eta += x[j] * th[j];
    return eta;
}

// forward pass, a position with an unmasked event: delta eta and delta x
CNF2_HD void qtlsurv_event_terms(QtlbinSums& u, const bool act[QTLBIN_W], const double x[QTLBIN_W], double eta)
{
    u.ll += eta;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) u.s[j] += x[j];
}

// forward pass, the last position of a tie group with ev unmasked events and the running sums S0, S1 there: the group's
// terms of l and G; returns c_r
CNF2_HD double qtlsurv_group_end(QtlbinSums& u, const bool act[QTLBIN_W], int ev, double S0, const double S1[QTLBIN_W])
{
    if (ev <= 0) return 0.0;
    const double e = (double)ev;
    u.ll -= e * log(S0);
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) {
            const double emj = e * (S1[j] / S0);
CNF2_QTL_UNROLL
            for (int k = 0; k < QTLBIN_W; k++)
                if (k <= j && act[k]) u.G[qtlbin_at(j, k)] -= emj * (S1[k] / S0);
        }
    return e / S0;
}

// backward pass, a position with wa = w_q A_q
CNF2_HD void qtlsurv_back_terms(QtlbinSums& u, const bool act[QTLBIN_W], const double x[QTLBIN_W], double wa)
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) {
            const double wx = wa * x[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTLBIN_W; k++)
                if (k <= j && act[k]) u.G[qtlbin_at(j, k)] += wx * x[k];
            u.s[j] -= wx;
        }
}

// the iterate of a fit: qtlbin's, and theta_{t-1} for the way back from a pass that is not finite
struct QtlsurvFit {
    QtlbinFit f;
    double    th_prev[QTLBIN_W];
};

CNF2_HD void qtlsurv_start(QtlsurvFit& s, const double g0[QTL_NX], int nx, double ll0)
{
    qtlbin_start(s.f, g0, nx, ll0);
    s.f.th[0] = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) s.th_prev[j] = s.f.th[j];
}

// After a pass at theta_t: true when the fit is over (cnf2_qtlbin.h's qtlbin_step, and the rule for a pass that is not finite)
CNF2_HD bool qtlsurv_step(QtlsurvFit& s, const bool act[QTLBIN_W], QtlbinSums& u, int max_iter, double tol, bool known0)
{
    if (s.f.iters >= 1 && !(u.ll - u.ll == 0.0)) {
CNF2_QTL_UNROLL
        for (int j = 0; j < QTLBIN_W; j++) s.f.th[j] = s.th_prev[j];
        s.f.ll = s.f.ll_prev;
        s.f.iters--;
        s.f.status = 2;
        return true;
    }
    double th[QTLBIN_W];
CNF2_QTL_UNROLL
    for (int j = 0; j < QTLBIN_W; j++) th[j] = s.f.th[j];
    const bool over = qtlbin_step(s.f, act, u, max_iter, tol, known0);
    if (!over) {
CNF2_QTL_UNROLL
        for (int j = 0; j < QTLBIN_W; j++) s.th_prev[j] = th[j];
    }
    return over;
}

// a finished null fit counts when it stopped by its tolerance; without covariates it is the pass at theta = 0 alone
CNF2_HD bool qtlsurv_null_ok(const QtlbinFit& f, int K, double ll)
{
    if (K == 0) return ll - ll == 0.0;
    return f.status == 0 && f.iters >= 1;
}

// The risk order of one column: individual i carries time[src(i) * stride], status[src(i) * stride] with src = perm (NULL:
// the identity); use[n] says who is used.  Stable: descending time, ties by ascending i; the unused follow in ascending
// order, each the end of a group of its own, without an event.  word[n].
inline void qtlsurv_order(int n, const double* time, const double* status, size_t stride, const int32_t* perm, const uint8_t* use,
                          uint32_t* word)
{
    std::vector<int32_t> idx;
    idx.reserve(n);
    for (int i = 0; i < n; i++)
        if (use[i]) idx.push_back(i);
    auto t = [&](int32_t i) { return time[(size_t)(perm ? perm[i] : i) * stride]; };
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return t(a) > t(b); });
    const size_t nu = idx.size();
    for (size_t r = 0; r < nu; r++) {
        const int32_t i   = idx[r];
        const bool    ev  = status[(size_t)(perm ? perm[i] : i) * stride] == 1.0;
        const bool    end = r + 1 == nu || t(idx[r + 1]) != t(i);
        word[r] = (uint32_t)i | (ev ? QTLSURV_EVENT : 0u) | (end ? QTLSURV_END : 0u);
    }
    size_t r = nu;
    for (int i = 0; i < n; i++)
        if (!use[i]) word[r++] = (uint32_t)i | QTLSURV_END;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One (marker, column) fit on the CPU: o[n][4] the marker's origin rows, time[n] and status[n] (finite, 0 or 1 where c is
// set), the covariates cov[n][K], c[n] the chromosome's mask.  Mirrors what the kernels do with the functions above, the
// running sums in the plain order of the positions.  As the scan does, it works on the covariates minus their means over the
// individuals of c, each difference rounded once.
// Returns false for bad arguments.  Outputs: lod, coef[ne] (NaN where dropped or not fitted), iters, status, rank, ll0 (0 for
// a column that is not scanned), n_events, n_c.
inline bool qtlsurv_fit_serial(int n, const double* o, const double* time, const double* status_in, int K, const double* cov_raw,
                               const uint8_t* c, bool additive, bool imprint, int max_iter, double tol, double* lod, double* coef,
                               int32_t* iters, int32_t* status, int32_t* rank, double* ll0_out, int32_t* nev_out, int32_t* nc_out)
{
    if (n < 1 || (uint32_t)n > QTLSURV_IND || !o || !time || !status_in || K < 0 || K > QTL_MAXK || (K > 0 && !cov_raw) || !c) return false;
    if (max_iter < 1 || max_iter > QTLSURV_MAX_ITER || !(tol - tol == 0.0)) return false;
    int n_c = 0, n_ev = 0;
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        if (!(status_in[i] == 0.0 || status_in[i] == 1.0) || !(time[i] - time[i] == 0.0)) return false;
        n_c++;
        n_ev += status_in[i] == 1.0 ? 1 : 0;
    }
    std::vector<double> cov(cov_raw, cov_raw + (K > 0 ? (size_t)n * K : 0));
    for (int k = 0; k < K; k++) {
        const QtlMean2 mean = qtl_column_mean2(cov.data() + k, n, K, c);
        for (int i = 0; i < n; i++)
            if (c[i]) cov[(size_t)i * K + k] = qtl_minus_mean2(cov[(size_t)i * K + k], mean);
    }
    std::vector<uint8_t> mask(n);
    for (int i = 0; i < n; i++) mask[i] = c[i] ? 1 : 0;
    std::vector<uint32_t> word(n);
    qtlsurv_order(n, time, status_in, 1, nullptr, mask.data(), word.data());

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
    qtlbin_active(ds, keep, act);          // the rank rule: with the intercept
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        row(i);
        qtlbin_raw_terms(u, act, x);
    }
    *rank    = qtlbin_rank(u, ds, n_c, keep, &scanned);
    *nev_out = n_ev;
    *nc_out  = n_c;
    *lod     = 0.0;
    *ll0_out = 0.0;
    *iters = *status = 0;
    for (int e = 0; e < ds.ne; e++) coef[e] = (double)NAN;
    if (!scanned || n_ev == 0) return true;

    std::vector<double> cr(n), wr(n);
    auto pass = [&](const double th[QTLBIN_W]) {
        qtlbin_zero(u);
        double S0 = 0.0, S1[QTLBIN_W];
        for (int j = 0; j < QTLBIN_W; j++) S1[j] = 0.0;
        int ev = 0;
        for (int r = 0; r < n; r++) {
            const int i = (int)(word[r] & QTLSURV_IND);
            double    w = 0.0;
            if (c[i]) {
                row(i);
                const double eta = qtlsurv_eta(act, th, x);
                w = exp(eta);
                if (word[r] & QTLSURV_EVENT) {
                    qtlsurv_event_terms(u, act, x, eta);
                    ev++;
                }
                S0 += w;
                for (int j = 0; j < QTLBIN_W; j++)
                    if (act[j]) S1[j] += w * x[j];
            }
            wr[r] = w;
            cr[r] = 0.0;
            if (word[r] & QTLSURV_END) {
                cr[r] = qtlsurv_group_end(u, act, ev, S0, S1);
                ev = 0;
            }
        }
        double A = 0.0;
        for (int r = n - 1; r >= 0; r--) {
            A += cr[r];
            if (wr[r] == 0.0) continue;
            row((int)(word[r] & QTLSURV_IND));
            qtlsurv_back_terms(u, act, x, wr[r] * A);
        }
    };
    // the null fit
    const bool none[QTLBIN_NE] = {false, false, false};
    double     g0[QTL_NX];
    for (int k = 0; k < QTL_NX; k++) g0[k] = 0.0;
    QtlsurvFit f0;
    qtlsurv_start(f0, g0, nx, 0.0);
    qtlsurv_active(ds, none, act);
    pass(f0.f.th);
    double l0 = u.ll;
    if (K > 0) {
        while (!qtlsurv_step(f0, act, u, QTLSURV_NULL_ITER, QTLSURV_NULL_TOL, false)) pass(f0.f.th);
        l0 = f0.f.ll;
    }
    if (!qtlsurv_null_ok(f0.f, K, l0)) return true;
    *ll0_out = l0;
    if (*rank == 0) return true;
    QtlsurvFit f;
    qtlsurv_start(f, f0.f.th, nx, l0);
    qtlsurv_active(ds, keep, act);
    for (;;) {
        pass(f.f.th);
        if (qtlsurv_step(f, act, u, max_iter, tol, true)) break;
    }
    *lod    = qtlbin_lod(f.f, l0);
    *iters  = f.f.iters;
    *status = f.f.status;
    for (int e = 0; e < ds.ne; e++) coef[e] = keep[e] ? f.f.th[QTL_NX + e] : (double)NAN;
    return true;
}
#endif

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlsurv_kernels.hip read and write (device pointers).  `b` is the binary scan's record: the rank
// kernel and the finish kernel are that scan's (launch_qtlbin_rank, launch_qtlbin_finish), the masks and n_c come from
// qtl_chrom_kernel; b.Y is not used (the order words take the column image's place), b.n_ones receives n_events.
struct QtlsurvParams {
    QtlbinParams    b;
    const uint32_t* ord;         // [rn][n] the risk order of the tile's columns
    double*         work;        // [waves][2][n]: c_r and w_r of the pass a wave is in
    int             null_blocks; // blocks of the null launch and
    int             fit_blocks;  //   of the fit launch: each strides over its cells
};
constexpr int QTLSURV_WAVES = QTLBIN_TILE;   // waves per block of both kernels
void launch_qtlsurv_null(const QtlsurvParams& q, hipStream_t stream);
void launch_qtlsurv_fit(const QtlsurvParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
