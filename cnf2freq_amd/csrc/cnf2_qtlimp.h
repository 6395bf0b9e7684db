// cnf2_qtlimp.h -- the multiple-imputation QTL scan (cnf2_qtl_scan_imp, include/cnf2hip.h), shared by host and device code:
// what a sampled state means to the model of cnf2_qtl.h, the check of a state array, the recurrence that combines the draws
// of one (marker, column) cell, that cell computed serially, and what the kernels of cnf2_qtlimp_kernels.hip read and write.
//
// Draw d of cnf2_sweep_sample gives every individual a hard origin class at every marker: state g < 64 has class
// k = bit0(g) + 2 bit3(g), the two bits cnf2_sweep_origins reads in every shift mode; 0xFF is "skipped".  The draw's one-hot
// row has a = [k = 3] - [k = 0] and d = [k = 1] + [k = 2], so a d = 0, and the draw is fitted by cnf2_qtl.h as it stands: the
// factor of X0'X0, qtl_marker_record with QTL_PIVOT, qtl_cell with its clamps.  The null fit does not depend on the draw, so
// the draws' likelihood ratios 10^lod_d have one denominator and their mean is the imputation estimate of the ratio
// (Sen and Churchill 2001):
//   m = max_d lod_d,  s = sum_d 10^(lod_d - m),  lod = m + log10(s / D),  coef = sum_d 10^(lod_d - m) coef_d / s.
#ifndef CNF2_QTLIMP_H
#define CNF2_QTLIMP_H

#include "cnf2_qtl.h"

namespace cnf2 {

constexpr int     QTLIMP_MAXD    = 1024;     // draws at most (cnf2_sweep_sample's bound)
constexpr uint8_t QTLIMP_SKIPPED = 0xFF;

// the origin class of a state below 64, and the draw's regressors for it
CNF2_HD int    qtlimp_class(uint8_t g) { return (g & 1) + ((g >> 2) & 2); }
CNF2_HD double qtlimp_a(int k) { return k == 3 ? 1.0 : (k == 0 ? -1.0 : 0.0); }
CNF2_HD double qtlimp_d(int k) { return (k == 1 || k == 2) ? 1.0 : 0.0; }

// The combination of one (marker, column) cell's draws, fed in ascending d.  m is the running maximum and s the sum of
// 10^(lod_d - m) so far; the coefficients are kept as the running weighted means ca, cd, which is the quotient above without
// its common scale: a new draw of weight w moves the mean by (w / s)(coef_d - mean).  Equal draws leave s = D, the means
// untouched and lod = m to the bit.  A draw that drops a column has a NaN coefficient, and the mean is NaN from there on.
struct QtlImpAcc {
    double m, s, ca, cd;
};
CNF2_HD void qtlimp_first(QtlImpAcc& r, const QtlCell& c)
{
    r.m = c.lod, r.s = 1.0, r.ca = c.ca, r.cd = c.cd;
}
CNF2_HD void qtlimp_next(QtlImpAcc& r, const QtlCell& c)
{
    double w = 1.0;                              // the new draw's weight against the maximum after it
    if (c.lod > r.m) {
        r.s = r.s * pow(10.0, r.m - c.lod) + 1.0;
        r.m = c.lod;
    } else {
        w = pow(10.0, c.lod - r.m);
        r.s += w;
    }
    const double f = w / r.s;
    r.ca += f * (c.ca - r.ca);
    r.cd += f * (c.cd - r.cd);
}
CNF2_HD QtlCell qtlimp_result(const QtlImpAcc& r, int D)
{
    QtlCell c;
    c.lod = r.m + log10(r.s / (double)D);     // a mean of ratios that are at least 1: not negative but for its rounding
    c.lod = c.lod > 0.0 ? c.lod : 0.0;
    c.ca  = r.ca;
    c.cd  = r.cd;
    return c;
}

// The check of the states of one (individual, chromosome): state[D][M] the individual's rows, first / len the chromosome.
// 0: fine; 1: a value in 64 .. 254; 2: skipped (0xFF) in some of the D x len cells and not in all.
enum { QTLIMP_STATE_OK = 0, QTLIMP_STATE_RANGE, QTLIMP_STATE_PARTIAL };
CNF2_HD int qtlimp_check_cells(const uint8_t* state, int D, size_t M, int first, int len)
{
    const bool skipped = state[first] == QTLIMP_SKIPPED;
    int        bad = QTLIMP_STATE_OK;
    for (int d = 0; d < D; d++)
        for (int j = 0; j < len; j++) {
            const uint8_t g = state[(size_t)d * M + first + j];
            if (g >= 64 && g != QTLIMP_SKIPPED) return QTLIMP_STATE_RANGE;
            if ((g == QTLIMP_SKIPPED) != skipped) bad = QTLIMP_STATE_PARTIAL;
        }
    return bad;
}

// One marker's combined cells on the CPU, the individuals and the draws in ascending order: state[n][D] the marker's states
// (below 64 wherever c is set), y[n][T] and cov[n][K] as they enter the sums (the callers centre them), c[n] the chromosome's
// mask.  lod[T], coef[T][2], the smallest rank, rss0[T], n_c, and draw_lod[D][T] where it is not null.  false: an argument
// out of range.
inline bool qtlimp_marker_serial(int n, int D, const uint8_t* state, int T, const double* y, int K, const double* cov, const uint8_t* c,
                                 bool additive, double* lod, double* coef, int32_t* rank, double* rss0, int32_t* n_c_out,
                                 double* draw_lod)
{
    if (n < 1 || D < 1 || D > QTLIMP_MAXD || T < 1 || K < 0 || K > QTL_MAXK) return false;
    for (int i = 0; i < n; i++)
        for (int d = 0; d < D; d++)
            if (c[i] && state[(size_t)i * D + d] >= 64) return false;
    const int nx = K + 1;
    auto      x  = [&](int i, int k) { return k == 0 ? 1.0 : cov[(size_t)i * K + (k - 1)]; };
    double    S[QTL_NX * QTL_NX] = {0.0};
    int       n_c = 0;
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        n_c++;
        for (int j = 0; j < nx; j++)
            for (int k = 0; k <= j; k++) S[j * QTL_NX + k] += x(i, j) * x(i, k);
    }
    const bool usable = qtl_cholesky(S, nx) && n_c >= K + 4;
    *n_c_out = n_c;
    *rank    = 2;
    for (int t = 0; t < T; t++) {
        double b[QTL_NX] = {0.0}, z[QTL_NX], yy = 0.0;
        for (int i = 0; i < n; i++) {
            if (!c[i]) continue;
            const double v = y[(size_t)i * T + t];
            for (int k = 0; k < nx; k++) b[k] += x(i, k) * v;
            yy += v * v;
        }
        double r0 = 0.0;
        if (usable) {
            for (int k = 0; k < QTL_NX; k++) z[k] = b[k];
            qtl_chol_solve(S, nx, z);
            double e = 0.0;
            for (int k = 0; k < nx; k++) e += b[k] * z[k];
            r0 = yy - e;
        }
        rss0[t] = r0;
        QtlImpAcc acc = {0.0, 0.0, 0.0, 0.0};
        for (int d = 0; d < D; d++) {
            double sa[QTL_NX] = {0.0}, sd[QTL_NX] = {0.0}, saa = 0.0, sdd = 0.0, va = 0.0, vd = 0.0;
            for (int i = 0; i < n; i++) {
                if (!c[i]) continue;
                const int    k = qtlimp_class(state[(size_t)i * D + d]);
                const double a = qtlimp_a(k), dd = qtlimp_d(k), v = y[(size_t)i * T + t];
                for (int j = 0; j < nx; j++) {
                    sa[j] += a * x(i, j);
                    sd[j] += dd * x(i, j);
                }
                saa += a * a, sdd += dd * dd;
                va += a * v, vd += dd * v;
            }
            double        rec[QTL_MK];
            const int32_t rk = qtl_marker_record(S, nx, usable, sa, sd, saa, 0.0, sdd, additive, rec);
            *rank            = rk < *rank ? rk : *rank;
            for (int k = 0; k < nx; k++) {
                va -= rec[k] * b[k];
                vd -= rec[QTL_NX + k] * b[k];
            }
            const QtlCell cell = qtl_cell(va, vd, rec[QTL_PA], rec[QTL_L], rec[QTL_PD], r0, n_c, usable);
            if (draw_lod) draw_lod[(size_t)d * T + t] = cell.lod;
            if (d == 0) qtlimp_first(acc, cell);
            else qtlimp_next(acc, cell);
        }
        const QtlCell out = qtlimp_result(acc, D);
        lod[t] = out.lod, coef[2 * t] = out.ca, coef[2 * t + 1] = out.cd;
    }
    return true;
}

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlimp_kernels.hip read and write beside the single scan's QtlParams (device pointers).  q.origin
// is null: the mask and the regressors come from the states; so is q.mk: the records are per draw.
struct QtlImpParams {
    QtlParams      q;
    int            D;
    const uint8_t* state;        // [n][D][M]
    double*        mkd;          // [D][M][QTL_MK] a draw's marker records
    int32_t*       bad;          // [2] set to 1 by the check: a value in 64 .. 254, a partly skipped (individual, chromosome)
    double*        draw_lod;     // [D][T][M] or null
};
void launch_qtlimp_check(const QtlImpParams& p, hipStream_t stream);
void launch_qtlimp_chrom(const QtlImpParams& p, hipStream_t stream);
void launch_qtlimp_design(const QtlImpParams& p, hipStream_t stream);
void launch_qtlimp_rank(const QtlImpParams& p, hipStream_t stream);
void launch_qtlimp_scan(const QtlImpParams& p, hipStream_t stream);
#endif

}  // namespace cnf2
#endif  // CNF2_QTLIMP_H
