// cnf2_qtl.h -- the small dense algebra of the QTL scan (cnf2_qtl_scan, include/cnf2hip.h), shared by host and device code:
// the Cholesky factor of the null design's normal matrix, the 2 x 2 pivoting of a marker's Schur complement with its rank
// rule, and the clamps and logarithm of one (marker, column) cell.  The kernels of cnf2_qtl_kernels.hip form the sums; every
// decision that gives the result its meaning (which column is dropped, what a degenerate cell reports) is taken here.
//
// Haley-Knott regression of phenotype columns y on the origin rows: null design X0 = [c, c z_1 .. c z_K], full design X0
// plus (c a, c d) with a = origin[3] - origin[0], d = origin[1] + origin[2] and c the 0/1 mask of the individuals used on the
// chromosome.  With S11 = X0'X0, S21 = A'X0, S22 = A'A, G = S21 S11^-1, W = S22 - G S21' (factored in the order a, d):
//   v = A'y - G b0,  dRSS = v' W^-1 v,  lod = (n_c / 2) log10(RSS0 / (RSS0 - dRSS)),  coef = W^-1 v.
// Every loop over the columns of X0 has the constant bound QTL_NX and a predicate, so that the device code keeps its
// vectors in registers.
#ifndef CNF2_QTL_H
#define CNF2_QTL_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef CNF2_HD
#define CNF2_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef CNF2_HD
#define CNF2_HD inline
#endif
#endif

// (the host compilers do not know the pragma)
#if defined(__HIPCC__)
#define CNF2_QTL_UNROLL _Pragma("unroll")
#else
#define CNF2_QTL_UNROLL
#endif

namespace cnf2 {

constexpr int    QTL_MAXK  = 8;                      // covariates at most
constexpr int    QTL_NX    = QTL_MAXK + 1;           // columns of X0 at most
constexpr int    QTL_CHOL  = QTL_NX * QTL_NX + 1;    // doubles per chromosome: L (lower, row-major, stride QTL_NX), then 1.0 = usable
constexpr int    QTL_MK    = 24;                     // doubles per marker record: G_a[9], G_d[9], pivot a, l, pivot d
constexpr int    QTL_PA    = 2 * QTL_NX, QTL_L = QTL_PA + 1, QTL_PD = QTL_PA + 2;
constexpr double QTL_PIVOT = 1e-8;                   // a column is dropped when its pivot is below this times its raw diagonal

// The mean of v[i * stride] over the individuals with use[i] != 0 (0 without any), in two passes: the second adds the mean of
// what the first left, so that the mean of equal values is that value and a constant column minus its mean is exactly 0.
// The scans subtract it from every trait and every covariate column of X0 before they form a sum (include/cnf2hip.h: they do
// not depend on units and offsets); the intercept takes it up.
CNF2_HD double qtl_column_mean(const double* v, int n, int stride, const uint8_t* use)
{
    int n_u = 0;
    for (int i = 0; i < n; i++) n_u += use[i] ? 1 : 0;
    if (n_u == 0) return 0.0;
    double mean = 0.0;
    for (int pass = 0; pass < 2; pass++) {
        double s = 0.0;
        for (int i = 0; i < n; i++)
            if (use[i]) s += v[(size_t)i * stride] - mean;
        mean += s / n_u;
    }
    return mean - mean == 0.0 ? mean : 0.0;       // (finite values whose sum is not: left as they are)
}

// The same mean carried as an unevaluated sum hi + lo of two doubles, for the binary-trait scan (cnf2_qtl_scan_binary).  The
// mean of n values is in general no double: rounded to one, the mean of z + 16384 is known 2^12 times less finely than that of
// z, and the two centred columns differ by 1e-12.  A logistic fit of a nearly collinear marker multiplies that by 1e7 and
// more, into the printed digits of its effects.  Here the sum keeps its rounding errors (two_sum), the quotient its remainder,
// and v - (hi + lo) is rounded once: the centred value is the true one to the last bit (but for ties of 2^-106), so columns that
// differ by an exact shift, or by a power of two, give the same centred bits.  The mean of equal values is that value.
// s + e = a + b exactly
CNF2_HD void qtl_two_sum(double a, double b, double& s, double& e)
{
    s               = a + b;
    const double bb = s - a;
    e               = (a - (s - bb)) + (b - bb);
}
struct QtlMean2 {
    double hi, lo;
};
CNF2_HD QtlMean2 qtl_column_mean2(const double* v, int n, int stride, const uint8_t* use)
{
    QtlMean2 m = {0.0, 0.0};
    int      n_u = 0;
    bool     equal = true;
    double   first = 0.0, s = 0.0, c = 0.0, e;
    for (int i = 0; i < n; i++) {
        if (!use[i]) continue;
        const double x = v[(size_t)i * stride];
        if (n_u == 0) first = x;
        equal = equal && x == first;
        qtl_two_sum(s, x, s, e);
        c += e;
        n_u++;
    }
    if (n_u == 0 || !(s - s == 0.0)) return m;        // (finite values whose sum is not: left as they are)
    if (equal) {
        m.hi = first;
        return m;
    }
    qtl_two_sum(s, c, s, c);
    const double hi = s / n_u, lo = (fma(-hi, (double)n_u, s) + c) / n_u;
    qtl_two_sum(hi, lo, m.hi, m.lo);
    return m;
}
CNF2_HD double qtl_minus_mean2(double v, const QtlMean2& m)
{
    double t, e;
    qtl_two_sum(v, -m.hi, t, e);
    return t + (e - m.lo);
}

// S = L L' in place on the lower triangle of S[nx][QTL_NX]; false when a pivot is not positive (X0 without full rank)
CNF2_HD bool qtl_cholesky(double* S, int nx)
{
    for (int j = 0; j < nx; j++) {
        double d = S[j * QTL_NX + j];
        for (int k = 0; k < j; k++) d -= S[j * QTL_NX + k] * S[j * QTL_NX + k];
        if (!(d > 0.0)) return false;
        d                 = sqrt(d);
        S[j * QTL_NX + j] = d;
        for (int i = j + 1; i < nx; i++) {
            double s = S[i * QTL_NX + j];
            for (int k = 0; k < j; k++) s -= S[i * QTL_NX + k] * S[j * QTL_NX + k];
            S[i * QTL_NX + j] = s / d;
        }
    }
    return true;
}

// x <- S^-1 x with S = L L'
CNF2_HD void qtl_chol_solve(const double* L, int nx, double x[QTL_NX])
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_NX; j++)
        if (j < nx) {
            double s = x[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTL_NX; k++)
                if (k < j) s -= L[j * QTL_NX + k] * x[k];
            x[j] = s / L[j * QTL_NX + j];
        }
CNF2_QTL_UNROLL
    for (int jj = 0; jj < QTL_NX; jj++) {
        const int j = QTL_NX - 1 - jj;
        if (j < nx) {
            double s = x[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTL_NX; k++)
                if (k > j && k < nx) s -= L[k * QTL_NX + j] * x[k];
            x[j] = s / L[j * QTL_NX + j];
        }
    }
}

// One marker's record (G, the pivots) from its sums: s21a / s21d = the rows of S21, S22 = (saa, sad, sdd).
// Returns the rank (0, 1 or 2); a dropped column has pivot 0 in the record.  usable = false (no Cholesky factor): rank 0.
CNF2_HD int qtl_marker_record(const double* L, int nx, bool usable, double s21a[QTL_NX], double s21d[QTL_NX], double saa,
                              double sad, double sdd, bool additive, double* rec)
{
    double ga[QTL_NX], gd[QTL_NX];
CNF2_QTL_UNROLL
    for (int k = 0; k < QTL_NX; k++) {
        ga[k] = (usable && k < nx) ? s21a[k] : 0.0;
        gd[k] = (usable && k < nx) ? s21d[k] : 0.0;
    }
    if (usable) {
        qtl_chol_solve(L, nx, ga);
        qtl_chol_solve(L, nx, gd);
    }
    double waa = saa, wad = sad, wdd = sdd;
CNF2_QTL_UNROLL
    for (int k = 0; k < QTL_NX; k++)
        if (k < nx) {
            waa -= ga[k] * s21a[k];
            wad -= ga[k] * s21d[k];
            wdd -= gd[k] * s21d[k];
        }
    const bool   keep_a = usable && saa > 0.0 && waa >= QTL_PIVOT * saa;
    const double pa     = keep_a ? waa : 0.0;
    const double l      = keep_a ? wad / pa : 0.0;
    const double wd     = wdd - l * wad;
    const bool   keep_d = usable && !additive && sdd > 0.0 && wd >= QTL_PIVOT * sdd;
CNF2_QTL_UNROLL
    for (int k = 0; k < QTL_NX; k++) {
        rec[k]          = ga[k];
        rec[QTL_NX + k] = gd[k];
    }
    rec[QTL_PA] = pa;
    rec[QTL_L]  = l;
    rec[QTL_PD] = keep_d ? wd : 0.0;
    return (keep_a ? 1 : 0) + (keep_d ? 1 : 0);
}

struct QtlCell {
    double lod, ca, cd;
};

// One (marker, column) cell from v = A'y - G b0, the marker's pivots and the column's RSS0.  usable: the chromosome has a
// Cholesky factor and n_c >= K + 4.  dRSS is clamped to [0, RSS0 (1 - 2^-52)]: the LOD is finite and not negative.
CNF2_HD QtlCell qtl_cell(double va, double vd, double pa, double l, double pd, double rss0, int n_c, bool usable)
{
    QtlCell r;
    r.lod = 0.0;
    r.ca = r.cd = (double)NAN;
    if (!usable || !(rss0 > 0.0)) return r;
    const double u = vd - l * va;
    double       d = 0.0;
    if (pd > 0.0) {
        r.cd = u / pd;
        d += u * r.cd;
    }
    if (pa > 0.0) {
        r.ca = va / pa;
        d += va * r.ca;
        if (pd > 0.0) r.ca -= l * r.cd;
    }
    const double hi = rss0 * (1.0 - 2.220446049250313e-16);
    d               = d < 0.0 ? 0.0 : (d > hi ? hi : d);
    if (d > 0.0) r.lod = 0.5 * (double)n_c * log10(rss0 / (rss0 - d));
    return r;
}

#if defined(__HIPCC__)
// What the kernels of cnf2_qtl_kernels.hip read and write (device pointers)
struct QtlParams {
    int n, M, C, T, P, K, nx, additive;
    const double*  origin;       // [n][M][4]
    const double*  pheno;        // [n][T]
    const double*  cov;          // [n][K]
    const uint8_t* use;          // [n]
    const int32_t* perm;         // [P][n]
    const int32_t* cs;           // [C + 1] chromstarts
    const int32_t* mchrom;       // [M] chromosome of a marker
    uint8_t*       cmask;        // [C][n] c_i
    int32_t*       nc;           // [C] n_c
    double*        chol;         // [C][QTL_CHOL]
    double*        mk;           // [M][QTL_MK]
    int32_t*       rank;         // [M]
    // the column tile: columns [r0, r0 + rn) of the R = T (1 + P)
    int            r0, rn, rstride;
    double*        Y;            // [n][rstride] the column image
    double*        nullq;        // [C][nx + 1][rstride]: b0, then RSS0
    const int32_t* tiles;        // [n_tiles][4] chromosome, first marker, markers (<= 16), 0
    const int32_t* tile_start;   // [C + 1]
    int            n_tiles;
    double*        tilemax;      // [n_tiles][rstride]
    double *       lod, *coef, *rss0, *pmax;
};
void launch_qtl_chrom(const QtlParams& q, hipStream_t stream);
void launch_qtl_design(const QtlParams& q, hipStream_t stream);
void launch_qtl_gather(const QtlParams& q, hipStream_t stream);
void launch_qtl_null(const QtlParams& q, hipStream_t stream);
void launch_qtl_scan(const QtlParams& q, hipStream_t stream);
void launch_qtl_finish(const QtlParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
