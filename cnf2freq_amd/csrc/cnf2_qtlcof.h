// cnf2_qtlcof.h -- the small dense algebra of the cofactor scan (cnf2_qtl_scan_cof, include/cnf2hip.h), shared by host and
// device code: which columns a marker's design has, which cofactors are left out at a marker, the sequential Cholesky
// factor of its normal matrix with the rank rule, and the substitutions, clamps and logarithms of one (marker, column) cell.
// The kernels of cnf2_qtlcof_kernels.hip form the sums; every decision that gives the result its meaning is taken here.
//
// Composite interval mapping by Haley-Knott regression under the mask c of a chromosome, with a = o[3] - o[0] and
// d = o[1] + o[2] of a locus's origin row o.  In this column order:
//   null        X0 = [c, c z_1 .. c z_K]
//   cofactors   for q = 0 .. Q - 1 in the order of cof: a_q, d_q of marker cof[q]   (CNF2_QTL_ADDITIVE: a_q)
//               -- a cofactor that is left out at the tested marker (excl_lo[q] <= m <= excl_hi[q]) keeps its place as zero
//               columns: raw diagonal 0, dropped by the rank rule, pivot 0.  The column order never closes up
//   marker      a, d of the tested marker                                            (CNF2_QTL_ADDITIVE: a)
// The additive model is linear in each locus's indicators, so the marginal rows are its exact Haley-Knott regressors, for
// cofactors on the tested marker's own chromosome as well.  One Cholesky factor L of the whole design's normal matrix in
// that order gives both nested comparisons: with w = L^-1 X'y over the kept columns
//   RSS0 = sum c y^2 - sum_{X0} w^2,  lod_base = LOD(sum_{cofactors} w^2),  lod = LOD(sum_{cofactors, marker} w^2) - lod_base
// (LOD = qtl2_lod: the cumulative reduction clamped, finite and not negative).  The effects of the marker in the full
// model come from the back-substitution L' beta = w on its columns, which are the last.
#ifndef CNF2_QTLCOF_H
#define CNF2_QTLCOF_H

#include "cnf2_qtlx.h"

namespace cnf2 {

constexpr int QTLCOF_MAXW = QTLX_MAXW;       // the design's width at most: cnf2_qtl_scanx's bound, for its reason
constexpr int QTLCOF_MAXQ = QTLCOF_MAXW - 2; // cofactors at most: 1 + Q + 1 <= 15 in the additive model
constexpr int QTLCOF_COF  = 5;               // the effect code of a cofactor column, beside QTLX_ONE .. QTLX_NONE

struct QtlcofDesign {
    int nx;          // columns of X0
    int ne;          // effects per locus: a, then d (unless additive)
    int nq;          // cofactors
    int nc;          // cofactor columns: ne nq
    int w;           // all columns
};
CNF2_HD QtlcofDesign qtlcof_design(int K, int Q, bool additive)
{
    QtlcofDesign ds;
    ds.nx = K + 1;
    ds.ne = additive ? 1 : 2;
    ds.nq = Q;
    ds.nc = ds.ne * Q;
    ds.w  = ds.nx + ds.nc + ds.ne;
    return ds;
}

// What column j of the design is:
//   *e: QTLX_ONE (the mask column for *z = 0, covariate *z - 1 otherwise), QTLCOF_COF (column *z of the cofactor image
//   [n][ne Q]: effect *z % ne of cofactor *z / ne), QTLX_A / QTLX_D (the tested marker's; *z = 0), QTLX_NONE (a zero column)
CNF2_HD void qtlcof_column(const QtlcofDesign& ds, int j, int* e, int* z)
{
    *e = QTLX_NONE;
    *z = 0;
    if (j < 0 || j >= ds.w) return;
    if (j < ds.nx) {
        *e = QTLX_ONE;
        *z = j;
    } else if (j < ds.nx + ds.nc) {
        *e = QTLCOF_COF;
        *z = j - ds.nx;
    } else
        *e = j - ds.nx - ds.nc == 0 ? QTLX_A : QTLX_D;
}

// bit q: cofactor q is left out of the design at marker m
CNF2_HD uint32_t qtlcof_skip_word(int m, int Q, const int32_t* excl_lo, const int32_t* excl_hi)
{
    uint32_t w = 0;
    for (int q = 0; q < Q; q++)
        if (excl_lo[q] <= m && m <= excl_hi[q]) w |= 1u << q;
    return w;
}

struct QtlcofFactor {
    int usable;      // the chromosome is scanned: n_c >= W + 1 (W the full width) and X0 has a Cholesky factor
    int rank_cof;    // kept cofactor columns
    int rank;        // kept effects of the tested marker
};

// G (lower triangle of the normal matrix, row-major with stride ld, QTL2_W rows) <- its sequential Cholesky factor in the
// column order of the design, by qtl2_factor's rule: a column of X0 must have a positive pivot (else the chromosome is not
// scanned); an added column is dropped -- pivot 0 and a zero column in L -- when its raw diagonal is 0 or its pivot is below
// QTL_PIVOT times its raw diagonal.  Only the first `cols` columns are factored (nx: the null design alone); whether the
// chromosome is scanned is decided by the whole design's width.
CNF2_HD QtlcofFactor qtlcof_factor(double* G, int ld, const QtlcofDesign& ds, int n_c, int cols)
{
    QtlcofFactor f;
    f.usable = n_c >= ds.w + 1 ? 1 : 0;
    int rc = 0, rm = 0;
    for (int j = 0; j < cols && f.usable; j++) {
        const double raw = G[j * ld + j];
        double       d   = raw;
        for (int k = 0; k < j; k++) d -= G[j * ld + k] * G[j * ld + k];
        bool keep;
        if (j < ds.nx) {
            keep = d > 0.0;
            if (!keep) f.usable = 0;
        } else
            keep = raw > 0.0 && d >= QTL_PIVOT * raw;
        if (!keep) {
            for (int i = j; i < cols; i++) G[i * ld + j] = 0.0;
            continue;
        }
        d             = sqrt(d);
        G[j * ld + j] = d;
        for (int i = j + 1; i < cols; i++) {
            double s = G[i * ld + j];
            for (int k = 0; k < j; k++) s -= G[i * ld + k] * G[j * ld + k];
            G[i * ld + j] = s / d;
        }
        if (j >= ds.nx + ds.nc) rm++;
        else if (j >= ds.nx) rc++;
    }
    if (!f.usable) rc = rm = 0;
    f.rank_cof = rc;
    f.rank     = rm;
    return f;
}

struct QtlcofCell {
    double rss0, lod_base, lod;
};

// One (marker, column) cell: L the factor qtlcof_factor left (stride ld), b = X'y (QTL2_W values, stride bs; zero past the
// design's width), yy = sum c y^2.  A chromosome that is not scanned, or a column with RSS0 <= 0: LODs 0 and effects NaN.
// With want_coef, b is the cell's working row as well: on return b[j] of the marker's columns j = nx + nc .. w - 1 holds the
// effect in the full model, NaN for a dropped one.  The forward substitution keeps its vector in registers (every column
// needs it); the back-substitution, which only the observed columns need, runs in the row.
CNF2_HD QtlcofCell qtlcof_cell(const double* L, int ld, const QtlcofDesign& ds, const QtlcofFactor& f, double* b, int bs, double yy,
                               int n_c, bool want_coef)
{
    QtlcofCell r;
    r.rss0 = r.lod_base = r.lod = 0.0;
    const int m0  = ds.nx + ds.nc;
    bool      fit = f.usable != 0;
    if (fit) {
        double w[QTLCOF_MAXW];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
CNF2_QTL_UNROLL
        for (int j = 0; j < QTLCOF_MAXW; j++) {
            const double p = L[j * ld + j];
            double       s = b[j * bs];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTLCOF_MAXW; k++)
                if (k < j) s -= L[j * ld + k] * w[k];
            w[j]           = p > 0.0 ? s / p : 0.0;
            const double q = w[j] * w[j];
            if (j < ds.nx) s0 += q;
            else if (j < m0) s1 += q;
            else s2 += q;
        }
        r.rss0 = yy - s0;
        fit    = r.rss0 > 0.0;
        if (fit) {
            r.lod_base = qtl2_lod(s1, r.rss0, n_c);
            if (f.rank > 0) {
                const double d = qtl2_lod(s1 + s2, r.rss0, n_c) - r.lod_base;
                r.lod          = d > 0.0 ? d : 0.0;
            }
        }
        if (want_coef && fit) {
CNF2_QTL_UNROLL
            for (int j = 0; j < QTLCOF_MAXW; j++) b[j * bs] = w[j];
        }
    }
    if (!want_coef) return r;
    if (!fit) {
CNF2_QTLX_ROLLED
        for (int j = m0; j < ds.w; j++) b[j * bs] = (double)NAN;
        return r;
    }
    // L' beta = w on the marker's columns, the last of the design; a dropped column (pivot 0) takes no part
CNF2_QTLX_ROLLED
    for (int j = ds.w - 1; j >= m0; j--) {
        const double p = L[j * ld + j];
        double       s = b[j * bs];
CNF2_QTLX_ROLLED
        for (int k = j + 1; k < ds.w; k++)
            if (L[k * ld + k] > 0.0) s -= L[k * ld + j] * b[k * bs];
        b[j * bs] = p > 0.0 ? s / p : (double)NAN;
    }
    return r;
}

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlcof_kernels.hip read and write (device pointers)
struct QtlcofParams {
    int n, M, C, T, P, K, Q, additive;
    const double*   origin;       // [n][M][4]
    const double*   cov;          // [n][K] every covariate minus its mean over the used individuals
    const uint8_t*  use;          // [n]
    const int32_t*  cs;           // [C + 1] chromstarts
    const int32_t*  cof;          // [Q] the cofactors' markers
    const int32_t*  cofstart;     // [Q] the first marker of each cofactor's chromosome
    const uint32_t* skipw;        // [M] bit q: cofactor q is left out at the marker
    double*         cofimg;       // [n][ne Q] the cofactor columns (qtlcof_gather_kernel)
    uint8_t*        cmask;        // [C][n]: use[i], not skipped on the chromosome nor on any cofactor's (qtlcof_mask_kernel)
    int32_t*        nc;           // [C] n_c
    // the column tile: columns [r0, r0 + rn) of the R = T (1 + P)
    int             r0, rn, rstride;
    const double*   Y;            // [n][rstride] the column image
    double*         yy;           // [C][rstride] sum c y^2
    const int32_t*  tiles;        // [n_tiles][4] chromosome, first marker, markers (<= QTLCOF_TILE), 0
    const int32_t*  tile_start;   // [C + 1]
    int             n_tiles;
    double*         tilemax;      // [n_tiles][rstride]
    double *        lod, *lod_base, *coef, *rss0, *pmax;
    int32_t *       rank, *rank_cof;
};
constexpr int QTLCOF_TILE = 16;   // markers per block of the marker kernel, all of one chromosome
void launch_qtlcof_mask(const QtlcofParams& q, hipStream_t stream);
void launch_qtlcof_gather(const QtlcofParams& q, hipStream_t stream);
void launch_qtlcof_null(const QtlcofParams& q, hipStream_t stream);
void launch_qtlcof_markers(const QtlcofParams& q, hipStream_t stream);
void launch_qtlcof_finish(const QtlcofParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
