// cnf2_qtlx.h -- the small dense algebra of the extended single-locus scan (cnf2_qtl_scanx, include/cnf2hip.h), shared by
// host and device code: which columns a marker's design has, the sequential Cholesky factor of its normal matrix with the
// rank rule, and the substitutions, clamps and logarithms of one (marker, column) cell.  The kernels of
// cnf2_qtlx_kernels.hip form the sums; every decision that gives the result its meaning is taken here.
//
// Nested Haley-Knott designs under the mask c of a chromosome, with a = o[3] - o[0], d = o[1] + o[2], i = o[1] - o[2] of the
// marker's origin row o, and the first Ki of the K covariates interactive.  In this column order:
//   null          X0 = [c, c z_1 .. c z_K]
//   stage 0       a, d                                  "Mendelian"    (CNF2_QTL_ADDITIVE: a)
//   stage 1       i                                     "imprinting"   (only with CNF2_QTL_IMPRINT)
//   stage 2       for k = 1 .. Ki: a z_k, d z_k, i z_k  "interaction"  (those effects that are present)
// One Cholesky factor L of the whole design's normal matrix in that order gives every stage: with w = L^-1 X'y over the kept
// columns, RSS0 = sum c y^2 - sum_{X0} w^2 and the reduction after stage s is the sum of w^2 over the kept columns of the
// stages 0 .. s.  The effects of the full model come from the back-substitution L' beta = w on the added columns.
#ifndef CNF2_QTLX_H
#define CNF2_QTLX_H

#include "cnf2_qtl2.h"

namespace cnf2 {

constexpr int QTLX_MAXW = QTL2_W - 1;        // the design's width at most: the rows of one matrix instruction less the padding row
constexpr int QTLX_NSTAT = 5;                // lod[0], lod[1], lod[2], lod[1] - lod[0], lod[2] - lod[1]

// the effect code of a column: what is taken from the origin row
constexpr int QTLX_ONE = 0, QTLX_A = 1, QTLX_D = 2, QTLX_I = 3, QTLX_NONE = 4;

struct QtlxDesign {
    int nx;          // columns of X0
    int ne;          // effects: a, then d (unless additive), then i (with imprinting)
    int ki;          // interactive covariates: the first ki of the K
    int ns[3];       // added columns of the three stages
    int w;           // all columns
    int eff[3];      // the effect codes in their order
};
CNF2_HD QtlxDesign qtlx_design(int K, int Ki, bool additive, bool imprint)
{
    QtlxDesign ds;
    ds.nx = K + 1;
    ds.ki = Ki;
    ds.ne = 1 + (additive ? 0 : 1) + (imprint ? 1 : 0);
    ds.eff[0] = QTLX_A;
    ds.eff[1] = additive ? (imprint ? QTLX_I : QTLX_NONE) : QTLX_D;
    ds.eff[2] = (!additive && imprint) ? QTLX_I : QTLX_NONE;
    ds.ns[0] = additive ? 1 : 2;
    ds.ns[1] = imprint ? 1 : 0;
    ds.ns[2] = ds.ne * Ki;
    ds.w     = ds.nx + ds.ne * (1 + Ki);
    return ds;
}

// What column j of the design is, as a product (effect of the origin row) x (modifier):
//   *e: QTLX_ONE = 1, QTLX_A, QTLX_D, QTLX_I, QTLX_NONE = nothing (the column is zero);  *z: 0 = 1, k >= 1 = covariate k - 1
// so the mask column is (ONE, 0), covariate k is (ONE, k), a main effect (e, 0) and an interaction (e, k).
CNF2_HD void qtlx_column(const QtlxDesign& ds, int j, int* e, int* z)
{
    *e = QTLX_NONE;
    *z = 0;
    if (j < 0 || j >= ds.w) return;
    if (j < ds.nx) {
        *e = QTLX_ONE;
        *z = j;
        return;
    }
    const int q = j - ds.nx, k = q / ds.ne, r = q - k * ds.ne;
    *e = r == 0 ? ds.eff[0] : (r == 1 ? ds.eff[1] : ds.eff[2]);
    *z = k;
}

// the stage (0, 1, 2) of the added column j >= nx
CNF2_HD int qtlx_stage(const QtlxDesign& ds, int j)
{
    const int q = j - ds.nx;
    return q < ds.ns[0] ? 0 : (q < ds.ns[0] + ds.ns[1] ? 1 : 2);
}

struct QtlxFactor {
    int usable;      // the chromosome is scanned: n_c >= W + 1 and X0 has a Cholesky factor
    int rank[3];     // kept added columns, cumulative over the stages
};

// G (lower triangle of the normal matrix, row-major with stride ld, QTL2_W rows) <- its sequential Cholesky factor in the
// column order of the design, by qtl2_factor's rule: a column of X0 must have a positive pivot (else the chromosome is not
// scanned); an added column is dropped -- pivot 0 and a zero column in L -- when its raw diagonal is 0 or its pivot is below
// QTL_PIVOT times its raw diagonal.  Only the first `cols` columns are factored (nx: the null design alone); whether the
// chromosome is scanned is decided by the whole design's width.
CNF2_HD QtlxFactor qtlx_factor(double* G, int ld, const QtlxDesign& ds, int n_c, int cols)
{
    QtlxFactor f;
    f.usable  = n_c >= ds.w + 1 ? 1 : 0;
    int r0 = 0, r1 = 0, r2 = 0;
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
        if (j >= ds.nx) {
            const int st = qtlx_stage(ds, j);
            r0 += st == 0 ? 1 : 0;
            r1 += st == 1 ? 1 : 0;
            r2 += st == 2 ? 1 : 0;
        }
    }
    if (!f.usable) r0 = r1 = r2 = 0;
    f.rank[0] = r0;
    f.rank[1] = r0 + r1;
    f.rank[2] = r0 + r1 + r2;
    return f;
}

struct QtlxCell {
    double rss0, lod[3];
};

// (a loop that must stay a loop in device code: its vector lives in memory, not in registers)
#if defined(__HIPCC__)
#define CNF2_QTLX_ROLLED _Pragma("unroll 1")
#else
#define CNF2_QTLX_ROLLED
#endif

// One (marker, column) cell: L the factor qtlx_factor left (stride ld), b = X'y (QTL2_W values, stride bs; zero past the
// design's width), yy = sum c y^2.  A chromosome that is not scanned, or a column with RSS0 <= 0: LODs 0 and effects NaN.
// With want_coef, b is the cell's working row as well: on return b[j] of every added column j holds the effect of the full
// model, NaN for a dropped one.  The forward substitution keeps its vector in registers (every column needs it); the
// back-substitution, which only the observed columns need, runs in the row.
CNF2_HD QtlxCell qtlx_cell(const double* L, int ld, const QtlxDesign& ds, const QtlxFactor& f, double* b, int bs, double yy, int n_c,
                           bool want_coef)
{
    QtlxCell r;
    r.rss0   = 0.0;
    r.lod[0] = r.lod[1] = r.lod[2] = 0.0;
    bool fit = f.usable != 0;
    if (fit) {
        double w[QTLX_MAXW];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        const int e0 = ds.nx + ds.ns[0], e1 = e0 + ds.ns[1];
CNF2_QTL_UNROLL
        for (int j = 0; j < QTLX_MAXW; j++) {
            const double p = L[j * ld + j];
            double       s = b[j * bs];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTLX_MAXW; k++)
                if (k < j) s -= L[j * ld + k] * w[k];
            w[j]           = p > 0.0 ? s / p : 0.0;
            const double q = w[j] * w[j];
            if (j < ds.nx) s0 += q;
            else if (j < e0) s1 += q;
            else if (j < e1) s2 += q;
            else s3 += q;
        }
        r.rss0 = yy - s0;
        fit    = r.rss0 > 0.0;
        if (fit) {
            r.lod[0] = qtl2_lod(s1, r.rss0, n_c);
            r.lod[1] = ds.ns[1] > 0 ? qtl2_lod(s1 + s2, r.rss0, n_c) : r.lod[0];
            r.lod[2] = ds.ns[2] > 0 ? qtl2_lod(s1 + s2 + s3, r.rss0, n_c) : r.lod[1];
        }
        if (want_coef && fit) {
CNF2_QTL_UNROLL
            for (int j = 0; j < QTLX_MAXW; j++) b[j * bs] = w[j];
        }
    }
    if (!want_coef) return r;
    if (!fit) {
CNF2_QTLX_ROLLED
        for (int j = ds.nx; j < ds.w; j++) b[j * bs] = (double)NAN;
        return r;
    }
    // L' beta = w from the last column up to the first added one; a dropped column (pivot 0) takes no part
CNF2_QTLX_ROLLED
    for (int j = ds.w - 1; j >= ds.nx; j--) {
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
// What the kernels of cnf2_qtlx_kernels.hip read and write (device pointers)
struct QtlxParams {
    int n, M, C, T, P, K, Ki, additive, imprint;
    const double*  origin;       // [n][M][4]
    const double*  cov;          // [n][K] the columns of X0: every covariate minus its mean over the used individuals
    const double*  cov_raw;      // [n][K] the covariates as given: the modifiers z_k of the interaction columns
    const uint8_t* use;          // [n]
    const int32_t* cs;           // [C + 1] chromstarts
    const uint8_t* cmask;        // [C][n]: use[i] and the row at the chromosome's first marker is not all zero (qtl2_mask_kernel)
    int32_t*       nc;           // [C] n_c
    // the column tile: columns [r0, r0 + rn) of the R = T (1 + P)
    int            r0, rn, rstride;
    const double*  Y;            // [n][rstride] the column image
    double*        yy;           // [C][rstride] sum c y^2
    const int32_t* tiles;        // [n_tiles][4] chromosome, first marker, markers (<= QTLX_TILE), 0
    const int32_t* tile_start;   // [C + 1]
    int            n_tiles;
    double*        tilemax;      // [n_tiles][QTLX_NSTAT][rstride]
    double *       lod, *coef, *rss0, *pmax;
    int32_t*       rank;
};
constexpr int QTLX_TILE = 16;    // markers per block of the marker kernel, all of one chromosome
void launch_qtlx_null(const QtlxParams& q, hipStream_t stream);
void launch_qtlx_markers(const QtlxParams& q, hipStream_t stream);
void launch_qtlx_finish(const QtlxParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
