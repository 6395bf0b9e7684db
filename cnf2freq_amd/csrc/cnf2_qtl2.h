// cnf2_qtl2.h -- the small dense algebra of the two-QTL pair scan (cnf2_qtl_scan2, include/cnf2hip.h), shared by host and
// device code: which columns a pair's design has, the sequential Cholesky factor of its normal matrix with the rank rule,
// and the clamps and logarithms of one (pair, column) cell.  The kernels of cnf2_qtl2_kernels.hip form the sums; every
// decision that gives the result its meaning is taken here.
//
// Three nested Haley-Knott designs under the mask c of a chromosome pair, in this column order:
//   null      X0 = [c, c z_1 .. c z_K]
//   additive  X0, a1, d1, a2, d2                                (CNF2_QTL_ADDITIVE: X0, a1, a2)
//   full      additive, then a1 a2, a1 d2, d1 a2, d1 d2         (CNF2_QTL_ADDITIVE: additive, then a1 a2)
// with a = origin[3] - origin[0], d = origin[1] + origin[2] at the pair's two loci.  cnf2_qtl_scan2 fits the full design only
// where the loci lie on different chromosomes: there the expectation of a product is the product of the expectations.
// cnf2_qtl_scan2_linked fits it on one chromosome too, with the interaction columns' expectations taken from the pair's joint
// row (qtl2_joint_cells below); for the design, the factor and the cell such a pair is then "not on one chromosome".  One Cholesky
// factor L of the full design's normal matrix in that order gives all three: with w = L^-1 X'y over the kept columns
//   RSS0 = sum c y^2 - sum_{X0} w^2,  RSS_add = RSS0 - sum_{kept additive} w^2,  RSS_full = RSS_add - sum_{kept interaction} w^2.
#ifndef CNF2_QTL2_H
#define CNF2_QTL2_H

#include "cnf2_qtl.h"

namespace cnf2 {

constexpr int QTL2_MAXK = 6;                 // covariates at most: 1 + K + 8 <= 15 columns
constexpr int QTL2_W    = 16;                // rows of one matrix instruction: the design's width at most, padded with zeros
constexpr int QTL2_MAXL = 4096;              // selected loci at most

// the widths of a pair's design
struct Qtl2Design {
    int nx, nadd, nint;      // columns of X0, additive columns of the two loci, interaction columns
};
CNF2_HD Qtl2Design qtl2_design(int K, bool additive, bool same_chrom)
{
    Qtl2Design ds;
    ds.nx   = K + 1;
    ds.nadd = additive ? 2 : 4;
    ds.nint = same_chrom ? 0 : (additive ? 1 : 4);
    return ds;
}

// What column j of the design is, as a product u v of a locus-1 side and a locus-2 side:
//   u: 0 = 1, 1 = covariate j - 1, 2 = a1, 3 = d1, 4 = nothing (the column is zero);  v: 0 = 1, 1 = a2, 2 = d2
CNF2_HD void qtl2_column(const Qtl2Design& ds, bool additive, int j, int* u, int* v)
{
    *u = 4;
    *v = 0;
    if (j < 0) return;
    if (j < ds.nx) {
        *u = j == 0 ? 0 : 1;
        return;
    }
    const int e = j - ds.nx;
    if (e >= ds.nadd + ds.nint) return;
    if (additive) {
        *u = e == 1 ? 0 : 2;
        *v = e == 0 ? 0 : 1;
    } else if (e < 4) {
        *u = e < 2 ? 2 + e : 0;
        *v = e < 2 ? 0 : e - 1;
    } else {
        *u = 2 + ((e - 4) >> 1);
        *v = 1 + ((e - 4) & 1);
    }
}

// A pair on one chromosome with its joint row J[4 u + v] = P(class u at locus 1, class v at locus 2) (cnf2_sweep_pairs;
// cnf2_qtl_scan2_linked): the expectation of an interaction column under it.  a is +1 on class 3 and -1 on class 0, d is 1 on
// classes 1 and 2:
//   E[a1 a2] = J33 + J00 - J30 - J03     E[a1 d2] = J31 + J32 - J01 - J02     E[d1 a2] = J13 + J23 - J10 - J20
//   E[d1 d2] = J11 + J12 + J21 + J22
// cell[0 .. 3]: the four cells, of which the last *neg are subtracted; the value is (J[0] + J[1]) -/+ (J[2] + J[3])
CNF2_HD void qtl2_joint_cells(bool dom1, bool dom2, int (&cell)[4], int* neg)
{
    if (dom1 && dom2) cell[0] = 5, cell[1] = 6, cell[2] = 9, cell[3] = 10, *neg = 0;
    else if (dom1) cell[0] = 7, cell[1] = 11, cell[2] = 4, cell[3] = 8, *neg = 2;
    else if (dom2) cell[0] = 13, cell[1] = 14, cell[2] = 1, cell[3] = 2, *neg = 2;
    else cell[0] = 15, cell[1] = 0, cell[2] = 12, cell[3] = 3, *neg = 2;
}
CNF2_HD double qtl2_joint_value(double j0, double j1, double j2, double j3, int neg)
{
    return neg ? (j0 + j1) - (j2 + j3) : (j0 + j1) + (j2 + j3);
}

struct Qtl2Factor {
    int usable;              // the chromosome pair is scanned: n_c >= K + 10 and X0 has a Cholesky factor
    int rank_add, rank_full; // kept added columns; rank_full = -1 for a pair on one chromosome
};

// G (lower triangle of the normal matrix, row-major with stride ld, QTL2_W rows) <- its sequential Cholesky factor in the
// column order of the design.  A column of X0 must have a positive pivot (else the pair is not scanned); an added column is
// dropped -- pivot 0 and a zero column in L -- when its raw diagonal is 0 or its pivot is below QTL_PIVOT times its raw
// diagonal.  Rows past the design's width are zero on entry and on return.
CNF2_HD Qtl2Factor qtl2_factor(double* G, int ld, const Qtl2Design& ds, int n_c, int K, bool same_chrom)
{
    Qtl2Factor f;
    f.usable    = n_c >= K + 10 ? 1 : 0;
    f.rank_add  = 0;
    f.rank_full = same_chrom ? -1 : 0;
    const int W = ds.nx + ds.nadd + ds.nint;
    for (int j = 0; j < W && f.usable; j++) {
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
            for (int i = j; i < W; i++) G[i * ld + j] = 0.0;
            continue;
        }
        d             = sqrt(d);
        G[j * ld + j] = d;
        for (int i = j + 1; i < W; i++) {
            double s = G[i * ld + j];
            for (int k = 0; k < j; k++) s -= G[i * ld + k] * G[j * ld + k];
            G[i * ld + j] = s / d;
        }
        if (j >= ds.nx + ds.nadd) f.rank_full++;
        else if (j >= ds.nx) f.rank_add++;
    }
    if (!f.usable) {
        f.rank_add  = 0;
        f.rank_full = same_chrom ? -1 : 0;
    } else if (!same_chrom)
        f.rank_full += f.rank_add;
    return f;
}

struct Qtl2Cell {
    double rss0, lod_add, lod_full;
};

// (n_c / 2) log10(RSS0 / (RSS0 - d)) with d clamped to [0, RSS0 (1 - 2^-52)]: finite and not negative
CNF2_HD double qtl2_lod(double d, double rss0, int n_c)
{
    const double hi = rss0 * (1.0 - 2.220446049250313e-16);
    d               = d < 0.0 ? 0.0 : (d > hi ? hi : d);
    return d > 0.0 ? 0.5 * (double)n_c * log10(rss0 / (rss0 - d)) : 0.0;
}

// One (pair, column) cell: L the factor qtl2_factor left (stride ld), b = X'y (QTL2_W values, stride bs; zero past the
// design's width), yy = sum c y^2.  A pair that is not scanned, or a column with RSS0 <= 0: LOD 0.  lod_full is NaN for a
// pair on one chromosome, whatever else holds.
CNF2_HD Qtl2Cell qtl2_cell(const double* L, int ld, const Qtl2Design& ds, const Qtl2Factor& f, const double* b, int bs, double yy,
                           int n_c, bool same_chrom)
{
    Qtl2Cell r;
    r.rss0     = 0.0;
    r.lod_add  = 0.0;
    r.lod_full = same_chrom ? (double)NAN : 0.0;
    if (!f.usable) return r;
    double w[QTL2_W - 1];
    double s0 = 0.0, sa = 0.0, si = 0.0;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL2_W - 1; j++) {
        const double p = L[j * ld + j];
        double       s = b[j * bs];
CNF2_QTL_UNROLL
        for (int k = 0; k < QTL2_W - 1; k++)
            if (k < j) s -= L[j * ld + k] * w[k];
        w[j]           = p > 0.0 ? s / p : 0.0;
        const double q = w[j] * w[j];
        if (j < ds.nx) s0 += q;
        else if (j < ds.nx + ds.nadd) sa += q;
        else si += q;
    }
    r.rss0 = yy - s0;
    if (!(r.rss0 > 0.0)) return r;
    r.lod_add = qtl2_lod(sa, r.rss0, n_c);
    if (!same_chrom) r.lod_full = qtl2_lod(sa + si, r.rss0, n_c);
    return r;
}

#if defined(__HIPCC__)
// What the kernels of cnf2_qtl2_kernels.hip read and write (device pointers)
struct Qtl2Params {
    int n, M, C, T, P, K, L, additive;
    const double*  origin;       // [n][M][4]
    const double*  pheno;        // [n][T]
    const double*  cov;          // [n][K]
    const uint8_t* use;          // [n]
    const int32_t* perm;         // [P][n]
    const int32_t* cs;           // [C + 1] chromstarts
    const int32_t* sel;          // [L] the selected markers
    const int32_t* selchrom;     // [L] their chromosomes
    uint8_t*       cmask;        // [C][n]: use[i] and the row at the chromosome's first marker is not all zero
    int32_t*       nc;           // [C][C] n_c
    // the column tile: columns [r0, r0 + rn) of the R = T (1 + P)
    int            r0, rn, rstride;
    double*        Y;            // [n][rstride] the column image
    double*        yy;           // [C][C][rstride] sum c y^2 (c1 <= c2)
    int            n_chunks;     // chunks of QTL2_CHUNK second loci per first locus
    double*        chunkmax;     // [L][n_chunks][3][rstride]
    double *       lod_add, *lod_full, *rss0, *pmax;
    int32_t *      rank_add, *rank_full;
    // cnf2_qtl_scan2_linked (null / 0 otherwise): the joint rows of the pairs on one chromosome, pair (j, k) at row
    // pair_off[j] + k - j - 1 of an individual's n_pairs
    const double*  joint;        // [n][n_pairs][16]
    const int32_t* pair_off;     // [L]
    int            n_pairs;
};
constexpr int QTL2_CHUNK = 64;   // second loci per block of the pair kernel
void launch_qtl2_mask(const Qtl2Params& q, hipStream_t stream);
void launch_qtl2_fill(const Qtl2Params& q, hipStream_t stream);
void launch_qtl2_gather(const Qtl2Params& q, hipStream_t stream);
void launch_qtl2_null(const Qtl2Params& q, hipStream_t stream);
void launch_qtl2_pairs(const Qtl2Params& q, hipStream_t stream);
void launch_qtl2_finish(const Qtl2Params& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
