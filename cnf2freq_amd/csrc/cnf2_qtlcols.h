// cnf2_qtlcols.h -- what the kernels of cnf2_qtlcols_kernels.hip read and write (cnf2_qtl_scan_cols, include/cnf2hip.h): the
// Haley-Knott product on prepared columns.  Ordinary least squares of phenotype columns, observed and permuted, on
// [x0, s_i reg(i, m, 0 .. ne-1)] at every marker of one block: x0 is the whole null design as the caller gives it (no
// implicit intercept, no centring), the regressors are doubles, and s scales their rows on the fly.  The algebra and every
// decision about a cell are cnf2_qtl.h's (qtl_cholesky, qtl_marker_record, qtl_cell); with ne = 1 the second column is the
// additive model's dropped one.
#ifndef CNF2_QTLCOLS_H
#define CNF2_QTLCOLS_H

#include "cnf2_qtl.h"

namespace cnf2 {

#if defined(__HIPCC__)
struct QtlColsParams {
    int n, M, ne, T, P, nx;      // individuals, markers of the block, regressors per marker, traits, permutations, columns of x0
    const double*  reg;          // [n][M][ne]
    const double*  scale;        // [n] or null
    const double*  x0;           // [n][nx]
    const double*  pheno;        // [n][T]
    const int32_t* perm;         // [P][n]
    double*        chol;         // [QTL_CHOL]
    double*        mk;           // [M][QTL_MK]
    int32_t*       rank;         // [M]
    // the column tile: columns [r0, r0 + rn) of the R = T (1 + P)
    int            r0, rn, rstride;
    double*        Y;            // [n][rstride] the column image
    double*        nullq;        // [nx + 1][rstride]: b0, then RSS0
    int            n_tiles;      // marker tiles of 16
    double*        tilemax;      // [n_tiles][rstride]
    double *       lod, *coef, *rss0, *pmax;
};
void launch_qtlcols_null(const QtlColsParams& q, hipStream_t stream);
void launch_qtlcols_design(const QtlColsParams& q, hipStream_t stream);
void launch_qtlcols_gather(const QtlColsParams& q, hipStream_t stream);
void launch_qtlcols_colnull(const QtlColsParams& q, hipStream_t stream);
void launch_qtlcols_scan(const QtlColsParams& q, hipStream_t stream);
void launch_qtlcols_finish(const QtlColsParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
