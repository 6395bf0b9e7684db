// cnf2_qtlplan.h -- what the QTL scan entry points of cnf2_capi.hip decide on the host before they allocate or launch: the
// marker map as the kernels read it, the column tile, and the checks of permutations and values.  Pure functions of the
// map and a few numbers; plain C++ (no HIP, no context) so that they are unit-tested without a GPU
// (tests/test_qtl_plan_host.py, through cnf2h_qtl_marker_map and cnf2h_qtl_column_tile of include/cnf2host.h).
#ifndef CNF2_QTLPLAN_H
#define CNF2_QTLPLAN_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace cnf2 {

// ------------------------------------------------------------------------------------------------ marker map
// The image a scan uploads, in int32 words:
//   header   whole_map_header: chromstarts[0 .. n_chrom] of the whole map; else the first marker of every chromosome of
//            the range chrom_begin .. chrom_end-1
//   mchrom   with_mchrom (whole_map_header only): the chromosome of every marker of the map           (at o_mchrom)
//   tiles    {c, m, len, 0} per tile of at most `tile` markers m .. m+len-1 of the range's chromosomes in order; no
//            tile straddles a chromosome start; c counts from 0 (whole_map_header) or from chrom_begin  (at o_tiles)
//   tstart   per chromosome of the range, and one past the last, the index of its first tile           (at o_tstart)
// What a caller appends to `image` follows the tile starts.
struct QtlMarkerMap {
    std::vector<int32_t> image;
    size_t               o_mchrom = 0, o_tiles = 0, o_tstart = 0, n_tiles = 0;
};

inline QtlMarkerMap qtl_marker_map(const int32_t* chromstarts, int n_chrom, int chrom_begin, int chrom_end, int tile, bool with_mchrom,
                                   bool whole_map_header)
{
    QtlMarkerMap          r;
    std::vector<int32_t>& map = r.image;
    if (whole_map_header) map.assign(chromstarts, chromstarts + n_chrom + 1);
    else map.assign(chromstarts + chrom_begin, chromstarts + chrom_end);
    r.o_mchrom = map.size();
    if (whole_map_header && with_mchrom)
        for (int c = 0; c < n_chrom; c++) map.insert(map.end(), (size_t)(chromstarts[c + 1] - chromstarts[c]), c);
    r.o_tiles = map.size();
    std::vector<int32_t> tstart(1, 0);
    for (int c = chrom_begin; c < chrom_end; c++) {
        const int32_t e = chromstarts[c + 1];
        for (int32_t m = chromstarts[c]; m < e; m += tile, r.n_tiles++) {
            const int32_t rec[4] = {whole_map_header ? c : c - chrom_begin, m, std::min<int32_t>(tile, e - m), 0};
            map.insert(map.end(), rec, rec + 4);
        }
        tstart.push_back((int32_t)r.n_tiles);
    }
    r.o_tstart = map.size();
    map.insert(map.end(), tstart.begin(), tstart.end());
    return r;
}

// ------------------------------------------------------------------------------------------------ column tile
// The columns (traits and their permutations, R in all) a scan takes per pass: as many as keep the column image
// Y[n][tile] under 1 GB, at least 16 and at most 4096; with permutations (P > 0) as many as keep the maxima under 256 MB,
// of which a scan holds maxima_doubles_per_column doubles per column (0: it has no such bound), at least 16; at most R;
// at most the caller's cap (cnf2_set_*_columns, 0 = none).
inline size_t qtl_column_tile(size_t n, size_t R, size_t P, size_t maxima_doubles_per_column, int cap)
{
    size_t rt = std::max<size_t>(16, ((size_t)1 << 30) / (8 * std::max<size_t>(1, n)));
    rt        = std::min(rt, (size_t)4096);
    if (P > 0 && maxima_doubles_per_column > 0) rt = std::min(rt, std::max<size_t>(16, ((size_t)1 << 28) / (8 * maxima_doubles_per_column)));
    rt = std::min(rt, R);
    if (cap > 0) rt = std::min(rt, (size_t)cap);
    return rt;
}

// The groups the multi-trait scan takes per pass out of G (the observed data and P permutations, T traits each): the rule
// above in whole groups.  A group is T columns padded to 4, 8 or 16; as many groups as keep the padded image under 1 GB (16
// to 4096 columns of it), at least one; with permutations as many as keep the maxima, n_tiles doubles per group, under
// 256 MB, at least one; at most G; at most the caller's cap (cnf2_set_qtlmv_groups, 0 = none).
inline size_t qtl_group_tile(size_t n, size_t T, size_t G, size_t P, size_t n_tiles, int cap)
{
    const size_t w = T <= 4 ? 4 : (T <= 8 ? 8 : 16);
    size_t       gt = std::max<size_t>(1, qtl_column_tile(n, std::max<size_t>(1, G) * w, 0, 0, 0) / w);
    if (P > 0 && n_tiles > 0) gt = std::min(gt, std::max<size_t>(1, ((size_t)1 << 28) / (8 * n_tiles)));
    gt = std::min(gt, std::max<size_t>(1, G));
    if (cap > 0) gt = std::min(gt, (size_t)cap);
    return gt;
}

// The replicates the bootstrap scan takes per pass: a multiple of 16 that keeps the weight image W[n][tile] under 1 GB, at
// least 16 and at most 4096; at most the B replicates rounded up to 16.
inline size_t qtl_replicate_tile(size_t n, size_t B)
{
    const size_t bt = std::max<size_t>(16, ((size_t)1 << 30) / (8 * std::max<size_t>(1, n)) / 16 * 16);
    return std::min(std::min(bt, (size_t)4096), (B + 15) / 16 * 16);
}

// ------------------------------------------------------------------------------------------------ checks
// The callers turn a code and its indices into their message.
enum { QTL_INPUT_OK = 0, QTL_PHENO_NOT_FINITE, QTL_COV_NOT_FINITE, QTL_NOT_A_PERMUTATION, QTL_PERM_TAKES_UNUSED };

// pheno[n][T] and cov[n][K] of the used individuals (use[n], NULL = all) must be finite: *bad_i the individual, *bad_col
// the trait or covariate
inline int qtl_check_finite(int n, int T, const double* pheno, int K, const double* cov, const uint8_t* use, int* bad_i, int* bad_col)
{
    for (int i = 0; i < n; i++) {
        if (use && !use[i]) continue;
        for (int t = 0; t < T; t++)
            if (!std::isfinite(pheno[(size_t)i * T + t])) return *bad_i = i, *bad_col = t, QTL_PHENO_NOT_FINITE;
        for (int k = 0; k < K; k++)
            if (!std::isfinite(cov[(size_t)i * K + k])) return *bad_i = i, *bad_col = k, QTL_COV_NOT_FINITE;
    }
    return QTL_INPUT_OK;
}

// every row of perm[P][n] must be a permutation of 0 .. n-1 that gives a used individual (use[n], NULL = all) a used one:
// *bad_row the row, and for QTL_PERM_TAKES_UNUSED *bad_i the used individual and *bad_j the unused one it is given
inline int qtl_check_permutations(int n, int P, const int32_t* perm, const uint8_t* use, int* bad_row, int* bad_i, int* bad_j)
{
    std::vector<uint8_t> seen(n);
    for (int p = 0; p < P; p++) {
        std::fill(seen.begin(), seen.end(), 0);
        const int32_t* row = perm + (size_t)p * n;
        for (int i = 0; i < n; i++) {
            const int32_t j = row[i];
            if (j < 0 || j >= n || seen[j]) return *bad_row = p, QTL_NOT_A_PERMUTATION;
            seen[j] = 1;
            if (use && use[i] && !use[j]) return *bad_row = p, *bad_i = i, *bad_j = j, QTL_PERM_TAKES_UNUSED;
        }
    }
    return QTL_INPUT_OK;
}

}  // namespace cnf2
#endif  // CNF2_QTLPLAN_H
