// cnf2_qtlfam.h -- the within-family QTL scan (cnf2_qtl_scan_fam, include/cnf2hip.h), shared by host and device code: the
// regressor of a side, the fitted rule of a family, the elimination of the families' diagonal block, the clamps and logarithm
// of one (marker, column) cell, the gather list the kernels walk, one marker fitted serially on the CPU, and what the kernels
// of cnf2_qtlfam_kernels.hip read and write.  The Cholesky factor of the null design is cnf2_qtl.h's.
//
// The nested (half-sib) model of Knott, Elsen and Haley (1996).  Individual i belongs to slope group grp[i] = 0 .. F-1 (the F1
// parent on the side; < 0: not nested, not used) and to mean cell cell[i] (NULL: grp); all members of a cell share one grp.
// Per chromosome c_i = use[i] and grp[i] >= 0 and the row at the chromosome's first marker is not all zero; n_c = sum c_i.
// Every column v -- a trait, a permuted trait, a covariate -- is centred within cells, v~_i = c_i (v_i - mean of v over the used
// members of cell(i)), which eliminates the cells' dummies.  S11 = Z~'Z~ (K x K), b0 = Z~'y~, yy = y~'y~,
// RSS0 = yy - b0' S11^-1 b0.  A chromosome is not scanned when S11 has no Cholesky factor or n_c - n_cells_used - K < 2.
// Per marker x_i = c_i (o1 + o3 - o0 - o2) for side 0 and c_i (o2 + o3 - o0 - o1) for side 1: bit 0 / bit 3 of the origin
// sweep's absolute frame as +-1.  Per family p, over its used members:
//   d_p = sum over the cells q of p (sum x^2 - (sum x)^2 / n_q),  raw_p = sum x^2,  u_p = sum x_i z~_i,  r_p = sum x_i y~_i.
// A family is fitted when raw_p > 0 and d_p >= 1e-8 raw_p; df = the fitted families.  The slope block of the normal matrix is
// diagonal (d_p), so it is eliminated family by family:
//   H = S11 - sum u_p u_p' / d_p,  g = b0 - sum u_p r_p / d_p,  gamma = H^-1 g,
//   RSS1 = yy - sum r_p^2 / d_p - g' gamma,  slope_p = (r_p - u_p' gamma) / d_p,
// the sums over the fitted families in ascending order.  dRSS = RSS0 - RSS1 = sum r_p^2 / d_p + g' gamma - b0' S11^-1 b0 is
// clamped to [0, RSS0 (1 - 2^-52)] and lod = (n_c / 2) log10(RSS0 / (RSS0 - dRSS)).  A marker whose H has no factor -- a pivot
// not positive or below QTL_PIVOT times S11's diagonal -- or with n_c - n_cells_used - K - df < 1 reports df 0, lod 0 and
// slopes NaN.  The records carry w_p = 1 / d_p (0 for a family that is not fitted) and u_p; every quotient by d_p above is a
// product with w_p.
// Every loop over the covariates has the constant bound QTL_MAXK and a predicate, so that the device code keeps its vectors
// in registers.
#ifndef CNF2_QTLFAM_H
#define CNF2_QTLFAM_H

#include "cnf2_qtl.h"

#include <algorithm>
#include <map>
#include <vector>

namespace cnf2 {

constexpr int QTLFAM_TRI   = QTL_MAXK * (QTL_MAXK + 1) / 2;   // the lower triangle of a K x K matrix, packed: (j, k) at j (j + 1) / 2 + k
constexpr int QTLFAM_CHROM = 2 * QTL_NX * QTL_NX + 1;         // doubles per chromosome: S11, its factor (both stride QTL_NX), 1.0 = scanned

CNF2_HD constexpr int qtlfam_tri(int j, int k) { return j * (j + 1) / 2 + k; }

// the regressor of a row (o0 .. o3) on a side: P(bit = 1) - P(bit = 0) of bit 0 (side 0) or bit 3 (side 1)
CNF2_HD double qtlfam_x(double o0, double o1, double o2, double o3, int side)
{
    return side == 0 ? (o1 + o3) - (o0 + o2) : (o2 + o3) - (o0 + o1);
}

// w_p = 1 / d_p of a family that is fitted, else 0
CNF2_HD double qtlfam_weight(double raw, double d) { return (raw > 0.0 && d >= QTL_PIVOT * raw) ? 1.0 / d : 0.0; }

// The mean of a cell's used values in two passes (cnf2_qtl.h qtl_column_mean: the mean of equal values is that value, so a
// column that is constant within a cell is centred to exactly 0).  val(s, &v) is false for a slot that is empty or masked.
template <class Val>
CNF2_HD double qtlfam_cell_mean(int s0, int s1, Val val)
{
    int    n_u = 0;
    double mean = 0.0, v;
    for (int s = s0; s < s1; s++) n_u += val(s, &v) ? 1 : 0;
    if (n_u == 0) return 0.0;
    for (int pass = 0; pass < 2; pass++) {
        double sum = 0.0;
        for (int s = s0; s < s1; s++)
            if (val(s, &v)) sum += v - mean;
        mean += sum / n_u;
    }
    return mean - mean == 0.0 ? mean : 0.0;
}

// H = L L' in place on the packed lower triangle; false when a pivot is not positive or below QTL_PIVOT times diag[j], the
// diagonal of S11 (the factor is then not used)
CNF2_HD bool qtlfam_factor(double H[QTLFAM_TRI], int K, const double diag[QTL_MAXK])
{
    bool ok = true;
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_MAXK; j++)
        if (j < K) {
            double d = H[qtlfam_tri(j, j)];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTL_MAXK; k++)
                if (k < j) d -= H[qtlfam_tri(j, k)] * H[qtlfam_tri(j, k)];
            ok = ok && d > 0.0 && d >= QTL_PIVOT * diag[j];
            d  = ok ? sqrt(d) : 1.0;
            H[qtlfam_tri(j, j)] = d;
CNF2_QTL_UNROLL
            for (int i = 0; i < QTL_MAXK; i++)
                if (i > j && i < K) {
                    double s = H[qtlfam_tri(i, j)];
CNF2_QTL_UNROLL
                    for (int k = 0; k < QTL_MAXK; k++)
                        if (k < j) s -= H[qtlfam_tri(i, k)] * H[qtlfam_tri(j, k)];
                    H[qtlfam_tri(i, j)] = s / d;
                }
        }
    return ok;
}

// x <- H^-1 x with H = L L', entry (j, k) of L at L[qtlfam_tri(j, k) * stride]
CNF2_HD void qtlfam_solve(const double* L, size_t stride, int K, double x[QTL_MAXK])
{
CNF2_QTL_UNROLL
    for (int j = 0; j < QTL_MAXK; j++)
        if (j < K) {
            double s = x[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTL_MAXK; k++)
                if (k < j) s -= L[(size_t)qtlfam_tri(j, k) * stride] * x[k];
            x[j] = s / L[(size_t)qtlfam_tri(j, j) * stride];
        }
CNF2_QTL_UNROLL
    for (int jj = 0; jj < QTL_MAXK; jj++) {
        const int j = QTL_MAXK - 1 - jj;
        if (j < K) {
            double s = x[j];
CNF2_QTL_UNROLL
            for (int k = 0; k < QTL_MAXK; k++)
                if (k > j && k < K) s -= L[(size_t)qtlfam_tri(k, j) * stride] * x[k];
            x[j] = s / L[(size_t)qtlfam_tri(j, j) * stride];
        }
    }
}

// One family's end: r = r_p of a column, w = w_p and u = u_p of the marker; sr2 += r^2 / d, gs += u r / d
template <int KB>
CNF2_HD void qtlfam_fold(double r, double w, const double u[KB], int K, double& sr2, double gs[KB])
{
    const double t = r * w;
    sr2 += r * t;
CNF2_QTL_UNROLL
    for (int k = 0; k < KB; k++)
        if (k < K) gs[k] += u[k] * t;
}

// One (marker, column) cell: sr2 = sum r_p^2 / d_p, gq = g' gamma, e0 = b0' S11^-1 b0.  ok: the chromosome is scanned, H has
// its factor and residual degrees of freedom are left.  The LOD is finite and not negative.
CNF2_HD double qtlfam_cell(double sr2, double gq, double e0, double rss0, int n_c, bool ok)
{
    if (!ok || !(rss0 > 0.0)) return 0.0;
    const double hi = rss0 * (1.0 - 2.220446049250313e-16);
    double       d  = (sr2 + gq) - e0;
    d               = d < 0.0 ? 0.0 : (d > hi ? hi : d);
    return d > 0.0 ? 0.5 * (double)n_c * log10(rss0 / (rss0 - d)) : 0.0;
}

// ------------------------------------------------------------------------------------------------ the gather list
// The used individuals (use[i] != 0 and grp[i] >= 0) ordered by (grp, cell, index), every cell padded with empty slots (-1)
// to a multiple of 4: a k-step of four slots never straddles two cells, and so never two families.
struct QtlFamLayout {
    std::vector<int32_t> gidx;        // [S] the individual of a slot, -1 for an empty one
    std::vector<int32_t> cellslot;    // [Q + 1] the first slot of a cell (cells in the order of the list)
    std::vector<int32_t> famcell;     // [F + 1] the first cell of a family
    std::vector<int32_t> stepend;     // [S / 4] 1 where a step of four slots is the last of its family
    std::vector<int32_t> folds;       // the families with slots in ascending order, the last once more (at least one word)
    std::vector<int32_t> cellof;      // [n] the cell of an individual, -1 for one that is not used
    int                  S = 0, Q = 0;
};
enum { QTLFAM_OK = 0, QTLFAM_GRP_RANGE, QTLFAM_CELL_NEGATIVE, QTLFAM_CELL_SPLIT, QTLFAM_PERM_LEAVES_CELL };

// *bad_i: the individual a refusal is about
inline int qtlfam_layout(int n, const uint8_t* use, const int32_t* grp, const int32_t* cell, int F, QtlFamLayout* out, int* bad_i)
{
    std::vector<int32_t>       order;
    std::map<int32_t, int32_t> owner;
    for (int i = 0; i < n; i++) {
        if ((use && !use[i]) || grp[i] < 0) continue;
        if (grp[i] >= F) return *bad_i = i, QTLFAM_GRP_RANGE;
        if (cell && cell[i] < 0) return *bad_i = i, QTLFAM_CELL_NEGATIVE;
        const int32_t key = cell ? cell[i] : grp[i];
        const auto    it  = owner.insert({key, grp[i]}).first;
        if (it->second != grp[i]) return *bad_i = i, QTLFAM_CELL_SPLIT;
        order.push_back(i);
    }
    auto key = [&](int32_t i) { return cell ? cell[i] : grp[i]; };
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        if (grp[a] != grp[b]) return grp[a] < grp[b];
        if (key(a) != key(b)) return key(a) < key(b);
        return a < b;
    });
    QtlFamLayout& L = *out;
    L = QtlFamLayout();
    L.cellof.assign(n, -1);
    L.famcell.assign((size_t)F + 1, 0);
    for (size_t j = 0; j < order.size(); j++) {
        const int32_t i = order[j];
        if (j == 0 || grp[i] != grp[order[j - 1]] || key(i) != key(order[j - 1])) {
            while (L.gidx.size() % 4) L.gidx.push_back(-1);
            L.cellslot.push_back((int32_t)L.gidx.size());
            L.famcell[(size_t)grp[i] + 1]++;
        }
        L.cellof[i] = (int32_t)L.cellslot.size() - 1;
        L.gidx.push_back(i);
    }
    while (L.gidx.size() % 4) L.gidx.push_back(-1);
    L.S = (int)L.gidx.size();
    L.Q = (int)L.cellslot.size();
    L.cellslot.push_back(L.S);
    for (int f = 0; f < F; f++) L.famcell[f + 1] += L.famcell[f];
    L.stepend.assign((size_t)L.S / 4, 0);
    for (int f = 0; f < F; f++)
        if (L.famcell[f + 1] > L.famcell[f]) {
            L.stepend[(size_t)L.cellslot[L.famcell[f + 1]] / 4 - 1] = 1;
            L.folds.push_back(f);
        }
    L.folds.push_back(L.folds.empty() ? 0 : L.folds.back());
    return QTLFAM_OK;
}

// every row of perm[P][n] must keep a used individual inside its cell: *bad_row the row, *bad_i the individual
inline int qtlfam_check_permutations(int n, int P, const int32_t* perm, const QtlFamLayout& L, int* bad_row, int* bad_i)
{
    for (int p = 0; p < P; p++)
        for (int i = 0; i < n; i++) {
            const int32_t j = perm[(size_t)p * n + i];
            if (L.cellof[i] >= 0 && (j < 0 || j >= n || L.cellof[j] != L.cellof[i])) return *bad_row = p, *bad_i = i, QTLFAM_PERM_LEAVES_CELL;
        }
    return QTLFAM_OK;
}

// ------------------------------------------------------------------------------------------------ one marker on the CPU
// One marker of the scan, serially, by the steps and in the order of the kernels: origin[n][4] the marker's rows, y[n][T] and
// cov[n][K] as they enter the sums (the scan centres them over the used individuals first; the centring within cells is
// done here), c[n] the chromosome's mask (an individual with grp < 0 is taken out here).  lod[T], *df, slope[T][F] (may be
// null), rss0[T], *n_used, *n_cells.  false: an argument out of range.
inline bool qtlfam_marker_serial(int n, const double* origin, int side, const int32_t* grp, const int32_t* cell, int F, int T,
                                 const double* y, int K, const double* cov, const uint8_t* c, double* lod, int32_t* df,
                                 double* slope, double* rss0, int32_t* n_used, int32_t* n_cells)
{
    if (n < 1 || T < 1 || K < 0 || K > QTL_MAXK || F < 1 || side < 0 || side > 1) return false;
    QtlFamLayout L;
    int          bad = 0;
    if (qtlfam_layout(n, c, grp, cell, F, &L, &bad) != QTLFAM_OK) return false;
    const int S = L.S, n_c = (int)std::count_if(L.gidx.begin(), L.gidx.end(), [](int32_t i) { return i >= 0; });
    // the centred images in gather order
    std::vector<double> Z((size_t)S * QTL_MAXK, 0.0), Y((size_t)S * T, 0.0), x(S, 0.0);
    auto centre = [&](const double* src, int w, int col, double* dst, int dw) {
        for (int q = 0; q < L.Q; q++) {
            auto val = [&](int s, double* v) {
                if (L.gidx[s] < 0) return false;
                *v = src[(size_t)L.gidx[s] * w + col];
                return true;
            };
            const double mean = qtlfam_cell_mean(L.cellslot[q], L.cellslot[q + 1], val);
            double       v;
            for (int s = L.cellslot[q]; s < L.cellslot[q + 1]; s++) dst[(size_t)s * dw + col] = val(s, &v) ? v - mean : 0.0;
        }
    };
    for (int k = 0; k < K; k++) centre(cov, K, k, Z.data(), QTL_MAXK);
    for (int t = 0; t < T; t++) centre(y, T, t, Y.data(), T);
    for (int s = 0; s < S; s++)
        if (L.gidx[s] >= 0) {
            const double* o = origin + (size_t)L.gidx[s] * 4;
            x[s] = qtlfam_x(o[0], o[1], o[2], o[3], side);
        }
    // the null design
    double S11[QTL_NX * QTL_NX] = {0.0}, Lc[QTL_NX * QTL_NX], diag[QTL_MAXK] = {0.0};
    for (int j = 0; j < K; j++)
        for (int k = 0; k <= j; k++) {
            double s = 0.0;
            for (int i = 0; i < S; i++) s += Z[(size_t)i * QTL_MAXK + j] * Z[(size_t)i * QTL_MAXK + k];
            S11[j * QTL_NX + k] = s;
        }
    for (int j = 0; j < K; j++) diag[j] = S11[j * QTL_NX + j];
    std::copy(S11, S11 + QTL_NX * QTL_NX, Lc);
    const bool scanned = qtl_cholesky(Lc, K) && n_c - L.Q - K >= 2;
    *n_used  = n_c;
    *n_cells = L.Q;
    // the design: w_p, u_p, H and its factor
    std::vector<double> w(F, 0.0), u((size_t)F * QTL_MAXK, 0.0);
    double              H[QTLFAM_TRI] = {0.0};
    for (int j = 0; j < K; j++)
        for (int k = 0; k <= j; k++) H[qtlfam_tri(j, k)] = S11[j * QTL_NX + k];
    int fitted = 0;
    for (int f = 0; f < F; f++) {
        double d = 0.0, raw = 0.0;
        for (int q = L.famcell[f]; q < L.famcell[f + 1]; q++) {
            double sx = 0.0, sxx = 0.0;
            int    nq = 0;
            for (int s = L.cellslot[q]; s < L.cellslot[q + 1]; s++) {
                if (L.gidx[s] < 0) continue;
                sx += x[s], sxx += x[s] * x[s], nq++;
                for (int k = 0; k < K; k++) u[(size_t)f * QTL_MAXK + k] += x[s] * Z[(size_t)s * QTL_MAXK + k];
            }
            if (nq > 0) d += sxx - sx * sx / nq, raw += sxx;
        }
        w[f] = qtlfam_weight(raw, d);
        if (w[f] > 0.0) {
            fitted++;
            for (int j = 0; j < K; j++)
                for (int k = 0; k <= j; k++) H[qtlfam_tri(j, k)] -= u[(size_t)f * QTL_MAXK + j] * u[(size_t)f * QTL_MAXK + k] * w[f];
        }
    }
    const bool ok = scanned && qtlfam_factor(H, K, diag) && n_c - L.Q - K - fitted >= 1;
    *df = ok ? fitted : 0;
    for (int t = 0; t < T; t++) {
        double b0[QTL_NX] = {0.0}, z[QTL_NX] = {0.0}, yy = 0.0, e0 = 0.0;
        for (int s = 0; s < S; s++) {
            const double v = Y[(size_t)s * T + t];
            for (int k = 0; k < K; k++) b0[k] += Z[(size_t)s * QTL_MAXK + k] * v;
            yy += v * v;
        }
        if (scanned) {
            for (int k = 0; k < K; k++) z[k] = b0[k];
            qtl_chol_solve(Lc, K, z);
            for (int k = 0; k < K; k++) e0 += b0[k] * z[k];
        }
        rss0[t] = scanned ? yy - e0 : 0.0;
        double              sr2 = 0.0, gs[QTL_MAXK] = {0.0}, g[QTL_MAXK] = {0.0};
        std::vector<double> r(F, 0.0);
        for (int f = 0; f < F; f++) {
            if (L.famcell[f + 1] == L.famcell[f]) continue;
            // (four slots to a step, as the matrix cores add them: the order within a step is the hardware's, and the
            // comparison with the kernels is at the project's bar, not to the bit)
            for (int s = L.cellslot[L.famcell[f]]; s < L.cellslot[L.famcell[f + 1]]; s++) r[f] += x[s] * Y[(size_t)s * T + t];
            qtlfam_fold<QTL_MAXK>(r[f], w[f], &u[(size_t)f * QTL_MAXK], K, sr2, gs);
        }
        for (int k = 0; k < K; k++) g[k] = b0[k] - gs[k];
        double gq = 0.0, gamma[QTL_MAXK];
        for (int k = 0; k < QTL_MAXK; k++) gamma[k] = g[k];
        if (ok) qtlfam_solve(H, 1, K, gamma);
        for (int k = 0; k < K; k++) gq += g[k] * gamma[k];
        lod[t] = qtlfam_cell(sr2, gq, e0, rss0[t], n_c, ok);
        if (slope)
            for (int f = 0; f < F; f++) {
                double ug = 0.0;
                for (int k = 0; k < K; k++) ug += u[(size_t)f * QTL_MAXK + k] * gamma[k];
                slope[(size_t)t * F + f] = (ok && w[f] > 0.0) ? (r[f] - ug) * w[f] : (double)NAN;
            }
    }
    return true;
}

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlfam_kernels.hip read and write (device pointers)
struct QtlFamParams {
    int n, M, C, T, P, K, F, side;
    int S, Q;                      // slots of the gather list (a multiple of 4), cells
    const double*  origin;         // [n][M][4]
    const double*  pheno;          // [n][T]
    const double*  cov;            // [n][K]
    const uint8_t* use;            // [n] use[i] and grp[i] >= 0
    const int32_t* perm;           // [P][n]
    const int32_t* cs;             // [C + 1] chromstarts
    const int32_t* mchrom;         // [M] chromosome of a marker
    const int32_t* tiles;          // [n_tiles][4] chromosome, first marker, markers (<= 16), 0
    const int32_t* tile_start;     // [C + 1]
    int            n_tiles;
    const int32_t* gidx;           // [S]
    const int32_t* cellslot;       // [Q + 1]
    const int32_t* famcell;        // [F + 1]
    const int32_t* stepend;        // [S / 4]
    const int32_t* folds;          // the families with slots, the last once more
    uint8_t*       cmask;          // [C][n] c_i
    int32_t*       nc;             // [C] n_c
    int32_t*       ncells;         // [C] the cells with a used member
    double*        Z;              // [C][S][QTL_MAXK] the centred covariates in gather order
    double*        chrom;          // [C][QTLFAM_CHROM]
    double*        rec;            // [F][1 + K][M] w_p, u_p
    double*        hrec;           // [K (K + 1) / 2 + 1][M] the factor of H, packed; 1.0 = the marker is fitted
    int32_t*       df;             // [M]
    // the column tile: columns [r0, r0 + rn) of the R = T (1 + P)
    int            r0, rn, rstride;
    double*        Y;              // [C][S][rstride] the centred column image in gather order
    double*        nullq;          // [C][K + 2][rstride]: b0, b0' S11^-1 b0, RSS0
    double*        tilemax;        // [n_tiles][rstride]
    double*        gamma;          // [T][M][K] of the observed columns (a call that asks for slopes)
    double *       lod, *slope, *rss0, *pmax;
};
void launch_qtlfam_mask(const QtlFamParams& q, hipStream_t stream);
void launch_qtlfam_image(const QtlFamParams& q, bool covariates, hipStream_t stream);
void launch_qtlfam_chrom(const QtlFamParams& q, hipStream_t stream);
void launch_qtlfam_design(const QtlFamParams& q, hipStream_t stream);
void launch_qtlfam_marker(const QtlFamParams& q, hipStream_t stream);
void launch_qtlfam_null(const QtlFamParams& q, hipStream_t stream);
void launch_qtlfam_scan(const QtlFamParams& q, hipStream_t stream);
void launch_qtlfam_slope(const QtlFamParams& q, hipStream_t stream);
void launch_qtlfam_finish(const QtlFamParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
