// cnf2_qtlhap.h -- the founder-haplotype QTL scan (cnf2_qtl_scan_hap, include/cnf2hip.h), shared by host and device code: the
// design row of an individual, the packed factor of a marker's Schur complement with its drop rule, the substitutions, the
// clamps and logarithm of one (marker, column) cell, the gather list the product walks, one marker fitted serially on the
// CPU, and what the kernels of cnf2_qtlhap_kernels.hip read and write.  The Cholesky factor of the null design is cnf2_qtl.h's.
//
// The trait is regressed on the expected dosage of every founder haplotype.  col[i][0..7] assigns the eight cells of an
// individual's descent row (cnf2_sweep_descent) to model columns 0 .. H-1, H <= 32.  pheno, use, cov (K <= 8), perm, the columns
// R = T (1 + P), X0 = [c, c z_1 .. c z_K], its centring, S11 = X0'X0, b0 = X0'y and RSS0 per chromosome and column, the clamp of
// dRSS and the LOD formula are cnf2_qtl_scan's (cnf2_qtl.h).  Per chromosome c_i = use[i] and every col[i][k] in [0, H) and the
// descent row at the chromosome's first marker is not all zero; n_c = sum c_i.  Per marker
//   Z[i][h] = c_i sum_k [col[i][k] == h] descent[i][m][k]                        (the expected dosage of column h, 0 .. 2)
//   S22 = Z'Z,  S21 = Z'X0,  G = S21 S11^-1,  W = S22 - G S21',  v = Z'y - G b0.
// W is factored in ascending column order, W_kept = L L'.  Column h is dropped when S22[h][h] == 0 or its pivot is below
// QTL_PIVOT times S22[h][h]; df = the columns kept.  The rows of Z add up to 2 c_i (and with one column per strand each side
// adds up to c_i), so the columns and the intercept are dependent at every marker: the rule is the normal path.
//   dRSS = |L^-1 v_kept|^2,  lod = (n_c / 2) log10(RSS0 / (RSS0 - dRSS)),  coef = W_kept^-1 v_kept, NaN where dropped.
// A chromosome is not scanned when S11 has no Cholesky factor or n_c < K + 4; a marker with n_c - 1 - K - df < 1 reports df 0,
// lod 0 and coef NaN.
#ifndef CNF2_QTLHAP_H
#define CNF2_QTLHAP_H

#include "cnf2_qtl.h"

#include <algorithm>
#include <vector>

namespace cnf2 {

constexpr int QTLHAP_MAXH = 32;                                   // model columns at most: 16 phased grandparents
constexpr int QTLHAP_TRI  = QTLHAP_MAXH * (QTLHAP_MAXH + 1) / 2;  // the packed lower triangle at H = 32: 528 doubles

CNF2_HD constexpr int qtlhap_tri(int j, int k) { return j * (j + 1) / 2 + k; }      // (j, k), k <= j
// doubles of a marker's record: the packed factor, then G[H][nx]
CNF2_HD constexpr int qtlhap_rec_size(int H, int nx) { return H * (H + 1) / 2 + H * nx; }

// Z[i][h] of one individual from its descent row d[8] and its columns col[8]
CNF2_HD double qtlhap_z(const double* d, const int32_t* col, int h)
{
    double z = 0.0;
CNF2_QTL_UNROLL
    for (int k = 0; k < 8; k++) z += col[k] == h ? d[k] : 0.0;
    return z;
}

// W = L L' over the kept columns, in place on the packed lower triangle; diag[h] = S22[h][h].  Returns the mask of the kept
// columns.  A dropped column's entries are left as they are and never read.
CNF2_HD uint32_t qtlhap_factor(double* W, int H, const double* diag)
{
    uint32_t kept = 0;
    for (int h = 0; h < H; h++) {
        double d = W[qtlhap_tri(h, h)];
        for (int k = 0; k < h; k++)
            if ((kept >> k) & 1) d -= W[qtlhap_tri(h, k)] * W[qtlhap_tri(h, k)];
        if (!(diag[h] > 0.0 && d >= QTL_PIVOT * diag[h])) continue;
        kept |= 1u << h;
        d = sqrt(d);
        W[qtlhap_tri(h, h)] = d;
        for (int i = h + 1; i < H; i++) {
            double s = W[qtlhap_tri(i, h)];
            for (int k = 0; k < h; k++)
                if ((kept >> k) & 1) s -= W[qtlhap_tri(i, k)] * W[qtlhap_tri(h, k)];
            W[qtlhap_tri(i, h)] = s / d;
        }
    }
    return kept;
}

CNF2_HD int qtlhap_count(uint32_t kept)
{
    int n = 0;
    for (int h = 0; h < QTLHAP_MAXH; h++) n += (kept >> h) & 1;
    return n;
}

// x <- L^-1 v over the kept columns (0 at a dropped one), entry h of the vector at x[h * stride]; returns |x|^2
CNF2_HD double qtlhap_forward(const double* L, int H, uint32_t kept, double* x, size_t stride)
{
    double d = 0.0;
    for (int h = 0; h < H; h++) {
        double s = 0.0;
        if ((kept >> h) & 1) {
            s = x[h * stride];
            for (int k = 0; k < h; k++)
                if ((kept >> k) & 1) s -= L[qtlhap_tri(h, k)] * x[k * stride];
            s /= L[qtlhap_tri(h, h)];
            d += s * s;
        }
        x[h * stride] = s;
    }
    return d;
}

// x <- L'^-1 x over the kept columns: after qtlhap_forward the coefficients W_kept^-1 v
CNF2_HD void qtlhap_backward(const double* L, int H, uint32_t kept, double* x, size_t stride)
{
    for (int h = H - 1; h >= 0; h--) {
        if (!((kept >> h) & 1)) continue;
        double s = x[h * stride];
        for (int i = h + 1; i < H; i++)
            if ((kept >> i) & 1) s -= L[qtlhap_tri(i, h)] * x[i * stride];
        x[h * stride] = s / L[qtlhap_tri(h, h)];
    }
}

// One (marker, column) cell from dRSS.  ok: the chromosome is scanned and the marker has residual degrees of freedom.  dRSS
// is clamped to [0, RSS0 (1 - 2^-52)]: the LOD is finite and not negative.
CNF2_HD double qtlhap_cell(double d, double rss0, int n_c, bool ok)
{
    if (!ok || !(rss0 > 0.0)) return 0.0;
    const double hi = rss0 * (1.0 - 2.220446049250313e-16);
    d               = d < 0.0 ? 0.0 : (d > hi ? hi : d);
    return d > 0.0 ? 0.5 * (double)n_c * log10(rss0 / (rss0 - d)) : 0.0;
}

// ------------------------------------------------------------------------------------------------ the gather list
// The used individuals ordered by their col row (lexicographically), then by index: a pattern is a run of equal rows -- in a
// cross from few founders one per pair of F1 parents.  Every pattern is padded with empty slots (-1) to a multiple of 4: a
// k-step of four slots never straddles two patterns, and inside a pattern the eight doubles of a descent row are the matrix
// cores' operand as they lie in memory.
struct QtlHapLayout {
    std::vector<int32_t> gidx;       // [S] the individual of a slot, -1 for an empty one
    std::vector<int32_t> steppat;    // [S / 4] the pattern of a step of four slots
    std::vector<int32_t> stepend;    // [S / 4] 1 where a step is the last of its pattern
    std::vector<int32_t> patcol;     // [patterns][8] the pattern's columns
    int                  S = 0, n_pat = 0;
};

// use[n]: the individuals with use != 0 and all eight columns in range
inline void qtlhap_layout(int n, const uint8_t* use, const int32_t* col, QtlHapLayout* out)
{
    std::vector<int32_t> order;
    for (int i = 0; i < n; i++)
        if (use[i]) order.push_back(i);
    auto row = [&](int32_t i) { return col + (size_t)i * 8; };
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        if (!std::equal(row(a), row(a) + 8, row(b))) return std::lexicographical_compare(row(a), row(a) + 8, row(b), row(b) + 8);
        return a < b;
    });
    QtlHapLayout& L = *out;
    L = QtlHapLayout();
    for (size_t j = 0; j < order.size(); j++) {
        const int32_t i = order[j];
        if (j == 0 || !std::equal(row(i), row(i) + 8, row(order[j - 1]))) {
            while (L.gidx.size() % 4) L.gidx.push_back(-1);
            L.patcol.insert(L.patcol.end(), row(i), row(i) + 8);
            L.n_pat++;
        }
        L.gidx.push_back(i);
        if (L.gidx.size() % 4 == 1) L.steppat.push_back(L.n_pat - 1);
    }
    while (L.gidx.size() % 4) L.gidx.push_back(-1);
    L.S = (int)L.gidx.size();
    L.stepend.assign(L.steppat.size(), 0);
    for (size_t s = 0; s < L.steppat.size(); s++)
        if (s + 1 == L.steppat.size() || L.steppat[s + 1] != L.steppat[s]) L.stepend[s] = 1;
}

// the mask the scan works with: use[i] (NULL: all) and every column of the individual in [0, H).  Returns the individual
// with a column >= H or < -1, or -1 when there is none
inline int qtlhap_mask(int n, const uint8_t* use, const int32_t* col, int H, uint8_t* mask)
{
    for (int i = 0; i < n; i++) {
        bool all = true;
        for (int k = 0; k < 8; k++) {
            const int32_t c = col[(size_t)i * 8 + k];
            if (c >= H || c < -1) return i;
            all = all && c >= 0;
        }
        mask[i] = ((!use || use[i]) && all) ? 1 : 0;
    }
    return -1;
}

// ------------------------------------------------------------------------------------------------ one marker on the CPU
// One marker of the scan, serially, by the steps and in the order of the kernels: descent[n][8] the marker's rows, col[n][8],
// y[n][T] and cov[n][K] as they enter the sums (the scan centres them over the used individuals first), c[n] the chromosome's
// mask (an individual with a column out of [0, H) is taken out here).  lod[T], *df, coef[T][H] (may be null), rss0[T],
// *n_used.  false: an argument out of range.
inline bool qtlhap_marker_serial(int n, const double* descent, const int32_t* col, int H, int T, const double* y, int K,
                                 const double* cov, const uint8_t* c, double* lod, int32_t* df, double* coef, double* rss0,
                                 int32_t* n_used)
{
    if (n < 1 || T < 1 || K < 0 || K > QTL_MAXK || H < 1 || H > QTLHAP_MAXH) return false;
    std::vector<uint8_t> mask(n);
    if (qtlhap_mask(n, c, col, H, mask.data()) >= 0) return false;
    const int nx = K + 1;
    int       n_c = 0;
    for (int i = 0; i < n; i++) n_c += mask[i];
    *n_used = n_c;
    auto x0 = [&](int i, int k) { return k == 0 ? 1.0 : cov[(size_t)i * K + (k - 1)]; };
    // the null design
    double S11[QTL_NX * QTL_NX] = {0.0};
    for (int j = 0; j < nx; j++)
        for (int k = 0; k <= j; k++) {
            double s = 0.0;
            for (int i = 0; i < n; i++)
                if (mask[i]) s += x0(i, j) * x0(i, k);
            S11[j * QTL_NX + k] = s;
        }
    const bool usable = qtl_cholesky(S11, nx) && n_c >= K + 4;
    // the design: S22, S21 over the individuals in ascending order, G, W and its factor
    std::vector<double> W((size_t)H * (H + 1) / 2, 0.0), S21((size_t)H * QTL_NX, 0.0), G((size_t)H * QTL_NX, 0.0), diag(H), z(H);
    for (int i = 0; i < n; i++) {
        if (!mask[i]) continue;
        for (int h = 0; h < H; h++) z[h] = qtlhap_z(descent + (size_t)i * 8, col + (size_t)i * 8, h);
        for (int j = 0; j < H; j++) {
            for (int k = 0; k <= j; k++) W[qtlhap_tri(j, k)] += z[j] * z[k];
            for (int k = 0; k < nx; k++) S21[(size_t)j * QTL_NX + k] += z[j] * x0(i, k);
        }
    }
    for (int h = 0; h < H; h++) diag[h] = W[qtlhap_tri(h, h)];
    uint32_t kept = 0;
    if (usable) {
        for (int h = 0; h < H; h++) {
            double g[QTL_NX] = {0.0};
            for (int k = 0; k < nx; k++) g[k] = S21[(size_t)h * QTL_NX + k];
            qtl_chol_solve(S11, nx, g);
            for (int k = 0; k < nx; k++) G[(size_t)h * QTL_NX + k] = g[k];
        }
        for (int j = 0; j < H; j++)
            for (int k = 0; k <= j; k++) {
                double s = 0.0;
                for (int kk = 0; kk < nx; kk++) s += G[(size_t)j * QTL_NX + kk] * S21[(size_t)k * QTL_NX + kk];
                W[qtlhap_tri(j, k)] -= s;
            }
        kept = qtlhap_factor(W.data(), H, diag.data());
    }
    const bool ok = usable && n_c - 1 - K - qtlhap_count(kept) >= 1;
    if (!ok) kept = 0;
    *df = qtlhap_count(kept);
    // the columns: b0, RSS0, then Z'y pattern by pattern as the product adds it
    QtlHapLayout lay;
    qtlhap_layout(n, mask.data(), col, &lay);
    for (int t = 0; t < T; t++) {
        double b0[QTL_NX] = {0.0}, s0[QTL_NX] = {0.0}, yy = 0.0, e0 = 0.0;
        for (int i = 0; i < n; i++) {
            if (!mask[i]) continue;
            const double v = y[(size_t)i * T + t];
            for (int k = 0; k < nx; k++) b0[k] += x0(i, k) * v;
            yy += v * v;
        }
        if (usable) {
            for (int k = 0; k < nx; k++) s0[k] = b0[k];
            qtl_chol_solve(S11, nx, s0);
            for (int k = 0; k < nx; k++) e0 += b0[k] * s0[k];
        }
        rss0[t] = usable ? yy - e0 : 0.0;
        std::vector<double> v(H, 0.0);
        double              part[8] = {0.0};
        for (size_t s = 0; s < lay.steppat.size(); s++) {
            for (int j = 0; j < 4; j++) {
                const int32_t i = lay.gidx[4 * s + j];
                if (i < 0) continue;
                for (int k = 0; k < 8; k++) part[k] += descent[(size_t)i * 8 + k] * y[(size_t)i * T + t];
            }
            if (lay.stepend[s])
                for (int k = 0; k < 8; k++) {
                    v[lay.patcol[(size_t)lay.steppat[s] * 8 + k]] += part[k];
                    part[k] = 0.0;
                }
        }
        for (int h = 0; h < H; h++)
            for (int k = 0; k < nx; k++) v[h] -= G[(size_t)h * QTL_NX + k] * b0[k];
        const double d = qtlhap_forward(W.data(), H, kept, v.data(), 1);
        lod[t] = qtlhap_cell(d, rss0[t], n_c, ok);
        if (coef) {
            qtlhap_backward(W.data(), H, kept, v.data(), 1);
            for (int h = 0; h < H; h++) coef[(size_t)t * H + h] = ((kept >> h) & 1) ? v[h] : (double)NAN;
        }
    }
    return true;
}

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlhap_kernels.hip read and write (device pointers).  The column image, the null quantities and
// the maxima of the permuted columns are cnf2_qtl_kernels.hip's (QtlParams: qtl_gather_kernel, qtl_null_kernel,
// qtl_finish_kernel), on tiles of two markers.
struct QtlHapParams {
    QtlParams      q;              // n, M, C, T, P, K, nx, pheno, cov, use (the scan's mask), perm, cs, mchrom, cmask, nc, chol,
                                   // r0, rn, rstride, Y, nullq, tiles (two markers each), tile_start, n_tiles, tilemax, lod, rss0, pmax
    int            H, S;           // model columns; slots of the gather list (a multiple of 4)
    const double*  descent;        // [n][M][8]
    const int32_t* col;            // [n][8]
    const int32_t* gidx;           // [S]
    const int32_t* steppat;        // [S / 4]
    const int32_t* stepend;        // [S / 4]
    const int32_t* patcol;         // [patterns][8]
    double*        rec;            // [M][qtlhap_rec_size(H, nx)] the packed factor, then G
    uint32_t*      kept;           // [M] the columns kept
    int32_t*       df;             // [M]
    double*        coef;           // [T][M][H] or null
};
void launch_qtlhap_chrom(const QtlHapParams& p, hipStream_t stream);
void launch_qtlhap_design(const QtlHapParams& p, hipStream_t stream);
void launch_qtlhap_scan(const QtlHapParams& p, hipStream_t stream);
#endif

} // namespace cnf2
#endif
