// cnf2_qtlboot.h -- the bootstrap QTL scan (cnf2_qtl_scan_boot, include/cnf2hip.h), shared by host and device code: what a
// replicate's weights change in the model of cnf2_qtl.h, one (replicate, marker) cell computed serially, and what the kernels
// of cnf2_qtlboot_kernels.hip read and write.
//
// Replicate b draws the individuals with replacement: count[b][i] times individual i.  Ordinary least squares on the
// resampled data set is weighted least squares on the original one with the integer weights w_i = count[b][i] c_i (c the 0/1
// mask of the chromosome): n_bc = sum w_i, S11 = X0'WX0, b0 = X0'Wy, RSS0 = y'Wy - b0' S11^-1 b0, S21 = A'WX0, S22 = A'WA,
// v = A'Wy - G b0.  Everything after the sums -- the factor, the rank rule with QTL_PIVOT, the clamps, the logarithm -- is
// cnf2_qtl.h's, called as it is with n_bc for n_c.
//
// One rule is the replicate's own.  The scans centre every covariate by its mean over the used individuals, so that a
// constant covariate is exactly 0 and X0 has no factor.  A replicate can make a covariate constant that is not constant in
// the data (a binary covariate whose one class was not drawn); centred by the unweighted mean it is a non-zero multiple of
// the intercept, and whether the factor's pivot is positive is a matter of rounding.  So a covariate that takes one value on
// all the individuals with w_i > 0 makes the replicate unusable on that chromosome, decided by comparing the values.
#ifndef CNF2_QTLBOOT_H
#define CNF2_QTLBOOT_H

#include "cnf2_qtl.h"

namespace cnf2 {

// doubles per (replicate, chromosome) record: QTL_CHOL (the factor of S11, then 1.0 = usable), then per trait b0[QTL_NX], RSS0
constexpr int QTLBOOT_TRAIT = QTL_NX + 1;
CNF2_HD size_t qtlboot_rec_doubles(int T) { return (size_t)QTL_CHOL + (size_t)T * QTLBOOT_TRAIT; }

// One (replicate, marker) cell on the CPU, the individuals in ascending order: origin[n][4] the marker's rows, y[n][T] and
// cov[n][K] as they enter the sums (the callers centre them), c[n] the chromosome's mask, count[n] the replicate.  lod[T],
// coef[T][2], rss0[T].  false: an argument out of range.
inline bool qtlboot_marker_serial(int n, const double* origin, int T, const double* y, int K, const double* cov, const uint8_t* c,
                                  const int32_t* count, bool additive, double* lod, double* coef, int32_t* rank, double* rss0,
                                  int32_t* n_bc_out)
{
    if (n < 1 || T < 1 || K < 0 || K > QTL_MAXK) return false;
    const int nx = K + 1;
    auto      x  = [&](int i, int k) { return k == 0 ? 1.0 : cov[(size_t)i * K + (k - 1)]; };
    double    S[QTL_NX * QTL_NX] = {0.0};
    double    first[QTL_NX] = {0.0};
    bool      varies[QTL_NX] = {false};
    long long n_bc = 0;
    bool      any = false;
    for (int i = 0; i < n; i++)
        if (count[i] < 0) return false;
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        const double w = (double)count[i];
        n_bc += count[i];
        for (int j = 0; j < nx; j++)
            for (int k = 0; k <= j; k++) S[j * QTL_NX + k] += w * x(i, j) * x(i, k);
        if (count[i] > 0) {
            for (int k = 1; k < nx; k++) {
                if (!any) first[k] = x(i, k);
                varies[k] = varies[k] || x(i, k) != first[k];
            }
            any = true;
        }
    }
    bool usable = n_bc >= K + 4 && n_bc <= 0x7fffffff;
    for (int k = 1; k < nx; k++) usable = usable && varies[k];
    usable = usable && qtl_cholesky(S, nx);
    double sa[QTL_NX] = {0.0}, sd[QTL_NX] = {0.0}, saa = 0.0, sad = 0.0, sdd = 0.0;
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        const double* o = origin + (size_t)i * 4;
        const double  w = (double)count[i], a = o[3] - o[0], d = additive ? 0.0 : o[1] + o[2];
        for (int k = 0; k < nx; k++) {
            sa[k] += w * (a * x(i, k));
            sd[k] += w * (d * x(i, k));
        }
        saa += w * (a * a), sad += w * (a * d), sdd += w * (d * d);
    }
    double rec[QTL_MK];
    *rank     = qtl_marker_record(S, nx, usable, sa, sd, saa, sad, sdd, additive, rec);
    *n_bc_out = (int32_t)n_bc;
    for (int t = 0; t < T; t++) {
        double b[QTL_NX] = {0.0}, z[QTL_NX], yy = 0.0, va = 0.0, vd = 0.0;
        for (int i = 0; i < n; i++) {
            if (!c[i]) continue;
            const double* o = origin + (size_t)i * 4;
            const double  w = (double)count[i], v = y[(size_t)i * T + t], a = o[3] - o[0], d = additive ? 0.0 : o[1] + o[2];
            for (int k = 0; k < nx; k++) b[k] += w * (x(i, k) * v);
            yy += w * (v * v);
            va += w * (a * v);
            vd += w * (d * v);
        }
        double r0 = 0.0;
        if (usable) {
            for (int k = 0; k < QTL_NX; k++) z[k] = b[k];
            qtl_chol_solve(S, nx, z);
            double e = 0.0;
            for (int k = 0; k < nx; k++) e += b[k] * z[k];
            r0 = yy - e;
        }
        for (int k = 0; k < nx; k++) {
            va -= rec[k] * b[k];
            vd -= rec[QTL_NX + k] * b[k];
        }
        const QtlCell cell = qtl_cell(va, vd, rec[QTL_PA], rec[QTL_L], rec[QTL_PD], r0, (int)n_bc, usable);
        rss0[t] = r0, lod[t] = cell.lod, coef[2 * t] = cell.ca, coef[2 * t + 1] = cell.cd;
    }
    return true;
}

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlboot_kernels.hip read and write (device pointers)
struct QtlBootParams {
    int n, M, T, K, nx, additive;
    int nc;                      // chromosomes scanned
    int m_lo, n_mark;            // the first scanned marker, the markers scanned
    int b0, bn, bstride;         // the replicate tile [b0, b0 + bn) of the B; the weight image's stride, a multiple of 16
    int t0, tn;                  // the trait chunk [t0, t0 + tn) of the hot kernel
    const double*  origin;       // [n][M][4]
    const double*  pheno;        // [n][T]
    const double*  cov;          // [n][K]
    const uint8_t* use;          // [n]
    const int32_t* count;        // [B][n]
    const int32_t* first;        // [nc] first marker of a scanned chromosome
    const int32_t* tiles;        // [n_tiles][4] scanned chromosome (0 .. nc-1), first marker, markers (<= 16), 0
    const int32_t* tile_start;   // [nc + 1]
    int            n_tiles;
    uint8_t*       cmask;        // [nc][n] c_i
    double*        W;            // [n][bstride] the weight image: count as doubles, 0 past the tile
    double*        rec;          // [bn][nc][qtlboot_rec_doubles(T)]
    double*        tilemax;      // [n_tiles][bn][T]
    int32_t*       tilearg;      // [n_tiles][bn][T]
    double*        boot_max;     // [B][T][nc]
    int32_t*       boot_arg;     // [B][T][nc]
    int32_t*       n_boot;       // [B][nc]
    double*        boot_lod;     // [B][T][n_mark] or null
};
void launch_qtlboot_mask(const QtlBootParams& q, hipStream_t stream);
void launch_qtlboot_gather(const QtlBootParams& q, hipStream_t stream);
void launch_qtlboot_design(const QtlBootParams& q, hipStream_t stream);
void launch_qtlboot_null(const QtlBootParams& q, hipStream_t stream);
int  qtlboot_trait_chunk(int T);
void launch_qtlboot_scan(const QtlBootParams& q, hipStream_t stream);
void launch_qtlboot_finish(const QtlBootParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
