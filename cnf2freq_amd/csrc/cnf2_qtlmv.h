// cnf2_qtlmv.h -- the multi-trait QTL scan (cnf2_qtl_scan_mv, include/cnf2hip.h), shared by host and device code: the null fit
// of a group of traits, one (marker, group) cell, one marker computed serially, and what the kernels of
// cnf2_qtlmv_kernels.hip read and write.  The kernels form the sums; every decision (which trait is dropped, what a
// degenerate cell reports) is taken here.
//
// Multivariate Haley-Knott regression (Knott and Haley 2000) of the T traits of a group -- the observed data or one
// permutation of the individuals, which moves all T traits of an individual together -- on the design of cnf2_qtl.h: X0, a, d,
// c, n_c, S11, G, W = (pa, l, pd) are that header's.  Per chromosome and group B0 = X0'Y (nx x T) and
// E0 = Y'CY - B0' S11^-1 B0 (T x T), factored E0 = L L' in trait order.  Trait t is dropped when E0[t][t] <= 0 or its pivot is
// below QTL_PIVOT E0[t][t]: its row of L is absent and it contributes nothing.  Per marker, with V = A'Y - G B0 (2 x T):
//   Vw = V L^-T,  u_t = vwd_t - l vwa_t,  qaa = sum vwa_t^2 / pa,  qdd = sum u_t^2 / pd,  qad^2 = (sum vwa_t u_t)^2 / (pa pd),
//   Lambda = (1 - qaa)(1 - qdd) - qad^2,  lod = -(n_c / 2) log10 Lambda
// over the kept traits; a dropped marker column (pivot 0) gives no terms.  Lambda is Wilks' det(E1) / det(E0), by
// det(I_T - E0^-1 V'W^-1 V) = det(I_2 - W^-1 V E0^-1 V'); it is clamped to [2^-52, 1] and lod is exactly 0 where it is 1.  For
// T = 1 it is 1 - dRSS / RSS0 of cnf2_qtl.h.  A chromosome is not scanned (lod 0, rank 0) when n_c < K + 3 + T, S11 has no
// factor or every trait is dropped.
#ifndef CNF2_QTLMV_H
#define CNF2_QTLMV_H

#include "cnf2_qtl.h"

namespace cnf2 {

constexpr int QTLMV_MAXT = 16;                                   // traits at most
constexpr int QTLMV_WORK = QTL_NX * QTLMV_MAXT;                  // doubles of workspace qtlmv_factor needs

// The traits of a group padded to the width the hot kernel is compiled for: 4, 8 or 16
CNF2_HD int qtlmv_width(int T) { return T <= 4 ? 4 : (T <= 8 ? 8 : 16); }

// The record per (chromosome, group), in doubles:
//   [0, TP)             L, lower, packed by rows (row t at t (t + 1) / 2), TP = T (T + 1) / 2; the diagonal holds 1 / L[t][t],
//                       and 0 for a dropped trait, whose row and column are 0
//   [TP, TP + T)        1.0 for a kept trait, 0.0 for a dropped one
//   [TP + T]            1.0 = the group is scanned on this chromosome
//   [TP + T + 1, ..)    B0, [nx][T]
CNF2_HD int    qtlmv_tp(int T) { return T * (T + 1) / 2; }
CNF2_HD int    qtlmv_o_keep(int T) { return qtlmv_tp(T); }
CNF2_HD int    qtlmv_o_usable(int T) { return qtlmv_tp(T) + T; }
CNF2_HD int    qtlmv_o_b0(int T) { return qtlmv_tp(T) + T + 1; }
CNF2_HD size_t qtlmv_rec_doubles(int T) { return (size_t)qtlmv_o_b0(T) + (size_t)QTL_NX * T; }

// E0 -> L with the drop rule, and the whole record.  yy[TP]: the lower triangle of Y'CY, packed as L; b0[nx][T] = X0'Y;
// chol: the chromosome's QTL_CHOL doubles of qtl_chrom_kernel; work[QTLMV_WORK].  Returns the number of traits kept (0: the
// group is not scanned).
CNF2_HD int qtlmv_factor(const double* yy, const double* b0, const double* chol, int nx, int K, int n_c, int T, double* work,
                         double* rec)
{
    const bool fit = chol[QTL_NX * QTL_NX] != 0.0 && n_c >= K + 3 + T;
    double*    L = rec;
    double*    keep = rec + qtlmv_o_keep(T);
    // work[k][t] = (S11^-1 B0)[k][t]
    for (int t = 0; t < T; t++) {
        double z[QTL_NX];
CNF2_QTL_UNROLL
        for (int k = 0; k < QTL_NX; k++) z[k] = (fit && k < nx) ? b0[k * T + t] : 0.0;
        if (fit) qtl_chol_solve(chol, nx, z);
CNF2_QTL_UNROLL
        for (int k = 0; k < QTL_NX; k++)
            if (k < nx) work[k * T + t] = z[k];
    }
    int kept = 0;
    for (int t = 0; t < T; t++) {
        const int row = t * (t + 1) / 2;
        // row t of E0, then of L: columns s < t against the rows before
        for (int s = 0; s <= t; s++) {
            double e = yy[row + s];
            for (int k = 0; k < nx; k++) e -= b0[k * T + s] * work[k * T + t];
            L[row + s] = e;
        }
        const double ett = L[row + t];
        double       d = ett;
        for (int s = 0; s < t; s++) {
            double    x = L[row + s];
            const int rs = s * (s + 1) / 2;
            for (int k = 0; k < s; k++) x -= L[row + k] * L[rs + k];
            x *= L[rs + s];                       // (0 for a dropped trait s)
            L[row + s] = x;
            d -= x * x;
        }
        const bool on = fit && ett > 0.0 && d >= QTL_PIVOT * ett && d > 0.0;
        if (!on)
            for (int s = 0; s < t; s++) L[row + s] = 0.0;
        L[row + t] = on ? 1.0 / sqrt(d) : 0.0;
        keep[t]    = on ? 1.0 : 0.0;
        kept += on ? 1 : 0;
    }
    rec[qtlmv_o_usable(T)] = kept > 0 ? 1.0 : 0.0;
    double* b = rec + qtlmv_o_b0(T);
    for (int e = 0; e < nx * T; e++) b[e] = b0[e];
    return kept;
}

// One (marker, group) cell from V = A'Y - G B0 (va[t], vd[t], t < T; whitened in place by forward substitution), the group's
// record and the marker's pivots.  TW >= T is a constant, so that the device code keeps va and vd in registers.
template <int TW>
CNF2_HD double qtlmv_cell(double* va, double* vd, const double* rec, int T, double pa, double l, double pd, int n_c)
{
    double qaa = 0.0, qdd = 0.0, qad = 0.0;
CNF2_QTL_UNROLL
    for (int t = 0; t < TW; t++)
        if (t < T) {
            const double* row = rec + t * (t + 1) / 2;
            double        sa = va[t], sd = vd[t];
CNF2_QTL_UNROLL
            for (int s = 0; s < TW; s++)
                if (s < t) {
                    const double x = row[s];
                    sa -= x * va[s];
                    sd -= x * vd[s];
                }
            const double r = row[t];
            sa *= r;
            sd *= r;
            va[t] = sa;
            vd[t] = sd;
            const double u = sd - l * sa;
            qaa += sa * sa;
            qdd += u * u;
            qad += sa * u;
        }
    if (rec[qtlmv_o_usable(T)] == 0.0) return 0.0;
    const bool ka = pa > 0.0, kd = pd > 0.0;
    qaa = ka ? qaa / pa : 0.0;
    qdd = kd ? qdd / pd : 0.0;
    qad = (ka && kd) ? qad * qad / (pa * pd) : 0.0;
    double lam = (1.0 - qaa) * (1.0 - qdd) - qad;
    lam        = lam >= 2.220446049250313e-16 ? lam : 2.220446049250313e-16;        // (a NaN takes the floor as well)
    return lam < 1.0 ? -0.5 * (double)n_c * log10(lam) : 0.0;
}

// the marker's rank as the scan reports it: the columns qtl_marker_record kept, 0 where the observed group is not scanned
CNF2_HD int qtlmv_rank(const double* rec0, int T, double pa, double pd)
{
    return rec0[qtlmv_o_usable(T)] != 0.0 ? (pa > 0.0 ? 1 : 0) + (pd > 0.0 ? 1 : 0) : 0;
}

// One marker and group on the CPU, the individuals in ascending order: origin[n][4] the marker's rows, y[n][T] and cov[n][K]
// as they enter the sums (the scan centres them first), c[n] the chromosome's mask.  false: an argument out of range.
inline bool qtlmv_marker_serial(int n, const double* origin, int T, const double* y, int K, const double* cov, const uint8_t* c,
                                bool additive, double* lod, int32_t* rank, int32_t* trait_rank, int32_t* n_c_out)
{
    if (n < 1 || T < 1 || T > QTLMV_MAXT || K < 0 || K > QTL_MAXK) return false;
    const int nx = K + 1;
    auto      x  = [&](int i, int k) { return k == 0 ? 1.0 : cov[(size_t)i * K + (k - 1)]; };
    double    chol[QTL_CHOL] = {0.0};
    int       n_c = 0;
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        n_c++;
        for (int j = 0; j < nx; j++)
            for (int k = 0; k <= j; k++) chol[j * QTL_NX + k] += x(i, j) * x(i, k);
    }
    const bool ok = qtl_cholesky(chol, nx);
    chol[QTL_NX * QTL_NX] = (ok && n_c >= K + 4) ? 1.0 : 0.0;
    double sa[QTL_NX] = {0.0}, sd[QTL_NX] = {0.0}, saa = 0.0, sad = 0.0, sdd = 0.0;
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        const double* o = origin + (size_t)i * 4;
        const double  a = o[3] - o[0], d = o[1] + o[2];
        for (int k = 0; k < nx; k++) {
            sa[k] += a * x(i, k);
            sd[k] += d * x(i, k);
        }
        saa += a * a, sad += a * d, sdd += d * d;
    }
    double mk[QTL_MK];
    qtl_marker_record(chol, nx, chol[QTL_NX * QTL_NX] != 0.0, sa, sd, saa, sad, sdd, additive, mk);
    double yy[QTLMV_MAXT * (QTLMV_MAXT + 1) / 2] = {0.0}, b0[QTL_NX * QTLMV_MAXT] = {0.0}, work[QTLMV_WORK];
    double va[QTLMV_MAXT] = {0.0}, vd[QTLMV_MAXT] = {0.0};
    double rec[QTLMV_MAXT * (QTLMV_MAXT + 1) / 2 + QTLMV_MAXT + 1 + QTL_NX * QTLMV_MAXT];
    for (int i = 0; i < n; i++) {
        if (!c[i]) continue;
        const double* o = origin + (size_t)i * 4;
        const double  a = o[3] - o[0], d = o[1] + o[2];
        for (int t = 0; t < T; t++) {
            const double v = y[(size_t)i * T + t];
            for (int s = 0; s <= t; s++) yy[t * (t + 1) / 2 + s] += v * y[(size_t)i * T + s];
            for (int k = 0; k < nx; k++) b0[k * T + t] += x(i, k) * v;
            va[t] += a * v;
            vd[t] += d * v;
        }
    }
    *trait_rank = qtlmv_factor(yy, b0, chol, nx, K, n_c, T, work, rec);
    for (int t = 0; t < T; t++)
        for (int k = 0; k < nx; k++) {
            va[t] -= mk[k] * b0[k * T + t];
            vd[t] -= mk[QTL_NX + k] * b0[k * T + t];
        }
    *lod     = qtlmv_cell<QTLMV_MAXT>(va, vd, rec, T, mk[QTL_PA], mk[QTL_L], mk[QTL_PD], n_c);
    *rank    = qtlmv_rank(rec, T, mk[QTL_PA], mk[QTL_PD]);
    *n_c_out = n_c;
    return true;
}

#if defined(__HIPCC__)
// What the kernels of cnf2_qtlmv_kernels.hip read and write (device pointers).  The chromosome masks, n_c, the factors of S11
// and the marker records are qtl_chrom_kernel's and qtl_design_kernel's (cnf2_qtl_kernels.hip).
struct QtlMvParams {
    int n, M, C, T, T4, P, K, nx;
    int g0, gn;                  // the group tile [g0, g0 + gn) of the 1 + P; group 0 is the observed data
    int ystride;                 // doubles per row of the image: 64 per wave of 64 / T4 groups
    int gstride;                 // groups the tile has room for: ystride / T4
    const double*  origin;       // [n][M][4]
    const double*  pheno;        // [n][T]
    const double*  cov;          // [n][K]
    const uint8_t* use;          // [n]
    const int32_t* perm;         // [P][n]
    const uint8_t* cmask;        // [C][n]
    int32_t*       nc;           // [C] (an output too: n_used)
    const double*  chol;         // [C][QTL_CHOL]
    const double*  mk;           // [M][QTL_MK]
    const int32_t* tiles;        // [n_tiles][4] chromosome, first marker, markers (<= 16), 0
    const int32_t* tile_start;   // [C + 1]
    int            n_tiles;
    double*        Y;            // [n][ystride] the image in operand order (qtlmv_image_column)
    double*        rec;          // [C][gstride][qtlmv_rec_doubles(T)]
    double*        tilemax;      // [n_tiles][gstride]
    double*        lod;          // [M]
    int32_t*       rank;         // [M]
    int32_t*       trait_rank;   // [C]
    double*        pmax;         // [P][C]
};
void launch_qtlmv_gather(const QtlMvParams& q, hipStream_t stream);
void launch_qtlmv_null(const QtlMvParams& q, hipStream_t stream);
void launch_qtlmv_scan(const QtlMvParams& q, hipStream_t stream);
void launch_qtlmv_finish(const QtlMvParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
