// cnf2_qtlfam_kernels.hip -- the kernels of the within-family QTL scan (cnf2_qtl_scan_fam, include/cnf2hip.h): the nested
// half-sib model on the origin rows, a mean per cell and a slope per family.  The model and every decision about degenerate
// families, markers and chromosomes live in cnf2_qtlfam.h; this file forms the sums.  All kernels walk the gather list of
// that header: the used individuals ordered by (family, cell, index), every cell padded to a multiple of four slots.
//
//   qtlfam_mask_kernel    per chromosome: c_i, n_c, the cells with a used member
//   qtlfam_image_kernel   per (chromosome, cell, column): the column centred within the cell, in gather order -- the
//                         covariates once per call, the observed and permuted phenotypes per column tile
//   qtlfam_chrom_kernel   per chromosome: S11 = Z~'Z~, its Cholesky factor, whether the chromosome is scanned
//   qtlfam_design_kernel  per (marker, family): d_p, raw_p, u_p; the record w_p = 1 / d_p (0: not fitted), u_p
//   qtlfam_marker_kernel  per marker: H = S11 - sum u_p u_p' w_p and its factor, df
//   qtlfam_null_kernel    per chromosome and column: b0 = Z~'y~, b0' S11^-1 b0, RSS0
//   qtlfam_scan_kernel    the hot path: r_p[m][col] = sum over the family's slots x(m, i) y~(i, col) on the f64 matrix cores,
//                         folded into sum r_p^2 w_p and sum u_p r_p w_p at every family end, the cell in registers
//   qtlfam_slope_kernel   per (observed column, marker, family): slope_p = (r_p - u_p' gamma) w_p
//   qtlfam_finish_kernel  per chromosome and permuted column: the maximum over the chromosome's marker tiles
//
// No kernel adds with atomics; every sum runs in ascending order of the individuals within a family and of the families
// within a marker: a call gives the same bits every time, whatever the column tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlfam.h"

namespace cnf2 {

typedef double fd2 __attribute__((ext_vector_type(2)));
typedef double fd4 __attribute__((ext_vector_type(4)));

constexpr int QTLFAM_BLOCK = 128;     // >= QTL_NX * QTL_NX
constexpr int QTLFAM_WAVES = 4;       // waves per block: the same 16 markers, consecutive column groups
constexpr int QTLFAM_KU    = 4;       // k-steps of 4 slots requested together

__device__ __forceinline__ double qtlfam_row_x(const double* p, int side)
{
    const fd2 o01 = *(const fd2*)p, o23 = *(const fd2*)(p + 2);
    return qtlfam_x(o01.x, o01.y, o23.x, o23.y, side);
}

__global__ __launch_bounds__(QTLFAM_BLOCK) void qtlfam_mask_kernel(QtlFamParams q)
{
    __shared__ int cnt[QTLFAM_BLOCK], cells[QTLFAM_BLOCK];
    const int      c = blockIdx.x, tid = threadIdx.x;
    const int      first = q.cs[c];
    uint8_t*       cm = q.cmask + (size_t)c * q.n;
    int            mine = 0, mycells = 0;
    for (int i = tid; i < q.n; i += QTLFAM_BLOCK) {
        const double* o  = q.origin + ((size_t)i * q.M + first) * 4;
        const bool    on = q.use[i] && (o[0] != 0.0 || o[1] != 0.0 || o[2] != 0.0 || o[3] != 0.0);
        cm[i] = on ? 1 : 0;
        mine += on ? 1 : 0;
    }
    __threadfence_block();
    __syncthreads();
    for (int cq = tid; cq < q.Q; cq += QTLFAM_BLOCK) {
        bool any = false;
        for (int s = q.cellslot[cq]; s < q.cellslot[cq + 1]; s++) {
            const int i = q.gidx[s];
            any = any || (i >= 0 && cm[i]);
        }
        mycells += any ? 1 : 0;
    }
    cnt[tid]   = mine;
    cells[tid] = mycells;
    __syncthreads();
    if (tid == 0) {
        int n_c = 0, n_q = 0;
        for (int t = 0; t < QTLFAM_BLOCK; t++) n_c += cnt[t], n_q += cells[t];
        q.nc[c]     = n_c;
        q.ncells[c] = n_q;
    }
}
void launch_qtlfam_mask(const QtlFamParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlfam_mask_kernel, dim3(q.C), dim3(QTLFAM_BLOCK), 0, stream, q);
}

// One thread per (cell, column) of a chromosome, the columns fastest: the mean over the cell's used members in two passes,
// then every slot of the cell -- 0 for an empty slot and for an individual that is not used on the chromosome, so that the
// product never meets a value it did not write.  Column r0 + rr = pq * T + t of the phenotypes is pheno[i][t] (pq = 0) or
// pheno[perm[pq - 1][i]][t].
template <bool COV>
__global__ __launch_bounds__(256) void qtlfam_image_kernel(QtlFamParams q)
{
    const int    ncol = COV ? q.K : q.rn;
    const size_t e    = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)q.Q * ncol) return;
    const int      cq = (int)(e / ncol), col = (int)(e % ncol), c = blockIdx.y;
    const uint8_t* cm = q.cmask + (size_t)c * q.n;
    const int      gr = q.r0 + col, pq = COV ? 0 : gr / q.T, t = COV ? 0 : gr % q.T;
    auto val = [&](int s, double* v) {
        const int i = q.gidx[s];
        if (i < 0 || !cm[i]) return false;
        if (COV) *v = q.cov[(size_t)i * q.K + col];
        else *v = q.pheno[(size_t)(pq == 0 ? i : q.perm[(size_t)(pq - 1) * q.n + i]) * q.T + t];
        return true;
    };
    const int    s0 = q.cellslot[cq], s1 = q.cellslot[cq + 1];
    const double mean = qtlfam_cell_mean(s0, s1, val);
    double*      dst  = COV ? q.Z + (size_t)c * q.S * QTL_MAXK : q.Y + (size_t)c * q.S * q.rstride;
    const int    ds   = COV ? QTL_MAXK : q.rstride;
    for (int s = s0; s < s1; s++) {
        double v;
        dst[(size_t)s * ds + col] = val(s, &v) ? v - mean : 0.0;
    }
}
void launch_qtlfam_image(const QtlFamParams& q, bool covariates, hipStream_t stream)
{
    const size_t e = (size_t)q.Q * (covariates ? q.K : q.rn);
    if (e == 0) return;
    const dim3 grid((unsigned)((e + 255) / 256), q.C);
    if (covariates) hipLaunchKernelGGL(qtlfam_image_kernel<true>, grid, dim3(256), 0, stream, q);
    else hipLaunchKernelGGL(qtlfam_image_kernel<false>, grid, dim3(256), 0, stream, q);
}

__global__ __launch_bounds__(QTLFAM_BLOCK) void qtlfam_chrom_kernel(QtlFamParams q)
{
    __shared__ double S[QTL_NX * QTL_NX];
    const int         c = blockIdx.x, tid = threadIdx.x;
    const double*     Z = q.Z + (size_t)c * q.S * QTL_MAXK;
    const int         j = tid / QTL_NX, k = tid % QTL_NX;
    double            s = 0.0;
    if (tid < QTL_NX * QTL_NX && j < q.K && k <= j)
        for (int i = 0; i < q.S; i++) s += Z[(size_t)i * QTL_MAXK + j] * Z[(size_t)i * QTL_MAXK + k];
    if (tid < QTL_NX * QTL_NX) S[tid] = s;
    __syncthreads();
    double* out = q.chrom + (size_t)c * QTLFAM_CHROM;
    if (tid < QTL_NX * QTL_NX) out[tid] = S[tid];
    __syncthreads();
    if (tid == 0) {
        const bool ok = qtl_cholesky(S, q.K);
        for (int t = 0; t < QTL_NX * QTL_NX; t++) out[QTL_NX * QTL_NX + t] = S[t];
        out[2 * QTL_NX * QTL_NX] = (ok && q.nc[c] - q.ncells[c] - q.K >= 2) ? 1.0 : 0.0;
    }
}
void launch_qtlfam_chrom(const QtlFamParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlfam_chrom_kernel, dim3(q.C), dim3(QTLFAM_BLOCK), 0, stream, q);
}

// one thread per (marker, family); the lanes of a wave read consecutive 32-byte rows of one individual
__global__ __launch_bounds__(64) void qtlfam_design_kernel(QtlFamParams q)
{
    const int m = blockIdx.x * 64 + threadIdx.x, f = blockIdx.y;
    if (m >= q.M) return;
    const int      c  = q.mchrom[m];
    const uint8_t* cm = q.cmask + (size_t)c * q.n;
    const double*  Z  = q.Z + (size_t)c * q.S * QTL_MAXK;
    const double*  o  = q.origin + (size_t)m * 4;
    const size_t   os = (size_t)q.M * 4;
    double         u[QTL_MAXK], d = 0.0, raw = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_MAXK; k++) u[k] = 0.0;
    for (int cq = q.famcell[f]; cq < q.famcell[f + 1]; cq++) {
        double sx = 0.0, sxx = 0.0;
        int    nq = 0;
        for (int s = q.cellslot[cq]; s < q.cellslot[cq + 1]; s++) {
            const int i = q.gidx[s];
            if (i < 0 || !cm[i]) continue;
            const double x = qtlfam_row_x(o + (size_t)i * os, q.side);
            sx += x, sxx += x * x, nq++;
#pragma unroll
            for (int k = 0; k < QTL_MAXK; k++)
                if (k < q.K) u[k] += x * Z[(size_t)s * QTL_MAXK + k];
        }
        if (nq > 0) d += sxx - sx * sx / nq, raw += sxx;
    }
    double* rec = q.rec + (size_t)f * (1 + q.K) * q.M + m;
    rec[0]      = qtlfam_weight(raw, d);
#pragma unroll
    for (int k = 0; k < QTL_MAXK; k++)
        if (k < q.K) rec[(size_t)(1 + k) * q.M] = u[k];
}
void launch_qtlfam_design(const QtlFamParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlfam_design_kernel, dim3((q.M + 63) / 64, q.F), dim3(64), 0, stream, q);
}

// one thread per marker: H over the fitted families in ascending order, its factor, df
__global__ __launch_bounds__(64) void qtlfam_marker_kernel(QtlFamParams q)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= q.M) return;
    const int     c  = q.mchrom[m];
    const double* ch = q.chrom + (size_t)c * QTLFAM_CHROM;
    double        H[QTLFAM_TRI], diag[QTL_MAXK], u[QTL_MAXK];
#pragma unroll
    for (int j = 0; j < QTL_MAXK; j++) {
        diag[j] = j < q.K ? ch[j * QTL_NX + j] : 0.0;
#pragma unroll
        for (int k = 0; k <= j; k++) H[qtlfam_tri(j, k)] = j < q.K ? ch[j * QTL_NX + k] : 0.0;
    }
    int fitted = 0;
    for (int f = 0; f < q.F; f++) {
        const double* rec = q.rec + (size_t)f * (1 + q.K) * q.M + m;
        const double  w   = rec[0];
        if (!(w > 0.0)) continue;
        fitted++;
#pragma unroll
        for (int k = 0; k < QTL_MAXK; k++) u[k] = k < q.K ? rec[(size_t)(1 + k) * q.M] : 0.0;
#pragma unroll
        for (int j = 0; j < QTL_MAXK; j++)
#pragma unroll
            for (int k = 0; k <= j; k++) H[qtlfam_tri(j, k)] -= u[j] * u[k] * w;
    }
    const bool ok = ch[2 * QTL_NX * QTL_NX] != 0.0 && qtlfam_factor(H, q.K, diag) && q.nc[c] - q.ncells[c] - q.K - fitted >= 1;
    q.df[m] = ok ? fitted : 0;
    const int nt = q.K * (q.K + 1) / 2;
#pragma unroll
    for (int t = 0; t < QTLFAM_TRI; t++)
        if (t < nt) q.hrec[(size_t)t * q.M + m] = H[t];
    q.hrec[(size_t)nt * q.M + m] = ok ? 1.0 : 0.0;
}
void launch_qtlfam_marker(const QtlFamParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlfam_marker_kernel, dim3((q.M + 63) / 64), dim3(64), 0, stream, q);
}

// one thread per (chromosome, column): b0 and yy over the slots in order, e0 = b0' S11^-1 b0, RSS0 = yy - e0
__global__ __launch_bounds__(64) void qtlfam_null_kernel(QtlFamParams q)
{
    const int rr = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (rr >= q.rn) return;
    const double* Z = q.Z + (size_t)c * q.S * QTL_MAXK;
    const double* Y = q.Y + (size_t)c * q.S * q.rstride;
    double        b[QTL_NX], z[QTL_NX], yy = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) b[k] = 0.0;
    for (int s = 0; s < q.S; s++) {
        const double y = Y[(size_t)s * q.rstride + rr];
#pragma unroll
        for (int k = 0; k < QTL_MAXK; k++)
            if (k < q.K) b[k] += Z[(size_t)s * QTL_MAXK + k] * y;
        yy += y * y;
    }
    const double* ch = q.chrom + (size_t)c * QTLFAM_CHROM;
    const bool    scanned = ch[2 * QTL_NX * QTL_NX] != 0.0;
    double        e0 = 0.0;
    if (scanned) {
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) z[k] = b[k];
        qtl_chol_solve(ch + QTL_NX * QTL_NX, q.K, z);
#pragma unroll
        for (int k = 0; k < QTL_MAXK; k++)
            if (k < q.K) e0 += b[k] * z[k];
    }
    const double rss0 = scanned ? yy - e0 : 0.0;
    double*      nq   = q.nullq + (size_t)c * (q.K + 2) * q.rstride;
#pragma unroll
    for (int k = 0; k < QTL_MAXK; k++)
        if (k < q.K) nq[(size_t)k * q.rstride + rr] = b[k];
    nq[(size_t)q.K * q.rstride + rr]       = e0;
    nq[(size_t)(q.K + 1) * q.rstride + rr] = rss0;
    const int gr = q.r0 + rr;
    if (gr < q.T) q.rss0[(size_t)gr * q.C + c] = rss0;
}
void launch_qtlfam_null(const QtlFamParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlfam_null_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

// The product, segmented by family.  A wave owns 16 markers of one chromosome x 16 NT columns, as qtl_scan_kernel
// (cnf2_qtl_kernels.hip) does: the columns are the rows of the result and the markers its columns, so that the 16 lanes of a
// result register hold 16 consecutive markers of one column.  It walks the slots of the gather list in order, four per
// v_mfma_f64_16x16x4_f64.  The marker operand comes from the origin rows in place: lane (marker, k) reads the individual of
// slot s0 + k from the list, then the 32 bytes of that individual at its marker, and forms x and the c-mask on the fly; the
// column operand is 16 consecutive doubles of the centred image's row s0 + k.  Neither goes through LDS.  Slots past the
// list, empty slots, markers past the chromosome's end and columns past the tile's are clamped addresses, zero operands
// and masked outputs: no load leaves its array.
// A step never straddles two families (the cells are padded to four slots), and the list says which steps end one.  There
// the accumulators are r_p: with the marker's record (w_p, u_p) -- read from the design kernel's records one family ahead --
// they are folded into the running sum r_p^2 w_p and into g's sum u_p r_p w_p, in registers, written out as the raw slope of
// an observed column, and cleared.  The branch is uniform over the wave.
// Epilogue, in registers: g = b0 - the sum, gamma = H^-1 g through the marker's packed factor, the cell (cnf2_qtlfam.h), and
// for the permuted columns the maximum over the tile's markers, one value per (tile, column).
// KB bounds the covariates of an instantiation and NT its column tiles: 4 NT (KB + 2) doubles of a lane are accumulators.
// With up to two covariates they leave room for two waves per SIMD; with eight the second bound would cost scratch.
template <int KB, int NT>
__global__ __launch_bounds__(64 * QTLFAM_WAVES, KB <= 2 ? 2 : 1) void qtlfam_scan_kernel(QtlFamParams q)
{
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int cb = (blockIdx.y * QTLFAM_WAVES + wib) * 16 * NT;
    if (cb >= q.rn) return;
    const int  oi = lane & 15, ok = lane >> 4;
    const bool mval = oi < len;
    const int  m = m0 + (mval ? oi : 0);
    const int  S = q.S, K = q.K, nsteps = S / 4;
    const size_t   M    = (size_t)q.M;
    const double*  orow = q.origin + (size_t)m * 4;
    const size_t   os   = M * 4;
    const uint8_t* cm   = q.cmask + (size_t)c * q.n;
    const double*  Y    = q.Y + (size_t)c * S * q.rstride;
    int  col[NT];
    bool cval[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int cc = cb + nt * 16 + oi;
        cval[nt] = cc < q.rn;
        col[nt]  = cval[nt] ? cc : 0;
    }
    fd4    acc[NT];
    double sr2[NT][4], gs[NT][4][KB];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        acc[nt] = fd4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            sr2[nt][reg] = 0.0;
#pragma unroll
            for (int k = 0; k < KB; k++) gs[nt][reg][k] = 0.0;
        }
    }
    // the record of the next family to end
    int    fold = 0, fam = q.folds[0];
    double w, u[KB];
    auto   load_record = [&]() {
        const double* rec = q.rec + (size_t)fam * (1 + K) * M + m;
        w = rec[0];
#pragma unroll
        for (int k = 0; k < KB; k++) u[k] = k < K ? rec[(size_t)(1 + k) * M] : 0.0;
    };
    load_record();

#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += 4 * QTLFAM_KU) {
        double x[QTLFAM_KU], y[QTLFAM_KU][NT];
        bool   in[QTLFAM_KU], end[QTLFAM_KU];
        int    ind[QTLFAM_KU];
#pragma unroll
        for (int uu = 0; uu < QTLFAM_KU; uu++) {
            const int s  = s0 + 4 * uu + ok;
            in[uu]       = s < S;
            const int sc = in[uu] ? s : S - 1;
            ind[uu]      = q.gidx[sc];
            const int step = (s0 >> 2) + uu;
            end[uu]      = step < nsteps && q.stepend[step < nsteps ? step : nsteps - 1] != 0;
#pragma unroll
            for (int nt = 0; nt < NT; nt++) y[uu][nt] = Y[(size_t)sc * q.rstride + col[nt]];
        }
#pragma unroll
        for (int uu = 0; uu < QTLFAM_KU; uu++) {
            const int  i  = ind[uu] < 0 ? 0 : ind[uu];
            const bool on = in[uu] && ind[uu] >= 0 && mval && cm[i] != 0;
            const double xv = qtlfam_row_x(orow + (size_t)i * os, q.side);
            x[uu] = on ? xv : 0.0;
        }
#pragma unroll
        for (int uu = 0; uu < QTLFAM_KU; uu++) {
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                const double yy = (in[uu] && cval[nt]) ? y[uu][nt] : 0.0;
                acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, x[uu], acc[nt], 0, 0, 0);
            }
            if (end[uu]) {
#pragma unroll
                for (int nt = 0; nt < NT; nt++) {
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const double r = acc[nt][reg];
                        qtlfam_fold<KB>(r, w, u, K, sr2[nt][reg], gs[nt][reg]);
                        const int rr = cb + nt * 16 + ok + 4 * reg, gr = q.r0 + rr;
                        if (q.slope && mval && rr < q.rn && gr < q.T) q.slope[((size_t)gr * M + m) * q.F + fam] = r;
                    }
                    acc[nt] = fd4{0.0, 0.0, 0.0, 0.0};
                }
                fold++;
                fam = q.folds[fold];
                load_record();
            }
        }
    }

    const int     nt_h    = K * (K + 1) / 2;
    const double* hl      = q.hrec + m;
    const bool    fitted  = hl[(size_t)nt_h * M] != 0.0;
    const int     n_c     = q.nc[c];
    const double* nq      = q.nullq + (size_t)c * (K + 2) * q.rstride;
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int  rr   = cb + nt * 16 + ok + 4 * reg;
            const bool rval = rr < q.rn;
            const int  rc   = rval ? rr : 0;
            double     g[QTL_MAXK], gamma[QTL_MAXK], gq = 0.0;
#pragma unroll
            for (int k = 0; k < QTL_MAXK; k++) {
                g[k] = 0.0;
                if (k < KB && k < K) g[k] = nq[(size_t)k * q.rstride + rc] - gs[nt][reg][k < KB ? k : 0];
                gamma[k] = g[k];
            }
            if (fitted) qtlfam_solve(hl, M, K, gamma);
#pragma unroll
            for (int k = 0; k < QTL_MAXK; k++)
                if (k < K) gq += g[k] * gamma[k];
            const double e0 = nq[(size_t)K * q.rstride + rc], rss0 = nq[(size_t)(K + 1) * q.rstride + rc];
            const double lod = qtlfam_cell(sr2[nt][reg], gq, e0, rss0, n_c, fitted);
            const int    gr  = q.r0 + rc;
            if (rval && mval && gr < q.T) {
                q.lod[(size_t)gr * M + m] = lod;
                if (q.gamma) {
#pragma unroll
                    for (int k = 0; k < QTL_MAXK; k++)
                        if (k < K) q.gamma[((size_t)gr * M + m) * K + k] = gamma[k];
                }
            }
            double v = (rval && mval) ? lod : 0.0;            // a LOD is never negative: 0 is the maximum's identity
            v = fmax(v, __shfl_xor(v, 1));
            v = fmax(v, __shfl_xor(v, 2));
            v = fmax(v, __shfl_xor(v, 4));
            v = fmax(v, __shfl_xor(v, 8));
            if (oi == 0 && rval && gr >= q.T) q.tilemax[(size_t)tile * q.rstride + rr] = v;
        }
}
void launch_qtlfam_scan(const QtlFamParams& q, hipStream_t stream)
{
    if (q.K <= 2) {
        const int cols = 16 * 4 * QTLFAM_WAVES;
        hipLaunchKernelGGL((qtlfam_scan_kernel<2, 4>), dim3(q.n_tiles, (q.rn + cols - 1) / cols), dim3(64 * QTLFAM_WAVES), 0, stream, q);
    } else {
        const int cols = 16 * 2 * QTLFAM_WAVES;
        hipLaunchKernelGGL((qtlfam_scan_kernel<QTL_MAXK, 2>), dim3(q.n_tiles, (q.rn + cols - 1) / cols), dim3(64 * QTLFAM_WAVES), 0, stream, q);
    }
}

// one thread per (observed column, marker, family), the families fastest: the raw r_p the product left becomes the slope
__global__ __launch_bounds__(256) void qtlfam_slope_kernel(QtlFamParams q)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)q.T * q.M * q.F) return;
    const int    f  = (int)(e % q.F);
    const size_t tm = e / q.F;
    const int    m  = (int)(tm % q.M);
    const int    nt_h = q.K * (q.K + 1) / 2;
    const double* rec = q.rec + (size_t)f * (1 + q.K) * q.M + m;
    const double  w   = rec[0];
    double        v   = (double)NAN;
    if (q.hrec[(size_t)nt_h * q.M + m] != 0.0 && w > 0.0) {
        double ug = 0.0;
        for (int k = 0; k < q.K; k++) ug += rec[(size_t)(1 + k) * q.M] * q.gamma[tm * q.K + k];
        v = (q.slope[e] - ug) * w;
    }
    q.slope[e] = v;
}
void launch_qtlfam_slope(const QtlFamParams& q, hipStream_t stream)
{
    const size_t e = (size_t)q.T * q.M * q.F;
    hipLaunchKernelGGL(qtlfam_slope_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, stream, q);
}

// perm_max[p][t][c] = the maximum over the chromosome's tiles, in ascending order (one thread per chromosome and column)
__global__ __launch_bounds__(64) void qtlfam_finish_kernel(QtlFamParams q)
{
    const int rr = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (rr >= q.rn) return;
    const int gr = q.r0 + rr;
    if (gr < q.T) return;
    double v = 0.0;
    for (int t = q.tile_start[c]; t < q.tile_start[c + 1]; t++) v = fmax(v, q.tilemax[(size_t)t * q.rstride + rr]);
    const int p = gr / q.T - 1, tr = gr % q.T;
    q.pmax[((size_t)p * q.T + tr) * q.C + c] = v;
}
void launch_qtlfam_finish(const QtlFamParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlfam_finish_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

} // namespace cnf2
