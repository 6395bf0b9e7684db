// cnf2_qtlcols_kernels.hip -- the kernels of the column scan (cnf2_qtl_scan_cols, include/cnf2hip.h): ordinary least squares
// of phenotype columns, observed and permuted, on [x0, s reg(m)] at every marker of one block.  The model's algebra and every
// decision about degenerate cells are cnf2_qtl.h's; this file forms the sums.  Its shape is cnf2_qtl_kernels.hip's:
//
//   qtlcols_null_kernel     S11 = x0'x0 and its Cholesky factor; usable = it has one and n >= nx + 3
//   qtlcols_design_kernel   per marker: S21, S22 (sums over the individuals in ascending order), G, the pivots of W, rank
//   qtlcols_gather_kernel   per column tile: the column image Y[n][rn] (observed and permuted phenotypes)
//   qtlcols_colnull_kernel  per column: b0 = x0'y, RSS0
//   qtlcols_scan_kernel     the hot path: C[(m, e)][r] = sum_i s_i reg(i, m, e) Y(i, r) on the f64 matrix cores, epilogue in registers
//   qtlcols_finish_kernel   per permuted column: the maximum over the block's marker tiles
//
// No kernel adds with atomics and every sum runs over the individuals in ascending order: a call gives the same bits every
// time, whatever the column tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlcols.h"

namespace cnf2 {

typedef double cd2 __attribute__((ext_vector_type(2)));
typedef double cd4 __attribute__((ext_vector_type(4)));

constexpr int QC_NULL_BLOCK = 128;     // >= QTL_NX * QTL_NX
constexpr int QC_NT         = 4;       // column tiles of 16 per wave
constexpr int QC_WAVES      = 4;       // waves per block: the same 16 markers, consecutive column groups
constexpr int QC_KU         = 4;       // k-steps of 4 individuals requested together

__global__ __launch_bounds__(QC_NULL_BLOCK) void qtlcols_null_kernel(QtlColsParams q)
{
    __shared__ double S[QTL_NX * QTL_NX];
    const int tid = threadIdx.x;
    if (tid < QTL_NX * QTL_NX) S[tid] = 0.0;
    __syncthreads();
    const int j = tid / QTL_NX, k = tid % QTL_NX;
    if (tid < QTL_NX * QTL_NX && j < q.nx && k <= j) {
        double s = 0.0;
        for (int i = 0; i < q.n; i++) s += q.x0[(size_t)i * q.nx + j] * q.x0[(size_t)i * q.nx + k];
        S[j * QTL_NX + k] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const bool ok = qtl_cholesky(S, q.nx);
        for (int t = 0; t < QTL_NX * QTL_NX; t++) q.chol[t] = S[t];
        q.chol[QTL_NX * QTL_NX] = (ok && q.n >= q.nx + 3) ? 1.0 : 0.0;
    }
}
void launch_qtlcols_null(const QtlColsParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlcols_null_kernel, dim3(1), dim3(QC_NULL_BLOCK), 0, stream, q);
}

// one thread per marker; the lanes of a wave read consecutive regressors of one individual
__global__ __launch_bounds__(64) void qtlcols_design_kernel(QtlColsParams q)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= q.M) return;
    const double* r  = q.reg + (size_t)m * q.ne;
    const size_t  rs = (size_t)q.M * q.ne;
    double        sa[QTL_NX], sd[QTL_NX], saa = 0.0, sad = 0.0, sdd = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) sa[k] = sd[k] = 0.0;
    for (int i = 0; i < q.n; i++) {
        const double s = q.scale ? q.scale[i] : 1.0;
        const double a = s * r[(size_t)i * rs], d = q.ne == 2 ? s * r[(size_t)i * rs + 1] : 0.0;
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < q.nx) {
                const double x = q.x0[(size_t)i * q.nx + k];
                sa[k] += a * x;
                sd[k] += d * x;
            }
        saa += a * a;
        sad += a * d;
        sdd += d * d;
    }
    q.rank[m] = qtl_marker_record(q.chol, q.nx, q.chol[QTL_NX * QTL_NX] != 0.0, sa, sd, saa, sad, sdd, q.ne == 1,
                                  q.mk + (size_t)m * QTL_MK);
}
void launch_qtlcols_design(const QtlColsParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlcols_design_kernel, dim3((q.M + 63) / 64), dim3(64), 0, stream, q);
}

// Y[i][rr] for column r0 + rr = p * T + t: pheno[i][t] (p = 0) or pheno[perm[p - 1][i]][t]
__global__ __launch_bounds__(256) void qtlcols_gather_kernel(QtlColsParams q)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)q.n * q.rn) return;
    const int i = (int)(e / q.rn), rr = (int)(e % q.rn);
    const int gr = q.r0 + rr, pq = gr / q.T, t = gr % q.T;
    const int src = pq == 0 ? i : q.perm[(size_t)(pq - 1) * q.n + i];
    q.Y[(size_t)i * q.rstride + rr] = q.pheno[(size_t)src * q.T + t];
}
void launch_qtlcols_gather(const QtlColsParams& q, hipStream_t stream)
{
    const size_t e = (size_t)q.n * q.rn;
    hipLaunchKernelGGL(qtlcols_gather_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, stream, q);
}

// one thread per column: b0 = x0'y and yy over the individuals in ascending order, RSS0 = yy - b0' S11^-1 b0
__global__ __launch_bounds__(64) void qtlcols_colnull_kernel(QtlColsParams q)
{
    const int rr = blockIdx.x * 64 + threadIdx.x;
    if (rr >= q.rn) return;
    double b[QTL_NX], z[QTL_NX], yy = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) b[k] = 0.0;
    for (int i = 0; i < q.n; i++) {
        const double y = q.Y[(size_t)i * q.rstride + rr];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < q.nx) b[k] += q.x0[(size_t)i * q.nx + k] * y;
        yy += y * y;
    }
    double rss0 = 0.0;
    if (q.chol[QTL_NX * QTL_NX] != 0.0) {
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) z[k] = b[k];
        qtl_chol_solve(q.chol, q.nx, z);
        double e = 0.0;
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < q.nx) e += b[k] * z[k];
        rss0 = yy - e;
    }
#pragma unroll
    for (int k = 0; k < QTL_NX; k++)
        if (k < q.nx) q.nullq[(size_t)k * q.rstride + rr] = b[k];
    q.nullq[(size_t)q.nx * q.rstride + rr] = rss0;
    const int gr = q.r0 + rr;
    if (gr < q.T) q.rss0[gr] = rss0;
}
void launch_qtlcols_colnull(const QtlColsParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlcols_colnull_kernel, dim3((q.rn + 63) / 64), dim3(64), 0, stream, q);
}

// The product, in qtl_scan_kernel's form (cnf2_qtl_kernels.hip, which documents the operand and result layout of
// v_mfma_f64_16x16x4_f64): a wave owns 16 markers x 64 columns and walks every individual in ascending order, four per
// instruction; the columns are the rows of the result and the markers its columns.  The marker operand comes straight from
// reg: lane (marker, k) reads the NE doubles of individual i0 + k at its marker -- 16 consecutive markers are 128 NE
// contiguous bytes -- and multiplies them by s of that individual; the column operand is 16 consecutive doubles of the
// image's row.  Individuals past n, markers past the block's end and columns past the tile's are clamped addresses, zero
// operands and masked outputs: no load leaves its array.
// Epilogue, in registers: v = C - G b0, the cell (cnf2_qtl.h), lod / coef of the observed columns, and for the permuted
// ones the maximum over the tile's markers, one value per (tile, column).
template <int NE>
__global__ __launch_bounds__(64 * QC_WAVES, 2) void qtlcols_scan_kernel(QtlColsParams q)
{
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x;
    const int m0 = tile * 16, len = min(16, q.M - m0);
    const int cb = (blockIdx.y * QC_WAVES + wib) * 16 * QC_NT;
    if (cb >= q.rn) return;
    const int  oi = lane & 15, ok = lane >> 4;
    const bool mval = oi < len;
    const int  m = m0 + (mval ? oi : 0);
    const int  n = q.n;
    const double* rrow = q.reg + (size_t)m * NE;
    const size_t  rs   = (size_t)q.M * NE;
    int  col[QC_NT];
    bool cval[QC_NT];
#pragma unroll
    for (int nt = 0; nt < QC_NT; nt++) {
        const int cc = cb + nt * 16 + oi;
        cval[nt] = cc < q.rn;
        col[nt]  = cval[nt] ? cc : 0;
    }
    cd4 accA[QC_NT], accD[QC_NT];
#pragma unroll
    for (int nt = 0; nt < QC_NT; nt++) accA[nt] = accD[nt] = cd4{0.0, 0.0, 0.0, 0.0};

#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += 4 * QC_KU) {
        double ra[QC_KU], rd[QC_KU], s[QC_KU];
        double y[QC_KU][QC_NT];
        bool   in[QC_KU];
#pragma unroll
        for (int u = 0; u < QC_KU; u++) {
            const int i  = i0 + 4 * u + ok;
            in[u]        = i < n;
            const int ic = in[u] ? i : n - 1;
            const double* p = rrow + (size_t)ic * rs;
            if (NE == 2) {
                const cd2 v = *(const cd2*)p;
                ra[u] = v.x, rd[u] = v.y;
            } else {
                ra[u] = *p, rd[u] = 0.0;
            }
            s[u] = q.scale ? q.scale[ic] : 1.0;
#pragma unroll
            for (int nt = 0; nt < QC_NT; nt++) y[u][nt] = q.Y[(size_t)ic * q.rstride + col[nt]];
        }
#pragma unroll
        for (int u = 0; u < QC_KU; u++) {
            const bool   on = in[u] && mval;
            const double a = on ? s[u] * ra[u] : 0.0;
            const double d = on ? s[u] * rd[u] : 0.0;
#pragma unroll
            for (int nt = 0; nt < QC_NT; nt++) {
                const double yy = (in[u] && cval[nt]) ? y[u][nt] : 0.0;
                accA[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, a, accA[nt], 0, 0, 0);
                if (NE == 2) accD[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, d, accD[nt], 0, 0, 0);
            }
        }
    }

    const double* rec = q.mk + (size_t)m * QTL_MK;
    double        ga[QTL_NX], gd[QTL_NX];
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) {
        ga[k] = k < q.nx ? rec[k] : 0.0;
        gd[k] = k < q.nx ? rec[QTL_NX + k] : 0.0;
    }
    const double pa = rec[QTL_PA], l = rec[QTL_L], pd = rec[QTL_PD];
    const bool   usable = q.chol[QTL_NX * QTL_NX] != 0.0;
#pragma unroll
    for (int nt = 0; nt < QC_NT; nt++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int  rr   = cb + nt * 16 + ok + 4 * reg;
            const bool rval = rr < q.rn;
            const int  rc   = rval ? rr : 0;
            double     gba = 0.0, gbd = 0.0;
#pragma unroll
            for (int k = 0; k < QTL_NX; k++)
                if (k < q.nx) {
                    const double b = q.nullq[(size_t)k * q.rstride + rc];
                    gba += ga[k] * b;
                    gbd += gd[k] * b;
                }
            const double  rss0 = q.nullq[(size_t)q.nx * q.rstride + rc];
            const QtlCell cell = qtl_cell(accA[nt][reg] - gba, accD[nt][reg] - gbd, pa, l, pd, rss0, n, usable);
            const int     gr   = q.r0 + rc;
            if (rval && mval && gr < q.T) {
                const size_t o = (size_t)gr * q.M + m;
                q.lod[o]          = cell.lod;
                q.coef[2 * o]     = cell.ca;
                q.coef[2 * o + 1] = cell.cd;
            }
            double v = (rval && mval) ? cell.lod : 0.0;       // a LOD is never negative: 0 is the maximum's identity
            v = fmax(v, __shfl_xor(v, 1));
            v = fmax(v, __shfl_xor(v, 2));
            v = fmax(v, __shfl_xor(v, 4));
            v = fmax(v, __shfl_xor(v, 8));
            if (oi == 0 && rval && gr >= q.T) q.tilemax[(size_t)tile * q.rstride + rr] = v;
        }
}
void launch_qtlcols_scan(const QtlColsParams& q, hipStream_t stream)
{
    const int  cols = 16 * QC_NT * QC_WAVES;
    const dim3 grid(q.n_tiles, (q.rn + cols - 1) / cols), block(64 * QC_WAVES);
    if (q.ne == 2) hipLaunchKernelGGL(qtlcols_scan_kernel<2>, grid, block, 0, stream, q);
    else hipLaunchKernelGGL(qtlcols_scan_kernel<1>, grid, block, 0, stream, q);
}

// perm_max[p][t] = the maximum over the block's tiles, in ascending order (one thread per column)
__global__ __launch_bounds__(64) void qtlcols_finish_kernel(QtlColsParams q)
{
    const int rr = blockIdx.x * 64 + threadIdx.x;
    if (rr >= q.rn) return;
    const int gr = q.r0 + rr;
    if (gr < q.T) return;
    double v = 0.0;
    for (int t = 0; t < q.n_tiles; t++) v = fmax(v, q.tilemax[(size_t)t * q.rstride + rr]);
    const int p = gr / q.T - 1, tr = gr % q.T;
    q.pmax[(size_t)p * q.T + tr] = v;
}
void launch_qtlcols_finish(const QtlColsParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlcols_finish_kernel, dim3((q.rn + 63) / 64), dim3(64), 0, stream, q);
}

} // namespace cnf2
