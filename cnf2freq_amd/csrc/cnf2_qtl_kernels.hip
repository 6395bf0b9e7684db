// cnf2_qtl_kernels.hip -- the kernels of the QTL scan (cnf2_qtl_scan / cnf2_sweep_qtl, include/cnf2hip.h): Haley-Knott
// regression of phenotype columns, observed and permuted, on the origin rows of cnf2_sweep_origins.  The model and every
// decision about degenerate cells live in cnf2_qtl.h; this file forms the sums.
//
//   qtl_chrom_kernel   per chromosome: c_i, n_c, S11 = X0'X0 and its Cholesky factor
//   qtl_design_kernel  per marker: S21, S22 (sums over the individuals in ascending order), G, the pivots of W, rank
//   qtl_gather_kernel  per column tile: the column image Y[n][rn] (observed and permuted phenotypes; 0 where use is 0)
//   qtl_null_kernel    per chromosome and column: b0 = X0'y, RSS0
//   qtl_scan_kernel    the hot path: C[(m, a|d)][r] = sum_i A(m, i) Y(i, r) on the f64 matrix cores, epilogue in registers
//   qtl_finish_kernel  per chromosome and permuted column: the maximum over the chromosome's marker tiles
//
// No kernel adds with atomics and every sum runs over the individuals in ascending order: a call gives the same bits every
// time, whatever the column tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtl.h"

namespace cnf2 {

typedef double qd2 __attribute__((ext_vector_type(2)));
typedef double qd4 __attribute__((ext_vector_type(4)));

constexpr int QTL_CHROM_BLOCK = 128;     // >= QTL_NX * QTL_NX
constexpr int QTL_NT          = 4;       // column tiles of 16 per wave
constexpr int QTL_WAVES       = 4;       // waves per block: the same 16 markers, consecutive column groups
constexpr int QTL_KU          = 4;       // k-steps of 4 individuals requested together

// covariate k of individual i as column k of X0 (column 0 is the intercept)
__device__ __forceinline__ double qtl_x(const QtlParams& q, int i, int k) { return k == 0 ? 1.0 : q.cov[(size_t)i * q.K + (k - 1)]; }

__global__ __launch_bounds__(QTL_CHROM_BLOCK) void qtl_chrom_kernel(QtlParams q)
{
    __shared__ int    cnt[QTL_CHROM_BLOCK];
    __shared__ double S[QTL_NX * QTL_NX];
    const int      c = blockIdx.x, tid = threadIdx.x;
    const int      first = q.cs[c];
    uint8_t*       cm = q.cmask + (size_t)c * q.n;
    int            mine = 0;
    for (int i = tid; i < q.n; i += QTL_CHROM_BLOCK) {
        const double* o  = q.origin + ((size_t)i * q.M + first) * 4;
        const bool    on = q.use[i] && (o[0] != 0.0 || o[1] != 0.0 || o[2] != 0.0 || o[3] != 0.0);
        cm[i] = on ? 1 : 0;
        mine += on ? 1 : 0;
    }
    cnt[tid] = mine;
    if (tid < QTL_NX * QTL_NX) S[tid] = 0.0;
    __threadfence_block();
    __syncthreads();
    const int j = tid / QTL_NX, k = tid % QTL_NX;
    if (tid < QTL_NX * QTL_NX && j < q.nx && k <= j) {
        double s = 0.0;
        for (int i = 0; i < q.n; i++)
            if (cm[i]) s += qtl_x(q, i, j) * qtl_x(q, i, k);
        S[j * QTL_NX + k] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int n_c = 0;
        for (int t = 0; t < QTL_CHROM_BLOCK; t++) n_c += cnt[t];
        q.nc[c] = n_c;
        const bool ok = qtl_cholesky(S, q.nx);
        double*    out = q.chol + (size_t)c * QTL_CHOL;
        for (int t = 0; t < QTL_NX * QTL_NX; t++) out[t] = S[t];
        out[QTL_NX * QTL_NX] = (ok && n_c >= q.K + 4) ? 1.0 : 0.0;
    }
}
void launch_qtl_chrom(const QtlParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtl_chrom_kernel, dim3(q.C), dim3(QTL_CHROM_BLOCK), 0, stream, q);
}

// one thread per marker; the lanes of a wave read consecutive 32-byte rows of one individual
__global__ __launch_bounds__(64) void qtl_design_kernel(QtlParams q)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= q.M) return;
    const int      c  = q.mchrom[m];
    const uint8_t* cm = q.cmask + (size_t)c * q.n;
    const double*  o  = q.origin + (size_t)m * 4;
    const size_t   os = (size_t)q.M * 4;
    double         sa[QTL_NX], sd[QTL_NX], saa = 0.0, sad = 0.0, sdd = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) sa[k] = sd[k] = 0.0;
    for (int i = 0; i < q.n; i++) {
        if (!cm[i]) continue;
        const qd2    o01 = *(const qd2*)(o + (size_t)i * os), o23 = *(const qd2*)(o + (size_t)i * os + 2);
        const double a = o23.y - o01.x, d = o01.y + o23.x;
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < q.nx) {
                const double x = qtl_x(q, i, k);
                sa[k] += a * x;
                sd[k] += d * x;
            }
        saa += a * a;
        sad += a * d;
        sdd += d * d;
    }
    const double* L = q.chol + (size_t)c * QTL_CHOL;
    q.rank[m] = qtl_marker_record(L, q.nx, L[QTL_NX * QTL_NX] != 0.0, sa, sd, saa, sad, sdd, q.additive != 0,
                                  q.mk + (size_t)m * QTL_MK);
}
void launch_qtl_design(const QtlParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtl_design_kernel, dim3((q.M + 63) / 64), dim3(64), 0, stream, q);
}

// Y[i][rr] for column r0 + rr = q * T + t: pheno[i][t] (q = 0) or pheno[perm[q - 1][i]][t]; 0 for an individual that is not
// used (its phenotype may be NaN).  c_i differs by chromosome, so the A side of the product carries it.
__global__ __launch_bounds__(256) void qtl_gather_kernel(QtlParams q)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)q.n * q.rn) return;
    const int i = (int)(e / q.rn), rr = (int)(e % q.rn);
    const int gr = q.r0 + rr, pq = gr / q.T, t = gr % q.T;
    double    y = 0.0;
    if (q.use[i]) {
        const int src = pq == 0 ? i : q.perm[(size_t)(pq - 1) * q.n + i];
        y = q.pheno[(size_t)src * q.T + t];
    }
    q.Y[(size_t)i * q.rstride + rr] = y;
}
void launch_qtl_gather(const QtlParams& q, hipStream_t stream)
{
    const size_t e = (size_t)q.n * q.rn;
    hipLaunchKernelGGL(qtl_gather_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, stream, q);
}

// one thread per (chromosome, column): b0 = X0'y and yy over the individuals in ascending order, RSS0 = yy - b0' S11^-1 b0
__global__ __launch_bounds__(64) void qtl_null_kernel(QtlParams q)
{
    const int rr = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (rr >= q.rn) return;
    const uint8_t* cm = q.cmask + (size_t)c * q.n;
    double         b[QTL_NX], z[QTL_NX], yy = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) b[k] = 0.0;
    for (int i = 0; i < q.n; i++) {
        if (!cm[i]) continue;
        const double y = q.Y[(size_t)i * q.rstride + rr];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < q.nx) b[k] += qtl_x(q, i, k) * y;
        yy += y * y;
    }
    const double* L = q.chol + (size_t)c * QTL_CHOL;
    double        rss0 = 0.0;
    if (L[QTL_NX * QTL_NX] != 0.0) {
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) z[k] = b[k];
        qtl_chol_solve(L, q.nx, z);
        double e = 0.0;
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < q.nx) e += b[k] * z[k];
        rss0 = yy - e;
    }
    double* nq = q.nullq + (size_t)c * (q.nx + 1) * q.rstride;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++)
        if (k < q.nx) nq[(size_t)k * q.rstride + rr] = b[k];
    nq[(size_t)q.nx * q.rstride + rr] = rss0;
    const int gr = q.r0 + rr;
    if (gr < q.T) q.rss0[(size_t)gr * q.C + c] = rss0;
}
void launch_qtl_null(const QtlParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtl_null_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

// The product.  A wave owns 16 markers of one chromosome (a tile never straddles a chromosome start) x 64 columns and walks
// every individual in ascending order, four per v_mfma_f64_16x16x4_f64 (operand and result layouts: place_rows_kernel in
// cnf2_kernels.hip).  The columns are the rows of the result and the markers its columns, so that the 16 lanes of a result
// register hold 16 consecutive markers of one column: 128 contiguous bytes of lod[].  The marker operand comes straight from
// the origin rows: lane (marker, k) reads the 32 bytes of individual i0 + k at its marker -- 16 consecutive markers are 512
// contiguous bytes -- and forms a, d and the c-mask on the fly; the column operand is 16 consecutive doubles of the image's
// row.  Neither goes through LDS: every operand value is used by the lane that loaded it.  The four waves of a block take
// the same markers and consecutive column groups, so that they ask for the same origin rows at the same time.  Individuals
// past n, markers past the chromosome's end and columns past the tile's are clamped addresses, zero operands and masked
// outputs: nothing is padded in HBM and no load leaves its array.
// Epilogue, in registers: v = C - G b0, the cell (cnf2_qtl.h), lod / coef of the observed columns, and for the permuted
// ones the maximum over the tile's markers (a butterfly over the 16 lanes of a register), one value per (tile, column).
__global__ __launch_bounds__(64 * QTL_WAVES, 2) void qtl_scan_kernel(QtlParams q)
{
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int cb = (blockIdx.y * QTL_WAVES + wib) * 16 * QTL_NT;
    if (cb >= q.rn) return;
    const int  oi = lane & 15, ok = lane >> 4;
    const bool mval = oi < len;
    const int  m = m0 + (mval ? oi : 0);
    const int  n = q.n;
    const double*  orow = q.origin + (size_t)m * 4;
    const size_t   os   = (size_t)q.M * 4;
    const uint8_t* cm   = q.cmask + (size_t)c * n;
    int  col[QTL_NT];
    bool cval[QTL_NT];
#pragma unroll
    for (int nt = 0; nt < QTL_NT; nt++) {
        const int cc = cb + nt * 16 + oi;
        cval[nt] = cc < q.rn;
        col[nt]  = cval[nt] ? cc : 0;
    }
    qd4 accA[QTL_NT], accD[QTL_NT];
#pragma unroll
    for (int nt = 0; nt < QTL_NT; nt++) accA[nt] = accD[nt] = qd4{0.0, 0.0, 0.0, 0.0};

#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += 4 * QTL_KU) {
        qd2    o01[QTL_KU], o23[QTL_KU];
        double y[QTL_KU][QTL_NT];
        bool   in[QTL_KU], on[QTL_KU];
#pragma unroll
        for (int u = 0; u < QTL_KU; u++) {
            const int i  = i0 + 4 * u + ok;
            in[u]        = i < n;
            const int ic = in[u] ? i : n - 1;
            const double* p = orow + (size_t)ic * os;
            o01[u] = *(const qd2*)p;
            o23[u] = *(const qd2*)(p + 2);
            on[u]  = in[u] && mval && cm[ic] != 0;
#pragma unroll
            for (int nt = 0; nt < QTL_NT; nt++) y[u][nt] = q.Y[(size_t)ic * q.rstride + col[nt]];
        }
#pragma unroll
        for (int u = 0; u < QTL_KU; u++) {
            const double a = on[u] ? o23[u].y - o01[u].x : 0.0;
            const double d = on[u] ? o01[u].y + o23[u].x : 0.0;
#pragma unroll
            for (int nt = 0; nt < QTL_NT; nt++) {
                const double yy = (in[u] && cval[nt]) ? y[u][nt] : 0.0;
                accA[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, a, accA[nt], 0, 0, 0);
                accD[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, d, accD[nt], 0, 0, 0);
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
    const double  pa = rec[QTL_PA], l = rec[QTL_L], pd = rec[QTL_PD];
    const int     n_c    = q.nc[c];
    const bool    usable = q.chol[(size_t)c * QTL_CHOL + QTL_NX * QTL_NX] != 0.0;
    const double* nq     = q.nullq + (size_t)c * (q.nx + 1) * q.rstride;
#pragma unroll
    for (int nt = 0; nt < QTL_NT; nt++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int  rr   = cb + nt * 16 + ok + 4 * reg;
            const bool rval = rr < q.rn;
            const int  rc   = rval ? rr : 0;
            double     gba = 0.0, gbd = 0.0;
#pragma unroll
            for (int k = 0; k < QTL_NX; k++)
                if (k < q.nx) {
                    const double b = nq[(size_t)k * q.rstride + rc];
                    gba += ga[k] * b;
                    gbd += gd[k] * b;
                }
            const double  rss0 = nq[(size_t)q.nx * q.rstride + rc];
            const QtlCell cell = qtl_cell(accA[nt][reg] - gba, accD[nt][reg] - gbd, pa, l, pd, rss0, n_c, usable);
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
void launch_qtl_scan(const QtlParams& q, hipStream_t stream)
{
    const int cols = 16 * QTL_NT * QTL_WAVES;
    hipLaunchKernelGGL(qtl_scan_kernel, dim3(q.n_tiles, (q.rn + cols - 1) / cols), dim3(64 * QTL_WAVES), 0, stream, q);
}

// perm_max[p][t][c] = the maximum over the chromosome's tiles, in ascending order (one thread per chromosome and column)
__global__ __launch_bounds__(64) void qtl_finish_kernel(QtlParams q)
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
void launch_qtl_finish(const QtlParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtl_finish_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

} // namespace cnf2
