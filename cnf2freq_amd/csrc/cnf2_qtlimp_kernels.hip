// cnf2_qtlimp_kernels.hip -- the kernels of the multiple-imputation QTL scan (cnf2_qtl_scan_imp, include/cnf2hip.h): the
// single scan's model (cnf2_qtl.h) fitted to every draw of sampled inheritance states and the draws combined per
// (marker, column) on the likelihood scale.  What a state means and the recurrence of the combination live in cnf2_qtlimp.h;
// the column image, the null fit and the finish are the single scan's launches (cnf2_qtl_kernels.hip).
//
//   qtlimp_check_kernel   per (individual, chromosome, draw): values below 64 or 0xFF, an individual skipped on all of a
//                         chromosome's cells or on none
//   qtlimp_chrom_kernel   per chromosome: c_i from the states, n_c, S11 = X0'X0 and its Cholesky factor
//   qtlimp_design_kernel  per (draw, marker): S21, S22 (diagonal: a d = 0), G, the pivots of W
//   qtlimp_rank_kernel    per marker: the smallest rank over the draws
//   qtlimp_scan_kernel    the hot path: per draw C[(m, a|d)][r] = sum_i A_d(m, i) Y(i, r) on the f64 matrix cores with the
//                         operand built from the state bytes, the cell, and the recurrence over the draws in registers
//
// No kernel adds with atomics, every sum runs over the individuals in ascending order and the draws are combined in
// ascending order: a call gives the same bits every time, whatever the column tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlimp.h"

namespace cnf2 {

typedef double qid4 __attribute__((ext_vector_type(4)));

constexpr int QTLIMP_CHROM_BLOCK = 128;     // >= QTL_NX * QTL_NX
constexpr int QTLIMP_WAVES       = 4;       // waves per block: consecutive marker tiles, the same 16 columns
constexpr int QTLIMP_KU          = 4;       // k-steps of 4 individuals requested together

__device__ __forceinline__ double qtlimp_x(const QtlParams& q, int i, int k) { return k == 0 ? 1.0 : q.cov[(size_t)i * q.K + (k - 1)]; }
__device__ __forceinline__ size_t qtlimp_stride(const QtlImpParams& p) { return (size_t)p.D * p.q.M; }

// One thread per (individual, chromosome, draw) walks the chromosome's bytes of its draw and compares them with the
// individual's first cell of the chromosome.  Every thread that finds something stores the same 1: no atomics.
__global__ __launch_bounds__(256) void qtlimp_check_kernel(QtlImpParams p)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)p.q.n * p.q.C * p.D) return;
    const int      d = (int)(e % p.D), c = (int)(e / p.D % p.q.C), i = (int)(e / p.D / p.q.C);
    const int      first = p.q.cs[c], len = p.q.cs[c + 1] - first;
    const uint8_t* row = p.state + (size_t)i * qtlimp_stride(p);
    const bool     skipped = row[first] == QTLIMP_SKIPPED;
    bool           range = false, partial = false;
    for (int j = 0; j < len; j++) {
        const uint8_t g = row[(size_t)d * p.q.M + first + j];
        range   = range || (g >= 64 && g != QTLIMP_SKIPPED);
        partial = partial || ((g == QTLIMP_SKIPPED) != skipped);
    }
    if (range) p.bad[0] = 1;
    if (partial) p.bad[1] = 1;
}
void launch_qtlimp_check(const QtlImpParams& p, hipStream_t stream)
{
    const size_t e = (size_t)p.q.n * p.q.C * p.D;
    hipLaunchKernelGGL(qtlimp_check_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, stream, p);
}

// qtl_chrom_kernel with the mask of the states: c_i = use[i] and the first draw's state at the chromosome's first marker
// is not "skipped"
__global__ __launch_bounds__(QTLIMP_CHROM_BLOCK) void qtlimp_chrom_kernel(QtlImpParams p)
{
    const QtlParams& q = p.q;
    __shared__ int    cnt[QTLIMP_CHROM_BLOCK];
    __shared__ double S[QTL_NX * QTL_NX];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int first = q.cs[c];
    uint8_t*  cm = q.cmask + (size_t)c * q.n;
    int       mine = 0;
    for (int i = tid; i < q.n; i += QTLIMP_CHROM_BLOCK) {
        const bool on = q.use[i] && p.state[(size_t)i * qtlimp_stride(p) + first] != QTLIMP_SKIPPED;
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
            if (cm[i]) s += qtlimp_x(q, i, j) * qtlimp_x(q, i, k);
        S[j * QTL_NX + k] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int n_c = 0;
        for (int t = 0; t < QTLIMP_CHROM_BLOCK; t++) n_c += cnt[t];
        q.nc[c] = n_c;
        const bool ok = qtl_cholesky(S, q.nx);
        double*    out = q.chol + (size_t)c * QTL_CHOL;
        for (int t = 0; t < QTL_NX * QTL_NX; t++) out[t] = S[t];
        out[QTL_NX * QTL_NX] = (ok && n_c >= q.K + 4) ? 1.0 : 0.0;
    }
}
void launch_qtlimp_chrom(const QtlImpParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlimp_chrom_kernel, dim3(p.q.C), dim3(QTLIMP_CHROM_BLOCK), 0, stream, p);
}

// One thread per (draw, marker); the lanes of a wave read 64 consecutive bytes of one individual's draw.  a and d are -1, 0
// or 1, so the sums are the single scan's on the draw's one-hot rows, term by term; S22 is diagonal.
__global__ __launch_bounds__(64) void qtlimp_design_kernel(QtlImpParams p)
{
    const QtlParams& q = p.q;
    const int        m = blockIdx.x * 64 + threadIdx.x, d = blockIdx.y;
    if (m >= q.M) return;
    const int      c  = q.mchrom[m];
    const uint8_t* cm = q.cmask + (size_t)c * q.n;
    const uint8_t* st = p.state + (size_t)d * q.M + m;
    const size_t   ss = qtlimp_stride(p);
    double         sa[QTL_NX], sd[QTL_NX], saa = 0.0, sdd = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) sa[k] = sd[k] = 0.0;
    for (int i = 0; i < q.n; i++) {
        if (!cm[i]) continue;
        const int    cls = qtlimp_class(st[(size_t)i * ss]);
        const double a = qtlimp_a(cls), dd = qtlimp_d(cls);
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < q.nx) {
                const double x = qtlimp_x(q, i, k);
                sa[k] += a * x;
                sd[k] += dd * x;
            }
        saa += a * a;
        sdd += dd * dd;
    }
    const double* L = q.chol + (size_t)c * QTL_CHOL;
    qtl_marker_record(L, q.nx, L[QTL_NX * QTL_NX] != 0.0, sa, sd, saa, 0.0, sdd, q.additive != 0,
                      p.mkd + ((size_t)d * q.M + m) * QTL_MK);
}
void launch_qtlimp_design(const QtlImpParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlimp_design_kernel, dim3((p.q.M + 63) / 64, p.D), dim3(64), 0, stream, p);
}

// a kept column has a positive pivot in its record and a dropped one 0 (qtl_marker_record): the rank is read from there
__global__ __launch_bounds__(64) void qtlimp_rank_kernel(QtlImpParams p)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= p.q.M) return;
    int rank = 2;
    for (int d = 0; d < p.D; d++) {
        const double* rec = p.mkd + ((size_t)d * p.q.M + m) * QTL_MK;
        rank = min(rank, (rec[QTL_PA] > 0.0 ? 1 : 0) + (rec[QTL_PD] > 0.0 ? 1 : 0));
    }
    p.q.rank[m] = rank;
}
void launch_qtlimp_rank(const QtlImpParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlimp_rank_kernel, dim3((p.q.M + 63) / 64), dim3(64), 0, stream, p);
}

// One draw's cell fed into its recurrence: the recurrence after it and the draw's own LOD, returned by value (in registers).
// Kept out of line: inlined four times, the logarithm and the power of the four cells a lane holds are interleaved and
// their temporaries take the kernel from 252 to 288 registers, one wave per SIMD instead of two.
struct QtlImpFed {
    QtlImpAcc acc;
    double    lod;
};
__device__ __noinline__ QtlImpFed qtlimp_feed(QtlImpAcc acc, bool first, double va, double vd, double pa, double l, double pd,
                                              double rss0, int n_c, bool usable)
{
    const QtlCell cell = qtl_cell(va, vd, pa, l, pd, rss0, n_c, usable);
    if (first) qtlimp_first(acc, cell);
    else qtlimp_next(acc, cell);
    return QtlImpFed{acc, cell.lod};
}

// The product and the combination.  A wave owns 16 markers of one chromosome (a tile never straddles a chromosome start) x 16
// columns for all the draws.  Per draw it walks every individual in ascending order, four per v_mfma_f64_16x16x4_f64, in the
// single scan's orientation (qtl_scan_kernel): the columns are the rows of the result and the markers its columns.  Lane
// (marker, k) reads the one state byte of individual i0 + k at its marker -- the 16 lanes of a k read 16 consecutive bytes,
// the tile's bytes of that individual and draw -- and forms a, d and the c-mask on the fly; the column operand is 16
// consecutive doubles of the image's row.  Neither goes through LDS.  The four waves of a block take consecutive marker tiles
// and the same columns, so that on a chromosome they read 64 consecutive bytes of an individual's draw, half a cache line,
// and the same image rows at the same time.  Individuals past n, markers past the tile's end and columns past the column
// tile's are clamped addresses, zero operands and masked outputs: no load leaves its array.
// After a draw's walk, in registers: v = C - G b0 with the draw's record, the cell (cnf2_qtl.h), and the recurrence
// (cnf2_qtlimp.h); after the last draw lod / coef of the observed columns and for the permuted ones the maximum of the
// combined LOD over the tile's markers (a butterfly over the 16 lanes of a register), one value per (tile, column).
__global__ __launch_bounds__(64 * QTLIMP_WAVES) void qtlimp_scan_kernel(QtlImpParams p)
{
    const QtlParams& q = p.q;
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x * QTLIMP_WAVES + wib;
    if (tile >= q.n_tiles) return;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int cb = blockIdx.y * 16;
    const int  oi = lane & 15, ok = lane >> 4;
    const bool mval = oi < len;
    const int  m = m0 + (mval ? oi : 0);
    const int  n = q.n;
    const size_t   ss = qtlimp_stride(p);
    const uint8_t* cm = q.cmask + (size_t)c * n;
    const bool     cval = cb + oi < q.rn;
    const int      col  = cval ? cb + oi : 0;

    const int     n_c    = q.nc[c];
    const bool    usable = q.chol[(size_t)c * QTL_CHOL + QTL_NX * QTL_NX] != 0.0;
    const double* nq     = q.nullq + (size_t)c * (q.nx + 1) * q.rstride;
    QtlImpAcc acc[4];

#pragma unroll 1
    for (int d = 0; d < p.D; d++) {
        const uint8_t* st = p.state + (size_t)d * q.M + m;
        qid4 accA = qid4{0.0, 0.0, 0.0, 0.0}, accD = qid4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int i0 = 0; i0 < n; i0 += 4 * QTLIMP_KU) {
            uint8_t g[QTLIMP_KU];
            double  y[QTLIMP_KU];
            bool    in[QTLIMP_KU], on[QTLIMP_KU];
#pragma unroll
            for (int u = 0; u < QTLIMP_KU; u++) {
                const int i  = i0 + 4 * u + ok;
                in[u]        = i < n;
                const int ic = in[u] ? i : n - 1;
                g[u]  = st[(size_t)ic * ss];
                on[u] = in[u] && mval && cm[ic] != 0;
                y[u]  = q.Y[(size_t)ic * q.rstride + col];
            }
#pragma unroll
            for (int u = 0; u < QTLIMP_KU; u++) {
                const int    cls = qtlimp_class(g[u]);
                const double a   = on[u] ? qtlimp_a(cls) : 0.0;
                const double dd  = on[u] ? qtlimp_d(cls) : 0.0;
                const double yy  = (in[u] && cval) ? y[u] : 0.0;
                accA = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, a, accA, 0, 0, 0);
                accD = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, dd, accD, 0, 0, 0);
            }
        }

        const double* rec = p.mkd + ((size_t)d * q.M + m) * QTL_MK;
        double        ga[QTL_NX], gd[QTL_NX];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) {
            ga[k] = k < q.nx ? rec[k] : 0.0;
            gd[k] = k < q.nx ? rec[QTL_NX + k] : 0.0;
        }
        const double pa = rec[QTL_PA], l = rec[QTL_L], pd = rec[QTL_PD];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int  rr   = cb + ok + 4 * reg;
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
            const QtlImpFed fed = qtlimp_feed(acc[reg], d == 0, accA[reg] - gba, accD[reg] - gbd, pa, l, pd, rss0, n_c, usable);
            acc[reg] = fed.acc;
            const int gr = q.r0 + rc;
            if (p.draw_lod && rval && mval && gr < q.T) p.draw_lod[((size_t)d * q.T + gr) * q.M + m] = fed.lod;
        }
    }

#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int     rr   = cb + ok + 4 * reg;
        const bool    rval = rr < q.rn;
        const int     gr   = q.r0 + (rval ? rr : 0);
        const QtlCell cell = qtlimp_result(acc[reg], p.D);
        if (rval && mval && gr < q.T) {
            const size_t o = (size_t)gr * q.M + m;
            q.lod[o]          = cell.lod;
            q.coef[2 * o]     = cell.ca;
            q.coef[2 * o + 1] = cell.cd;
        }
        double v = (rval && mval) ? cell.lod : 0.0;       // a combined LOD is never negative: 0 is the maximum's identity
        v = fmax(v, __shfl_xor(v, 1));
        v = fmax(v, __shfl_xor(v, 2));
        v = fmax(v, __shfl_xor(v, 4));
        v = fmax(v, __shfl_xor(v, 8));
        if (oi == 0 && rval && gr >= q.T) q.tilemax[(size_t)tile * q.rstride + rr] = v;
    }
}
void launch_qtlimp_scan(const QtlImpParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlimp_scan_kernel, dim3((p.q.n_tiles + QTLIMP_WAVES - 1) / QTLIMP_WAVES, (p.q.rn + 15) / 16),
                       dim3(64 * QTLIMP_WAVES), 0, stream, p);
}

}  // namespace cnf2
