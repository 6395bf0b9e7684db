// cnf2_qtlem_kernels.hip -- the kernels of the maximum-likelihood single-locus scan (cnf2_qtl_scan_em, include/cnf2hip.h):
// per marker and phenotype column, observed and permuted, the normal mixture over the four origin classes fitted by EM.  The
// model and every decision about degenerate cells live in cnf2_qtlem.h; this file forms the sums.
//
//   (qtl_chrom_kernel, qtl_gather_kernel and qtl_null_kernel of cnf2_qtl_kernels.hip make the masks, n_c, the factor of S11,
//    the column image and the null fit b0, RSS0)
//   qtlem_rank_kernel    per marker: the sums of the prior means, the rank rule, which effects are kept
//   qtlem_fit_kernel     the hot path: one wavefront per (marker, column) fit, from the null start to its stop
//   qtlem_finish_kernel  per chromosome and permuted column: the maximum over the chromosome's marker tiles
//
// No kernel adds with atomics, the individuals of a fit are never split between waves, every lane walks its individuals in
// ascending order and the lanes' sums meet in a fixed butterfly: a call gives the same bits every time, whatever the column
// tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlem.h"

namespace cnf2 {

typedef double qed2 __attribute__((ext_vector_type(2)));

constexpr int QTLEM_WAVES = QTLEM_TILE;      // waves per block: adjacent markers of one chromosome, the same column

// X0's row of individual i: the intercept, then the covariates
__device__ __forceinline__ void qtlem_x(const QtlemParams& q, int i, int nx, double x[QTL_NX])
{
    x[0] = 1.0;
#pragma unroll
    for (int k = 1; k < QTL_NX; k++) x[k] = k < nx ? q.cov[(size_t)i * q.K + (k - 1)] : 0.0;
}

// one thread per marker; the lanes of a wave read consecutive 32-byte rows of one individual
__global__ __launch_bounds__(64) void qtlem_rank_kernel(QtlemParams q)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= q.M) return;
    const int         c  = q.mchrom[m];
    const uint8_t*    cm = q.cmask + (size_t)c * q.n;
    const double*     o  = q.origin + (size_t)m * 4;
    const size_t      os = (size_t)q.M * 4;
    const QtlemDesign ds = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
    const double*     L  = q.chol + (size_t)c * QTL_CHOL;
    const bool        usable = qtlem_usable(L[QTL_NX * QTL_NX] != 0.0, q.nc[c], ds);
    QtlemSums         s;
    qtlem_zero(s);
    if (usable)
        for (int i = 0; i < q.n; i++) {
            if (!cm[i]) continue;
            const qed2 o01 = *(const qed2*)(o + (size_t)i * os), o23 = *(const qed2*)(o + (size_t)i * os + 2);
            double     pi[4], x[QTL_NX];
            if (!qtlem_prior(o01.x, o01.y, o23.x, o23.y, pi)) continue;
            qtlem_x(q, i, ds.nx, x);
            qtlem_prior_terms(s, pi, x, ds.nx);
        }
    bool keep[QTLEM_NE];
    q.rank[m] = qtlem_rank(L, ds, usable, s, keep);
    q.keep[m] = (keep[0] ? 1 : 0) | (keep[1] ? 2 : 0) | (keep[2] ? 4 : 0);
}
void launch_qtlem_rank(const QtlemParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlem_rank_kernel, dim3((q.M + 63) / 64), dim3(64), 0, stream, q);
}

// the sum over the 64 lanes, in every lane: a butterfly whose order is fixed, and both partners of a step add the same pair
__device__ __forceinline__ double qtlem_wave_sum(double v)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
    return v;
}

// The fit.  A wave owns one (marker, column) cell from the null start to its stop: iteration counts differ from cell to cell,
// and no cell waits for another (the block's only barrier is at its end).  Lane l walks the individuals l, l + 64, .. in
// ascending order; per pass it keeps the 3 (K + 1) + 4 + 3 + 1 sums of cnf2_qtlem.h in registers, the wave adds them by
// the butterfly above, and every lane then takes the same step (the stopping rule and the <= 3 x 3 Schur system) on the same
// values.  The four waves of a block take adjacent markers of one chromosome (no tile straddles a chromosome start) for the
// same column, so that their 32-byte rows share one 128-byte line.  Markers past the tile's end fit nothing.
__global__ __launch_bounds__(64 * QTLEM_WAVES) void qtlem_fit_kernel(QtlemParams q)
{
    __shared__ double wl[QTLEM_WAVES];
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x, rr = blockIdx.y;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int gr = q.r0 + rr;
    double    lod = 0.0;
    if (wib < len) {
        const int         m  = m0 + wib;
        const QtlemDesign ds = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
        const int         nx = ds.nx, n = q.n;
        const double*     L  = q.chol + (size_t)c * QTL_CHOL;
        const double*     nq = q.nullq + (size_t)c * (nx + 1) * q.rstride;
        const int         n_c  = q.nc[c];
        const double      rss0 = nq[(size_t)nx * q.rstride + rr];
        const bool        scanned = qtlem_usable(L[QTL_NX * QTL_NX] != 0.0, n_c, ds);
        const bool        usable  = scanned && rss0 > 0.0;
        const int         kb = q.keep[m];
        bool              keep[QTLEM_NE];
#pragma unroll
        for (int e = 0; e < QTLEM_NE; e++) keep[e] = ((kb >> e) & 1) != 0;
        QtlemFit f;
        double   sigma2 = (double)NAN;
        int      iters = 0, status = 0;
        if (usable) {
            double b0[QTL_NX];
#pragma unroll
            for (int k = 0; k < QTL_NX; k++) b0[k] = k < nx ? nq[(size_t)k * q.rstride + rr] : 0.0;
            qtlem_start(f, L, nx, b0, rss0, n_c);
            sigma2 = f.th.sigma2;
        }
        if (usable && kb != 0) {
            const uint8_t* cm = q.cmask + (size_t)c * n;
            const double*  o  = q.origin + (size_t)m * 4;
            const size_t   os = (size_t)q.M * 4;
            const double*  Y  = q.Y + rr;
#pragma unroll 1
            for (;;) {
                QtlemSums s;
                qtlem_zero(s);
#pragma unroll 1
                for (int i = lane; i < n; i += 64) {
                    if (!cm[i]) continue;
                    const qed2 o01 = *(const qed2*)(o + (size_t)i * os), o23 = *(const qed2*)(o + (size_t)i * os + 2);
                    double     pi[4], x[QTL_NX];
                    if (!qtlem_prior(o01.x, o01.y, o23.x, o23.y, pi)) continue;
                    qtlem_x(q, i, nx, x);
                    qtlem_terms(s, ds, keep, f.th, pi, x, Y[(size_t)i * q.rstride]);
                }
#pragma unroll
                for (int e = 0; e < QTLEM_NE; e++) {
#pragma unroll
                    for (int k = 0; k < QTL_NX; k++)
                        if (k < nx) s.s21[e][k] = qtlem_wave_sum(s.s21[e][k]);
                    s.r[e] = qtlem_wave_sum(s.r[e]);
                }
                s.saa = qtlem_wave_sum(s.saa);
                s.sdd = qtlem_wave_sum(s.sdd);
                s.sii = qtlem_wave_sum(s.sii);
                s.sdi = qtlem_wave_sum(s.sdi);
                s.ll  = qtlem_wave_sum(s.ll);
                if (qtlem_step(f, L, ds, keep, s, q.max_iter, q.tol)) break;
            }
            lod    = qtlem_lod(f);
            sigma2 = f.th.sigma2;
            iters  = f.iters;
            status = f.status;
        }
        if (lane == 0 && gr < q.T) {
            const size_t at = (size_t)gr * q.M + m;
            q.lod[at]    = lod;
            q.sigma2[at] = sigma2;
            q.iters[at]  = iters;
            q.status[at] = status;
            if (m == q.cs[c]) q.rss0[(size_t)gr * q.C + c] = scanned ? rss0 : 0.0;       // (the chromosome's first marker reports it)
#pragma unroll
            for (int e = 0; e < QTLEM_NE; e++)
                if (e < ds.ne) q.coef[at * ds.ne + e] = (usable && keep[e]) ? f.th.beta[e] : (double)NAN;
        }
    }
    if (gr < q.T) return;                    // (the whole block: gr is the block's)
    if (lane == 0) wl[wib] = lod;            // a LOD is never negative: 0 is the maximum's identity
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = wl[0];
#pragma unroll
        for (int w = 1; w < QTLEM_WAVES; w++) v = fmax(v, wl[w]);
        q.tilemax[(size_t)tile * q.rstride + rr] = v;
    }
}
void launch_qtlem_fit(const QtlemParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlem_fit_kernel, dim3(q.n_tiles, q.rn), dim3(64 * QTLEM_WAVES), 0, stream, q);
}

// perm_max[p][t][c] = the maximum over the chromosome's tiles, in ascending order (one thread per chromosome and column)
__global__ __launch_bounds__(64) void qtlem_finish_kernel(QtlemParams q)
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
void launch_qtlem_finish(const QtlemParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlem_finish_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

} // namespace cnf2
