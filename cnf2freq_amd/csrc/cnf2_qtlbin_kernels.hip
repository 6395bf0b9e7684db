// cnf2_qtlbin_kernels.hip -- the kernels of the binary-trait single-locus scan (cnf2_qtl_scan_binary, include/cnf2hip.h):
// per marker and 0/1 phenotype column, observed and permuted, a logistic regression on the origin rows fitted by iteratively
// reweighted least squares (Newton's method).  The model and every decision about degenerate cells live in cnf2_qtlbin.h;
// this file forms the sums.
//
//   (qtl_chrom_kernel and qtl_gather_kernel of cnf2_qtl_kernels.hip make the masks, n_c and the column image)
//   qtlbin_rank_kernel    per marker: the unweighted normal matrix, the rank rule, which effects are kept; per chromosome
//                         whether it is scanned
//   qtlbin_null_kernel    one wavefront per (chromosome, column): n_1 and the null fit on X0
//   qtlbin_fit_kernel     the hot path: one wavefront per (marker, column) fit, from the null start to its stop
//   qtlbin_finish_kernel  per chromosome and permuted column: the maximum over the chromosome's marker tiles
//
// No kernel adds with atomics, the individuals of a fit are never split between waves, every lane walks its individuals in
// ascending order and the lanes' sums meet in a fixed butterfly: a call gives the same bits every time, whatever the column
// tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlbin.h"

namespace cnf2 {

typedef double qbd2 __attribute__((ext_vector_type(2)));

constexpr int QTLBIN_WAVES = QTLBIN_TILE;    // waves per block of the fit kernel: adjacent markers of one chromosome, the same column
constexpr int QTLBIN_NULL_WAVES = 4;         // waves per block of the null kernel: consecutive columns of one chromosome

// X0's row of individual i: the intercept, then the covariates
__device__ __forceinline__ void qtlbin_x0(const QtlbinParams& q, int i, int nx, double x[QTL_NX])
{
    x[0] = 1.0;
#pragma unroll
    for (int k = 1; k < QTL_NX; k++) x[k] = k < nx ? q.cov[(size_t)i * q.K + (k - 1)] : 0.0;
}

// one thread per marker; the lanes of a wave read consecutive 32-byte rows of one individual
__global__ __launch_bounds__(64) void qtlbin_rank_kernel(QtlbinParams q)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= q.M) return;
    const int         c  = q.mchrom[m];
    const uint8_t*    cm = q.cmask + (size_t)c * q.n;
    const double*     o  = q.origin + (size_t)m * 4;
    const size_t      os = (size_t)q.M * 4;
    const QtlemDesign ds = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
    bool              keep[QTLBIN_NE] = {true, true, true}, act[QTLBIN_W], scanned;
    qtlbin_active(ds, keep, act);
    QtlbinSums u;
    qtlbin_zero(u);
    for (int i = 0; i < q.n; i++) {
        if (!cm[i]) continue;
        const qbd2 o01 = *(const qbd2*)(o + (size_t)i * os), o23 = *(const qbd2*)(o + (size_t)i * os + 2);
        double     x0[QTL_NX], x[QTLBIN_W];
        qtlbin_x0(q, i, ds.nx, x0);
        qtlbin_row(ds, act, x0, o01.x, o01.y, o23.x, o23.y, x);
        qtlbin_raw_terms(u, act, x);
    }
    q.rank[m] = qtlbin_rank(u, ds, q.nc[c], keep, &scanned);
    q.keep[m] = (keep[0] ? 1 : 0) | (keep[1] ? 2 : 0) | (keep[2] ? 4 : 0);
    if (m == q.cs[c]) q.scan[c] = scanned ? 1 : 0;      // (every marker of a chromosome finds the same; its first one reports it)
}
void launch_qtlbin_rank(const QtlbinParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlbin_rank_kernel, dim3((q.M + 63) / 64), dim3(64), 0, stream, q);
}

// the sum over the 64 lanes, in every lane: a butterfly whose order is fixed, and both partners of a step add the same pair
__device__ __forceinline__ double qtlbin_wave_sum(double v)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
    return v;
}
__device__ __forceinline__ void qtlbin_wave_sums(QtlbinSums& u, const bool act[QTLBIN_W])
{
#pragma unroll
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) {
#pragma unroll
            for (int k = 0; k < QTLBIN_W; k++)
                if (k <= j && act[k]) u.G[qtlbin_at(j, k)] = qtlbin_wave_sum(u.G[qtlbin_at(j, k)]);
            u.s[j] = qtlbin_wave_sum(u.s[j]);
        }
    u.ll = qtlbin_wave_sum(u.ll);
}

// One wave per (chromosome, column): n_1, then IRLS on X0 from (logit(n_1 / n_c), 0, ..).  Lane l walks the individuals
// l, l + 64, .. in ascending order, as the fit kernel does.  nullq receives gamma0, l0 and whether the column is scanned on
// the chromosome; the observed columns report ll0 and n_ones.
__global__ __launch_bounds__(64 * QTLBIN_NULL_WAVES) void qtlbin_null_kernel(QtlbinParams q)
{
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rr = blockIdx.x * QTLBIN_NULL_WAVES + wib, c = blockIdx.y;
    if (rr >= q.rn) return;
    const QtlemDesign ds = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
    const int         nx = ds.nx, n = q.n, n_c = q.nc[c];
    const uint8_t*    cm = q.cmask + (size_t)c * n;
    const double*     Y  = q.Y + rr;
    const bool        scanned = q.scan[c] != 0;
    const bool        none[QTLBIN_NE] = {false, false, false};
    bool              act[QTLBIN_W];
    qtlbin_active(ds, none, act);
    double ones = 0.0;           // (a count below 2^53: exact in any order)
    for (int i = lane; i < n; i += 64)
        if (cm[i]) ones += Y[(size_t)i * q.rstride];
    const int n_1 = (int)qtlbin_wave_sum(ones);
    QtlbinFit f;
    bool      ok = qtlbin_null_start(f, n_1, n_c) && scanned;
    if (ok) {
#pragma unroll 1
        for (;;) {
            QtlbinSums u;
            qtlbin_zero(u);
#pragma unroll 1
            for (int i = lane; i < n; i += 64) {
                if (!cm[i]) continue;
                double x0[QTL_NX], x[QTLBIN_W];
                qtlbin_x0(q, i, nx, x0);
                qtlbin_row(ds, act, x0, 0.0, 0.0, 0.0, 0.0, x);
                qtlbin_terms(u, act, f.th, x, Y[(size_t)i * q.rstride]);
            }
            qtlbin_wave_sums(u, act);
            if (qtlbin_step(f, act, u, QTLBIN_NULL_ITER, QTLBIN_NULL_TOL, false)) break;
        }
        ok = qtlbin_null_ok(f);
    }
    if (lane != 0) return;
    double* nq = q.nullq + (size_t)c * QTLBIN_NULLQ * q.rstride + rr;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) nq[(size_t)k * q.rstride] = ok ? f.th[k] : 0.0;
    nq[(size_t)QTL_NX * q.rstride]       = ok ? f.ll : 0.0;
    nq[(size_t)(QTL_NX + 1) * q.rstride] = ok ? 1.0 : 0.0;
    const int gr = q.r0 + rr;
    if (gr < q.T) {
        q.ll0[(size_t)gr * q.C + c]    = ok ? f.ll : 0.0;
        q.n_ones[(size_t)gr * q.C + c] = n_1;
    }
}
void launch_qtlbin_null(const QtlbinParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlbin_null_kernel, dim3((q.rn + QTLBIN_NULL_WAVES - 1) / QTLBIN_NULL_WAVES, q.C), dim3(64 * QTLBIN_NULL_WAVES), 0,
                       stream, q);
}

// The fit.  A wave owns one (marker, column) cell from the null start to its stop: iteration counts differ from cell to cell,
// and no cell waits for another (the block's only barrier is at its end).  Lane l walks the individuals l, l + 64, .. in
// ascending order; per pass it keeps the packed lower triangle of G = X'WX, s = X'(y - p) and l of cnf2_qtlbin.h in
// registers, the wave adds them by the butterfly above, and every lane then takes the same step (the stopping rule, the
// Cholesky factor of G and the two substitutions) on the same values.  The four waves of a block take adjacent markers of one
// chromosome (no tile straddles a chromosome start) for the same column, so that their 32-byte rows share one 128-byte line.
// Markers past the tile's end fit nothing.
// NXT = K + 1 is a template argument: which places of X0 take part is then known to the compiler, which keeps sums, registers
// and instructions only for those (with two covariates 21 of the 78 entries of G); the effect places stay a runtime matter of
// the marker's rank.  The arithmetic on the places that take part is the same in every instance.
template <int NXT>
__global__ __launch_bounds__(64 * QTLBIN_WAVES) void qtlbin_fit_kernel(QtlbinParams q)
{
    __shared__ double wl[QTLBIN_WAVES];
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x, rr = blockIdx.y;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int gr = q.r0 + rr;
    double    lod = 0.0;
    if (wib < len) {
        const int         m  = m0 + wib;
        const QtlemDesign ds = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
        const int         nx = NXT, n = q.n;
        const double*     nq = q.nullq + (size_t)c * QTLBIN_NULLQ * q.rstride + rr;
        const bool        usable = nq[(size_t)(QTL_NX + 1) * q.rstride] != 0.0;     // (the null kernel looked at the chromosome)
        const double      ll0 = nq[(size_t)QTL_NX * q.rstride];
        const int         kb  = q.keep[m];
        bool              keep[QTLBIN_NE], act[QTLBIN_W];
#pragma unroll
        for (int e = 0; e < QTLBIN_NE; e++) keep[e] = ((kb >> e) & 1) != 0;
        qtlbin_active(ds, keep, act);
#pragma unroll
        for (int j = 0; j < QTL_NX; j++) act[j] = j < NXT;       // (what qtlbin_active found, as a constant)
        QtlbinFit f;
        int       iters = 0, status = 0;
        const bool fit = usable && kb != 0;
        if (fit) {
            double g0[QTL_NX];
#pragma unroll
            for (int k = 0; k < QTL_NX; k++) g0[k] = k < nx ? nq[(size_t)k * q.rstride] : 0.0;
            qtlbin_start(f, g0, nx, ll0);
            const uint8_t* cm = q.cmask + (size_t)c * n;
            const double*  o  = q.origin + (size_t)m * 4;
            const size_t   os = (size_t)q.M * 4;
            const double*  Y  = q.Y + rr;
#pragma unroll 1
            for (;;) {
                QtlbinSums u;
                qtlbin_zero(u);
#pragma unroll 1
                for (int i = lane; i < n; i += 64) {
                    if (!cm[i]) continue;
                    const qbd2 o01 = *(const qbd2*)(o + (size_t)i * os), o23 = *(const qbd2*)(o + (size_t)i * os + 2);
                    double     x0[QTL_NX], x[QTLBIN_W];
                    qtlbin_x0(q, i, nx, x0);
                    qtlbin_row(ds, act, x0, o01.x, o01.y, o23.x, o23.y, x);
                    qtlbin_terms(u, act, f.th, x, Y[(size_t)i * q.rstride]);
                }
                qtlbin_wave_sums(u, act);
                if (qtlbin_step(f, act, u, q.max_iter, q.tol, true)) break;
            }
            lod    = qtlbin_lod(f, ll0);
            iters  = f.iters;
            status = f.status;
        }
        if (lane == 0 && gr < q.T) {
            const size_t at = (size_t)gr * q.M + m;
            q.lod[at]    = lod;
            q.iters[at]  = iters;
            q.status[at] = status;
#pragma unroll
            for (int e = 0; e < QTLBIN_NE; e++)
                if (e < ds.ne) q.coef[at * ds.ne + e] = (fit && keep[e]) ? f.th[QTL_NX + e] : (double)NAN;
        }
    }
    if (gr < q.T) return;                    // (the whole block: gr is the block's)
    if (lane == 0) wl[wib] = lod;            // a LOD is never negative: 0 is the maximum's identity
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = wl[0];
#pragma unroll
        for (int w = 1; w < QTLBIN_WAVES; w++) v = fmax(v, wl[w]);
        q.tilemax[(size_t)tile * q.rstride + rr] = v;
    }
}
template <int NXT>
static void qtlbin_fit_launch(const QtlbinParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlbin_fit_kernel<NXT>, dim3(q.n_tiles, q.rn), dim3(64 * QTLBIN_WAVES), 0, stream, q);
}
void launch_qtlbin_fit(const QtlbinParams& q, hipStream_t stream)
{
    static_assert(QTL_NX == 9, "one instance per width of X0");
    switch (q.K + 1) {
    case 1: qtlbin_fit_launch<1>(q, stream); break;
    case 2: qtlbin_fit_launch<2>(q, stream); break;
    case 3: qtlbin_fit_launch<3>(q, stream); break;
    case 4: qtlbin_fit_launch<4>(q, stream); break;
    case 5: qtlbin_fit_launch<5>(q, stream); break;
    case 6: qtlbin_fit_launch<6>(q, stream); break;
    case 7: qtlbin_fit_launch<7>(q, stream); break;
    case 8: qtlbin_fit_launch<8>(q, stream); break;
    default: qtlbin_fit_launch<9>(q, stream); break;
    }
}

// perm_max[p][t][c] = the maximum over the chromosome's tiles, in ascending order (one thread per chromosome and column)
__global__ __launch_bounds__(64) void qtlbin_finish_kernel(QtlbinParams q)
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
void launch_qtlbin_finish(const QtlbinParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlbin_finish_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

} // namespace cnf2
