// cnf2_qtlvar_kernels.hip -- the kernels of the variance-QTL single-locus scan (cnf2_qtl_scan_var, include/cnf2hip.h): per
// marker and phenotype column, observed and permuted, the double generalised linear model on the origin rows -- a mean part
// and a log-variance part -- fitted three times (mean-only, variance-only, full) from the null fit.  The model, the iteration
// and every decision about degenerate cells live in cnf2_qtlvar.h; this file forms the sums.
//
//   (qtl_chrom_kernel and qtl_gather_kernel of cnf2_qtl_kernels.hip make the masks, n_c and the column image;
//    qtlbin_rank_kernel of cnf2_qtlbin_kernels.hip applies the rank rule)
//   qtlvar_threshold_kernel  per marker: this scan's threshold on n_c, on top of the rank rule's
//   qtlvar_null_kernel       one wavefront per (chromosome, column): the null fit on (X0, V0)
//   qtlvar_fit_kernel        the hot path: one wavefront per (marker, column) cell, its three fits in sequence
//   qtlvar_finish_kernel     per chromosome and permuted column: the maxima of the three LODs over the chromosome's tiles
//
// No kernel adds with atomics, the individuals of a fit are never split between waves, every lane walks its individuals in
// ascending order and the lanes' sums meet in a fixed butterfly: a call gives the same bits every time, whatever the column
// tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlvar.h"

namespace cnf2 {

typedef double qvd2 __attribute__((ext_vector_type(2)));

constexpr int QTLVAR_WAVES      = QTLBIN_TILE;   // waves per block of the fit kernel: adjacent markers of one chromosome, the same column
constexpr int QTLVAR_NULL_WAVES = 4;             // waves per block of the null kernel: consecutive columns of one chromosome

// one thread per marker: a chromosome with fewer individuals than both designs need is not scanned
__global__ __launch_bounds__(64) void qtlvar_threshold_kernel(QtlvarParams p)
{
    const QtlbinParams& q = p.b;
    const int           m = blockIdx.x * 64 + threadIdx.x;
    if (m >= q.M) return;
    const int         c  = q.mchrom[m];
    const QtlemDesign ds = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
    if (q.nc[c] >= qtlvar_min_n(ds, p.n_var)) return;
    q.rank[m] = 0;
    q.keep[m] = 0;
    if (m == q.cs[c]) q.scan[c] = 0;
}
void launch_qtlvar_threshold(const QtlvarParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlvar_threshold_kernel, dim3((p.b.M + 63) / 64), dim3(64), 0, stream, p);
}

// the sum and the maximum over the 64 lanes, in every lane: butterflies whose order is fixed
__device__ __forceinline__ double qtlvar_wave_sum(double v)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
    return v;
}
__device__ __forceinline__ double qtlvar_wave_max(double v)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v = fmax(v, __shfl_xor(v, k));
    return v;
}
__device__ __forceinline__ void qtlvar_wave_sums(QtlbinSums& u, const bool act[QTLBIN_W])
{
#pragma unroll
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) {
#pragma unroll
            for (int k = 0; k < QTLBIN_W; k++)
                if (k <= j && act[k]) u.G[qtlbin_at(j, k)] = qtlvar_wave_sum(u.G[qtlbin_at(j, k)]);
            u.s[j] = qtlvar_wave_sum(u.s[j]);
        }
}

// what a wave reads of its cell: the mask, the marker's origin rows (NULL: the null fit, without effects), the column
struct QtlvarCell {
    const uint8_t* cm;
    const double*  o;
    size_t         os;
    const double*  Y;
    size_t         ys;
    const double*  cov;
    int            K, n, n_c;
};

// x of individual i: X0's row, then every effect place of the design (the active masks choose among them)
template <int NXT>
__device__ __forceinline__ void qtlvar_x(const QtlvarCell& ce, const QtlemDesign& ds, const bool all[QTLBIN_W], int i, double x[QTLBIN_W])
{
    double x0[QTL_NX];
    x0[0] = 1.0;
#pragma unroll
    for (int k = 1; k < QTL_NX; k++) x0[k] = k < NXT ? ce.cov[(size_t)i * ce.K + (k - 1)] : 0.0;
    qvd2 o01 = {0.0, 0.0}, o23 = {0.0, 0.0};
    if (ce.o) {
        o01 = *(const qvd2*)(ce.o + (size_t)i * ce.os);
        o23 = *(const qvd2*)(ce.o + (size_t)i * ce.os + 2);
    }
    qtlbin_row(ds, all, x0, o01.x, o01.y, o23.x, o23.y, x);
}

// One fit from its start to its stop, by the wave: lane l walks the individuals l, l + 64, .. in ascending order.  An
// iteration costs two passes: step 2's, and one that forms l of the trial gamma' together with step 1's sums at gamma' for
// the next iteration (the weight exp(-eta) is the same); only a halving repeats it.  The first iteration's step 1 is a pass
// of its own.  Every lane takes the same decisions on the same values.
template <int NXT>
__device__ __forceinline__ void qtlvar_run(QtlvarFit& f, const QtlvarCell& ce, const QtlemDesign& ds, const bool all[QTLBIN_W],
                                           const bool actx[QTLBIN_W], const bool actv[QTLBIN_W], int lane, int max_iter, double tol)
{
    QtlbinSums u;
    qtlbin_zero(u);
#pragma unroll 1
    for (int i = lane; i < ce.n; i += 64) {
        if (!ce.cm[i]) continue;
        double x[QTLBIN_W];
        qtlvar_x<NXT>(ce, ds, all, i, x);
        qtlvar_mean_terms(u, actx, x, exp(-qtlvar_eta(actv, f.ga, x)), ce.Y[(size_t)i * ce.ys]);
    }
#pragma unroll 1
    for (;;) {
        qtlvar_wave_sums(u, actx);
        if (!qtlvar_beta(f, actx, u)) return;
        qtlbin_zero(u);
#pragma unroll 1
        for (int i = lane; i < ce.n; i += 64) {
            if (!ce.cm[i]) continue;
            double x[QTLBIN_W];
            qtlvar_x<NXT>(ce, ds, all, i, x);
            qtlvar_var_terms(u, actx, actv, f.bn, f.ga, x, ce.Y[(size_t)i * ce.ys]);
        }
        qtlvar_wave_sums(u, actv);
        if (!qtlvar_delta(f, actv, u)) return;
        int next;
#pragma unroll 1
        do {
            QtlvarTrial tr = {0.0, 0.0};
            qtlbin_zero(u);
#pragma unroll 1
            for (int i = lane; i < ce.n; i += 64) {
                if (!ce.cm[i]) continue;
                double x[QTLBIN_W];
                qtlvar_x<NXT>(ce, ds, all, i, x);
                const double y = ce.Y[(size_t)i * ce.ys];
                const double w = qtlvar_trial_terms(tr, actx, actv, f.bn, f.gt, x, y);
                qtlvar_mean_terms(u, actx, x, w, y);
            }
            next = qtlvar_accept(f, actv, qtlvar_ll(qtlvar_wave_sum(tr.s), ce.n_c), qtlvar_wave_max(tr.emax), max_iter, tol);
        } while (next == QTLVAR_HALVE);
        if (next == QTLVAR_OVER) return;
    }
}

// One wave per (chromosome, column): whether the column varies there, then the null fit.  nullq receives beta0, gamma0, l0
// and whether the column is scanned on the chromosome; the observed columns report ll0.
template <int NXT>
__global__ __launch_bounds__(64 * QTLVAR_NULL_WAVES) void qtlvar_null_kernel(QtlvarParams p)
{
    const QtlbinParams& q = p.b;
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rr = blockIdx.x * QTLVAR_NULL_WAVES + wib, c = blockIdx.y;
    if (rr >= q.rn) return;
    const QtlemDesign ds = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
    const int         n_var = p.n_var;
    const QtlvarCell  ce = {q.cmask + (size_t)c * q.n, nullptr, 0, q.Y + rr, (size_t)q.rstride, q.cov, q.K, q.n, q.nc[c]};
    const bool        none[QTLBIN_NE] = {false, false, false};
    bool              actx[QTLBIN_W], actv[QTLBIN_W];
    qtlvar_active(ds, n_var, none, -1, actx, actv);
#pragma unroll
    for (int j = 0; j < QTL_NX; j++) actx[j] = j < NXT;          // (what qtlvar_active found, as a constant)
    double yy = 0.0, lo = QTLBIN_DBL_MAX, hi = -QTLBIN_DBL_MAX;
    for (int i = lane; i < ce.n; i += 64)
        if (ce.cm[i]) {
            const double y = ce.Y[(size_t)i * ce.ys];
            yy += y * y;
            lo = fmin(lo, y);
            hi = fmax(hi, y);
        }
    yy = qtlvar_wave_sum(yy);
    lo = -qtlvar_wave_max(-lo);
    hi = qtlvar_wave_max(hi);
    QtlvarFit f;
    bool      ok = q.scan[c] != 0 && lo < hi;
    if (ok) {
        qtlvar_null_start(f, yy, ce.n_c);
        qtlvar_run<NXT>(f, ce, ds, actx, actx, actv, lane, QTLVAR_NULL_ITER, QTLVAR_NULL_TOL);
        ok = qtlvar_null_ok(f);
    }
    if (lane != 0) return;
    double* nq = q.nullq + (size_t)c * QTLVAR_NULLQ * q.rstride + rr;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) nq[(size_t)k * q.rstride] = (ok && k < NXT) ? f.be[k] : 0.0;
#pragma unroll
    for (int k = 0; k < QTLVAR_NV0; k++) nq[(size_t)(QTL_NX + k) * q.rstride] = (ok && k <= n_var) ? f.ga[k] : 0.0;
    nq[(size_t)(QTL_NX + QTLVAR_NV0) * q.rstride]     = ok ? f.ll : 0.0;
    nq[(size_t)(QTL_NX + QTLVAR_NV0 + 1) * q.rstride] = ok ? 1.0 : 0.0;
    const int gr = q.r0 + rr;
    if (gr < q.T) q.ll0[(size_t)gr * q.C + c] = ok ? f.ll : 0.0;
}
template <int NXT>
static void qtlvar_null_launch(const QtlvarParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlvar_null_kernel<NXT>, dim3((p.b.rn + QTLVAR_NULL_WAVES - 1) / QTLVAR_NULL_WAVES, p.b.C),
                       dim3(64 * QTLVAR_NULL_WAVES), 0, stream, p);
}

// The fit.  A wave owns one (marker, column) cell: its three fits in sequence, each from the null start to its stop, then the
// three LODs.  Iteration counts differ from cell to cell, and no cell waits for another (the block's only barrier is at its
// end).  The four waves of a block take adjacent markers of one chromosome (no tile straddles a chromosome start) for the
// same column, so that their 32-byte rows share one 128-byte line.  Markers past the tile's end fit nothing.
// NXT = K + 1 is a template argument, as in qtlbin_fit_kernel: the compiler keeps sums, registers and instructions only for
// the places of X0 that take part; which places of V0 and which effect places do stays a runtime matter.
// Up to K = 3 the sums of a pass and the iterate fit into 256 registers without scratch, and the instance is held to that, so
// that two waves share a SIMD; left to itself the compiler takes about 390 for every instance.  From K = 4 on that bound would
// cost scratch (72 B at K = 4 to 660 B at K = 8), and the instance keeps the whole file.
constexpr int qtlvar_fit_waves_per_simd(int nxt) { return nxt <= 4 ? 2 : 1; }
template <int NXT>
__global__ __launch_bounds__(64 * QTLVAR_WAVES, qtlvar_fit_waves_per_simd(NXT)) void qtlvar_fit_kernel(QtlvarParams p)
{
    __shared__ double   wl[QTLVAR_WAVES][QTLVAR_NFIT];
    const QtlbinParams& q = p.b;
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x, rr = blockIdx.y;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int gr = q.r0 + rr;
    double    lod[QTLVAR_NFIT] = {0.0, 0.0, 0.0};
    if (wib < len) {
        const int         m  = m0 + wib;
        const QtlemDesign ds = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
        const int         n_var = p.n_var;
        const double*     nq = q.nullq + (size_t)c * QTLVAR_NULLQ * q.rstride + rr;
        const bool        usable = nq[(size_t)(QTL_NX + QTLVAR_NV0 + 1) * q.rstride] != 0.0;
        const double      ll0 = nq[(size_t)(QTL_NX + QTLVAR_NV0) * q.rstride];
        const int         kb  = q.keep[m];
        bool              keep[QTLBIN_NE], all[QTLBIN_W];
#pragma unroll
        for (int e = 0; e < QTLBIN_NE; e++) keep[e] = ((kb >> e) & 1) != 0;
        qtlbin_active(ds, keep, all);
#pragma unroll
        for (int j = 0; j < QTL_NX; j++) all[j] = j < NXT;
        int        iters[QTLVAR_NFIT] = {0, 0, 0}, status[QTLVAR_NFIT] = {0, 0, 0};
        double     cmean[QTLBIN_NE], cvar[QTLBIN_NE];
        const bool fit = usable && kb != 0;
#pragma unroll
        for (int e = 0; e < QTLBIN_NE; e++) cmean[e] = cvar[e] = (double)NAN;
        if (fit) {
            double b0[QTL_NX], g0[QTLVAR_NV0], ll[QTLVAR_NFIT];
#pragma unroll
            for (int k = 0; k < QTL_NX; k++) b0[k] = k < NXT ? nq[(size_t)k * q.rstride] : 0.0;
#pragma unroll
            for (int k = 0; k < QTLVAR_NV0; k++) g0[k] = k <= n_var ? nq[(size_t)(QTL_NX + k) * q.rstride] : 0.0;
            const QtlvarCell ce = {q.cmask + (size_t)c * q.n, q.origin + (size_t)m * 4, (size_t)q.M * 4, q.Y + rr, (size_t)q.rstride, q.cov,
                                   q.K, q.n, q.nc[c]};
#pragma unroll 1
            for (int k = 0; k < QTLVAR_NFIT; k++) {
                bool actx[QTLBIN_W], actv[QTLBIN_W];
                qtlvar_active(ds, n_var, keep, k, actx, actv);
#pragma unroll
                for (int j = 0; j < QTL_NX; j++) actx[j] = j < NXT;
                QtlvarFit f;
                qtlvar_start(f, b0, NXT, g0, n_var, ll0);
                qtlvar_run<NXT>(f, ce, ds, all, actx, actv, lane, q.max_iter, q.tol);
                ll[k]     = f.ll;
                iters[k]  = f.iters;
                status[k] = f.status;
                if (k == QTLVAR_NFIT - 1) {
#pragma unroll
                    for (int e = 0; e < QTLBIN_NE; e++)
                        if (keep[e]) cmean[e] = f.be[QTL_NX + e], cvar[e] = f.ga[QTL_NX + e];
                }
            }
            qtlvar_lods(ll, ll0, lod);
        }
        if (lane == 0 && gr < q.T) {
            const size_t at = (size_t)gr * q.M + m;
#pragma unroll
            for (int k = 0; k < QTLVAR_NFIT; k++) {
                q.lod[at * QTLVAR_NFIT + k]    = lod[k];
                q.iters[at * QTLVAR_NFIT + k]  = iters[k];
                q.status[at * QTLVAR_NFIT + k] = status[k];
            }
#pragma unroll
            for (int e = 0; e < QTLBIN_NE; e++)
                if (e < ds.ne) {
                    q.coef[at * ds.ne + e]     = cmean[e];
                    p.coef_var[at * ds.ne + e] = cvar[e];
                }
        }
    }
    if (gr < q.T) return;                    // (the whole block: gr is the block's)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < QTLVAR_NFIT; k++) wl[wib][k] = lod[k];     // a LOD is never negative: 0 is the maximum's identity
    }
    __syncthreads();
    if (threadIdx.x < QTLVAR_NFIT) {
        double v = wl[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < QTLVAR_WAVES; w++) v = fmax(v, wl[w][threadIdx.x]);
        q.tilemax[((size_t)tile * QTLVAR_NFIT + threadIdx.x) * q.rstride + rr] = v;
    }
}
template <int NXT>
static void qtlvar_fit_launch(const QtlvarParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlvar_fit_kernel<NXT>, dim3(p.b.n_tiles, p.b.rn), dim3(64 * QTLVAR_WAVES), 0, stream, p);
}

#define CNF2_QTLVAR_INSTANCES(launch)                                                                                               \
    static_assert(QTL_NX == 9, "one instance per width of X0");                                                                     \
    switch (p.b.K + 1) {                                                                                                            \
    case 1: launch<1>(p, stream); break;                                                                                            \
    case 2: launch<2>(p, stream); break;                                                                                            \
    case 3: launch<3>(p, stream); break;                                                                                            \
    case 4: launch<4>(p, stream); break;                                                                                            \
    case 5: launch<5>(p, stream); break;                                                                                            \
    case 6: launch<6>(p, stream); break;                                                                                            \
    case 7: launch<7>(p, stream); break;                                                                                            \
    case 8: launch<8>(p, stream); break;                                                                                            \
    default: launch<9>(p, stream); break;                                                                                           \
    }
void launch_qtlvar_null(const QtlvarParams& p, hipStream_t stream) { CNF2_QTLVAR_INSTANCES(qtlvar_null_launch) }
void launch_qtlvar_fit(const QtlvarParams& p, hipStream_t stream) { CNF2_QTLVAR_INSTANCES(qtlvar_fit_launch) }

// perm_max[p][t][c][k] = the maximum of LOD k over the chromosome's tiles, in ascending order (one thread per chromosome and
// column)
__global__ __launch_bounds__(64) void qtlvar_finish_kernel(QtlvarParams p)
{
    const QtlbinParams& q = p.b;
    const int rr = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (rr >= q.rn) return;
    const int gr = q.r0 + rr;
    if (gr < q.T) return;
    const int pp = gr / q.T - 1, tr = gr % q.T;
#pragma unroll
    for (int k = 0; k < QTLVAR_NFIT; k++) {
        double v = 0.0;
        for (int t = q.tile_start[c]; t < q.tile_start[c + 1]; t++) v = fmax(v, q.tilemax[((size_t)t * QTLVAR_NFIT + k) * q.rstride + rr]);
        q.pmax[(((size_t)pp * q.T + tr) * q.C + c) * QTLVAR_NFIT + k] = v;
    }
}
void launch_qtlvar_finish(const QtlvarParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlvar_finish_kernel, dim3((p.b.rn + 63) / 64, p.b.C), dim3(64), 0, stream, p);
}

} // namespace cnf2
