// cnf2_qtlsurv_kernels.hip -- the kernels of the survival-trait single-locus scan (cnf2_qtl_scan_surv, include/cnf2hip.h):
// per marker and (time, status) column, observed and permuted, Cox's proportional hazards regression on the origin rows
// fitted by Newton's method.  The model and every decision about degenerate cells live in cnf2_qtlsurv.h and cnf2_qtlbin.h;
// this file forms the running sums along the risk order.
//
//   (qtl_chrom_kernel of cnf2_qtl_kernels.hip makes the masks and n_c; qtlbin_rank_kernel of cnf2_qtlbin_kernels.hip the
//    rank rule, with the intercept; the host the order words of a column tile, qtlsurv_order)
//   qtlsurv_null_kernel   one wavefront per (chromosome, column): n_events and the null fit on the covariates
//   qtlsurv_fit_kernel    the hot path: one wavefront per (marker, column) fit, from the null start to its stop
//   (qtlbin_finish_kernel: per chromosome and permuted column the maximum over the chromosome's marker tiles)
//
// A pass (qtlsurv_pass) walks the risk order in rounds of 64 positions, lane l at position 64 round + l: forward with an
// inclusive wave scan of w and w x_j plus the carries of the earlier rounds, then backward with a suffix scan of c.  c_r and
// w_r of a position wait for the backward pass in the wave's work row, written and read back by the same lane.  No kernel adds
// with atomics, the scans and the butterfly have a fixed order and a wave's sums do not depend on which block or wave forms
// them: a call gives the same bits every time, whatever the column tiling and the number of blocks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlsurv.h"

namespace cnf2 {

typedef double qsd2 __attribute__((ext_vector_type(2)));

// inclusive scans over the 64 lanes in six fixed steps: towards higher lanes, and towards lower ones
__device__ __forceinline__ double qtlsurv_scan_up(double v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ double qtlsurv_scan_down(double v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_down(v, d);
        if (lane + d < 64) v += t;
    }
    return v;
}
__device__ __forceinline__ int qtlsurv_iscan_up(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
// the largest value on the lanes below this one (0 on lane 0; the values are not negative)
__device__ __forceinline__ int qtlsurv_imax_below(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v = max(v, t);
    }
    const int t = __shfl_up(v, 1);
    return lane >= 1 ? t : 0;
}
// the sum over the 64 lanes, in every lane: a butterfly whose order is fixed (as the binary scan's)
__device__ __forceinline__ double qtlsurv_wave_sum(double v)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
    return v;
}

// x of individual i at the marker whose rows start at o (stride os doubles); o = nullptr: the null fit, no effects
__device__ __forceinline__ void qtlsurv_x(const QtlbinParams& q, const QtlemDesign& ds, const bool act[QTLBIN_W], int nx, const double* o,
                                          size_t os, int i, double x[QTLBIN_W])
{
    double x0[QTL_NX];
    x0[0] = 0.0;
#pragma unroll
    for (int k = 1; k < QTL_NX; k++) x0[k] = k < nx ? q.cov[(size_t)i * q.K + (k - 1)] : 0.0;
    qsd2 o01 = {0.0, 0.0}, o23 = {0.0, 0.0};
    if (o) {
        o01 = *(const qsd2*)(o + (size_t)i * os);
        o23 = *(const qsd2*)(o + (size_t)i * os + 2);
    }
    qtlbin_row(ds, act, x0, o01.x, o01.y, o23.x, o23.y, x);
}

// One pass at th: the sums of cnf2_qtlsurv.h in u, the same in every lane.  ord[n] the column's order words, cm[n] the
// chromosome's mask, wc[n] and ww[n] the wave's work rows.  Returns the number of unmasked events.
__device__ __forceinline__ int qtlsurv_pass(const QtlbinParams& q, const QtlemDesign& ds, const bool act[QTLBIN_W], int nx,
                                            const double th[QTLBIN_W], const uint32_t* ord, const uint8_t* cm, const double* o, double* wc,
                                            double* ww, int lane, QtlbinSums& u)
{
    const int    n = q.n, rounds = (n + 63) >> 6;
    const size_t os = (size_t)q.M * 4;
    qtlbin_zero(u);
    double cS0 = 0.0, cS1[QTLBIN_W];       // the carries: the running sums at the end of the round before,
    int    cE = 0, cB = 0;                 //   the unmasked events so far, and so far at the last group end
#pragma unroll
    for (int j = 0; j < QTLBIN_W; j++) cS1[j] = 0.0;
#pragma unroll 1
    for (int rd = 0; rd < rounds; rd++) {
        const int      r    = rd * 64 + lane;
        const bool     live = r < n;
        const uint32_t word = live ? ord[r] : 0u;
        const int      i    = (int)(word & QTLSURV_IND);
        const bool     on   = live && cm[i] != 0;
        const bool     ev   = on && (word & QTLSURV_EVENT) != 0;
        const bool     end  = live && (word & QTLSURV_END) != 0;
        double         x[QTLBIN_W], w = 0.0;
#pragma unroll
        for (int j = 0; j < QTLBIN_W; j++) x[j] = 0.0;
        if (on) {
            qtlsurv_x(q, ds, act, nx, o, os, i, x);
            const double eta = qtlsurv_eta(act, th, x);
            w = exp(eta);
            if (ev) qtlsurv_event_terms(u, act, x, eta);
        }
        const double S0 = cS0 + qtlsurv_scan_up(w, lane);
        double       S1[QTLBIN_W];
#pragma unroll
        for (int j = 0; j < QTLBIN_W; j++) S1[j] = act[j] ? cS1[j] + qtlsurv_scan_up(w * x[j], lane) : 0.0;
        const int E    = cE + qtlsurv_iscan_up(ev ? 1 : 0, lane);
        const int Bown = end ? E : 0;
        const int B    = max(cB, qtlsurv_imax_below(Bown, lane));       // the events up to the group end before this position
        double    c    = 0.0;
        if (end) c = qtlsurv_group_end(u, act, E - B, S0, S1);
        if (live) {
            wc[r] = c;
            ww[r] = w;
        }
        cS0 = __shfl(S0, 63);
#pragma unroll
        for (int j = 0; j < QTLBIN_W; j++)
            if (act[j]) cS1[j] = __shfl(S1[j], 63);
        cE = __shfl(E, 63);
        cB = __shfl(max(B, Bown), 63);
    }
    double cA = 0.0;                       // the sum of c over the later rounds
#pragma unroll 1
    for (int rd = rounds - 1; rd >= 0; rd--) {
        const int    r    = rd * 64 + lane;
        const bool   live = r < n;
        const double c = live ? wc[r] : 0.0, w = live ? ww[r] : 0.0;
        const double A = cA + qtlsurv_scan_down(c, lane);
        cA             = __shfl(A, 0);
        if (w != 0.0) {                    // (a masked individual has w = 0, and nothing of its row is read)
            double x[QTLBIN_W];
            qtlsurv_x(q, ds, act, nx, o, os, (int)(ord[r] & QTLSURV_IND), x);
            qtlsurv_back_terms(u, act, x, w * A);
        }
    }
#pragma unroll
    for (int j = 0; j < QTLBIN_W; j++)
        if (act[j]) {
#pragma unroll
            for (int k = 0; k < QTLBIN_W; k++)
                if (k <= j && act[k]) u.G[qtlbin_at(j, k)] = qtlsurv_wave_sum(u.G[qtlbin_at(j, k)]);
            u.s[j] = qtlsurv_wave_sum(u.s[j]);
        }
    u.ll = qtlsurv_wave_sum(u.ll);
    return cE;
}

// the places of X0 that take part, as constants: the covariates 1 .. NXT - 1
template <int NXT>
__device__ __forceinline__ void qtlsurv_act0(bool act[QTLBIN_W])
{
#pragma unroll
    for (int j = 0; j < QTL_NX; j++) act[j] = j >= 1 && j < NXT;
}

// One wave per (chromosome, column), the waves striding over those cells: the number of events and the null fit on the
// covariates from theta = 0.  nullq receives gamma0 (by place), l0 and whether the column is scanned on the chromosome; the
// observed columns report ll0 and n_events.
template <int NXT>
__global__ __launch_bounds__(64 * QTLSURV_WAVES) void qtlsurv_null_kernel(QtlsurvParams p)
{
    const QtlbinParams& q    = p.b;
    const int           lane = threadIdx.x & 63;
    const int           wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int           gw = blockIdx.x * QTLSURV_WAVES + wib, waves = gridDim.x * QTLSURV_WAVES, n = q.n;
    const QtlemDesign   ds = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
    double*             wc = p.work + (size_t)gw * 2 * n;
    double*             ww = wc + n;
    bool                act[QTLBIN_W];
#pragma unroll
    for (int j = 0; j < QTLBIN_W; j++) act[j] = false;
    qtlsurv_act0<NXT>(act);
#pragma unroll 1
    for (int cell = gw; cell < q.C * q.rn; cell += waves) {
        const int      c = cell / q.rn, rr = cell % q.rn;
        const uint8_t* cm = q.cmask + (size_t)c * n;
        double         g0[QTL_NX];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) g0[k] = 0.0;
        QtlsurvFit f;
        QtlbinSums u;
        qtlsurv_start(f, g0, NXT, 0.0);
        const int n_ev = qtlsurv_pass(q, ds, act, NXT, f.f.th, p.ord + (size_t)rr * n, cm, nullptr, wc, ww, lane, u);
        double    l0 = u.ll;
        bool      ok = q.scan[c] != 0 && n_ev > 0;
        if (ok && NXT > 1) {
#pragma unroll 1
            while (!qtlsurv_step(f, act, u, QTLSURV_NULL_ITER, QTLSURV_NULL_TOL, false))
                qtlsurv_pass(q, ds, act, NXT, f.f.th, p.ord + (size_t)rr * n, cm, nullptr, wc, ww, lane, u);
            l0 = f.f.ll;
        }
        ok = ok && qtlsurv_null_ok(f.f, NXT - 1, l0);
        if (lane == 0) {
            double* nq = q.nullq + (size_t)c * QTLBIN_NULLQ * q.rstride + rr;
    #pragma unroll
            for (int k = 0; k < QTL_NX; k++) nq[(size_t)k * q.rstride] = (ok && k < NXT) ? f.f.th[k] : 0.0;
            nq[(size_t)QTL_NX * q.rstride]       = ok ? l0 : 0.0;
            nq[(size_t)(QTL_NX + 1) * q.rstride] = ok ? 1.0 : 0.0;
            const int gr = q.r0 + rr;
            if (gr < q.T) {
                q.ll0[(size_t)gr * q.C + c]    = ok ? l0 : 0.0;
                q.n_ones[(size_t)gr * q.C + c] = n_ev;
            }
        }
    }
}

// The fit.  A wave owns one (marker, column) cell from the null start to its stop; the four waves of a block take adjacent
// markers of one chromosome (a tile of the marker map) for the same column, so that their 32-byte rows share one 128-byte
// line, and a block strides over the (tile, column) cells: the work rows are as many as the launch has waves, whatever the
// scan's size.  Markers past the tile's end fit nothing.  NXT = K + 1 is a template argument, as in the binary scan: sums,
// registers and instructions exist only for the covariates there are; the effect places stay a runtime matter of the marker's
// rank.
template <int NXT>
__global__ __launch_bounds__(64 * QTLSURV_WAVES) void qtlsurv_fit_kernel(QtlsurvParams p)
{
    __shared__ double   wl[QTLSURV_WAVES];
    const QtlbinParams& q    = p.b;
    const int           lane = threadIdx.x & 63;
    const int           wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int           n    = q.n;
    const QtlemDesign   ds   = qtlem_design(q.K, q.additive != 0, q.imprint != 0);
    double*             wc   = p.work + ((size_t)blockIdx.x * QTLSURV_WAVES + wib) * 2 * n;
    double*             ww   = wc + n;
#pragma unroll 1
    for (int cell = blockIdx.x; cell < q.n_tiles * q.rn; cell += gridDim.x) {
        const int tile = cell % q.n_tiles, rr = cell / q.n_tiles;
        const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
        const int gr = q.r0 + rr;
        double    lod = 0.0;
        if (wib < len) {
            const int     m  = m0 + wib;
            const double* nq = q.nullq + (size_t)c * QTLBIN_NULLQ * q.rstride + rr;
            const bool    usable = nq[(size_t)(QTL_NX + 1) * q.rstride] != 0.0;
            const double  ll0 = nq[(size_t)QTL_NX * q.rstride];
            const int     kb  = q.keep[m];
            bool          keep[QTLBIN_NE], act[QTLBIN_W];
#pragma unroll
            for (int e = 0; e < QTLBIN_NE; e++) keep[e] = ((kb >> e) & 1) != 0;
            qtlsurv_active(ds, keep, act);
            qtlsurv_act0<NXT>(act);
            QtlsurvFit f;
            QtlbinSums u;
            int        iters = 0, status = 0;
            const bool fit = usable && kb != 0;
            if (fit) {
                double g0[QTL_NX];
#pragma unroll
                for (int k = 0; k < QTL_NX; k++) g0[k] = (k >= 1 && k < NXT) ? nq[(size_t)k * q.rstride] : 0.0;
                qtlsurv_start(f, g0, NXT, ll0);
                const uint8_t* cm = q.cmask + (size_t)c * n;
                const double*  o  = q.origin + (size_t)m * 4;
#pragma unroll 1
                for (;;) {
                    qtlsurv_pass(q, ds, act, NXT, f.f.th, p.ord + (size_t)rr * n, cm, o, wc, ww, lane, u);
                    if (qtlsurv_step(f, act, u, q.max_iter, q.tol, true)) break;
                }
                lod    = qtlbin_lod(f.f, ll0);
                iters  = f.f.iters;
                status = f.f.status;
            }
            if (lane == 0 && gr < q.T) {
                const size_t at = (size_t)gr * q.M + m;
                q.lod[at]    = lod;
                q.iters[at]  = iters;
                q.status[at] = status;
#pragma unroll
                for (int e = 0; e < QTLBIN_NE; e++)
                    if (e < ds.ne) q.coef[at * ds.ne + e] = (fit && keep[e]) ? f.f.th[QTL_NX + e] : (double)NAN;
            }
        }
        if (gr < q.T) continue;                  // (the whole block: gr is the block's)
        if (lane == 0) wl[wib] = lod;            // a LOD is never negative: 0 is the maximum's identity
        __syncthreads();
        if (threadIdx.x == 0) {
            double v = wl[0];
#pragma unroll
            for (int w = 1; w < QTLSURV_WAVES; w++) v = fmax(v, wl[w]);
            q.tilemax[(size_t)tile * q.rstride + rr] = v;
        }
        __syncthreads();                         // (wl is the next cell's too)
    }
}

template <int NXT>
static void qtlsurv_launch(const QtlsurvParams& p, hipStream_t stream, bool fit)
{
    if (fit) hipLaunchKernelGGL(qtlsurv_fit_kernel<NXT>, dim3(p.fit_blocks), dim3(64 * QTLSURV_WAVES), 0, stream, p);
    else hipLaunchKernelGGL(qtlsurv_null_kernel<NXT>, dim3(p.null_blocks), dim3(64 * QTLSURV_WAVES), 0, stream, p);
}
static void qtlsurv_dispatch(const QtlsurvParams& p, hipStream_t stream, bool fit)
{
    static_assert(QTL_NX == 9, "one instance per width of X0");
    switch (p.b.K + 1) {
    case 1: qtlsurv_launch<1>(p, stream, fit); break;
    case 2: qtlsurv_launch<2>(p, stream, fit); break;
    case 3: qtlsurv_launch<3>(p, stream, fit); break;
    case 4: qtlsurv_launch<4>(p, stream, fit); break;
    case 5: qtlsurv_launch<5>(p, stream, fit); break;
    case 6: qtlsurv_launch<6>(p, stream, fit); break;
    case 7: qtlsurv_launch<7>(p, stream, fit); break;
    case 8: qtlsurv_launch<8>(p, stream, fit); break;
    default: qtlsurv_launch<9>(p, stream, fit); break;
    }
}
void launch_qtlsurv_null(const QtlsurvParams& p, hipStream_t stream) { qtlsurv_dispatch(p, stream, false); }
void launch_qtlsurv_fit(const QtlsurvParams& p, hipStream_t stream) { qtlsurv_dispatch(p, stream, true); }

} // namespace cnf2
