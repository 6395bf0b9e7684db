// cnf2_qtlvc_kernels.hip -- the kernels of the variance-component QTL scan (cnf2_qtl_scan_vc, include/cnf2hip.h): random
// founder-haplotype effects, one variance component per locus, on the descent rows of cnf2_sweep_descent and the column map
// col[n][8] with up to 64 columns.  The model, the Jacobi schedule, the rank rule and the search of a cell live in
// cnf2_qtlvc.h; this file forms the sums and runs the iteration a wave wide.
//
//   qtlvc_design_kernel   per marker, a wave: S22 = Z'Z (lane t its row) and S21 = Z'X0 over the individuals in ascending order,
//                         G = S21 S11^-1, W = S22 - G S21' into LDS, the cyclic Jacobi iteration on W and Qt in LDS, the sorted
//                         eigenvalues, the rank, the grid tables: the marker's record
//   qtlvc_scan_kernel     the hot path: the founder-haplotype scan's product (the eight cells of a descent row x the trait and
//                         permutation columns on the f64 matrix cores, pattern by pattern of the gather list, scattered into the
//                         wave's G[2][H][32] in LDS); epilogue per (marker, column): v, t = Q'v into the wave's second LDS
//                         block, the grid from the tables, the bisection, the cell; h, sigma2 and the BLUP of an observed
//                         column, the maximum of a permuted column over the tile
// c_i, n_c and the Cholesky factor of S11 are qtlhap_chrom_kernel's; the column image, b0 and RSS0, and the maxima over a
// chromosome's tiles are cnf2_qtl_kernels.hip's kernels on the same QtlParams.
//
// No kernel adds with atomics; every sum runs in a fixed order and every loop has a fixed bound (QTLVC_SWEEPS sweeps,
// QTLVC_REFINE bisections): a call gives the same bits every time, whatever the column tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlvc.h"

namespace cnf2 {

typedef double vd4 __attribute__((ext_vector_type(4)));

constexpr int QTLVC_NT    = 2;      // column tiles of 16 per wave
constexpr int QTLVC_WAVES = 2;      // waves per block: the same two markers, consecutive column groups
constexpr int QTLVC_KU    = 4;      // k-steps of 4 slots requested together
constexpr int QTLVC_COLS  = 16 * QTLVC_NT;

__device__ __forceinline__ double qtlvc_x0(const QtlParams& q, int i, int k) { return k == 0 ? 1.0 : q.cov[(size_t)i * q.K + (k - 1)]; }

// (LDS traffic of one wave among its own lanes: the compiler must not move it, the hardware keeps its order)
__device__ __forceinline__ void qtlvc_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

void launch_qtlvc_chrom(const QtlVcParams& p, hipStream_t stream)
{
    QtlHapParams hp = {};
    hp.q = p.q, hp.descent = p.descent;
    launch_qtlhap_chrom(hp, stream);
}

// One wave per marker.  Lane t < H owns row t of S22 and of S21 in registers.  Per used individual, in ascending order: lanes
// 0 .. H-1 form Z[i][.] into LDS, then every lane adds its row's products.  Then G = S21 S11^-1 (lane t its row) and the lower
// triangle of W = S22 - G S21' into LDS, mirrored.  The Jacobi iteration (cnf2_qtlvc.h): per round lane k < Hp / 2 decides
// its pair's rotation; lane t then rotates its row of W through the columns of every rotated pair and column t of Qt
// (W has an odd leading dimension: the 64 rows of a column lie in 64 banks), then its column of W through the rows; then the
// pair's lane writes the closed form of the 2 x 2 block.
__global__ __launch_bounds__(64) void qtlvc_design_kernel(QtlVcParams p)
{
    extern __shared__ __attribute__((aligned(16))) double qtlvc_lds[];
    __shared__ double z[QTLVC_MAXH], Gs[QTLVC_MAXH * QTL_NX], Ss[QTLVC_MAXH * QTL_NX], dr[QTLVC_MAXH], ds[QTLVC_MAXH];
    __shared__ double rc[QTLVC_MAXH / 2], rs[QTLVC_MAXH / 2];
    __shared__ int    rp[QTLVC_MAXH / 2], rq[QTLVC_MAXH / 2], ron[QTLVC_MAXH / 2], inv[QTLVC_MAXH];
    const QtlParams& q = p.q;
    const int        m = blockIdx.x, t = threadIdx.x, H = p.H, nx = q.nx, ld = qtlvc_ld(H);
    const int        c = q.mchrom[m];
    const uint8_t*   cm = q.cmask + (size_t)c * q.n;
    double*          W  = qtlvc_lds;                   // [H][ld]
    double*          Qt = qtlvc_lds + (size_t)H * ld;  // [H][H]
    double           acc[QTLVC_MAXH], s21[QTL_NX];
#pragma unroll
    for (int k = 0; k < QTLVC_MAXH; k++) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) s21[k] = 0.0;
    z[t] = 0.0;
    __syncthreads();
    for (int i = 0; i < q.n; i++) {
        if (!cm[i]) continue;                     // (uniform over the wave)
        double zi = 0.0;
        if (t < H) {
            zi   = qtlhap_z(p.descent + ((size_t)i * q.M + m) * 8, p.col + (size_t)i * 8, t);
            z[t] = zi;
        }
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < QTLVC_MAXH; k0 += 8)
            if (k0 < H) {
#pragma unroll
                for (int k = k0; k < k0 + 8; k++) acc[k] += zi * z[k];      // (z is 0 past H)
            }
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < nx) s21[k] += zi * qtlvc_x0(q, i, k);
        __syncthreads();
    }
    const double* L      = q.chol + (size_t)c * QTL_CHOL;
    const bool    usable = L[QTL_NX * QTL_NX] != 0.0;
    double*       rec    = p.rec + (size_t)m * qtlvc_rec_size(H, nx);
    if (!usable) {                                // (uniform)
        if (t == 0) p.rank[m] = 0;
        if (t < H) {
            rec[t] = 0.0;
            if (p.eval) p.eval[(size_t)m * H + t] = 0.0;
        }
        return;
    }
    if (t < H) {
        double g[QTL_NX];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) g[k] = k < nx ? s21[k] : 0.0;
        qtl_chol_solve(L, nx, g);
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < nx) {
                Gs[t * QTL_NX + k] = g[k];
                Ss[t * QTL_NX + k] = s21[k];
                rec[qtlvc_o_g(H) + t * nx + k] = g[k];
            }
    }
    __syncthreads();
    if (t < H) {
#pragma unroll
        for (int k = 0; k < QTLVC_MAXH; k++)
            if (k <= t) {
                double s = 0.0;
                for (int kk = 0; kk < nx; kk++) s += Gs[t * QTL_NX + kk] * Ss[k * QTL_NX + kk];
                const double w = acc[k] - s;
                W[t * ld + k] = w;
                W[k * ld + t] = w;
            }
        for (int k = 0; k < H; k++) Qt[k * H + t] = k == t ? 1.0 : 0.0;
    }
    __syncthreads();

    const int Hp = H + (H & 1), np = Hp / 2;
    bool      converged = false;
#pragma unroll 1
    for (int sweep = 0; sweep < QTLVC_SWEEPS; sweep++) {
        bool any = false;
#pragma unroll 1
        for (int r = 0; r < Hp - 1; r++) {
            bool   on = false;
            int    pp = 0, qq = 0;
            double napp = 0.0, naqq = 0.0;
            if (t < np) {
                qtlvc_pair(Hp, r, t, &pp, &qq);
                double cc = 1.0, ss = 0.0, tt = 0.0;
                if (qq < H) {
                    const double app = W[pp * ld + pp], aqq = W[qq * ld + qq], apq = W[pp * ld + qq];
                    on   = qtlvc_rotation(app, aqq, apq, &cc, &ss, &tt);
                    napp = app - tt * apq;
                    naqq = aqq + tt * apq;
                }
                rp[t] = pp, rq[t] = qq, rc[t] = cc, rs[t] = ss, ron[t] = on ? 1 : 0;
                any = any || on;
            }
            __syncthreads();
            if (t < H)
#pragma unroll 1
                for (int k = 0; k < np; k++) {
                    if (!ron[k]) continue;
                    const int    a = rp[k], b = rq[k];
                    const double cc = rc[k], ss = rs[k];
                    const double x = W[t * ld + a], y = W[t * ld + b];
                    W[t * ld + a] = cc * x - ss * y;
                    W[t * ld + b] = ss * x + cc * y;
                    const double e = Qt[a * H + t], f = Qt[b * H + t];
                    Qt[a * H + t] = cc * e - ss * f;
                    Qt[b * H + t] = ss * e + cc * f;
                }
            __syncthreads();
            if (t < H)
#pragma unroll 1
                for (int k = 0; k < np; k++) {
                    if (!ron[k]) continue;
                    const int    a = rp[k], b = rq[k];
                    const double cc = rc[k], ss = rs[k];
                    const double x = W[a * ld + t], y = W[b * ld + t];
                    W[a * ld + t] = cc * x - ss * y;
                    W[b * ld + t] = ss * x + cc * y;
                }
            __syncthreads();
            if (on) {
                W[pp * ld + pp] = napp;
                W[qq * ld + qq] = naqq;
                W[pp * ld + qq] = 0.0;
                W[qq * ld + pp] = 0.0;
            }
            __syncthreads();
        }
        if (__ballot(any) == 0) {                 // (uniform)
            converged = true;
            break;
        }
    }
    if (!converged) {
        if (t == 0) p.rank[m] = -1;
        if (t < H) {
            rec[t] = 0.0;
            if (p.eval) p.eval[(size_t)m * H + t] = 0.0;
        }
        return;
    }
    if (t < H) dr[t] = W[t * ld + t] > 0.0 ? W[t * ld + t] : 0.0;
    __syncthreads();
    if (t < H) {
        const int pos = qtlvc_position(dr, H, t);
        ds[pos]  = dr[t];
        inv[pos] = t;
    }
    __syncthreads();
    const int rank = __popcll(__ballot(t < H && ds[t] > QTLVC_RANK * ds[0]));
    const int nu   = q.nc[c] - 1 - q.K;
    if (t == 0) p.rank[m] = rank;
    if (t < H) {
        rec[t] = ds[t];
        if (p.eval) p.eval[(size_t)m * H + t] = ds[t];
    }
    for (int e = t; e < H * H; e += 64) rec[qtlvc_o_qt(H) + e] = Qt[inv[e / H] * H + e % H];
    if (rank > 0 && nu >= 2 && t < QTLVC_GRID)
        rec[qtlvc_o_e(H, nx) + t] = qtlvc_grid_tables(ds, H, rank, nu, t, rec + qtlvc_o_gtab(H, nx) + (size_t)t * H);
}
bool launch_qtlvc_design(const QtlVcParams& p, hipStream_t stream)
{
    const size_t lds = ((size_t)p.H * qtlvc_ld(p.H) + (size_t)p.H * p.H) * sizeof(double);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(qtlvc_design_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return false;
    hipLaunchKernelGGL(qtlvc_design_kernel, dim3(p.q.M), dim3(64), lds, stream, p);
    return true;
}

// The product is qtlhap_scan_kernel's (see there for the operands, the clamped addresses and the scatter at a pattern's end);
// a wave's two blocks of LDS, G[2][H][32] and T[2][H][32], are sized by H.  Epilogue, a lane per (marker, column):
// v = G - G_m b0 in place, t_k = sum_h Qt[k][h] v_h for k below the rank into T, the cell (cnf2_qtlvc.h); for an observed column
// h, sigma2 and the BLUP sum_k Qt[k][h] (g / (1 + g d_k)) t_k; for a permuted one the maximum over the tile's markers.
__global__ __launch_bounds__(64 * QTLVC_WAVES) void qtlvc_scan_kernel(QtlVcParams p)
{
    extern __shared__ __attribute__((aligned(16))) double qtlvc_lds[];
    const QtlParams& q = p.q;
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int cb = (blockIdx.y * QTLVC_WAVES + wib) * QTLVC_COLS;
    if (cb >= q.rn) return;                                    // (no block-wide barrier below: a wave's LDS is its own)
    const int  S = p.S, H = p.H, nx = q.nx, nsteps = S / 4;
    const int  blk = 2 * H * QTLVC_COLS;                       // doubles of G, and of T
    double*    G   = qtlvc_lds + (size_t)wib * 2 * blk;        // [2][H][QTLVC_COLS]
    double*    Tb  = G + blk;
    const int  oi = lane & 15, ok4 = lane >> 4;
    const int  cell = oi & 7, mp = oi >> 3;
    const bool mval = mp < len;
    const size_t   M    = (size_t)q.M;
    const double*  drow = p.descent + (size_t)m0 * 8 + (mval ? oi : cell);
    const size_t   ds   = M * 8;
    const uint8_t* cm   = q.cmask + (size_t)c * q.n;
    int  col[QTLVC_NT];
    bool cval[QTLVC_NT];
#pragma unroll
    for (int nt = 0; nt < QTLVC_NT; nt++) {
        const int cc = cb + nt * 16 + oi;
        cval[nt] = cc < q.rn;
        col[nt]  = cval[nt] ? cc : 0;
    }
    for (int e = lane; e < 2 * blk; e += 64) G[e] = 0.0;
    qtlvc_wave_fence();
    vd4 acc[QTLVC_NT];
#pragma unroll
    for (int nt = 0; nt < QTLVC_NT; nt++) acc[nt] = vd4{0.0, 0.0, 0.0, 0.0};

#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += 4 * QTLVC_KU) {
        double x[QTLVC_KU], y[QTLVC_KU][QTLVC_NT];
        bool   on[QTLVC_KU];
#pragma unroll
        for (int u = 0; u < QTLVC_KU; u++) {
            const int  s   = s0 + 4 * u + ok4;
            const bool in  = s < S;
            const int  ind = p.gidx[in ? s : S - 1];
            const int  i   = ind < 0 ? 0 : ind;
            on[u] = in && ind >= 0 && cm[i] != 0;
            x[u]  = drow[(size_t)i * ds];
#pragma unroll
            for (int nt = 0; nt < QTLVC_NT; nt++) y[u][nt] = q.Y[(size_t)i * q.rstride + col[nt]];
        }
#pragma unroll
        for (int u = 0; u < QTLVC_KU; u++) {
            const double xv = (on[u] && mval) ? x[u] : 0.0;
#pragma unroll
            for (int nt = 0; nt < QTLVC_NT; nt++) {
                const double yy = (on[u] && cval[nt]) ? y[u][nt] : 0.0;
                acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, xv, acc[nt], 0, 0, 0);
            }
            const int step = (s0 >> 2) + u;
            if (step < nsteps && p.stepend[step] != 0) {
                const int h = p.patcol[(size_t)p.steppat[step] * 8 + cell];
#pragma unroll 1
                for (int k = 0; k < 8; k++) {
                    if (cell == k && mval) {
#pragma unroll
                        for (int nt = 0; nt < QTLVC_NT; nt++)
#pragma unroll
                            for (int reg = 0; reg < 4; reg++) G[(mp * H + h) * QTLVC_COLS + nt * 16 + ok4 + 4 * reg] += acc[nt][reg];
                    }
                    qtlvc_wave_fence();
                }
#pragma unroll
                for (int nt = 0; nt < QTLVC_NT; nt++) acc[nt] = vd4{0.0, 0.0, 0.0, 0.0};
            }
        }
    }
    qtlvc_wave_fence();

    // a lane per (marker, column)
    const int  mk = lane >> 5, cc = lane & 31;
    const int  rr = cb + cc;
    const bool rval = rr < q.rn, mv = mk < len;
    const int  rc = rval ? rr : 0, m = m0 + (mv ? mk : 0);
    const double* rec  = p.rec + (size_t)m * qtlvc_rec_size(H, nx);
    const double* Qt   = rec + qtlvc_o_qt(H);
    const double* Gm   = rec + qtlvc_o_g(H);
    const int     rank = p.rank[m];
    const int     nu   = q.nc[c] - 1 - q.K;
    const bool    fit  = rank > 0 && nu >= 2;
    const double* nq   = q.nullq + (size_t)c * (nx + 1) * q.rstride;
    double        b0[QTL_NX];
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) b0[k] = k < nx ? nq[(size_t)k * q.rstride + rc] : 0.0;
    const double rss0 = nq[(size_t)nx * q.rstride + rc];
    double*      v    = G + (size_t)mk * H * QTLVC_COLS + cc;
    double*      tb   = Tb + (size_t)mk * H * QTLVC_COLS + cc;
    const int nk = fit ? rank : 0;
    for (int h = 0; h < (fit ? H : 0); h++) {        // (a marker that is not fitted has no G or Qt in its record)
        double s = v[h * QTLVC_COLS];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < nx) s -= Gm[h * nx + k] * b0[k];
        v[h * QTLVC_COLS] = s;
    }
    for (int k = 0; k < nk; k++) {
        const double* qk = Qt + (size_t)k * H;
        double        s  = 0.0;
#pragma unroll 4
        for (int h = 0; h < H; h++) s += qk[h] * v[h * QTLVC_COLS];
        tb[k * QTLVC_COLS] = s;
    }
    const QtlVcCell r = qtlvc_cell(rec, rec + qtlvc_o_e(H, nx), rec + qtlvc_o_gtab(H, nx), H, nk, tb, QTLVC_COLS, rss0, nu, fit);
    const int gr = q.r0 + rc;
    if (rval && mv && gr < q.T) {
        q.lod[(size_t)gr * M + m]    = r.lod;
        p.h[(size_t)gr * M + m]      = r.h;
        p.sigma2[(size_t)gr * M + m] = r.sigma2;
        if (p.blup) {
            const bool some = r.lod > 0.0;
            if (some)
                for (int k = 0; k < nk; k++) tb[k * QTLVC_COLS] *= r.g / (1.0 + r.g * rec[k]);
            double* bo = p.blup + ((size_t)gr * M + m) * H;
            for (int h = 0; h < H; h++) {
                double s = 0.0;
                if (some)
                    for (int k = 0; k < nk; k++) s += Qt[(size_t)k * H + h] * tb[k * QTLVC_COLS];
                bo[h] = s;
            }
        }
    }
    double best = (rval && mv) ? r.lod : 0.0;           // a LOD is never negative: 0 is the maximum's identity
    best = fmax(best, __shfl_xor(best, 32));
    if (mk == 0 && rval && gr >= q.T) q.tilemax[(size_t)tile * q.rstride + rr] = best;
}
bool launch_qtlvc_scan(const QtlVcParams& p, hipStream_t stream)
{
    const int    cols = QTLVC_COLS * QTLVC_WAVES;
    const size_t lds  = (size_t)QTLVC_WAVES * 2 * 2 * p.H * QTLVC_COLS * sizeof(double);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(qtlvc_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return false;
    hipLaunchKernelGGL(qtlvc_scan_kernel, dim3(p.q.n_tiles, (p.q.rn + cols - 1) / cols), dim3(64 * QTLVC_WAVES), lds, stream, p);
    return true;
}

} // namespace cnf2
