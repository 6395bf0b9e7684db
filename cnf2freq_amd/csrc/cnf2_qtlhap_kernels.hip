// cnf2_qtlhap_kernels.hip -- the kernels of the founder-haplotype QTL scan (cnf2_qtl_scan_hap, include/cnf2hip.h): the trait
// regressed on the expected dosage of up to 32 founder haplotypes, formed from the descent rows of cnf2_sweep_descent and the
// column map col[n][8].  The model and every decision about dropped columns, degenerate markers and chromosomes live in
// cnf2_qtlhap.h; this file forms the sums.
//
//   qtlhap_chrom_kernel   per chromosome: c_i, n_c, S11 = X0'X0 and its Cholesky factor (qtl_chrom_kernel on rows of eight)
//   qtlhap_design_kernel  per marker, a wave: S22 = Z'Z and S21 = Z'X0 over the individuals in ascending order, G = S21 S11^-1,
//                         W = S22 - G S21' and its packed factor with the drop rule in LDS, the kept mask, df
//   qtlhap_scan_kernel    the hot path: the eight cells of a descent row x the trait and permutation columns on the f64 matrix
//                         cores, pattern by pattern of the gather list; a pattern's block is added into G[H][columns] at the
//                         pattern's rows; epilogue per (marker, column): v, the forward substitution, the cell, the
//                         coefficients of an observed column, the maximum of a permuted column over the tile
// The column image, b0 and RSS0, and the maxima over a chromosome's tiles are cnf2_qtl_kernels.hip's kernels on the same
// QtlParams.
//
// No kernel adds with atomics; every sum runs in a fixed order (the individuals ascending in the design, the gather list's
// order in the product, a wave owning its tile): a call gives the same bits every time, whatever the column tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlhap.h"

namespace cnf2 {

typedef double hd4 __attribute__((ext_vector_type(4)));

constexpr int QTLHAP_CHROM_BLOCK = 128;    // >= QTL_NX * QTL_NX
constexpr int QTLHAP_NT          = 2;      // column tiles of 16 per wave
constexpr int QTLHAP_WAVES       = 2;      // waves per block: the same two markers, consecutive column groups
constexpr int QTLHAP_KU          = 4;      // k-steps of 4 slots requested together
constexpr int QTLHAP_COLS        = 16 * QTLHAP_NT;

__device__ __forceinline__ double qtlhap_x0(const QtlParams& q, int i, int k) { return k == 0 ? 1.0 : q.cov[(size_t)i * q.K + (k - 1)]; }

// (LDS traffic of one wave among its own lanes: the compiler must not move it, the hardware keeps its order)
__device__ __forceinline__ void qtlhap_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

__global__ __launch_bounds__(QTLHAP_CHROM_BLOCK) void qtlhap_chrom_kernel(QtlHapParams p)
{
    __shared__ int    cnt[QTLHAP_CHROM_BLOCK];
    __shared__ double S[QTL_NX * QTL_NX];
    const QtlParams& q = p.q;
    const int        c = blockIdx.x, tid = threadIdx.x;
    const int        first = q.cs[c];
    uint8_t*         cm = q.cmask + (size_t)c * q.n;
    int              mine = 0;
    for (int i = tid; i < q.n; i += QTLHAP_CHROM_BLOCK) {
        const double* d  = p.descent + ((size_t)i * q.M + first) * 8;
        bool          any = false;
#pragma unroll
        for (int k = 0; k < 8; k++) any = any || d[k] != 0.0;
        const bool on = q.use[i] && any;
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
            if (cm[i]) s += qtlhap_x0(q, i, j) * qtlhap_x0(q, i, k);
        S[j * QTL_NX + k] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int n_c = 0;
        for (int t = 0; t < QTLHAP_CHROM_BLOCK; t++) n_c += cnt[t];
        q.nc[c] = n_c;
        const bool ok = qtl_cholesky(S, q.nx);
        double*    out = q.chol + (size_t)c * QTL_CHOL;
        for (int t = 0; t < QTL_NX * QTL_NX; t++) out[t] = S[t];
        out[QTL_NX * QTL_NX] = (ok && n_c >= q.K + 4) ? 1.0 : 0.0;
    }
}
void launch_qtlhap_chrom(const QtlHapParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlhap_chrom_kernel, dim3(p.q.C), dim3(QTLHAP_CHROM_BLOCK), 0, stream, p);
}

// One wave per marker.  Lane t owns the entries t, t + 64, .. of the packed triangle of S22 (at most nine) in registers and,
// for t < H, row t of S21.  Per used individual, in ascending order: lanes 0 .. H-1 form Z[i][.] into LDS, then every lane adds
// its products.  Then G = S21 S11^-1 (lane h its row), W = S22 - G S21' in LDS, and lane 0 factors it by cnf2_qtlhap.h's rule.
__global__ __launch_bounds__(64) void qtlhap_design_kernel(QtlHapParams p)
{
    __shared__ double W[QTLHAP_TRI], z[QTLHAP_MAXH], diag[QTLHAP_MAXH], Gs[QTLHAP_MAXH * QTL_NX], Ss[QTLHAP_MAXH * QTL_NX];
    __shared__ uint32_t kept_s;
    const QtlParams& q = p.q;
    const int        m = blockIdx.x, t = threadIdx.x, H = p.H, nx = q.nx;
    const int        c = q.mchrom[m];
    const uint8_t*   cm = q.cmask + (size_t)c * q.n;
    const int        ntri = H * (H + 1) / 2;
    constexpr int    NE = (QTLHAP_TRI + 63) / 64;
    int              ej[NE], ek[NE];
    double           acc[NE], s21[QTL_NX];
#pragma unroll
    for (int e = 0; e < NE; e++) {
        const int idx = t + 64 * e;
        int       j = 0;
        while ((j + 1) * (j + 2) / 2 <= idx) j++;
        ej[e]  = j;
        ek[e]  = idx - j * (j + 1) / 2;
        acc[e] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) s21[k] = 0.0;
    for (int i = 0; i < q.n; i++) {
        if (!cm[i]) continue;                     // (uniform over the wave)
        double zi = 0.0;
        if (t < H) {
            zi   = qtlhap_z(p.descent + ((size_t)i * q.M + m) * 8, p.col + (size_t)i * 8, t);
            z[t] = zi;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NE; e++)
            if (t + 64 * e < ntri) acc[e] += z[ej[e]] * z[ek[e]];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < nx) s21[k] += zi * qtlhap_x0(q, i, k);
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < NE; e++)
        if (t + 64 * e < ntri) W[t + 64 * e] = acc[e];
    __syncthreads();
    const double* L      = q.chol + (size_t)c * QTL_CHOL;
    const bool    usable = L[QTL_NX * QTL_NX] != 0.0;
    double*       rec    = p.rec + (size_t)m * qtlhap_rec_size(H, nx);
    if (t < H) {
        diag[t] = W[qtlhap_tri(t, t)];
        double g[QTL_NX];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) g[k] = (usable && k < nx) ? s21[k] : 0.0;
        if (usable) qtl_chol_solve(L, nx, g);
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < nx) {
                Gs[t * QTL_NX + k] = g[k];
                Ss[t * QTL_NX + k] = s21[k];
                rec[ntri + t * nx + k] = g[k];
            }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NE; e++)
        if (t + 64 * e < ntri) {
            double s = 0.0;
            for (int k = 0; k < nx; k++) s += Gs[ej[e] * QTL_NX + k] * Ss[ek[e] * QTL_NX + k];
            W[t + 64 * e] -= s;
        }
    __syncthreads();
    if (t == 0) {
        uint32_t kept = usable ? qtlhap_factor(W, H, diag) : 0u;
        if (!(usable && q.nc[c] - 1 - q.K - qtlhap_count(kept) >= 1)) kept = 0;
        kept_s    = kept;
        p.kept[m] = kept;
        p.df[m]   = qtlhap_count(kept);
    }
    __syncthreads();
    for (int e = t; e < ntri; e += 64) rec[e] = W[e];
}
void launch_qtlhap_design(const QtlHapParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlhap_design_kernel, dim3(p.q.M), dim3(64), 0, stream, p);
}

// The product, segmented by pattern.  A wave owns two markers of one chromosome (a tile never straddles a chromosome start) x
// 16 QTLHAP_NT columns.  It walks the slots of the gather list in order, four per v_mfma_f64_16x16x4_f64: the columns are the
// rows of the result, and its sixteen columns are the eight cells of the descent row at the two markers -- sixteen consecutive
// doubles of an individual as they lie in memory, with no compare: lane (cell, marker; k) reads the individual of slot s0 + k
// from the list, then its double.  The column operand is sixteen consecutive doubles of the image's row of that individual.
// Slots past the list, empty slots, an individual not used on the chromosome, a second marker past the chromosome's end and
// columns past the tile's are clamped addresses and zero operands: no load leaves its array.
// A step never straddles two patterns (they are padded to four slots), and the list says which steps end one.  There the
// accumulators -- the pattern's 8 x columns block per marker -- are added into the wave's G[marker][H][columns] in LDS at the
// rows the pattern's columns name, one cell at a time (two cells of a pattern may share a row), and cleared.  The branch is
// uniform over the wave; the wave owns its G, so there are no atomics and the order is the list's.
// Epilogue, a lane per (marker, column): v = G - G_m b0 in place, the forward substitution through the marker's packed
// factor, the cell (cnf2_qtlhap.h); for an observed column the back substitution and the coefficients; for a permuted one the
// maximum over the tile's markers, one value per (tile, column).
__global__ __launch_bounds__(64 * QTLHAP_WAVES) void qtlhap_scan_kernel(QtlHapParams p)
{
    __shared__ double Gall[QTLHAP_WAVES][2][QTLHAP_MAXH][QTLHAP_COLS];
    const QtlParams& q = p.q;
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int cb = (blockIdx.y * QTLHAP_WAVES + wib) * QTLHAP_COLS;
    if (cb >= q.rn) return;                                    // (no block-wide barrier below: a wave's G is its own)
    double (*G)[QTLHAP_MAXH][QTLHAP_COLS] = Gall[wib];
    const int  oi = lane & 15, ok = lane >> 4;
    const int  cell = oi & 7, mp = oi >> 3;
    const bool mval = mp < len;
    const int  S = p.S, H = p.H, nx = q.nx, nsteps = S / 4;
    const size_t   M    = (size_t)q.M;
    const double*  drow = p.descent + (size_t)m0 * 8 + (mval ? oi : cell);
    const size_t   ds   = M * 8;
    const uint8_t* cm   = q.cmask + (size_t)c * q.n;
    int  col[QTLHAP_NT];
    bool cval[QTLHAP_NT];
#pragma unroll
    for (int nt = 0; nt < QTLHAP_NT; nt++) {
        const int cc = cb + nt * 16 + oi;
        cval[nt] = cc < q.rn;
        col[nt]  = cval[nt] ? cc : 0;
    }
    for (int e = lane; e < 2 * QTLHAP_MAXH * QTLHAP_COLS; e += 64) (&G[0][0][0])[e] = 0.0;
    qtlhap_wave_fence();
    hd4 acc[QTLHAP_NT];
#pragma unroll
    for (int nt = 0; nt < QTLHAP_NT; nt++) acc[nt] = hd4{0.0, 0.0, 0.0, 0.0};

#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += 4 * QTLHAP_KU) {
        double x[QTLHAP_KU], y[QTLHAP_KU][QTLHAP_NT];
        bool   on[QTLHAP_KU];
#pragma unroll
        for (int u = 0; u < QTLHAP_KU; u++) {
            const int  s   = s0 + 4 * u + ok;
            const bool in  = s < S;
            const int  ind = p.gidx[in ? s : S - 1];
            const int  i   = ind < 0 ? 0 : ind;
            on[u] = in && ind >= 0 && cm[i] != 0;
            x[u]  = drow[(size_t)i * ds];
#pragma unroll
            for (int nt = 0; nt < QTLHAP_NT; nt++) y[u][nt] = q.Y[(size_t)i * q.rstride + col[nt]];
        }
#pragma unroll
        for (int u = 0; u < QTLHAP_KU; u++) {
            const double xv = (on[u] && mval) ? x[u] : 0.0;
#pragma unroll
            for (int nt = 0; nt < QTLHAP_NT; nt++) {
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
                        for (int nt = 0; nt < QTLHAP_NT; nt++)
#pragma unroll
                            for (int reg = 0; reg < 4; reg++) G[mp][h][nt * 16 + ok + 4 * reg] += acc[nt][reg];
                    }
                    qtlhap_wave_fence();
                }
#pragma unroll
                for (int nt = 0; nt < QTLHAP_NT; nt++) acc[nt] = hd4{0.0, 0.0, 0.0, 0.0};
            }
        }
    }
    qtlhap_wave_fence();

    // a lane per (marker, column)
    const int  mk = lane >> 5, cc = lane & 31;
    const int  rr = cb + cc;
    const bool rval = rr < q.rn, mv = mk < len;
    const int  rc = rval ? rr : 0, m = m0 + (mv ? mk : 0);
    const double*  rec   = p.rec + (size_t)m * qtlhap_rec_size(H, nx);
    const double*  Gm    = rec + H * (H + 1) / 2;
    const uint32_t kept  = p.kept[m];
    const int      n_c   = q.nc[c];
    const double*  nq    = q.nullq + (size_t)c * (nx + 1) * q.rstride;
    double         b0[QTL_NX];
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) b0[k] = k < nx ? nq[(size_t)k * q.rstride + rc] : 0.0;
    const double rss0 = nq[(size_t)nx * q.rstride + rc];
    double*      v    = &G[mk][0][cc];
    for (int h = 0; h < H; h++) {
        double s = v[h * QTLHAP_COLS];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < nx) s -= Gm[h * nx + k] * b0[k];
        v[h * QTLHAP_COLS] = s;
    }
    const double d   = qtlhap_forward(rec, H, kept, v, QTLHAP_COLS);
    const double lod = qtlhap_cell(d, rss0, n_c, kept != 0);
    const int    gr  = q.r0 + rc;
    if (rval && mv && gr < q.T) {
        q.lod[(size_t)gr * M + m] = lod;
        if (p.coef) {
            qtlhap_backward(rec, H, kept, v, QTLHAP_COLS);
            double* co = p.coef + ((size_t)gr * M + m) * H;
            for (int h = 0; h < H; h++) co[h] = ((kept >> h) & 1) ? v[h * QTLHAP_COLS] : (double)NAN;
        }
    }
    double best = (rval && mv) ? lod : 0.0;             // a LOD is never negative: 0 is the maximum's identity
    best = fmax(best, __shfl_xor(best, 32));
    if (mk == 0 && rval && gr >= q.T) q.tilemax[(size_t)tile * q.rstride + rr] = best;
}
void launch_qtlhap_scan(const QtlHapParams& p, hipStream_t stream)
{
    const int cols = QTLHAP_COLS * QTLHAP_WAVES;
    hipLaunchKernelGGL(qtlhap_scan_kernel, dim3(p.q.n_tiles, (p.q.rn + cols - 1) / cols), dim3(64 * QTLHAP_WAVES), 0, stream, p);
}

} // namespace cnf2
