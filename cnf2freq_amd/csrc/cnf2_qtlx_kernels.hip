// cnf2_qtlx_kernels.hip -- the kernels of the extended single-locus scan (cnf2_qtl_scanx, include/cnf2hip.h): per marker the
// nested Haley-Knott models Mendelian (a, d), imprinting (+ i) and interaction (+ a z, d z, i z) of phenotype columns, observed
// and permuted, on the origin rows.  The model and every decision about degenerate cells live in cnf2_qtlx.h; this file
// forms the sums.
//
//   (qtl2_mask_kernel of cnf2_qtl2_kernels.hip makes the masks, qtl_gather_kernel of cnf2_qtl_kernels.hip the column image)
//   qtlx_null_kernel    per chromosome and column: n_c, sum c y^2, RSS0 of the null design
//   qtlx_marker_kernel  the hot path: per marker the Gram matrix X'X and X'Y on the f64 matrix cores, factored once per marker
//   qtlx_finish_kernel  per chromosome and permuted column: the five maxima over the chromosome's marker tiles
//
// No kernel adds with atomics, the individuals are never split between waves and every sum runs over them in ascending
// order: a call gives the same bits every time, whatever the column tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlx.h"

namespace cnf2 {

typedef double qxd2 __attribute__((ext_vector_type(2)));
typedef double qxd4 __attribute__((ext_vector_type(4)));

constexpr int QTLX_LD    = QTL2_W + 1;   // doubles per LDS row: the 32 lanes a ds_read_b64 serves cover the 64 banks
constexpr int QTLX_NT    = 4;            // column tiles of 16 per wave: a block takes 64 columns
constexpr int QTLX_WAVES = 4;            // waves per block: the same columns, adjacent markers of the tile
constexpr int QTLX_KU    = 4;            // k-steps of 4 individuals requested together

// what a wave wrote to LDS is there for its other lanes
__device__ __forceinline__ void qtlx_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// covariate k of individual i as column k of X0 (column 0 is the intercept)
__device__ __forceinline__ double qtlx_x(const QtlxParams& q, int i, int k) { return k == 0 ? 1.0 : q.cov[(size_t)i * q.K + (k - 1)]; }

// One block per chromosome and 64 columns: n_c, S11 = X0'X0 (one thread per entry) and its factor, then one thread per
// column b0 = X0'y and sum c y^2 over the individuals in ascending order, and the cell of the null design alone
// (cnf2_qtlx.h).  yy is kept for the marker kernel.
__global__ __launch_bounds__(64) void qtlx_null_kernel(QtlxParams q)
{
    __shared__ double G[QTL2_W * QTLX_LD];
    __shared__ double B[64 * QTLX_LD];
    __shared__ int    cnt[64];
    __shared__ int    fshare[2];
    constexpr int NX = 8;                // columns of X0 per row of threads: 64 threads cover an 8 x 8 block of S11 at a time
    const int      tid = threadIdx.x, c = blockIdx.y;
    const uint8_t* cm = q.cmask + (size_t)c * q.n;
    const int      nx = q.K + 1;
    for (int t = tid; t < QTL2_W * QTLX_LD; t += 64) G[t] = 0.0;
    for (int t = tid; t < 64 * QTLX_LD; t += 64) B[t] = 0.0;
    int mine = 0;
    for (int i = tid; i < q.n; i += 64) mine += cm[i] ? 1 : 0;
    cnt[tid] = mine;
    __syncthreads();
    for (int jb = 0; jb < nx; jb += NX)
        for (int kb = 0; kb <= jb; kb += NX) {
            const int jx = jb + tid / NX, kx = kb + tid % NX;
            if (jx < nx && kx <= jx) {
                double s = 0.0;
                for (int i = 0; i < q.n; i++)
                    if (cm[i]) s += qtlx_x(q, i, jx) * qtlx_x(q, i, kx);
                G[jx * QTLX_LD + kx] = s;
            }
        }
    const int  rr = blockIdx.x * 64 + tid;
    const bool valid = rr < q.rn;
    const int  rc = valid ? rr : 0;
    double     yy = 0.0;
    double*    b = B + tid * QTLX_LD;
    for (int i = 0; i < q.n; i++) {
        if (!cm[i]) continue;
        const double y = q.Y[(size_t)i * q.rstride + rc];
        for (int k = 0; k < nx; k++) b[k] += qtlx_x(q, i, k) * y;
        yy += y * y;
    }
    __syncthreads();
    const QtlxDesign ds = qtlx_design(q.K, q.Ki, q.additive != 0, q.imprint != 0);
    if (tid == 0) {
        int n_c = 0;
        for (int t = 0; t < 64; t++) n_c += cnt[t];
        const QtlxFactor f0 = qtlx_factor(G, QTLX_LD, ds, n_c, ds.nx);
        fshare[0] = n_c;
        fshare[1] = f0.usable;
    }
    __syncthreads();
    const int n_c = fshare[0];
    double    rss0 = 0.0;
    if (fshare[1]) {
        double s0 = 0.0;
        for (int j = 0; j < nx; j++) {
            double s = b[j];
            for (int k = 0; k < j; k++) s -= G[j * QTLX_LD + k] * b[k];
            b[j] = s / G[j * QTLX_LD + j];
            s0 += b[j] * b[j];
        }
        rss0 = yy - s0;
    }
    if (tid == 0 && blockIdx.x == 0 && q.r0 == 0) q.nc[c] = n_c;
    if (!valid) return;
    q.yy[(size_t)c * q.rstride + rr] = yy;
    const int gr = q.r0 + rr;
    if (gr < q.T) q.rss0[(size_t)gr * q.C + c] = rss0;
}
void launch_qtlx_null(const QtlxParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlx_null_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

// The marker kernel: a batched small SYRK.  A block takes one marker tile -- at most QTLX_TILE consecutive markers of one
// chromosome; no tile straddles a chromosome start -- and 64 columns; its four waves take the tile's markers in turn, so that
// the waves running together read adjacent 32-byte rows of an individual: one 128-byte line.  Per marker a wave walks every
// individual in ascending order, four per v_mfma_f64_16x16x4_f64 (operand and result layouts: place_rows_kernel in
// cnf2_kernels.hip).  Lane (design column oi, individual ok) forms its own design entry in registers from the individual's
// 32-byte origin row and one covariate, by the two codes of qtlx_column: (1, a, d or i) x (1 or z_k); rows past the design's
// width are zero.  In this instruction's layout the A operand X' and the B operand X are the same register value, so the
// Gram matrix is acc = mfma(x, x, acc); X'Y is one more instruction per 16 columns against 16 doubles of an image row, with
// the columns as the rows of the result.  Individuals past n and columns past the tile's are clamped addresses, zero operands
// and masked outputs: nothing is padded in HBM and no load leaves its array.
// Epilogue: the Gram tile and X'Y go through the wave's LDS; lane 0 factors the tile once with the rank rule, then one lane
// per column does the forward substitution, for an observed column the back-substitution, and the cell (cnf2_qtlx.h).  The
// observed columns are stored; the permuted ones go into five running maxima per lane, reduced over the block's waves in a
// fixed order: one value per (tile, statistic, column).
__global__ __launch_bounds__(64 * QTLX_WAVES, 2) void qtlx_marker_kernel(QtlxParams q)
{
    __shared__ double lds[QTLX_WAVES][(QTL2_W + 16 * QTLX_NT) * QTLX_LD];
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x, cb = blockIdx.y * 16 * QTLX_NT;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int oi = lane & 15, ok = lane >> 4;
    const int n = q.n;
    const size_t   os = (size_t)q.M * 4;
    const uint8_t* cm = q.cmask + (size_t)c * n;
    const int      n_c = q.nc[c];
    const QtlxDesign ds = qtlx_design(q.K, q.Ki, q.additive != 0, q.imprint != 0);
    const int        ncoef = ds.w - ds.nx;
    int se, sz;
    qtlx_column(ds, oi, &se, &sz);
    // (a column of X0 reads the centred covariate, an interaction column the raw one: cnf2_qtlx.h)
    const double* covp = (se == QTLX_ONE ? q.cov : q.cov_raw) + (sz > 0 ? sz - 1 : 0);
    double* G = lds[wib];
    double* B = G + QTL2_W * QTLX_LD;
    int  col[QTLX_NT];
    bool cval[QTLX_NT];
#pragma unroll
    for (int nt = 0; nt < QTLX_NT; nt++) {
        const int cc = cb + nt * 16 + oi;
        cval[nt] = cc < q.rn;
        col[nt]  = cval[nt] ? cc : 0;
    }
    const bool mycol = cb + lane < q.rn;
    const int  myc   = mycol ? cb + lane : 0;
    const int  gr    = q.r0 + myc;
    const double yy  = q.yy[(size_t)c * q.rstride + myc];
    double     mx0 = 0.0, mx1 = 0.0, mx2 = 0.0, mx3 = 0.0, mx4 = 0.0;       // (no LOD or difference of nested LODs is negative: 0 is the maximum's identity)

#pragma unroll 1
    for (int s = wib; s < len; s += QTLX_WAVES) {
        const int m = m0 + s;
        qxd4 accG = qxd4{0.0, 0.0, 0.0, 0.0}, accY[QTLX_NT];
#pragma unroll
        for (int nt = 0; nt < QTLX_NT; nt++) accY[nt] = qxd4{0.0, 0.0, 0.0, 0.0};

        if (n_c >= ds.w + 1) {
#pragma unroll 1
            for (int i0 = 0; i0 < n; i0 += 4 * QTLX_KU) {
                qxd2   p01[QTLX_KU], p23[QTLX_KU];
                double z[QTLX_KU], y[QTLX_KU][QTLX_NT];
                bool   in[QTLX_KU], on[QTLX_KU];
#pragma unroll
                for (int u = 0; u < QTLX_KU; u++) {
                    const int i  = i0 + 4 * u + ok;
                    in[u]        = i < n;
                    const int ic = in[u] ? i : n - 1;
                    const double* p = q.origin + (size_t)ic * os + (size_t)m * 4;
                    p01[u] = *(const qxd2*)p;
                    p23[u] = *(const qxd2*)(p + 2);
                    on[u]  = in[u] && cm[ic] != 0;
                    z[u]   = sz > 0 ? covp[(size_t)ic * q.K] : 1.0;
#pragma unroll
                    for (int nt = 0; nt < QTLX_NT; nt++) y[u][nt] = q.Y[(size_t)ic * q.rstride + col[nt]];
                }
#pragma unroll
                for (int u = 0; u < QTLX_KU; u++) {
                    const double a = p23[u].y - p01[u].x, d = p01[u].y + p23[u].x, im = p01[u].y - p23[u].x;
                    const double ee = se == QTLX_ONE ? 1.0 : (se == QTLX_A ? a : (se == QTLX_D ? d : im));
                    const double x  = (on[u] && se != QTLX_NONE) ? ee * z[u] : 0.0;
                    accG = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, accG, 0, 0, 0);
#pragma unroll
                    for (int nt = 0; nt < QTLX_NT; nt++) {
                        const double yv = (in[u] && cval[nt]) ? y[u][nt] : 0.0;
                        accY[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yv, x, accY[nt], 0, 0, 0);
                    }
                }
            }
        }

        // G[row][column] and B[column of Y][design column]
#pragma unroll
        for (int reg = 0; reg < 4; reg++) G[(ok + 4 * reg) * QTLX_LD + oi] = accG[reg];
#pragma unroll
        for (int nt = 0; nt < QTLX_NT; nt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) B[(nt * 16 + ok + 4 * reg) * QTLX_LD + oi] = accY[nt][reg];
        qtlx_wave_sync();
        QtlxFactor f;
        f.usable = 0, f.rank[0] = f.rank[1] = f.rank[2] = 0;
        if (lane == 0) f = qtlx_factor(G, QTLX_LD, ds, n_c, ds.w);
        f.usable  = __builtin_amdgcn_readfirstlane(f.usable);
        f.rank[0] = __builtin_amdgcn_readfirstlane(f.rank[0]);
        f.rank[1] = __builtin_amdgcn_readfirstlane(f.rank[1]);
        f.rank[2] = __builtin_amdgcn_readfirstlane(f.rank[2]);
        qtlx_wave_sync();
        const bool observed = mycol && gr < q.T;
        double*    brow = B + lane * QTLX_LD;
        const QtlxCell cell = qtlx_cell(G, QTLX_LD, ds, f, brow, 1, yy, n_c, observed);
        if (observed) {
            const size_t o = (size_t)gr * q.M + m;
            q.lod[3 * o]     = cell.lod[0];
            q.lod[3 * o + 1] = cell.lod[1];
            q.lod[3 * o + 2] = cell.lod[2];
            double* co = q.coef + o * ncoef;
#pragma unroll 1
            for (int j = 0; j < ncoef; j++) co[j] = brow[ds.nx + j];
        }
        if (mycol && gr >= q.T) {
            mx0 = fmax(mx0, cell.lod[0]);
            mx1 = fmax(mx1, cell.lod[1]);
            mx2 = fmax(mx2, cell.lod[2]);
            mx3 = fmax(mx3, cell.lod[1] - cell.lod[0]);
            mx4 = fmax(mx4, cell.lod[2] - cell.lod[1]);
        }
        if (lane == 0 && q.r0 == 0 && cb == 0) {
            q.rank[3 * m]     = f.rank[0];
            q.rank[3 * m + 1] = f.rank[1];
            q.rank[3 * m + 2] = f.rank[2];
        }
        qtlx_wave_sync();       // the reads of G and B are done before the next marker's tile is written
    }

    if (q.r0 + q.rn <= q.T) return;       // (the same for every wave: a tile without permuted columns)
    __syncthreads();
    double* R = &lds[0][0];
    R[(wib * QTLX_NSTAT + 0) * 64 + lane] = mx0;
    R[(wib * QTLX_NSTAT + 1) * 64 + lane] = mx1;
    R[(wib * QTLX_NSTAT + 2) * 64 + lane] = mx2;
    R[(wib * QTLX_NSTAT + 3) * 64 + lane] = mx3;
    R[(wib * QTLX_NSTAT + 4) * 64 + lane] = mx4;
    __syncthreads();
    if (wib == 0 && mycol && gr >= q.T) {
        double* out = q.tilemax + (size_t)tile * QTLX_NSTAT * q.rstride;
#pragma unroll
        for (int t = 0; t < QTLX_NSTAT; t++) {
            double v = R[t * 64 + lane];
#pragma unroll
            for (int w = 1; w < QTLX_WAVES; w++) v = fmax(v, R[(w * QTLX_NSTAT + t) * 64 + lane]);
            out[(size_t)t * q.rstride + cb + lane] = v;
        }
    }
}
void launch_qtlx_markers(const QtlxParams& q, hipStream_t stream)
{
    const int cols = 16 * QTLX_NT;
    hipLaunchKernelGGL(qtlx_marker_kernel, dim3(q.n_tiles, (q.rn + cols - 1) / cols), dim3(64 * QTLX_WAVES), 0, stream, q);
}

// perm_max[p][t][c][5] = the maxima over the chromosome's tiles, in ascending order (one thread per chromosome and column)
__global__ __launch_bounds__(64) void qtlx_finish_kernel(QtlxParams q)
{
    const int rr = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (rr >= q.rn) return;
    const int gr = q.r0 + rr;
    if (gr < q.T) return;
    double v[QTLX_NSTAT];
#pragma unroll
    for (int t = 0; t < QTLX_NSTAT; t++) v[t] = 0.0;
    for (int tl = q.tile_start[c]; tl < q.tile_start[c + 1]; tl++) {
        const double* in = q.tilemax + (size_t)tl * QTLX_NSTAT * q.rstride + rr;
#pragma unroll
        for (int t = 0; t < QTLX_NSTAT; t++) v[t] = fmax(v[t], in[(size_t)t * q.rstride]);
    }
    const int p = gr / q.T - 1, tr = gr % q.T;
    double*   out = q.pmax + (((size_t)p * q.T + tr) * q.C + c) * QTLX_NSTAT;
#pragma unroll
    for (int t = 0; t < QTLX_NSTAT; t++) out[t] = v[t];
}
void launch_qtlx_finish(const QtlxParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlx_finish_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

} // namespace cnf2
