// cnf2_qtlcof_kernels.hip -- the kernels of the cofactor scan (cnf2_qtl_scan_cof, include/cnf2hip.h): per marker the
// Haley-Knott model [X0, cofactors, marker] of phenotype columns, observed and permuted, on the origin rows, with every
// cofactor left out of the design inside its own window.  The model and every decision about degenerate cells live in
// cnf2_qtlcof.h; this file forms the sums.
//
//   qtlcof_mask_kernel    per chromosome and individual: used, and skipped neither there nor on any cofactor's chromosome
//   qtlcof_gather_kernel  the cofactor columns [n][ne Q], once per call
//   (qtl_gather_kernel of cnf2_qtl_kernels.hip makes the column image)
//   qtlcof_null_kernel    per chromosome and column: n_c, sum c y^2, RSS0 of the null design
//   qtlcof_marker_kernel  the hot path: per marker the Gram matrix X'X and X'Y on the f64 matrix cores, factored once per marker
//   qtlcof_finish_kernel  per chromosome and permuted column: the maximum over the chromosome's marker tiles
//
// No kernel adds with atomics, the individuals are never split between waves and every sum runs over them in ascending
// order: a call gives the same bits every time, whatever the column tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlcof.h"

namespace cnf2 {

typedef double qcd2 __attribute__((ext_vector_type(2)));
typedef double qcd4 __attribute__((ext_vector_type(4)));

constexpr int QTLCOF_LD    = QTL2_W + 1;   // doubles per LDS row: the 32 lanes a ds_read_b64 serves cover the 64 banks
constexpr int QTLCOF_NT    = 4;            // column tiles of 16 per wave: a block takes 64 columns
constexpr int QTLCOF_WAVES = 4;            // waves per block: the same columns, adjacent markers of the tile
constexpr int QTLCOF_KU    = 4;            // k-steps of 4 individuals requested together

// what a wave wrote to LDS is there for its other lanes
__device__ __forceinline__ void qtlcof_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool qtlcof_row_set(const double* o) { return o[0] != 0.0 || o[1] != 0.0 || o[2] != 0.0 || o[3] != 0.0; }

// c_i of chromosome c: used, not skipped on c, not skipped on the chromosome of any cofactor (left out anywhere or not), so
// that the mask and n_c depend on the chromosome only
__global__ __launch_bounds__(256) void qtlcof_mask_kernel(QtlcofParams q)
{
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (i >= q.n) return;
    const double* row = q.origin + (size_t)i * q.M * 4;
    bool          on  = q.use[i] != 0 && qtlcof_row_set(row + (size_t)q.cs[c] * 4);
    for (int k = 0; k < q.Q; k++) on = on && qtlcof_row_set(row + (size_t)q.cofstart[k] * 4);
    q.cmask[(size_t)c * q.n + i] = on ? 1 : 0;
}
void launch_qtlcof_mask(const QtlcofParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlcof_mask_kernel, dim3((q.n + 255) / 256, q.C), dim3(256), 0, stream, q);
}

// cofimg[i][ne k + e]: effect e of cofactor k's row, one thread per individual and cofactor: the marker kernel then forms a
// cofactor entry with one load, as it forms a covariate entry
__global__ __launch_bounds__(256) void qtlcof_gather_kernel(QtlcofParams q)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= q.n * q.Q) return;
    const int     i = t / q.Q, k = t - i * q.Q, ne = q.additive ? 1 : 2;
    const double* o = q.origin + ((size_t)i * q.M + q.cof[k]) * 4;
    double*       out = q.cofimg + (size_t)i * ne * q.Q + (size_t)ne * k;
    out[0] = o[3] - o[0];
    if (ne == 2) out[1] = o[1] + o[2];
}
void launch_qtlcof_gather(const QtlcofParams& q, hipStream_t stream)
{
    if (q.Q == 0) return;
    hipLaunchKernelGGL(qtlcof_gather_kernel, dim3((q.n * q.Q + 255) / 256), dim3(256), 0, stream, q);
}

// covariate k of individual i as column k of X0 (column 0 is the intercept)
__device__ __forceinline__ double qtlcof_x(const QtlcofParams& q, int i, int k) { return k == 0 ? 1.0 : q.cov[(size_t)i * q.K + (k - 1)]; }

// One block per chromosome and 64 columns: n_c, S11 = X0'X0 (one thread per entry) and its factor, then one thread per
// column b0 = X0'y and sum c y^2 over the individuals in ascending order, and RSS0 (cnf2_qtlcof.h).  yy is kept for the
// marker kernel.
__global__ __launch_bounds__(64) void qtlcof_null_kernel(QtlcofParams q)
{
    __shared__ double G[QTL2_W * QTLCOF_LD];
    __shared__ double B[64 * QTLCOF_LD];
    __shared__ int    cnt[64];
    __shared__ int    fshare[2];
    constexpr int NX = 8;                // columns of X0 per row of threads: 64 threads cover an 8 x 8 block of S11 at a time
    const int      tid = threadIdx.x, c = blockIdx.y;
    const uint8_t* cm = q.cmask + (size_t)c * q.n;
    const int      nx = q.K + 1;
    for (int t = tid; t < QTL2_W * QTLCOF_LD; t += 64) G[t] = 0.0;
    for (int t = tid; t < 64 * QTLCOF_LD; t += 64) B[t] = 0.0;
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
                    if (cm[i]) s += qtlcof_x(q, i, jx) * qtlcof_x(q, i, kx);
                G[jx * QTLCOF_LD + kx] = s;
            }
        }
    const int  rr = blockIdx.x * 64 + tid;
    const bool valid = rr < q.rn;
    const int  rc = valid ? rr : 0;
    double     yy = 0.0;
    double*    b = B + tid * QTLCOF_LD;
    for (int i = 0; i < q.n; i++) {
        if (!cm[i]) continue;
        const double y = q.Y[(size_t)i * q.rstride + rc];
        for (int k = 0; k < nx; k++) b[k] += qtlcof_x(q, i, k) * y;
        yy += y * y;
    }
    __syncthreads();
    const QtlcofDesign ds = qtlcof_design(q.K, q.Q, q.additive != 0);
    if (tid == 0) {
        int n_c = 0;
        for (int t = 0; t < 64; t++) n_c += cnt[t];
        const QtlcofFactor f0 = qtlcof_factor(G, QTLCOF_LD, ds, n_c, ds.nx);
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
            for (int k = 0; k < j; k++) s -= G[j * QTLCOF_LD + k] * b[k];
            b[j] = s / G[j * QTLCOF_LD + j];
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
void launch_qtlcof_null(const QtlcofParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlcof_null_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

// The marker kernel: qtlx_marker_kernel's batched small SYRK (cnf2_qtlx_kernels.hip) with another design.  A block takes one
// marker tile -- at most QTLCOF_TILE consecutive markers of one chromosome -- and 64 columns; its four waves take the tile's
// markers in turn, so that the waves running together read adjacent 32-byte rows of an individual: one 128-byte line.  Per
// marker a wave walks every individual in ascending order, four per v_mfma_f64_16x16x4_f64.  Lane (design column oi,
// individual ok) forms its own design entry in registers: a column of X0 or of the cofactors is one load from the covariates
// or the cofactor image (which column, and with which stride, is fixed per lane before the loops: no register array is
// indexed), a column of the marker is a or d of the individual's 32-byte origin row; rows past the design's width are zero.
// Which cofactors are left out at the marker is the wave-uniform word skipw[m]; the lanes of a left-out cofactor's columns
// feed exact zeros, so that the column has raw diagonal 0 and the rank rule drops it: the column order is the same at every
// marker.  In this instruction's layout the A operand X' and the B operand X are the same register value, so the Gram matrix
// is acc = mfma(x, x, acc); X'Y is one more instruction per 16 columns against 16 doubles of an image row.  Individuals past
// n and columns past the tile's are clamped addresses, zero operands and masked outputs: no load leaves its array.
// Epilogue: the Gram tile and X'Y go through the wave's LDS; lane 0 factors the tile once with the rank rule, then one lane
// per column does the forward substitution, for an observed column the back-substitution, and the cell (cnf2_qtlcof.h).
// The observed columns are stored; a permuted one goes into a running maximum per lane where the marker lies in no
// cofactor's range, reduced over the block's waves in a fixed order: one value per (tile, column).
__global__ __launch_bounds__(64 * QTLCOF_WAVES, 2) void qtlcof_marker_kernel(QtlcofParams q)
{
    __shared__ double lds[QTLCOF_WAVES][(QTL2_W + 16 * QTLCOF_NT) * QTLCOF_LD];
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x, cb = blockIdx.y * 16 * QTLCOF_NT;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int oi = lane & 15, ok = lane >> 4;
    const int n = q.n;
    const size_t   os = (size_t)q.M * 4;
    const uint8_t* cm = q.cmask + (size_t)c * n;
    const int      n_c = q.nc[c];
    const QtlcofDesign ds = qtlcof_design(q.K, q.Q, q.additive != 0);
    int se, sz;
    qtlcof_column(ds, oi, &se, &sz);
    // the lane's column of the covariates or of the cofactor image: one pointer and one stride, fixed here
    const bool    zload = (se == QTLX_ONE && sz > 0) || se == QTLCOF_COF;
    const double* zp = se == QTLCOF_COF ? q.cofimg + sz : q.cov + (sz > 0 ? sz - 1 : 0);
    const size_t  zs = se == QTLCOF_COF ? (size_t)ds.nc : (size_t)q.K;
    const uint32_t mybit = se == QTLCOF_COF ? 1u << (sz / ds.ne) : 0u;
    double* G = lds[wib];
    double* B = G + QTL2_W * QTLCOF_LD;
    int  col[QTLCOF_NT];
    bool cval[QTLCOF_NT];
#pragma unroll
    for (int nt = 0; nt < QTLCOF_NT; nt++) {
        const int cc = cb + nt * 16 + oi;
        cval[nt] = cc < q.rn;
        col[nt]  = cval[nt] ? cc : 0;
    }
    const bool mycol = cb + lane < q.rn;
    const int  myc   = mycol ? cb + lane : 0;
    const int  gr    = q.r0 + myc;
    const double yy  = q.yy[(size_t)c * q.rstride + myc];
    double     mx = 0.0;                   // (no conditional LOD is negative: 0 is the maximum's identity)

#pragma unroll 1
    for (int s = wib; s < len; s += QTLCOF_WAVES) {
        const int      m = m0 + s;
        const uint32_t skipped = q.skipw[m];
        const bool     live = se != QTLX_NONE && (skipped & mybit) == 0u;       // the lane's column is in the design at m
        qcd4 accG = qcd4{0.0, 0.0, 0.0, 0.0}, accY[QTLCOF_NT];
#pragma unroll
        for (int nt = 0; nt < QTLCOF_NT; nt++) accY[nt] = qcd4{0.0, 0.0, 0.0, 0.0};

        if (n_c >= ds.w + 1) {
#pragma unroll 1
            for (int i0 = 0; i0 < n; i0 += 4 * QTLCOF_KU) {
                qcd2   p01[QTLCOF_KU], p23[QTLCOF_KU];
                double z[QTLCOF_KU], y[QTLCOF_KU][QTLCOF_NT];
                bool   in[QTLCOF_KU], on[QTLCOF_KU];
#pragma unroll
                for (int u = 0; u < QTLCOF_KU; u++) {
                    const int i  = i0 + 4 * u + ok;
                    in[u]        = i < n;
                    const int ic = in[u] ? i : n - 1;
                    const double* p = q.origin + (size_t)ic * os + (size_t)m * 4;
                    p01[u] = *(const qcd2*)p;
                    p23[u] = *(const qcd2*)(p + 2);
                    on[u]  = in[u] && cm[ic] != 0;
                    z[u]   = zload ? zp[(size_t)ic * zs] : 1.0;
#pragma unroll
                    for (int nt = 0; nt < QTLCOF_NT; nt++) y[u][nt] = q.Y[(size_t)ic * q.rstride + col[nt]];
                }
#pragma unroll
                for (int u = 0; u < QTLCOF_KU; u++) {
                    const double a = p23[u].y - p01[u].x, d = p01[u].y + p23[u].x;
                    const double ee = se == QTLX_A ? a : (se == QTLX_D ? d : z[u]);
                    const double x  = (on[u] && live) ? ee : 0.0;
                    accG = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, accG, 0, 0, 0);
#pragma unroll
                    for (int nt = 0; nt < QTLCOF_NT; nt++) {
                        const double yv = (in[u] && cval[nt]) ? y[u][nt] : 0.0;
                        accY[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yv, x, accY[nt], 0, 0, 0);
                    }
                }
            }
        }

        // G[row][column] and B[column of Y][design column]
#pragma unroll
        for (int reg = 0; reg < 4; reg++) G[(ok + 4 * reg) * QTLCOF_LD + oi] = accG[reg];
#pragma unroll
        for (int nt = 0; nt < QTLCOF_NT; nt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) B[(nt * 16 + ok + 4 * reg) * QTLCOF_LD + oi] = accY[nt][reg];
        qtlcof_wave_sync();
        QtlcofFactor f;
        f.usable = 0, f.rank_cof = 0, f.rank = 0;
        if (lane == 0) f = qtlcof_factor(G, QTLCOF_LD, ds, n_c, ds.w);
        f.usable   = __builtin_amdgcn_readfirstlane(f.usable);
        f.rank_cof = __builtin_amdgcn_readfirstlane(f.rank_cof);
        f.rank     = __builtin_amdgcn_readfirstlane(f.rank);
        qtlcof_wave_sync();
        const bool observed = mycol && gr < q.T;
        double*    brow = B + lane * QTLCOF_LD;
        const QtlcofCell cell = qtlcof_cell(G, QTLCOF_LD, ds, f, brow, 1, yy, n_c, observed);
        if (observed) {
            const size_t o = (size_t)gr * q.M + m;
            q.lod[o]      = cell.lod;
            q.lod_base[o] = cell.lod_base;
            double* co = q.coef + o * ds.ne;
#pragma unroll 1
            for (int j = 0; j < ds.ne; j++) co[j] = brow[ds.nx + ds.nc + j];
        }
        if (mycol && gr >= q.T && skipped == 0u) mx = fmax(mx, cell.lod);
        if (lane == 0 && q.r0 == 0 && cb == 0) {
            q.rank[m]     = f.rank;
            q.rank_cof[m] = f.rank_cof;
        }
        qtlcof_wave_sync();       // the reads of G and B are done before the next marker's tile is written
    }

    if (q.r0 + q.rn <= q.T) return;       // (the same for every wave: a tile without permuted columns)
    __syncthreads();
    double* R = &lds[0][0];
    R[wib * 64 + lane] = mx;
    __syncthreads();
    if (wib == 0 && mycol && gr >= q.T) {
        double v = R[lane];
#pragma unroll
        for (int w = 1; w < QTLCOF_WAVES; w++) v = fmax(v, R[w * 64 + lane]);
        q.tilemax[(size_t)tile * q.rstride + cb + lane] = v;
    }
}
void launch_qtlcof_markers(const QtlcofParams& q, hipStream_t stream)
{
    const int cols = 16 * QTLCOF_NT;
    hipLaunchKernelGGL(qtlcof_marker_kernel, dim3(q.n_tiles, (q.rn + cols - 1) / cols), dim3(64 * QTLCOF_WAVES), 0, stream, q);
}

// perm_max[p][t][c] = the maximum over the chromosome's tiles, in ascending order (one thread per chromosome and column)
__global__ __launch_bounds__(64) void qtlcof_finish_kernel(QtlcofParams q)
{
    const int rr = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (rr >= q.rn) return;
    const int gr = q.r0 + rr;
    if (gr < q.T) return;
    double v = 0.0;
    for (int tl = q.tile_start[c]; tl < q.tile_start[c + 1]; tl++) v = fmax(v, q.tilemax[(size_t)tl * q.rstride + rr]);
    const int p = gr / q.T - 1, tr = gr % q.T;
    q.pmax[((size_t)p * q.T + tr) * q.C + c] = v;
}
void launch_qtlcof_finish(const QtlcofParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlcof_finish_kernel, dim3((q.rn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

} // namespace cnf2
