// cnf2_qtl2_kernels.hip -- the kernels of the two-QTL pair scan (cnf2_qtl_scan2, include/cnf2hip.h): for every pair of
// selected loci the additive-pair and the full (epistatic) Haley-Knott model of phenotype columns, observed and permuted, on
// the origin rows.  The model and every decision about degenerate cells live in cnf2_qtl2.h; this file forms the sums.
//
//   qtl2_mask_kernel    per chromosome and individual: used, and not skipped on the chromosome
//   qtl2_fill_kernel    the cells of the L x L outputs that carry no pair: NaN / -1
//   (qtl_gather_kernel of cnf2_qtl_kernels.hip makes the column image Y[n][rn] of a tile)
//   qtl2_null_kernel    per chromosome pair and column: n_c, sum c y^2, RSS0 of the null design
//   qtl2_pair_kernel    the hot path: per pair the Gram matrix X'X and X'Y on the f64 matrix cores, factored once per pair
//   qtl2_pair_linked_kernel   the same body with the joint rows of the pairs on one chromosome (cnf2_qtl_scan2_linked)
//   qtl2_finish_kernel  per permuted column: the three maxima over all pairs
//
// No kernel adds with atomics, the individuals are never split between waves and every sum runs over them in ascending
// order: a call gives the same bits every time, whatever the column tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtl2.h"

namespace cnf2 {

typedef double q2d2 __attribute__((ext_vector_type(2)));
typedef double q2d4 __attribute__((ext_vector_type(4)));

constexpr int QTL2_LD    = QTL2_W + 1;   // doubles per LDS row: the 32 lanes a ds_read_b64 serves cover the 64 banks
constexpr int QTL2_NT    = 4;            // column tiles of 16 per wave: a block takes 64 columns
constexpr int QTL2_WAVES = 4;            // waves per block: the same first locus and columns, consecutive second loci
constexpr int QTL2_KU    = 4;            // k-steps of 4 individuals requested together

// what a wave wrote to LDS is there for its other lanes
__device__ __forceinline__ void qtl2_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void qtl2_mask_kernel(Qtl2Params q)
{
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (i >= q.n) return;
    const double* o = q.origin + ((size_t)i * q.M + q.cs[c]) * 4;
    q.cmask[(size_t)c * q.n + i] = (q.use[i] && (o[0] != 0.0 || o[1] != 0.0 || o[2] != 0.0 || o[3] != 0.0)) ? 1 : 0;
}
void launch_qtl2_mask(const Qtl2Params& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtl2_mask_kernel, dim3((q.n + 255) / 256, q.C), dim3(256), 0, stream, q);
}

// one thread per cell (j, k) of the L x L outputs: the diagonal and the lower triangle carry no pair
__global__ __launch_bounds__(256) void qtl2_fill_kernel(Qtl2Params q)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, LL = (size_t)q.L * q.L;
    if (e >= LL) return;
    const int j = (int)(e / q.L), k = (int)(e % q.L);
    if (j < k) return;
    q.rank_add[e] = q.rank_full[e] = -1;
    for (int t = 0; t < q.T; t++) q.lod_add[(size_t)t * LL + e] = q.lod_full[(size_t)t * LL + e] = (double)NAN;
}
void launch_qtl2_fill(const Qtl2Params& q, hipStream_t stream)
{
    const size_t LL = (size_t)q.L * q.L;
    hipLaunchKernelGGL(qtl2_fill_kernel, dim3((unsigned)((LL + 255) / 256)), dim3(256), 0, stream, q);
}

// covariate k of individual i as column k of X0 (column 0 is the intercept)
__device__ __forceinline__ double qtl2_x(const Qtl2Params& q, int i, int k) { return k == 0 ? 1.0 : q.cov[(size_t)i * q.K + (k - 1)]; }

// One block per chromosome pair c1 <= c2 and 64 columns: n_c, S11 = X0'X0 (one thread per entry) and its factor, then one
// thread per column b0 = X0'y and sum c y^2 over the individuals in ascending order, and the cell of the null design alone
// (cnf2_qtl2.h).  rss0 and n_used are symmetric; yy is kept for the pair kernel.
__global__ __launch_bounds__(64) void qtl2_null_kernel(Qtl2Params q)
{
    __shared__ double G[QTL2_W * QTL2_LD];
    __shared__ double B[64 * QTL2_LD];
    __shared__ int    cnt[64];
    __shared__ int    fshare[2];
    constexpr int NX = QTL2_MAXK + 1;
    const int tid = threadIdx.x, c1 = blockIdx.y / q.C, c2 = blockIdx.y % q.C;
    if (c1 > c2) return;
    const uint8_t *cm1 = q.cmask + (size_t)c1 * q.n, *cm2 = q.cmask + (size_t)c2 * q.n;
    const int      nx = q.K + 1;
    for (int t = tid; t < QTL2_W * QTL2_LD; t += 64) G[t] = 0.0;
    for (int t = tid; t < 64 * QTL2_LD; t += 64) B[t] = 0.0;
    int mine = 0;
    for (int i = tid; i < q.n; i += 64) mine += (cm1[i] && cm2[i]) ? 1 : 0;
    cnt[tid] = mine;
    __syncthreads();
    const int jx = tid / NX, kx = tid % NX;
    if (tid < NX * NX && jx < nx && kx <= jx) {
        double s = 0.0;
        for (int i = 0; i < q.n; i++)
            if (cm1[i] && cm2[i]) s += qtl2_x(q, i, jx) * qtl2_x(q, i, kx);
        G[jx * QTL2_LD + kx] = s;
    }
    const int  rr = blockIdx.x * 64 + tid;
    const bool valid = rr < q.rn;
    const int  rc = valid ? rr : 0;
    double     b[NX], yy = 0.0;
#pragma unroll
    for (int k = 0; k < NX; k++) b[k] = 0.0;
    for (int i = 0; i < q.n; i++) {
        if (!(cm1[i] && cm2[i])) continue;
        const double y = q.Y[(size_t)i * q.rstride + rc];
#pragma unroll
        for (int k = 0; k < NX; k++)
            if (k < nx) b[k] += qtl2_x(q, i, k) * y;
        yy += y * y;
    }
#pragma unroll
    for (int k = 0; k < NX; k++) B[tid * QTL2_LD + k] = b[k];
    __syncthreads();
    Qtl2Design ds;
    ds.nx = nx, ds.nadd = 0, ds.nint = 0;
    if (tid == 0) {
        int n_c = 0;
        for (int t = 0; t < 64; t++) n_c += cnt[t];
        const Qtl2Factor f0 = qtl2_factor(G, QTL2_LD, ds, n_c, q.K, true);
        fshare[0] = n_c;
        fshare[1] = f0.usable;
    }
    __syncthreads();
    const int  n_c = fshare[0];
    Qtl2Factor f;
    f.usable = fshare[1], f.rank_add = 0, f.rank_full = -1;
    const Qtl2Cell cell = qtl2_cell(G, QTL2_LD, ds, f, B + tid * QTL2_LD, 1, yy, n_c, true);
    if (tid == 0 && blockIdx.x == 0) q.nc[c1 * q.C + c2] = q.nc[c2 * q.C + c1] = n_c;
    if (!valid) return;
    q.yy[(size_t)(c1 * q.C + c2) * q.rstride + rr] = yy;
    const int gr = q.r0 + rr;
    if (gr < q.T) q.rss0[((size_t)gr * q.C + c1) * q.C + c2] = q.rss0[((size_t)gr * q.C + c2) * q.C + c1] = cell.rss0;
}
void launch_qtl2_null(const Qtl2Params& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtl2_null_kernel, dim3((q.rn + 63) / 64, q.C * q.C), dim3(64), 0, stream, q);
}

// The pair kernel: a batched small SYRK.  A block takes one first locus j, QTL2_CHUNK consecutive second loci and 64
// columns; its four waves take the second loci in turn, so that they ask for the same rows of locus 1 at the same time.  Per
// pair a wave walks every individual in ascending order, four per v_mfma_f64_16x16x4_f64 (operand and result layouts:
// place_rows_kernel in cnf2_kernels.hip).  Lane (design column oi, individual ok) forms its own design entry in registers
// from the individual's two 32-byte origin rows and its covariate: a mask or covariate value, a, d, or a product; rows past
// the design's width are zero.  In this instruction's layout the A operand X' and the B operand X are the same register
// value, so the Gram matrix is acc = mfma(x, x, acc); X'Y is one more instruction per 16 columns against 16 doubles of an
// image row, with the columns as the rows of the result.  Individuals past n and columns past the tile's are clamped
// addresses, zero operands and masked outputs: nothing is padded in HBM and no load leaves its array.
// Epilogue: the Gram tile and X'Y go through the wave's LDS; lane 0 factors the tile once with the rank rule, then one lane
// per column does the forward substitution and the cell (cnf2_qtl2.h).  The observed columns are stored; the permuted ones
// go into three running maxima per lane, reduced over the block's waves in a fixed order: one value per (j, chunk, column).
// LINKED (cnf2_qtl_scan2_linked): a pair on one chromosome is fitted the full design too.  The lane of an interaction column
// reads four cells of the pair's 128-byte joint row instead of forming a product from the two origin rows:
//   E[a1 a2] = J33 - J30 - J03 + J00,  E[a1 d2] = J31 + J32 - J01 - J02,  E[d1 a2] = J13 + J23 - J10 - J20,  E[d1 d2] = J11 + J12 + J21 + J22
// (J[4 u + v], u the class at locus 1).  Every other column, and every pair on two chromosomes, is formed as without it.
template <bool LINKED>
__device__ __forceinline__ void qtl2_pair_body(const Qtl2Params& q)
{
    __shared__ double lds[QTL2_WAVES][(QTL2_W + 16 * QTL2_NT) * QTL2_LD];
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = blockIdx.x, kb = j + 1 + blockIdx.y * QTL2_CHUNK, cb = blockIdx.z * 16 * QTL2_NT;
    if (kb >= q.L) return;
    const int oi = lane & 15, ok = lane >> 4;
    const int n = q.n;
    const int m1 = q.sel[j], c1 = q.selchrom[j];
    const size_t   os  = (size_t)q.M * 4;
    const uint8_t* cm1 = q.cmask + (size_t)c1 * n;
    double* G = lds[wib];
    double* B = G + QTL2_W * QTL2_LD;
    int  col[QTL2_NT];
    bool cval[QTL2_NT];
#pragma unroll
    for (int nt = 0; nt < QTL2_NT; nt++) {
        const int cc = cb + nt * 16 + oi;
        cval[nt] = cc < q.rn;
        col[nt]  = cval[nt] ? cc : 0;
    }
    const bool mycol = cb + lane < q.rn;
    const int  myc   = mycol ? cb + lane : 0;
    const int  gr    = q.r0 + myc;
    double     mx0 = 0.0, mx1 = 0.0, mx2 = 0.0;      // a LOD and lod_full - lod_add are never negative: 0 is the maximum's identity

#pragma unroll 1
    for (int s = wib; s < QTL2_CHUNK; s += QTL2_WAVES) {
        const int k = kb + s;
        if (k >= q.L) break;
        const int      m2 = q.sel[k], c2 = q.selchrom[k];
        const bool     linked = LINKED && c1 == c2;          // a pair of one chromosome with its joint rows
        const bool     same = !LINKED && c1 == c2;           // ... without: no full design
        const uint8_t* cm2 = q.cmask + (size_t)c2 * n;
        const int      cp  = c1 * q.C + c2;
        const int      n_c = q.nc[cp];
        const Qtl2Design ds = qtl2_design(q.K, q.additive != 0, same);
        int su, sv;
        qtl2_column(ds, q.additive != 0, oi, &su, &sv);
        const double* covp = q.cov + (su == 1 ? oi - 1 : 0);
        // LINKED: the four cells of the joint row that this lane's interaction column adds up (cnf2_qtl2.h)
        const bool inter = linked && su >= 2 && su != 4 && sv >= 1;
        int        jc[4] = {0, 0, 0, 0}, neg = 0;
        size_t     prow = 0;
        if (LINKED && inter) {
            qtl2_joint_cells(su == 3, sv == 2, jc, &neg);
            prow = (size_t)(q.pair_off[j] + k - j - 1) * 16;
        }
        q2d4 accG = q2d4{0.0, 0.0, 0.0, 0.0}, accY[QTL2_NT];
#pragma unroll
        for (int nt = 0; nt < QTL2_NT; nt++) accY[nt] = q2d4{0.0, 0.0, 0.0, 0.0};

        if (n_c >= q.K + 10) {
#pragma unroll 1
            for (int i0 = 0; i0 < n; i0 += 4 * QTL2_KU) {
                q2d2   p01[QTL2_KU], p23[QTL2_KU], r01[QTL2_KU], r23[QTL2_KU];
                double z[QTL2_KU], y[QTL2_KU][QTL2_NT], jq[QTL2_KU][4];
                bool   in[QTL2_KU], on[QTL2_KU];
#pragma unroll
                for (int u = 0; u < QTL2_KU; u++) {
                    const int i  = i0 + 4 * u + ok;
                    in[u]        = i < n;
                    const int ic = in[u] ? i : n - 1;
                    const double* p = q.origin + (size_t)ic * os + (size_t)m1 * 4;
                    const double* r = q.origin + (size_t)ic * os + (size_t)m2 * 4;
                    p01[u] = *(const q2d2*)p;
                    p23[u] = *(const q2d2*)(p + 2);
                    r01[u] = *(const q2d2*)r;
                    r23[u] = *(const q2d2*)(r + 2);
                    on[u]  = in[u] && cm1[ic] != 0 && cm2[ic] != 0;
                    z[u]   = su == 1 ? covp[(size_t)ic * q.K] : 1.0;
                    if constexpr (LINKED) {
#pragma unroll
                        for (int t = 0; t < 4; t++) jq[u][t] = 0.0;
                        if (inter) {
                            const double* jr = q.joint + (size_t)ic * q.n_pairs * 16 + prow;
#pragma unroll
                            for (int t = 0; t < 4; t++) jq[u][t] = jr[jc[t]];
                        }
                    }
#pragma unroll
                    for (int nt = 0; nt < QTL2_NT; nt++) y[u][nt] = q.Y[(size_t)ic * q.rstride + col[nt]];
                }
#pragma unroll
                for (int u = 0; u < QTL2_KU; u++) {
                    const double a1 = p23[u].y - p01[u].x, d1 = p01[u].y + p23[u].x;
                    const double a2 = r23[u].y - r01[u].x, d2 = r01[u].y + r23[u].x;
                    const double uu = su == 0 ? 1.0 : (su == 1 ? z[u] : (su == 2 ? a1 : d1));
                    const double vv = sv == 0 ? 1.0 : (sv == 1 ? a2 : d2);
                    double       x  = (on[u] && su != 4) ? uu * vv : 0.0;
                    if constexpr (LINKED) {
                        if (inter) x = on[u] ? qtl2_joint_value(jq[u][0], jq[u][1], jq[u][2], jq[u][3], neg) : 0.0;
                    }
                    accG = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, accG, 0, 0, 0);
#pragma unroll
                    for (int nt = 0; nt < QTL2_NT; nt++) {
                        const double yv = (in[u] && cval[nt]) ? y[u][nt] : 0.0;
                        accY[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yv, x, accY[nt], 0, 0, 0);
                    }
                }
            }
        }

        // G[row][column] and B[column of Y][design column]
#pragma unroll
        for (int reg = 0; reg < 4; reg++) G[(ok + 4 * reg) * QTL2_LD + oi] = accG[reg];
#pragma unroll
        for (int nt = 0; nt < QTL2_NT; nt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) B[(nt * 16 + ok + 4 * reg) * QTL2_LD + oi] = accY[nt][reg];
        qtl2_wave_sync();
        Qtl2Factor f;
        f.usable = 0, f.rank_add = 0, f.rank_full = 0;
        if (lane == 0) f = qtl2_factor(G, QTL2_LD, ds, n_c, q.K, same);
        f.usable    = __builtin_amdgcn_readfirstlane(f.usable);
        f.rank_add  = __builtin_amdgcn_readfirstlane(f.rank_add);
        f.rank_full = __builtin_amdgcn_readfirstlane(f.rank_full);
        qtl2_wave_sync();
        const double   yy   = q.yy[(size_t)cp * q.rstride + myc];
        const Qtl2Cell cell = qtl2_cell(G, QTL2_LD, ds, f, B + lane * QTL2_LD, 1, yy, n_c, same);
        const size_t   o    = (size_t)j * q.L + k;
        if (mycol && gr < q.T) {
            const size_t LL = (size_t)q.L * q.L;
            q.lod_add[(size_t)gr * LL + o]  = cell.lod_add;
            q.lod_full[(size_t)gr * LL + o] = cell.lod_full;
        }
        if (mycol && gr >= q.T) {
            mx0 = fmax(mx0, cell.lod_add);
            if (!same) {
                mx1 = fmax(mx1, cell.lod_full);
                mx2 = fmax(mx2, cell.lod_full - cell.lod_add);
            }
        }
        if (lane == 0 && q.r0 == 0 && cb == 0) {
            q.rank_add[o]  = f.rank_add;
            q.rank_full[o] = f.rank_full;
        }
        qtl2_wave_sync();       // the reads of G and B are done before the next pair's tile is written
    }

    if (q.r0 + q.rn <= q.T) return;       // (the same for every wave: a tile without permuted columns)
    __syncthreads();
    double* R = &lds[0][0];
    R[(wib * 3 + 0) * 64 + lane] = mx0;
    R[(wib * 3 + 1) * 64 + lane] = mx1;
    R[(wib * 3 + 2) * 64 + lane] = mx2;
    __syncthreads();
    if (wib == 0 && mycol && gr >= q.T) {
        double* out = q.chunkmax + ((size_t)j * q.n_chunks + blockIdx.y) * 3 * q.rstride;
#pragma unroll
        for (int t = 0; t < 3; t++) {
            double v = R[t * 64 + lane];
#pragma unroll
            for (int w = 1; w < QTL2_WAVES; w++) v = fmax(v, R[(w * 3 + t) * 64 + lane]);
            out[(size_t)t * q.rstride + cb + lane] = v;
        }
    }
}
__global__ __launch_bounds__(64 * QTL2_WAVES, 2) void qtl2_pair_kernel(Qtl2Params q) { qtl2_pair_body<false>(q); }
__global__ __launch_bounds__(64 * QTL2_WAVES, 2) void qtl2_pair_linked_kernel(Qtl2Params q) { qtl2_pair_body<true>(q); }
void launch_qtl2_pairs(const Qtl2Params& q, hipStream_t stream)
{
    const int  cols = 16 * QTL2_NT;
    const dim3 grid(q.L - 1, q.n_chunks, (q.rn + cols - 1) / cols);
    if (q.joint) hipLaunchKernelGGL(qtl2_pair_linked_kernel, grid, dim3(64 * QTL2_WAVES), 0, stream, q);
    else hipLaunchKernelGGL(qtl2_pair_kernel, grid, dim3(64 * QTL2_WAVES), 0, stream, q);
}

// perm_max[p][t][3]: one thread per permuted column takes the maxima over every first locus and its chunks
__global__ __launch_bounds__(64) void qtl2_finish_kernel(Qtl2Params q)
{
    const int rr = blockIdx.x * 64 + threadIdx.x;
    if (rr >= q.rn) return;
    const int gr = q.r0 + rr;
    if (gr < q.T) return;
    double v[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j + 1 < q.L; j++) {
        const int nch = (q.L - 1 - j + QTL2_CHUNK - 1) / QTL2_CHUNK;
        for (int ch = 0; ch < nch; ch++) {
            const double* in = q.chunkmax + ((size_t)j * q.n_chunks + ch) * 3 * q.rstride + rr;
#pragma unroll
            for (int t = 0; t < 3; t++) v[t] = fmax(v[t], in[(size_t)t * q.rstride]);
        }
    }
    const int p = gr / q.T - 1, tr = gr % q.T;
#pragma unroll
    for (int t = 0; t < 3; t++) q.pmax[((size_t)p * q.T + tr) * 3 + t] = v[t];
}
void launch_qtl2_finish(const Qtl2Params& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtl2_finish_kernel, dim3((q.rn + 63) / 64), dim3(64), 0, stream, q);
}

} // namespace cnf2
