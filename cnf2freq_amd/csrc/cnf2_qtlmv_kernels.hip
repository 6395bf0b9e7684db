// cnf2_qtlmv_kernels.hip -- the kernels of the multi-trait QTL scan (cnf2_qtl_scan_mv, include/cnf2hip.h): the joint Wilks'
// lambda LOD of T traits, observed and permuted, on the origin rows.  The model and every decision live in cnf2_qtlmv.h; this
// file forms the sums.  The chromosome masks, S11 and the marker records come from qtl_chrom_kernel and qtl_design_kernel
// (cnf2_qtl_kernels.hip).
//
//   qtlmv_gather_kernel    per group tile: the column image in operand order, traits padded with zero columns to T4
//   qtlmv_null_kernel      one wave per (chromosome, group): Y'CY, B0 = X0'Y, then the factor of E0 (qtlmv_factor)
//   qtlmv_scan_kernel<T4>  the hot path: qtl_scan_kernel's product on the f64 matrix cores, with the columns assigned to MFMA
//                          rows so that a lane's 16 accumulators are whole groups of one marker; epilogue in registers
//   qtlmv_finish_kernel    per chromosome and permuted group: the maximum over the chromosome's marker tiles
//
// No kernel adds with atomics and every sum runs over the individuals in ascending order: a call gives the same bits every
// time, whatever the group tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_qtlmv.h"

namespace cnf2 {

typedef double mvd2 __attribute__((ext_vector_type(2)));
typedef double mvd4 __attribute__((ext_vector_type(4)));

constexpr int QTLMV_NT    = 4;       // row blocks of 16 per wave: 64 padded columns
constexpr int QTLMV_WAVES = 4;       // waves per block: the same 16 markers, consecutive chunks of 64 columns
constexpr int QTLMV_KU    = 4;       // k-steps of 4 individuals requested together

// The row map.  In the result of v_mfma_f64_16x16x4_f64 (layouts: place_rows_kernel in cnf2_kernels.hip) lane (oi, ok) holds
// rows ok + 4 reg of block nt, for column oi.  A wave's 64 columns are 64 / T4 groups of T4 padded traits, and column
// 16 nt + r of the chunk, r = ok + 4 reg, is
//   T4 = 16: group ok,               trait 4 nt + reg
//   T4 =  8: group ok + 4 (nt / 2),  trait 4 (nt % 2) + reg
//   T4 =  4: group ok + 4 nt,        trait reg
// so that the 16 accumulators of a lane are 16 / T4 whole groups: group ok + 4 j of the wave, j < 16 / T4, has trait t in
// accumulator [j (T4 / 4) + t / 4][t % 4].
__device__ __forceinline__ void qtlmv_image_column(int T4, int col, int& group, int& trait)
{
    const int nt = col >> 4, r = col & 15, ok = r & 3, reg = r >> 2, per = T4 >> 2;       // per: blocks of a group
    group = ok + 4 * (nt / per);
    trait = 4 * (nt % per) + reg;
}

// Y[i][64 w + col]: wave chunk w holds the groups g0 + w (64 / T4) + group(col); 0 for an individual that is not used, a trait
// past T and a group past the tile
__global__ __launch_bounds__(256) void qtlmv_gather_kernel(QtlMvParams q)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)q.n * q.ystride) return;
    const int i = (int)(e / q.ystride), cc = (int)(e % q.ystride);
    int       gw, t;
    qtlmv_image_column(q.T4, cc & 63, gw, t);
    const int gl = (cc >> 6) * (64 / q.T4) + gw;
    double    y = 0.0;
    if (q.use[i] && t < q.T && gl < q.gn) {
        const int g = q.g0 + gl, src = g == 0 ? i : q.perm[(size_t)(g - 1) * q.n + i];
        y = q.pheno[(size_t)src * q.T + t];
    }
    q.Y[e] = y;
}
void launch_qtlmv_gather(const QtlMvParams& q, hipStream_t stream)
{
    const size_t e = (size_t)q.n * q.ystride;
    hipLaunchKernelGGL(qtlmv_gather_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, stream, q);
}

// One wave per (chromosome, group).  Its lanes take the pairs (t, s <= t) of Y'CY and the entries of B0, each summed over the
// individuals in ascending order; lane 0 then factors (qtlmv_factor) and writes the record.
__global__ __launch_bounds__(64) void qtlmv_null_kernel(QtlMvParams q)
{
    constexpr int TPMAX = QTLMV_MAXT * (QTLMV_MAXT + 1) / 2;
    __shared__ double yy[TPMAX];
    __shared__ double b0[QTL_NX * QTLMV_MAXT];
    __shared__ double work[QTLMV_WORK];
    const int      gl = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const int      g = q.g0 + gl, T = q.T, n = q.n;
    const uint8_t* cm = q.cmask + (size_t)c * n;
    const int32_t* pr = g == 0 ? nullptr : q.perm + (size_t)(g - 1) * n;
    const int      tp = qtlmv_tp(T);
    for (int p = lane; p < tp; p += 64) {
        int t = 0;
        while ((t + 1) * (t + 2) / 2 <= p) t++;
        const int s = p - t * (t + 1) / 2;
        double    sum = 0.0;
        for (int i = 0; i < n; i++) {
            if (!cm[i]) continue;
            const double* row = q.pheno + (size_t)(pr ? pr[i] : i) * T;
            sum += row[t] * row[s];
        }
        yy[p] = sum;
    }
    for (int e = lane; e < q.nx * T; e += 64) {
        const int k = e / T, t = e % T;
        double    sum = 0.0;
        for (int i = 0; i < n; i++) {
            if (!cm[i]) continue;
            const double x = k == 0 ? 1.0 : q.cov[(size_t)i * q.K + (k - 1)];
            sum += x * q.pheno[(size_t)(pr ? pr[i] : i) * T + t];
        }
        b0[e] = sum;
    }
    __syncthreads();
    if (lane == 0) {
        double*   rec = q.rec + ((size_t)c * q.gstride + gl) * qtlmv_rec_doubles(T);
        const int kept = qtlmv_factor(yy, b0, q.chol + (size_t)c * QTL_CHOL, q.nx, q.K, q.nc[c], T, work, rec);
        if (g == 0) q.trait_rank[c] = kept;
    }
}
void launch_qtlmv_null(const QtlMvParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlmv_null_kernel, dim3(q.gn, q.C), dim3(64), 0, stream, q);
}

// The product is qtl_scan_kernel's: a wave owns 16 markers of one tile x 64 padded columns and walks every individual in
// ascending order, four per v_mfma_f64_16x16x4_f64, both operands straight from global memory -- the marker operand from the
// 32-byte origin rows in place, the column operand 16 consecutive doubles of the image's row, which is laid out in operand
// order and padded, so that it needs no trait predicate.  Individuals past n and markers past the tile's end are clamped
// addresses and zero operands.
// Epilogue, lane-local: V = C - G B0, then qtlmv_cell with L streamed from the group's record (the 16 lanes of a quarter-wave
// read the same addresses).  The observed group writes lod and rank; a permuted group takes the maximum over the tile's
// markers, a butterfly over the 16 lanes.
template <int T4>
__global__ __launch_bounds__(64 * QTLMV_WAVES, 2) void qtlmv_scan_kernel(QtlMvParams q)
{
    constexpr int GL = 16 / T4, PER = T4 / 4;       // groups of a lane, row blocks of a group
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x;
    const int c = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int chunk = blockIdx.y * QTLMV_WAVES + wib, cb = chunk * 64;
    if (cb >= q.ystride) return;
    const int  oi = lane & 15, ok = lane >> 4;
    const bool mval = oi < len;
    const int  m = m0 + (mval ? oi : 0);
    const int  n = q.n;
    const double*  orow = q.origin + (size_t)m * 4;
    const size_t   os   = (size_t)q.M * 4;
    const uint8_t* cm   = q.cmask + (size_t)c * n;
    const double*  yrow = q.Y + cb + oi;
    mvd4 accA[QTLMV_NT], accD[QTLMV_NT];
#pragma unroll
    for (int nt = 0; nt < QTLMV_NT; nt++) accA[nt] = accD[nt] = mvd4{0.0, 0.0, 0.0, 0.0};

#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += 4 * QTLMV_KU) {
        mvd2   o01[QTLMV_KU], o23[QTLMV_KU];
        double y[QTLMV_KU][QTLMV_NT];
        bool   in[QTLMV_KU], on[QTLMV_KU];
#pragma unroll
        for (int u = 0; u < QTLMV_KU; u++) {
            const int i  = i0 + 4 * u + ok;
            in[u]        = i < n;
            const int ic = in[u] ? i : n - 1;
            const double* p = orow + (size_t)ic * os;
            o01[u] = *(const mvd2*)p;
            o23[u] = *(const mvd2*)(p + 2);
            on[u]  = in[u] && mval && cm[ic] != 0;
#pragma unroll
            for (int nt = 0; nt < QTLMV_NT; nt++) y[u][nt] = yrow[(size_t)ic * q.ystride + nt * 16];
        }
#pragma unroll
        for (int u = 0; u < QTLMV_KU; u++) {
            const double a = on[u] ? o23[u].y - o01[u].x : 0.0;
            const double d = on[u] ? o01[u].y + o23[u].x : 0.0;
#pragma unroll
            for (int nt = 0; nt < QTLMV_NT; nt++) {
                const double yy = in[u] ? y[u][nt] : 0.0;
                accA[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, a, accA[nt], 0, 0, 0);
                accD[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yy, d, accD[nt], 0, 0, 0);
            }
        }
    }

    const double* mrec = q.mk + (size_t)m * QTL_MK;
    const double  pa = mrec[QTL_PA], l = mrec[QTL_L], pd = mrec[QTL_PD];
    const int     n_c = q.nc[c], T = q.T;
    const size_t  recd = qtlmv_rec_doubles(T);
#pragma unroll
    for (int j = 0; j < GL; j++) {
        const int     gl   = chunk * (64 / T4) + ok + 4 * j;
        const bool    gval = gl < q.gn;
        const double* rec  = q.rec + ((size_t)c * q.gstride + (gval ? gl : 0)) * recd;
        const double* b0   = rec + qtlmv_o_b0(T);
        double        va[T4], vd[T4];
#pragma unroll
        for (int t = 0; t < T4; t++) {
            va[t] = accA[j * PER + t / 4][t % 4];
            vd[t] = accD[j * PER + t / 4][t % 4];
        }
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < q.nx) {
                const double ga = mrec[k], gd = mrec[QTL_NX + k];
#pragma unroll
                for (int t = 0; t < T4; t++)
                    if (t < T) {
                        const double b = b0[k * T + t];
                        va[t] -= ga * b;
                        vd[t] -= gd * b;
                    }
            }
        const double lod = qtlmv_cell<T4>(va, vd, rec, T, pa, l, pd, n_c);
        const int    g   = q.g0 + gl;
        if (gval && mval && g == 0) {
            q.lod[m]  = lod;
            q.rank[m] = qtlmv_rank(rec, T, pa, pd);
        }
        double v = (gval && mval) ? lod : 0.0;       // a LOD is never negative: 0 is the maximum's identity
        v = fmax(v, __shfl_xor(v, 1));
        v = fmax(v, __shfl_xor(v, 2));
        v = fmax(v, __shfl_xor(v, 4));
        v = fmax(v, __shfl_xor(v, 8));
        if (oi == 0 && gval && g > 0) q.tilemax[(size_t)tile * q.gstride + gl] = v;
    }
}
void launch_qtlmv_scan(const QtlMvParams& q, hipStream_t stream)
{
    const dim3 grid(q.n_tiles, (q.ystride / 64 + QTLMV_WAVES - 1) / QTLMV_WAVES), block(64 * QTLMV_WAVES);
    if (q.T4 == 4) hipLaunchKernelGGL(qtlmv_scan_kernel<4>, grid, block, 0, stream, q);
    else if (q.T4 == 8) hipLaunchKernelGGL(qtlmv_scan_kernel<8>, grid, block, 0, stream, q);
    else hipLaunchKernelGGL(qtlmv_scan_kernel<16>, grid, block, 0, stream, q);
}

// perm_max[p][c] = the maximum over the chromosome's tiles, in ascending order (one thread per chromosome and group)
__global__ __launch_bounds__(64) void qtlmv_finish_kernel(QtlMvParams q)
{
    const int gl = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (gl >= q.gn) return;
    const int g = q.g0 + gl;
    if (g == 0) return;
    double v = 0.0;
    for (int t = q.tile_start[c]; t < q.tile_start[c + 1]; t++) v = fmax(v, q.tilemax[(size_t)t * q.gstride + gl]);
    q.pmax[(size_t)(g - 1) * q.C + c] = v;
}
void launch_qtlmv_finish(const QtlMvParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlmv_finish_kernel, dim3((q.gn + 63) / 64, q.C), dim3(64), 0, stream, q);
}

} // namespace cnf2
