// cnf2_kinship_kernels.hip -- the kernels of cnf2_kinship_sums (include/cnf2hip.h): sum[i][j] = sum_m a_i(m) a_j(m) over the
// markers of a chromosome range, a = origin[3] - origin[0], on the f64 matrix cores.
//
//   kin_pack_kernel    the image a[m_pad][n_pad], marker-major and zero-padded, from the origin rows (a transpose through LDS)
//   kin_syrk_kernel    the product: a 128 x 128 output tile per block, on or below the diagonal, fed through LDS panels
//   kin_finish_kernel  where the marker range is split: the chunks' partial sums added in ascending order
//
// Read in place, a wave would load 32-byte origin rows to use 8 bytes of each and reach about 2 flop per byte.  The image
// costs one pass over the range's rows and makes every later load a contiguous run of individuals at one marker: a block
// copies two panels of KIN_KC markers x 128 individuals into LDS (16 flop per byte of global traffic) and its four waves
// read their operands from there.  The image is padded with zeros to whole tiles and panels, so no load needs a clamp and
// none leaves the image; the outputs are masked.
// No kernel adds with atomics, the markers are summed in ascending order, and a mirrored tile is written from the
// accumulator that holds the tile itself: sum[i][j] and sum[j][i] are the same bits, and a call gives the same bits every
// time (the split of the range: cnf2_kinship.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_kinship.h"

namespace cnf2 {

typedef double kd2 __attribute__((ext_vector_type(2)));
typedef double kd4 __attribute__((ext_vector_type(4)));

// a panel's row stride in doubles: 128 individuals and 16 more, so that the rows k and k + 1 that one half of a wave reads
// together start 128 bytes apart modulo the 256 bytes of the banks
constexpr int KIN_LD = KIN_TILE + 16;

// 32 markers x 32 individuals per block: read along the markers (consecutive 32-byte rows), written along the individuals
__global__ __launch_bounds__(256) void kin_pack_kernel(KinParams q)
{
    __shared__ double t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = blockIdx.y * 32 + ty + 8 * r, m = blockIdx.x * 32 + tx;
        double    v = 0.0;
        if (i < q.n && m < q.n_mark) {
            const double* p = q.origin + ((size_t)i * q.M + q.m_lo + m) * 4;
            v = p[3] - p[0];
        }
        t[ty + 8 * r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int m = blockIdx.x * 32 + ty + 8 * r, i = blockIdx.y * 32 + tx;
        if (m < q.m_pad) q.image[(size_t)m * q.n_pad + i] = t[tx][ty + 8 * r];
    }
}
void launch_kin_pack(const KinParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(kin_pack_kernel, dim3((q.m_pad + 31) / 32, q.n_pad / 32), dim3(256), 0, stream, q);
}

// Block (bi, bj), bj <= bi, sums the image rows [k_lo + z k_len, ... + k_len) for the individuals 128 bi .. and 128 bj ..;
// wave w owns the 64 x 64 quarter (w >> 1, w & 1) as 4 x 4 results of v_mfma_f64_16x16x4_f64 (operand and result layout:
// qtl_scan_kernel in cnf2_qtl_kernels.hip).  Per panel of 16 markers every thread copies eight pairs of doubles -- wave w the
// image rows w, w + 4, .. of both panels, 1 KiB contiguous each -- which are requested a panel ahead and held in registers
// while the current panel is multiplied.  A diagonal block computes all four quarters: (i, j) and (j, i) are then the same
// products added in the same order.
__global__ __launch_bounds__(256, 2) void kin_syrk_kernel(KinParams q)
{
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    __shared__ double pI[KIN_KC][KIN_LD], pJ[KIN_KC][KIN_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w   = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = w >> 1, wj = w & 1, oi = lane & 15, ok = lane >> 4;
    const int k_begin = q.k_lo + (int)blockIdx.z * q.k_len;
    const int k_end   = min(k_begin + q.k_len, q.m_pad);
    const double* gI = q.image + (size_t)bi * KIN_TILE + 2 * lane;
    const double* gJ = q.image + (size_t)bj * KIN_TILE + 2 * lane;
    const size_t  ld = (size_t)q.n_pad;

    kd4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = kd4{0.0, 0.0, 0.0, 0.0};

    kd2 rI[4], rJ[4];
    if (k_begin < k_end) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
            rI[p] = *(const kd2*)(gI + (size_t)(k_begin + w + 4 * p) * ld);
            rJ[p] = *(const kd2*)(gJ + (size_t)(k_begin + w + 4 * p) * ld);
        }
    }
#pragma unroll 1
    for (int k0 = k_begin; k0 < k_end; k0 += KIN_KC) {
        __syncthreads();                               // the panel of the step before has been read
#pragma unroll
        for (int p = 0; p < 4; p++) {
            *(kd2*)&pI[w + 4 * p][2 * lane] = rI[p];
            *(kd2*)&pJ[w + 4 * p][2 * lane] = rJ[p];
        }
        __syncthreads();
        if (k0 + KIN_KC < k_end) {
#pragma unroll
            for (int p = 0; p < 4; p++) {
                rI[p] = *(const kd2*)(gI + (size_t)(k0 + KIN_KC + w + 4 * p) * ld);
                rJ[p] = *(const kd2*)(gJ + (size_t)(k0 + KIN_KC + w + 4 * p) * ld);
            }
        }
#pragma unroll
        for (int kk = 0; kk < KIN_KC / 4; kk++) {
            double aI[4], aJ[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                aI[t] = pI[kk * 4 + ok][wi * 64 + t * 16 + oi];
                aJ[t] = pJ[kk * 4 + ok][wj * 64 + t * 16 + oi];
            }
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI[a], aJ[b], acc[a][b], 0, 0, 0);
        }
    }

    const size_t n   = (size_t)q.n;
    double*      out = q.out + (size_t)blockIdx.z * n * n;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const size_t i = (size_t)bi * KIN_TILE + wi * 64 + a * 16 + ok + 4 * reg;
                const size_t j = (size_t)bj * KIN_TILE + wj * 64 + b * 16 + oi;
                if (i < n && j < n) {
                    out[i * n + j] = acc[a][b][reg];
                    if (bi != bj) out[j * n + i] = acc[a][b][reg];
                }
            }
}
void launch_kin_syrk(const KinParams& q, int chunks, hipStream_t stream)
{
    const int nt = q.n_pad / KIN_TILE;
    hipLaunchKernelGGL(kin_syrk_kernel, dim3(nt, nt, chunks), dim3(256), 0, stream, q);
}

// sum[e] = (first ? 0 : sum[e]) + out[0][e] + out[1][e] + ..: ascending chunks, whatever number of them a round held
__global__ __launch_bounds__(256) void kin_finish_kernel(KinParams q)
{
    const size_t nn = (size_t)q.n * q.n;
    const size_t e  = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nn) return;
    double v = q.first ? 0.0 : q.sum[e];
    for (int g = 0; g < q.parts; g++) v += q.out[(size_t)g * nn + e];
    q.sum[e] = v;
}
void launch_kin_finish(const KinParams& q, hipStream_t stream)
{
    const size_t nn = (size_t)q.n * q.n;
    hipLaunchKernelGGL(kin_finish_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, stream, q);
}

} // namespace cnf2
