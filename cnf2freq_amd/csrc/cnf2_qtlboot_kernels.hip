// cnf2_qtlboot_kernels.hip -- the kernels of the bootstrap QTL scan (cnf2_qtl_scan_boot, include/cnf2hip.h): the Haley-Knott
// scan of cnf2_qtl_kernels.hip on resampled individuals.  A replicate changes the design, not the columns: every sum of the
// model carries the replicate's weights w_i = count[b][i] c_i.  The model is cnf2_qtlboot.h's, the cell algebra cnf2_qtl.h's;
// this file forms the sums.
//
//   qtlboot_mask_kernel    per scanned chromosome: c_i
//   qtlboot_gather_kernel  per replicate tile: the weight image W[n][bstride] (doubles, individual-major; 0 past the tile)
//   qtlboot_design_kernel  per (replicate, chromosome): n_bc, S11 = X0'WX0 and its Cholesky factor, usable or not
//   qtlboot_null_kernel    per (replicate, chromosome, trait): b0 = X0'Wy, RSS0
//   qtlboot_scan_kernel    the hot path: every weighted sum of a (replicate, marker) cell on the f64 matrix cores, the cell
//                          and the (maximum, marker) of a tile in registers
//   qtlboot_finish_kernel  per (replicate, trait, chromosome): the (maximum, marker) over the chromosome's tiles
//
// No kernel adds with atomics and every sum runs over the individuals in ascending order: a call gives the same bits every
// time, whatever the replicate tiling and the trait chunking.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "cnf2_qtlboot.h"

namespace cnf2 {

typedef double bd2 __attribute__((ext_vector_type(2)));
typedef double bd4 __attribute__((ext_vector_type(4)));

constexpr int QTLBOOT_WAVES = 4;      // waves per block: the same 16 markers, consecutive groups of 16 replicates
constexpr int QTLBOOT_TC    = 4;      // traits per chunk of the hot kernel (one for a single trait)
constexpr int QTLBOOT_AHEAD = 8;      // individuals whose weights the per-replicate kernels request together

// column k of X0 for individual i (column 0 is the intercept)
__device__ __forceinline__ double qtlboot_x(const QtlBootParams& q, int i, int k) { return k == 0 ? 1.0 : q.cov[(size_t)i * q.K + (k - 1)]; }

// one thread per (individual, scanned chromosome)
__global__ __launch_bounds__(256) void qtlboot_mask_kernel(QtlBootParams q)
{
    const int i = blockIdx.x * 256 + threadIdx.x, cc = blockIdx.y;
    if (i >= q.n) return;
    const double* o  = q.origin + ((size_t)i * q.M + q.first[cc]) * 4;
    const bool    on = q.use[i] && (o[0] != 0.0 || o[1] != 0.0 || o[2] != 0.0 || o[3] != 0.0);
    q.cmask[(size_t)cc * q.n + i] = on ? 1 : 0;
}
void launch_qtlboot_mask(const QtlBootParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlboot_mask_kernel, dim3((q.n + 255) / 256, q.nc), dim3(256), 0, stream, q);
}

// W[i][bb] = count[b0 + bb][i] for bb < bn, 0 up to the stride: the hot kernel's replicate operand needs no mask
__global__ __launch_bounds__(256) void qtlboot_gather_kernel(QtlBootParams q)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)q.n * q.bstride) return;
    const int i = (int)(e / q.bstride), bb = (int)(e % q.bstride);
    q.W[e] = bb < q.bn ? (double)q.count[(size_t)(q.b0 + bb) * q.n + i] : 0.0;
}
void launch_qtlboot_gather(const QtlBootParams& q, hipStream_t stream)
{
    const size_t e = (size_t)q.n * q.bstride;
    hipLaunchKernelGGL(qtlboot_gather_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, stream, q);
}

// One thread per (replicate, chromosome); neighbouring threads read neighbouring weights.  The sums stay in registers, the
// factor is taken in place in the record.  A covariate that is constant over the drawn individuals: unusable (cnf2_qtlboot.h).
__global__ __launch_bounds__(64) void qtlboot_design_kernel(QtlBootParams q)
{
    const int bb = blockIdx.x * 64 + threadIdx.x, cc = blockIdx.y;
    if (bb >= q.bn) return;
    const uint8_t* cm = q.cmask + (size_t)cc * q.n;
    double         S[QTL_NX * (QTL_NX + 1) / 2], first[QTL_NX];
    bool           varies[QTL_NX], any = false;
    long long      n_bc = 0;
#pragma unroll
    for (int e = 0; e < QTL_NX * (QTL_NX + 1) / 2; e++) S[e] = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) first[k] = 0.0, varies[k] = false;
    // (QTLBOOT_AHEAD weights are requested together; the covariates and the mask are wave-uniform loads)
    for (int i0 = 0; i0 < q.n; i0 += QTLBOOT_AHEAD) {
        double wa[QTLBOOT_AHEAD];
#pragma unroll
        for (int u = 0; u < QTLBOOT_AHEAD; u++) wa[u] = q.W[(size_t)(i0 + u < q.n ? i0 + u : q.n - 1) * q.bstride + bb];
#pragma unroll
        for (int u = 0; u < QTLBOOT_AHEAD; u++) {
            const int i = i0 + u;
            if (i >= q.n || !cm[i]) continue;
            const double w = wa[u];
            double       x[QTL_NX];
#pragma unroll
            for (int k = 0; k < QTL_NX; k++) x[k] = k < q.nx ? qtlboot_x(q, i, k) : 0.0;
            n_bc += (long long)w;
#pragma unroll
            for (int j = 0; j < QTL_NX; j++)
#pragma unroll
                for (int k = 0; k <= j; k++)
                    if (j < q.nx) S[j * (j + 1) / 2 + k] += w * x[j] * x[k];
            if (w > 0.0) {
#pragma unroll
                for (int k = 1; k < QTL_NX; k++) {
                    if (!any) first[k] = x[k];
                    varies[k] = varies[k] || x[k] != first[k];
                }
                any = true;
            }
        }
    }
    bool ok = n_bc >= q.K + 4 && n_bc <= INT_MAX;
#pragma unroll
    for (int k = 1; k < QTL_NX; k++)
        if (k < q.nx) ok = ok && varies[k];
    double* rec = q.rec + ((size_t)bb * q.nc + cc) * qtlboot_rec_doubles(q.T);
#pragma unroll
    for (int j = 0; j < QTL_NX; j++)
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) rec[j * QTL_NX + k] = k <= j ? S[j * (j + 1) / 2 + k] : 0.0;
    ok                       = qtl_cholesky(rec, q.nx) && ok;
    rec[QTL_NX * QTL_NX]     = ok ? 1.0 : 0.0;
    q.n_boot[(size_t)(q.b0 + bb) * q.nc + cc] = (int32_t)(n_bc <= INT_MAX ? n_bc : INT_MAX);
}
void launch_qtlboot_design(const QtlBootParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlboot_design_kernel, dim3((q.bn + 63) / 64, q.nc), dim3(64), 0, stream, q);
}

// one thread per (replicate, chromosome, trait): b0 = X0'Wy and y'Wy over the individuals in ascending order, RSS0
__global__ __launch_bounds__(64) void qtlboot_null_kernel(QtlBootParams q)
{
    const int bb = blockIdx.x * 64 + threadIdx.x, cc = blockIdx.y, t = blockIdx.z;
    if (bb >= q.bn) return;
    const uint8_t* cm = q.cmask + (size_t)cc * q.n;
    double         b[QTL_NX], z[QTL_NX], yy = 0.0;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) b[k] = 0.0;
    for (int i0 = 0; i0 < q.n; i0 += QTLBOOT_AHEAD) {
        double wa[QTLBOOT_AHEAD];
#pragma unroll
        for (int u = 0; u < QTLBOOT_AHEAD; u++) wa[u] = q.W[(size_t)(i0 + u < q.n ? i0 + u : q.n - 1) * q.bstride + bb];
#pragma unroll
        for (int u = 0; u < QTLBOOT_AHEAD; u++) {
            const int i = i0 + u;
            if (i >= q.n || !cm[i]) continue;
            const double w = wa[u], y = q.pheno[(size_t)i * q.T + t];
#pragma unroll
            for (int k = 0; k < QTL_NX; k++)
                if (k < q.nx) b[k] += w * (qtlboot_x(q, i, k) * y);
            yy += w * (y * y);
        }
    }
    double*       rec  = q.rec + ((size_t)bb * q.nc + cc) * qtlboot_rec_doubles(q.T);
    const double* L    = rec;
    double        rss0 = 0.0;
    if (L[QTL_NX * QTL_NX] != 0.0) {
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) z[k] = b[k];
        qtl_chol_solve(L, q.nx, z);
        double e = 0.0;
#pragma unroll
        for (int k = 0; k < QTL_NX; k++)
            if (k < q.nx) e += b[k] * z[k];
        rss0 = yy - e;
    }
    double* out = rec + QTL_CHOL + (size_t)t * QTLBOOT_TRAIT;
#pragma unroll
    for (int k = 0; k < QTL_NX; k++) out[k] = k < q.nx ? b[k] : 0.0;
    out[QTL_NX] = rss0;
}
void launch_qtlboot_null(const QtlBootParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlboot_null_kernel, dim3((q.bn + 63) / 64, q.nc, q.T), dim3(64), 0, stream, q);
}

// The product.  qtl_scan_kernel's shape with the weight image in place of the column image: a wave owns 16 markers of one
// chromosome (a tile never straddles a chromosome start) x 16 replicates and walks every individual in ascending order, four
// per v_mfma_f64_16x16x4_f64.  The replicates are the rows of the result and the markers its columns.  The replicate operand
// is 16 consecutive doubles of the image's row.  The marker operand is formed in registers: lane (marker, k) reads the 32
// bytes of individual i0 + k at its marker, forms a, d and the c-mask, and issues one MFMA per feature of the weighted design
// -- a a, a d, d d, a x_k, d x_k, a y_t, d y_t: 3 + 2 nx + 2 tn accumulators, 1 + nx + tn in the additive model (ADD), whose
// d is never formed.  NXMAX and TC bound nx and tn for the registers; the features past q.nx and q.tn are skipped by
// wave-uniform branches.  Neither operand goes through LDS.  Individuals past n and markers past the tile's end are clamped
// addresses and zero operands; replicates past the tile are zeros of the image: no load leaves its array.
// Every feature of a (replicate, marker) cell ends in one register of one lane, so the epilogue stays there: the replicate's
// factor, b0 and RSS0 from its record, qtl_marker_record and qtl_cell (cnf2_qtl.h), the profile if it is asked for, and a
// (value, marker) butterfly over the 16 marker lanes in which the lower marker wins among equal values.
template <int NXMAX, bool ADD, int TC>
__global__ __launch_bounds__(64 * QTLBOOT_WAVES) void qtlboot_scan_kernel(QtlBootParams q)
{
    constexpr int KU = NXMAX > 2 ? 2 : 4;      // k-steps of 4 individuals requested together
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x;
    const int cc = q.tiles[tile * 4], m0 = q.tiles[tile * 4 + 1], len = q.tiles[tile * 4 + 2];
    const int rb = (blockIdx.y * QTLBOOT_WAVES + wib) * 16;
    if (rb >= q.bn) return;
    const int  oi = lane & 15, ok = lane >> 4;
    const bool mval = oi < len;
    const int  m = m0 + (mval ? oi : 0);
    const int  n = q.n, nx = q.nx < NXMAX ? q.nx : NXMAX, tn = q.tn < TC ? q.tn : TC;
    const double*  orow = q.origin + (size_t)m * 4;
    const size_t   os   = (size_t)q.M * 4;
    const uint8_t* cm   = q.cmask + (size_t)cc * n;
    const double*  wcol = q.W + rb + oi;                       // rb + oi < bstride, a multiple of 16
    bd4 accAA, accAD, accDD, accAX[NXMAX], accDX[NXMAX], accAY[TC], accDY[TC];
    const bd4 zero = {0.0, 0.0, 0.0, 0.0};
    accAA = accAD = accDD = zero;
#pragma unroll
    for (int k = 0; k < NXMAX; k++) accAX[k] = accDX[k] = zero;
#pragma unroll
    for (int t = 0; t < TC; t++) accAY[t] = accDY[t] = zero;

#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += 4 * KU) {
        bd2    o01[KU], o23[KU];
        double w[KU], x[KU][NXMAX], y[KU][TC];
        bool   on[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int  i  = i0 + 4 * u + ok;
            const bool in = i < n;
            const int  ic = in ? i : n - 1;
            const double* p = orow + (size_t)ic * os;
            o01[u] = *(const bd2*)p;
            o23[u] = *(const bd2*)(p + 2);
            on[u]  = in && mval && cm[ic] != 0;
            w[u]   = wcol[(size_t)ic * q.bstride];
            if (!in) w[u] = 0.0;
#pragma unroll
            for (int k = 1; k < NXMAX; k++) x[u][k] = k < nx ? q.cov[(size_t)ic * q.K + (k - 1)] : 0.0;
#pragma unroll
            for (int t = 0; t < TC; t++) y[u][t] = t < tn ? q.pheno[(size_t)ic * q.T + q.t0 + t] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < KU; u++) {
            // (an unused individual's phenotype and covariates may be NaN: every feature of a masked row is 0, not 0 * y)
            const double a = on[u] ? o23[u].y - o01[u].x : 0.0;
            const double d = (on[u] && !ADD) ? o01[u].y + o23[u].x : 0.0;
            accAA = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], a * a, accAA, 0, 0, 0);
            accAX[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], a, accAX[0], 0, 0, 0);
            if (!ADD) {
                accAD = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], a * d, accAD, 0, 0, 0);
                accDD = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], d * d, accDD, 0, 0, 0);
                accDX[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], d, accDX[0], 0, 0, 0);
            }
#pragma unroll
            for (int k = 1; k < NXMAX; k++)
                if (k < nx) {
                    const double xv = on[u] ? x[u][k] : 0.0;
                    accAX[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], a * xv, accAX[k], 0, 0, 0);
                    if (!ADD) accDX[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], d * xv, accDX[k], 0, 0, 0);
                }
#pragma unroll
            for (int t = 0; t < TC; t++)
                if (t < tn) {
                    const double yv = on[u] ? y[u][t] : 0.0;
                    accAY[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], a * yv, accAY[t], 0, 0, 0);
                    if (!ADD) accDY[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], d * yv, accDY[t], 0, 0, 0);
                }
        }
    }

    const size_t recd = qtlboot_rec_doubles(q.T);
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int     bb     = rb + ok + 4 * reg;
        const bool    bval   = bb < q.bn;
        const int     bc     = bval ? bb : 0;
        const double* L      = q.rec + ((size_t)bc * q.nc + cc) * recd;
        const bool    usable = L[QTL_NX * QTL_NX] != 0.0;
        const int     n_bc   = q.n_boot[(size_t)(q.b0 + bc) * q.nc + cc];
        double        sa[QTL_NX], sd[QTL_NX], mk[QTL_MK];
#pragma unroll
        for (int k = 0; k < QTL_NX; k++) sa[k] = sd[k] = 0.0;
#pragma unroll
        for (int k = 0; k < NXMAX; k++) {
            sa[k] = k < nx ? accAX[k][reg] : 0.0;
            sd[k] = (k < nx && !ADD) ? accDX[k][reg] : 0.0;
        }
        qtl_marker_record(L, nx, usable, sa, sd, accAA[reg], ADD ? 0.0 : accAD[reg], ADD ? 0.0 : accDD[reg], ADD, mk);
#pragma unroll
        for (int t = 0; t < TC; t++)
            if (t < tn) {
                const int     gt  = q.t0 + t;
                const double* nq  = L + QTL_CHOL + (size_t)gt * QTLBOOT_TRAIT;
                double        gba = 0.0, gbd = 0.0;
#pragma unroll
                for (int k = 0; k < NXMAX; k++)
                    if (k < nx) {
                        const double b = nq[k];
                        gba += mk[k] * b;
                        gbd += mk[QTL_NX + k] * b;
                    }
                const QtlCell cell = qtl_cell(accAY[t][reg] - gba, ADD ? 0.0 : accDY[t][reg] - gbd, mk[QTL_PA], mk[QTL_L], mk[QTL_PD],
                                              nq[QTL_NX], n_bc, usable);
                const bool    cval = bval && mval;
                if (cval && q.boot_lod) q.boot_lod[((size_t)(q.b0 + bb) * q.T + gt) * q.n_mark + (m - q.m_lo)] = cell.lod;
                double v   = cval ? cell.lod : -1.0;         // a LOD is never negative: -1 loses against every cell
                int    arg = cval ? m : INT_MAX;
#pragma unroll
                for (int s = 1; s < 16; s <<= 1) {
                    const double ov = __shfl_xor(v, s);
                    const int    oa = __shfl_xor(arg, s);
                    if (ov > v || (ov == v && oa < arg)) v = ov, arg = oa;
                }
                if (oi == 0 && bval) {
                    const size_t o = ((size_t)tile * q.bn + bb) * q.T + gt;
                    q.tilemax[o] = v;
                    q.tilearg[o] = arg;
                }
            }
    }
}

int qtlboot_trait_chunk(int T) { return T == 1 ? 1 : QTLBOOT_TC; }

template <int NXMAX, bool ADD, int TC>
static void qtlboot_scan_go(const QtlBootParams& q, hipStream_t stream)
{
    const int reps = 16 * QTLBOOT_WAVES;
    hipLaunchKernelGGL((qtlboot_scan_kernel<NXMAX, ADD, TC>), dim3(q.n_tiles, (q.bn + reps - 1) / reps), dim3(64 * QTLBOOT_WAVES), 0,
                       stream, q);
}
template <int NXMAX, bool ADD>
static void qtlboot_scan_tc(const QtlBootParams& q, hipStream_t stream)
{
    if (q.T == 1) qtlboot_scan_go<NXMAX, ADD, 1>(q, stream);
    else qtlboot_scan_go<NXMAX, ADD, QTLBOOT_TC>(q, stream);
}
// the instantiation by the width of X0 (up to one covariate, or up to QTL_MAXK), the model and the trait chunk
void launch_qtlboot_scan(const QtlBootParams& q, hipStream_t stream)
{
    if (q.nx <= 2) {
        if (q.additive) qtlboot_scan_tc<2, true>(q, stream);
        else qtlboot_scan_tc<2, false>(q, stream);
    } else {
        if (q.additive) qtlboot_scan_tc<QTL_NX, true>(q, stream);
        else qtlboot_scan_tc<QTL_NX, false>(q, stream);
    }
}

// boot_max / boot_arg: the chromosome's tiles in ascending order, a later tile wins only with a larger value (its markers are
// the higher ones); an unusable replicate reports 0 and -1 (one thread per replicate, trait and chromosome)
__global__ __launch_bounds__(64) void qtlboot_finish_kernel(QtlBootParams q)
{
    const int bb = blockIdx.x * 64 + threadIdx.x, cc = blockIdx.y, t = blockIdx.z;
    if (bb >= q.bn) return;
    const double* rec = q.rec + ((size_t)bb * q.nc + cc) * qtlboot_rec_doubles(q.T);
    double        v   = 0.0;
    int           arg = -1;
    if (rec[QTL_NX * QTL_NX] != 0.0) {
        v = -1.0;
        for (int tl = q.tile_start[cc]; tl < q.tile_start[cc + 1]; tl++) {
            const size_t o = ((size_t)tl * q.bn + bb) * q.T + t;
            if (q.tilemax[o] > v) v = q.tilemax[o], arg = q.tilearg[o];
        }
    }
    const size_t o = ((size_t)(q.b0 + bb) * q.T + t) * q.nc + cc;
    q.boot_max[o] = v;
    q.boot_arg[o] = arg;
}
void launch_qtlboot_finish(const QtlBootParams& q, hipStream_t stream)
{
    hipLaunchKernelGGL(qtlboot_finish_kernel, dim3((q.bn + 63) / 64, q.nc, q.T), dim3(64), 0, stream, q);
}

} // namespace cnf2
