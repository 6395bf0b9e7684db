// cnf2_kernels.hip -- gfx950 kernels of the cnF2freq forward-backward sweep.
//
// One wavefront = one job (analysed individual x chromosome), all 8 shift modes at once:
//     lane = chain<<3 | lo      chain = shift mode s (cnF2freq.cpp:5375), lo = state bits 0-2
//     register j = 0..7         state bits 3-5            state g = j*8 + lo
// so the 8 x 64 state values of the 8 concurrent HMM chains sit in 8 VGPR pairs per lane.
//   * emission (adjustprobs + trackpossible, cnF2freq.cpp:1579-1670, 1075-1359): the same 64 lanes
//     first act as the 64 entries of the rank-2 emission table of this (individual, marker)
//     (cnf2_emission.h / cnf2_lane.h), hand them over through 512 B of LDS, then every lane
//     forms e(g) = sum_f c_f A_f[lo] B_f[j] for its 8 states;
//   * transition (realanalyze, cnF2freq.cpp:2273-2367): the 64x64 XOR-indexed matrix is the
//     6-fold Kronecker product of [[1-r, r],[r, 1-r]]; bits 3-5 are register pairs, bits 0-2
//     are DPP lane exchanges inside a row -- no LDS, no MFMA;
//   * scaling (cnF2freq.cpp:1656-1669): per-chain sum by 3 DPP steps; the 8 chains' reciprocals
//     are computed by one instruction stream (8 lanes each); log scales are carried as
//     mantissa x 2^exponent and only turned into a logarithm once per chromosome.
// The forward pass spills alpha-minus (before emission) in register-major order, 8 coalesced
// 512 B stores per marker; the backward pass of the same wave reads it back, forms the per-locus
// allele-2 dosage row (genotypereporter, cnF2freq.cpp:3532-3538, closed form of the fan-out of
// cnF2freq.cpp:5416-5553) and carries beta.
#include <hip/hip_runtime.h>

#include <string.h>
#include <type_traits>

#include "cnf2_device.h"
#include "cnf2_lane.h"
#include "cnf2_emtab.h"
#include "cnf2_accum.h"
#include "cnf2_acctab.h"
#include "cnf2_accpath.h"
#include "cnf2_variance.h"

namespace cnf2 {

// ------------------------------------------------------------------ lane exchange helpers
// full-wave DPP move without a tied "old" operand (every lane is written, so no copy is needed)
template <int CTRL>
__device__ __forceinline__ double dpp_mov_all(double v)
{
    int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
    int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// lane exchange through the LDS crossbar (no LDS memory is touched): BitMode swizzle, xor mask K
template <int K>
__device__ __forceinline__ double swizzle_xor(double v)
{
    int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), (K << 10) | 0x1F);
    int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), (K << 10) | 0x1F);
    return __hiloint2double(hi, lo);
}

// value of lane (id ^ 1), (id ^ 2), (id ^ 4)
__device__ __forceinline__ double lane_xor1(double v) { return dpp_mov_all<0xB1>(v); } // quad_perm [1,0,3,2]
__device__ __forceinline__ double lane_xor2(double v) { return dpp_mov_all<0x4E>(v); } // quad_perm [2,3,0,1]
// xor 4 has no single DPP form on gfx950 (row_shl/row_shr with bank masks costs two tied moves per
// dword plus hazard nops); the LDS crossbar does it in one ds_swizzle per dword and runs beside the VALU
__device__ __forceinline__ double lane_xor4(double v) { return swizzle_xor<4>(v); }
// State bit 2 does not have to live in lane bit 2.  With lane(lo) = b0 ^ 2 b1 ^ 7 b2 (an invertible
// GF(2) map of the three low state bits) flipping b2 is "lane i <-> lane 7-i" inside each group of 8 =
// DPP row_half_mirror, a plain VALU move like the two quad_perm stages: no trip through the LDS pipe.
// CNF2_XCHG (A/B timing): 0 = all three lane stages on DPP; 1 = bit 2, 2 = bits 1 and 2 through the LDS
// crossbar (ds_swizzle: fewer VALU slots, longer latency).
#ifndef CNF2_XCHG
#define CNF2_XCHG 0
#endif
// (state_lo, the lane's low state bits under that map: cnf2_lane.h)
#if CNF2_XCHG == 0
__device__ __forceinline__ double lane_flip_b1(double v) { return lane_xor2(v); }
__device__ __forceinline__ double lane_flip_b2(double v) { return dpp_mov_all<0x141>(v); }
#elif CNF2_XCHG == 1
__device__ __forceinline__ double lane_flip_b1(double v) { return lane_xor2(v); }
__device__ __forceinline__ double lane_flip_b2(double v) { return swizzle_xor<7>(v); }
#else
__device__ __forceinline__ double lane_flip_b1(double v) { return swizzle_xor<2>(v); }
__device__ __forceinline__ double lane_flip_b2(double v) { return swizzle_xor<7>(v); }
#endif
__device__ __forceinline__ double lane_xor8(double v) { return dpp_mov_all<0x128>(v); } // row_ror:8
__device__ __forceinline__ double lane_xor16(double v) { return swizzle_xor<16>(v); }
// lane id of a full wavefront, recomputed where it is asked for (volatile: not hoisted out of a job loop, where it would
// occupy a register -- or a scratch slot -- for the whole kernel)
__device__ __forceinline__ int fresh_lane()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
__device__ __forceinline__ double lane_xor32(double v)
{
    const int a  = (fresh_lane() ^ 32) << 2;
    const int lo = __builtin_amdgcn_ds_bpermute(a, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(a, __double2hiint(v));
    return __hiloint2double(hi, lo);
}

// sum over the 8 lanes of a chain (lanes differing in bits 0-2); result in every lane.
// Third step pairs lane i with lane 7-i of its group of 8 (row_half_mirror): after the two quad
// steps every lane of a quad holds the quad total, so any quad<->quad pairing finishes the sum,
// and this one is a plain DPP move (no trip through the LDS crossbar on the critical path).
__device__ __forceinline__ double chain_sum(double v)
{
    v += lane_xor1(v);
    v += lane_xor2(v);
    v += dpp_mov_all<0x141>(v);
    return v;
}
// sum over the 8 chains of values that are already uniform inside each chain
__device__ __forceinline__ double across_chains_sum(double v)
{
    v += lane_xor8(v);
    v += lane_xor16(v);
    v += lane_xor32(v);
    return v;
}
__device__ __forceinline__ double across_chains_max(double v)
{
    v = fmax(v, lane_xor8(v));
    v = fmax(v, lane_xor16(v));
    v = fmax(v, lane_xor32(v));
    return v;
}

// ------------------------------------------------------------------ transition
// One Kronecker factor on a register pair / on a lane pair: x' = (1-r) x + r partner
// (recombprec of cnF2freq.cpp:2329-2340 factorised over the 6 state bits).
__device__ __forceinline__ void transition(double (&a)[8], double r0, double r1)
{
    // bit t uses genrec[TYPEGENS[t]], TYPEGENS = {1,0,0,1,0,0} (settings.h:23)
    const double k0 = 1.0 - r0, k1 = 1.0 - r1;
    // bits 0..2: lanes.  All partner values of a stage are requested before any is used, so the
    // eight exchanges overlap (the xor-4 stage goes through the LDS crossbar: one latency, not eight).
    double q[8];
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = lane_xor1(a[j]);
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = k1 * a[j] + r1 * q[j];
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = lane_flip_b1(a[j]);
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = k0 * a[j] + r0 * q[j];
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = lane_flip_b2(a[j]);
#if CNF2_XCHG >= 1
    __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = k0 * a[j] + r0 * q[j];
    // bits 3..5: registers.  The multiply-add is written out, the same form for both elements of a pair: left to the
    // compiler, the two were fused differently (fma(k, x, r y) for one, fma(r, x, k y) for the other), so that two states
    // holding the same bits -- the grandparental bits of a cross of inbred lines -- came out an ulp apart in the
    // reference-layout store (tests/test_gpu_uniform_states.py: the premise)
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        double x = a[j], y = a[j + 1];
        a[j]     = fma(r1, y, k1 * x);
        a[j + 1] = fma(r1, x, k1 * y);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j & 2) continue;
        double x = a[j], y = a[j + 2];
        a[j]     = fma(r0, y, k0 * x);
        a[j + 2] = fma(r0, x, k0 * y);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double x = a[j], y = a[j + 4];
        a[j]     = fma(r0, y, k0 * x);
        a[j + 4] = fma(r0, x, k0 * y);
    }
}

// Same operator up to a per-gap constant: with t = r / (1 - r) every butterfly is x' = x + t * partner
// and the dropped factor (1-r0)^4 (1-r1)^2 is a scalar common to all states and shift modes, so it
// only moves the normaliser of the step.  The host adds its logarithm, summed over the chromosome,
// to the reported log-likelihoods; ratios (the per-locus rows) never see it.  One fused multiply-add
// per element and stage instead of a multiply and an FMA.
__device__ __forceinline__ void transition_scaled(double (&a)[8], double t0, double t1)
{
    double q[8];
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = lane_xor1(a[j]);
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = fma(t1, q[j], a[j]);
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = lane_flip_b1(a[j]);
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = fma(t0, q[j], a[j]);
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = lane_flip_b2(a[j]);
#if CNF2_XCHG >= 1
    __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = fma(t0, q[j], a[j]);
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const double x = a[j], y = a[j + 1];
        a[j]     = fma(t1, y, x);
        a[j + 1] = fma(t1, x, y);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j & 2) continue;
        const double x = a[j], y = a[j + 2];
        a[j]     = fma(t0, y, x);
        a[j + 2] = fma(t0, x, y);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const double x = a[j], y = a[j + 4];
        a[j]     = fma(t0, y, x);
        a[j + 4] = fma(t0, x, y);
    }
}

// transition_scaled for a vector that does not depend on the four grandparental state bits (the t0 stages: lane stages b1
// and b2, register-index bits 1 and 2 -- a window with slots_uniform, cnf2_emission.h): the partner such a stage would fetch
// is the lane's own value, so the stage is a[j] = fma(t0, a[j], a[j]) -- the same FMA on the same operands, the same bits,
// and no exchange.  N = 8: all eight registers are carried (they hold two distinct numbers); N = 2: only register bit 0,
// and the two register stages on the uniform bits become the same self-FMA.
template <int N>
__device__ __forceinline__ void transition_uniform(double (&a)[N], double t0, double t1)
{
    static_assert(N == 8 || N == 2, "all eight registers of a lane, or the two that differ");
    double q[N];
#pragma unroll
    for (int j = 0; j < N; j++) q[j] = lane_xor1(a[j]);
#pragma unroll
    for (int j = 0; j < N; j++) a[j] = fma(t1, q[j], a[j]);
#pragma unroll
    for (int j = 0; j < N; j++) a[j] = fma(t0, a[j], a[j]);
#pragma unroll
    for (int j = 0; j < N; j++) a[j] = fma(t0, a[j], a[j]);
#pragma unroll
    for (int j = 0; j < N; j += 2) {
        const double x = a[j], y = a[j + 1];
        a[j]     = fma(t1, y, x);
        a[j + 1] = fma(t1, x, y);
    }
    if constexpr (N == 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (j & 2) continue;
            const double x = a[j], y = a[j + 2];
            a[j]     = fma(t0, y, x);
            a[j + 2] = fma(t0, x, y);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double x = a[j], y = a[j + 4];
            a[j]     = fma(t0, y, x);
            a[j + 4] = fma(t0, x, y);
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) a[j] = fma(t0, a[j], a[j]);
#pragma unroll
        for (int j = 0; j < N; j++) a[j] = fma(t0, a[j], a[j]);
    }
}

// The three butterflies on the state bits that currently sit in the registers (bit 0 of the triple belongs to a
// parent's meiosis: genrec[1], the other two to grandparental ones: genrec[0]; settings.h:23).
__device__ __forceinline__ void register_stages(double (&a)[8], double t0, double t1)
{
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const double x = a[j], y = a[j + 1];
        a[j]     = fma(t1, y, x);
        a[j + 1] = fma(t1, x, y);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j & 2) continue;
        const double x = a[j], y = a[j + 2];
        a[j]     = fma(t0, y, x);
        a[j + 2] = fma(t0, x, y);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const double x = a[j], y = a[j + 4];
        a[j]     = fma(t0, y, x);
        a[j + 4] = fma(t0, x, y);
    }
}

// Transposing form of transition_scaled (CNF2_XPOSE variant of the fast kernel): instead of exchanging the three
// lane-held state bits by DPP (48 v_mov_dpp per transition, a quarter of the kernel's VALU work), the wave swaps
// which triple of state bits sits in the lanes: register stages on the triple held in registers, an 8 x 8 transpose
// of every chain's (lane, register) block through LDS (8 ds_write_b64 + 8 ds_read_b64, no VALU slot), register
// stages on the other triple.  The layout therefore alternates from marker to marker: even local markers keep state
// bits 0-2 in the lanes (as the spill rows and the table reads of the DPP variant assume), odd ones bits 3-5.
// xb: this wave's 64 x XPOSE_RS doubles.  Row stride 9 spreads the eight chains over the LDS banks.
#define XPOSE_RS 9
__device__ __forceinline__ void transition_xpose(double (&a)[8], double t0, double t1, double* xb, int lane)
{
    register_stages(a, t0, t1);
    const int s8 = lane & 56, l = lane & 7;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // earlier reads of xb are done
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < 8; j++) xb[(s8 + j) * XPOSE_RS + l] = a[j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = xb[(s8 + l) * XPOSE_RS + j];
    register_stages(a, t0, t1);
}

// ------------------------------------------------------------------ per-job lane state
struct LaneCtx {
    LaneJob L;            // producer role
    int     row_root;
    bool    root_attop;
    int     s0, s1, s2;   // consumer role: bits of this lane's shift mode
    int     lo;
    bool    active;       // chain takes part (not masked by shiftignore / shiftend)
    int     n_combo;      // 1 << n_groups (1 with CNF2_NO_TIES)
};

__device__ __forceinline__ Slot load_slot(const KernelParams& p, int row, int m)
{
    size_t  i  = (size_t)row * p.n_markers + m;
    uint8_t ap = p.allele8[i];
    double2 s  = p.sure[i];
    return unpack_slot(ap, s.x, s.y, p.hw[i]);
}

// Producer half: this lane's table entry for marker m.
// Returns the unrestricted value; if WITH_CLASSES also the restricted value and its class-2
// part for tie combination `combo` (LineTerms kept by the caller).
__device__ __forceinline__ double produce_entry(const KernelParams& p, const LaneCtx& c, const Slot& root, int m,
                                                LineTerms* T)
{
    RootTerms R;
    root_terms(root, c.root_attop, c.L.f, &R);
    Slot par = load_slot(p, c.L.row_par, m);
    Slot tr  = load_slot(p, c.L.row_tr, m);
    Slot ot  = load_slot(p, c.L.row_ot, m);
    line_terms(c.L.cfg, par, tr, ot, c.L.P ? R.inmv1 : R.inmv0, c.L.P ? R.sv1 : R.sv0,
               c.L.P == 0 && R.inmv0 == 2, T);
    double tot = line_total(*T);
    if (c.root_attop) {
        // the root is the top of its single line (cnF2freq.cpp:1260-1271): tables are 1
        tot = 1.0;
    }
    return tot;
}

__device__ __forceinline__ void restricted_entry(const LaneCtx& c, const Slot& root, const LineTerms& T, int combo,
                                                 double* rtot, double* two)
{
    if (c.root_attop) {
        *rtot = 1.0;
        int mf = c.L.f ? root.a1 : root.a0;
        *two   = (c.L.P == 0 && mf == 2) ? 1.0 : 0.0;
        return;
    }
    line_restricted(c.L.cfg, T, tie_force(c.L.tie_par, combo), tie_force(c.L.tie_tr, combo),
                    tie_force(c.L.tie_ot, combo), rtot, two);
}

// Consumer half: root weights c_f(s0) of this lane's shift mode.
__device__ __forceinline__ void root_weights(const LaneCtx& c, const Slot& root, double* c0, double* c1)
{
    RootTerms R0, R1;
    root_terms(root, c.root_attop, 0, &R0);
    root_terms(root, c.root_attop, 1, &R1);
    *c0 = R0.cbase * phase_weight(root, 0 ^ c.s0);
    *c1 = R1.cbase * phase_weight(root, 1 ^ c.s0);
}

__device__ __forceinline__ void wave_lds_fence()
{
    // producer lanes -> consumer lanes of the SAME wave: order the LDS write before the reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// e[j] for the lane's 8 states from one 64-entry table in LDS.
__device__ __forceinline__ void emission_from_table(const double* tab, const LaneCtx& c, double c0, double c1,
                                                    double (&e)[8])
{
    const double A0 = tab[(0 << 5) | (0 << 4) | (c.s1 << 3) | c.lo];
    const double A1 = tab[(0 << 5) | (1 << 4) | (c.s1 << 3) | c.lo];
    const double* B0 = tab + ((1 << 5) | (0 << 4) | (c.s2 << 3));
    const double* B1 = tab + ((1 << 5) | (1 << 4) | (c.s2 << 3));
#pragma unroll
    for (int j = 0; j < 8; j++) {
        // same association as the reference: ((c * other parent) * traced parent), f = 0 then 1
        e[j] = (c0 * B0[j]) * A0 + (c1 * B1[j]) * A1;
    }
}

// adjustprobs' scaling for the 8 chains at once (cnF2freq.cpp:1656-1669).
// mant/expo carry prod(sum) as mant * 2^expo; dead = a sum <= 0 was seen (factor := MINFACTOR).
// 1/x for a positive normal double: hardware estimate + two Newton steps (full double accuracy up
// to the last bit or two; the reference divides each state by sum, cnF2freq.cpp:1664-1667).
__device__ __forceinline__ double fast_rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r        = fma(fma(-x, r, 1.0), r, r);
    r        = fma(fma(-x, r, 1.0), r, r);
    return r;
}

// Sum of a chain's 64 states: over the lane's registers, then over the chain's 8 lanes.  UNI: the vector does not depend on
// the four grandparental state bits (transition_uniform).  With N = 2 the tree's four pair sums are one number s and the
// tree is (s + s) + (s + s); the two lane steps over uniform bits add a value to itself.  Doubling is exact: the same bits
// as the full tree and the three exchanges.
template <bool UNI, int N>
__device__ __forceinline__ double chain_total(const double (&v)[N])
{
    if constexpr (N == 8) {
        double sum = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        if (!UNI) return chain_sum(sum);
        sum += lane_xor1(sum);
        sum += sum;
        sum += sum;
        return sum;
    } else {
        static_assert(UNI && N == 2, "two registers per lane: uniform windows only");
        double sum = v[0] + v[1];
        sum += sum;
        sum += sum;
        sum += lane_xor1(sum);
        sum += sum;
        sum += sum;
        return sum;
    }
}

template <bool UNI = false, int N>
__device__ __forceinline__ double scale_chain(double (&v)[N], double* mant, int* expo, bool* dead, double* inv_out = nullptr)
{
    const double sum = chain_total<UNI>(v);
    // sum <= 0: probs stay as they are (they are all zero), factor = MINFACTOR (cnF2freq.cpp:1656-1660);
    // written branch-free: a dead step scales by 1 and leaves the running scale alone
    const bool   ok  = sum > 0.0;
    const double ss  = ok ? sum : 1.0;
    const double inv = fast_rcp(ss);
    if (!ok) *dead = true;
    if (inv_out) *inv_out = inv;
#pragma unroll
    for (int j = 0; j < N; j++) v[j] *= inv;
    int    ex;
    double mm = frexp(*mant * ss, &ex);
    *mant     = mm;
    *expo += ex;
    return sum;
}

// Same bookkeeping, but the vector is left as it is: returns the reciprocal for the caller to fold into
// the next emission product (it is a per-chain scalar and every step is linear), which takes the
// reduction -> reciprocal chain off the critical path and saves six of the eight multiplies.
template <bool UNI = false, int N>
__device__ __forceinline__ double chain_normaliser(const double (&v)[N], double* mant, int* expo, bool* dead)
{
    const double sum = chain_total<UNI>(v);
    const bool   ok  = sum > 0.0;
    const double ss  = ok ? sum : 1.0;
    const double inv = fast_rcp(ss);
    if (!ok) *dead = true;
    int    ex;
    double mm = frexp(*mant * ss, &ex);
    *mant     = mm;
    *expo += ex;
    return inv;
}

// ------------------------------------------------------------------ crossover posteriors (STOREW == 4)
// Single Kronecker factors of the transition on one state bit: x' = (1-r) x + r partner (general kernel), or with
// SC the fast kernel's scaled butterfly x' = x + t partner, t = r / (1-r) (the dropped (1-r) is common to every state).
template <bool SC, int BIT>
__device__ __forceinline__ void xo_lane_stage(double (&v)[8], double r)
{
    double q[8];
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = BIT == 0 ? lane_xor1(v[j]) : BIT == 1 ? lane_flip_b1(v[j]) : lane_flip_b2(v[j]);
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = SC ? fma(r, q[j], v[j]) : (1.0 - r) * v[j] + r * q[j];
}
template <bool SC, int BIT>
__device__ __forceinline__ void xo_reg_stage(double (&v)[8], double r)
{
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j & (1 << BIT)) continue;
        const double x = v[j], y = v[j + (1 << BIT)];
        v[j]              = SC ? fma(r, y, x) : (1.0 - r) * x + r * y;
        v[j + (1 << BIT)] = SC ? fma(r, x, y) : (1.0 - r) * y + r * x;
    }
}
template <int N>
__device__ __forceinline__ void xo_copy(double (&d)[N], const double (&s)[N])
{
#pragma unroll
    for (int j = 0; j < N; j++) d[j] = s[j];
}

// Numerators of the pairwise posterior of one gap m -> m+1 for this lane's chain: n[t] = sum over (g, g') with state bit t
// flipped of al(g) T(g, g') eb(g'), divided by the flipped factor of bit t (r_t; t_t = r_t / (1-r_t) with SC), which the
// caller multiplies back.  al = alpha after emission at m, eb = e_{m+1} . beta_{m+1}, both in the sweep's layout (state
// g = j * 8 + lo).  T is the Kronecker product of six commuting symmetric 2 x 2 factors, so with X_t on bit t
//     n[t] = < T_A al , X_t T_B eb >   for ANY split A + B of the other five bits.
// Register bits t = 3..5: B = the three lane bits (shared), A = the two other register bits; lane bits t = 0..2: A = the
// three register bits (al in place: it is destroyed), B = the two other lane bits.  Two arrays of temporaries.
// With SC every factor carries the same dropped constant prod (1 - r_u): it cancels against the normaliser <al, T' eb>.
template <bool SC>
__device__ __forceinline__ void xo_numerators(double (&al)[8], const double (&eb)[8], double r0, double r1, double (&n)[6])
{
    // TYPEGENS = {1,0,0,1,0,0}: bits 0 and 3 use r1 (genrec[1]), the other four r0
    double R[8], L[8];
    xo_copy(R, eb);
    xo_lane_stage<SC, 0>(R, r1);
    xo_lane_stage<SC, 1>(R, r0);
    xo_lane_stage<SC, 2>(R, r0);             // R = T_{0,1,2} eb
    double s3 = 0.0, s4 = 0.0, s5 = 0.0;
    xo_copy(L, al);
    xo_reg_stage<SC, 1>(L, r0);
    xo_reg_stage<SC, 2>(L, r0);              // T_{4,5} al
#pragma unroll
    for (int j = 0; j < 8; j++) s3 += L[j] * R[j ^ 1];
    xo_copy(L, al);
    xo_reg_stage<SC, 0>(L, r1);
    xo_reg_stage<SC, 2>(L, r0);              // T_{3,5} al
#pragma unroll
    for (int j = 0; j < 8; j++) s4 += L[j] * R[j ^ 2];
    xo_copy(L, al);
    xo_reg_stage<SC, 0>(L, r1);
    xo_reg_stage<SC, 1>(L, r0);              // T_{3,4} al
#pragma unroll
    for (int j = 0; j < 8; j++) s5 += L[j] * R[j ^ 4];
    xo_reg_stage<SC, 0>(al, r1);
    xo_reg_stage<SC, 1>(al, r0);
    xo_reg_stage<SC, 2>(al, r0);             // al := T_{3,4,5} al
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    xo_copy(R, eb);
    xo_lane_stage<SC, 1>(R, r0);
    xo_lane_stage<SC, 2>(R, r0);             // T_{1,2} eb
#pragma unroll
    for (int j = 0; j < 8; j++) s0 += al[j] * lane_xor1(R[j]);
    xo_copy(R, eb);
    xo_lane_stage<SC, 0>(R, r1);
    xo_lane_stage<SC, 2>(R, r0);             // T_{0,2} eb
#pragma unroll
    for (int j = 0; j < 8; j++) s1 += al[j] * lane_flip_b1(R[j]);
    xo_copy(R, eb);
    xo_lane_stage<SC, 0>(R, r1);
    xo_lane_stage<SC, 1>(R, r0);             // T_{0,1} eb
#pragma unroll
    for (int j = 0; j < 8; j++) s2 += al[j] * lane_flip_b2(R[j]);
    n[0] = s0;
    n[1] = s1;
    n[2] = s2;
    n[3] = s3;
    n[4] = s4;
    n[5] = s5;
}

// Crossover posteriors of one gap m -> m+1 from the chain's numerators: xi_t = sum over chains of w_s f_t n_t / D_s
// (f_t = r_t, or t_t in the scaled form; w_s = the chain's posterior weight, 0 for a chain that does not count; D_s = <al,
// T eb>, the chain's normaliser at m).  Lanes 0..5 write column t of the individual's row and add it to the interval's sum.
__device__ __forceinline__ void xo_store(const KernelParams& p, int ind, int m, const double (&nn)[6], double f0, double f1,
                                         double sw, int lane)
{
    const double ft[6] = {f1, f0, f0, f1, f0, f0};
    double       xt[6];
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const double v = chain_sum(nn[t]);
        xt[t] = across_chains_sum(sw != 0.0 ? sw * ft[t] * v : 0.0);
    }
    const double xv = lane == 0 ? xt[0] : lane == 1 ? xt[1] : lane == 2 ? xt[2] : lane == 3 ? xt[3] : lane == 4 ? xt[4] : xt[5];
    if (lane < 6) {
        if (p.xo) p.xo[((size_t)ind * p.n_markers + m) * 6 + lane] = xv;
        if (xv != 0.0) atomicAdd(&p.xo_sum[(size_t)m * 6 + lane], xv);
    }
}
// the row of the last marker of a chromosome (no gap)
__device__ __forceinline__ void xo_store_zero(const KernelParams& p, int ind, int m, int lane)
{
    if (lane < 6 && p.xo) p.xo[((size_t)ind * p.n_markers + m) * 6 + lane] = 0.0;
}

// ------------------------------------------------------------------ Viterbi decoding (fast kernel, STOREW == 5)
// Max-product form of transition_scaled: every butterfly x' = max(x, t partner), the state keeping its own value unless
// the flipped partner is strictly larger.  The decision (1 = the partner won) of every stage and register is shifted into
// d, first stage / register first: decision (stage k, register j) ends at bit vit_pos(k, j) of the lane's 64-bit word
// (stages 0-3 in the low half, 4-5 in the high half).  A decision belongs to the state the value is written to.
__device__ __forceinline__ int vit_pos(int k, int j) { return k < 4 ? 31 - 8 * k - j : 47 - 8 * (k - 4) - j; }
__device__ __forceinline__ void vit_pick(double& x, double p, uint32_t& d)
{
    const bool c = p > x;
    x = c ? p : x;
    d = d + d + (c ? 1u : 0u);
}
template <int BIT>
__device__ __forceinline__ void vit_lane_stage(double (&v)[8], double t, uint32_t& d)
{
    double q[8];
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = BIT == 0 ? lane_xor1(v[j]) : BIT == 1 ? lane_flip_b1(v[j]) : lane_flip_b2(v[j]);
#pragma unroll
    for (int j = 0; j < 8; j++) vit_pick(v[j], t * q[j], d);
}
template <int BIT>
__device__ __forceinline__ void vit_reg_stage(double (&v)[8], double t, uint32_t& d)
{
    double q[8];
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = v[j ^ (1 << BIT)];
#pragma unroll
    for (int j = 0; j < 8; j++) vit_pick(v[j], t * q[j], d);
}
__device__ __forceinline__ unsigned long long vit_transition(double (&v)[8], double t0, double t1)
{
    uint32_t lo = 0, hi = 0;
    vit_lane_stage<0>(v, t1, lo);          // state bit order and factors of transition_scaled
    vit_lane_stage<1>(v, t0, lo);
    vit_lane_stage<2>(v, t0, lo);
    vit_reg_stage<0>(v, t1, lo);
    vit_reg_stage<1>(v, t0, hi);
    vit_reg_stage<2>(v, t0, hi);
    return ((unsigned long long)hi << 32) | lo;
}
// per-chain maximum (the three DPP steps of chain_sum)
__device__ __forceinline__ double chain_max(double v)
{
    v = fmax(v, lane_xor1(v));
    v = fmax(v, lane_xor2(v));
    v = fmax(v, dpp_mov_all<0x141>(v));
    return v;
}
__device__ __forceinline__ int chain_min_int(int v)
{
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true));
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true));
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true));
    return v;
}
// the lane (within its chain) that holds low state bits lo: lane(lo) = b0 ^ 2 b1 ^ 7 b2 (state_lo is its own inverse)
__device__ __forceinline__ int vit_lane_of(int lo) { return lo ^ ((lo & 4) ? 3 : 0); }
// One gap of the backtrace: the state at marker m from the state x at marker m+1 and the chain's eight decision words of
// the gap (W[lane of lo]).  The stages are undone in reverse order, each decision read at the state the walk has reached.
__device__ __forceinline__ int vit_undo(const unsigned long long* W, int x)
{
    int j = x >> 3, lo = x & 7;
    unsigned long long w = W[vit_lane_of(lo)];
    j ^= (int)((w >> vit_pos(5, j)) & 1) << 2;
    j ^= (int)((w >> vit_pos(4, j)) & 1) << 1;
    j ^= (int)((w >> vit_pos(3, j)) & 1);
    lo ^= (int)((w >> vit_pos(2, j)) & 1) << 2;
    w = W[vit_lane_of(lo)];
    lo ^= (int)((w >> vit_pos(1, j)) & 1) << 1;
    w = W[vit_lane_of(lo)];
    lo ^= (int)((w >> vit_pos(0, j)) & 1);
    return j * 8 + lo;
}

// ------------------------------------------------------------------ posterior sampling (fast kernel, STOREW == 6)
// The counter-based generator of cnf2_sweep_sample (include/cnf2hip.h): SplitMix64's mixing function, and a uniform in
// [0, 1) from the top 53 bits of mix(key ^ j).
__device__ __forceinline__ unsigned long long smp_mix(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double smp_uniform(unsigned long long key, unsigned long long j)
{
    return (double)(smp_mix(key ^ j) >> 11) * 0x1.0p-53;
}
__device__ __forceinline__ double readlane_d(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// Transition factors of one triple of state bits towards the state x drawn at the marker above: f[v] = prod over the bits
// b where v and x differ of t_b (first bit: ta, the other two: tb; the scaled butterflies' T, whose dropped constant is
// common to every weight of a draw).  ta = tb = 1 and x = 0: no transition (the last marker).
__device__ __forceinline__ void smp_factors(int x, double ta, double tb, double (&f)[8])
{
    const double p0 = (x & 1) ? ta : 1.0, q0 = (x & 1) ? 1.0 : ta;        // value of bit 0 is 0 / 1
    const double p1 = (x & 2) ? tb : 1.0, q1 = (x & 2) ? 1.0 : tb;
    const double p2 = (x & 4) ? tb : 1.0, q2 = (x & 4) ? 1.0 : tb;
    const double b01[4] = {p0 * p1, q0 * p1, p0 * q1, q0 * q1};
#pragma unroll
    for (int v = 0; v < 4; v++) {
        f[v]     = b01[v] * p2;
        f[v + 4] = b01[v] * q2;
    }
}
// One draw of the backward walk: the state g of a marker with weights w(g) = al(g) T(g, x), al = the 64 alpha values of
// the draw's chain (g = j*8 + lo, in LDS), x = the state drawn at the marker above; t0 / t1 the gap's factors (state bits
// 0 and 3: t1, the other four: t0).  Inverse CDF in ascending state order (STATE_ORDER is the identity): the group sums
// G_j over the states j*8 .. j*8 + 7 first, then the states of the chosen group -- the first whose running sum exceeds
// u W, or else the last one with a positive weight.  *ratio = w(g) / W.
__device__ __forceinline__ int smp_draw(const double* al, int x, double t0, double t1, double u, double* ratio)
{
    double fl[8];
    smp_factors(x, t1, t0, fl);
    const int    xh = x >> 3;
    double       G[8], W = 0.0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        double sj = 0.0;
#pragma unroll
        for (int l = 0; l < 8; l += 2) {
            const double2 v = *(const double2*)(al + j * 8 + l);
            sj = fma(v.x, fl[l], sj);
            sj = fma(v.y, fl[l + 1], sj);
        }
        const int d = j ^ xh;
        G[j] = sj * (((d & 1) ? t1 : 1.0) * ((d & 2) ? t0 : 1.0) * ((d & 4) ? t0 : 1.0));
        W += G[j];
    }
    const double target = u * W;
    int    jj = -1, jl = 0;
    double base = 0.0, cum = 0.0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const double nc = cum + G[j];
        if (jj < 0 && nc > target) {
            jj   = j;
            base = cum;
        }
        if (G[j] > 0.0) jl = j;
        cum = nc;
    }
    double tg = target;
    if (jj < 0) {
        jj = jl;
        tg = INFINITY;     // (the walk below then takes the group's last positive state)
    }
    const int     d  = jj ^ xh;
    const double  fj = ((d & 1) ? t1 : 1.0) * ((d & 2) ? t0 : 1.0) * ((d & 4) ? t0 : 1.0);
    const double* ag = al + jj * 8;
    int    lp = -1, ll = 0;
    double wp = 0.0, wl = 0.0, run = base;
#pragma unroll
    for (int l = 0; l < 8; l++) {
        const double w = ag[l] * fl[l] * fj;
        run += w;
        if (lp < 0 && run > tg) {
            lp = l;
            wp = w;
        }
        if (w > 0.0) {
            ll = l;
            wl = w;
        }
    }
    if (lp < 0) {
        lp = ll;
        wp = wl;
    }
    *ratio = W > 0.0 ? wp * fast_rcp(W) : 0.0;
    return jj * 8 + lp;
}

// STOREW: 0 = plain sweep; 1 = accumulate mode (posterior weights of every marker into p.wbuf); 2 = turn-scan mode
// (alpha after emission and beta of every marker with their scales into p.wbuf, CNF2_TURN_ROW doubles per marker);
// 4 = crossover mode (posterior probability that each state bit flips across each gap into p.xo / p.xo_sum / p.xo_cnt;
// run with KP_NO_DOSAGE: the dosage rows are not formed)
template <bool DEBUG_STORE, int STOREW = 0>
__global__ __launch_bounds__(CNF2_BLOCK) void fb_kernel(KernelParams p)
{
    __shared__ double lds_tab[CNF2_WAVES_PER_BLOCK][64];
    __shared__ double lds_rt[CNF2_WAVES_PER_BLOCK][64];
    __shared__ double lds_two[CNF2_WAVES_PER_BLOCK][64];

    const int lane  = threadIdx.x & 63;
    const int wib   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave  = blockIdx.x * CNF2_WAVES_PER_BLOCK + wib;
    const int nwave = gridDim.x * CNF2_WAVES_PER_BLOCK;
    double*   tab   = lds_tab[wib];
    double*   tabr  = lds_rt[wib];
    double*   tab2  = lds_two[wib];
    double*   spill = p.spill + (size_t)wave * p.spill_stride;

    for (int job = wave; job < p.n_jobs; job += nwave) {
        const Job    jb = p.jobs[job];
        const Window w  = p.windows[jb.ind];
        if (p.path_log && lane == 0) p.path_log[(size_t)jb.ind * p.n_chrom + jb.chrom] = PATH_GENERAL;
        LaneCtx      c;
        make_lane(w, lane, &c.L);
        c.row_root   = w.row[0];
        c.root_attop = (w.flags[0] & SLOT_FOUNDER) != 0;
        const int s  = lane >> 3;
        c.s0 = s & 1;
        c.s1 = (s >> 1) & 1;
        c.s2 = (s >> 2) & 1;
        c.lo      = state_lo(lane);
        c.active  = !(s & w.shiftignore) && s < w.shiftend;
        c.n_combo = (p.flags & KP_NO_TIES) ? 1 : (1 << w.n_groups);
        if (p.flags & KP_NO_TIES) c.L.tie_par = c.L.tie_tr = c.L.tie_ot = -1;
        const int first = jb.first, last = jb.last, len = last - first + 1;

        // ---------------------------------------------------------------- forward
        double a[8];
#pragma unroll
        for (int j = 0; j < 8; j++) a[j] = 1.0 / 64.0;           // EVENGEN, cnF2freq.cpp:2100-2104
        double mant = 1.0;
        int    expo = 0;
        bool   dead = false;
        double dbg_factor = 0.0;
        for (int m = first; m <= last; m++) {
            const Slot root = load_slot(p, c.row_root, m);
            LineTerms  T;
            double     tot = produce_entry(p, c, root, m, &T);
            tab[lane]      = tot;
            wave_lds_fence();
            double c0, c1, e[8];
            root_weights(c, root, &c0, &c1);
            emission_from_table(tab, c, c0, c1, e);
            wave_lds_fence();                                   // table may be overwritten next round

            // alpha-minus: register-major spill, 8 x 512 B coalesced
            double* sp = spill + (size_t)(m - first) * 512 + lane;
#pragma unroll
            for (int j = 0; j < 8; j++) sp[j * 64] = a[j];
            if (DEBUG_STORE) {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    p.dbg_fwbw[(((size_t)s * len + (m - first)) * 3 + 0) * 64 + j * 8 + c.lo] = a[j];
                if (c.lo == 0) p.dbg_factors[((size_t)s * len + (m - first)) * 3 + 0] = dbg_factor;
            }
            // "We will multiply this already small number with an even smaller number... let's assume it's zero" (adjustprobs,
            // cnF2freq.cpp:1607-1611): the vector is normalised here as it is there, so the threshold is the reference's
            if (p.flags & KP_FLUSH_TINY) {
#pragma unroll
                for (int j = 0; j < 8; j++) a[j] = a[j] < 1e-300 ? 0.0 : a[j];
            }
#pragma unroll
            for (int j = 0; j < 8; j++) a[j] *= e[j];
            bool   was_dead = dead;
            double sum      = scale_chain(a, &mant, &expo, &dead);
            if (DEBUG_STORE) {
                if (dead) dbg_factor = (double)CNF2_MINFACTOR_F;
                else dbg_factor += log(sum);
                (void)was_dead;
#pragma unroll
                for (int j = 0; j < 8; j++)
                    p.dbg_fwbw[(((size_t)s * len + (m - first)) * 3 + 2) * 64 + j * 8 + c.lo] = a[j];
                if (c.lo == 0) p.dbg_factors[((size_t)s * len + (m - first)) * 3 + 2] = dbg_factor;
            }
            if (m < last) {
                const double2 r = p.rho[m];                     // gap m -> m+1 (0 when dist <= 0)
                transition(a, r.x, r.y);
            }
        }

        // ---------------------------------------------------------------- likelihoods
        // factors[s] (cnF2freq.cpp:5375-5382) and factor = logsumexp (cnF2freq.cpp:5384-5400)
        double fs = dead ? (double)CNF2_MINFACTOR_F : (log(mant) + (double)expo * 0.69314718055994530942);
        if (!c.active) fs = CNF2_IGNORED_D;
        double fmaxv = across_chains_max(fs);
        fmaxv        = fmax(fmaxv, -1e15);                      // cnF2freq.cpp:5373
        double term  = c.active ? exp(fs - fmaxv) : 0.0;
        double real  = across_chains_sum(term);
        double factor = fmaxv + log(real);
        if (c.lo == 0) p.factors[((size_t)jb.ind * p.n_chrom + jb.chrom) * 8 + s] = fs;
        if (lane == 0) p.loglik[(size_t)jb.ind * p.n_chrom + jb.chrom] = factor;
        const bool skip = isnan(factor) || factor < (double)CNF2_MINFACTOR_F;      // cnF2freq.cpp:5403
        // weight of this chain in the per-locus row; cnF2freq.cpp:5421 drops modes 40 log units down
        const double ws = (c.active && !skip && !(factor - fs > 40.0)) ? exp(fs - factor) : 0.0;

        if (STOREW == 4 && lane == 0 && !skip) atomicAdd(&p.xo_cnt[jb.chrom], 1);
        if ((p.flags & KP_NO_DOSAGE) && !DEBUG_STORE && STOREW != 4) continue;

        // ---------------------------------------------------------------- backward + rows
        double b[8];
        double eb[8];                                            // crossover mode: e_{m+1} . beta_{m+1} of the marker after m
        (void)eb;
#pragma unroll
        for (int j = 0; j < 8; j++) b[j] = 1.0;                  // cnF2freq.cpp:2111-2114
        double bmant = 1.0;
        int    bexpo = 0;
        bool   bdead = false;
        double dbg_bfactor = 0.0;
        for (int m = last; m >= first; m--) {
            const Slot root = load_slot(p, c.row_root, m);
            LineTerms  T;
            double     tot = produce_entry(p, c, root, m, &T);
            double     c0, c1, e[8];
            root_weights(c, root, &c0, &c1);
            tab[lane] = tot;
            wave_lds_fence();
            emission_from_table(tab, c, c0, c1, e);

            if (DEBUG_STORE) {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    p.dbg_fwbw[(((size_t)s * len + (m - first)) * 3 + 1) * 64 + j * 8 + c.lo] = b[j];
                if (c.lo == 0) p.dbg_factors[((size_t)s * len + (m - first)) * 3 + 1] = dbg_bfactor;
            }

            if (STOREW == 4) {
                // pairwise posterior of the gap m -> m+1 (the last marker has no gap; a gap with rho 0 gives 0).
                // D = <alpha-minus e, beta> is the chain's normaliser at m, and beta_m = T eb exactly (no rescale between)
                if (m < last) {
                    const double* sp = spill + (size_t)(m - first) * 512 + lane;
                    double        al[8], D = 0.0;
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        al[j] = sp[j * 64] * e[j];
                        D += al[j] * b[j];
                    }
                    D = chain_sum(D);
                    const double2 r = p.rho[m];
                    double        nn[6];
                    xo_numerators<false>(al, eb, r.x, r.y, nn);
                    xo_store(p, jb.ind, m, nn, r.x, r.y, (D > 0.0 && ws != 0.0) ? ws / D : 0.0, lane);
                } else xo_store_zero(p, jb.ind, m, lane);
            }

            if (!(p.flags & KP_NO_DOSAGE)) {
                // w_j = alpha-minus * beta ; D = sum_g w e  (normaliser of this chain at this locus)
                const double* sp = spill + (size_t)(m - first) * 512 + lane;
                double        wj[8], D = 0.0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    wj[j] = sp[j * 64] * b[j];
                    D += wj[j] * e[j];
                }
                double n_tot = 0.0, n_a1 = 0.0, n_b1 = 0.0, n_2 = 0.0;
                for (int combo = 0; combo < c.n_combo; combo++) {
                    double rt, tw;
                    restricted_entry(c, root, T, combo, &rt, &tw);
                    wave_lds_fence();
                    tabr[lane] = rt;
                    tab2[lane] = tw;
                    wave_lds_fence();
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        const int    ia = (0 << 5) | (f << 4) | (c.s1 << 3) | c.lo;
                        const double* Br = tabr + ((1 << 5) | (f << 4) | (c.s2 << 3));
                        const double* B1 = tab2 + ((1 << 5) | (f << 4) | (c.s2 << 3));
                        const double  av = tabr[ia], a1 = tab2[ia];
                        double        sb = 0.0, sb1 = 0.0;
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            sb += wj[j] * Br[j];
                            sb1 += wj[j] * B1[j];
                        }
                        const double cf = f ? c1 : c0;
                        n_tot += cf * av * sb;
                        n_a1 += cf * a1 * sb;
                        n_b1 += cf * av * sb1;
                        n_2 += cf * a1 * sb1;
                    }
                }
                D     = chain_sum(D);
                if (STOREW == 2) {
                    // turn-scan mode: A = alphaminus e, B = beta (both as the normalised vectors held here) and their
                    // scales as mantissa and binary exponent: log2 P(data, mode) = fs / ln 2 = lgA + lgB + log2 D
                    double* wp = p.wbuf + ((size_t)job * p.wstride + (m - first)) * CNF2_TURN_ROW;
                    const double lgA = fs * 1.4426950408889634074 - log2(D) - (log2(bmant) + (double)bexpo);
                    const double eA  = floor(lgA);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        *(double2*)(wp + k * 128 + lane * 2) = make_double2(sp[(2 * k) * 64] * e[2 * k], sp[(2 * k + 1) * 64] * e[2 * k + 1]);
                        *(double2*)(wp + 512 + k * 128 + lane * 2) = make_double2(b[2 * k], b[2 * k + 1]);
                    }
                    if (c.lo == 0) {
                        // a chain with no likelihood at all (fs = -inf or the sentinel): scale 0, the turn scan's floor
                        const bool none = !(lgA > -1e300);
                        *(double2*)(wp + 1024 + 4 * s)     = make_double2(none ? 0.0 : exp2(lgA - eA), none ? 0.0 : eA);
                        *(double2*)(wp + 1024 + 4 * s + 2) = make_double2(bmant, (double)bexpo);
                    }
                }
                if (STOREW == 1) {
                    // accumulate mode: wg(s, g) = exp(scales - factor) alphaminus beta = wj * ws / D
                    const double sw = (D > 0.0) ? ws / D : 0.0;
                    double*      wp = p.wbuf + ((size_t)job * p.wstride + (m - first)) * 512;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        double2 v2 = make_double2(sw != 0.0 ? sw * wj[2 * k] : 0.0, sw != 0.0 ? sw * wj[2 * k + 1] : 0.0);
                        *(double2*)(wp + k * 128 + lane * 2) = v2;
                    }
                }
                n_tot = chain_sum(n_tot);
                n_a1  = chain_sum(n_a1);
                n_b1  = chain_sum(n_b1);
                n_2   = chain_sum(n_2);
                const double scale = (D > 0.0) ? ws / D : 0.0;
                // (inclusion-exclusion of non-negative sums: a true zero can come out as -1e-16; clamp)
                double d2 = fmax(across_chains_sum(scale * n_2), 0.0);
                double d1 = fmax(across_chains_sum(scale * (n_a1 + n_b1 - 2.0 * n_2)), 0.0);
                double d0 = fmax(across_chains_sum(scale * (n_tot - n_a1 - n_b1 + n_2)), 0.0);
                if (lane == 0) {
                    if (!(p.flags & KP_RAW_DOSAGE)) {
                        double tsum = d0 + d1 + d2;
                        double inv  = tsum > 0.0 ? 1.0 / tsum : 0.0;
                        d0 *= inv;
                        d1 *= inv;
                        d2 *= inv;
                    }
                    double* out = p.dosage + ((size_t)jb.ind * p.n_markers + m) * 3;
                    out[0] = d0;
                    out[1] = d1;
                    out[2] = d2;
                }
            }

            // beta_{m-1} = T (e_m . beta_m), rescaled (cnF2freq.cpp:2238 with d = -1, then 2273-2367)
            if (m > first) {
                if (p.flags & KP_FLUSH_TINY) {
#pragma unroll
                    for (int j = 0; j < 8; j++) b[j] = b[j] < 1e-300 ? 0.0 : b[j];
                }
#pragma unroll
                for (int j = 0; j < 8; j++) b[j] *= e[j];
                double sum = scale_chain(b, &bmant, &bexpo, &bdead);
                if (DEBUG_STORE) {
                    if (bdead) dbg_bfactor = (double)CNF2_MINFACTOR_F;
                    else dbg_bfactor += log(sum);
                }
                if (STOREW == 4) xo_copy(eb, b);
                const double2 r = p.rho[m - 1];
                transition(b, r.x, r.y);
            }
            wave_lds_fence();
        }
    }
}


// =====================================================================================
// Fast kernel: windows without an active tie (the common case; F2, outbred, ...).
// Same lane/register layout and the same sweep arithmetic as fb_kernel; the emission tables
// are produced per tile of 8 markers by cnf2_emtab.h (lane = part x marker, division-free)
// into LDS, so the per-marker critical path only reads them.
// LDS per wave: 8 markers x TAB_STRIDE doubles: [0,64) tot, [64,68) root weights c[f][s0],
// and for the backward pass [72,136) restricted totals, [136,200) class-2 parts.
// =====================================================================================
#ifndef CNF2_RESCALE_MASK
#define CNF2_RESCALE_MASK 7   /* half-spill sweep: rescale alpha / beta at markers whose local index has these bits clear
                                 (7 = once per tile of 8 markers; measured +3.3 % over rescaling at every second marker) */
#endif
#define CNF2_RESCALE_GUARD 1e150 /* a normaliser below 1 / this makes the wave rescale at every second marker from there on */
#define TAB_STRIDE 202   /* doubles per marker row: 16-B aligned rows, conflict-free producer stores */
#define TAB_C 64
#define TAB_T 68     /* double2: r/(1-r) of the gap carried by this row */
#define TAB_R 72
#define TAB_2 136

typedef double d2v __attribute__((ext_vector_type(2)));     // 16-byte operand of the nontemporal builtins

struct FastCtx {
    PartCfg pc;
    int     part, mi;
    int     idx_base, idx_k01, idx_k10;   // where this lane's entries go in a table row (produce_tile)
    int32_t row_root, row_par, row_tr, row_ot;
    int     slot_a;                       // two-phase producer: window slot this lane prepares (lane >> 3; 7 = none)
    int32_t row_a;                        //                     and its genotype row
    int     s0, s1, s2, lo;
    bool    active;
};

// Raw inputs of one lane of the tile producer (4 window members at one marker), kept packed so
// that they can be requested a whole tile ahead.
struct RawSlots {
    uint8_t ap[4];
    double2 su[4];
    double  hw[4];
    double2 tq;      // scaled recombination odds of the gap this marker's row carries (see produce_tile)
};

// TQ_SHIFT: the forward pass needs the gap after marker m in row m, the backward pass the gap before it
template <int TQ_SHIFT>
__device__ __forceinline__ void load_raw_at(const KernelParams& p, const FastCtx& c, int m, int lo_m, int hi_m, RawSlots* r)
{
    m = m < lo_m ? lo_m : (m > hi_m ? hi_m : m);          // clamp: lanes beyond the chromosome load a valid marker
    const int32_t rows[4] = {c.row_root, c.row_par, c.row_tr, c.row_ot};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t i = (size_t)rows[k] * p.n_markers + m;
        r->ap[k] = p.allele8[i];
        r->su[k] = p.sure[i];
        r->hw[k] = p.hw[i];
    }
    const int mt = m + TQ_SHIFT;
    r->tq        = p.tq[mt < 0 ? 0 : mt];
}
template <int TQ_SHIFT>
__device__ __forceinline__ void load_raw(const KernelParams& p, const FastCtx& c, int m0, int lo_m, int hi_m, RawSlots* r)
{
    load_raw_at<TQ_SHIFT>(p, c, m0 + c.mi, lo_m, hi_m, r);
}

// the table row c.mi of the tile from this lane's raw inputs (valid: the row's marker exists)
// STRIDE: doubles per table row; KOFF > 0 (tie combinations, second of a pair): only the restricted tables are stored,
// KOFF doubles behind the first combination's
template <bool CLASSES, bool HOMPAR = false, bool HOMLEAF = false, bool NORESTR = false, bool TIES = false, int STRIDE = TAB_STRIDE,
          int KOFF = 0>
__device__ __forceinline__ void produce_row(const FastCtx& c, double* tab, bool valid, const RawSlots& raw)
{
    if (valid) {
        const Slot root = unpack_slot(raw.ap[0], raw.su[0].x, raw.su[0].y, raw.hw[0]);
        const Slot par  = unpack_slot(raw.ap[1], raw.su[1].x, raw.su[1].y, raw.hw[1]);
        const Slot tr   = unpack_slot(raw.ap[2], raw.su[2].x, raw.su[2].y, raw.hw[2]);
        const Slot ot   = unpack_slot(raw.ap[3], raw.su[3].x, raw.su[3].y, raw.hw[3]);
        double  cw[2];
        double* row = tab + c.mi * STRIDE;
        // entry e = sp*4 + bit_ot*2 + bit_tr goes to table index base + sp*8 + k: k = 0 / 6 for the two
        // diagonal entries, and the two off-diagonal ones swap places with firstpar (part_entry_index); the
        // two lane-dependent offsets are per-job constants, so no value is ever selected.  Entries are stored
        // as they are formed: the producer holds no output array in registers.
        double* rb = row + c.idx_base;
        emtab_part_to<CLASSES, HOMPAR, HOMLEAF, NORESTR, TIES>(c.pc, root, par, tr, ot,
                               [&](int kind, int e, double v) {
                                   if (KOFF > 0 && kind == 0) return;
                                   const int b  = e & 3;
                                   const int k  = b == 0 ? 0 : (b == 1 ? c.idx_k01 : (b == 2 ? c.idx_k10 : 6));
                                   rb[(kind == 0 ? 0 : (kind == 1 ? TAB_R : TAB_2) + KOFF) + (e >> 2) * 8 + k] = v;
                               },
                               cw);
        if (KOFF > 0) return;
        if ((c.part & 5) == 0) {                    // P == 0, firstpar == 0: one writer per f
            row[TAB_C + c.pc.f * 2 + 0] = cw[0];
            row[TAB_C + c.pc.f * 2 + 1] = cw[1];
        }
        // the gap's butterfly factors ride in the row: the marker loop never touches vmcnt for them
        // (a vector load there would make every s_waitcnt drain the spill stores as well)
        if (c.part == 0) *(double2*)(row + TAB_T) = raw.tq;
    }
}
// hom (wave-uniform): 1 = both parents of the window are homozygous with equal sure at every marker (SLOT_HOM),
// so each part evaluates one allele index of its parent (cnf2_emtab.h HOMPAR); 2 = the four grandparents are
// present and homozygous everywhere as well (HOMLEAF) -- the F2 with empty F1 parents and inbred founders;
// 3 = no slot of the window is restricted (flag2ignore == 0: a complete window): the restricted table is a
// copy of the unrestricted one (NORESTR)
// TIES: the restricted tables of the tie combination whose forces are in c.pc (general form of the producer)
template <bool CLASSES, bool TIES = false, int STRIDE = TAB_STRIDE, int KOFF = 0>
__device__ __forceinline__ void produce_tile(const KernelParams& p, const FastCtx& c, double* tab, int m0, int last,
                                             const RawSlots& raw, int hom)
{
    if (TIES) {
        produce_row<CLASSES, false, false, false, CLASSES, STRIDE, KOFF>(c, tab, m0 + c.mi <= last, raw);
        return;
    }
    if (hom == 2) produce_row<CLASSES, true, true, false, false, STRIDE>(c, tab, m0 + c.mi <= last, raw);
    else if (hom == 1) produce_row<CLASSES, true, false, false, false, STRIDE>(c, tab, m0 + c.mi <= last, raw);
    else if (hom == 3) produce_row<CLASSES, false, false, true, false, STRIDE>(c, tab, m0 + c.mi <= last, raw);
    else produce_row<CLASSES, false, false, false, false, STRIDE>(c, tab, m0 + c.mi <= last, raw);
}

// ---- The tile producer on line records (UNI instantiation; cnf2_emtab.h): a lane loads the root's data
// and the record of (its line, the marker, firstpar, the allele the root hands down) instead of four window members.  The
// record's address depends on the root's allele byte, so that byte is requested one tile earlier than the rest.
struct RawRec {
    uint8_t  ap;                          // the root
    double   s0, s1, hw;
    double   Bp, Cp, Kp, t0, t1, oo;      // the record (LineRec)
    uint32_t bits;
    double   tq0, tq1;                    // scaled recombination odds of the gap this marker's row carries (see produce_tile)
};
__device__ __forceinline__ int clamp_marker(int m, int lo_m, int hi_m) { return m < lo_m ? lo_m : (m > hi_m ? hi_m : m); }
__device__ __forceinline__ uint8_t load_root_allele(const KernelParams& p, const FastCtx& c, int m0, int lo_m, int hi_m)
{
    // (device memory, said so: a caller may hand the base over through a register the compiler cannot see through, and a flat
    // load counts in lgkmcnt as well, where the LDS reads behind it would wait for it)
    const __attribute__((address_space(1))) uint8_t* a8 = (const __attribute__((address_space(1))) uint8_t*)p.allele8;
    return a8[(size_t)c.row_root * p.n_markers + clamp_marker(m0 + c.mi, lo_m, hi_m)];
}
#ifndef CNF2_X_ROOTONCE
#define CNF2_X_ROOTONCE 0
#endif
#if CNF2_X_ROOTONCE      /* timing ablation only (bit 0: the eights' forward pass, bit 1: their backward pass): results are wrong */
struct RawRoot {
    uint8_t ap;
    double  s0, s1, hw;
    __device__ __forceinline__ void into(RawRec* r) const
    {
        r->ap = ap;
        r->s0 = s0;
        r->s1 = s1;
        r->hw = hw;
    }
};
__device__ __forceinline__ void load_root(const KernelParams& p, const FastCtx& c, int m0, int lo_m, int hi_m, RawRoot* r)
{
    const size_t  i  = (size_t)c.row_root * p.n_markers + clamp_marker(m0 + c.mi, lo_m, hi_m);
    const double2 su = p.sure[i];
    r->ap = load_root_allele(p, c, m0, lo_m, hi_m);
    r->s0 = su.x;
    r->s1 = su.y;
    r->hw = p.hw[i];
}
#endif
// ap: load_root_allele of the same tile; rec_row: line * n_markers of this lane's line
// ONE_MARKER: every lane of the wave looks at the same marker (the eights: c.mi is the job), so the gap's factors are one
// value for the wave and come through the scalar cache instead of a vector load of 64 equal addresses (CNF2_UP8_SCALAR_GAP)
// ROOT: the root's own data (sure, hw) is loaded here; false: the caller has it from elsewhere and r keeps what it holds
template <int TQ_SHIFT, bool ONE_MARKER = false, bool ROOT = true>
__device__ __forceinline__ void load_rec(const KernelParams& p, const FastCtx& c, uint32_t rec_row, int m0, int lo_m, int hi_m,
                                         uint8_t ap, RawRec* r)
{
    const int     m = clamp_marker(m0 + c.mi, lo_m, hi_m);
    r->ap = ap;
    if (ROOT) {
        const size_t  i = (size_t)c.row_root * p.n_markers + m;
        const double2 su = p.sure[i];
        r->s0 = su.x;
        r->s1 = su.y;
        r->hw = p.hw[i];
    }
    // the value handed down: root allele f for the line of parent 0, the other one for parent 1
    const int v = ((c.pc.P ^ c.pc.f) & 1) ? (ap >> 4) : (ap & 15);
    const double2* q = (const double2*)(p.line_rec + (((size_t)(rec_row + (uint32_t)m) * LINE_VALUES + v) * 2 + c.pc.firstpar));
    // (ordinary loads: every wave of the launch reads these records, they should stay in the caches)
    const double2 q0 = q[0], q1 = q[1], q2 = q[2];
    r->Bp   = q0.x;
    r->Cp   = q0.y;
    r->Kp   = q1.x;
    r->t0   = q1.y;
    r->t1   = q2.x;
    r->oo   = q2.y;
    r->bits = ((const uint32_t*)q)[12];
    const int mt = m + TQ_SHIFT;
    if (ONE_MARKER) {
        // (constant address space: nothing writes the map's factors while a sweep runs, and the index is the wave's)
        typedef double sd2 __attribute__((ext_vector_type(2)));
        const int mu = __builtin_amdgcn_readfirstlane(mt < 0 ? 0 : mt);
        const sd2 tq = ((const __attribute__((address_space(4))) sd2*)p.tq)[mu];
        r->tq0 = tq.x;
        r->tq1 = tq.y;
    } else {
        const double2 tq = p.tq[mt < 0 ? 0 : mt];
        r->tq0 = tq.x;
        r->tq1 = tq.y;
    }
}
// PACKED: the unrestricted entries a packed sweep reads only (cnf2_emtab.h packed_reads_unrestricted)
template <bool CLASSES, bool PACKED = false>
__device__ __forceinline__ void produce_row_rec(const FastCtx& c, double* tab, bool valid, const RawRec& raw)
{
    if (valid) {
        const Slot root = unpack_slot(raw.ap, raw.s0, raw.s1, raw.hw);
        LineRec rec;
        rec.Bp   = raw.Bp;
        rec.Cp   = raw.Cp;
        rec.Kp   = raw.Kp;
        rec.t0   = raw.t0;
        rec.t1   = raw.t1;
        rec.oo   = raw.oo;
        rec.bits = raw.bits;
        double  cw[2];
        double* row = tab + c.mi * TAB_STRIDE;
        double* rb  = row + c.idx_base;
        emtab_part_rec<CLASSES, PACKED>(c.pc.P, c.pc.f, root, rec,
                                [&](int kind, int e, double v) {        // (the entry's place: see produce_row)
                                    const int b = e & 3;
                                    const int k = b == 0 ? 0 : (b == 1 ? c.idx_k01 : (b == 2 ? c.idx_k10 : 6));
                                    rb[(kind == 0 ? 0 : (kind == 1 ? TAB_R : TAB_2)) + (e >> 2) * 8 + k] = v;
                                },
                                cw);
        if ((c.part & 5) == 0) {
            row[TAB_C + c.pc.f * 2 + 0] = cw[0];
            row[TAB_C + c.pc.f * 2 + 1] = cw[1];
        }
        if (c.part == 0) *(double2*)(row + TAB_T) = make_double2(raw.tq0, raw.tq1);
    }
}
// One thread per record of the launch's lines: [line][marker][value][firstpar]
__global__ __launch_bounds__(256) void line_records_kernel(const LineKey* lines, int n_lines, const uint8_t* allele8,
                                                           const double2* sure, const double* hw, int n_markers, LineRec* out)
{
    const size_t per_line = (size_t)n_markers * LINE_VALUES * 2;
    const size_t t        = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= per_line * (size_t)n_lines) return;
    const int     firstpar = (int)(t & 1), v = (int)((t >> 1) & (LINE_VALUES - 1));
    const size_t  lm = t / (LINE_VALUES * 2);
    const int     m = (int)(lm % (size_t)n_markers);
    const LineKey k = lines[lm / (size_t)n_markers];
    auto slot = [&](int32_t row) {
        const size_t i = (size_t)row * n_markers + m;
        const double2 s = sure[i];
        return unpack_slot(allele8[i], s.x, s.y, hw[i]);
    };
    const Slot par = slot(k.row_par), ga = slot(k.row_a), gb = slot(k.row_b);
    LineRec r;
    line_record_make(k.fl_par, firstpar ? k.fl_b : k.fl_a, firstpar ? k.fl_a : k.fl_b, firstpar, v, par, firstpar ? gb : ga,
                     firstpar ? ga : gb, &r);
    out[t] = r;
}

// Raw inputs of one lane of the tile producer's first phase (ONE window member at one marker), requested a
// whole tile ahead.
struct RawOne {
    uint8_t ap;
    double2 su;
    double  hw;
    double2 tq;      // scaled recombination odds of the gap this marker's row carries (lanes of slot 0)
};

// TQ_SHIFT: the forward pass needs the gap after marker m in row m, the backward pass the gap before it
template <int TQ_SHIFT>
__device__ __forceinline__ void load_raw1_at(const KernelParams& p, const FastCtx& c, int m, int lo_m, int hi_m, RawOne* r)
{
    m = m < lo_m ? lo_m : (m > hi_m ? hi_m : m);          // clamp: lanes beyond the chromosome load a valid marker
    const size_t i = (size_t)c.row_a * p.n_markers + m;
    r->ap = p.allele8[i];
    r->su = p.sure[i];
    r->hw = p.hw[i];
    const int mt = m + TQ_SHIFT;
    r->tq        = p.tq[mt < 0 ? 0 : mt];
}
// Two-phase form of produce_row (used by the packed kernel, where the producer runs every second marker and
// its register footprint decides what spills; for the ordinary kernel the extra LDS round trips cost more than
// the shorter match logic saves: measured 657 against 629 ms).  The table row c.mi in two phases: lanes (slot, row) turn the raw
// data of one window member into its match record (cnf2_emtab.h slot_table: 20 doubles in the row itself); then
// lanes (part, row) combine the records of their line into their 8 entries per table kind and, once every
// lane has read what it needs, store them over the records.
template <bool CLASSES, bool HOMPAR = false, bool HOMLEAF = false>
__device__ __forceinline__ void produce_row2(const FastCtx& c, double* tab, bool valid, const RawOne& raw)
{
    double* row = tab + c.mi * TAB_STRIDE;
    if (valid && c.slot_a < 7)
        slot_table(unpack_slot(raw.ap, raw.su.x, raw.su.y, raw.hw), row + c.slot_a * SLOTTAB_DOUBLES);
    wave_lds_fence();
    double tot[8], rtot[8], two[8], cw[2];
    if (valid)
        emtab_part_tables<CLASSES, HOMPAR, HOMLEAF>(c.pc, row,
                                   [&](int kind, int e, double v) { (kind == 0 ? tot : (kind == 1 ? rtot : two))[e] = v; }, cw);
    wave_lds_fence();
    if (valid) {
        // entry e = sp*4 + bit_ot*2 + bit_tr goes to table index base + sp*8 + k: k = 0 / 6 for the two
        // diagonal entries, and the two off-diagonal ones swap places with firstpar (part_entry_index); the
        // two lane-dependent offsets are per-job constants, so no value is ever selected
        double* rb = row + c.idx_base;
#pragma unroll
        for (int sp = 0; sp < 2; sp++) {
            double* r8 = rb + sp * 8;
            r8[0]         = tot[sp * 4 + 0];
            r8[c.idx_k01] = tot[sp * 4 + 1];
            r8[c.idx_k10] = tot[sp * 4 + 2];
            r8[6]         = tot[sp * 4 + 3];
            if (CLASSES) {
                r8[TAB_R + 0]         = rtot[sp * 4 + 0];
                r8[TAB_R + c.idx_k01] = rtot[sp * 4 + 1];
                r8[TAB_R + c.idx_k10] = rtot[sp * 4 + 2];
                r8[TAB_R + 6]         = rtot[sp * 4 + 3];
                r8[TAB_2 + 0]         = two[sp * 4 + 0];
                r8[TAB_2 + c.idx_k01] = two[sp * 4 + 1];
                r8[TAB_2 + c.idx_k10] = two[sp * 4 + 2];
                r8[TAB_2 + 6]         = two[sp * 4 + 3];
            }
        }
        if ((c.part & 5) == 0) {                    // P == 0, firstpar == 0: one writer per f
            row[TAB_C + c.pc.f * 2 + 0] = cw[0];
            row[TAB_C + c.pc.f * 2 + 1] = cw[1];
        }
        // the gap's butterfly factors ride in the row: the marker loop never touches vmcnt for them
        // (a vector load there would make every s_waitcnt drain the spill stores as well)
        if (c.part == 0) *(double2*)(row + TAB_T) = raw.tq;
    }
}
// (N = 2: a window whose tables do not depend on register-index bits 1 and 2 -- B0[j] = B0[j & 1] -- keeps two registers)
template <int N>
__device__ __forceinline__ void emission_from_row(const double* row, const FastCtx& c, double (&e)[N], double k = 1.0)
{
    const double cA0 = row[TAB_C + 0 + c.s0] * row[(0 << 5) | (0 << 4) | (c.s1 << 3) | c.lo] * k;
    const double cA1 = row[TAB_C + 2 + c.s0] * row[(0 << 5) | (1 << 4) | (c.s1 << 3) | c.lo] * k;
    const double* B0 = row + ((1 << 5) | (0 << 4) | (c.s2 << 3));
    const double* B1 = row + ((1 << 5) | (1 << 4) | (c.s2 << 3));
#pragma unroll
    for (int j = 0; j < N; j++) e[j] = cA0 * B0[j] + cA1 * B1[j];
}

// The same in the transposed layout of an odd marker (XPOSE variant): the lane holds state bits 3-5 (its low lane bits
// index the B half of the table), the registers state bits 0-2 (the A half).
template <int N>
__device__ __forceinline__ void emission_from_row_t(const double* row, const FastCtx& c, double (&e)[N], double k = 1.0)
{
    static_assert(N == 8, "the transposed layout keeps all eight registers");
    const double cB0 = row[TAB_C + 0 + c.s0] * row[(1 << 5) | (0 << 4) | (c.s2 << 3) | c.lo] * k;
    const double cB1 = row[TAB_C + 2 + c.s0] * row[(1 << 5) | (1 << 4) | (c.s2 << 3) | c.lo] * k;
    const double* A0 = row + ((0 << 5) | (0 << 4) | (c.s1 << 3));
    const double* A1 = row + ((0 << 5) | (1 << 4) | (c.s1 << 3));
#pragma unroll
    for (int j = 0; j < 8; j++) e[j] = cB0 * A0[j] + cB1 * A1[j];
}

// Running state of the backward pass of one lane (kept in one struct so that the per-marker body can be
// instantiated for even and odd markers without a merge of differently-defined values between them).
#define CNF2_LI_K __attribute__((always_inline))
template <int N = 8>       // registers per lane (2: fb_fast_kernel's UNI instantiation)
struct BwdState {
    double b[N];          // beta
    double am[N];         // alpha-minus of the row in flight (HALF: of the even marker of the pair)
    double inv_even;      // reciprocal normaliser stored with that row
    double inv_odd;       // HALF: the one of an unrescaled odd last marker (else 1)
    double bmant, fmant;
    int    bexpo, fexpo;
    bool   bdead;
    double ec[N];         // emission of the even marker of the pair: formed for the odd marker's rebuild, reused when
                          // the even marker itself is reached (it is the next one; measured +2.2 %)
    double eb[8];         // crossover mode: e . beta of the marker above (the vector the last beta step transitioned)
};

// HALF: alpha-minus is spilled for every second marker only; the backward pass rebuilds the odd ones
// with one forward step from the stored even neighbour (same arithmetic, same bits).  Halves the
// spill traffic for ~15 % more arithmetic.
// TIED: windows with tie groups (ignoreflag2's all-or-none rule, cnF2freq.cpp:3484-3486).  The forward pass and the beta
// recursion do not see the rule; the per-locus rows are sums over the tie combinations (2, 4 or 8 of them) of class sums
// taken with that combination's restricted tables.  A table row holds the restricted tables of TWO combinations; a marker's
// posterior weights are contracted with both (everything else at the marker is the same for every combination), so a
// window with one tie group -- most of them -- is swept in one backward pass, one with two groups in two.  Every further
// pass over a tile starts from the tile's state (beta, scales: kept in LDS; spill row and tile inputs: asked for again)
// and the tile epilogue adds the passes up before it writes the rows.  The tables are dynamic LDS (84 KB a block, see the
// declaration): a block shares a CU with a block of the untied windows' kernel, not with another of its own.
// UNI: the plain half-spill sweep of the windows with slots_uniform (cnf2_emission.h) -- every cross of inbred lines.  Their
// unrestricted tables, and so alpha and beta, do not depend on the four grandparental state bits: the transition's stages on
// those bits need no exchange (transition_uniform), and a lane carries CNF2_UNI_REGS registers per vector: the two that
// differ (register bit 0), or all 8 (A/B: the exchanges alone).  Same operations on the same numbers: the bits of the
// ordinary instantiation.  Jobs of other windows are skipped (the ordinary instantiation skips these under KP_SKIP_UNIFORM
// when both run over one job list).  The restricted tables do depend on those bits and are read in full -- once per group of
// four lanes that would form the same class sums (the `marker` lambda of the backward pass).
#ifndef CNF2_UNI_REGS
#define CNF2_UNI_REGS 2
#endif
// blocks per CU the UNI instantiation is compiled for (the others, and its A/B form with 8 registers a vector: 2).  3: at most
// 168 registers a lane
#ifndef CNF2_UNI_MIN_BLOCKS
#define CNF2_UNI_MIN_BLOCKS 3
#endif
// UNI comes in two forms over the same job list, each skipping the other's jobs.  REC, the instantiation with STOREW =
// SW_PLAIN: the tile producer on the launch's line records (produce_row_rec), for the windows that have their two lines in
// p.line_keys.  STOREW = SW_PLAIN_UNIFORM_ROWS: the plain sweep all the same, with the ordinary tile producer, for the uniform
// windows that have not (all of them when p.line_keys is NULL).
template <bool HALF, int STOREW_ARG = 0, bool XPOSE = false, bool TIED = false, bool UNI = false>
__global__ __launch_bounds__(CNF2_BLOCK, UNI && CNF2_UNI_REGS == 2 ? CNF2_UNI_MIN_BLOCKS : 2) void fb_fast_kernel(KernelParams p)
{
    static_assert(UNI || STOREW_ARG != SW_PLAIN_UNIFORM_ROWS, "a form of the uniform-state variant");
    constexpr int  STOREW = STOREW_ARG == SW_PLAIN_UNIFORM_ROWS ? (int)SW_PLAIN : STOREW_ARG;
    constexpr bool REC    = UNI && STOREW_ARG != SW_PLAIN_UNIFORM_ROWS;
    static_assert(!UNI || (HALF && STOREW == SW_PLAIN && !XPOSE && !TIED), "the uniform-state variant exists for the plain half-spill sweep");
    static_assert(CNF2_UNI_REGS == 2 || CNF2_UNI_REGS == 8, "registers per lane and vector of the uniform-state variant");
    constexpr int  NR   = UNI ? CNF2_UNI_REGS : 8;      // registers per lane and vector
    constexpr bool PAIR = HALF && STOREW == SW_PLAIN && !XPOSE && !TIED && !UNI;    // the instantiation UNI may run beside
    static_assert(!XPOSE || (HALF && STOREW == SW_PLAIN), "the transposing variant exists for the plain half-spill sweep");
    // STOREW is a SweepVariant (cnf2_device.h: SW_PLAIN .. SW_DESCENT); by value:
    // STOREW: 0 plain sweep; 1 accumulate mode (also stores the posterior weights wg); 2 turn-scan mode (stores alpha e, beta
    // and their scales; no rows); 3 accumulate mode of a call that did not ask for the per-locus rows (wg only); 4 crossover
    // mode (posterior probability of a flip of every state bit across every gap into p.xo / p.xo_sum / p.xo_cnt; no rows);
    // 5 Viterbi mode (no alpha spill: the max-product recursion beside the forward pass stores its decisions in the spill
    // slot, and a backtrace replaces the backward pass: p.vit_logmax / p.vit_state / p.vit_shift; no rows); 6 sampling mode
    // (the plain forward pass; backward walks that rebuild alpha and draw whole paths from the posterior, one draw per
    // lane: p.smp_state / p.smp_shift / p.smp_logp; no beta, no rows); 7 placement mode (stores the state posteriors
    // gamma = wg e of every marker where the accumulate mode stores wg; counts the jobs with a likelihood in p.xo_cnt; no rows);
    // 8 leave-one-out mode (per marker sum_s L_s,-m / L over every mode with a likelihood and the marker's unlinked emission
    // mean into p.loo / p.unl, their logarithms left to loo_finish_kernel; counts the jobs with a likelihood in p.xo_cnt; no rows);
    // 9 origin mode (per marker eight masked sums of the state posterior gamma = wg e over the modes the rows count, normalised
    // by their total: the four origin cells into p.org, P(bit t = 1) into p.obits; counts the jobs with a likelihood in
    // p.xo_cnt; no rows); 11 descent mode (the origin mode's posterior and normaliser; per marker the eight descent classes,
    // four per side, eight to a row of p.org; counts the jobs with a likelihood in p.xo_cnt; no rows)
    constexpr bool ROWS = STOREW == SW_PLAIN || STOREW == SW_WEIGHTS_ROWS;      // class sums, restricted tables, tile epilogue, p.dosage
    constexpr bool WG   = STOREW == SW_WEIGHTS_ROWS || STOREW == SW_WEIGHTS;
    constexpr bool VIT  = STOREW == SW_VITERBI;
    constexpr bool SMP  = STOREW == SW_SAMPLING;
    constexpr bool POST = STOREW == SW_POSTERIOR;
    constexpr bool LOO  = STOREW == SW_LOO;
    constexpr bool ORG  = STOREW == SW_ORIGINS;
    constexpr bool DSC  = STOREW == SW_DESCENT;
    static_assert(!ORG || (!XPOSE && !TIED), "the origin mode is an instantiation of the untied DPP kernel");
    static_assert(!DSC || (!XPOSE && !TIED), "the descent mode is an instantiation of the untied DPP kernel");
    static_assert(!LOO || (!XPOSE && !TIED), "the leave-one-out mode is an instantiation of the untied DPP kernel");
    static_assert(!POST || (!XPOSE && !TIED), "the placement mode is an instantiation of the untied DPP kernel");
    static_assert(!VIT || (!XPOSE && !TIED), "the Viterbi mode is an instantiation of the untied DPP kernel");
    static_assert(!SMP || (!XPOSE && !TIED), "the sampling mode is an instantiation of the untied DPP kernel");
    static_assert(!TIED || (!XPOSE && ROWS), "tie combinations only matter to the rows");
    // Spill row (528 doubles): [k = 0..3][lane][2] = registers 2k, 2k+1 of every lane (one 16-byte access
    // per lane and k), then [chain][2] = reciprocal normaliser of the (even) marker and, HALF only, of
    // an odd last marker.
    // UNI with two registers per lane: the compact row of cnf2_lane.h (48 doubles: every distinct value once).  The wave's slot
    // is p.spill_stride doubles whatever the row's size, so an ordinary instantiation may follow in the same slots.
    constexpr bool URow = UNI && NR == 2;
    constexpr int  ROW  = URow ? (int)UNI_SPILL_ROW : 528;
    constexpr int  INV  = URow ? (int)UNI_SPILL_INV : 512;     // the reciprocals' place in a row
    // TIED: the restricted tables of TWO tie combinations per row (the second pair TIE_KOFF doubles behind the first)
    constexpr int TIE_KOFF = 128;
    constexpr int TS = TIED ? TAB_STRIDE + TIE_KOFF : TAB_STRIDE;
    // (TIED: the tables are dynamic LDS, CNF2_TIED_LDS_BYTES at the launch.  With 105 KB of static LDS the compiler concludes
    // that only one block fits a CU and hands every wave 400 registers -- which keeps the block from sharing a CU with a
    // block of the untied windows' kernel; what it cannot see it does not count, and the launch bounds' 256 registers stand)
    __shared__ __attribute__((aligned(16))) double lds[TIED ? 1 : CNF2_WAVES_PER_BLOCK][TIED ? 2 : 8 * TS];
    extern __shared__ __attribute__((aligned(16))) double lds_tied[];
    __shared__ __attribute__((aligned(16))) double xlds[XPOSE ? CNF2_WAVES_PER_BLOCK : 1][XPOSE ? 64 * XPOSE_RS : 2];
    __shared__ double tsum[TIED ? CNF2_WAVES_PER_BLOCK : 1][TIED ? 24 : 1];     // TIED: class sums of the tile's markers over the combinations
    // TIED: beta and the two scale mantissas as they stand at the tile's start ([k][lane]: conflict-free), read back for
    // every further combination -- 20 registers per lane that would otherwise live (in scratch) across the whole tile
    __shared__ double tsave[TIED ? CNF2_WAVES_PER_BLOCK : 1][TIED ? 11 * 64 : 1];

    const int wib   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave  = blockIdx.x * CNF2_WAVES_PER_BLOCK + wib;
    const int nwave = gridDim.x * CNF2_WAVES_PER_BLOCK;
    double*   tab   = TIED ? lds_tied + wib * (8 * TS) : lds[TIED ? 0 : wib];
    double*   xb    = xlds[XPOSE ? wib : 0];
    double*   spill = p.spill + (size_t)wave * p.spill_stride;
    // shader-clock and wall-clock ticks of the first wave (the bench's effective clock of this very kernel)
    const bool stamp = p.clock_out != nullptr && wave == 0;
    unsigned long long t_shader = 0, t_wall = 0;
    if (stamp) {
        t_shader = __builtin_readcyclecounter();
        t_wall   = wall_clock64();
    }

    // the next job of this wave: from the launch's counter (one atomic per job, by lane 0) or, without one, by striding
    auto take_job = [&](int strided) {
        if (!p.job_next) return strided;
        int j = 0;
        if (fresh_lane() == 0) j = atomicAdd(p.job_next, 1);
        return __builtin_amdgcn_readfirstlane(j);
    };
    for (int job = take_job(wave); job < p.n_jobs; job = take_job(job + nwave)) {
        // the lane number read afresh, as a value the compiler cannot see through: what is derived from it is formed per
        // job, where it is used, instead of being held in registers (or spilled) for the whole kernel
        const int lane = fresh_lane();
        const Job    jb = p.jobs[job];
        const Window w  = p.windows[jb.ind];
        FastCtx      c;
        c.part = lane >> 3;
        c.mi   = lane & 7;
        make_part(w, c.part, &c.pc, &c.row_par, &c.row_tr, &c.row_ot);
        c.idx_base  = part_entry_index(c.part, 0);          // (sp, bit_ot, bit_tr) = (0, 0, 0)
        c.idx_k01   = part_entry_index(c.part, 1) - c.idx_base;
        c.idx_k10   = part_entry_index(c.part, 2) - c.idx_base;
        c.row_root  = w.row[0];
        int hom = 0;
        if (w.flags[1] & w.flags[4] & SLOT_HOM) hom = slots_uniform(w.flags) ? 2 : 1;
        if (hom == 0 && w.flag2ignore == 0) hom = 3;
        if (TIED) hom = 0;
        hom = __builtin_amdgcn_readfirstlane(hom);
        if (UNI && hom != 2) continue;
        if (PAIR && (p.flags & KP_SKIP_UNIFORM) && hom == 2) continue;
        // UNI: the window's two lines, where the launch holds records for them (wave-uniform); else the ordinary producer
        uint32_t rec_row = 0;      // line * n_markers of this lane's line
        uint8_t  ap_next = 0;      // the root's allele byte of the tile after the one whose inputs are in flight
        if constexpr (UNI) {
            bool on_rec = false;
            if (p.line_keys) {
                const int32_t k0 = p.line_keys[2 * (size_t)jb.ind], k1 = p.line_keys[2 * (size_t)jb.ind + 1];
                on_rec  = __builtin_amdgcn_readfirstlane((int)(k0 >= 0 && k1 >= 0)) != 0;
                rec_row = (uint32_t)(c.pc.P ? k1 : k0) * (uint32_t)p.n_markers;
            }
            if (on_rec != REC) continue;
        }
        const int n_combo = TIED ? __builtin_amdgcn_readfirstlane(1 << w.n_groups) : 1;
        // TIED: the tie groups of this lane's three slots (part_forces), one byte each, so that the window itself need not
        // stay live for the combinations' loop
        int my_ties = 0;
        if (TIED) {
            const bool   hi = (c.part >> 2) != 0, fp = (c.part & 1) != 0;
            const int8_t tp = hi ? w.tie[4] : w.tie[1];
            const int8_t ta = hi ? w.tie[5] : w.tie[2], tb = hi ? w.tie[6] : w.tie[3];
            const int8_t tt = fp ? tb : ta, to = fp ? ta : tb;
            my_ties = (tp & 255) | ((tt & 255) << 8) | ((to & 255) << 16);
        }
        if (p.path_log && lane == 0) p.path_log[(size_t)jb.ind * p.n_chrom + jb.chrom] = TIED ? PATH_TIED : hom;
        const int s = lane >> 3;
        c.s0 = s & 1;
        c.s1 = (s >> 1) & 1;
        c.s2 = (s >> 2) & 1;
        c.lo = XPOSE ? (lane & 7) : state_lo(lane);   // no DPP butterflies in the transposing variant: plain order
        c.active = !(s & w.shiftignore) && s < w.shiftend;
        const int first = jb.first, last = jb.last;
        const int ntile = (last - first + 8) >> 3;
        // compact spill row: the lane's place in it, and whether it writes its pair / its chain's reciprocals there.  A launch
        // that stops after the forward pass (KP_NO_DOSAGE: the plain sweep forms no rows) reads no spill row, so nobody
        // writes one: the launch's flag is folded into the lanes' store predicates, no branch in the marker loop
        const bool uspill = !URow || !(p.flags & KP_NO_DOSAGE);
        const int  uoff   = URow ? uni_spill_value(lane) : 0;
        const bool uwr    = URow && uspill && uni_spill_writer(lane);
        const bool iwr    = c.lo == 0 && !(STOREW == SW_VITERBI) && uspill;

        using odd_t  = std::integral_constant<bool, true>;
        using even_t = std::integral_constant<bool, false>;

        // ---------------------------------------------------------------- forward
        double a[NR];
#pragma unroll
        for (int j = 0; j < NR; j++) a[j] = 1.0 / 64.0;
        double mant = 1.0;
        int    expo = 0;
        bool   dead = false;
        double pend = 1.0;     // reciprocal normaliser not yet applied to a[] (folded into the next emission)
        int    rmask = CNF2_RESCALE_MASK, bmask = CNF2_RESCALE_MASK;   // rescaling pattern of the forward / backward pass
        // Viterbi mode: the max-product vector of the same chains.  It takes the same emission products as a[] (HALF: with
        // the folded reciprocals, so it lives in a[]'s scale; full spill: unscaled), and its own power-of-two rescaling by
        // the chain maximum (exact: no decision changes), whose exponents sum to vexpo.  Decisions: [gap][lane] words.
        double vt[8];
        int    vexpo = 0;
        unsigned long long* const vbits = (unsigned long long*)spill;
#pragma unroll
        for (int j = 0; j < 8; j++) vt[j] = 1.0 / 64.0;
        // One marker of the forward pass.  ODD (HALF only): nothing is spilled and, except at the last
        // marker of the chromosome, nothing is rescaled: two emission products in a row cannot underflow a
        // double.  A skipped step has normaliser 1 (the reference rescales at every marker,
        // cnF2freq.cpp:1664-1668; only the bookkeeping of the scale differs, not the normalised values).
        auto fwd_step = [&](auto odd_tag, const double* row, int m) {
            constexpr bool ODD = decltype(odd_tag)::value;
            double         e[NR];
            if constexpr (XPOSE && ODD) emission_from_row_t(row, c, e, pend);
            else emission_from_row(row, c, e, pend);
            const double2 r  = *(const double2*)(row + TAB_T);
            const int     ml = m - first;
            double*       sp = spill + (size_t)(HALF ? (ml >> 1) : ml) * ROW;
            if (!ODD && !VIT) {
#ifndef CNF2_X_NOSTORE   /* timing ablation only: results are wrong */
                if constexpr (URow) {
                    // the two lanes of a chain that stand for its two classes: 16 lanes, 256 contiguous bytes
                    const d2v v = {a[0], a[1]};
                    if (uwr) __builtin_nontemporal_store(v, (d2v*)(sp + uoff));
                } else {
#pragma unroll
                    for (int k = 0; k < NR / 2; k++) {
                        // written once, read once a whole chromosome later: streaming (nt) accesses keep the rows
                        // from churning L2 (measured: -2 %)
                        const d2v v = {a[2 * k], a[2 * k + 1]};
                        __builtin_nontemporal_store(v, (d2v*)(sp + k * 128 + lane * 2));
                    }
                }
#endif
            }
#pragma unroll
            for (int j = 0; j < NR; j++) a[j] *= e[j];
            if constexpr (VIT) {
#pragma unroll
                for (int j = 0; j < 8; j++) vt[j] *= e[j];
                if (!ODD) {
                    // (HALF: every second marker; two markers cannot lose 300 decades against a[])
                    const double vm = fmax(fmax(fmax(vt[0], vt[1]), fmax(vt[2], vt[3])), fmax(fmax(vt[4], vt[5]), fmax(vt[6], vt[7])));
                    int ex;
                    (void)frexp(chain_max(vm), &ex);
#pragma unroll
                    for (int j = 0; j < 8; j++) vt[j] = ldexp(vt[j], -ex);
                    vexpo += ex;
                }
            }
            pend = 1.0;
            // HALF: the vectors are rescaled at every CNF2_RESCALE-th marker only (and at the last one): a few emission
            // products in a row cannot underflow a double, and a skipped step simply has normaliser 1
            const bool norm_here = !HALF || m == last || (!ODD && (ml & rmask) == 0);
            if (norm_here) {
                // reciprocal of this step's normaliser, per chain: stored so that the backward pass can
                // rebuild the forward scale before each marker without a reduction (and redo the forward step)
                double inv;
                if (HALF) {
                    inv  = chain_normaliser<UNI>(a, &mant, &expo, &dead);
                    pend = inv;
                    // data that loses > 150 decades in one stretch: keep the vectors in range by rescaling densely
                    if (__ballot(inv > CNF2_RESCALE_GUARD)) rmask = 1;
                } else {
                    scale_chain<UNI>(a, &mant, &expo, &dead, &inv);     // full spill: the stored rows are normalised at once
                }
                if (iwr) sp[INV + 2 * s + (ODD ? 1 : 0)] = inv;
            } else if (!ODD && !VIT) {
                if (iwr) sp[INV + 2 * s] = 1.0;
            }
            if (m < last) {
                if constexpr (XPOSE) transition_xpose(a, r.x, r.y, xb, lane);
                else if constexpr (UNI) transition_uniform(a, r.x, r.y);
                else transition_scaled(a, r.x, r.y);
                if (VIT) {
                    const unsigned long long d = vit_transition(vt, r.x, r.y);
                    __builtin_nontemporal_store(d, vbits + (size_t)ml * 64 + lane);
                }
            }
        };
        RawSlots raw;
        RawRec   rraw;
        if constexpr (REC) {
            load_rec<0>(p, c, rec_row, first, first, last, load_root_allele(p, c, first, first, last), &rraw);
            ap_next = load_root_allele(p, c, first + 8, first, last);
        } else load_raw<0>(p, c, first, first, last, &raw);
        for (int t = 0; t < ntile; t++) {
            const int m0 = first + t * 8;
            if constexpr (REC) {
                produce_row_rec<false>(c, tab, m0 + c.mi <= last, rraw);
                if (t + 1 < ntile) {
                    load_rec<0>(p, c, rec_row, m0 + 8, first, last, ap_next, &rraw);
                    ap_next = load_root_allele(p, c, m0 + 16, first, last);
                }
            } else
#ifdef CNF2_X_NOPRODUCE  /* timing ablation only: results are wrong */
            if (t == 0)
#endif
            {
                produce_tile<false, false, TS>(p, c, tab, m0, last, raw, hom);
                if (t + 1 < ntile) load_raw<0>(p, c, m0 + 8, first, last, &raw);   // next tile's inputs, a tile ahead
            }
            wave_lds_fence();
            const int mend = (m0 + 7 < last) ? m0 + 7 : last;
            if (HALF) {
                const int itop = mend - m0;
                for (int i = 0; i <= itop; i += 2) {
                    fwd_step(even_t(), tab + i * TS, m0 + i);
                    if (i < itop) fwd_step(odd_t(), tab + (i + 1) * TS, m0 + i + 1);
                }
            } else {
                for (int m = m0; m <= mend; m++) fwd_step(even_t(), tab + (m - m0) * TS, m);
            }
            wave_lds_fence();
        }

        // ---------------------------------------------------------------- likelihoods
        // P(data, mode s) = mant 2^expo per chain.  Everything the backward pass needs of them is exact binary scaling:
        // with T = sum over the live chains of mant 2^(expo - emax), exp(-factor) = (1 / T) 2^-emax, and the reference's
        // "40 below the total" rule (cnF2freq.cpp:5420-5421) compares a chain's term with T.  The logarithms the
        // outputs hold (and the chromosome's dropped butterfly constants) are taken by likelihood_logs_kernel after the
        // sweep: the sweep kernel has no transcendental and none of their constants in its registers.
        const bool   alive  = c.active && !dead;
        const double emaxd  = across_chains_max(alive ? (double)expo : -1e300);
        const bool   any_alive = emaxd > -1e299;
        const int    emax   = any_alive ? (int)emaxd : 0;
        int          dsh    = expo - emax;
        dsh                 = dsh < -2000 ? -2000 : dsh;
        const double tmine  = alive ? ldexp(mant, dsh) : 0.0;
        const double T      = across_chains_sum(tmine);
        {
            const size_t e = (size_t)jb.ind * p.n_chrom + jb.chrom;
            const int    n_active = __builtin_popcountll(__ballot(c.active)) >> 3;
            if (c.lo == 0) {
                p.factors[e * 8 + s] = mant;
                p.fexp[e * 8 + s]    = alive ? expo : (c.active ? CNF2_LEXP_DEAD : CNF2_LEXP_IGNORED);
            }
            if (lane == 0) {
                // no live chain: every analysed mode sits at the floor, the total is the floor + log(their number)
                p.loglik[e] = any_alive ? T : (double)n_active;
                p.lexp[e]   = any_alive ? emax : CNF2_LEXP_DEAD;
            }
        }
        if ((STOREW == 4 || POST || LOO || ORG || DSC) && lane == 0 && any_alive) atomicAdd(&p.xo_cnt[jb.chrom], 1);
        if (VIT) {
            // ------------------------------------------------------------ Viterbi: logmax, MAP mode, backtrace
            // logmax_s = log(max-product) + the chromosome's dropped butterfly constants, as likelihood_logs_kernel finishes
            // the factors.  HALF: vt[] carries a[]'s scale F, and F = mant 2^expo / (last normaliser) = mant 2^expo pend.
            const size_t e    = (size_t)jb.ind * p.n_chrom + jb.chrom;
            uint8_t*     st   = p.vit_state + (size_t)jb.ind * p.n_markers + first;
            double       vm   = vt[0];
#pragma unroll
            for (int j = 1; j < 8; j++) vm = fmax(vm, vt[j]);
            vm = chain_max(vm);
            int          qe;
            const double qm   = frexp(vm * (HALF ? pend * mant : 1.0), &qe);
            const bool   live = alive && vm > 0.0;
            const double lm   = live ? log(qm) + (double)(qe + vexpo + (HALF ? expo : 0)) * 0.69314718055994530942 +
                                           p.chrom_logk[jb.chrom]
                                     : (c.active ? (double)CNF2_MINFACTOR_F : CNF2_IGNORED_D);
            const double best = across_chains_max(live ? lm : -INFINITY);
            if (!any_alive || !(best > -INFINITY)) {
                // skipped, as the sweep skips it: no state, no mode, every logmax CNF2_IGNORED
                if (c.lo == 0) p.vit_logmax[e * 8 + s] = CNF2_IGNORED_D;
                if (lane == 0) p.vit_shift[e] = -1;
                for (int ml = lane; ml <= last - first; ml += 64) st[ml] = 0xFF;
                continue;
            }
            if (c.lo == 0) p.vit_logmax[e * 8 + s] = lm;
            // MAP mode: the lowest chain among the maxima; its final state: the lowest state index among the maxima
            const int sstar = __builtin_amdgcn_readfirstlane(__builtin_ctzll(__ballot((lane & 7) == 0 && live && lm == best)) >> 3);
            int       g     = 64;
#pragma unroll
            for (int j = 7; j >= 0; j--)
                if (vt[j] == vm) g = j * 8 + c.lo;
            int x = __builtin_amdgcn_readlane(chain_min_int(g), sstar * 8);
            if (lane == 0) {
                p.vit_shift[e]    = sstar;
                st[last - first] = (uint8_t)x;
            }
            // backtrace: 64 gaps at a time, lane i fetches the 64 B of chain s* of gap top - i into LDS (the tile below
            // is requested before the walk of this one); the walk itself is wave-uniform, three LDS reads a gap
            using u2v = unsigned long long __attribute__((ext_vector_type(2)));
            unsigned long long* tl   = (unsigned long long*)tab;
            const unsigned long long* vsrc = vbits + sstar * 8;
            u2v w4[4];
            auto load_tile = [&](int top) {
                const int gi = top - lane < 0 ? 0 : top - lane;
#pragma unroll
                for (int k = 0; k < 4; k++) w4[k] = __builtin_nontemporal_load((const u2v*)(vsrc + (size_t)gi * 64) + k);
            };
            const int ngap = last - first;
            if (ngap > 0) load_tile(ngap - 1);
            for (int top = ngap - 1; top >= 0; top -= 64) {
#pragma unroll
                for (int k = 0; k < 4; k++) *(u2v*)(tl + lane * 8 + 2 * k) = w4[k];
                wave_lds_fence();
                if (top >= 64) load_tile(top - 64);
                const int cnt  = top < 63 ? top + 1 : 64;
                int       mine = 0;
                for (int i = 0; i < cnt; i++) {
                    x    = vit_undo(tl + i * 8, x);
                    mine = lane == i ? x : mine;
                }
                if (lane < cnt) st[top - lane] = (uint8_t)mine;
                wave_lds_fence();
            }
            continue;
        }
        if (SMP) {
            // ------------------------------------------------------------ sampling: forward filtering, backward sampling
            // Lane k of a walk makes draw k0 + k: a mode from P(s | data) over the modes the dosage rows count, then the
            // states from the last marker down, each from w(g) = alpha_m(g) T(g, g_m+1) in the drawn mode's chain.  At
            // every marker the wave rebuilds alpha (= alpha-minus e up to a per-chain factor, which cancels in a draw) as
            // the crossover mode does and parks the 8 chains' vectors in the tile rows' free restricted-table space (row s,
            // [TAB_R, TAB_R + 64): chain s), from where each lane reads its own chain.  More than 64 draws: further walks
            // over the same spill rows.  logp = log P(s | data) + the log of every pick's w / W, carried as mantissa and
            // exponent; one log per draw and chromosome.
            const int K   = p.smp_draws;
            const int len = last - first + 1;
            if (!any_alive) {
                // skipped, as the sweep skips it: no mode, no state
                for (int k = lane; k < K; k += 64) {
                    const size_t o = ((size_t)jb.ind * K + k) * p.n_chrom + jb.chrom;
                    p.smp_shift[o] = -1;
                    if (p.smp_logp) p.smp_logp[o] = CNF2_IGNORED_D;
                }
                for (int k = 0; k < K; k++) {
                    uint8_t* st = p.smp_state + ((size_t)jb.ind * K + k) * p.n_markers + first;
                    for (int ml = lane; ml < len; ml += 64) st[ml] = 0xFF;
                }
                continue;
            }
            // P(s | data) of the counted modes (factor - fs <= 40: cnF2freq.cpp:5420-5421), wave-uniform
            const bool   on_s = alive && !(tmine * 2.3538526683701998e17 < T);
            const double pws  = on_s ? tmine / T : 0.0;
            double       pw[8];
#pragma unroll
            for (int m8 = 0; m8 < 8; m8++) pw[m8] = readlane_d(pws, m8 * 8);
            const unsigned long long key0 = smp_mix(smp_mix(p.smp_seed) ^ (unsigned long long)(long long)(p.smp_ind0 + jb.ind));
            double* const al0 = tab + TAB_R;
            for (int k0 = 0; k0 < K; k0 += 64) {
                const int                k   = k0 + lane;
                const bool               on  = k < K;
                const unsigned long long key = smp_mix(key0 ^ (unsigned long long)k);
                // the mode: inverse CDF over the 8 chains in ascending order
                int sm = -1, sl = 0;
                {
                    double W = 0.0;
#pragma unroll
                    for (int m8 = 0; m8 < 8; m8++) W += pw[m8];
                    const double tg = smp_uniform(key, (unsigned long long)(p.n_markers + jb.chrom)) * W;
                    double       cum = 0.0;
#pragma unroll
                    for (int m8 = 0; m8 < 8; m8++) {
                        cum += pw[m8];
                        if (sm < 0 && cum > tg) sm = m8;
                        if (pw[m8] > 0.0) sl = m8;
                    }
                    if (sm < 0) sm = sl;
                }
                double pmant = 0.0;
#pragma unroll
                for (int m8 = 0; m8 < 8; m8++) pmant = sm == m8 ? pw[m8] : pmant;
                int pexp = 0;
                pmant    = frexp(pmant, &pexp);
                const double* al = al0 + sm * TS;
                uint8_t*      st = p.smp_state + ((size_t)jb.ind * K + (on ? k : 0)) * p.n_markers;
                int           x  = 0;                    // state drawn at the marker above
                double        rt0 = 1.0, rt1 = 1.0;      // factors of the gap to it (none at the last marker)
                double        am[8];                     // alpha-minus of the spill row in flight
                auto load_am = [&](int idx) {
                    const double* sp = spill + (size_t)idx * ROW;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const d2v v = __builtin_nontemporal_load((const d2v*)(sp + q * 128 + lane * 2));
                        am[2 * q]     = v.x;
                        am[2 * q + 1] = v.y;
                    }
                };
                // One marker of the walk.  ODD (HALF only): alpha-minus rebuilt from the even neighbour's row.
                auto smp_marker = [&](auto odd_tag, const double* row, int m) {
                    constexpr bool ODD = decltype(odd_tag)::value;
                    const int      ml  = m - first;
                    const double2  r_m = *(const double2*)(row + TAB_T);     // gap m-1 -> m
                    double         av[8];
                    if (ODD) {
                        double ep[8];
                        emission_from_row(row - TS, c, ep);
#pragma unroll
                        for (int j = 0; j < 8; j++) av[j] = am[j] * ep[j];
                        transition_scaled(av, r_m.x, r_m.y);
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; j++) av[j] = am[j];
                        asm volatile("" : "+v"(av[0]), "+v"(av[1]), "+v"(av[2]), "+v"(av[3]), "+v"(av[4]), "+v"(av[5]),
                                     "+v"(av[6]), "+v"(av[7]) : : "memory");
                        const int idx = HALF ? (ml >> 1) - 1 : ml - 1;
                        load_am(idx < 0 ? 0 : idx);
                    }
                    double e[8];
                    emission_from_row(row, c, e);
                    wave_lds_fence();                    // the previous marker's draws have read their chains
                    double* ap = al0 + s * TS + c.lo;
#pragma unroll
                    for (int j = 0; j < 8; j++) ap[j * 8] = av[j] * e[j];
                    wave_lds_fence();
                    double ratio;
                    x = smp_draw(al, x, rt0, rt1, smp_uniform(key, (unsigned long long)m), &ratio);
                    int ex;
                    pmant = frexp(pmant * ratio, &ex);
                    pexp += ex;
                    if (on) st[m] = (uint8_t)x;
                    rt0 = r_m.x;
                    rt1 = r_m.y;
                };
                load_raw<-1>(p, c, first + (ntile - 1) * 8, first, last, &raw);
                load_am(HALF ? ((last - first) >> 1) : (last - first));
                for (int t = ntile - 1; t >= 0; t--) {
                    const int m0 = first + t * 8;
                    produce_tile<false, false, TS>(p, c, tab, m0, last, raw, hom);
                    wave_lds_fence();
                    const int mend = (m0 + 7 < last) ? m0 + 7 : last;
                    int       i    = mend - m0;
                    if (HALF) {
                        if (!(i & 1)) {
                            smp_marker(even_t(), tab + i * TS, m0 + i);
                            i--;
                        }
                        for (; i >= 1; i -= 2) {
                            smp_marker(odd_t(), tab + i * TS, m0 + i);
                            smp_marker(even_t(), tab + (i - 1) * TS, m0 + i - 1);
                        }
                    } else {
                        for (; i >= 0; i--) smp_marker(even_t(), tab + i * TS, m0 + i);
                    }
                    wave_lds_fence();
                    if (t > 0) load_raw<-1>(p, c, m0 - 8, first, last, &raw);
                }
                if (on) {
                    const size_t o = ((size_t)jb.ind * K + k) * p.n_chrom + jb.chrom;
                    p.smp_shift[o] = sm;
                    if (p.smp_logp)
                        p.smp_logp[o] = pmant > 0.0 ? log(pmant) + (double)pexp * 0.69314718055994530942 : -INFINITY;
                }
            }
            continue;
        }
        // (the leave-one-out, origin and descent modes form no rows and are launched for their backward pass: they run with
        // KP_NO_DOSAGE, as the general kernel's crossover instantiation does)
        if (!LOO && !ORG && !DSC && (p.flags & KP_NO_DOSAGE)) continue;
        if (DSC && !any_alive) {
            // skipped, as the sweep skips it: all-zero rows, as the origin mode leaves them
            double* dr = p.org + ((size_t)jb.ind * p.n_markers + first) * 8;
            const int len = last - first + 1;
            for (int k = lane; k < len * 8; k += 64) dr[k] = 0.0;
            continue;
        }
        if (ORG && !any_alive) {
            // skipped, as the sweep skips it: all-zero rows, as the dosage rows are (origin_finish_kernel adds them as they are)
            double* og = p.org + ((size_t)jb.ind * p.n_markers + first) * 4;
            double* ob = p.obits + ((size_t)jb.ind * p.n_markers + first) * 6;
            const int len = last - first + 1;
            for (int k = lane; k < len * 4; k += 64) og[k] = 0.0;
            for (int k = lane; k < len * 6; k += 64) ob[k] = 0.0;
            continue;
        }
        if (LOO && !any_alive) {
            // skipped, as the sweep skips it: both rows marked for loo_finish_kernel (CNF2_IGNORED, left out of the sums)
            double* lo = p.loo + (size_t)jb.ind * p.n_markers + first;
            double* un = p.unl + (size_t)jb.ind * p.n_markers + first;
            for (int ml = lane; ml <= last - first; ml += 64) {
                lo[ml] = -1.0;
                un[ml] = -1.0;
            }
            continue;
        }

        // ---------------------------------------------------------------- backward + rows
        // Row of the reference: sum over (g, s, path) of val = exp(query - factor) by class
        // (cnF2freq.cpp:5499-5508, 3536).  With Fpre(m) = prod_{k<m} sum_k (forward normalisers) and
        // Bsuf(m) the backward ones, val summed over paths of class d and states is
        //     exp(-factor) * Fpre_s(m) * Bsuf_s(m) * sum_g alphaminus_s(g) beta_s(g) e^{(d)}_s(g).
        // Scales are carried as mantissa * 2^exponent; Fpre is rebuilt from the stored reciprocals.
        BwdState<NR> S;
#pragma unroll
        for (int j = 0; j < NR; j++) S.b[j] = 1.0;
        S.bmant = 1.0;
        S.bexpo = 0;
        S.bdead = false;
        S.fmant = mant;          // becomes Fpre(m) after multiplying the reciprocals of k >= m
        S.fexpo = expo;
        // exp(-factor) = xm * 2^xe; a job without a live chain has no rows (cnF2freq.cpp:5403)
        const double xm  = any_alive ? 1.0 / T : 0.0;
        const int    xe  = -emax;
        // (leave-one-out mode: every mode with a likelihood counts -- a marker that alone pushes a mode out of the band is what
        // the mode looks for)
        const bool   chain_on = alive && (LOO || !(tmine * 2.3538526683701998e17 < T));        // factor - fs > 40: cnF2freq.cpp:5420-5421
        // leave-one-out mode: 1 / (64 x analysed modes), the unlinked mean's divisor
        const double loo_k = LOO ? 1.0 / (double)(64 * (__builtin_popcountll(__ballot(c.active)) >> 3)) : 0.0;
        const double xo_w     = (STOREW == 4 && chain_on) ? tmine * xm : 0.0;           // crossover mode: P(mode s | data)
        // software pipeline: the spill row (and its reciprocals) is requested one row ahead, straight into
        // the registers it is used from; nothing else in the marker loop is a vector memory operation
        // (compact rows: two and three rows ahead, through a queue of registers, measured 2 - 3 % slower than one)
        auto load_row = [&](int idx) {
            const double* sp = spill + (size_t)idx * ROW;
#ifdef CNF2_X_NOLOAD     /* timing ablation only: results are wrong */
            if (idx >= 0) return;
#endif
            if constexpr (URow) {
                // the pair of the lane's class: four lanes an address, three lines a wave and row
                const d2v v = __builtin_nontemporal_load((const d2v*)(sp + uoff));
                S.am[0]     = v.x;
                S.am[1]     = v.y;
            } else {
#pragma unroll
                for (int k = 0; k < NR / 2; k++) {
                    const d2v v = __builtin_nontemporal_load((const d2v*)(sp + k * 128 + lane * 2));
                    S.am[2 * k]     = v.x;
                    S.am[2 * k + 1] = v.y;
                }
            }
            const double2 iv = *(const double2*)(sp + INV + 2 * s);
            S.inv_even       = iv.x;
            S.inv_odd        = iv.y;
        };
        S.inv_odd = 1.0;
        load_row(HALF ? ((last - first) >> 1) : (last - first));

        int cur_combo = 0;     // TIED: tie combination of the pass over the tile that is running
        // One marker of the backward pass.  ODD (HALF only): the marker's alpha-minus is rebuilt from the
        // row of its even neighbour.  LOADS: request the next spill row once this one has been used.
        auto marker = [&](auto odd_tag, double* row, int m, bool carried = false) {
            constexpr bool ODD = decltype(odd_tag)::value;
            const int      ml  = m - first;
            double         wj[NR];
            double         aw[STOREW == 2 || STOREW == 4 ? 8 : 1];  // turn-scan / crossover mode: alpha-minus of this marker, unscaled
            const double2 r_m = *(const double2*)(row + TAB_T);     // gap m-1 -> m
            double        inv_m;
            if (ODD) {
                // odd marker: alpha-minus(m) = T( alpha-minus(m-1) * e(m-1) * inv(m-1) ), exactly the
                // forward step (cnF2freq.cpp:2238-2367); marker m-1 is the previous row of this tile
                double ep[NR];
                emission_from_row(row - TS, c, ep);
                if (!TIED && STOREW != 4) {        // (TIED, crossover mode: the 16 registers are needed elsewhere; the even marker forms its own)
#pragma unroll
                    for (int j = 0; j < NR; j++) S.ec[j] = ep[j];
                }
#pragma unroll
                for (int j = 0; j < NR; j++) wj[j] = S.am[j] * ep[j];
                // the normaliser inv(m-1) is a per-chain scalar and everything below is linear in wj:
                // it is applied to the three class sums (`scale`) instead of to the eight states
                if constexpr (XPOSE) transition_xpose(wj, r_m.x, r_m.y, xb, lane);
                else if constexpr (UNI) transition_uniform(wj, r_m.x, r_m.y);
                else transition_scaled(wj, r_m.x, r_m.y);
                if constexpr (STOREW == 2 || STOREW == 4) {
#pragma unroll
                    for (int j = 0; j < 8; j++) aw[j] = wj[j];
                }
#pragma unroll
                for (int j = 0; j < NR; j++) wj[j] *= S.b[j];
                inv_m = S.inv_odd;
            } else {
                if constexpr (STOREW == 2 || STOREW == 4) {
#pragma unroll
                    for (int j = 0; j < 8; j++) aw[j] = S.am[j];
                }
#pragma unroll
                for (int j = 0; j < NR; j++) wj[j] = S.am[j] * S.b[j];
                inv_m = S.inv_even;
                // the row is used up: request the one below it (clamped at the chromosome start, where the
                // reload is harmless) so that a whole marker, or two, of arithmetic covers the latency.
                // The empty asm pins "last use, then reload" in that order: otherwise the loads are hoisted
                // above the products, land in fresh registers and are copied (and waited for) at once.
                if constexpr (NR == 8)
                    asm volatile("" : "+v"(wj[0]), "+v"(wj[1]), "+v"(wj[2]), "+v"(wj[3]), "+v"(wj[4]), "+v"(wj[5]),
                                 "+v"(wj[6]), "+v"(wj[7]), "+v"(inv_m) : : "memory");
                else asm volatile("" : "+v"(wj[0]), "+v"(wj[1]), "+v"(inv_m) : : "memory");
                const int idx = HALF ? (ml >> 1) - 1 : ml - 1;
                load_row(idx < 0 ? 0 : idx);
            }
            if (!HALF || !ODD || m == last) {     // skipped (odd) steps have normaliser 1
                // (so do the even markers between two rescalings: their stored reciprocal is exactly 1.  Updating the
                // scale only where a chain really was rescaled -- a wave-uniform branch -- was measured 2.4 % SLOWER
                // than this unconditional straight-line form)
                int ex;
                S.fmant = frexp(S.fmant * inv_m, &ex);
                S.fexpo += ex;
            }
            double n_tot = 0.0, n_a1 = 0.0, n_b1 = 0.0, n_2 = 0.0;
#ifdef CNF2_X_FUSEDACC   /* timing ablation only (tools/ablate_fused_acc.sh): results are wrong */
            double x_av[2], x_sb[2], x_t0[2], x_t1[2], x_cf[2];
#endif
            // TIED: the sums of the pair of tie combinations whose restricted tables the row holds (everything else at this
            // marker -- the posterior weights wj, the scale -- is the same for every combination)
            // (no rows asked for: no class sums, no restricted tables, no epilogue)
            // UNI, two registers: the four B-side class sums below (sb and sb1 for f = 0, 1) depend on the lane only through
            // its chain and state bit 0 -- wj does not depend on state bits 1 and 2, the tables are indexed by (f, s2, j) --
            // so the four lanes of a chain that share bit 0 would form the same four sums.  Lane kq (its state bits 1 and 2)
            // forms sum kq alone, the same multiply-adds on the same operands, and fetches the other three: cs[t] is sum
            // t = 2 f + (TAB_2 ? 1 : 0).  Every lane takes part, whatever its chain holds.
            double cs[4];
            if constexpr (UNI && NR == 2) {
                const int     kq = (c.lo >> 1) & 3;
                const double* Bk = row + ((kq & 1) ? TAB_2 : TAB_R) + ((1 << 5) | ((kq >> 1) << 4) | (c.s2 << 3));
                double        z  = 0.0;
#pragma unroll
                for (int j = 0; j < 8; j++) z += wj[j & 1] * Bk[j];
                // the pair (sums kq & 2 and kq & 2 | 1) first, then the other pair from the lane across state bit 2
                const bool   b0 = (kq & 1) != 0, b1 = (kq & 2) != 0;
                const double z1 = lane_flip_b1(z);
                const double pe = b0 ? z1 : z, po = b0 ? z : z1;
                const double qe = lane_flip_b2(pe), qo = lane_flip_b2(po);
                cs[0] = b1 ? qe : pe;
                cs[1] = b1 ? qo : po;
                cs[2] = b1 ? pe : qe;
                cs[3] = b1 ? po : qo;
            }
#pragma unroll 1
            for (int ko = 0; ko < (!ROWS ? 0 : (TIED ? 2 * TIE_KOFF : 1)); ko += TIE_KOFF)
#pragma unroll
            for (int f = 0; f < 2; f++) {
                // the lane's own line (its low bits index that half of the tables) and the line held in the registers:
                // A / B as printed, B / A in the transposed layout of an odd marker (n_a1 and n_b1 then swap roles,
                // which the class sums below do not notice: they use n_a1 + n_b1)
                constexpr bool T = XPOSE && ODD;
                const int     ia = ((T ? 1 : 0) << 5) | (f << 4) | ((T ? c.s2 : c.s1) << 3) | c.lo;
                const double* Br = row + ko + TAB_R + (((T ? 0 : 1) << 5) | (f << 4) | ((T ? c.s1 : c.s2) << 3));
                const double* B1 = row + ko + TAB_2 + (((T ? 0 : 1) << 5) | (f << 4) | ((T ? c.s1 : c.s2) << 3));
                const double  cf = row[TAB_C + f * 2 + c.s0];
                const double  av = cf * row[ko + TAB_R + ia], a1 = cf * row[ko + TAB_2 + ia];
                double        sb = 0.0, sb1 = 0.0;
                if constexpr (UNI && NR == 2) {
                    sb  = cs[2 * f];
                    sb1 = cs[2 * f + 1];
                } else {
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        sb += wj[j] * Br[j];
                        sb1 += wj[j] * B1[j];
                    }
                }
                n_tot += av * sb;
                n_a1 += a1 * sb;
                n_b1 += av * sb1;
                n_2 += a1 * sb1;
#ifdef CNF2_X_FUSEDACC
                if (WG) {
                    // the two HOMOZYGOUS probe contractions of phase B: stand-in tables of the same shape in the same row
                    const double* H0 = row + (((T ? 0 : 1) << 5) | (f << 4) | ((T ? c.s1 : c.s2) << 3));
                    double        t0 = 0.0, t1 = 0.0;
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        t0 += wj[j] * H0[j];
                        t1 += wj[j] * H0[j ^ 1];
                    }
                    x_av[f] = av;
                    x_sb[f] = sb;
                    x_t0[f] = t0;
                    x_t1[f] = t1;
                    x_cf[f] = cf;
                }
#endif
            }
            const double sc0   = ODD ? xm * S.inv_even : xm;
            const double scale = chain_on ? ldexp(sc0 * S.fmant * S.bmant, xe + S.fexpo + S.bexpo) : 0.0;
            double q2 = scale * n_2;
            double q1 = scale * (n_a1 + n_b1 - 2.0 * n_2);
            double q0 = scale * (n_tot - n_a1 - n_b1 + n_2);
#ifdef CNF2_X_FUSEDACC
            if (WG && (!TIED || cur_combo == 0)) {
                // phase B of acc_tile_kernel formed here: v (sum over s2), z (over s0 and s2), u (over the 32 lanes of a half)
                double*   wp = p.wbuf + ((size_t)job * p.wstride + ml) * 160;
                const int e0 = (c.s1 << 3) | c.lo;
                double    uu[16];
#pragma unroll
                for (int f = 0; f < 2; f++) {
                    const double k = scale * x_cf[f];
                    double       v = k * x_sb[f], z0 = k * x_t0[f], z1 = k * x_t1[f];
                    v += lane_xor32(v);
                    z0 += lane_xor32(z0);
                    z1 += lane_xor32(z1);
                    z0 += lane_xor8(z0);
                    z1 += lane_xor8(z1);
                    if (c.s2 == 0) wp[(f * 2 + c.s0) * 16 + e0] = v;
                    if (c.s2 == 0 && c.s0 == 0) {
                        wp[96 + (f * 2 + 0) * 16 + e0] = z0;
                        wp[96 + (f * 2 + 1) * 16 + e0] = z1;
                    }
                    const double ka = scale * x_av[f];
#pragma unroll
                    for (int j = 0; j < 8; j++) uu[f * 8 + j] = wj[j] * ka;
                }
                auto halve = [&](double a, double b, bool bit, int which) CNF2_LI_K {
                    const double keep = bit ? b : a, send = bit ? a : b;
                    return keep + (which == 0 ? lane_xor1(send) : (which == 1 ? lane_xor2(send) : (which == 2 ? lane_xor4(send) : lane_xor8(send))));
                };
                double h8[8], h4[4], h2[2];
#pragma unroll
                for (int k = 0; k < 8; k++) h8[k] = halve(uu[2 * k], uu[2 * k + 1], (lane & 1) != 0, 0);
#pragma unroll
                for (int k = 0; k < 4; k++) h4[k] = halve(h8[2 * k], h8[2 * k + 1], (lane & 2) != 0, 1);
#pragma unroll
                for (int k = 0; k < 2; k++) h2[k] = halve(h4[2 * k], h4[2 * k + 1], (lane & 4) != 0, 2);
                double h1v = halve(h2[0], h2[1], (lane & 8) != 0, 3);
                h1v += lane_xor16(h1v);
                if ((lane & 16) == 0) wp[64 + ((lane >> 3) & 1) * 16 + (c.s2 << 3) + (lane & 7)] = h1v;
            }
#else
            if constexpr (WG) if (!TIED || cur_combo == 0) {
                // accumulate mode: wg(s, g) = exp(scales - factor) alphaminus beta for the batched HOT LOOP 2 kernel
                // (the same in every tie combination)
                double* wp = p.wbuf + ((size_t)job * p.wstride + ml) * 512;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const d2v v = {scale != 0.0 ? scale * wj[2 * k] : 0.0, scale != 0.0 ? scale * wj[2 * k + 1] : 0.0};
                    __builtin_nontemporal_store(v, (d2v*)(wp + k * 128 + lane * 2));
                }
            }
#endif
            if constexpr (STOREW == 4) {
                // crossover mode, gap m -> m+1: al = alpha-minus e (up to a per-chain scalar), S.b = T' eb exactly, so the
                // normaliser D = <al, S.b> and the flipped masses carry the same scalars and the same dropped (1 - r)
                // constants; the flipped factor of bit t is t_t = r_t / (1 - r_t) of the gap (p.tq[m])
                // (the marker's emission is formed here for al and once more below for the beta step: not held across)
                if (m < last) {
                    double al[8], D = 0.0;
                    emission_from_row(row, c, al);
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        al[j] *= aw[j];
                        D += al[j] * S.b[j];
                    }
                    D = chain_sum(D);
                    const double2 tq = p.tq[m];
                    double        nn[6];
                    xo_numerators<true>(al, S.eb, tq.x, tq.y, nn);
                    xo_store(p, jb.ind, m, nn, tq.x, tq.y, (D > 0.0 && xo_w != 0.0) ? xo_w / D : 0.0, lane);
                } else xo_store_zero(p, jb.ind, m, lane);
            }
            // this marker's own emission is only needed for the beta step: formed here, after the sums, so
            // that it does not occupy registers across them
            double e[NR];
            if constexpr (XPOSE && ODD) emission_from_row_t(row, c, e);
            else if (!ODD && carried) {
#pragma unroll
                for (int j = 0; j < NR; j++) e[j] = S.ec[j];
            }
            else emission_from_row(row, c, e);
            if constexpr (LOO) {
                // leave-one-out mode: sum_g alphaminus beta with the row scale is L_s,-m / L, the mode's likelihood with this
                // marker's emission replaced by 1 over the total; the emission's own sum over the analysed modes is the
                // unlinked term.  The logarithms: loo_finish_kernel
                const double sw  = ((wj[0] + wj[1]) + (wj[2] + wj[3])) + ((wj[4] + wj[5]) + (wj[6] + wj[7]));
                const double rat = across_chains_sum(chain_sum(scale != 0.0 ? scale * sw : 0.0));    // (a chain that is off: 0, whatever it holds)
                const double es  = chain_sum(((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
                const double tot = across_chains_sum(c.active ? es : 0.0);
                if (lane == 0) {
                    const size_t o = (size_t)jb.ind * p.n_markers + m;
                    p.loo[o] = rat;
                    p.unl[o] = tot * loo_k;
                }
            }
            if constexpr (ORG) {
                // origin mode: gamma(s, g) = wg e as the placement mode stores it, summed here instead.  The register index j is
                // state bits 3-5, c.lo the lane's state bits 0-2 (state_lo, not the raw lane number).  A lane's four sums over
                // its registers: all of them, and those with bit 3, 4, 5 set; bits 0-2 select per lane.  Eight reductions over
                // the wave; the total of the four cells is the weight of the modes the rows count, and dividing by it is the
                // definition's renormalisation over those modes
                double gs = 0.0, g3 = 0.0, g4 = 0.0, g5 = 0.0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const double g = scale != 0.0 ? scale * wj[j] * e[j] : 0.0;    // (a chain that is off: 0, whatever it holds)
                    gs += g;
                    if (j & 1) g3 += g;
                    if (j & 2) g4 += g;
                    if (j & 4) g5 += g;
                }
                const bool   b0 = (c.lo & 1) != 0, b1 = (c.lo & 2) != 0, b2 = (c.lo & 4) != 0;
                const double g03 = gs - g3;
                const double k0 = across_chains_sum(chain_sum(b0 ? 0.0 : g03));
                const double k1 = across_chains_sum(chain_sum(b0 ? g03 : 0.0));
                const double k2 = across_chains_sum(chain_sum(b0 ? 0.0 : g3));
                const double k3 = across_chains_sum(chain_sum(b0 ? g3 : 0.0));
                const double t1 = across_chains_sum(chain_sum(b1 ? gs : 0.0));
                const double t2 = across_chains_sum(chain_sum(b2 ? gs : 0.0));
                const double t4 = across_chains_sum(chain_sum(g4));
                const double t5 = across_chains_sum(chain_sum(g5));
                if (lane == 0) {
                    const double tot = (k0 + k1) + (k2 + k3);
                    const double inv = tot > 0.0 ? 1.0 / tot : 0.0;
                    double*      og  = p.org + ((size_t)jb.ind * p.n_markers + m) * 4;
                    double*      ob  = p.obits + ((size_t)jb.ind * p.n_markers + m) * 6;
                    og[0] = k0 * inv;
                    og[1] = k1 * inv;
                    og[2] = k2 * inv;
                    og[3] = k3 * inv;
                    ob[0] = (k1 + k3) * inv;
                    ob[1] = t1 * inv;
                    ob[2] = t2 * inv;
                    ob[3] = (k2 + k3) * inv;
                    ob[4] = t4 * inv;
                    ob[5] = t5 * inv;
                }
            }
            if constexpr (DSC) {
                // descent mode: the origin mode's gamma(s, g) = wg e and its normaliser.  Per side a class k = 2 w + b: the
                // allele descends from that parent's par[.][w], strand b of that grandparent.  w is the parent's own meiosis
                // bit (0 or 3) and b the meiosis bit of the grandparent it selected (1 or 2 on the first side, 4 or 5 on the
                // second).  The register index j is state bits 3-5: a lane's four sums over its registers are the second
                // side's classes; its own state bits 0-2 (c.lo, not the raw lane number) select the one first-side class all
                // eight registers belong to.  The eight values are reduced together by halving: lane bit 0 keeps the odd or
                // the even ones and sends the others to its neighbour, then bit 1, then bit 2 (4 + 2 + 1 exchanges), which
                // leaves lane l of a chain with value l & 7 added over the chain's lanes; three more exchanges add the chains.
                // Lanes 0-7 then hold the row and store it, one value each
                double s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const double g = scale != 0.0 ? scale * wj[j] * e[j] : 0.0;    // (a chain that is off: 0, whatever it holds)
                    s2[(j & 1) ? 2 + ((j >> 2) & 1) : ((j >> 1) & 1)] += g;
                }
                const double gs = (s2[0] + s2[1]) + (s2[2] + s2[3]);
                const int    k1 = (c.lo & 1) ? 2 + ((c.lo >> 2) & 1) : ((c.lo >> 1) & 1);
                auto halve = [&](double a, double b, bool bit, int which) CNF2_LI_K {
                    const double keep = bit ? b : a, send = bit ? a : b;
                    return keep + (which == 0 ? lane_xor1(send) : (which == 1 ? lane_xor2(send) : lane_xor4(send)));
                };
                double h4[4], h2[2];
                h4[0] = halve(k1 == 0 ? gs : 0.0, k1 == 1 ? gs : 0.0, (lane & 1) != 0, 0);
                h4[1] = halve(k1 == 2 ? gs : 0.0, k1 == 3 ? gs : 0.0, (lane & 1) != 0, 0);
                h4[2] = halve(s2[0], s2[1], (lane & 1) != 0, 0);
                h4[3] = halve(s2[2], s2[3], (lane & 1) != 0, 0);
                h2[0] = halve(h4[0], h4[1], (lane & 2) != 0, 1);
                h2[1] = halve(h4[2], h4[3], (lane & 2) != 0, 1);
                const double dv = across_chains_sum(halve(h2[0], h2[1], (lane & 4) != 0, 2));
                // the normaliser is the origin mode's, the total of the first side's four cells: lanes 0-3 of a group of
                // eight add theirs, lanes 4-7 take it from lanes 3-0 (row_half_mirror)
                double tot = dv + lane_xor1(dv);
                tot += lane_xor2(tot);
                const double tmir = dpp_mov_all<0x141>(tot);
                if (lane & 4) tot = tmir;
                if (lane < 8) p.org[((size_t)jb.ind * p.n_markers + m) * 8 + lane] = tot > 0.0 ? dv * (1.0 / tot) : 0.0;
            }
            if constexpr (POST) {
                // placement mode: gamma(s, g) = wg e, the posterior of state g in mode s at this marker, where the accumulate
                // mode stores wg (same row, same layout); sums to the weight of the modes the rows count
                double* wp = p.wbuf + ((size_t)job * p.wstride + ml) * 512;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const d2v v = {scale != 0.0 ? scale * wj[2 * k] * e[2 * k] : 0.0,
                                   scale != 0.0 ? scale * wj[2 * k + 1] * e[2 * k + 1] : 0.0};
                    __builtin_nontemporal_store(v, (d2v*)(wp + k * 128 + lane * 2));
                }
            }
            if constexpr (STOREW == 2) {
                // turn-scan mode: A = alphaminus e and B = beta as held here, with the log2 of the scales that make them
                // absolute (alphaminus: Fpre, and the stored normaliser of the even neighbour for a rebuilt odd marker)
                double* wp = p.wbuf + ((size_t)job * p.wstride + ml) * CNF2_TURN_ROW;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const d2v va = {aw[2 * k] * e[2 * k], aw[2 * k + 1] * e[2 * k + 1]};
                    const d2v vb = {S.b[2 * k], S.b[2 * k + 1]};
                    __builtin_nontemporal_store(va, (d2v*)(wp + k * 128 + lane * 2));
                    __builtin_nontemporal_store(vb, (d2v*)(wp + 512 + k * 128 + lane * 2));
                }
                if (c.lo == 0) {
                    *(double2*)(wp + 1024 + 4 * s)     = make_double2((ODD ? S.inv_even : 1.0) * S.fmant, (double)S.fexpo);
                    *(double2*)(wp + 1024 + 4 * s + 2) = make_double2(S.bmant, (double)S.bexpo);
                }
            }
            // every lane parks its three class partials in this marker's row (all of it is dead by now:
            // tables, root weights and gap factors have been read); the tile epilogue sums them
            if (ROWS) {
                wave_lds_fence();
                row[lane]       = q0;
                row[64 + lane]  = q1;
                row[128 + lane] = q2;
            }
            // beta(m-1) = T( beta(m) * e(m) ); at the first marker the result is never used
#pragma unroll
            for (int j = 0; j < NR; j++) S.b[j] *= e[j];
            // (deferring this normaliser like the forward one was measured slower here: the row scale and the
            // emission of the next step would both wait for the reciprocal)
            if (!HALF || (!ODD && (ml & bmask) == 0)) {
                const double bsum = scale_chain<UNI>(S.b, &S.bmant, &S.bexpo, &S.bdead);
                if (HALF && __ballot(bsum > 0.0 && bsum * CNF2_RESCALE_GUARD < 1.0)) bmask = 1;
            }
            if constexpr (STOREW == 4) xo_copy(S.eb, S.b);
            if constexpr (XPOSE) transition_xpose(S.b, r_m.x, r_m.y, xb, lane);
            else if constexpr (UNI) transition_uniform(S.b, r_m.x, r_m.y);
            else transition_scaled(S.b, r_m.x, r_m.y);
        };
        if constexpr (REC) {
            load_rec<-1>(p, c, rec_row, first + (ntile - 1) * 8, first, last, load_root_allele(p, c, first + (ntile - 1) * 8, first, last), &rraw);
            ap_next = load_root_allele(p, c, first + (ntile - 2) * 8, first, last);
        } else load_raw<-1>(p, c, first + (ntile - 1) * 8, first, last, &raw);
        for (int t = ntile - 1; t >= 0; t--) {
            const int m0 = first + t * 8;
            // TIED: the state at the tile's start, restored for every combination: beta, the mantissas and the exponents from
            // LDS, the spill row in flight by asking for it again
            const int bmask0 = bmask;
            const bool bdead0 = S.bdead;
            if constexpr (TIED) {
                double* sv = tsave[wib] + lane;
#pragma unroll
                for (int j = 0; j < 8; j++) sv[j * 64] = S.b[j];
                sv[8 * 64] = S.bmant;
                sv[9 * 64] = S.fmant;
                sv[10 * 64] = __hiloint2double(S.bexpo, S.fexpo);
                double zero = 0.0;
                asm volatile("" : "+v"(zero));          // formed here: the compiler would keep (and spill) a 0.0 for the whole kernel
                if (lane < 24) tsum[wib][lane] = zero;
            }
          // TIED: the tie combinations two at a time (there are 2, 4 or 8): one pass over the tile per pair
          for (int combo = 0; combo < n_combo; combo += (TIED ? 2 : 1)) {
            const int tp = (int8_t)(my_ties & 255), tt = (int8_t)((my_ties >> 8) & 255), to = (int8_t)((my_ties >> 16) & 255);
            auto forces = [&](int k) {                                       // = part_forces(w, c.part, k, &c.pc)
                c.pc.force_par = tp < 0 ? -1 : ((k >> tp) & 1);
                c.pc.force_tr  = tt < 0 ? -1 : ((k >> tt) & 1);
                c.pc.force_ot  = to < 0 ? -1 : ((k >> to) & 1);
            };
            if (TIED) {
                cur_combo = combo;
                // the spill row of the tile's top marker once more (the first pass has it in flight from the tile
                // above): asked for here, so that the producer's work covers the latency
                if (combo > 0) load_row(HALF ? ((((m0 + 7 < last) ? m0 + 7 : last) - first) >> 1) : (((m0 + 7 < last) ? m0 + 7 : last) - first));
                forces(combo);
            }
            if constexpr (REC) {
                produce_row_rec<ROWS>(c, tab, m0 + c.mi <= last, rraw);
                // the next tile's inputs a whole tile ahead, as in the forward pass: this form has the registers to hold them
                // across the marker loop
                if (t > 0) {
                    load_rec<-1>(p, c, rec_row, m0 - 8, first, last, ap_next, &rraw);
                    ap_next = load_root_allele(p, c, m0 - 16, first, last);
                }
            } else
#ifdef CNF2_X_NOPRODUCE  /* timing ablation only: results are wrong */
            if (t == ntile - 1)
#endif
            {
                produce_tile<ROWS, TIED, TS>(p, c, tab, m0, last, raw, hom);
                if (TIED) {
                    forces(combo + 1);
                    produce_tile<true, TIED, TS, TIE_KOFF>(p, c, tab, m0, last, raw, hom);
                }
            }
            wave_lds_fence();
            const int mend = (m0 + 7 < last) ? m0 + 7 : last;
            if constexpr (TIED) {
                // (for the first combination too: nothing of the backward state is then live across the producer, whose tie
                // form needs the registers)
                const double* sv = tsave[wib] + lane;
#pragma unroll
                for (int j = 0; j < 8; j++) S.b[j] = sv[j * 64];
                S.bmant = sv[8 * 64];
                S.fmant = sv[9 * 64];
                S.bexpo = __double2hiint(sv[10 * 64]);
                S.fexpo = __double2loint(sv[10 * 64]);
                S.bdead = bdead0;
                bmask   = bmask0;
            }
            int       i    = mend - m0;                 // local index; its parity is the parity of m - first
            if (HALF) {
                if (!(i & 1)) {                         // an even top marker: only the last tile of a chromosome
                    marker(even_t(), tab + i * TS, m0 + i);
                    i--;
                }
                for (; i >= 1; i -= 2) {
                    marker(odd_t(), tab + i * TS, m0 + i);
                    marker(even_t(), tab + (i - 1) * TS, m0 + i - 1, !TIED && STOREW != 4);
                }
            } else {
                for (; i >= 0; i--) marker(even_t(), tab + i * TS, m0 + i);
            }
            wave_lds_fence();
            // next tile's inputs: requested here, before the epilogue's LDS work (holding them across the
            // whole marker loop costs more in registers than the extra latency it hides; measured)
#ifndef CNF2_X_NOPRODUCE
            // (TIED: the tile's own inputs once more for its next combination, rather than 29 registers held across the
            // marker loop; the tile's start goes through an empty asm so that the eight addresses are formed here, not kept)
            if (TIED) {
                int m0x = (combo + 2 < n_combo) ? m0 : m0 - 8;
                asm volatile("" : "+s"(m0x));
                if (t > 0 || combo + 2 < n_combo) load_raw<-1>(p, c, m0x, first, last, &raw);
            } else if constexpr (REC) {
            } else if (t > 0) load_raw<-1>(p, c, m0 - 8, first, last, &raw);
#endif
            // tile epilogue: lanes (marker mi = lane >> 3, eighth sub = lane & 7) add up the 3 x 64 partials
            // of the tile's markers, lane sub == 0 normalises and stores the row
            if (ROWS) {
                const int     mi2 = lane >> 3, sub = lane & 7;
                const double* red = tab + mi2 * TS + sub * 8;
                double        d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
                for (int i2 = 0; i2 < 8; i2++) {
                    d0 += red[i2];
                    d1 += red[64 + i2];
                    d2 += red[128 + i2];
                }
                d0 = chain_sum(d0);
                d1 = chain_sum(d1);
                d2 = chain_sum(d2);
                if (TIED) {
                    // add this combination's class sums to the tile's; the rows are written after the last one
                    if (sub == 0) {
                        d0 += tsum[wib][mi2 * 3 + 0];
                        d1 += tsum[wib][mi2 * 3 + 1];
                        d2 += tsum[wib][mi2 * 3 + 2];
                        tsum[wib][mi2 * 3 + 0] = d0;
                        tsum[wib][mi2 * 3 + 1] = d1;
                        tsum[wib][mi2 * 3 + 2] = d2;
                    }
                }
                // class 0 and 1 are formed by inclusion-exclusion of non-negative sums: a true zero can come
                // out as -1e-16; the reference adds non-negative terms (cnF2freq.cpp:3536), so clamp
                d0 = fmax(d0, 0.0);
                d1 = fmax(d1, 0.0);
                d2 = fmax(d2, 0.0);
                if (sub == 0 && m0 + mi2 <= last && combo + (TIED ? 2 : 1) >= n_combo) {
                    if (!(p.flags & KP_RAW_DOSAGE)) {
                        const double tsum = d0 + d1 + d2;
                        const double inv  = tsum > 0.0 ? 1.0 / tsum : 0.0;
                        d0 *= inv;
                        d1 *= inv;
                        d2 *= inv;
                    }
                    double* out = p.dosage + ((size_t)jb.ind * p.n_markers + (m0 + mi2)) * 3;
                    out[0] = d0;
                    out[1] = d1;
                    out[2] = d2;
                }
            }
            wave_lds_fence();
          }
        }
    }
    if (stamp && fresh_lane() == 0) {
        p.clock_out[0] = __builtin_readcyclecounter() - t_shader;
        p.clock_out[1] = wall_clock64() - t_wall;
    }
}

// =====================================================================================
// Four uniform windows to a wave: the plain half-spill sweep of fb_fast_kernel's UNI / REC instantiation for groups of four
// jobs of one chromosome whose windows have their lines among the launch's records (p.pjobs).  In a uniform
// window the four lanes of a chain that differ in state bits 1 and 2 run the recursion on the same numbers, and
// transition_uniform, chain_total and the reductions across chains never exchange over those bits: here each of the four carries
// another job (cnf2_lane.h upk_job).  Per job every floating-point operation is the UNI instantiation's, on the same operands in
// the same order -- the same bits -- and a wave-wide instruction of the recursion serves four jobs.  What was wave-wide and
// would tie a job to its neighbours (dense rescaling, the count of analysed modes) is taken per job.
//   tile:     2 markers x 4 jobs, table row = marker_in_tile << 2 | job (the 8 rows of fb_packed_kernel); the producer lane
//             (part, row) works on the window of its row's job
//   rows:     a lane forms the four B-side class sums of its job itself and then stands, one after the other, for the four
//             lanes (upk_virtual_lane) that form the row partials in the job's own sweep; they are parked in the job's table row
//             at those lanes' places, and the UNI tile epilogue adds them up in its order
//   spill:    UPK_SPILL_ROW doubles per marker pair, the four compact rows side by side (the same bytes per unit)
// =====================================================================================
__global__ __launch_bounds__(CNF2_BLOCK, CNF2_UNI_MIN_BLOCKS) void fb_unipack_kernel(KernelParams p)
{
    constexpr int NR = 2, ROW = UPK_SPILL_ROW, TS = TAB_STRIDE;
    __shared__ __attribute__((aligned(16))) double lds[CNF2_WAVES_PER_BLOCK][8 * TS];

    const int wib   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave  = blockIdx.x * CNF2_WAVES_PER_BLOCK + wib;
    const int nwave = gridDim.x * CNF2_WAVES_PER_BLOCK;
    double*   spill = p.spill + (size_t)wave * p.spill_stride;
    const bool stamp = p.clock_out != nullptr && wave == 0;
    unsigned long long t_shader = 0, t_wall = 0;
    if (stamp) {
        t_shader = __builtin_readcyclecounter();
        t_wall   = wall_clock64();
    }

    auto take_job = [&](int strided) {
        if (!p.job_next) return strided;
        int j = 0;
        if (fresh_lane() == 0) j = atomicAdd(p.job_next, 1);
        return __builtin_amdgcn_readfirstlane(j);
    };
    for (int job = take_job(wave); job < p.n_pjobs; job = take_job(job + nwave)) {
        const int       lane = fresh_lane();
        const PackedJob& pj  = p.pjobs[job];
        // the wave's tables and the windows, from scalars the compiler cannot see through: as values of the whole kernel their
        // vector copies would be kept (in scratch) across every job
        int           wq   = wib;
        const Window* wins = p.windows;
        KernelParams  pq   = p;        // (for the producer's loads: the rows' base likewise)
        asm volatile("" : "+s"(wq), "+s"(wins), "+s"(pq.allele8));
        double* const tab = lds[wq];
        const int first = __builtin_amdgcn_readfirstlane(pj.first), last = __builtin_amdgcn_readfirstlane(pj.last);
        const int chrom = __builtin_amdgcn_readfirstlane(pj.chrom);
        const int ntile = (last - first + 2) >> 1;
        // producer role: part x (marker in tile, job) on the window of the row's job
        FastCtx cp;
        cp.part = lane >> 3;
        cp.mi   = lane & 7;
        const int pmt  = cp.mi >> 2;
        const int moff = pmt - cp.mi;          // load_rec and load_root_allele look at marker m0 + c.mi: this lane's is m0 + pmt
        uint32_t  rec_row;                     // line * n_markers of this lane's line
        {
            const int    pind = pj.ind[cp.mi & 3];
            const Window wp   = wins[pind];
            make_part(wp, cp.part, &cp.pc, &cp.row_par, &cp.row_tr, &cp.row_ot);
            cp.row_root = wp.row[0];
            rec_row     = (uint32_t)p.line_keys[2 * (size_t)pind + (cp.pc.P ? 1 : 0)] * (uint32_t)p.n_markers;
        }
        cp.idx_base = part_entry_index(cp.part, 0);
        cp.idx_k01  = part_entry_index(cp.part, 1) - cp.idx_base;
        cp.idx_k10  = part_entry_index(cp.part, 2) - cp.idx_base;
        // recursion role: chain s of job rj, class b0 (the tables of a uniform window do not depend on state bits 1 and 2:
        // the lane reads them at those bits clear)
        const int s = lane >> 3, rj = upk_job(lane), b0 = state_lo(lane) & 1;
        const int ind = pj.ind[rj];
        const int eind = pj.ind[s & 3];        // epilogue role: the individual of table row lane >> 3 = (marker in tile) << 2 | job
        FastCtx   c;
        c.s0 = s & 1;
        c.s1 = (s >> 1) & 1;
        c.s2 = (s >> 2) & 1;
        c.lo = b0;
        {
            const Window& w = wins[ind];
            c.active        = !(s & w.shiftignore) && s < w.shiftend;
        }
        const size_t je = (size_t)ind * p.n_chrom + chrom;
        if (p.path_log && s == 0 && b0 == 0) p.path_log[je] = 2;
        // the lanes of this lane's job, for what the one-job sweep asks of the whole wave: its two places among the 8 lanes of a
        // chain; a ballot is folded over the chains on the scalar unit first
        const unsigned jbits = (1u << state_lo(2 * rj)) | (1u << state_lo(2 * rj + 1));
        auto any_in_job = [&](unsigned long long ballot) {
            unsigned t = (unsigned)ballot | (unsigned)(ballot >> 32);
            t |= t >> 16;
            t |= t >> 8;
            return (t & jbits) != 0;
        };
        double* const myrow0 = tab + rj * TS;            // the job's row of the tile's even marker
        double* const myrow1 = myrow0 + 4 * TS;          // and of its odd one
        const bool uspill = !(p.flags & KP_NO_DOSAGE);   // (a launch that forms no rows reads no spill row: nobody writes one)
        const int  uoff   = upk_spill_value(lane);
        const int  ioff   = upk_spill_inv(rj, s);
        const bool iwr    = b0 == 0 && uspill;

        using odd_t  = std::integral_constant<bool, true>;
        using even_t = std::integral_constant<bool, false>;

        // ---------------------------------------------------------------- forward (fb_fast_kernel's fwd_step, HALF, UNI)
        double a[NR];
#pragma unroll
        for (int j = 0; j < NR; j++) a[j] = 1.0 / 64.0;
        double mant = 1.0;
        int    expo = 0;
        bool   dead = false;
        double pend = 1.0;
        int    rmask = CNF2_RESCALE_MASK, bmask = CNF2_RESCALE_MASK;   // per job
        auto fwd_step = [&](auto odd_tag, const double* row, int m) {
            constexpr bool ODD = decltype(odd_tag)::value;
            double         e[NR];
            emission_from_row(row, c, e, pend);
            const double2 r  = *(const double2*)(row + TAB_T);
            const int     ml = m - first;
            double*       sp = spill + (size_t)(ml >> 1) * ROW;
            if (!ODD) {
                const d2v v = {a[0], a[1]};
                if (uspill) __builtin_nontemporal_store(v, (d2v*)(sp + uoff));
            }
#pragma unroll
            for (int j = 0; j < NR; j++) a[j] *= e[j];
            pend = 1.0;
            // a job renormalises exactly where it would alone: every lane computes, the job's lanes take the result
            const bool norm_here = m == last || (!ODD && (ml & rmask) == 0);
            if (__ballot(norm_here)) {
                double       mt = mant;
                int          ex = expo;
                bool         dd = dead;
                const double inv = chain_normaliser<true>(a, &mt, &ex, &dd);
                mant = norm_here ? mt : mant;
                expo = norm_here ? ex : expo;
                dead = norm_here ? dd : dead;
                pend = norm_here ? inv : 1.0;
                if (any_in_job(__ballot(norm_here && inv > CNF2_RESCALE_GUARD))) rmask = 1;
                if (iwr && (!ODD || norm_here)) sp[ioff + (ODD ? 1 : 0)] = pend;
            } else if (!ODD) {
                if (iwr) sp[ioff] = 1.0;
            }
            if (m < last) transition_uniform(a, r.x, r.y);
        };
        RawRec  rraw;
        uint8_t ap_next;
        load_rec<0>(pq, cp, rec_row, first + moff, first, last, load_root_allele(pq, cp, first + moff, first, last), &rraw);
        ap_next = load_root_allele(pq, cp, first + 2 + moff, first, last);
        for (int t = 0; t < ntile; t++) {
            const int m0 = first + t * 2;
            produce_row_rec<false, true>(cp, tab, m0 + pmt <= last, rraw);
            // (unconditional: behind a window's end the clamps reload its last tile.  Under a condition the loaded values reach
            // the carried registers through a copy, and that copy waits for every load right here)
            load_rec<0>(pq, cp, rec_row, m0 + 2 + moff, first, last, ap_next, &rraw);
            ap_next = load_root_allele(pq, cp, m0 + 4 + moff, first, last);
            wave_lds_fence();
            fwd_step(even_t(), myrow0, m0);
            if (m0 < last) fwd_step(odd_t(), myrow1, m0 + 1);
            wave_lds_fence();
        }

        // ---------------------------------------------------------------- likelihoods (per job: the reductions across chains
        // pair lanes of equal lane & 7)
        const bool   alive  = c.active && !dead;
        const double emaxd  = across_chains_max(alive ? (double)expo : -1e300);
        const bool   any_alive = emaxd > -1e299;
        const int    emax   = any_alive ? (int)emaxd : 0;
        int          dsh    = expo - emax;
        dsh                 = dsh < -2000 ? -2000 : dsh;
        const double tmine  = alive ? ldexp(mant, dsh) : 0.0;
        const double T      = across_chains_sum(tmine);
        {
            const int n_active = __builtin_popcountll(__ballot(c.active) & ((unsigned long long)jbits * 0x0101010101010101ull)) >> 1;
            if (b0 == 0) {
                p.factors[je * 8 + s] = mant;
                p.fexp[je * 8 + s]    = alive ? expo : (c.active ? CNF2_LEXP_DEAD : CNF2_LEXP_IGNORED);
            }
            if (s == 0 && b0 == 0) {
                p.loglik[je] = any_alive ? T : (double)n_active;
                p.lexp[je]   = any_alive ? emax : CNF2_LEXP_DEAD;
            }
        }
        if (p.flags & KP_NO_DOSAGE) continue;

        // ---------------------------------------------------------------- backward + rows (fb_fast_kernel's marker, HALF, UNI)
        BwdState<NR> S;
#pragma unroll
        for (int j = 0; j < NR; j++) S.b[j] = 1.0;
        S.bmant = 1.0;
        S.bexpo = 0;
        S.bdead = false;
        S.fmant = mant;
        S.fexpo = expo;
        const double xm  = any_alive ? 1.0 / T : 0.0;
        const int    xe  = -emax;
        const bool   chain_on = alive && !(tmine * 2.3538526683701998e17 < T);        // factor - fs > 40: cnF2freq.cpp:5420-5421
        auto load_row = [&](int idx) {
            const double* sp = spill + (size_t)idx * ROW;
            const d2v     v  = __builtin_nontemporal_load((const d2v*)(sp + uoff));
            S.am[0]          = v.x;
            S.am[1]          = v.y;
            const double2 iv = *(const double2*)(sp + ioff);
            S.inv_even       = iv.x;
            S.inv_odd        = iv.y;
        };
        S.inv_odd = 1.0;
        load_row((last - first) >> 1);

        auto marker = [&](auto odd_tag, double* row, int m, bool carried = false) {
            constexpr bool ODD = decltype(odd_tag)::value;
            const int      ml  = m - first;
            double         wj[NR];
            const double2  r_m = *(const double2*)(row + TAB_T);     // gap m-1 -> m
            double         inv_m;
            if (ODD) {
                double ep[NR];
                emission_from_row(row - 4 * TS, c, ep);             // the even marker's row of this job
#pragma unroll
                for (int j = 0; j < NR; j++) S.ec[j] = ep[j];
#pragma unroll
                for (int j = 0; j < NR; j++) wj[j] = S.am[j] * ep[j];
                transition_uniform(wj, r_m.x, r_m.y);
#pragma unroll
                for (int j = 0; j < NR; j++) wj[j] *= S.b[j];
                inv_m = S.inv_odd;
            } else {
#pragma unroll
                for (int j = 0; j < NR; j++) wj[j] = S.am[j] * S.b[j];
                inv_m = S.inv_even;
                asm volatile("" : "+v"(wj[0]), "+v"(wj[1]), "+v"(inv_m) : : "memory");
                const int idx = (ml >> 1) - 1;
                load_row(idx < 0 ? 0 : idx);
            }
            if (!ODD || m == last) {
                int ex;
                S.fmant = frexp(S.fmant * inv_m, &ex);
                S.fexpo += ex;
            }
            // the four B-side class sums of the job, z[2 f + (TAB_2 ? 1 : 0)]: the chains the UNI instantiation shares out over
            // the four lanes, each formed here by the one lane
            double        z[4];
            const double* Bs = row + ((1 << 5) | (c.s2 << 3));
#pragma unroll
            for (int kq = 0; kq < 4; kq++) {
                const double* Bk = Bs + ((kq & 1) ? TAB_2 : TAB_R) + ((kq >> 1) << 4);
                double        zz = 0.0;
#pragma unroll
                for (int j = 0; j < 8; j++) zz += wj[j & 1] * Bk[j];
                z[kq] = zz;
            }
            const double sc0   = ODD ? xm * S.inv_even : xm;
            const double scale = chain_on ? ldexp(sc0 * S.fmant * S.bmant, xe + S.fexpo + S.bexpo) : 0.0;
            const double cf0 = row[TAB_C + 0 + c.s0], cf1 = row[TAB_C + 2 + c.s0];
            double       q[4][3];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                double n_tot = 0.0, n_a1 = 0.0, n_b1 = 0.0, n_2 = 0.0;
#pragma unroll
                for (int f = 0; f < 2; f++) {
                    const int    ia = (f << 4) | (c.s1 << 3) | b0 | (v << 1);
                    const double cf = f ? cf1 : cf0;
                    const double av = cf * row[TAB_R + ia], a1 = cf * row[TAB_2 + ia];
                    const double sb = z[2 * f], sb1 = z[2 * f + 1];
                    n_tot += av * sb;
                    n_a1 += a1 * sb;
                    n_b1 += av * sb1;
                    n_2 += a1 * sb1;
                }
                q[v][2] = scale * n_2;
                q[v][1] = scale * (n_a1 + n_b1 - 2.0 * n_2);
                q[v][0] = scale * (n_tot - n_a1 - n_b1 + n_2);
            }
            double e[NR];
            if (!ODD && carried) {
#pragma unroll
                for (int j = 0; j < NR; j++) e[j] = S.ec[j];
            }
            else emission_from_row(row, c, e);
            // the partials into the job's row, where the lanes of its own sweep would park theirs
            wave_lds_fence();
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int vl = upk_virtual_lane(lane, v);
                row[vl]       = q[v][0];
                row[64 + vl]  = q[v][1];
                row[128 + vl] = q[v][2];
            }
#pragma unroll
            for (int j = 0; j < NR; j++) S.b[j] *= e[j];
            const bool scale_here = !ODD && (ml & bmask) == 0;      // per job
            if (!ODD && __ballot(scale_here)) {
                double bb[NR] = {S.b[0], S.b[1]};
                double bm = S.bmant;
                int    be = S.bexpo;
                bool   bd = S.bdead;
                const double bsum = scale_chain<true>(bb, &bm, &be, &bd);
#pragma unroll
                for (int j = 0; j < NR; j++) S.b[j] = scale_here ? bb[j] : S.b[j];
                S.bmant = scale_here ? bm : S.bmant;
                S.bexpo = scale_here ? be : S.bexpo;
                S.bdead = scale_here ? bd : S.bdead;
                if (any_in_job(__ballot(scale_here && bsum > 0.0 && bsum * CNF2_RESCALE_GUARD < 1.0))) bmask = 1;
            }
            transition_uniform(S.b, r_m.x, r_m.y);
        };
        {
            const int mtop = first + (ntile - 1) * 2;
            load_rec<-1>(pq, cp, rec_row, mtop + moff, first, last, load_root_allele(pq, cp, mtop + moff, first, last), &rraw);
            ap_next = load_root_allele(pq, cp, mtop - 2 + moff, first, last);
        }
        // epilogue role: row mi2 = (marker in tile) << 2 | job
        const int    mi2 = lane >> 3, sub = lane & 7;
        for (int t = ntile - 1; t >= 0; t--) {
            const int m0 = first + t * 2;
            produce_row_rec<true, true>(cp, tab, m0 + pmt <= last, rraw);
            load_rec<-1>(pq, cp, rec_row, m0 - 2 + moff, first, last, ap_next, &rraw);      // (unconditional, as forward)
            ap_next = load_root_allele(pq, cp, m0 - 4 + moff, first, last);
            wave_lds_fence();
            if (m0 < last) {
                marker(odd_t(), myrow1, m0 + 1);
                marker(even_t(), myrow0, m0, true);
            } else marker(even_t(), myrow0, m0);
            wave_lds_fence();
            // tile epilogue, as fb_fast_kernel's: lanes (row mi2, eighth sub) add up the 3 x 64 partials of the tile's rows
            {
                const double* red = tab + mi2 * TS + sub * 8;
                double        d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
                for (int i2 = 0; i2 < 8; i2++) {
                    d0 += red[i2];
                    d1 += red[64 + i2];
                    d2 += red[128 + i2];
                }
                d0 = chain_sum(d0);
                d1 = chain_sum(d1);
                d2 = chain_sum(d2);
                d0 = fmax(d0, 0.0);
                d1 = fmax(d1, 0.0);
                d2 = fmax(d2, 0.0);
                if (sub == 0 && m0 + (mi2 >> 2) <= last) {
                    if (!(p.flags & KP_RAW_DOSAGE)) {
                        const double tsum = d0 + d1 + d2;
                        const double inv  = tsum > 0.0 ? 1.0 / tsum : 0.0;
                        d0 *= inv;
                        d1 *= inv;
                        d2 *= inv;
                    }
                    // (the row's address is formed here, from a value the compiler cannot see through: hoisted out of the tile
                    // loop it would live, in scratch, across the whole backward pass)
                    int ei = eind;
                    asm volatile("" : "+v"(ei));
                    double* out = p.dosage + ((size_t)ei * p.n_markers + (m0 + (mi2 >> 2))) * 3;
                    out[0] = d0;
                    out[1] = d1;
                    out[2] = d2;
                }
            }
            wave_lds_fence();
        }
    }
    if (stamp && fresh_lane() == 0) {
        p.clock_out[0] = __builtin_readcyclecounter() - t_shader;
        p.clock_out[1] = wall_clock64() - t_wall;
    }
}

// =====================================================================================
// Eight uniform windows to a wave: fb_unipack_kernel's sweep for pairs of its groups (p.pjobs[2 e], p.pjobs[2 e + 1]) whose eight
// windows have all eight shift modes analysed (shiftignore == 0, shiftend == 8; pair_uniform_groups).  On line records the
// unrestricted table is one value per part whatever the parent's shift bit, so the chains of a job with equal s0 see the same
// emissions and carry the same alpha, beta and scales: the lanes that differ in s1 take another job as well (cnf2_lane.h
// up8_*).  Per job every floating-point operation is fb_unipack_kernel's, on the same operands in the same order.
//   tile:     backward: 1 marker x 8 jobs, table row = job; the producer lane is (part, job).  Forward: CNF2_UP8_FWD_TILE
//             markers x 8 jobs of compact slots (cnf2_lane.h up8_fwd_*), over the same region
//   rows:     a lane forms the four B-side class sums of (s0, s2) once, takes its b0 partner's, and adds up the eight partials
//             of one chain (s0, s1 = its b0, s2) in registers, in the order of a one-job sweep's tile epilogue; the job's eight
//             chains are then added across lanes (s0, s1, s2: chain_sum's tree) and the job's lead lane stores the row
//             (cnf2_lane.h up8_sum_*).  Nothing is written to the table rows behind the producer: two fences a marker.
//             CNF2_UP8_ROW_SUMS == 0 (A/B): a lane forms the partials of its class for s1 = 1 and then s1 = 0, parks them in
//             the job's row in two steps (up8_park), each over what nobody reads any more, and the lanes (row, eighth) of a
//             tile epilogue add them up once per marker: five fences a marker
//   rebuild:  the odd marker's rebuild starts from alpha x emission of the even marker, which the forward pass spills beside
//             alpha (the even marker's row does not exist yet when the odd one is worked on); the even marker forms its
//             emission from its own row
//   spill:    UP8_SPILL_ROW doubles per marker pair, stored by the lanes with s2 = 0
// =====================================================================================
static_assert(TAB_R == 72 && TAB_2 == 136 && TAB_STRIDE >= 200, "up8_park (cnf2_lane.h) is written for this row layout");
static_assert(TAB_R % 2 == 0 && TAB_2 % 2 == 0 && TAB_STRIDE % 2 == 0, "the A-side runs of a chain (up8_sum_run) are read 16 bytes at a time");
// 1: a lane adds up the row partials of one chain in registers; 0: the partials are parked in the table row for an epilogue (A/B)
#ifndef CNF2_UP8_ROW_SUMS
#define CNF2_UP8_ROW_SUMS 1
#endif
// 1: the gap's factors of the wave's marker through the scalar cache; 0: a vector load, every lane the same address (A/B)
#ifndef CNF2_UP8_SCALAR_GAP
#define CNF2_UP8_SCALAR_GAP 1
#endif
// 1: the root's sure, hw and allele byte are loaded once a tile of eight markers and staged in the LDS (cnf2_lane.h
// up8_stage_*); 0: every producer lane loads them at every marker (A/B).  _FWD, _BWD: each pass alone (A/B)
#ifndef CNF2_UP8_ROOT_STAGE
#define CNF2_UP8_ROOT_STAGE 1
#endif
#ifndef CNF2_UP8_ROOT_STAGE_FWD
#define CNF2_UP8_ROOT_STAGE_FWD CNF2_UP8_ROOT_STAGE
#endif
#ifndef CNF2_UP8_ROOT_STAGE_BWD
#define CNF2_UP8_ROOT_STAGE_BWD CNF2_UP8_ROOT_STAGE
#endif
// markers to a forward tile (cnf2_lane.h up8_fwd_*); 1: the forward pass on one table row a marker, as the backward pass (A/B)
#ifndef CNF2_UP8_FWD_TILE
#define CNF2_UP8_FWD_TILE 8
#endif
// markers of a tile whose slots a recursion lane reads at a time, in front of their steps (ten doubles a marker)
#ifndef CNF2_UP8_FWD_READ
#define CNF2_UP8_FWD_READ 2
#endif
static_assert(CNF2_UP8_FWD_TILE == 1 || (CNF2_UP8_FWD_TILE >= 2 && CNF2_UP8_FWD_TILE % 2 == 0), "a forward tile holds an even number of markers");
static_assert(CNF2_UP8_FWD_TILE == 1 || up8_fwd_buffers(CNF2_UP8_FWD_TILE, 8 * TAB_STRIDE) * CNF2_UP8_FWD_TILE * UP8_FWD_MARKER <= 8 * TAB_STRIDE,
              "the forward tiles live in the wave's eight table rows");
// The slot of (marker, job) of a forward tile from the root's data and the record of the lane's line: emtab_part_rec's value
// of the lane's part (one for all eight unrestricted entries), the root weights and the gap's factors, each by the lane that
// stores it in a table row (produce_row_rec).  slot: the marker's 128 doubles; the lane's job is c.mi.
__device__ __forceinline__ void produce_slot_rec(const FastCtx& c, double* slot, const RawRec& raw)
{
    const Slot root = unpack_slot(raw.ap, raw.s0, raw.s1, raw.hw);
    LineRec rec;
    rec.Bp   = raw.Bp;
    rec.Cp   = raw.Cp;
    rec.Kp   = raw.Kp;
    rec.t0   = raw.t0;
    rec.t1   = raw.t1;
    rec.oo   = raw.oo;
    rec.bits = raw.bits;
    double  cw[2];
    double* d = slot + up8_fwd_at(0, c.mi, 0);
    emtab_part_rec<false, true>(c.pc.P, c.pc.f, root, rec,
                                [&](int, int e, double v) {
                                    if (e == 0) d[up8_fwd_at(0, 0, up8_fwd_part(c.part))] = v;
                                },
                                cw);
    if ((c.part & 5) == 0) {
        d[up8_fwd_at(0, 0, up8_fwd_weight(c.pc.f, 0))] = cw[0];
        d[up8_fwd_at(0, 0, up8_fwd_weight(c.pc.f, 1))] = cw[1];
    }
    if (c.part == 0) {
        d[up8_fwd_at(0, 0, up8_fwd_gap(0))] = raw.tq0;
        d[up8_fwd_at(0, 0, up8_fwd_gap(1))] = raw.tq1;
    }
}
// Root staging (cnf2_lane.h up8_stage_*): what lane (t = c.part, job = c.mi) loads once a tile for the
// producer lanes of (marker t of the tile, job), clamped to the window as load_rec clamps, and where it goes in the LDS
struct StagedRoot {
    double2  su;
    double   hw;
    uint32_t ap;
};
__device__ __forceinline__ void load_stage(const KernelParams& p, const FastCtx& c, int m, int lo_m, int hi_m, StagedRoot* s)
{
    const __attribute__((address_space(1))) uint8_t* a8 = (const __attribute__((address_space(1))) uint8_t*)p.allele8;
    const size_t i = (size_t)c.row_root * p.n_markers + clamp_marker(m, lo_m, hi_m);
    s->su = p.sure[i];
    s->hw = p.hw[i];
    s->ap = a8[i];
}
// forward: e = the entry of (t, job)
__device__ __forceinline__ void store_stage_fwd(double* e, const StagedRoot& s)
{
    *(double2*)(e + UP8_STAGE_SURE)    = s.su;
    e[UP8_STAGE_HW]                    = s.hw;
    *(uint32_t*)(e + UP8_STAGE_ALLELE) = s.ap;
}
// backward: row = the job's table row
__device__ __forceinline__ void store_stage_bwd(double* row, int buf, int t, const StagedRoot& s)
{
    *(double2*)(row + (buf ? up8_stage_bwd_sure(1, 0) : up8_stage_bwd_sure(0, 0)) + 8 * t) = s.su;
    row[(buf ? up8_stage_bwd_hw(1, 0) : up8_stage_bwd_hw(0, 0)) + 8 * t]                   = s.hw;
    ((uint8_t*)(row + up8_stage_bwd_alleles(0) + buf))[t]                                  = (uint8_t)s.ap;
}
static_assert(up8_stage_bwd_sure(0, 3) == up8_stage_bwd_sure(0, 0) + 24 && up8_stage_bwd_hw(1, 3) == up8_stage_bwd_hw(1, 0) + 24 &&
              up8_stage_bwd_alleles(1) == up8_stage_bwd_alleles(0) + 1, "store_stage_bwd and the staged readers step by marker and by buffer");
static_assert(up8_stage_bwd_alleles(1) < TAB_R && up8_stage_bwd_alleles(0) >= TAB_T + 2, "the allele bytes sit behind the gap's factors");
// What a forward step of the eights reads, from the job's table row or from its slot of a forward tile.  The slot's emission
// is emission_from_row's expression on the same values (N = 2, s1 = 0, lo = the class): the same products fuse.
struct Up8FwdRow {
    const double*  row;
    const FastCtx& c;
    __device__ __forceinline__ void emission(double (&e)[2], double k) const { emission_from_row(row, c, e, k); }
    __device__ __forceinline__ double2 gap() const { return *(const double2*)(row + TAB_T); }
};
// (the slot's ten values of the lane are read when the object is made, so that the caller can place the reads of several
// markers in front of their steps: behind a step's branches each slot is a round trip of its own in the recursion's chain)
struct Up8FwdSlot {
    double w0, a0, w1, a1, B0[2], B1[2], g0, g1;
    Up8FwdSlot() = default;
    // a, w: parts (f = 0, class) and root weight c_0(s0) of the lane; b: part 4 of the slot
    __device__ __forceinline__ Up8FwdSlot(const double* a, const double* w, const double* b)
    {
        constexpr int F = up8_fwd_at(0, 0, 2);         // from f = 0 to f = 1: two parts, or two weights, on
        w0 = w[0];
        a0 = a[0];
        w1 = w[F];
        a1 = a[F];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            B0[j] = b[up8_fwd_at(0, 0, j)];
            B1[j] = b[F + up8_fwd_at(0, 0, j)];
        }
        g0 = b[up8_fwd_at(0, 0, up8_fwd_gap(0) - 4)];
        g1 = b[up8_fwd_at(0, 0, up8_fwd_gap(1) - 4)];
    }
    __device__ __forceinline__ void emission(double (&e)[2], double k) const
    {
        const double cA0 = w0 * a0 * k;
        const double cA1 = w1 * a1 * k;
#pragma unroll
        for (int j = 0; j < 2; j++) e[j] = cA0 * B0[j] + cA1 * B1[j];
    }
    __device__ __forceinline__ double2 gap() const { return make_double2(g0, g1); }
};
__global__ __launch_bounds__(CNF2_BLOCK, CNF2_UNI_MIN_BLOCKS) void fb_unipack8_kernel(KernelParams p)
{
    constexpr int  NR = 2, ROW = UP8_SPILL_ROW, TS = TAB_STRIDE;
    constexpr bool SG = CNF2_UP8_SCALAR_GAP != 0;
    __shared__ __attribute__((aligned(16))) double lds[CNF2_WAVES_PER_BLOCK][8 * TS];

    const int wib   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave  = blockIdx.x * CNF2_WAVES_PER_BLOCK + wib;
    const int nwave = gridDim.x * CNF2_WAVES_PER_BLOCK;
    double*   spill = p.spill + (size_t)wave * p.spill_stride;
    const bool stamp = p.clock_out != nullptr && wave == 0;
    unsigned long long t_shader = 0, t_wall = 0;
    if (stamp) {
        t_shader = __builtin_readcyclecounter();
        t_wall   = wall_clock64();
    }

    auto take_job = [&](int strided) {
        if (!p.job_next) return strided;
        int j = 0;
        if (fresh_lane() == 0) j = atomicAdd(p.job_next, 1);
        return __builtin_amdgcn_readfirstlane(j);
    };
    for (int job = take_job(wave); job < p.n_pjobs; job = take_job(job + nwave)) {
        const int        lane = fresh_lane();
        const PackedJob* pj   = p.pjobs + 2 * (size_t)job;      // the eight's two fours
        // (scalars the compiler cannot see through, as in fb_unipack_kernel)
        int           wq   = wib;
        const Window* wins = p.windows;
        KernelParams  pq   = p;
        asm volatile("" : "+s"(wq), "+s"(wins), "+s"(pq.allele8));
        double* const tab = lds[wq];
        const int first = __builtin_amdgcn_readfirstlane(pj[0].first), last = __builtin_amdgcn_readfirstlane(pj[0].last);
        const int chrom = __builtin_amdgcn_readfirstlane(pj[0].chrom);
        // producer role: part x job, one marker at a time
        FastCtx cp;
        cp.part = lane >> 3;
        cp.mi   = lane & 7;
        const int moff = -cp.mi;               // load_rec and load_root_allele look at marker m0 + c.mi: this lane's is m0
        uint32_t  rec_row;                     // line * n_markers of this lane's line
        {
            const int    pind = pj[cp.mi >> 2].ind[cp.mi & 3];
            const Window wp   = wins[pind];
            make_part(wp, cp.part, &cp.pc, &cp.row_par, &cp.row_tr, &cp.row_ot);
            cp.row_root = wp.row[0];
            rec_row     = (uint32_t)p.line_keys[2 * (size_t)pind + (cp.pc.P ? 1 : 0)] * (uint32_t)p.n_markers;
        }
        cp.idx_base = part_entry_index(cp.part, 0);
        cp.idx_k01  = part_entry_index(cp.part, 1) - cp.idx_base;
        cp.idx_k10  = part_entry_index(cp.part, 2) - cp.idx_base;
        // recursion role: the chains (s0, s1 = 0 and 1, s2) of job rj, class b0 (the unrestricted table does not depend on a
        // parent's shift bit: the lane reads it at s1 = 0)
        const int rj = up8_job(lane), b0 = up8_b0(lane);
        const int ind = pj[rj >> 2].ind[rj & 3];
#if !CNF2_UP8_ROW_SUMS
        const int eind = pj[lane >> 5].ind[(lane >> 3) & 3];    // epilogue role: the individual of table row lane >> 3 = job
#endif
        FastCtx   c;
        c.s0 = up8_s0(lane);
        c.s1 = 0;
        c.s2 = up8_s2(lane);
        c.lo = b0;
        c.active = true;                       // (eligibility: all eight modes of every window)
        const size_t je = (size_t)ind * p.n_chrom + chrom;
        const bool   jlead = c.s0 == 0 && c.s2 == 0 && b0 == 0;
        if (p.path_log && jlead) p.path_log[je] = 2;
        // the lanes of this lane's job, for what the one-job sweep asks of the whole wave: its two places among the 8 lanes of
        // a group, in the groups of its half of the wave; a ballot's halves are folded on the scalar unit first
        const unsigned jbits = (1u << state_lo(2 * (rj & 3))) | (1u << state_lo(2 * (rj & 3) + 1));
        auto any_in_job = [&](unsigned long long ballot) {
            unsigned tl = (unsigned)ballot, th = (unsigned)(ballot >> 32);
            tl |= tl >> 16;
            tl |= tl >> 8;
            th |= th >> 16;
            th |= th >> 8;
            return (((rj & 4) ? th : tl) & jbits) != 0;
        };
        double* const myrow = tab + rj * TS;             // the job's row
        const bool uspill = !(p.flags & KP_NO_DOSAGE);   // (a launch that forms no rows reads no spill row: nobody writes one)
        const int  uoff   = up8_spill_value(lane);
        const int  ioff   = up8_spill_inv(rj, c.s0);
        const bool vwr    = up8_spill_writer(lane) && uspill;
        const bool iwr    = b0 == 0 && vwr;

        using odd_t  = std::integral_constant<bool, true>;
        using even_t = std::integral_constant<bool, false>;

        // ---------------------------------------------------------------- forward (fb_unipack_kernel's fwd_step)
        double a[NR];
#pragma unroll
        for (int j = 0; j < NR; j++) a[j] = 1.0 / 64.0;
        double mant = 1.0;
        int    expo = 0;
        bool   dead = false;
        double pend = 1.0;
        int    rmask = CNF2_RESCALE_MASK, bmask = CNF2_RESCALE_MASK;   // per job
        auto fwd_step = [&](auto odd_tag, const auto& src, int m) {
            constexpr bool ODD = decltype(odd_tag)::value;
            double         e[NR];
            src.emission(e, pend);
            const double2 r  = src.gap();
            const int     ml = m - first;
            double*       sp = spill + (size_t)(ml >> 1) * ROW;
            if (!ODD) {
                // alpha, and alpha x the marker's emission: what the backward pass's rebuild of the odd marker starts from
                double ep[NR];
                src.emission(ep, 1.0);
                const d2v v = {a[0], a[1]};
                const d2v w = {a[0] * ep[0], a[1] * ep[1]};
                if (vwr) {
                    __builtin_nontemporal_store(v, (d2v*)(sp + uoff));
                    __builtin_nontemporal_store(w, (d2v*)(sp + UP8_SPILL_EMIT + uoff));
                }
            }
#pragma unroll
            for (int j = 0; j < NR; j++) a[j] *= e[j];
            pend = 1.0;
            // a job renormalises exactly where it would alone: every lane computes, the job's lanes take the result
            const bool norm_here = m == last || (!ODD && (ml & rmask) == 0);
            if (__ballot(norm_here)) {
                double       mt = mant;
                int          ex = expo;
                bool         dd = dead;
                const double inv = chain_normaliser<true>(a, &mt, &ex, &dd);
                mant = norm_here ? mt : mant;
                expo = norm_here ? ex : expo;
                dead = norm_here ? dd : dead;
                pend = norm_here ? inv : 1.0;
                if (any_in_job(__ballot(norm_here && inv > CNF2_RESCALE_GUARD))) rmask = 1;
                if (iwr && (!ODD || norm_here)) sp[ioff + (ODD ? 1 : 0)] = pend;
            } else if (!ODD) {
                if (iwr) sp[ioff] = 1.0;
            }
            if (m < last) transition_uniform(a, r.x, r.y);
        };
        RawRec  rraw;
        uint8_t ap_next;
        if constexpr (CNF2_UP8_FWD_TILE == 1) {
            // A/B form: a table row per marker, as the backward pass keeps them
            const Up8FwdRow src{myrow, c};
            load_rec<0, SG>(pq, cp, rec_row, first + moff, first, last, load_root_allele(pq, cp, first + moff, first, last), &rraw);
            ap_next = load_root_allele(pq, cp, first + 1 + moff, first, last);
            for (int m = first; m <= last; m++) {
                produce_row_rec<false, true>(cp, tab, true, rraw);
                // (unconditional, as in fb_unipack_kernel: no copy, so no wait, between these loads and the next marker's producer)
                load_rec<0, SG>(pq, cp, rec_row, m + 1 + moff, first, last, ap_next, &rraw);
                ap_next = load_root_allele(pq, cp, m + 2 + moff, first, last);
                wave_lds_fence();
                if ((m - first) & 1) fwd_step(odd_t(), src, m);
                else fwd_step(even_t(), src, m);
                wave_lds_fence();
            }
        } else {
            // compact tiles of T markers (cnf2_lane.h up8_fwd_*): the producer lanes walk the tile's markers with the records of two
            // markers in flight, one fence, and the recursion lanes take T steps with none in between (a second fence behind
            // them where the region holds one tile only).  T is even: the parity of a marker in its window is that of its place
            // in the tile.  The loads behind a window's end are clamped to its last marker and their slots are never used.
            constexpr int T = CNF2_UP8_FWD_TILE, REGION = 8 * TS;
            // the lane's places in the slot of (marker 0 of buffer 0, its job): the A-side parts of its class, the root weights
            // of its s0, and the B-side parts with the gap's factors behind them
            const double* const qa = tab + up8_fwd_at(0, rj, up8_fwd_part(b0));
            const double* const qc = tab + up8_fwd_at(0, rj, up8_fwd_weight(0, c.s0));
            const double* const qb = tab + up8_fwd_at(0, rj, up8_fwd_part(4));
            // root staging (cnf2_lane.h up8_stage_*): tile k's root data sits in buffer k & 1 behind the tile.  As a staging lane
            // this one is (marker cp.part of a tile, job cp.mi); as a producer it reads the entries of its job
            constexpr bool STAGE = CNF2_UP8_ROOT_STAGE_FWD != 0 && T == UP8_STAGE_T && up8_fwd_buffers(T, REGION) == 1 &&
                                   up8_stage_fwd_room(T, REGION) >= 2 * UP8_STAGE_BUFFER;
            constexpr int SB = UP8_STAGE_BUFFER, SM = 8 * UP8_STAGE_ENTRY;      // from buffer to buffer, from marker to marker
            double* const       sgw = tab + up8_stage_fwd_at(T, REGION, 0, cp.part, cp.mi);
            const double* const sgr = tab + up8_stage_fwd_at(T, REGION, 0, 0, cp.mi);
            auto allele_at = [&](const double* e) { return (uint8_t) * (const uint32_t*)(e + UP8_STAGE_ALLELE); };
            StagedRoot sg;
            RawRec     rr[2];
            uint8_t    ap[2];
            if constexpr (STAGE) {
                // (the region is the wave's to write: the job before ended behind a fence)
                StagedRoot sg1;
                load_stage(pq, cp, first + cp.part, first, last, &sg);
                load_stage(pq, cp, first + T + cp.part, first, last, &sg1);
                store_stage_fwd(sgw, sg);
                store_stage_fwd(sgw + SB, sg1);
                load_stage(pq, cp, first + 2 * T + cp.part, first, last, &sg);
                wave_lds_fence();
                load_rec<0, SG, false>(pq, cp, rec_row, first + moff, first, last, allele_at(sgr), &rr[0]);
                load_rec<0, SG, false>(pq, cp, rec_row, first + 1 + moff, first, last, allele_at(sgr + SM), &rr[1]);
                ap[0] = allele_at(sgr + 2 * SM);
                ap[1] = allele_at(sgr + 3 * SM);
            } else {
                load_rec<0, SG>(pq, cp, rec_row, first + moff, first, last, load_root_allele(pq, cp, first + moff, first, last), &rr[0]);
                load_rec<0, SG>(pq, cp, rec_row, first + 1 + moff, first, last, load_root_allele(pq, cp, first + 1 + moff, first, last), &rr[1]);
                ap[0] = load_root_allele(pq, cp, first + 2 + moff, first, last);
                ap[1] = load_root_allele(pq, cp, first + 3 + moff, first, last);
            }
#if CNF2_X_ROOTONCE & 1    /* timing ablation only: results are wrong (a tile's markers all take the root's data of its first) */
            static_assert(!STAGE, "the ablation is of the per-marker loads");
            RawRoot rt_cur, rt_nxt;
            load_root(pq, cp, first + moff, first, last, &rt_cur);
            load_root(pq, cp, first + T + moff, first, last, &rt_nxt);
#endif
            int tile = 0;
            for (int m0 = first; m0 <= last; m0 += T, tile++) {
                const int toff = up8_fwd_tile(T, REGION, tile);
                if constexpr (STAGE) {
                    // the root of marker t + 1 is read in front of marker t's stores, the allele byte that the record's address
                    // takes four markers ahead as the byte's load was: in this tile's buffer or, from its end on, in the next one's
                    const double* const cur = sgr + (tile & 1) * SB;
                    const double* const nxt = sgr + ((tile & 1) ^ 1) * SB;
                    double2 su = *(const double2*)(cur + UP8_STAGE_SURE);
                    double  hw = cur[UP8_STAGE_HW];
#pragma unroll
                    for (int t = 0; t < T; t++) {
                        rr[t & 1].s0 = su.x;
                        rr[t & 1].s1 = su.y;
                        rr[t & 1].hw = hw;
                        if (t + 1 < T) {
                            su = *(const double2*)(cur + (t + 1) * SM + UP8_STAGE_SURE);
                            hw = cur[(t + 1) * SM + UP8_STAGE_HW];
                        }
                        produce_slot_rec(cp, tab + toff + up8_fwd_at(t, 0, 0), rr[t & 1]);
                        load_rec<0, SG, false>(pq, cp, rec_row, m0 + t + 2 + moff, first, last, ap[t & 1], &rr[t & 1]);
                        ap[t & 1] = allele_at(t + 4 < T ? cur + (t + 4) * SM : nxt + (t + 4 - T) * SM);
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < T; t++) {
#if CNF2_X_ROOTONCE & 1
                        rt_cur.into(&rr[t & 1]);
                        produce_slot_rec(cp, tab + toff + up8_fwd_at(t, 0, 0), rr[t & 1]);
                        load_rec<0, SG, false>(pq, cp, rec_row, m0 + t + 2 + moff, first, last, rt_cur.ap, &rr[t & 1]);
#else
                        produce_slot_rec(cp, tab + toff + up8_fwd_at(t, 0, 0), rr[t & 1]);
                        // (unconditional, as above; what is asked for here is produced two markers on)
                        load_rec<0, SG>(pq, cp, rec_row, m0 + t + 2 + moff, first, last, ap[t & 1], &rr[t & 1]);
                        ap[t & 1] = load_root_allele(pq, cp, m0 + t + 4 + moff, first, last);
#endif
                    }
                }
#if CNF2_X_ROOTONCE & 1
                rt_cur = rt_nxt;
                load_root(pq, cp, m0 + 2 * T + moff, first, last, &rt_nxt);
#endif
                wave_lds_fence();
                if constexpr (STAGE) {
                    // tile + 2 goes where this tile's root data was, its readers a fence behind and its own a fence (the one
                    // behind the steps) ahead; tile + 3 has the steps and a tile's producer to arrive
                    store_stage_fwd(sgw + (tile & 1) * SB, sg);
                    load_stage(pq, cp, m0 + 3 * T + cp.part, first, last, &sg);
                }
                // (CNF2_UP8_FWD_READ markers' slots are read in front of the steps that use them: every slot of the tile has been
                // produced, whether its marker is inside the window or not)
                auto slot_at = [&](int t) {
                    const int o = toff + up8_fwd_at(t, 0, 0);
                    return Up8FwdSlot(qa + o, qc + o, qb + o);
                };
                constexpr int RD = CNF2_UP8_FWD_READ < T ? CNF2_UP8_FWD_READ : T;
                static_assert(T % RD == 0, "a forward tile is read in equal parts");
#pragma unroll
                for (int t0 = 0; t0 < T; t0 += RD) {
                    Up8FwdSlot src[RD];
#pragma unroll
                    for (int t = 0; t < RD; t++) src[t] = slot_at(t0 + t);
#pragma unroll
                    for (int t = 0; t < RD; t++) {
                        if (t0 + t == 0 || m0 + t0 + t <= last) {
                            if ((t0 + t) & 1) fwd_step(odd_t(), src[t], m0 + t0 + t);
                            else fwd_step(even_t(), src[t], m0 + t0 + t);
                        }
                    }
                }
                // (one buffer: the next tile goes over this one.  Two: over the one before, whose readers are a fence behind)
                if (up8_fwd_buffers(T, REGION) == 1) wave_lds_fence();
            }
            // the tiles' last readers are done: the region goes to the backward pass's rows, or to the next job's first tile
            if (up8_fwd_buffers(T, REGION) == 2) wave_lds_fence();
        }

        // ---------------------------------------------------------------- likelihoods (per job: its two distinct chains sit
        // eight lanes apart; the sum over its eight chains doubles their sum twice, which is exact)
        const bool   alive  = !dead;
        const double emine  = alive ? (double)expo : -1e300;
        const double emaxd  = fmax(emine, lane_xor8(emine));
        const bool   any_alive = emaxd > -1e299;
        const int    emax   = any_alive ? (int)emaxd : 0;
        int          dsh    = expo - emax;
        dsh                 = dsh < -2000 ? -2000 : dsh;
        const double tmine  = alive ? ldexp(mant, dsh) : 0.0;
        double       T      = tmine + lane_xor8(tmine);
        T += T;
        T += T;
        if (b0 == 0 && c.s2 == 0) {
#pragma unroll
            for (int s1 = 0; s1 < 2; s1++) {
                const int s = c.s0 | (s1 << 1);
#pragma unroll
                for (int s2 = 0; s2 < 2; s2++) {
                    p.factors[je * 8 + (s | (s2 << 2))] = mant;
                    p.fexp[je * 8 + (s | (s2 << 2))]    = alive ? expo : CNF2_LEXP_DEAD;
                }
            }
        }
        if (jlead) {
            p.loglik[je] = any_alive ? T : 8.0;          // (the count of analysed modes)
            p.lexp[je]   = any_alive ? emax : CNF2_LEXP_DEAD;
        }
        if (p.flags & KP_NO_DOSAGE) continue;

        // ---------------------------------------------------------------- backward + rows (fb_unipack_kernel's marker)
        BwdState<NR> S;
#pragma unroll
        for (int j = 0; j < NR; j++) S.b[j] = 1.0;
        S.bmant = 1.0;
        S.bexpo = 0;
        S.bdead = false;
        S.fmant = mant;
        S.fexpo = expo;
        const double xm  = any_alive ? 1.0 / T : 0.0;
        const int    xe  = -emax;
        const bool   chain_on = alive && !(tmine * 2.3538526683701998e17 < T);        // factor - fs > 40: cnF2freq.cpp:5420-5421
        // S.am holds what a marker starts from: alpha x emission of the pair's even marker at an odd marker, alpha at an even
        // one, and S.inv_* the pair's two reciprocals.  The marker loop asks for them one marker ahead, at one place outside the
        // odd / even branch, into nx_*: it takes them over at the top of the next iteration, the one place that waits for them
        // (assigned inside the branches they were awaited at each branch's end, behind the marker that asked for them)
        double nx_am[NR], nx_inv_even, nx_inv_odd;
        auto ask_spill = [&](int mn) {          // for marker first + mn (mn = -1 below the window: its first pair again)
            const double* sp = spill + (size_t)(mn < 0 ? 0 : mn >> 1) * ROW;
            const d2v     v  = __builtin_nontemporal_load((const d2v*)(sp + ((mn & 1) ? UP8_SPILL_EMIT : 0) + uoff));
            nx_am[0]         = v.x;
            nx_am[1]         = v.y;
            const double2 iv = *(const double2*)(sp + ioff);
            nx_inv_even      = iv.x;
            nx_inv_odd       = iv.y;
        };
        auto take_spill = [&]() {
#pragma unroll
            for (int j = 0; j < NR; j++) S.am[j] = nx_am[j];
            S.inv_even = nx_inv_even;
            S.inv_odd  = nx_inv_odd;
        };
        ask_spill(last - first);

        auto marker = [&](auto odd_tag, double* row, int m) {
            constexpr bool ODD = decltype(odd_tag)::value;
            const int      ml  = m - first;
            double         wj[NR];
            const double2  r_m = *(const double2*)(row + TAB_T);     // gap m-1 -> m
            double         inv_m;
            if (ODD) {
#pragma unroll
                for (int j = 0; j < NR; j++) wj[j] = S.am[j];
                transition_uniform(wj, r_m.x, r_m.y);
#pragma unroll
                for (int j = 0; j < NR; j++) wj[j] *= S.b[j];
                inv_m = S.inv_odd;
            } else {
#pragma unroll
                for (int j = 0; j < NR; j++) wj[j] = S.am[j] * S.b[j];
                inv_m = S.inv_even;
            }
            if (!ODD || m == last) {
                int ex;
                S.fmant = frexp(S.fmant * inv_m, &ex);
                S.fexpo += ex;
            }
            // the four B-side class sums of (s0, s2), z[2 f + (TAB_2 ? 1 : 0)]
            double        z[4];
            const double* Bs = row + ((1 << 5) | (c.s2 << 3));
#pragma unroll
            for (int kq = 0; kq < 4; kq++) {
                const double* Bk = Bs + ((kq & 1) ? TAB_2 : TAB_R) + ((kq >> 1) << 4);
                double        zz = 0.0;
#pragma unroll
                for (int j = 0; j < 8; j++) zz += wj[j & 1] * Bk[j];
                z[kq] = zz;
            }
            const double sc0   = ODD ? xm * S.inv_even : xm;
            const double scale = chain_on ? ldexp(sc0 * S.fmant * S.bmant, xe + S.fexpo + S.bexpo) : 0.0;
            const double cf0 = row[TAB_C + 0 + c.s0], cf1 = row[TAB_C + 2 + c.s0];
            double e[NR];
            emission_from_row(row, c, e);
#if CNF2_UP8_ROW_SUMS
            // the b0 pair's class sums by absolute class, and the eight partials of the lane's chain (cnf2_lane.h up8_sum_*),
            // each formed in front of its addition.  A partial is the parked form's, expression for expression; it is made
            // opaque before it is added so that its product with `scale` is rounded, as a parked one is.
            double zb[2][4];
#pragma unroll
            for (int kq = 0; kq < 4; kq++) {
                const double zp = lane_xor1(z[kq]);
                zb[0][kq] = b0 ? zp : z[kq];
                zb[1][kq] = b0 ? z[kq] : zp;
            }
            const double* const A = row + up8_sum_run(0, up8_sum_s1(lane));
            double d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
            for (int ip = 0; ip < 4; ip++) {
                // two places that follow each other share v: their entries are the two classes of one 16-byte read a run
                const int v = up8_place_v(2 * ip);
                static_assert(up8_place_v(0) == up8_place_v(1) && up8_place_v(2) == up8_place_v(3) && up8_place_v(4) == up8_place_v(5) &&
                              up8_place_v(6) == up8_place_v(7), "a pair of places is one v");
                double2 ar[2], a2[2];
#pragma unroll
                for (int f = 0; f < 2; f++) {
                    ar[f] = *(const double2*)(A + TAB_R + (up8_sum_run(f, 0) | (v << 1)));
                    a2[f] = *(const double2*)(A + TAB_2 + (up8_sum_run(f, 0) | (v << 1)));
                }
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int b = up8_place_b(2 * ip + k);
                    double    n_tot = 0.0, n_a1 = 0.0, n_b1 = 0.0, n_2 = 0.0;
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        const double cf = f ? cf1 : cf0;
                        const double av = cf * (b ? ar[f].y : ar[f].x), a1 = cf * (b ? a2[f].y : a2[f].x);
                        const double sb = zb[b][2 * f], sb1 = zb[b][2 * f + 1];
                        n_tot += av * sb;
                        n_a1 += a1 * sb;
                        n_b1 += av * sb1;
                        n_2 += a1 * sb1;
                    }
                    double q2 = scale * n_2;
                    double q1 = scale * (n_a1 + n_b1 - 2.0 * n_2);
                    double q0 = scale * (n_tot - n_a1 - n_b1 + n_2);
                    asm("" : "+v"(q0), "+v"(q1), "+v"(q2));
                    d0 += q0;
                    d1 += q1;
                    d2 += q2;
                }
            }
            // the job's eight chains, as chain_sum adds the lanes of an epilogue's row: s0, s1, s2, each from the lane
            // up8_partner(lane, level) of level 0, 1, 2 (cnf2_lane.h; tests/test_uniform_pack8_rows_host.py holds it to that tree)
            static_assert((up8_partner(0, 0) ^ 0) == 8 && (up8_partner(63, 0) ^ 63) == 8, "level 0 is lane_xor8");
            static_assert((up8_partner(0, 1) ^ 0) == 1 && (up8_partner(63, 1) ^ 63) == 1, "level 1 is lane_xor1");
            static_assert((up8_partner(0, 2) ^ 0) == 16 && (up8_partner(63, 2) ^ 63) == 16, "level 2 is lane_xor16");
            d0 += lane_xor8(d0);
            d1 += lane_xor8(d1);
            d2 += lane_xor8(d2);
            d0 += lane_xor1(d0);
            d1 += lane_xor1(d1);
            d2 += lane_xor1(d2);
            d0 += lane_xor16(d0);
            d1 += lane_xor16(d1);
            d2 += lane_xor16(d2);
            d0 = fmax(d0, 0.0);
            d1 = fmax(d1, 0.0);
            d2 = fmax(d2, 0.0);
            if (jlead) {
                if (!(p.flags & KP_RAW_DOSAGE)) {
                    const double tsum = d0 + d1 + d2;
                    const double inv  = tsum > 0.0 ? 1.0 / tsum : 0.0;
                    d0 *= inv;
                    d1 *= inv;
                    d2 *= inv;
                }
                // (the row's address is formed here, from a value the compiler cannot see through)
                int ei = ind;
                asm volatile("" : "+v"(ei));
                double* out = p.dosage + ((size_t)ei * p.n_markers + m) * 3;
                out[0] = d0;
                out[1] = d1;
                out[2] = d2;
            }
#else
            // the partials of s1 = 1, then of s1 = 0, into the job's row where the epilogue looks for them
#ifdef CNF2_X_NOPARK
            double x_sum[3];
#endif
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int s1 = 1 - h;
                double    q[4][3];
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    double n_tot = 0.0, n_a1 = 0.0, n_b1 = 0.0, n_2 = 0.0;
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        const int    ia = (f << 4) | (s1 << 3) | b0 | (v << 1);
                        const double cf = f ? cf1 : cf0;
                        const double av = cf * row[TAB_R + ia], a1 = cf * row[TAB_2 + ia];
                        const double sb = z[2 * f], sb1 = z[2 * f + 1];
                        n_tot += av * sb;
                        n_a1 += a1 * sb;
                        n_b1 += av * sb1;
                        n_2 += a1 * sb1;
                    }
                    q[v][2] = scale * n_2;
                    q[v][1] = scale * (n_a1 + n_b1 - 2.0 * n_2);
                    q[v][0] = scale * (n_tot - n_a1 - n_b1 + n_2);
#ifdef CNF2_X_NOPARK     /* timing ablation only: results are wrong (no parking stores, no read-back, none of their fences) */
#pragma unroll
                    for (int k = 0; k < 3; k++) x_sum[k] = (h == 0 && v == 0 ? 0.0 : x_sum[k]) + q[v][k];
#endif
                }
#ifndef CNF2_X_NOPARK
                wave_lds_fence();
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const int vl = up8_virtual_lane(lane, s1, v);
                    row[up8_park(0, vl)] = q[v][0];
                    row[up8_park(1, vl)] = q[v][1];
                    row[up8_park(2, vl)] = q[v][2];
                }
#endif
            }
#ifdef CNF2_X_NOPARK
            {   // (the epilogue below on this lane's own sums, so that they never leave registers)
                const double d0 = fmax(chain_sum(x_sum[0]), 0.0), d1 = fmax(chain_sum(x_sum[1]), 0.0), d2 = fmax(chain_sum(x_sum[2]), 0.0);
                const double tsum = d0 + d1 + d2;
                const double inv  = (p.flags & KP_RAW_DOSAGE) ? 1.0 : (tsum > 0.0 ? 1.0 / tsum : 0.0);
                if ((lane & 7) == 0) {
                    int ei = eind;
                    asm volatile("" : "+v"(ei));
                    double* out = p.dosage + ((size_t)ei * p.n_markers + m) * 3;
                    out[0] = d0 * inv;
                    out[1] = d1 * inv;
                    out[2] = d2 * inv;
                }
            }
#endif
#endif
#pragma unroll
            for (int j = 0; j < NR; j++) S.b[j] *= e[j];
            const bool scale_here = !ODD && (ml & bmask) == 0;      // per job
            if (!ODD && __ballot(scale_here)) {
                double bb[NR] = {S.b[0], S.b[1]};
                double bm = S.bmant;
                int    be = S.bexpo;
                bool   bd = S.bdead;
                const double bsum = scale_chain<true>(bb, &bm, &be, &bd);
#pragma unroll
                for (int j = 0; j < NR; j++) S.b[j] = scale_here ? bb[j] : S.b[j];
                S.bmant = scale_here ? bm : S.bmant;
                S.bexpo = scale_here ? be : S.bexpo;
                S.bdead = scale_here ? bd : S.bdead;
                if (any_in_job(__ballot(scale_here && bsum > 0.0 && bsum * CNF2_RESCALE_GUARD < 1.0))) bmask = 1;
            }
            transition_uniform(S.b, r_m.x, r_m.y);
        };
        // root staging (cnf2_lane.h up8_stage_bwd_*): the marker d below `last` is marker d & 7 of tile d >> 3, whose root data
        // sits in buffer (d >> 3) & 1 of the job's row, in places the packed producer leaves alone and marker() does not read
        // (with the parked row sums the partials go over them).  As a staging lane this one is (marker cp.part of a tile, job
        // cp.mi); as a producer it reads its job's
        constexpr bool STAGE_B = CNF2_UP8_ROOT_STAGE_BWD != 0 && CNF2_UP8_ROW_SUMS != 0;
        double* const prow = tab + cp.mi * TS;
        auto staged_sure = [&](int d) {
            return *(const double2*)(prow + (((d >> 3) & 1) ? up8_stage_bwd_sure(1, 0) : up8_stage_bwd_sure(0, 0)) + 8 * (d & 7));
        };
        auto staged_hw = [&](int d) { return prow[(((d >> 3) & 1) ? up8_stage_bwd_hw(1, 0) : up8_stage_bwd_hw(0, 0)) + 8 * (d & 7)]; };
        auto staged_allele = [&](int d) { return ((const uint8_t*)(prow + up8_stage_bwd_alleles(0) + ((d >> 3) & 1)))[d & 7]; };
        StagedRoot sgb;
        double2    su_n;
        double     hw_n;
        if constexpr (STAGE_B) {
            // (the forward pass ended behind a fence: the region is the wave's to write)
            load_stage(pq, cp, last - cp.part, first, last, &sgb);
            store_stage_bwd(prow, 0, cp.part, sgb);
            load_stage(pq, cp, last - 8 - cp.part, first, last, &sgb);
            wave_lds_fence();
            load_rec<-1, SG, false>(pq, cp, rec_row, last + moff, first, last, staged_allele(0), &rraw);
            ap_next = staged_allele(1);
            su_n    = staged_sure(0);
            hw_n    = staged_hw(0);
        } else {
            load_rec<-1, SG>(pq, cp, rec_row, last + moff, first, last, load_root_allele(pq, cp, last + moff, first, last), &rraw);
            ap_next = load_root_allele(pq, cp, last - 1 + moff, first, last);
        }
#if CNF2_X_ROOTONCE & 2
        static_assert(!STAGE_B, "the ablation is of the per-marker loads");
        RawRoot rt_cur, rt_nxt;
        load_root(pq, cp, last + moff, first, last, &rt_cur);
        load_root(pq, cp, last - 8 + moff, first, last, &rt_nxt);
#endif
#if !CNF2_UP8_ROW_SUMS && !defined(CNF2_X_NOPARK)
        // epilogue role: row mi2 = job, chain sub
        const int mi2 = lane >> 3, sub = lane & 7;
#endif
        for (int m = last; m >= first; m--) {
            take_spill();
            ask_spill(m - first - 1);
#if CNF2_X_ROOTONCE & 2    /* timing ablation only: results are wrong (eight markers take the root's data of the first of them) */
            rt_cur.into(&rraw);
            produce_row_rec<true, true>(cp, tab, true, rraw);
            load_rec<-1, SG, false>(pq, cp, rec_row, m - 1 + moff, first, last, rt_cur.ap, &rraw);
            if (((last - m) & 7) == 7) {
                rt_cur = rt_nxt;
                load_root(pq, cp, m - 9 + moff, first, last, &rt_nxt);
            }
#else
            if constexpr (STAGE_B) {
                const int d = last - m;
                rraw.s0 = su_n.x;
                rraw.s1 = su_n.y;
                rraw.hw = hw_n;
                produce_row_rec<true, true>(cp, tab, true, rraw);
                load_rec<-1, SG, false>(pq, cp, rec_row, m - 1 + moff, first, last, ap_next, &rraw);
                // (read a marker, and the byte two markers, ahead as they were loaded: from the next tile's buffer at a tile's end)
                ap_next = staged_allele(d + 2);
                su_n    = staged_sure(d + 1);
                hw_n    = staged_hw(d + 1);
            } else {
                produce_row_rec<true, true>(cp, tab, true, rraw);
                load_rec<-1, SG>(pq, cp, rec_row, m - 1 + moff, first, last, ap_next, &rraw);       // (unconditional, as forward)
                ap_next = load_root_allele(pq, cp, m - 2 + moff, first, last);
            }
#endif
            wave_lds_fence();                   // the producer lanes' rows are in place for the recursion lanes that read them
            if constexpr (STAGE_B) {
                // at a tile's first marker the next tile goes into the other buffer: its last readers (the marker before) are
                // a fence behind, its first (this tile's seventh marker) fences ahead; the tile after that has eight markers to arrive
                if (((last - m) & 7) == 0) {
                    store_stage_bwd(prow, (((last - m) >> 3) + 1) & 1, cp.part, sgb);
                    load_stage(pq, cp, m - 16 - cp.part, first, last, &sgb);
                }
            }
            if ((m - first) & 1) marker(odd_t(), myrow, m);
            else marker(even_t(), myrow, m);
#if !CNF2_UP8_ROW_SUMS && !defined(CNF2_X_NOPARK)
            wave_lds_fence();
            // tile epilogue, as fb_fast_kernel's: lanes (row mi2, eighth sub) add up the 3 x 64 partials of the tile's rows
            {
                const double *red0 =tab + mi2 * TS + up8_park(0, sub * 8), *red1 = tab + mi2 * TS + up8_park(1, sub * 8),
                             *red2 = tab + mi2 * TS + up8_park(2, sub * 8);
                double        d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
                for (int i2 = 0; i2 < 8; i2++) {
                    d0 += red0[i2];
                    d1 += red1[i2];
                    d2 += red2[i2];
                }
                d0 = chain_sum(d0);
                d1 = chain_sum(d1);
                d2 = chain_sum(d2);
                d0 = fmax(d0, 0.0);
                d1 = fmax(d1, 0.0);
                d2 = fmax(d2, 0.0);
                if (sub == 0) {
                    if (!(p.flags & KP_RAW_DOSAGE)) {
                        const double tsum = d0 + d1 + d2;
                        const double inv  = tsum > 0.0 ? 1.0 / tsum : 0.0;
                        d0 *= inv;
                        d1 *= inv;
                        d2 *= inv;
                    }
                    // (the row's address is formed here, from a value the compiler cannot see through)
                    int ei = eind;
                    asm volatile("" : "+v"(ei));
                    double* out = p.dosage + ((size_t)ei * p.n_markers + m) * 3;
                    out[0] = d0;
                    out[1] = d1;
                    out[2] = d2;
                }
            }
#endif
            // the row's last readers are done (marker() with row sums, the epilogue without): the region goes to the next
            // marker's producer, or to the first forward tile of the wave's next job
            wave_lds_fence();
        }
    }
    if (stamp && fresh_lane() == 0) {
        p.clock_out[0] = __builtin_readcyclecounter() - t_shader;
        p.clock_out[1] = wall_clock64() - t_wall;
    }
}

// The logarithms of the likelihoods a fast-kernel launch left as mantissa and binary exponent: one thread per (job, shift
// mode), thread 0 of a job also the job's total.  Adds the chromosome's dropped butterfly constants (chrom_logk).
__global__ __launch_bounds__(256) void likelihood_logs_kernel(KernelParams p)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.n_jobs * 8) return;
    const Job    jb   = p.jobs[t >> 3];
    const int    s    = t & 7;
    const size_t e    = (size_t)jb.ind * p.n_chrom + jb.chrom;
    const double logk = p.chrom_logk[jb.chrom];
    const double ln2  = 0.69314718055994530942;
    const int    fe   = p.fexp[e * 8 + s];
    double       fs;
    if (fe == CNF2_LEXP_IGNORED) fs = CNF2_IGNORED_D;
    else if (fe == CNF2_LEXP_DEAD) fs = (double)CNF2_MINFACTOR_F;
    else fs = log(p.factors[e * 8 + s]) + (double)fe * ln2 + logk;
    p.factors[e * 8 + s] = fs;
    if (s == 0) {
        const int    le = p.lexp[e];
        const double T  = p.loglik[e];
        p.loglik[e] = (le == CNF2_LEXP_DEAD) ? (double)CNF2_MINFACTOR_F + log(T) : log(T) + (double)le * ln2 + logk;
    }
}
static void launch_likelihood_logs(const KernelParams& p, hipStream_t stream)
{
    if (p.n_jobs > 0) hipLaunchKernelGGL(likelihood_logs_kernel, dim3((p.n_jobs * 8 + 255) / 256), dim3(256), 0, stream, p);
}

// The logarithms of what a leave-one-out sweep left (the sweep kernel takes none): thread t is marker t and walks the
// individuals in ascending order -- coalesced across markers, and sums that are the same bits on every call.  A skipped
// individual's cells (-1 from the sweep) become CNF2_IGNORED and stay out of the sums.
__global__ __launch_bounds__(256) void loo_finish_kernel(double* loo, double* unl, int n_ind, int n_markers, double* loo_sum,
                                                         double* unl_sum)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_markers) return;
    double sl = 0.0, su = 0.0;
    for (int i = 0; i < n_ind; i++) {
        const size_t o = (size_t)i * n_markers + m;
        const double r = loo[o], u = unl[o];
        const bool   skipped = r < 0.0;
        const double lr = skipped ? CNF2_IGNORED_D : log(r), lu = skipped ? CNF2_IGNORED_D : -log(u);
        loo[o] = lr;
        unl[o] = lu;
        sl += skipped ? 0.0 : lr;
        su += skipped ? 0.0 : lu;
    }
    loo_sum[m] = sl;
    unl_sum[m] = su;
}
void launch_loo_finish(double* loo, double* unl, int n_ind, int n_markers, double* loo_sum, double* unl_sum, hipStream_t stream)
{
    if (n_markers > 0)
        hipLaunchKernelGGL(loo_finish_kernel, dim3((n_markers + 255) / 256), dim3(256), 0, stream, loo, unl, n_ind, n_markers,
                           loo_sum, unl_sum);
}

// The column sums of an origin sweep's rows: thread t is column t of [n_markers][4] and walks the individuals in ascending
// order -- coalesced across columns, and sums that are the same bits on every call.  A skipped individual's rows are zeros.
__global__ __launch_bounds__(256) void origin_finish_kernel(const double* org, int n_ind, int n_cols, double* org_sum)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cols) return;
    double s = 0.0;
    for (int i = 0; i < n_ind; i++) s += org[(size_t)i * n_cols + t];
    org_sum[t] = s;
}
void launch_origin_finish(const double* org, int n_ind, int n_markers, double* org_sum, hipStream_t stream)
{
    const int n_cols = n_markers * 4;
    if (n_cols > 0)
        hipLaunchKernelGGL(origin_finish_kernel, dim3((n_cols + 255) / 256), dim3(256), 0, stream, org, n_ind, n_cols, org_sum);
}

// =====================================================================================
// Packed kernel: four jobs per wavefront for windows whose BOTH parents are homozygous with equal sure
// at every marker (e.g. the private empty F1 parents of an F2, cnF2freq.cpp:6515-6527).  For such a
// parent the two allele indices are interchangeable, its phase weight is 0/1 (cnF2freq.cpp:1235-1239)
// and the unrestricted table does not depend on its shift bit: shift modes that differ in shift bits
// 1, 2 carry bit-identical alpha and beta.  Only the two modes s0 = 0, 1 are swept; the per-locus row
// sums the restricted / class-2 tables over both values of each parent's shift bit, which is exactly the
// sum of the four copies.  Lane layout: chain = lane >> 3 = (job in wave) << 1 | s0, the rest as in
// fb_fast_kernel; a tile is 2 markers x 4 jobs (same 8 table rows of LDS, row = marker << 2 | job).
// Always half-spill.  Outputs are written for all 8 shift modes.
// =====================================================================================
__global__ __launch_bounds__(CNF2_BLOCK, 2) void fb_packed_kernel(KernelParams p)
{
    constexpr int ROW = 528;
    __shared__ __attribute__((aligned(16))) double lds[CNF2_WAVES_PER_BLOCK][8 * TAB_STRIDE];

    const int lane  = threadIdx.x & 63;
    const int wib   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave  = blockIdx.x * CNF2_WAVES_PER_BLOCK + wib;
    const int nwave = gridDim.x * CNF2_WAVES_PER_BLOCK;
    double*   tab   = lds[wib];
    double*   spill = p.spill + (size_t)wave * p.spill_stride;

    // (jobs from the launch's counter, as in fb_fast_kernel)
    auto take_job = [&](int strided) {
        if (!p.job_next) return strided;
        int j = 0;
        if (lane == 0) j = atomicAdd(p.job_next, 1);
        return __builtin_amdgcn_readfirstlane(j);
    };
    for (int job = take_job(wave); job < p.n_pjobs; job = take_job(job + nwave)) {
        const PackedJob pj = p.pjobs[job];
        // producer role: part x (marker in tile, job)
        FastCtx c;
        c.part = lane >> 3;
        c.mi   = lane & 7;                                   // table row = marker_in_tile << 2 | job
        const int pmt = c.mi >> 2;
        {
            const Window wp = p.windows[pj.ind[c.mi & 3]];
            int32_t      rp, rt, ro;
            make_part(wp, c.part, &c.pc, &rp, &rt, &ro);
            c.slot_a = lane >> 3;
            c.row_a  = (c.slot_a < 7 && wp.row[c.slot_a] >= 0) ? wp.row[c.slot_a] : 0;
        }
        c.idx_base = part_entry_index(c.part, 0);
        c.idx_k01  = part_entry_index(c.part, 1) - c.idx_base;
        c.idx_k10  = part_entry_index(c.part, 2) - c.idx_base;
        // consumer role: chain = job << 1 | s0; shift bits 1, 2 are represented by 0
        const int s    = lane >> 3;
        const int cjob = s >> 1;
        const int ind  = pj.ind[cjob];
        c.s0 = s & 1;
        c.s1 = 0;
        c.s2 = 0;
        c.lo = state_lo(lane);
        c.active = true;                                     // eligibility: shiftignore == 0, shiftend == 8
        const int first = pj.first, last = pj.last;
        const int ntile = (last - first + 2) >> 1;
        if (p.path_log && (lane & 15) == 0) p.path_log[(size_t)ind * p.n_chrom + pj.chrom] = PATH_PACKED | pj.homleaf;
        double*   myrow0 = tab + cjob * TAB_STRIDE;          // this lane's job, marker 0 of the tile
        double*   myrow1 = myrow0 + 4 * TAB_STRIDE;

        using odd_t  = std::integral_constant<bool, true>;
        using even_t = std::integral_constant<bool, false>;

        // ---------------------------------------------------------------- forward
        double a[8];
#pragma unroll
        for (int j = 0; j < 8; j++) a[j] = 1.0 / 64.0;
        double mant = 1.0;
        int    expo = 0;
        bool   dead = false;
        double pend = 1.0;
        auto fwd_step = [&](auto odd_tag, const double* row, int m) {
            constexpr bool ODD = decltype(odd_tag)::value;
            double         e[8];
            emission_from_row(row, c, e, pend);
            const double2 r  = *(const double2*)(row + TAB_T);
            const int     ml = m - first;
            double*       sp = spill + (size_t)(ml >> 1) * ROW;
            if (!ODD) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const d2v v = {a[2 * k], a[2 * k + 1]};
                    __builtin_nontemporal_store(v, (d2v*)(sp + k * 128 + lane * 2));
                }
            }
#pragma unroll
            for (int j = 0; j < 8; j++) a[j] *= e[j];
            pend = 1.0;
            if (!ODD || m == last) {
                const double inv = chain_normaliser(a, &mant, &expo, &dead);
                pend             = inv;
                if (c.lo == 0) sp[512 + 2 * s + (ODD ? 1 : 0)] = inv;
            }
            if (m < last) transition_scaled(a, r.x, r.y);
        };
        RawOne raw;
        load_raw1_at<0>(p, c, first + pmt, first, last, &raw);
        for (int t = 0; t < ntile; t++) {
            const int m0 = first + t * 2;
            if (pj.homleaf) produce_row2<false, true, true>(c, tab, m0 + pmt <= last, raw);
            else produce_row2<false, true, false>(c, tab, m0 + pmt <= last, raw);
            if (t + 1 < ntile) load_raw1_at<0>(p, c, m0 + 2 + pmt, first, last, &raw);
            wave_lds_fence();
            fwd_step(even_t(), myrow0, m0);
            if (m0 < last) fwd_step(odd_t(), myrow1, m0 + 1);
            wave_lds_fence();
        }

        // ---------------------------------------------------------------- likelihoods
        // every mode s has the likelihood of mode s & 1; the log-sum-exp over 8 modes adds the same two
        // terms four times (the pairwise tree of fb_fast_kernel doubles exactly, so the bits agree)
        const double logk = p.chrom_logk[pj.chrom];
        const double fs   = dead ? (double)CNF2_MINFACTOR_F : (log(mant) + (double)expo * 0.69314718055994530942);
        double fmaxv = fmax(fs, lane_xor8(fs));
        fmaxv        = fmax(fmaxv, -1e15);
        const double term = exp(fs - fmaxv);
        const double real = 4.0 * (term + lane_xor8(term));
        const double factor = fmaxv + log(real);
        if (c.lo == 0) {
            double* fo = p.factors + ((size_t)ind * p.n_chrom + pj.chrom) * 8 + c.s0;
            const double v = !dead ? fs + logk : fs;
            fo[0] = v;
            fo[2] = v;
            fo[4] = v;
            fo[6] = v;
        }
        if ((lane & 15) == 0) p.loglik[(size_t)ind * p.n_chrom + pj.chrom] = (fmaxv > -1e14) ? factor + logk : factor;
        const bool skip = isnan(factor) || factor < (double)CNF2_MINFACTOR_F;     // cnF2freq.cpp:5403
        if (p.flags & KP_NO_DOSAGE) continue;

        // ---------------------------------------------------------------- backward + rows
        BwdState<> S;
#pragma unroll
        for (int j = 0; j < 8; j++) S.b[j] = 1.0;
        S.bmant = 1.0;
        S.bexpo = 0;
        S.bdead = false;
        S.fmant = mant;
        S.fexpo = expo;
        const double nf  = -factor * 1.4426950408889634074;
        const double nfk = floor(nf);
        const double xm  = exp2(nf - nfk);
        const int    xe  = (int)nfk;
        const bool   chain_on = !skip && !dead && !(factor - fs > 40.0);          // cnF2freq.cpp:5420-5421
        auto load_row = [&](int idx) {
            const double* sp = spill + (size_t)idx * ROW;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const d2v v = __builtin_nontemporal_load((const d2v*)(sp + k * 128 + lane * 2));
                S.am[2 * k]     = v.x;
                S.am[2 * k + 1] = v.y;
            }
            const double2 iv = *(const double2*)(sp + 512 + 2 * s);
            S.inv_even       = iv.x;
            S.inv_odd        = iv.y;
        };
        S.inv_odd = 1.0;
        load_row((last - first) >> 1);

        auto marker = [&](auto odd_tag, double* row, int m) {
            constexpr bool ODD = decltype(odd_tag)::value;
            const int      ml  = m - first;
            double         wj[8];
            const double2 r_m = *(const double2*)(row + TAB_T);     // gap m-1 -> m
            double        inv_m;
            if (ODD) {
                double ep[8];
                emission_from_row(row - 4 * TAB_STRIDE, c, ep);     // the even marker of the pair: same job, marker 0
#pragma unroll
                for (int j = 0; j < 8; j++) wj[j] = S.am[j] * ep[j];
                transition_scaled(wj, r_m.x, r_m.y);
#pragma unroll
                for (int j = 0; j < 8; j++) wj[j] *= S.b[j];
                inv_m = S.inv_odd;
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) wj[j] = S.am[j] * S.b[j];
                inv_m = S.inv_even;
                asm volatile("" : "+v"(wj[0]), "+v"(wj[1]), "+v"(wj[2]), "+v"(wj[3]), "+v"(wj[4]), "+v"(wj[5]),
                             "+v"(wj[6]), "+v"(wj[7]), "+v"(inv_m) : : "memory");
                const int idx = (ml >> 1) - 1;
                load_row(idx < 0 ? 0 : idx);
            }
            if (!ODD || m == last) {
                int ex;
                S.fmant = frexp(S.fmant * inv_m, &ex);
                S.fexpo += ex;
            }
            // class sums over the four copies (s1, s2) of this mode: tables summed over the parents' shift bits
            double n_tot = 0.0, n_a1 = 0.0, n_b1 = 0.0, n_2 = 0.0;
#pragma unroll
            for (int f = 0; f < 2; f++) {
                const int     ia = (0 << 5) | (f << 4) | c.lo;
                const double* Br = row + TAB_R + ((1 << 5) | (f << 4));
                const double* B1 = row + TAB_2 + ((1 << 5) | (f << 4));
                const double  cf = row[TAB_C + f * 2 + c.s0];
                const double  av = cf * (row[TAB_R + ia] + row[TAB_R + ia + 8]);
                const double  a1 = cf * (row[TAB_2 + ia] + row[TAB_2 + ia + 8]);
                double        sb = 0.0, sb1 = 0.0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    sb += wj[j] * (Br[j] + Br[8 + j]);
                    sb1 += wj[j] * (B1[j] + B1[8 + j]);
                }
                n_tot += av * sb;
                n_a1 += a1 * sb;
                n_b1 += av * sb1;
                n_2 += a1 * sb1;
            }
            const double sc0   = ODD ? xm * S.inv_even : xm;
            const double scale = chain_on ? ldexp(sc0 * S.fmant * S.bmant, xe + S.fexpo + S.bexpo) : 0.0;
            const double q2 = scale * n_2;
            const double q1 = scale * (n_a1 + n_b1 - 2.0 * n_2);
            const double q0 = scale * (n_tot - n_a1 - n_b1 + n_2);
            double e[8];
            emission_from_row(row, c, e);
            // the 16 lanes of this job park their partials in the job's own row of this marker
            wave_lds_fence();
            row[lane & 15]         = q0;
            row[64 + (lane & 15)]  = q1;
            row[128 + (lane & 15)] = q2;
#pragma unroll
            for (int j = 0; j < 8; j++) S.b[j] *= e[j];
            if (!ODD) scale_chain(S.b, &S.bmant, &S.bexpo, &S.bdead);
            transition_scaled(S.b, r_m.x, r_m.y);
        };
        load_raw1_at<-1>(p, c, first + (ntile - 1) * 2 + pmt, first, last, &raw);
        for (int t = ntile - 1; t >= 0; t--) {
            const int m0 = first + t * 2;
            if (pj.homleaf) produce_row2<true, true, true>(c, tab, m0 + pmt <= last, raw);
            else produce_row2<true, true, false>(c, tab, m0 + pmt <= last, raw);
            wave_lds_fence();
            if (m0 < last) marker(odd_t(), myrow1, m0 + 1);
            marker(even_t(), myrow0, m0);
            wave_lds_fence();
            if (t > 0) load_raw1_at<-1>(p, c, m0 - 2 + pmt, first, last, &raw);
            // tile epilogue: lane = table row (marker << 2 | job) x eighth: 3 x 16 partials per row
            {
                const int     r8 = lane >> 3, sub = lane & 7;
                const double* red = tab + r8 * TAB_STRIDE + sub * 2;
                double d0 = red[0] + red[1], d1 = red[64] + red[65], d2 = red[128] + red[129];
                d0 = fmax(chain_sum(d0), 0.0);
                d1 = fmax(chain_sum(d1), 0.0);
                d2 = fmax(chain_sum(d2), 0.0);
                const int mm = m0 + (r8 >> 2);
                if (sub == 0 && mm <= last) {
                    if (!(p.flags & KP_RAW_DOSAGE)) {
                        const double tsum = d0 + d1 + d2;
                        const double inv  = tsum > 0.0 ? 1.0 / tsum : 0.0;
                        d0 *= inv;
                        d1 *= inv;
                        d2 *= inv;
                    }
                    double* out = p.dosage + ((size_t)pj.ind[r8 & 3] * p.n_markers + mm) * 3;
                    out[0] = d0;
                    out[1] = d1;
                    out[2] = d2;
                }
            }
            wave_lds_fence();
        }
    }
}

// per-row flag: every marker homozygous (or doubly unknown) with equal sure -- such an ancestor
// can never make a tie group active (cnF2freq.cpp:3488: its zero-weight paths are the pruned ones)
__global__ __launch_bounds__(256) void row_flags_kernel(const uint8_t* allele8, const double2* sure, int n_markers,
                                                        uint8_t* flags)
{
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * n_markers;
    int          mine = 0;
    for (int m = threadIdx.x; m < n_markers; m += blockDim.x) {
        const uint8_t ap = allele8[base + m];
        const double2 s  = sure[base + m];
        if ((ap & 15) != (ap >> 4) || s.x != s.y) mine = 1;
    }
    if (mine) bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) flags[blockIdx.x] = bad ? 0 : 1;
}

// Parity hook: path-free emission e_s(g) of one (individual, marker) for the 8 shift modes,
// through exactly the producer/consumer code of the sweep.
__global__ __launch_bounds__(64) void emission_kernel(KernelParams p, int ind, int marker, double* out)
{
    __shared__ double tab[64];
    const int    lane = threadIdx.x;
    const Window w    = p.windows[ind];
    LaneCtx      c;
    make_lane(w, lane, &c.L);
    c.row_root   = w.row[0];
    c.root_attop = (w.flags[0] & SLOT_FOUNDER) != 0;
    const int s  = lane >> 3;
    c.s0 = s & 1;
    c.s1 = (s >> 1) & 1;
    c.s2 = (s >> 2) & 1;
    c.lo = state_lo(lane);
    c.active = true;
    c.n_combo = 1;
    const Slot root = load_slot(p, c.row_root, marker);
    LineTerms  T;
    tab[lane] = produce_entry(p, c, root, marker, &T);
    wave_lds_fence();
    double c0, c1, e[8];
    root_weights(c, root, &c0, &c1);
    emission_from_table(tab, c, c0, c1, e);
#pragma unroll
    for (int j = 0; j < 8; j++) out[s * 64 + j * 8 + c.lo] = e[j];
}

// Self-test of the lane-exchange helpers (tests/test_gpu_parity.py): out[k][lane] = value
// received by `lane` for xor distance 1<<k.
__global__ __launch_bounds__(64) void xor_selftest_kernel(double* out)
{
    const int lane = threadIdx.x;
    double    v    = 1000.0 + lane;
    out[0 * 64 + lane] = lane_xor1(v);
    out[1 * 64 + lane] = lane_xor2(v);
    out[2 * 64 + lane] = lane_xor4(v);
    out[3 * 64 + lane] = lane_xor8(v);
    out[4 * 64 + lane] = lane_xor16(v);
    out[5 * 64 + lane] = lane_xor32(v);
}


// =====================================================================================
// Stage-2 consumers of the alpha/beta store, parity level:
// they read the reference-layout store that fb_kernel<true> leaves for ONE individual and
// chromosome and answer the queries of HOT LOOP 2 / 3 in bulk.  Not tuned; one thread per answer.
// =====================================================================================
__device__ __forceinline__ double s2_fw(const Stage2Params& q, int s, int ml, int slot, int g)
{
    return q.fwbw[(((size_t)s * q.len + ml) * 3 + slot) * 64 + g];
}
__device__ __forceinline__ double s2_ff(const Stage2Params& q, int s, int ml, int slot)
{
    return q.fwbwfactors[((size_t)s * q.len + ml) * 3 + slot];
}

// Terms of the two lines of state g under shift mode s for root allele f.
__device__ __forceinline__ void s2_lines(const Stage2Params& q, const Window& w, int m, int g, int s, int f,
                                         LaneJob* L0, LaneJob* L1, LineTerms* T0, LineTerms* T1, double* cf, bool* attop)
{
    const KernelParams& p = q.kp;
    const Slot root = load_slot(p, w.row[0], m);
    *attop = (w.flags[0] & SLOT_FOUNDER) != 0;
    RootTerms R;
    root_terms(root, *attop, f, &R);
    *cf = R.cbase * phase_weight(root, f ^ (s & 1));
    make_lane(w, (0 << 5) | (f << 4) | (((s >> 1) & 1) << 3) | (g & 7), L0);
    make_lane(w, (1 << 5) | (f << 4) | (((s >> 2) & 1) << 3) | (g >> 3), L1);
    line_terms(L0->cfg, load_slot(p, L0->row_par, m), load_slot(p, L0->row_tr, m), load_slot(p, L0->row_ot, m),
               R.inmv0, R.sv0, R.inmv0 == 2, T0);
    line_terms(L1->cfg, load_slot(p, L1->row_par, m), load_slot(p, L1->row_tr, m), load_slot(p, L1->row_ot, m),
               R.inmv1, R.sv1, false, T1);
}

// One allele assignment (path) of a line: parent allele fp, traced / other grandparent alleles.
__device__ __forceinline__ double s2_path_term(const LineCfg& c, const LineTerms& T, int fp, int fg_tr, int fg_ot)
{
    const bool par_line = !(c.par & SLOT_PRESENT) || (c.par & SLOT_FOUNDER);
    if (!(c.par & SLOT_PRESENT)) fp = 0;                 // 1 + secondval, whatever the path bits say
    if (par_line || !(c.tr & SLOT_PRESENT)) fg_tr = 0;
    if (par_line || !(c.ot & SLOT_PRESENT)) fg_ot = 0;
    return (T.base[fp] * T.ot[fp][fg_ot]) * T.tr[fp][fg_tr];
}

// val(s, g, flag2) = exp(doanalyze(classicstop(q, g), flag2) - factor) of cnF2freq.cpp:5499-5508 for one
// marker: out[s][g][flag2]; 0 where the reference would not count it (not finite or <= -200).
__global__ __launch_bounds__(128) void locked_query_kernel(Stage2Params q, int marker, double* out)
{
    const int flag2 = threadIdx.x;            // 0..127
    const int g     = blockIdx.x & 63;
    const int s     = blockIdx.x >> 6;
    const Window w  = q.kp.windows[0];
    const int ml    = marker - q.first;
    const int f     = flag2 & 1;
    LaneJob   L0, L1;
    LineTerms T0, T1;
    double    cf;
    bool      attop;
    s2_lines(q, w, marker, g, s, f, &L0, &L1, &T0, &T1, &cf, &attop);
    double e;
    if (attop) e = cf;
    else {
        const int fp0 = (flag2 >> 1) & 1, fp1 = (flag2 >> 4) & 1;
        const int a0 = (flag2 >> (2 + L0.cfg.firstpar)) & 1, o0 = (flag2 >> (2 + (L0.cfg.firstpar ^ 1))) & 1;
        const int a1 = (flag2 >> (5 + L1.cfg.firstpar)) & 1, o1 = (flag2 >> (5 + (L1.cfg.firstpar ^ 1))) & 1;
        e = (cf * s2_path_term(L1.cfg, T1, fp1, a1, o1)) * s2_path_term(L0.cfg, T0, fp0, a0, o0);
    }
    const double factor = q.loglik[0];
    const double am = s2_fw(q, s, ml, 0, g), be = s2_fw(q, s, ml, 1, g);
    // cnF2freq.cpp:1960-2016: alpha-minus filtered to g, emission of the path, beta of g
    double lv = s2_ff(q, s, ml, 0) + log(am * e) + s2_ff(q, s, ml, 1) + log(be) - factor;
    double v  = (isfinite(lv) && lv > -200.0) ? exp(lv) : 0.0;
    out[((size_t)s * 64 + g) * 128 + flag2] = v;
}

// Parity hook: path-resolved emission e_s(g, flag2) = trackpossible<0,0>(..., 2g, flag2, s) of cnF2freq.cpp:1380-1385
// for one (individual, marker): out[s][g][flag2], through the line terms the stage-2 kernels use.
__global__ __launch_bounds__(128) void emission_paths_kernel(Stage2Params q, int marker, double* out)
{
    const int flag2 = threadIdx.x;            // 0..127
    const int g     = blockIdx.x & 63;
    const int s     = blockIdx.x >> 6;
    const Window w  = q.kp.windows[0];
    const int f     = flag2 & 1;
    LaneJob   L0, L1;
    LineTerms T0, T1;
    double    cf;
    bool      attop;
    s2_lines(q, w, marker, g, s, f, &L0, &L1, &T0, &T1, &cf, &attop);
    double e;
    if (attop) e = cf;
    else {
        const int fp0 = (flag2 >> 1) & 1, fp1 = (flag2 >> 4) & 1;
        const int a0 = (flag2 >> (2 + L0.cfg.firstpar)) & 1, o0 = (flag2 >> (2 + (L0.cfg.firstpar ^ 1))) & 1;
        const int a1 = (flag2 >> (5 + L1.cfg.firstpar)) & 1, o1 = (flag2 >> (5 + (L1.cfg.firstpar ^ 1))) & 1;
        e = (cf * s2_path_term(L1.cfg, T1, fp1, a1, o1)) * s2_path_term(L0.cfg, T0, fp0, a0, o0);
    }
    out[((size_t)s * 64 + g) * 128 + flag2] = e;
}
void launch_emission_paths(const KernelParams& p, int marker, double* out, hipStream_t stream)
{
    Stage2Params q;
    memset(&q, 0, sizeof(q));
    q.kp = p;
    hipLaunchKernelGGL(emission_paths_kernel, dim3(512), dim3(128), 0, stream, q, marker, out);
}

// rawervals[turn][s] of cnF2freq.cpp:5686-5752 for one marker (aroundturner, cnF2freq.cpp:498-554):
// alpha (after emission) of mode s, states XOR-permuted by turn & 54, times beta of the turned mode.
__global__ __launch_bounds__(64) void turn_scan_kernel(Stage2Params q, int marker, double* out)
{
    const int k    = threadIdx.x;
    const int s    = blockIdx.x & 7;
    const int turn = blockIdx.x >> 3;
    const int ml   = marker - q.first;
    const int xorturn = turn & 54;                                                      // cnF2freq.cpp:508
    const int shiftx  = (turn >> 6) | ((turn & 1) ? 2 : 0) | ((turn & 8) ? 4 : 0);     // cnF2freq.cpp:509-510
    const int s2      = s ^ shiftx;
    double v = s2_fw(q, s, ml, 2, k ^ xorturn) * s2_fw(q, s2, ml, 1, k);
    v += lane_xor1(v);
    v += lane_xor2(v);
    v += dpp_mov_all<0x141>(v);
    v += lane_xor8(v);
    v += lane_xor16(v);
    v += lane_xor32(v);
    if (k == 0) {
        double r = (v > 0.0) ? s2_ff(q, s, ml, 2) + s2_ff(q, s2, ml, 1) + log(v) : (double)CNF2_MINFACTOR_F;
        out[turn * 8 + s] = r - q.loglik[0];
    }
}

// statereporter row (cnF2freq.cpp:3540-3546): sum of val over shift modes and paths, by state g,
// for every marker of the chromosome: out[len][64] (un-normalised like the reference's reporter).
__global__ __launch_bounds__(64) void state_rows_kernel(Stage2Params q, uint32_t flags, double* out)
{
    const int g  = threadIdx.x;
    const int ml = blockIdx.x;
    const int m  = q.first + ml;
    const Window w = q.kp.windows[0];
    const double factor = q.loglik[0];
    const int n_combo = (flags & KP_NO_TIES) ? 1 : (1 << w.n_groups);
    double acc = 0.0;
    for (int s = 0; s < 8; s++) {
        if ((s & w.shiftignore) || s >= w.shiftend) continue;
        if (factor - q.factors[s] > 40.0) continue;                                    // cnF2freq.cpp:5421
        double e = 0.0;
        for (int f = 0; f < 2; f++) {
            LaneJob   L0, L1;
            LineTerms T0, T1;
            double    cf;
            bool      attop;
            s2_lines(q, w, m, g, s, f, &L0, &L1, &T0, &T1, &cf, &attop);
            if (attop) {
                e += cf;
                continue;
            }
            for (int combo = 0; combo < n_combo; combo++) {
                const bool nt = (flags & KP_NO_TIES) != 0;
                double r0, r1, t2;
                line_restricted(L0.cfg, T0, nt ? -1 : tie_force(L0.tie_par, combo), nt ? -1 : tie_force(L0.tie_tr, combo),
                                nt ? -1 : tie_force(L0.tie_ot, combo), &r0, &t2);
                line_restricted(L1.cfg, T1, nt ? -1 : tie_force(L1.tie_par, combo), nt ? -1 : tie_force(L1.tie_tr, combo),
                                nt ? -1 : tie_force(L1.tie_ot, combo), &r1, &t2);
                e += (cf * r1) * r0;
            }
        }
        const double sc = exp(s2_ff(q, s, ml, 0) + s2_ff(q, s, ml, 1) - factor);
        acc += s2_fw(q, s, ml, 0, g) * s2_fw(q, s, ml, 1, g) * sc * e;
    }
    out[(size_t)ml * 64 + g] = acc;
}


// Crossover posteriors from the store, brute force (the cross-check of the sweep's crossover mode): one block per gap
// ml -> ml+1, thread g.  For every admissible shift mode s within 40 log units (cnF2freq.cpp:5421) the pairwise posterior
// alpha_ml(g) T(g, g') e_{ml+1}(g') beta_{ml+1}(g') is summed with the explicit 64 x 64 transition and normalised by its own
// total; xi_t = sum_s exp(factors[s] - factor) * (mass with state bit t flipped) / total.  out[len][6]; row len-1 and gaps
// with rho 0 are zero.
__global__ __launch_bounds__(64) void crossover_rows_kernel(Stage2Params q, double* out)
{
    __shared__ double tab[64];
    __shared__ double ebs[64];
    const int    g  = threadIdx.x;
    const int    ml = blockIdx.x;
    const Window w  = q.kp.windows[0];
    const double factor = q.loglik[0];
    double xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double2 r = q.kp.rho[q.first + ml];
    const bool skip = isnan(factor) || factor < (double)CNF2_MINFACTOR_F;
    if (ml + 1 < q.len && !skip && (r.x > 0.0 || r.y > 0.0)) {
        const int m = q.first + ml + 1;
        // e_{ml+1} of all 8 modes through the sweep's producer / consumer code (as emission_kernel)
        LaneCtx c;
        make_lane(w, g, &c.L);
        c.row_root   = w.row[0];
        c.root_attop = (w.flags[0] & SLOT_FOUNDER) != 0;
        const int sl = g >> 3;
        c.s0 = sl & 1;
        c.s1 = (sl >> 1) & 1;
        c.s2 = (sl >> 2) & 1;
        c.lo = state_lo(g);
        c.active  = true;
        c.n_combo = 1;
        const Slot root = load_slot(q.kp, c.row_root, m);
        LineTerms  T;
        tab[g] = produce_entry(q.kp, c, root, m, &T);
        __syncthreads();
        double c0, c1, e[8];
        root_weights(c, root, &c0, &c1);
        emission_from_table(tab, c, c0, c1, e);
        __syncthreads();
        const double rt[6] = {r.y, r.x, r.x, r.y, r.x, r.x};
        for (int s = 0; s < 8; s++) {
            // e of mode s, state g' = j * 8 + lo sits in lane s * 8 + (the lane holding lo), register j
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (sl == s) ebs[j * 8 + c.lo] = e[j];
            __syncthreads();
            const double eg = ebs[g];
            __syncthreads();
            ebs[g] = eg * s2_fw(q, s, ml + 1, 1, g);
            __syncthreads();
            const bool use = !((s & w.shiftignore) || s >= w.shiftend) && !(factor - q.factors[s] > 40.0);
            if (use) {
                const double a = s2_fw(q, s, ml, 2, g);
                double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, tot = 0.0;
                for (int g2 = 0; g2 < 64; g2++) {
                    const int d = g ^ g2;
                    double    tr = 1.0;
#pragma unroll
                    for (int t = 0; t < 6; t++) tr *= ((d >> t) & 1) ? rt[t] : 1.0 - rt[t];
                    const double v = a * tr * ebs[g2];
                    tot += v;
#pragma unroll
                    for (int t = 0; t < 6; t++)
                        if ((d >> t) & 1) acc[t] += v;
                }
                tot = across_chains_sum(chain_sum(tot));
                const double ws = exp(q.factors[s] - factor);
#pragma unroll
                for (int t = 0; t < 6; t++) {
                    const double v = across_chains_sum(chain_sum(acc[t]));
                    if (tot > 0.0) xi[t] += ws * v / tot;
                }
            }
            __syncthreads();
        }
    }
    if (g < 6) out[(size_t)ml * 6 + g] = xi[g];
}


// The leave-one-out rows from the store, brute force (the cross-check of the sweep's leave-one-out mode): one block per
// marker ml, thread g.  loo = log sum over the analysed modes with a likelihood of sum_g alphaminus(g) beta(g) (slots 0 and
// 1 with their cumulative scales) - factor; the same sum with slot 2 in place of slot 0 is the mode's likelihood itself, and
// a mode whose own is 0 has none.  unlinked = -log of the mean over the analysed modes of (1 / 64) sum_g e(g), e through the
// sweep's producer / consumer code (as emission_kernel).  out[len][2]; both CNF2_IGNORED where no mode has a likelihood.
__global__ __launch_bounds__(64) void loo_rows_kernel(Stage2Params q, double* out)
{
    __shared__ double tab[64];
    const int    g  = threadIdx.x;
    const int    ml = blockIdx.x;
    const int    m  = q.first + ml;
    const Window w  = q.kp.windows[0];
    const double factor = q.loglik[0];
    double acc = 0.0;
    bool   any = false;
    for (int s = 0; s < 8; s++) {
        if ((s & w.shiftignore) || s >= w.shiftend) continue;
        const double b    = s2_fw(q, s, ml, 1, g);
        const double own  = across_chains_sum(chain_sum(s2_fw(q, s, ml, 2, g) * b));
        if (!(own > 0.0) || !(q.factors[s] > (double)CNF2_MINFACTOR_F)) continue;
        any = true;
        const double part = across_chains_sum(chain_sum(s2_fw(q, s, ml, 0, g) * b));
        acc += part * exp(s2_ff(q, s, ml, 0) + s2_ff(q, s, ml, 1) - factor);
    }
    LaneCtx c;
    make_lane(w, g, &c.L);
    c.row_root   = w.row[0];
    c.root_attop = (w.flags[0] & SLOT_FOUNDER) != 0;
    const int sl = g >> 3;
    c.s0 = sl & 1;
    c.s1 = (sl >> 1) & 1;
    c.s2 = (sl >> 2) & 1;
    c.lo = state_lo(g);
    c.active  = true;
    c.n_combo = 1;
    const Slot root = load_slot(q.kp, c.row_root, m);
    LineTerms  T;
    tab[g] = produce_entry(q.kp, c, root, m, &T);
    __syncthreads();
    double c0, c1, e[8];
    root_weights(c, root, &c0, &c1);
    emission_from_table(tab, c, c0, c1, e);
    const bool   on   = !(sl & w.shiftignore) && sl < w.shiftend;
    const double mine = chain_sum(((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
    const double tot  = across_chains_sum(on ? mine : 0.0);
    const int    n_on = __builtin_popcountll(__ballot(on)) >> 3;
    if (g == 0) {
        const bool skip = !any || isnan(factor);
        out[(size_t)ml * 2 + 0] = skip ? CNF2_IGNORED_D : log(acc);
        out[(size_t)ml * 2 + 1] = skip ? CNF2_IGNORED_D : -log(tot / (64.0 * n_on));
    }
}


// The origin rows from the store, brute force (the cross-check of the sweep's origin mode): one block per marker ml, thread g.
// gamma(g) = sum_s w_s gamma_s(g) / sum_s w_s with gamma_s = slot 2 (alpha after the emission) x slot 1 (beta) normalised
// within the mode and w_s = exp(factors[s] - factor), over the analysed modes with a likelihood that are not 40 below the
// total; then the ten masked sums.  out[len][10] = origin[4], bits[6]; zeros where no mode has a likelihood.
__global__ __launch_bounds__(64) void origin_rows_kernel(Stage2Params q, double* out)
{
    const int    g  = threadIdx.x;
    const int    ml = blockIdx.x;
    const Window w  = q.kp.windows[0];
    const double factor = q.loglik[0];
    double acc = 0.0, wsum = 0.0;
    for (int s = 0; s < 8; s++) {
        if ((s & w.shiftignore) || s >= w.shiftend) continue;
        const double fs = q.factors[s];
        if (!(fs > (double)CNF2_MINFACTOR_F) || factor - fs > 40.0) continue;
        const double gam = s2_fw(q, s, ml, 2, g) * s2_fw(q, s, ml, 1, g);
        const double own = across_chains_sum(chain_sum(gam));
        if (!(own > 0.0)) continue;
        const double ws = exp(fs - factor);
        acc += ws * (gam / own);
        wsum += ws;
    }
    const bool   skip = !(wsum > 0.0) || isnan(factor);
    const double ga = skip ? 0.0 : acc / wsum;
    auto total = [&](bool on) { return across_chains_sum(chain_sum(on ? ga : 0.0)); };
    double r[10];
    for (int k = 0; k < 4; k++) r[k] = total(((g & 1) | ((g >> 2) & 2)) == k);
    for (int t = 0; t < 6; t++) r[4 + t] = total(((g >> t) & 1) != 0);
    if (g == 0)
        for (int k = 0; k < 10; k++) out[(size_t)ml * 10 + k] = r[k];
}

// The descent rows from the store, brute force (the cross-check of the sweep's descent mode): origin_rows_kernel's gamma(g) and
// normaliser, then the eight masked sums: first side k = 2 bit0 + (bit0 ? bit2 : bit1), second side k = 2 bit3 + (bit3 ? bit5 :
// bit4) of the state g.  out[len][8]; zeros where no mode has a likelihood.
__global__ __launch_bounds__(64) void descent_rows_kernel(Stage2Params q, double* out)
{
    const int    g  = threadIdx.x;
    const int    ml = blockIdx.x;
    const Window w  = q.kp.windows[0];
    const double factor = q.loglik[0];
    double acc = 0.0, wsum = 0.0;
    for (int s = 0; s < 8; s++) {
        if ((s & w.shiftignore) || s >= w.shiftend) continue;
        const double fs = q.factors[s];
        if (!(fs > (double)CNF2_MINFACTOR_F) || factor - fs > 40.0) continue;
        const double gam = s2_fw(q, s, ml, 2, g) * s2_fw(q, s, ml, 1, g);
        const double own = across_chains_sum(chain_sum(gam));
        if (!(own > 0.0)) continue;
        const double ws = exp(fs - factor);
        acc += ws * (gam / own);
        wsum += ws;
    }
    const bool   skip = !(wsum > 0.0) || isnan(factor);
    const double ga = skip ? 0.0 : acc / wsum;
    const int    k1 = (g & 1) ? 2 + ((g >> 2) & 1) : ((g >> 1) & 1);
    const int    k2 = (g & 8) ? 2 + ((g >> 5) & 1) : ((g >> 4) & 1);
    for (int k = 0; k < 8; k++) {
        const double r = across_chains_sum(chain_sum((k < 4 ? k1 == k : k2 == k - 4) ? ga : 0.0));
        if (g == 0) out[(size_t)ml * 8 + k] = r;
    }
}


// HAPLOS accumulators of HOT LOOP 2 (cnF2freq.cpp:5554-5556 -> updatehaplo 1561-1575 -> trackpossible<HAPLOS>
// 1347-1350), per marker and window slot: out[len][7][2], out[..][k][phase] = sum of val over states,
// shift modes and admissible paths on which the individual in slot k is used with that phase
// (allele index ^ firstpar ^ localshift).  A slot that is homozygous with equal sure at the marker,
// or that the recursion does not reach, stays 0.  (movehaplos, cnF2freq.cpp:3601-3616, then turns the
// pair into haplobase/haplocount on the host, summed per individual.)
__global__ __launch_bounds__(64) void haplos_rows_kernel(Stage2Params q, uint32_t flags, double* out)
{
    const int g  = threadIdx.x;
    const int ml = blockIdx.x;
    const int m  = q.first + ml;
    const Window w = q.kp.windows[0];
    const double factor = q.loglik[0];
    const bool   nt = (flags & KP_NO_TIES) != 0;
    const int    n_combo = nt ? 1 : (1 << w.n_groups);
    double acc[7][2];
#pragma unroll
    for (int k = 0; k < 7; k++) acc[k][0] = acc[k][1] = 0.0;
    bool upd[7];                                   // doupdatehaplo of the slot at this marker
#pragma unroll
    for (int k = 0; k < 7; k++) {
        upd[k] = false;
        if (w.flags[k] & SLOT_PRESENT) {
            const Slot d = load_slot(q.kp, w.row[k], m);
            upd[k] = !(d.a0 == d.a1 && d.s0 == d.s1);          // cnF2freq.cpp:1235-1239
        }
    }
    const bool skip = isnan(factor) || factor < (double)CNF2_MINFACTOR_F;
    for (int s = 0; s < 8 && !skip; s++) {
        if ((s & w.shiftignore) || s >= w.shiftend) continue;
        if (factor - q.factors[s] > 40.0) continue;
        const double wg = s2_fw(q, s, ml, 0, g) * s2_fw(q, s, ml, 1, g) *
                          exp(s2_ff(q, s, ml, 0) + s2_ff(q, s, ml, 1) - factor);
        for (int f = 0; f < 2; f++) {
            LaneJob   L[2];
            LineTerms T[2];
            double    cf;
            bool      attop;
            s2_lines(q, w, m, g, s, f, &L[0], &L[1], &T[0], &T[1], &cf, &attop);
            // root: phase = f ^ shift bit 0 (firstpar is 0 at the root, cnF2freq.cpp:1156,1227)
            if (attop) {
                if (upd[0]) acc[0][f ^ (s & 1)] += wg * cf;
                continue;
            }
            for (int combo = 0; combo < n_combo; combo++) {
                int    force[2][3];                // [line][par, tr, ot]
                double r[2], t2;
                for (int P = 0; P < 2; P++) {
                    force[P][0] = nt ? -1 : tie_force(L[P].tie_par, combo);
                    force[P][1] = nt ? -1 : tie_force(L[P].tie_tr, combo);
                    force[P][2] = nt ? -1 : tie_force(L[P].tie_ot, combo);
                    line_restricted(L[P].cfg, T[P], force[P][0], force[P][1], force[P][2], &r[P], &t2);
                }
                const double e = (cf * r[1]) * r[0];
                if (upd[0]) acc[0][f ^ (s & 1)] += wg * e;
                for (int P = 0; P < 2; P++) {
                    const LineCfg& c = L[P].cfg;
                    if (!(c.par & SLOT_PRESENT)) continue;
                    const int  slot_par = 1 + 3 * P;
                    const int  ls = P ? (s >> 2) & 1 : (s >> 1) & 1;      // the parent's localshift
                    const bool interior = !(c.par & SLOT_FOUNDER);
                    for (int x = 0; x < 3; x++) {                          // 0 parent, 1 traced gp, 2 other gp
                        int slot;
                        if (x == 0) slot = slot_par;
                        else {
                            if (!interior) continue;
                            if (!((x == 1 ? c.tr : c.ot) & SLOT_PRESENT)) continue;
                            slot = slot_par + 1 + (x == 1 ? c.firstpar : (c.firstpar ^ 1));
                        }
                        if (!upd[slot]) continue;
                        for (int psi = 0; psi < 2; psi++) {
                            if (force[P][x] >= 0 && force[P][x] != psi) continue;   // tied slot: this combination fixes it
                            int fo[3] = {force[P][0], force[P][1], force[P][2]};
                            fo[x] = psi;
                            double rr;
                            line_restricted(c, T[P], fo[0], fo[1], fo[2], &rr, &t2);
                            const double ev = P ? (cf * rr) * r[0] : (cf * r[1]) * rr;
                            const int phase = (x == 0) ? (psi ^ ls) : psi;         // grandparents have localshift 0
                            acc[slot][phase] += wg * ev;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 7; k++)
#pragma unroll
        for (int ph = 0; ph < 2; ph++) {
            double v = acc[k][ph];
            v += lane_xor1(v);
            v += lane_xor2(v);
            v += dpp_mov_all<0x141>(v);
            v += lane_xor8(v);
            v += lane_xor16(v);
            v += lane_xor32(v);
            if (g == 0) out[((size_t)ml * 7 + k) * 2 + ph] = v;
        }
}

// ---------------------------------------------------------------------------------------------------
// Update-mode trackpossible for ONE path (flag99 >= 0), restated for the device: cnF2freq.cpp:1075-1359 with
// update in {GENOS = 2, HOMOZYGOUS = 4, GENOSPROBE = 8} (cnF2freq.cpp:792-795), zeropropagate = false,
// CORRECTIONINFERENCE = false.  A node is a window slot; the recursion depth is the template parameter
// (genwidth 4 -> 2 -> 1), so it unrolls into straight-line code.  GENOS adds updateval to
// inf[slot][allele index][markerval - 1] of every visited node of the traced line (cnF2freq.cpp:1351-1354).
// ---------------------------------------------------------------------------------------------------
#define TP_GENOS 2
#define TP_HOMOZYGOUS 4
#define TP_GENOSPROBE 8

__device__ __forceinline__ int tp_upflagit(int flag, int parnum, int genwidth)      // cnF2freq.cpp:321-329
{
    if (flag < 0) return flag;
    flag >>= parnum * (genwidth - 1);
    return flag & ((1 << (genwidth - 1)) - 1);
}

// NOEQ: zeropropagate = NO_EQUIVALENCE (cnF2freq.cpp:42): alleles are matched but an unknown incoming value is
// not bound (cnF2freq.cpp:311), every level weighs 0.5 instead of its phase weight (cnF2freq.cpp:1229-1233) and
// below the root only the traced line is followed (cnF2freq.cpp:1291); used by addvariance.
// CI: CORRECTIONINFERENCE is set (postmarkerdata, cnF2freq.cpp:8083-8085): a pair of equal alleles weighs 0 / 1 whatever
// its sure values are (cnF2freq.cpp:1235).
template <int GW, bool NOEQ = false, bool CI = false>
__device__ double tp_path(const KernelParams& p, const Window& w, int m, int slot, int inmv, double secondval,
                          unsigned flag, int flag99, int localshift, int update, double updateval, double* inf)
{
    const bool attopnow = !(update & TP_HOMOZYGOUS) && (GW == 1 || (w.flags[slot] & SLOT_FOUNDER));   // cpp:1120
    const Slot d        = load_slot(p, w.row[slot], m);
    const int  upflag2  = flag99 >> 1;                                   // cpp:1141-1146 (flag99 != -1)
    const int  upflag   = (int)(flag >> 1);
    const int  upshift  = localshift >> 1;
    const int  firstpar = flag & 1;                                      // cpp:1156
    const int  realf2n  = flag99 & 1;
    int        f2n      = realf2n;
    const int    mf = realf2n ? d.a1 : d.a0, mo = realf2n ? d.a0 : d.a1;
    const double sf = realf2n ? d.s1 : d.s0, so = realf2n ? d.s0 : d.s1;
    int    markerval;
    double baseval, mainsecondval = 0.0;
    const bool miss = markermiss(inmv, mf, &markerval);
    if (NOEQ && inmv == 0) markerval = 0;                                // cpp:311: no binding
    if (miss) {                                                          // cpp:1198-1202
        baseval = sf;
        if (sf != 0.0 && secondval != 0.0) mainsecondval = (1.0 - sf) * secondval;
    } else {                                                             // cpp:1203-1210
        const double esv = (inmv == 0 && markerval != 0) ? 1.0 : secondval;
        baseval          = 1.0 - sf;
        mainsecondval    = (mf == 0 ? 1.0 : sf) * esv;
    }
    if (attopnow) {                                                      // cpp:1213 (`update & 1` is false here)
        baseval += mainsecondval;
        mainsecondval = 0.0;
    } else if (mainsecondval != 0.0) mainsecondval /= baseval;
    f2n ^= (firstpar ^ localshift) & 1;                                  // cpp:1227
    if (NOEQ) baseval *= 0.5;                                            // cpp:1229-1233
    else if (d.a0 == d.a1 && (CI || d.s0 == d.s1)) baseval *= (f2n ? 1.0 : 0.0); // cpp:1235-1239
    else baseval *= fabs((f2n ? 1.0 : 0.0) - d.hw);                      // cpp:1245
    if constexpr (GW > 1) {
        if (baseval != 0.0 && !attopnow) {                               // cpp:1271
            const int down = update & ~TP_HOMOZYGOUS;                    // cpp:1280, 1322
            auto recurse = [&](int fp, int mv, double sv) -> double {    // recursetrackpossible, cpp:984-986, 1035-1057
                const int child = slot == 0 ? (fp ? 4 : 1) : slot + 1 + fp;
                if (!(w.flags[child] & SLOT_PRESENT)) return 1.0 + sv;   // cpp:1043-1046
                return tp_path<GW / 2, NOEQ, CI>(p, w, m, child, mv, sv, (unsigned)tp_upflagit(upflag, fp, GW),
                                       tp_upflagit(upflag2, fp, GW), tp_upflagit(upshift, fp, GW >> 1), down,
                                       updateval, inf);
            };
            if (!(update & TP_GENOS) && (!NOEQ || GW == 4)) {            // cpp:1291
                double secsecondval = 0.0;
                int    secmark      = mo;
                if (!(update & TP_HOMOZYGOUS)) {
                    if (so != 0.0) {                                     // cpp:1298-1302
                        baseval *= (1.0 - so);
                        secsecondval = so / (1.0 - so);
                    }
                } else if (markerval != secmark) {                       // cpp:1304-1313
                    if (secmark != 0) baseval *= so;
                    secmark = markerval;
                } else {                                                 // cpp:1314-1318
                    baseval *= (1.0 - so);
                }
                baseval *= recurse(firstpar ^ 1, secmark, secsecondval);
            }
            if (baseval != 0.0) baseval *= recurse(firstpar, markerval, mainsecondval);      // cpp:1336-1340
        }
    }
    if (baseval != 0.0 && (update & TP_GENOS) && (markerval == 1 || markerval == 2))        // cpp:1351-1354
        atomicAdd(inf + (slot * 2 + realf2n) * 2 + (markerval - 1), updateval);
    return baseval;
}

// infprobs / homozyg accumulators of HOT LOOP 2 at one marker (cnF2freq.cpp:5513-5577, DOINFPROBS), brute
// force like the reference: one thread per (shift mode, state, path).  out[0..27] = infprobs[slot][allele
// index][markerval - 1] before moveinfprobs (cnF2freq.cpp:3577-3597), out[28..29] = what is added to the
// individual's homozyg[marker].  Paths are masked as ignoreflag2 does where that changes a sum
// (flag2ignore and the all-or-none rule, cnF2freq.cpp:3478-3486; its third rule only drops zero terms).
__global__ __launch_bounds__(128) void infprobs_kernel(Stage2Params q, int marker, uint32_t flags, double* out)
{
    const int flag2 = threadIdx.x;            // 0..127
    const int g     = blockIdx.x & 63;
    const int s     = blockIdx.x >> 6;
    const Window w  = q.kp.windows[0];
    const double factor = q.loglik[0];
    if ((s & w.shiftignore) || s >= w.shiftend) return;
    if (isnan(factor) || factor < (double)CNF2_MINFACTOR_F) return;                   // cnF2freq.cpp:5403
    if (factor - q.factors[s] > 40.0) return;                                         // cnF2freq.cpp:5421
    if (flag2 & w.flag2ignore) return;                                                // cnF2freq.cpp:3478
    if (!(flags & KP_NO_TIES)) {
        for (int t = 0; t < w.n_groups; t++) {                                        // cnF2freq.cpp:3483-3486
            int mask = 0;
            for (int k = 0; k < 7; k++)
                if (w.tie[k] == t) mask |= 1 << k;
            const int filtered = (flag2 ^ (g * 2)) & mask;
            if (filtered && filtered != mask) return;
        }
    }
    // val of the path (as locked_query_kernel)
    const int ml = marker - q.first;
    const int f  = flag2 & 1;
    LaneJob   L0, L1;
    LineTerms T0, T1;
    double    cf;
    bool      attop;
    s2_lines(q, w, marker, g, s, f, &L0, &L1, &T0, &T1, &cf, &attop);
    double e;
    if (attop) e = cf;
    else {
        const int fp0 = (flag2 >> 1) & 1, fp1 = (flag2 >> 4) & 1;
        const int a0 = (flag2 >> (2 + L0.cfg.firstpar)) & 1, o0 = (flag2 >> (2 + (L0.cfg.firstpar ^ 1))) & 1;
        const int a1 = (flag2 >> (5 + L1.cfg.firstpar)) & 1, o1 = (flag2 >> (5 + (L1.cfg.firstpar ^ 1))) & 1;
        e = (cf * s2_path_term(L1.cfg, T1, fp1, a1, o1)) * s2_path_term(L0.cfg, T0, fp0, a0, o0);
    }
    const double am = s2_fw(q, s, ml, 0, g), be = s2_fw(q, s, ml, 1, g);
    const double lv = s2_ff(q, s, ml, 0) + log(am * e) + s2_ff(q, s, ml, 1) + log(be) - factor;
    if (!(isfinite(lv) && lv > -200.0)) return;                                       // cnF2freq.cpp:5502
    const double val = exp(lv);

    const KernelParams& p = q.kp;
    double sidevals[2][2], sums[2] = {0.0, 0.0}, homozyg[2];
    for (int side = 0; side < 2; side++)                                              // cnF2freq.cpp:5519-5528
        for (int i = 1; i <= 2; i++) {
            const double sv = tp_path<4>(p, w, marker, 0, i, 0.0, (unsigned)(g * 2 + side), flag2 ^ side, s,
                                         TP_GENOSPROBE, 0.0, nullptr);
            sidevals[side][i - 1] = sv;
            sums[side] += sv;
        }
    for (int i = 1; i <= 2; i++)                                                      // cnF2freq.cpp:5531-5537
        homozyg[i - 1] = tp_path<4>(p, w, marker, 0, i, 0.0, (unsigned)(g * 2), flag2, s, TP_HOMOZYGOUS, 0.0, nullptr);
    for (int side = 0; side < 2; side++)                                              // cnF2freq.cpp:5560-5568
        for (int i = 1; i <= 2; i++)
            tp_path<4>(p, w, marker, 0, i, 0.0, (unsigned)(g * 2 + side), flag2 ^ side, s, TP_GENOS,
                       val * sidevals[side][i - 1] / sums[side], out);
    for (int i = 1; i <= 2; i++) atomicAdd(out + 28 + (i - 1), val * homozyg[i - 1] / sums[0]);   // cnF2freq.cpp:5571-5575
}

// The same accumulators for every marker of the chromosome through the closed form of cnf2_accum.h (one
// line at a time instead of 128 paths per state and mode): out[len][30] = infprobs[7][2][2] then homozyg[2].
__global__ __launch_bounds__(64) void infprobs_rows_kernel(Stage2Params q, uint32_t flags, double* out)
{
    const int g  = threadIdx.x;
    const int ml = blockIdx.x;
    const int m  = q.first + ml;
    const Window w = q.kp.windows[0];
    const double factor = q.loglik[0];
    double acc[30];
#pragma unroll
    for (int k = 0; k < 30; k++) acc[k] = 0.0;
    Slot slot[7];
#pragma unroll
    for (int k = 0; k < 7; k++) slot[k] = load_slot(q.kp, w.row[k] < 0 ? 0 : w.row[k], m);
    const bool skip = isnan(factor) || factor < (double)CNF2_MINFACTOR_F;              // cnF2freq.cpp:5403
    for (int s = 0; s < 8 && !skip; s++) {
        if ((s & w.shiftignore) || s >= w.shiftend) continue;
        if (factor - q.factors[s] > 40.0) continue;                                    // cnF2freq.cpp:5421
        const double wg = s2_fw(q, s, ml, 0, g) * s2_fw(q, s, ml, 1, g) *
                          exp(s2_ff(q, s, ml, 0) + s2_ff(q, s, ml, 1) - factor);
        if (wg != 0.0) accum_infprobs(w, slot, g, s, wg, (flags & KP_NO_TIES) != 0, acc, acc + 28);
    }
    for (int k = 0; k < 30; k++) {
        double v = acc[k];
        v += lane_xor1(v);
        v += lane_xor2(v);
        v += dpp_mov_all<0x141>(v);
        v += lane_xor8(v);
        v += lane_xor16(v);
        v += lane_xor32(v);
        if (g == 0) out[(size_t)ml * 30 + k] = v;
    }
}

// individ::addvariance (cnF2freq.cpp:1489-1558) for the analysed individual of windows[0] and every marker in
// [first, first + len): trackpossible<false, NO_EQUIVALENCE> fed the individual's own two alleles (their sure
// as error odds) over shift modes 0-1, the 128 flags i = 2 g + firstpar and the admissible paths; per
// (shift, i & 1, flag2 & 1) the signed sum over the two alleles is squared.  out[ml] = variance, NaN when every
// term is zero (the reference leaves variances[marker] alone).  One block per marker, brute force.
__global__ __launch_bounds__(256) void addvariance_kernel(KernelParams p, int first, double* out)
{
    __shared__ double red_ok[8][256], red_full[256];
    const int    m  = first + blockIdx.x;
    const Window w  = p.windows[blockIdx.y];
    const Slot   me = load_slot(p, w.row[0], m);
    double ok[8], full = 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) ok[k] = 0.0;
    // 2 shifts x 128 flags x 128 paths = 32768 (shift, i, flag2) triples, 128 per thread
    for (int t = threadIdx.x; t < 2 * 128 * 128; t += 256) {
        const int flag2 = t & 127, i = (t >> 7) & 127, shift = t >> 14;
        if (flag2 & w.flag2ignore) continue;
        double d = 0.0;
        for (int allele = 0; allele < 2; allele++) {
            const double term = tp_path<4, true>(p, w, m, 0, allele ? me.a1 : me.a0, allele ? me.s1 : me.s0, (unsigned)i,
                                                 flag2, shift, 0, 0.0, nullptr);
            d += allele ? term : -term;
            full += term;
        }
        ok[(shift << 2) | ((i & 1) << 1) | (flag2 & 1)] += d;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) red_ok[k][threadIdx.x] = ok[k];
    red_full[threadIdx.x] = full;
    __syncthreads();
    if (threadIdx.x < 9) {
        const double* src = threadIdx.x < 8 ? red_ok[threadIdx.x] : red_full;
        double acc = 0.0;
        for (int k = 0; k < 256; k++) acc += src[k];
        if (threadIdx.x < 8) red_ok[threadIdx.x][0] = acc;
        else red_full[0] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sq = 0.0;
        for (int k = 0; k < 8; k++) sq += red_ok[k][0] * red_ok[k][0];
        out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red_full[0] != 0.0 ? sq : nan("");
    }
}

// fixparents' admissibility test (cnF2freq.cpp:1411-1431) for window y of p.windows at every marker: is there a state i
// and a path flag2 of parity b with a non-zero emission under shift mode 0, CORRECTIONINFERENCE set?  out[y][m][b].
// One thread per (marker, parity) tries the first paths of state 0, where nearly every admissible genotype is found at
// once; an item that found nothing there may need all 64 x 64 (state, path) pairs -- as a thread of its own it kept the
// other 63 lanes of its wavefront waiting for 4 096 evaluations (160 ms of a 5 000-individual set-up) -- so the wavefront
// takes such items one at a time, lane = state, and stops at the first path for which any state is non-zero.
__global__ __launch_bounds__(256) void okvals_kernel(KernelParams p, uint8_t* out)
{
    const int    t = blockIdx.x * blockDim.x + threadIdx.x;
    const int    lane = threadIdx.x & 63;
    const bool   live = t < p.n_markers * 2;
    const int    m = live ? t >> 1 : 0, b = t & 1;
    const Window w = p.windows[blockIdx.y];
    bool         ok = false;
    if (live)
        for (int flag2 = b; flag2 < 16 && !ok; flag2 += 2)
            ok = tp_path<4, false, true>(p, w, m, 0, 0, 0.0, 0u, flag2, 0, 0, 0.0, nullptr) != 0.0;
    unsigned long long pend = __ballot(live && !ok);
    while (pend) {
        const int L = __ffsll((long long)pend) - 1;
        pend &= pend - 1;
        const int mL = __shfl(m, L), bL = __shfl(b, L);
        bool      found = false;
        for (int flag2 = bL; flag2 < 128; flag2 += 2) {
            const double v = tp_path<4, false, true>(p, w, mL, 0, 0, 0.0, (unsigned)(lane * 2), flag2, 0, 0, 0.0, nullptr);
            if (__ballot(v != 0.0)) {
                found = true;
                break;
            }
        }
        if (lane == L) ok = found;
    }
    if (live) out[((size_t)blockIdx.y * p.n_markers + m) * 2 + b] = ok ? 1 : 0;
}
void launch_okvals(const KernelParams& p, int n_windows, uint8_t* out, hipStream_t stream)
{
    hipLaunchKernelGGL(okvals_kernel, dim3((p.n_markers * 2 + 255) / 256, n_windows), dim3(256), 0, stream, p, out);
}
void launch_addvariance_batch(const KernelParams& p, int n_windows, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(addvariance_kernel, dim3(p.n_markers, n_windows), dim3(256), 0, stream, p, 0, out);
}

// addvariance for window y of p.windows at every marker through its closed form (cnf2_variance.h): one thread per
// (window, marker) instead of 65 536 emission calls.  out[y][m], NaN where the reference leaves the entry alone.
__global__ __launch_bounds__(256) void variance_closed_kernel(KernelParams p, double* out)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= p.n_markers) return;
    const Window w = p.windows[blockIdx.y];
    Slot slot[7];
#pragma unroll
    for (int k = 0; k < 7; k++) slot[k] = load_slot(p, w.row[k] < 0 ? 0 : w.row[k], m);
    bool         valid;
    const double v = variance_closed(w, slot, &valid);
    out[(size_t)blockIdx.y * p.n_markers + m] = valid ? v : nan("");
}
void launch_variance_closed(const KernelParams& p, int n_windows, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(variance_closed_kernel, dim3((p.n_markers + 255) / 256, n_windows), dim3(256), 0, stream, p, out);
}

// addvariance for (window q of p.windows, markers[q]) with the reference's own rounding (variance_exact, cnf2_variance.h): four
// lanes per entry, one per class of the reference's loops -- 32 768 additions each, in the reference's order --, the first of
// them squares and adds the four.  out[q], NaN where the reference leaves the entry alone.  Called for the handful of markers
// per (record, chromosome) that can win lockhaplos' comparison, never for all.
__global__ __launch_bounds__(256) void variance_exact_kernel(KernelParams p, const int32_t* markers, int n, double* out)
{
    const int  t = blockIdx.x * blockDim.x + threadIdx.x;
    const int  k = t & 3;
    const bool live = (t >> 2) < n;
    const int  q = live ? t >> 2 : n - 1;
    const Window w = p.windows[q];
    const int    m = markers[q];
    Slot slot[7];
#pragma unroll
    for (int j = 0; j < 7; j++) slot[j] = load_slot(p, w.row[j] < 0 ? 0 : w.row[j], m);
    double ok, full;
    variance_exact_class(w, slot, k >> 1, k & 1, &ok, &full);
    double oks[4], fulls[4];
    const int base = (threadIdx.x & 63) & ~3;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        oks[j] = __shfl(ok, base + j);
        fulls[j] = __shfl(full, base + j);
    }
    if (live && k == 0) {
        bool         valid;
        const double v = variance_exact_finish(oks, fulls, &valid);
        out[q] = valid ? v : nan("");
    }
}
void launch_variance_exact(const KernelParams& p, const int32_t* markers, int n, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(variance_exact_kernel, dim3((n * 4 + 255) / 256), dim3(256), 0, stream, p, markers, n, out);
}

// =====================================================================================
// Batched HOT LOOP 2: every accumulator of cnF2freq.cpp:5416-5577 for one (job, marker)
// per wavefront, from the posterior weights a STOREW sweep left behind, through the table form of cnf2_acctab.h:
//   1. lane = table entry (P, f, sp, k): its AK_COUNT per-line sums (acc_entry) into LDS;
//   2. lane = (shift mode, low state bits) as in the sweep, registers = high state bits: the partial contractions
//      v (by f, s0), u (by f), z (by f, allele value) of wg with the restricted totals / HOMOZYGOUS probe sums;
//   3. lane = accumulator: 16-term dot products;
//   4. the per-locus reductions of doit (homozyg scale, moveinfprobs, movehaplos; cnF2freq.cpp:5876-5902,
//      3577-3616) with f64 atomics into the per-record arrays.
// Not tuned beyond the algebra (the table entries are evaluated by the plain host/device code of cnf2_accum.h).
// =====================================================================================
// What a window member receives at a locus (moveinfprobs / movehaplos, cnF2freq.cpp:3577-3616).  Default: f64 atomics on
// the per-record slabs (ranks and jobs add in whatever order they arrive).  CNF2_DETERMINISTIC (q.part != null): the six
// values go to the job's own row part[ind][m][slot][6] instead, and acc_gather_kernel adds the rows of a record in
// ascending order of the analysed individual -- one writer per element, the same sum to the bit on every run.
__device__ __forceinline__ void acc_emit(const AccParams& q, int ind, int slot, int rec, int m, const double inf[4], double norm,
                                         bool hap, double hbv, double hcv)
{
    const size_t M = (size_t)q.kp.n_markers;
    if (q.part) {
        double* d = q.part + (((size_t)ind * M + m) * 7 + slot) * 6;
#pragma unroll
        for (int t = 0; t < 4; t++) d[t] = inf[t] * norm;
        d[4] = hap ? hbv : 0.0;
        d[5] = hap ? hcv : 0.0;
        return;
    }
    double* dst = q.acc_inf + ((size_t)rec * M + m) * 4;
#pragma unroll
    for (int t = 0; t < 4; t++) atomicAdd(dst + t, inf[t] * norm);
    if (hap) {
        atomicAdd(q.acc_hb + (size_t)rec * M + m, hbv);
        atomicAdd(q.acc_hc + (size_t)rec * M + m, hcv);
    }
}

// CNF2_DETERMINISTIC: one thread per (record, marker) adds the rows its record received, in the order of list
// (ascending analysed individual, then slot): list[rec_start[r] .. rec_start[r + 1]) holds ind * 8 + slot.
__global__ __launch_bounds__(256) void acc_gather_kernel(AccParams q, const int32_t* rec_start, const int32_t* list, int n_rec)
{
    const size_t M = (size_t)q.kp.n_markers;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n_rec * M) return;
    const int    r = (int)(t / M), m = (int)(t % M);
    double       v[6] = {0, 0, 0, 0, 0, 0};
    for (int e = rec_start[r]; e < rec_start[r + 1]; e++) {
        const int     ind = list[e] >> 3, slot = list[e] & 7;
        const double* d = q.part + (((size_t)ind * M + m) * 7 + slot) * 6;
#pragma unroll
        for (int i = 0; i < 6; i++) v[i] += d[i];
    }
    double* dst = q.acc_inf + t * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) dst[i] += v[i];
    q.acc_hb[t] += v[4];
    q.acc_hc[t] += v[5];
}
void launch_acc_gather(const AccParams& q, const int32_t* rec_start, const int32_t* list, int n_rec, hipStream_t stream)
{
    const size_t n = (size_t)n_rec * q.kp.n_markers;
    hipLaunchKernelGGL(acc_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, q, rec_start, list, n_rec);
}

// The per-locus reductions of doit for one (job, marker) (cnF2freq.cpp:5876-5902, 3577-3616): out[44] = inf[7][2][2],
// homozyg[2], haplos[7][2] of the window's slots -> homozyg scale, moveinfprobs, movehaplos with f64 atomics.
__device__ __forceinline__ void acc_reduce_locus(const AccParams& q, const Job& jb, int m, int lane, double* out)
{
    const KernelParams& p = q.kp;
    const int32_t* srec = q.slot_rec + (size_t)jb.ind * 7;
    // this lane's own window member (lanes 0-6), read with the lane as index straight from memory
    const Window* wg = p.windows + jb.ind;
    const int     kk = lane < 7 ? lane : 0;
    const int     myrow = wg->row[kk];
    const Slot    mine = load_slot(p, myrow < 0 ? 0 : myrow, m);
    if (lane < 7) {
        // doupdatehaplo (cnF2freq.cpp:1224-1239): nothing for a slot that is homozygous with equal sure here
        const bool upd = (wg->flags[kk] & SLOT_PRESENT) && !(mine.a0 == mine.a1 && mine.s0 == mine.s1);
        if (!upd) out[30 + kk * 2] = out[30 + kk * 2 + 1] = 0.0;
    }
    wave_lds_fence();
    double self0 = 0.0;
    for (int k = 0; k < 7; k++)
        if (srec[k] == srec[0]) self0 += out[(k * 2 + 0) * 2 + 0] + out[(k * 2 + 0) * 2 + 1];
    const double sum = 1.0 / self0;                                                            // cnF2freq.cpp:5880-5885
    if (lane < 2) q.acc_hz[((size_t)jb.ind * p.n_markers + m) * 2 + lane] = out[28 + lane] * sum;
    if (lane < 7) {
        const int k = lane, r = srec[k];
        bool first = r >= 0;
        for (int k2 = 0; k2 < k; k2++) first = first && (srec[k2] != r);                      // reltree: unique members
        if (first) {
            double inf[4] = {0, 0, 0, 0}, h0 = 0.0, h1 = 0.0;
            int    occ = 0;
            for (int k2 = k; k2 < 7; k2++) {
                if (srec[k2] != r) continue;
                for (int t = 0; t < 4; t++) inf[t] += out[k2 * 4 + t];
                h0 += out[30 + k2 * 2];
                h1 += out[30 + k2 * 2 + 1];
                // reltreeordered: the individual itself always, ancestors only when non-empty (cnF2freq.cpp:3111-3152)
                if (k2 == 0 || !q.rec_empty[r]) occ++;
            }
            const double descf = (double)q.desc[srec[0]];
            double       norm = sum * 2;                                                       // cnF2freq.cpp:3582-3587
            for (int t = 0; t < occ; t++) norm /= 2;
            norm *= descf;
            const bool   hap = (h0 != 0.0 || h1 != 0.0) && fabs(mine.hw - 0.5) < 0.5 - 1e-12;      // cnF2freq.cpp:3601-3616
            const double md = (double)0.000005f;
            const double b1 = h0 + exp(-400.0) * md * md * 0.5;
            const double b2 = h1 + exp(-400.0) * md * md * 0.5;
            acc_emit(q, jb.ind, k, r, m, inf, norm, hap, b1 / (b1 + b2) * descf, descf);
        }
    }
}

#define ACC_TAB (64 * AK_COUNT)
#define ACC_LDS (ACC_TAB + 64 + 32 + 64 + 48)
#ifndef CNF2_ACC_MINBLOCKS
#define CNF2_ACC_MINBLOCKS 2   /* 2 blocks per CU (<= 256 VGPRs): measured 1.8 x faster than 1 block at 280 VGPRs */
#endif
__global__ __launch_bounds__(CNF2_BLOCK, CNF2_ACC_MINBLOCKS) void acc_rows_kernel(AccParams q)
{
    __shared__ double lds[CNF2_WAVES_PER_BLOCK][ACC_LDS];
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int job  = blockIdx.x;
    const int ml   = blockIdx.y * CNF2_WAVES_PER_BLOCK + wib;
    const KernelParams& p = q.kp;
    const Job jb = p.jobs[job];
    const int len = jb.last - jb.first + 1;
    if (ml >= len) return;
    const int    m  = jb.first + ml;
    const double factor = p.loglik[(size_t)jb.ind * p.n_chrom + jb.chrom];
    if (isnan(factor) || factor < (double)CNF2_MINFACTOR_F) return;                     // cnF2freq.cpp:5403
    const Window w = p.windows[jb.ind];
    if (!(q.flags & KP_ACC_TABLE) && !(w.flags[0] & SLOT_FOUNDER)) return;               // acc_paths_kernel's
    double* tab = lds[wib];                    // [64 entries][AK_COUNT]
    double* vt  = tab + ACC_TAB;               // [f][s0][16]
    double* ut  = vt + 64;                     // [f][16]
    double* zt  = ut + 32;                     // [f][i][16]
    double* out = zt + 64;                     // [44]: inf 28, hz 2, hap 14

    // posterior weights of this lane's 8 states
    double x[8];
    {
        const double* wp = p.wbuf + ((size_t)job * p.wstride + ml) * 512;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double2 v2 = *(const double2*)(wp + k * 128 + lane * 2);
            x[2 * k]     = v2.x;
            x[2 * k + 1] = v2.y;
        }
    }
    Slot slot[7];
#pragma unroll
    for (int k = 0; k < 7; k++) slot[k] = load_slot(p, w.row[k] < 0 ? 0 : w.row[k], m);
    const bool no_ties    = (q.flags & KP_NO_TIES) != 0;
    const bool root_attop = (w.flags[0] & SLOT_FOUNDER) != 0;
    const int  n_combo    = (no_ties || root_attop) ? 1 : (1 << w.n_groups);
    const int  s = lane >> 3, s0 = s & 1, s1 = (s >> 1) & 1, s2 = (s >> 2) & 1, lo = state_lo(lane);
    // per root allele f (no run-time indexed arrays: everything the later steps need is selected from ar0 / ar1)
    AccRoot ar0, ar1;
    acc_root(slot[0], root_attop, 0, &ar0);
    acc_root(slot[0], root_attop, 1, &ar1);
    if (lane < 44) out[lane] = 0.0;

    for (int combo = 0; combo < n_combo; combo++) {
        // ---- 1. table entries
        wave_lds_fence();
        {
            double e[AK_COUNT];
            const bool f_e = ((lane >> 4) & 1) != 0;
            if (f_e ? ar1.live : ar0.live) {
                if (f_e) acc_entry(w, slot, lane, combo, no_ties, ar1, e);
                else acc_entry(w, slot, lane, combo, no_ties, ar0, e);
            } else {
#pragma unroll
                for (int k = 0; k < AK_COUNT; k++) e[k] = 0.0;
            }
#pragma unroll
            for (int k = 0; k < AK_COUNT; k++) tab[lane * AK_COUNT + k] = e[k];
        }
        wave_lds_fence();
        // ---- 2. partial contractions
#pragma unroll
        for (int f = 0; f < 2; f++) {
            const AccRoot& af = f ? ar1 : ar0;
            const double cf = af.live ? (s0 ? af.cf[1] : af.cf[0]) : 0.0;
            const double* t1 = tab + (size_t)((1 << 5) | (f << 4) | (s2 << 3)) * AK_COUNT;    // line 1 entries of this chain
            double tr = 0.0, th0 = 0.0, th1 = 0.0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const double cx = cf * x[j];
                if (cx != 0.0) {
                    tr += cx * t1[j * AK_COUNT + AK_R];
                    th0 += cx * t1[j * AK_COUNT + AK_HZ + 0];
                    th1 += cx * t1[j * AK_COUNT + AK_HZ + 1];
                }
            }
            // v: sum over s2 (lane bit 5); z: over s0 and s2 (lane bits 3, 5)
            tr += lane_xor32(tr);
            th0 += lane_xor32(th0);
            th1 += lane_xor32(th1);
            th0 += lane_xor8(th0);
            th1 += lane_xor8(th1);
            const int e0 = (s1 << 3) | lo;
            if (s2 == 0) vt[(f * 2 + s0) * 16 + e0] = tr;
            if (s2 == 0 && s0 == 0) {
                zt[(f * 2 + 0) * 16 + e0] = th0;
                zt[(f * 2 + 1) * 16 + e0] = th1;
            }
            // u: per high state j, sum over the chain's 8 lanes and over s0, s1 (lane bits 0-4)
            const double r0 = tab[(size_t)((0 << 5) | (f << 4) | (s1 << 3) | lo) * AK_COUNT + AK_R];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const double cx = cf * x[j];
                double       pj = (cx != 0.0) ? cx * r0 : 0.0;
                pj = chain_sum(pj);
                pj += lane_xor8(pj);
                pj += lane_xor16(pj);
                if ((lane & 31) == 0) ut[f * 16 + (s2 << 3) + j] = pj;
            }
        }
        wave_lds_fence();
        // ---- 3. lane = accumulator
        if (lane < 44) {
            double acc = 0.0;
            if (lane < 28) {                                   // inf[slot][allele index][i]
                const int slotk = lane >> 2, ax = (lane >> 1) & 1, i = lane & 1;
                if (slotk == 0) {
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        const AccRoot& af = f ? ar1 : ar0;
                        if (!af.live) continue;
                        if (root_attop) {
                            const bool side = (f != ax);
                            double     vsum = 0.0;
                            for (int e = 0; e < 16; e++) vsum += vt[(f * 2 + 0) * 16 + e] + vt[(f * 2 + 1) * 16 + e];
                            const double r0 = side ? af.Rs[1][0] : af.Rs[0][0], r1 = side ? af.Rs[1][1] : af.Rs[0][1];
                            acc += vsum * ((i ? r1 : r0) / (r0 + r1));
                        } else {
                            const int P = (f == ax) ? 0 : 1;                                   // fr = P ? f ^ 1 : f
                            for (int e = 0; e < 16; e++) {
                                const double wt = P ? ut[f * 16 + e] : vt[(f * 2 + 0) * 16 + e] + vt[(f * 2 + 1) * 16 + e];
                                acc += mul0(tab[(size_t)((P << 5) | (f << 4) | e) * AK_COUNT + AK_WROOT + i], wt);
                            }
                        }
                    }
                } else if (!root_attop) {
                    const int P = slotk >= 4, rel = slotk - (1 + 3 * P);                       // 0 parent, 1 / 2 grandparents
                    const int kind = rel == 0 ? AK_WPAR + ax * 2 + i : AK_WGP + ((rel - 1) * 2 + ax) * 2 + i;
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        if (!(f ? ar1.live : ar0.live)) continue;
                        for (int e = 0; e < 16; e++) {
                            const double wt = P ? ut[f * 16 + e] : vt[(f * 2 + 0) * 16 + e] + vt[(f * 2 + 1) * 16 + e];
                            acc += mul0(tab[(size_t)((P << 5) | (f << 4) | e) * AK_COUNT + kind], wt);
                        }
                    }
                }
            } else if (lane < 30) {                            // homozyg[i]
                const int i = lane - 28;
#pragma unroll
                for (int f = 0; f < 2; f++) {
                    const AccRoot& af = f ? ar1 : ar0;
                    if (!af.live) continue;
                    double t = 0.0;
                    for (int e = 0; e < 16; e++)
                        t += mul0(tab[(size_t)((0 << 5) | (f << 4) | e) * AK_COUNT + AK_HZ + i], zt[(f * 2 + i) * 16 + e]);
                    acc += (i ? af.hzscale[1] : af.hzscale[0]) * t;
                }
            } else {                                           // haplos[slot][phase]
                const int slotk = (lane - 30) >> 1, ph = (lane - 30) & 1;
                if (slotk == 0) {
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        if (!(f ? ar1.live : ar0.live)) continue;
                        const int s0v = f ^ ph;                                                // phase = f ^ s0
                        for (int e = 0; e < 16; e++)
                            acc += mul0(tab[(size_t)((0 << 5) | (f << 4) | e) * AK_COUNT + AK_R], vt[(f * 2 + s0v) * 16 + e]);
                    }
                } else if (!root_attop) {
                    const int P = slotk >= 4, rel = slotk - (1 + 3 * P);
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        if (!(f ? ar1.live : ar0.live)) continue;
                        for (int e = 0; e < 16; e++) {
                            const double wt = P ? ut[f * 16 + e] : vt[(f * 2 + 0) * 16 + e] + vt[(f * 2 + 1) * 16 + e];
                            acc += mul0(tab[(size_t)((P << 5) | (f << 4) | e) * AK_COUNT + AK_HAP + rel * 2 + ph], wt);
                        }
                    }
                }
            }
            out[lane] += acc;
        }
    }
    wave_lds_fence();
    acc_reduce_locus(q, jb, m, lane, out);
}

// ---------------------------------------------------------------------------------------------------
// The same accumulators in the path form of cnf2_accpath.h, for every window whose root is not the top of its own
// lines (the others stay with acc_rows_kernel).  One wavefront per (job, marker):
//   1. lane = path (P, f, fp, t, g1, g0): the line's three match terms, its GENOS weights and probe products -- once;
//   2. three butterfly stages (DPP on lane bits 0, 1, 3) turn paths into the 64 restricted totals and the
//      HOMOZYGOUS probe sums of line 1; into LDS in the emission-table numbering;
//   3. lane = (shift mode, low state bits): partial contractions v, u, z of the posterior weights (as acc_rows_kernel);
//   4. lane = entry: its weight from v / u / z; the transposed butterflies give every path the sum Omega of the
//      weights of the entries it belongs to, with the last stage kept split for each slot (HAPLOS phases);
//   5. lane = path: products, 8-lane sums, and a last gather by the 44 accumulators through LDS;
//   6. the per-locus reductions of doit (as acc_rows_kernel).
// ---------------------------------------------------------------------------------------------------
#define APL_RT   0                 /* [64] restricted totals, emission-table numbering */
#define APL_HT   64                /* [i][32] HOMOZYGOUS probe sums of the entries of line 1 */
#define APL_VT   128               /* [f][s0][s2][16] partial sums of v */
#define APL_ZT   256               /* [f][i][s0][s2][16] partial sums of z */
#define APL_UT   512               /* [f][16] */
#define APL_RED  544               /* [12 kinds][8 groups] */
#define APL_TW   640               /* [i][64] GENOS terms per path lane */
#define APL_OUT  768               /* [44] accumulators; [44..47] stay 0 (padding target of the gather lists) */
#define APL_OFF  816               /* [64][8] int: gather list of every accumulator lane */
#define APL_LDS  (816 + 256)
#define APL_ZERO (APL_OUT + 44)

template <int BIT>
__device__ __forceinline__ double path_xchg(double v)
{
    if (BIT == 0) return lane_xor1(v);
    if (BIT == 1) return lane_xor2(v);
    if (BIT == 2) return lane_xor4(v);
    return lane_xor8(v);
}
template <int BIT>
__device__ __forceinline__ double path_stage(double v, double own, double other)
{
    return own * v + other * path_xchg<BIT>(v);
}
// One halving step of a sum over lanes: of the pair (a, c) the lane keeps a (its bit BIT clear) or c (set) and adds
// the partner's copy of the same one; N values become N / 2, each summed over the lane pair.
template <int BIT>
__device__ __forceinline__ double halve_pair(double a, double c, bool bit)
{
    const double keep = bit ? c : a, send = bit ? a : c;
    return keep + path_xchg<BIT>(send);
}

#ifndef CNF2_APL_TILE
#define CNF2_APL_TILE 8            /* consecutive markers per wavefront (what depends on the window only is formed once) */
#endif
#ifndef CNF2_APL_MINBLOCKS
#define CNF2_APL_MINBLOCKS 2   /* 3 needs <= 168 VGPRs: 92 B of scratch and no faster */
#endif
__global__ __launch_bounds__(CNF2_BLOCK, CNF2_APL_MINBLOCKS) void acc_paths_kernel(AccParams q)
{
    __shared__ double lds[CNF2_WAVES_PER_BLOCK][APL_LDS];
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int job  = blockIdx.x;
    const int ml0  = (blockIdx.y * CNF2_WAVES_PER_BLOCK + wib) * CNF2_APL_TILE;
    const KernelParams& p = q.kp;
    const Job jb = p.jobs[job];
    const int len = jb.last - jb.first + 1;
    if (ml0 >= len) return;
    const double factor = p.loglik[(size_t)jb.ind * p.n_chrom + jb.chrom];
    if (isnan(factor) || factor < (double)CNF2_MINFACTOR_F) return;                     // cnF2freq.cpp:5403
    const Window w = p.windows[jb.ind];
    if (w.flags[0] & SLOT_FOUNDER) return;                                              // acc_rows_kernel's
    double* L = lds[wib];
    const bool no_ties = (q.flags & KP_NO_TIES) != 0;
    const int  n_combo = no_ties ? 1 : (1 << w.n_groups);
    // consumer role of this lane (step 3): shift mode bits and low state bits
    const int  s = lane >> 3, s0 = s & 1, s1 = (s >> 1) & 1, s2 = (s >> 2) & 1, lo = state_lo(lane);
    // path / entry role (steps 1, 2, 4, 5): this lane's line and what it reads of the window
    const int  P = lane >> 5, f = (lane >> 4) & 1, t = (lane >> 2) & 1;
    const int  eidx = path_entry_index(lane), e4 = eidx & 15;
    PathLine   ln;
    ln.fl_par  = P ? w.flags[4] : w.flags[1];
    ln.fl_a    = P ? w.flags[5] : w.flags[2];
    ln.fl_b    = P ? w.flags[6] : w.flags[3];
    ln.tie_par = P ? w.tie[4] : w.tie[1];
    ln.tie_a   = P ? w.tie[5] : w.tie[2];
    ln.tie_b   = P ? w.tie[6] : w.tie[3];
    const int row_root = w.row[0] < 0 ? 0 : w.row[0];
    int       row_par = P ? w.row[4] : w.row[1], row_a = P ? w.row[5] : w.row[2], row_b = P ? w.row[6] : w.row[3];
    row_par = row_par < 0 ? 0 : row_par;
    row_a   = row_a < 0 ? 0 : row_a;
    row_b   = row_b < 0 ? 0 : row_b;
    const uint32_t plan1 = path_coef_plan(ln, lane, 0, no_ties);
    const uint32_t outflags = ((ln.fl_par & SLOT_PRESENT) ? PO_PAR : 0) |
                              (((ln.fl_par & (SLOT_PRESENT | SLOT_FOUNDER)) == SLOT_PRESENT && (ln.fl_a & SLOT_PRESENT)) ? PO_G0 : 0) |
                              (((ln.fl_par & (SLOT_PRESENT | SLOT_FOUNDER)) == SLOT_PRESENT && (ln.fl_b & SLOT_PRESENT)) ? PO_G1 : 0) |
                              (((ln.fl_par & (SLOT_PRESENT | SLOT_FOUNDER)) == SLOT_PRESENT && ((t ? ln.fl_b : ln.fl_a) & SLOT_PRESENT)) ? PO_TR : 0);
    // gather list of this lane as an accumulator (step 5): which 8-lane sums / GENOS terms it adds up
    {
        int* off = (int*)(L + APL_OFF) + lane * 8;
        int  o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) o[k] = APL_ZERO;
        if (lane < 28) {
            const int slotk = lane >> 2, ax = (lane >> 1) & 1, i = lane & 1;
            const int PP = slotk >= 4, rel = slotk == 0 ? -1 : slotk - (1 + 3 * PP);
            if (slotk == 0) {                                             // root: allele index f ^ P; group = P<<2 | f<<1 | fp
                o[0] = APL_RED + i * 8 + (0 << 2 | ax << 1);
                o[1] = APL_RED + i * 8 + (0 << 2 | ax << 1 | 1);
                o[2] = APL_RED + i * 8 + (1 << 2 | (ax ^ 1) << 1);
                o[3] = APL_RED + i * 8 + (1 << 2 | (ax ^ 1) << 1 | 1);
            } else if (rel == 0) {                                        // parent: allele index fp
                if ((PP ? w.flags[4] : w.flags[1]) & SLOT_PRESENT) {
                    o[0] = APL_RED + i * 8 + (PP << 2 | 0 << 1 | ax);
                    o[1] = APL_RED + i * 8 + (PP << 2 | 1 << 1 | ax);
                }
            } else {                                                      // grandparent rel - 1 as the traced one: allele index g
                const int tt = rel - 1;
#pragma unroll
                for (int k = 0; k < 8; k++) {                             // over f, fp and the other grandparent's allele
                    const int ff = k & 1, pp = (k >> 1) & 1, go = k >> 2;
                    const int gg0 = tt ? go : ax, gg1 = tt ? ax : go;
                    o[k] = APL_TW + i * 64 + (PP << 5 | ff << 4 | pp << 3 | tt << 2 | gg1 << 1 | gg0);
                }
            }
        } else if (lane < 30) {
            const int i = lane - 28;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = APL_RED + (2 + i) * 8 + k;
        } else if (lane < 44) {
            const int slotk = (lane - 30) >> 1, ph = (lane - 30) & 1;
            const int PP = slotk >= 4, rel = slotk == 0 ? -1 : slotk - (1 + 3 * PP);
            const int kind = 4 + (rel + 1) * 2 + ph;                      // root, parent, grandparent 0, grandparent 1
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = APL_RED + kind * 8 + PP * 4 + k;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) off[k] = o[k];
        if (lane < 4) L[APL_ZERO + lane] = 0.0;
    }
    // per-locus reductions (step 6): what lanes 0-6 need of the window's members
    const int32_t* srec = q.slot_rec + (size_t)jb.ind * 7;
    const int      kk = lane < 7 ? lane : 0;
    const int      myrec = srec[kk];
    int            mymask = 0, mask0 = 0;                                 // slots holding the same record as mine / as the root
    {
        const int r0 = srec[0];
        for (int k2 = 0; k2 < 7; k2++) {
            const int r2 = srec[k2];
            if (r2 == myrec) mymask |= 1 << k2;
            if (r2 == r0) mask0 |= 1 << k2;
        }
    }
    const bool   myfirst = lane < 7 && myrec >= 0 && (mymask & ((1 << kk) - 1)) == 0;              // reltree: unique members
    const Window* wmem = p.windows + jb.ind;                              // own member: read with the lane as index from memory
    const int    myrow_raw = wmem->row[kk];
    const int    myrow = myrow_raw < 0 ? 0 : myrow_raw;
    const bool   mypresent = (wmem->flags[kk] & SLOT_PRESENT) != 0;
    double       mynorm = 0.0;                                            // 2 / 2^occ * descendants (cnF2freq.cpp:3582-3587)
    const double descf = (double)q.desc[srec[0]];
    if (myfirst) {
        // reltreeordered: the individual itself always, ancestors only when non-empty (cnF2freq.cpp:3111-3152)
        const int occ = q.rec_empty[myrec] ? (mymask & 1) : __popc(mymask);
        mynorm = 2.0;
        for (int k2 = 0; k2 < occ; k2++) mynorm *= 0.5;
        mynorm *= descf;
    }

  for (int mi = 0; mi < CNF2_APL_TILE; mi++) {
    const int ml = ml0 + mi;
    if (ml >= len) break;
    const int m = jb.first + ml;
    double x[8];
    {
        const double* wp = p.wbuf + ((size_t)job * p.wstride + ml) * 512;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double2 v2 = *(const double2*)(wp + k * 128 + lane * 2);
            x[2 * k]     = v2.x;
            x[2 * k + 1] = v2.y;
        }
    }
    const Slot root = load_slot(p, row_root, m);
    ln.par = load_slot(p, row_par, m);
    ln.gpa = load_slot(p, row_a, m);
    ln.gpb = load_slot(p, row_b, m);
    const Slot mine = load_slot(p, myrow, m);
    double     cf0, cf1, hzs0, hzs1;            // c_f(s0 of the consumer role) for f = 0, 1; HOMOZYGOUS scale of this lane's f
    bool       live;
    PathTerms  T;
    {
        const double c0 = path_root_cbase(root, 0), c1 = path_root_cbase(root, 1);
        const double p0 = phase_weight(root, 0), p1 = phase_weight(root, 1);
        const bool   live0 = (c0 * p0 != 0.0) || (c0 * p1 != 0.0), live1 = (c1 * p0 != 0.0) || (c1 * p1 != 0.0);
        cf0  = live0 ? c0 * (s0 ? p1 : p0) : 0.0;              // c_0(s0) = cbase_0 * phase weight(0 ^ s0)
        cf1  = live1 ? c1 * (s0 ? p0 : p1) : 0.0;
        live = f ? live1 : live0;
        PathRoot pr;
        path_root(root, f, P, &pr);
        hzs0 = pr.hzscale0;
        hzs1 = pr.hzscale1;
        path_terms(ln, lane, pr, &T);
    }
    if (!live) T.term0 = T.k0 = T.k1 = 0.0;
    wave_lds_fence();
    if (lane < 44) L[APL_OUT + lane] = 0.0;

    for (int combo = 0; combo < n_combo; combo++) {
        PathCoef C;
        uint32_t plan = plan1;
        if (__builtin_amdgcn_readfirstlane(n_combo) != 1) plan = path_coef_plan(ln, lane, combo, no_ties);
        path_coef_apply(plan, ln, &C);
        // ---- 2. paths -> entries
        wave_lds_fence();
        {
            double R = T.term0, H0 = T.k0, H1 = T.k1;
            R  = path_stage<0>(R, C.g0_s, C.g0_f);
            H0 = path_stage<0>(H0, C.g0_s, C.g0_f);
            H1 = path_stage<0>(H1, C.g0_s, C.g0_f);
            R  = path_stage<1>(R, C.g1_s, C.g1_f);
            H0 = path_stage<1>(H0, C.g1_s, C.g1_f);
            H1 = path_stage<1>(H1, C.g1_s, C.g1_f);
            R  = path_stage<3>(R, C.par_s, C.par_f);
            H0 = path_stage<3>(H0, C.par_s, C.par_f);
            H1 = path_stage<3>(H1, C.par_s, C.par_f);
            L[APL_RT + eidx] = R;
            if (P) {
                L[APL_HT + (eidx & 31)]      = H0;
                L[APL_HT + 32 + (eidx & 31)] = H1;
            }
        }
        wave_lds_fence();
        const double Rmine = L[APL_RT + eidx];
        // ---- 3. partial contractions (lane = shift mode and low state bits, registers = high state bits)
        {
            const int e0 = (s1 << 3) | lo;
            double    uu[16];                                             // [f][j]: this lane's terms of u
#pragma unroll
            for (int ff = 0; ff < 2; ff++) {
                const double  cf = ff ? cf1 : cf0;
                const double* t1 = L + APL_RT + ((1 << 5) | (ff << 4) | (s2 << 3));      // line 1 entries of this chain
                const double* h0 = L + APL_HT + ((ff << 4) | (s2 << 3));
                const double* h1 = h0 + 32;
                const double  r0 = cf * L[APL_RT + ((0 << 5) | (ff << 4) | (s1 << 3) | lo)];
                double tr = 0.0, th0 = 0.0, th1 = 0.0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    tr  = fma(x[j], t1[j], tr);
                    th0 = fma(x[j], h0[j], th0);
                    th1 = fma(x[j], h1[j], th1);
                    uu[ff * 8 + j] = x[j] * r0;
                }
                // v: still to be summed over s2; z: over s0 and s2 -- by the entry lanes that read them
                L[APL_VT + ((ff * 2 + s0) * 2 + s2) * 16 + e0]            = cf * tr;
                L[APL_ZT + (((ff * 2 + 0) * 2 + s0) * 2 + s2) * 16 + e0] = cf * th0;
                L[APL_ZT + (((ff * 2 + 1) * 2 + s0) * 2 + s2) * 16 + e0] = cf * th1;
            }
            // u[f][s2][j]: sum over the 32 lanes of this half (s0, s1, low bits), 16 values -> one per lane
            double h8[8], h4[4], h2[2];
#pragma unroll
            for (int k = 0; k < 8; k++) h8[k] = halve_pair<0>(uu[2 * k], uu[2 * k + 1], (lane & 1) != 0);
#pragma unroll
            for (int k = 0; k < 4; k++) h4[k] = halve_pair<1>(h8[2 * k], h8[2 * k + 1], (lane & 2) != 0);
#pragma unroll
            for (int k = 0; k < 2; k++) h2[k] = halve_pair<2>(h4[2 * k], h4[2 * k + 1], (lane & 4) != 0);
            double h1v = halve_pair<3>(h2[0], h2[1], (lane & 8) != 0);
            h1v += lane_xor16(h1v);
            // the lane holds index (f<<3 | j) = its low four lane bits
            if ((lane & 16) == 0) L[APL_UT + ((lane >> 3) & 1) * 16 + (s2 << 3) + (lane & 7)] = h1v;
        }
        wave_lds_fence();
        // ---- 4. lane = entry: weights, then entries -> paths
        double v0, v1, wt, z0 = 0.0, z1 = 0.0;
        {
            const double* vt = L + APL_VT + (f * 2) * 2 * 16 + e4;
            v0 = vt[0] + vt[16];
            v1 = vt[32] + vt[48];
            if (P == 0) {
                const double* zt = L + APL_ZT + (f * 2) * 4 * 16 + e4;
                z0 = (zt[0] + zt[16]) + (zt[32] + zt[48]);
                z1 = (zt[64] + zt[80]) + (zt[96] + zt[112]);
            }
            wt = P ? L[APL_UT + f * 16 + e4] : v0 + v1;
        }
        // HAPLOS of the root straight from the entries: phase f ^ s0 (cnF2freq.cpp:1227)
        double hr0 = 0.0, hr1 = 0.0;
        if (P == 0 && live) {
            const double a = Rmine * v0, b = Rmine * v1;               // totals and weights are finite: plain products
            hr0 = f ? b : a;
            hr1 = f ? a : b;
        }
        const double X1  = path_stage<1>(wt, C.g1_s, C.g1_r);
        const double X01 = path_stage<0>(X1, C.g0_s, C.g0_r);
        const double Y   = path_stage<3>(X1, C.par_s, C.par_r);
        const double X0  = path_stage<0>(wt, C.g0_s, C.g0_r);
        const double Z   = path_stage<3>(X0, C.par_s, C.par_r);
        z0 = path_stage<1>(z0, C.g1_s, C.g1_r);
        z1 = path_stage<1>(z1, C.g1_s, C.g1_r);
        z0 = path_stage<0>(z0, C.g0_s, C.g0_r);
        z1 = path_stage<0>(z1, C.g0_s, C.g0_r);
        z0 = path_stage<3>(z0, C.par_s, C.par_r);
        z1 = path_stage<3>(z1, C.par_s, C.par_r);
        const double o_par_self = C.par_s * X01, o_par_part = C.par_r * path_xchg<3>(X01);      // phase t / !t
        const double o_g0_self = C.g0_s * Y, o_g0_part = C.g0_r * path_xchg<0>(Y);              // phase 0 / 1
        const double o_g1_self = C.g1_s * Z, o_g1_part = C.g1_r * path_xchg<1>(Z);
        // ---- 5. lane = path
        double val[12];
        {
            const double c = (o_par_self + o_par_part) * T.term0;
            const bool   ok = c != 0.0 && T.den_ok;
            val[0] = ok ? c * T.w0 : 0.0;                               // GENOS terms
            val[1] = ok ? c * T.w1 : 0.0;
            const double c0 = z0 * T.term0, c1 = z1 * T.term0;          // HOMOZYGOUS (line 0)
            val[2] = (P == 0 && c0 != 0.0) ? hzs0 * (c0 * T.w0) : 0.0;
            val[3] = (P == 0 && c1 != 0.0) ? hzs1 * (c1 * T.w1) : 0.0;
            val[4] = hr0;
            val[5] = hr1;
            const double tp = (outflags & PO_PAR) ? T.term0 : 0.0, ta = (outflags & PO_G0) ? T.term0 : 0.0, tb = (outflags & PO_G1) ? T.term0 : 0.0;
            const double ps = tp * o_par_self, pp = tp * o_par_part;
            val[6] = t ? pp : ps;
            val[7] = t ? ps : pp;
            val[8]  = ta * o_g0_self;
            val[9]  = ta * o_g0_part;
            val[10] = tb * o_g1_self;
            val[11] = tb * o_g1_part;
        }
        L[APL_TW + lane]      = (outflags & PO_TR) ? val[0] : 0.0;
        L[APL_TW + 64 + lane] = (outflags & PO_TR) ? val[1] : 0.0;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            // sum over lane bits 0-2 (g0, g1, t): xor1, xor2, then the pairing i <-> 7 - i finishes it
            double v = val[k];
            v += lane_xor1(v);
            v += lane_xor2(v);
            v += dpp_mov_all<0x141>(v);
            if ((lane & 7) == 0) L[APL_RED + k * 8 + (lane >> 3)] = v;
        }
        wave_lds_fence();
        if (lane < 44) {
            const int* off = (const int*)(L + APL_OFF) + lane * 8;
            double     acc = 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) acc += L[off[k]];
            L[APL_OUT + lane] += acc;
        }
    }
    // ---- 6. per-locus reductions (cnF2freq.cpp:5876-5902, 3577-3616)
    double* out = L + APL_OUT;
    if (lane < 7) {
        // doupdatehaplo (cnF2freq.cpp:1224-1239): nothing for a slot that is homozygous with equal sure here
        const bool upd = mypresent && !(mine.a0 == mine.a1 && mine.s0 == mine.s1);
        if (!upd) out[30 + kk * 2] = out[30 + kk * 2 + 1] = 0.0;
    }
    wave_lds_fence();
    double self0 = 0.0;
    for (int mm = mask0; mm; mm &= mm - 1) {
        const int k = __ffs(mm) - 1;
        self0 += out[k * 4 + 0] + out[k * 4 + 1];
    }
    const double sum = 1.0 / self0;                                                                // cnF2freq.cpp:5880-5885
    if (lane < 2) q.acc_hz[((size_t)jb.ind * p.n_markers + m) * 2 + lane] = out[28 + lane] * sum;
    if (myfirst) {
        double inf[4] = {0, 0, 0, 0}, h0 = 0.0, h1 = 0.0;
        for (int mm = mymask; mm; mm &= mm - 1) {
            const int k2 = __ffs(mm) - 1;
#pragma unroll
            for (int i = 0; i < 4; i++) inf[i] += out[k2 * 4 + i];
            h0 += out[30 + k2 * 2];
            h1 += out[30 + k2 * 2 + 1];
        }
        const double norm = sum * mynorm;
        const bool   hap = (h0 != 0.0 || h1 != 0.0) && fabs(mine.hw - 0.5) < 0.5 - 1e-12;         // cnF2freq.cpp:3601-3616
        const double md = (double)0.000005f;
        const double b1 = h0 + exp(-400.0) * md * md * 0.5;
        const double b2 = h1 + exp(-400.0) * md * md * 0.5;
        acc_emit(q, jb.ind, kk, myrec, m, inf, norm, hap, b1 / (b1 + b2) * descf, descf);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// The path form once more, laid out like the sweep's tile producer (cnf2_accpath.h, "tile form"): a wavefront takes
// 8 consecutive markers of a job at a time and
//   A. lane = part x marker (part = P, f, traced grandparent): the match terms of its 8 paths, butterflies in
//      registers, its 8 restricted totals (and HOMOZYGOUS probe sums) into the marker's table in LDS;
//   B. marker by marker, lane = (shift mode, low state bits): the contractions v, u, z of the 512 posterior weights;
//   C. lane = part x marker again: the weights of its 8 entries back to paths, the sums over its paths;
//   D. lane = accumulator x marker: gathers over the parts; lane = window member x marker: the per-locus
//      reductions of doit with f64 atomics.
// A and C run once per 8 markers instead of once per marker: the per-path work of acc_paths_kernel divided by 8.
// Two wavefronts per block (25 KB of LDS each: three blocks per CU).  Windows with tie groups (a loop over phase
// combinations) stay with acc_paths_kernel.
// ---------------------------------------------------------------------------------------------------
#define APT_WAVES 2
#ifndef CNF2_APT_TILES
#define CNF2_APT_TILES 4           /* tiles (of 8 markers) per wavefront: amortises the per-job set-up */
#endif
#define APT_SSTRIDE 110            /* staging block of one marker: 4 (P, f) x 17 (16 sums over t, odd stride), then 8 parts x 5 (the
                                      traced grandparent's 4 infprobs sums) */
/* strides are padded so that the 8 markers of a tile (lane bits 0-2) fall into different LDS banks */
#define APT_TSTRIDE 138            /* table of one marker: R of line 0 [0, 32), of line 1 [34, 66), H[0] [68, 100), H[1] [102, 134) */
#define APT_R1    34
#define APT_H0    68
#define APT_H1    102
#define APT_VSTRIDE 162            /* V[f][s0][16] at 0, U[f][16] at 64, Z[f][i][16] at 96 */
#define APT_OSTRIDE 50
#define APT_TAB   0                /* [mi][APT_TSTRIDE]; later the staging blocks [mi][APT_SSTRIDE] */
#define APT_CF    (8 * APT_TSTRIDE) /* [mi][f][s0] */
#define APT_VUZ   (APT_CF + 32)    /* [mi][APT_VSTRIDE] */
#define APT_OUT   APT_VUZ           /* [mi][APT_OSTRIDE]: over the weights, once they have been read */
#define APT_LIST  (APT_VUZ + 8 * APT_VSTRIDE) /* int [44][2]: the two staged sums every accumulator adds (offsets inside a staging block) */
#define APT_LDS   (APT_LIST + 44)

__global__ __launch_bounds__(64 * APT_WAVES, 2) void acc_tile_kernel(AccParams q)
{
    __shared__ double lds[APT_WAVES][APT_LDS];
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int job  = blockIdx.x;
    const KernelParams& p = q.kp;
    const Job jb = p.jobs[job];
    const int len = jb.last - jb.first + 1;
    const int ml_wave = (blockIdx.y * APT_WAVES + wib) * (8 * CNF2_APT_TILES);
    if (ml_wave >= len) return;
    const double factor = p.loglik[(size_t)jb.ind * p.n_chrom + jb.chrom];
    if (isnan(factor) || factor < (double)CNF2_MINFACTOR_F) return;                     // cnF2freq.cpp:5403
    const Window w = p.windows[jb.ind];
    if (w.flags[0] & SLOT_FOUNDER) return;                                              // acc_rows_kernel's
    double* L = lds[wib];
    const bool no_ties = (q.flags & KP_NO_TIES) != 0;
    if (!no_ties && w.n_groups > 0) return;                                              // tie combinations: acc_paths_kernel's
    // role B: shift mode bits and low state bits
    const int  s = lane >> 3, s0 = s & 1, s1 = (s >> 1) & 1, s2 = (s >> 2) & 1, lo = state_lo(lane);
    // roles A, C: part and marker of the tile
    const int  part = lane >> 3, mi = lane & 7;
    const int  P = part >> 2, f = (part >> 1) & 1, t = part & 1;
    PathLine   ln;
    ln.fl_par  = P ? w.flags[4] : w.flags[1];
    ln.fl_a    = P ? w.flags[5] : w.flags[2];
    ln.fl_b    = P ? w.flags[6] : w.flags[3];
    ln.tie_par = P ? w.tie[4] : w.tie[1];
    ln.tie_a   = P ? w.tie[5] : w.tie[2];
    ln.tie_b   = P ? w.tie[6] : w.tie[3];
    const int row_root = w.row[0] < 0 ? 0 : w.row[0];
    int       row_par = P ? w.row[4] : w.row[1], row_a = P ? w.row[5] : w.row[2], row_b = P ? w.row[6] : w.row[3];
    row_par = row_par < 0 ? 0 : row_par;
    row_a   = row_a < 0 ? 0 : row_a;
    row_b   = row_b < 0 ? 0 : row_b;
    const uint32_t plan1 = path_mats_plan(ln, t, 0, no_ties);
    const bool     general = (ln.fl_par & (SLOT_PRESENT | SLOT_FOUNDER)) == SLOT_PRESENT;
    const bool     do_par = (ln.fl_par & SLOT_PRESENT) != 0;
    const bool     do_tr = general && ((t ? ln.fl_b : ln.fl_a) & SLOT_PRESENT), do_ot = general && ((t ? ln.fl_a : ln.fl_b) & SLOT_PRESENT);
    // where entry r = sp<<2 | b_ot<<1 | b_tr of this lane sits in the table: sp<<3 | u1<<2 | u0<<1 | t, the roles mapped
    // to grandparents 0 / 1 by t (two per-job offsets, as in the sweep's tile producer)
    const int      e_tr = t ? 4 : 2, e_ot = t ? 2 : 4;
    // gather lists (role D): the two staged sums every accumulator adds up; offsets inside a marker's staging block
    // ((P, f) block pf = P*2 + f at pf*17: 0-1 root infprobs [i], 2-5 parent [a][i], 6-7 homozyg [i], 8-9 HAPLOS of the root
    // [phase], 10-11 of the parent, 12-13 / 14-15 of grandparent 0 / 1; part block at 68 + part*5: traced grandparent [a][i])
    if (lane < 44) {
        int o2[2];
        if (lane < 28) {
            const int slotk = lane >> 2, ax = (lane >> 1) & 1, i = lane & 1;
            const int PP = slotk >= 4, rel = slotk == 0 ? -1 : slotk - (1 + 3 * PP);
            if (slotk == 0) {                                             // root: allele index f ^ P
                o2[0] = (0 * 2 + ax) * 17 + i;
                o2[1] = (1 * 2 + (ax ^ 1)) * 17 + i;
            } else if (rel == 0) {                                        // parent: allele index fp
                o2[0] = (PP * 2 + 0) * 17 + 2 + ax * 2 + i;
                o2[1] = (PP * 2 + 1) * 17 + 2 + ax * 2 + i;
            } else {                                                      // grandparent rel - 1 where it is the traced one
                o2[0] = 68 + (PP << 2 | 0 << 1 | (rel - 1)) * 5 + ax * 2 + i;
                o2[1] = 68 + (PP << 2 | 1 << 1 | (rel - 1)) * 5 + ax * 2 + i;
            }
        } else if (lane < 30) {
            o2[0] = 0 * 17 + 6 + (lane - 28);
            o2[1] = 1 * 17 + 6 + (lane - 28);
        } else {
            const int slotk = (lane - 30) >> 1, ph = (lane - 30) & 1;
            const int PP = slotk >= 4, rel = slotk == 0 ? -1 : slotk - (1 + 3 * PP);
            o2[0] = (PP * 2 + 0) * 17 + 8 + (rel + 1) * 2 + ph;
            o2[1] = (PP * 2 + 1) * 17 + 8 + (rel + 1) * 2 + ph;
        }
        int* list = (int*)(L + APT_LIST) + lane * 2;
        list[0] = o2[0];
        list[1] = o2[1];
    }
    // role D, per-locus reductions: lane = member k x marker
    const int      dk = lane >> 3;                                        // window slot 0-6 (7: idle)
    const int32_t* srec = q.slot_rec + (size_t)jb.ind * 7;
    const int      kk = dk < 7 ? dk : 0;
    const int      myrec = srec[kk];
    int            mymask = 0, mask0 = 0;                                 // slots holding the same record as mine / as the root
    {
        const int r0 = srec[0];
        for (int k2 = 0; k2 < 7; k2++) {
            const int r2 = srec[k2];
            if (r2 == myrec) mymask |= 1 << k2;
            if (r2 == r0) mask0 |= 1 << k2;
        }
    }
    const bool    myfirst = dk < 7 && myrec >= 0 && (mymask & ((1 << kk) - 1)) == 0;             // reltree: unique members
    const Window* wmem = p.windows + jb.ind;
    const int     myrow_raw = wmem->row[kk];
    const int     myrow = myrow_raw < 0 ? 0 : myrow_raw;
    const bool    mypresent = (wmem->flags[kk] & SLOT_PRESENT) != 0;
    const double  descf = (double)q.desc[srec[0]];
    double        mynorm = 0.0;                                           // 2 / 2^occ * descendants (cnF2freq.cpp:3582-3587)
    if (myfirst) {
        // reltreeordered: the individual itself always, ancestors only when non-empty (cnF2freq.cpp:3111-3152)
        const int occ = q.rec_empty[myrec] ? (mymask & 1) : __popc(mymask);
        mynorm = 2.0;
        for (int k2 = 0; k2 < occ; k2++) mynorm *= 0.5;
        mynorm *= descf;
    }

    for (int tile = 0; tile < CNF2_APT_TILES; tile++) {
        const int ml0 = ml_wave + tile * 8;
        if (ml0 >= len) break;
        const int nvalid = (len - ml0 < 8) ? len - ml0 : 8;
        const int mlc = ml0 + (mi < nvalid ? mi : nvalid - 1);            // lanes beyond the chromosome redo its last marker
        const int m = jb.first + mlc;
        // ---- A. paths of this lane's part at its marker
        const Slot root = load_slot(p, row_root, m);
        ln.par = load_slot(p, row_par, m);
        ln.gpa = load_slot(p, row_a, m);
        ln.gpb = load_slot(p, row_b, m);
        const Slot mine = load_slot(p, myrow, m);
        PathTile T;
        double   hzs0, hzs1;
        {
            const double cb = path_root_cbase(root, f);
            const double c0 = cb * phase_weight(root, f ^ 0), c1 = cb * phase_weight(root, f ^ 1);      // c_f(s0 = 0), c_f(1)
            const bool   live = (c0 != 0.0) || (c1 != 0.0);
            PathRoot pr;
            path_root(root, f, P, &pr);
            hzs0 = pr.hzscale0;
            hzs1 = pr.hzscale1;
            path_terms8(ln, t, pr, &T);
            if (!live) {
#pragma unroll
                for (int r = 0; r < 8; r++) T.term0[r] = T.k0[r] = T.k1[r] = 0.0;
            }
            wave_lds_fence();                                             // the previous tile's readers are done
            if ((part & 5) == 0) {                                        // P == 0, t == 0: one writer per f
                L[APT_CF + mi * 4 + f * 2 + 0] = c0;
                L[APT_CF + mi * 4 + f * 2 + 1] = c1;
            }
        }
        {
            PathMats M;
            path_mats_apply(plan1, ln, t, &M);
            {
                double R[8], H0[8], H1[8];
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    R[r]  = T.term0[r];
                    H0[r] = T.k0[r];
                    H1[r] = T.k1[r];
                }
                tile_fwd<0>(R, M.tr);
                tile_fwd<1>(R, M.ot);
                tile_fwd<2>(R, M.par);
                double* tab = L + APT_TAB + mi * APT_TSTRIDE + ((f << 4) | t);
#pragma unroll
                for (int r = 0; r < 8; r++)
                    tab[(P ? APT_R1 : 0) + ((r >> 2) << 3) + ((r & 2) ? e_ot : 0) + ((r & 1) ? e_tr : 0)] = R[r];
                if (P) {
                    tile_fwd<0>(H0, M.tr);
                    tile_fwd<0>(H1, M.tr);
                    tile_fwd<1>(H0, M.ot);
                    tile_fwd<1>(H1, M.ot);
                    tile_fwd<2>(H0, M.par);
                    tile_fwd<2>(H1, M.par);
#pragma unroll
                    for (int r = 0; r < 8; r++) {
                        const int e3 = ((r >> 2) << 3) + ((r & 2) ? e_ot : 0) + ((r & 1) ? e_tr : 0);
                        tab[APT_H0 + e3] = H0[r];
                        tab[APT_H1 + e3] = H1[r];
                    }
                }
            }
            wave_lds_fence();
            // ---- B. contractions, one marker at a time (every lane in the consumer role)
            double xn[8];                                                 // posterior weights of the next marker, in flight
            {
                const double* wp = p.wbuf + ((size_t)job * p.wstride + ml0) * 512;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double2 v2 = *(const double2*)(wp + k * 128 + lane * 2);
                    xn[2 * k]     = v2.x;
                    xn[2 * k + 1] = v2.y;
                }
            }
#ifdef CNF2_X_FUSEDACC   /* timing ablation only: the contractions come from the sweep (160 doubles per marker) */
            for (int mj = 0; mj < nvalid; mj++) {
                const double* wp = p.wbuf + ((size_t)job * p.wstride + (ml0 + mj)) * 160;
                double*       vuz = L + APT_VUZ + mj * APT_VSTRIDE;
                vuz[lane] = wp[lane];
                vuz[64 + lane] = wp[64 + lane];
                if (lane < 32) vuz[128 + lane] = wp[128 + lane];
            }
            (void)xn;
            for (int mj = 0; mj < 0; mj++) {
#else
            for (int mj = 0; mj < nvalid; mj++) {
#endif
                double x[8];
#pragma unroll
                for (int k = 0; k < 8; k++) x[k] = xn[k];
                if (mj + 1 < nvalid) {
                    const double* wp = p.wbuf + ((size_t)job * p.wstride + (ml0 + mj + 1)) * 512;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const double2 v2 = *(const double2*)(wp + k * 128 + lane * 2);
                        xn[2 * k]     = v2.x;
                        xn[2 * k + 1] = v2.y;
                    }
                }
                const double* tab = L + APT_TAB + mj * APT_TSTRIDE;
                double*       vuz = L + APT_VUZ + mj * APT_VSTRIDE;
                const int     e0 = (s1 << 3) | lo;
                double        uu[16];
#pragma unroll
                for (int ff = 0; ff < 2; ff++) {
                    const double  cf = L[APT_CF + mj * 4 + ff * 2 + s0];
                    const double* t1 = tab + APT_R1 + ((ff << 4) | (s2 << 3));            // line 1 entries of this chain
                    const double* h0 = tab + APT_H0 + ((ff << 4) | (s2 << 3));
                    const double* h1 = tab + APT_H1 + ((ff << 4) | (s2 << 3));
                    const double  r0 = cf * tab[(ff << 4) | (s1 << 3) | lo];
                    double tr = 0.0, th0 = 0.0, th1 = 0.0;
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        tr  = fma(x[j], t1[j], tr);
                        th0 = fma(x[j], h0[j], th0);
                        th1 = fma(x[j], h1[j], th1);
                        uu[ff * 8 + j] = x[j] * r0;
                    }
                    tr *= cf;
                    th0 *= cf;
                    th1 *= cf;
                    // v: sum over s2 (lane bit 5); z: over s0 and s2 (lane bits 3, 5)
                    tr += lane_xor32(tr);
                    th0 += lane_xor32(th0);
                    th1 += lane_xor32(th1);
                    th0 += lane_xor8(th0);
                    th1 += lane_xor8(th1);
                    if (s2 == 0) vuz[(ff * 2 + s0) * 16 + e0] = tr;
                    if (s2 == 0 && s0 == 0) {
                        vuz[96 + (ff * 2 + 0) * 16 + e0] = th0;
                        vuz[96 + (ff * 2 + 1) * 16 + e0] = th1;
                    }
                }
                // u[f][s2][j]: sum over the 32 lanes of this half, 16 values -> one per lane (index = low four lane bits).
                // (Measured alternatives: the weights read a second time in the transposed role, from memory or through
                // LDS, so that u sums in registers: 20 % fewer VALU instructions, 3-9 % slower -- the kernel waits on
                // dependent LDS / memory round trips at 1.5 waves per SIMD, not on the VALU.)
                double h8[8], h4[4], h2[2];
#pragma unroll
                for (int k = 0; k < 8; k++) h8[k] = halve_pair<0>(uu[2 * k], uu[2 * k + 1], (lane & 1) != 0);
#pragma unroll
                for (int k = 0; k < 4; k++) h4[k] = halve_pair<1>(h8[2 * k], h8[2 * k + 1], (lane & 2) != 0);
#pragma unroll
                for (int k = 0; k < 2; k++) h2[k] = halve_pair<2>(h4[2 * k], h4[2 * k + 1], (lane & 4) != 0);
                double h1v = halve_pair<3>(h2[0], h2[1], (lane & 8) != 0);
                h1v += lane_xor16(h1v);
                if ((lane & 16) == 0) vuz[64 + ((lane >> 3) & 1) * 16 + (s2 << 3) + (lane & 7)] = h1v;
            }
            wave_lds_fence();
            // ---- C. the weights of this lane's entries, back to its paths
            TileSums S;
            double   hroot0 = 0.0, hroot1 = 0.0;
            {
                const double* vuz = L + APT_VUZ + mi * APT_VSTRIDE;
                const double* tab = L + APT_TAB + mi * APT_TSTRIDE;
                double wt[8];
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    const int e4 = ((r >> 2) << 3) + ((r & 2) ? e_ot : 0) + ((r & 1) ? e_tr : 0) + t;
                    if (P) {
                        wt[r] = vuz[64 + f * 16 + e4];
                    } else {
                        const double v0 = vuz[(f * 2 + 0) * 16 + e4], v1 = vuz[(f * 2 + 1) * 16 + e4];
                        wt[r] = v0 + v1;
                        // HAPLOS of the root straight from the entries: phase f ^ s0 (cnF2freq.cpp:1227)
                        const double Re = tab[(f << 4) | e4];
                        const double a = Re * v0, b = Re * v1;
                        hroot0 += f ? b : a;
                        hroot1 += f ? a : b;
                    }
                }
                tile_accumulate(T, M, t, wt, do_par, do_tr, do_ot, do_tr, &S);
                S.hz[0] = S.hz[1] = 0.0;
                if (P == 0) {
                    double z[8];
#pragma unroll
                    for (int r = 0; r < 8; r++)
                        z[r] = vuz[96 + (f * 2 + 0) * 16 + ((r >> 2) << 3) + ((r & 2) ? e_ot : 0) + ((r & 1) ? e_tr : 0) + t];
                    S.hz[0] = tile_homozyg(T, M, z, T.w0, hzs0);
#pragma unroll
                    for (int r = 0; r < 8; r++)
                        z[r] = vuz[96 + (f * 2 + 1) * 16 + ((r >> 2) << 3) + ((r & 2) ? e_ot : 0) + ((r & 1) ? e_tr : 0) + t];
                    S.hz[1] = tile_homozyg(T, M, z, T.w1, hzs1);
                }
            }
            wave_lds_fence();                                             // tables and weights are read: stage over the tables
            {
                // sums over the two traced grandparents of a (P, f) first (lane bit 3), then one writer per pair
                double sv[16] = {S.inf_root[0], S.inf_root[1], S.inf_par[0][0], S.inf_par[0][1], S.inf_par[1][0], S.inf_par[1][1],
                                 S.hz[0], S.hz[1], hroot0, hroot1, S.hap_par[0], S.hap_par[1],
                                 t ? S.hap_ot[0] : S.hap_tr[0], t ? S.hap_ot[1] : S.hap_tr[1],        // grandparent 0: traced iff t == 0
                                 t ? S.hap_tr[0] : S.hap_ot[0], t ? S.hap_tr[1] : S.hap_ot[1]};
#pragma unroll
                for (int k = 0; k < 16; k++) sv[k] += lane_xor8(sv[k]);
                double* blk = L + APT_TAB + mi * APT_SSTRIDE;
                if (t == 0) {
                    double* st = blk + (part >> 1) * 17;
#pragma unroll
                    for (int k = 0; k < 16; k++) st[k] = sv[k];
                }
                double* sp = blk + 68 + part * 5;
                sp[0] = S.inf_tr[0][0];
                sp[1] = S.inf_tr[0][1];
                sp[2] = S.inf_tr[1][0];
                sp[3] = S.inf_tr[1][1];
            }
            wave_lds_fence();
            // ---- D1. lane = accumulator x marker
#pragma unroll
            for (int round = 0; round < 6; round++) {
                const int o = (lane >> 3) + 8 * round;
                if (o < 44) {
                    const int*    list = (const int*)(L + APT_LIST) + o * 2;
                    const double* st = L + APT_TAB + mi * APT_SSTRIDE;
                    L[APT_OUT + mi * APT_OSTRIDE + o] = st[list[0]] + st[list[1]];
                }
            }
        }
        wave_lds_fence();
        // ---- D2. per-locus reductions (cnF2freq.cpp:5876-5902, 3577-3616): lane = window member x marker
        double* out = L + APT_OUT + mi * APT_OSTRIDE;
        const bool valid = mi < nvalid;
        if (dk < 7) {
            // doupdatehaplo (cnF2freq.cpp:1224-1239): nothing for a slot that is homozygous with equal sure here
            const bool upd = mypresent && !(mine.a0 == mine.a1 && mine.s0 == mine.s1);
            if (!upd) out[30 + kk * 2] = out[30 + kk * 2 + 1] = 0.0;
        }
        wave_lds_fence();
        double self0 = 0.0;
        for (int mm = mask0; mm; mm &= mm - 1) {
            const int k = __ffs(mm) - 1;
            self0 += out[k * 4 + 0] + out[k * 4 + 1];
        }
        const double sum = 1.0 / self0;                                                            // cnF2freq.cpp:5880-5885
        if (valid && dk < 2) q.acc_hz[((size_t)jb.ind * p.n_markers + m) * 2 + dk] = out[28 + dk] * sum;
        if (valid && myfirst) {
            double inf[4] = {0, 0, 0, 0}, h0 = 0.0, h1 = 0.0;
            for (int mm = mymask; mm; mm &= mm - 1) {
                const int k2 = __ffs(mm) - 1;
#pragma unroll
                for (int i = 0; i < 4; i++) inf[i] += out[k2 * 4 + i];
                h0 += out[30 + k2 * 2];
                h1 += out[30 + k2 * 2 + 1];
            }
            const double norm = sum * mynorm;
            const bool   hap = (h0 != 0.0 || h1 != 0.0) && fabs(mine.hw - 0.5) < 0.5 - 1e-12;     // cnF2freq.cpp:3601-3616
            const double md = (double)0.000005f;
            const double b1 = h0 + exp(-400.0) * md * md * 0.5;
            const double b2 = h1 + exp(-400.0) * md * md * 0.5;
            acc_emit(q, jb.ind, kk, myrec, m, inf, norm, hap, b1 / (b1 + b2) * descf, descf);
        }
    }
}

void launch_acc_rows(const AccParams& q, hipStream_t stream)
{
    dim3 grid(q.n_jobs, (q.max_len + CNF2_WAVES_PER_BLOCK - 1) / CNF2_WAVES_PER_BLOCK);
    const int per_block = CNF2_WAVES_PER_BLOCK * CNF2_APL_TILE;
    dim3 gridp(q.n_jobs, (q.max_len + per_block - 1) / per_block);
    const int per_block_t = APT_WAVES * 8 * CNF2_APT_TILES;
    dim3 gridt(q.n_jobs, (q.max_len + per_block_t - 1) / per_block_t);
    if (!(q.flags & KP_ACC_TABLE)) {
        if (q.flags & KP_ACC_LANES) hipLaunchKernelGGL(acc_paths_kernel, gridp, dim3(CNF2_BLOCK), 0, stream, q);
        else hipLaunchKernelGGL(acc_tile_kernel, gridt, dim3(64 * APT_WAVES), 0, stream, q);
    }
    if (q.flags & (KP_ACC_TABLE | KP_ACC_ATTOP)) hipLaunchKernelGGL(acc_rows_kernel, grid, dim3(CNF2_BLOCK), 0, stream, q);
}

void launch_addvariance(const KernelParams& p, int first, int len, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(addvariance_kernel, dim3(len), dim3(256), 0, stream, p, first, out);
}

void launch_infprobs_rows(const Stage2Params& q, uint32_t flags, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(infprobs_rows_kernel, dim3(q.len), dim3(64), 0, stream, q, flags, out);
}

void launch_infprobs(const Stage2Params& q, int marker, uint32_t flags, double* out, hipStream_t stream)
{
    (void)hipMemsetAsync(out, 0, 30 * sizeof(double), stream);
    hipLaunchKernelGGL(infprobs_kernel, dim3(8 * 64), dim3(128), 0, stream, q, marker, flags, out);
}

void launch_locked_query(const Stage2Params& q, int marker, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(locked_query_kernel, dim3(512), dim3(128), 0, stream, q, marker, out);
}
void launch_turn_scan(const Stage2Params& q, int marker, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(turn_scan_kernel, dim3(1024), dim3(64), 0, stream, q, marker, out);
}
// every marker of the chromosome: out[len][128][8]
__global__ __launch_bounds__(64) void turn_scan_rows_kernel(Stage2Params q, double* out)
{
    const int k    = threadIdx.x;
    const int s    = blockIdx.x & 7;
    const int turn = blockIdx.x >> 3;
    const int ml   = blockIdx.y;
    const int xorturn = turn & 54;                                                      // cnF2freq.cpp:508
    const int shiftx  = (turn >> 6) | ((turn & 1) ? 2 : 0) | ((turn & 8) ? 4 : 0);     // cnF2freq.cpp:509-510
    const int s2      = s ^ shiftx;
    double v = s2_fw(q, s, ml, 2, k ^ xorturn) * s2_fw(q, s2, ml, 1, k);
    v += lane_xor1(v);
    v += lane_xor2(v);
    v += dpp_mov_all<0x141>(v);
    v += lane_xor8(v);
    v += lane_xor16(v);
    v += lane_xor32(v);
    if (k == 0) {
        double r = (v > 0.0) ? s2_ff(q, s, ml, 2) + s2_ff(q, s2, ml, 1) + log(v) : (double)CNF2_MINFACTOR_F;
        out[((size_t)ml * 128 + turn) * 8 + s] = r - q.loglik[0];
    }
}
void launch_turn_scan_rows(const Stage2Params& q, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(turn_scan_rows_kernel, dim3(1024, q.len), dim3(64), 0, stream, q, out);
}
void launch_haplos_rows(const Stage2Params& q, uint32_t flags, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(haplos_rows_kernel, dim3(q.len), dim3(64), 0, stream, q, flags, out);
}
void launch_state_rows(const Stage2Params& q, uint32_t flags, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(state_rows_kernel, dim3(q.len), dim3(64), 0, stream, q, flags, out);
}

static void zero_job_counter(const KernelParams& p, hipStream_t stream)
{
    if (p.job_next) (void)hipMemsetAsync(p.job_next, 0, sizeof(int), stream);
}

void launch_fb_packed(const KernelParams& p, int grid, hipStream_t stream)
{
    zero_job_counter(p, stream);
    hipLaunchKernelGGL(fb_packed_kernel, dim3(grid), dim3(CNF2_BLOCK), 0, stream, p);
}

// dynamic LDS of the tied instantiations: 8 table rows per wave, each with the restricted tables of two tie combinations
#define CNF2_TIED_LDS_BYTES (CNF2_WAVES_PER_BLOCK * 8 * (TAB_STRIDE + 128) * (int)sizeof(double))
template <bool HALF, int STOREW, bool XPOSE = false, bool TIED = false, bool UNI = false>
static void launch_fast_as(const KernelParams& p, int grid, hipStream_t stream)
{
    const auto kernel = fb_fast_kernel<HALF, STOREW, XPOSE, TIED, UNI>;
    static bool asked = false;       // (per instantiation; more than 64 KB of dynamic LDS has to be asked for once)
    if (TIED && !asked) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CNF2_TIED_LDS_BYTES);
        asked = true;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(CNF2_BLOCK), TIED ? CNF2_TIED_LDS_BYTES : 0, stream, p);
}
static constexpr int fast_key(int storew, bool half, bool xpose = false, bool tied = false)
{
    return storew | (half ? 16 : 0) | (xpose ? 32 : 0) | (tied ? 64 : 0);
}
hipError_t launch_fb_fast(const KernelParams& p, int grid, FastVariant v, hipStream_t stream)
{
    // the plain half-spill sweep: the uniform windows' jobs through the UNI instantiation, the others through the ordinary
    // one; a list that holds both is swept by both, one after the other in the same spill slots, each skipping the other
    // class and each with its own job counter.  The logarithms are taken once, after both
    const bool plain_half = fast_key(v.storew, v.half, v.xpose, v.tied) == fast_key(SW_PLAIN, true);
    const int  n_uni      = plain_half ? v.n_uniform : 0;
    // the groups of four of fb_unipack_kernel: their jobs are the list's tail, which no other kernel of the launch sweeps
    const int  n_pack     = plain_half && v.pack_groups && v.n_lines > 0 && p.line_rec && p.line_keys ? v.n_pack_groups : 0;
    const int  n_sweep    = p.n_jobs - 4 * n_pack;
    if (n_sweep < 0) return hipErrorInvalidValue;
    if (n_uni > 0 || n_pack > 0) {
        KernelParams pu = p;
        pu.n_jobs = n_sweep;
        if (pu.job_next) pu.job_next = v.job_next_uniform;
        const int gu = v.grid_uniform > 0 ? v.grid_uniform : grid;
        // the launch's line records first, on the same stream (rebuilt for every launch: the rows change between sweeps), then
        // the pairs of groups of four (eight jobs to a wave), the groups of four left, then the single windows that have their
        // lines among the records; then the others (n_uniform_rows
        // of the n_uniform jobs) through the UNI form with the ordinary producer -- all in the same spill slots, each with a job
        // counter of its own
        const bool records = v.n_lines > 0 && pu.line_rec && pu.line_keys && (v.n_uniform_rows < n_uni || n_pack > 0);
        if (records) {
            const size_t n_rec = (size_t)v.n_lines * p.n_markers * LINE_VALUES * 2;
            hipLaunchKernelGGL(line_records_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, stream, v.lines, v.n_lines,
                               p.allele8, p.sure, p.hw, p.n_markers, const_cast<LineRec*>(pu.line_rec));
            // (the pairs of groups first, eight jobs to a wave; the groups left behind them four to a wave)
            const int n_eight = n_pack > 0 ? v.n_pack_eights : 0;
            if (n_eight < 0 || 2 * n_eight > n_pack) return hipErrorInvalidValue;
            if (n_eight > 0) {
                KernelParams pk = pu;
                pk.pjobs   = v.pack_groups;
                pk.n_pjobs = n_eight;
                if (pk.job_next) pk.job_next = v.job_next_uniform + 3;
                zero_job_counter(pk, stream);
                hipLaunchKernelGGL(fb_unipack8_kernel, dim3(v.grid_pack8 > 0 ? v.grid_pack8 : gu), dim3(CNF2_BLOCK), 0, stream, pk);
                pu.clock_out = nullptr;
            }
            if (n_pack > 2 * n_eight) {
                KernelParams pk = pu;
                pk.pjobs   = v.pack_groups + 2 * n_eight;
                pk.n_pjobs = n_pack - 2 * n_eight;
                if (pk.job_next) pk.job_next = v.job_next_uniform + 2;
                zero_job_counter(pk, stream);
                hipLaunchKernelGGL(fb_unipack_kernel, dim3(v.grid_pack > 0 ? v.grid_pack : gu), dim3(CNF2_BLOCK), 0, stream, pk);
                pu.clock_out = nullptr;
            }
            if (v.n_uniform_rows < n_uni) {
                zero_job_counter(pu, stream);
                launch_fast_as<true, SW_PLAIN, false, false, true>(pu, gu, stream);
            }
        } else {
            pu.line_rec  = nullptr;
            pu.line_keys = nullptr;
        }
        if (n_uni > 0 && (!records || v.n_uniform_rows > 0)) {
            if (records) {
                pu.clock_out = nullptr;
                if (pu.job_next) pu.job_next = v.job_next_uniform + 1;
            }
            zero_job_counter(pu, stream);
            launch_fast_as<true, SW_PLAIN_UNIFORM_ROWS, false, false, true>(pu, gu, stream);
        }
        if (n_uni >= n_sweep) {
            launch_likelihood_logs(p, stream);
            return hipGetLastError();
        }
    }
    KernelParams po = p;
    po.n_jobs = n_sweep;
    if (n_pack > 0) po.clock_out = nullptr;
    if (n_uni > 0) po.flags |= KP_SKIP_UNIFORM;
    zero_job_counter(po, stream);
    switch (fast_key(v.storew, v.half, v.xpose, v.tied)) {       // the twenty-two instantiations there are (and UNI above)
    case fast_key(SW_PLAIN, true): launch_fast_as<true, SW_PLAIN>(po, grid, stream); break;
    case fast_key(SW_PLAIN, false): launch_fast_as<false, SW_PLAIN>(p, grid, stream); break;
    case fast_key(SW_PLAIN, true, true): launch_fast_as<true, SW_PLAIN, true>(p, grid, stream); break;
    case fast_key(SW_PLAIN, true, false, true): launch_fast_as<true, SW_PLAIN, false, true>(p, grid, stream); break;
    case fast_key(SW_WEIGHTS_ROWS, true): launch_fast_as<true, SW_WEIGHTS_ROWS>(p, grid, stream); break;
    case fast_key(SW_WEIGHTS_ROWS, true, false, true): launch_fast_as<true, SW_WEIGHTS_ROWS, false, true>(p, grid, stream); break;
    case fast_key(SW_ALPHA_BETA, true): launch_fast_as<true, SW_ALPHA_BETA>(p, grid, stream); break;
    case fast_key(SW_WEIGHTS, true): launch_fast_as<true, SW_WEIGHTS>(p, grid, stream); break;
    case fast_key(SW_CROSSOVERS, true): launch_fast_as<true, SW_CROSSOVERS>(p, grid, stream); break;
    case fast_key(SW_CROSSOVERS, false): launch_fast_as<false, SW_CROSSOVERS>(p, grid, stream); break;
    case fast_key(SW_VITERBI, true): launch_fast_as<true, SW_VITERBI>(p, grid, stream); break;
    case fast_key(SW_VITERBI, false): launch_fast_as<false, SW_VITERBI>(p, grid, stream); break;
    case fast_key(SW_SAMPLING, true): launch_fast_as<true, SW_SAMPLING>(p, grid, stream); break;
    case fast_key(SW_SAMPLING, false): launch_fast_as<false, SW_SAMPLING>(p, grid, stream); break;
    case fast_key(SW_POSTERIOR, true): launch_fast_as<true, SW_POSTERIOR>(p, grid, stream); break;
    case fast_key(SW_POSTERIOR, false): launch_fast_as<false, SW_POSTERIOR>(p, grid, stream); break;
    case fast_key(SW_LOO, true): launch_fast_as<true, SW_LOO>(p, grid, stream); break;
    case fast_key(SW_LOO, false): launch_fast_as<false, SW_LOO>(p, grid, stream); break;
    case fast_key(SW_ORIGINS, true): launch_fast_as<true, SW_ORIGINS>(p, grid, stream); break;
    case fast_key(SW_ORIGINS, false): launch_fast_as<false, SW_ORIGINS>(p, grid, stream); break;
    case fast_key(SW_DESCENT, true): launch_fast_as<true, SW_DESCENT>(p, grid, stream); break;
    case fast_key(SW_DESCENT, false): launch_fast_as<false, SW_DESCENT>(p, grid, stream); break;
    default: return hipErrorInvalidValue;
    }
    launch_likelihood_logs(p, stream);
    return hipGetLastError();
}

hipError_t launch_fb(const KernelParams& p, int grid, SweepVariant variant, hipStream_t stream, bool debug_store)
{
    const dim3 g(grid), b(CNF2_BLOCK);
    if (debug_store && variant != SW_PLAIN) return hipErrorInvalidValue;
    switch (variant) {                                               // the five instantiations there are
    case SW_PLAIN:
        if (debug_store) hipLaunchKernelGGL(fb_kernel<true>, g, b, 0, stream, p);
        else hipLaunchKernelGGL(fb_kernel<false>, g, b, 0, stream, p);
        break;
    case SW_WEIGHTS_ROWS: hipLaunchKernelGGL((fb_kernel<false, SW_WEIGHTS_ROWS>), g, b, 0, stream, p); break;
    case SW_ALPHA_BETA: hipLaunchKernelGGL((fb_kernel<false, SW_ALPHA_BETA>), g, b, 0, stream, p); break;
    case SW_CROSSOVERS: hipLaunchKernelGGL((fb_kernel<false, SW_CROSSOVERS>), g, b, 0, stream, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

void launch_row_flags(const uint8_t* allele8, const double2* sure, int n_rows, int n_markers, uint8_t* flags,
                      hipStream_t stream)
{
    hipLaunchKernelGGL(row_flags_kernel, dim3(n_rows), dim3(256), 0, stream, allele8, sure, n_markers, flags);
}

int fb_xo_blocks_per_cu()
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fb_kernel<false, SW_CROSSOVERS>, CNF2_BLOCK, 0) != hipSuccess) n = 1;
    return n < 1 ? 1 : n;
}

// =====================================================================================
// Batched turn scan (HOT LOOP 3, cnF2freq.cpp:5686-5752): rawervals[turn][s] =
// doanalyze<aroundturner>(turn, classicstop(q, -1)) - factor for every marker of every job of a turn-scan sweep.
// aroundturner(turn) XORs the states with turn & 54 and the shift mode with
// (turn >> 6) | (turn & 1 ? 2 : 0) | (turn & 8 ? 4 : 0) (cnF2freq.cpp:506-511), so
//     rawervals[turn][s] = log sum_k A_s(k ^ (turn & 54)) B_{s ^ shiftx}(k) + scales - factor:
// per (job, marker) 64 pairs of shift modes (s, s ^ sx) x 16 flips of state bits 1, 2, 4, 5 = 1 024 dot products of
// 64 terms -- 131 072 flops on 8.4 KB read: the kernel is bound by the f64 FMA rate, not by HBM.
// One wavefront per (job, marker), lane = sx << 3 | s.  The sweep's rows go through LDS once ([chain][k][l][2], rows
// padded to 66 doubles so that the 8 chains a read touches sit in different banks); a lane keeps its A_s whole in
// registers (64 doubles), streams B_{s ^ sx} from LDS (one 16-byte read per 32 FMAs) and runs 16 accumulators, one
// per flip: the flips are register renaming (A[l ^ L(x)][j ^ J(x)] with compile-time indices), there is no
// cross-lane sum and no multiply is done twice.  Scales are mantissa and binary exponent (CNF2_TURN_ROW), so the
// log-sum-exp over the admissible shift modes per turn (what the clause weights of cnF2freq.cpp:5800-5817 are made of)
// is exact scaling (frexp / ldexp), a halving exchange over the 8 lanes of a group that leaves every lane 2 of the
// group's 16 sums, and 2 logarithms per lane.  The full table costs 16 logarithms per lane (parity / debugging).
// Each wave walks CNF2_TURN_SPAN consecutive markers; the second wave of the SIMD computes while this one waits for its rows.
// =====================================================================================
// log of a positive normal double: frexp to [sqrt(1/2), sqrt(2)), log m = 2 atanh((m-1)/(m+1)) by its series to t^21
// (|t| <= 0.1716: remainder 6e-19), reciprocal-based quotient.  About a third of the library routine's instructions;
// absolute error of log m below 2e-16 (the turn scan is compared at 1e-9).
__device__ __forceinline__ double log_pos(double w)
{
    int    e;
    double m = frexp(w, &e);                     // [0.5, 1)
    const bool lowhalf = m < 0.70710678118654752440;
    m = lowhalf ? m + m : m;
    e = lowhalf ? e - 1 : e;
    const double n = m - 1.0, d = m + 1.0;
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    double t = n * r;
    t = fma(fma(-d, t, n), r, t);
    const double t2 = t * t;
    double p = 1.0 / 21.0;
    p = fma(p, t2, 1.0 / 19.0);
    p = fma(p, t2, 1.0 / 17.0);
    p = fma(p, t2, 1.0 / 15.0);
    p = fma(p, t2, 1.0 / 13.0);
    p = fma(p, t2, 1.0 / 11.0);
    p = fma(p, t2, 1.0 / 9.0);
    p = fma(p, t2, 1.0 / 7.0);
    p = fma(p, t2, 1.0 / 5.0);
    p = fma(p, t2, 1.0 / 3.0);
    p = p * t2;                                  // log m = 2 t (1 + p)
    const double lm = fma(t + t, p, t + t);
    const double ed = (double)e;
    return fma(ed, 0.69314718036912381649, fma(ed, 1.9082149292705877e-10, lm));   // ln 2 split: the high part has 21 trailing zero bits
}

// Sums over the 8 admissible shift modes of a lane group (lanes differing in bits 0-2) of acc[x] K 2^E for the 16 flips
// x, as mantissa sums w2[i] relative to 2^e2[i]: lane s returns the flips x = (s0 s1 s2 i), i = 0, 1 (halving exchange:
// after the step with partner lane ^ 1 a lane keeps the 8 flips whose bit 3 is its s bit 0, then bit 2 <- s bit 1,
// bit 1 <- s bit 2).  PER_FLIP: the reference exponent is the largest E + exponent(acc[x] K) of the flip (exact for
// any spread); otherwise the largest E of the group.
template <bool PER_FLIP>
__device__ __forceinline__ void turn_group_sums(const double (&acc)[16], double K, int E, bool s_ok, int s, double (&w2)[2], int (&e2)[2])
{
    const bool on0 = s_ok && K > 0.0;
    double mt[16];
    int    emax[16];
    if (PER_FLIP) {
#pragma unroll
        for (int x = 0; x < 16; x++) {
            const double kk = acc[x] * K;
            const bool   on = on0 && kk > 0.0;
            int          fe;
            const double fm = frexp(kk, &fe);
            const int    et = on ? E + fe : -(1 << 29);
            int          mx = et;
            mx = max(mx, __builtin_amdgcn_mov_dpp(mx, 0xB1, 0xF, 0xF, true));
            mx = max(mx, __builtin_amdgcn_mov_dpp(mx, 0x4E, 0xF, 0xF, true));
            mx = max(mx, __builtin_amdgcn_ds_swizzle(mx, (4 << 10) | 0x1F));
            emax[x] = mx;
            const int d = et - mx;
            mt[x] = (on && d > -1100) ? ldexp(fm, d) : 0.0;
        }
    } else {
        const int Ee = on0 ? E : -(1 << 29);
        int       mx = Ee;
        mx = max(mx, __builtin_amdgcn_mov_dpp(mx, 0xB1, 0xF, 0xF, true));
        mx = max(mx, __builtin_amdgcn_mov_dpp(mx, 0x4E, 0xF, 0xF, true));
        mx = max(mx, __builtin_amdgcn_ds_swizzle(mx, (4 << 10) | 0x1F));
        const double Ke = on0 ? K : 0.0;
        int          d  = Ee - mx;
        d = d < -2000 ? -2000 : d;
#pragma unroll
        for (int x = 0; x < 16; x++) {
            mt[x]   = ldexp(acc[x] * Ke, d);
            emax[x] = mx;
        }
    }
    const bool b0 = s & 1, b1 = s & 2, b2 = s & 4;
    double u[8], t4[4];
    int    eu[8], e4[4];
    // (both candidates are read before the choice: a conditional read of an array element would put the array in scratch)
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const double lo = mt[i], hi = mt[8 + i];
        const int    el = emax[i], eh = emax[8 + i];
        u[i]  = (b0 ? hi : lo) + lane_xor1(b0 ? lo : hi);
        eu[i] = b0 ? eh : el;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double lo = u[i], hi = u[4 + i];
        const int    el = eu[i], eh = eu[4 + i];
        t4[i] = (b1 ? hi : lo) + lane_xor2(b1 ? lo : hi);
        e4[i] = b1 ? eh : el;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const double lo = t4[i], hi = t4[2 + i];
        const int    el = e4[i], eh = e4[2 + i];
        w2[i] = (b2 ? hi : lo) + lane_xor4(b2 ? lo : hi);
        e2[i] = b2 ? eh : el;
    }
}

#ifndef CNF2_TURN_SPAN
#define CNF2_TURN_SPAN 8
#endif
constexpr int TURN_RS = 66;
// MFMA form: the 1 024 dot products of a unit are one 32 x 32 x 64 product C[(s, xa)][(s2, xb)] = sum_k A_s(k ^ F(xa))
// B_s2(k ^ F(xb)) -- the flip x = xa | xb << 2 splits into the two that move the lane-held state bits (on A) and the two
// that move the register-held ones (on B) -- run as 2 x 2 tiles x 16 k-steps of v_mfma_f64_16x16x4_f64.  The operands come
// from LDS images in which every state coordinate is an address bit of a chain's 512-byte row (the four a flip can move --
// fp, fq of the lane position, j1, j2 of the register index -- and the two none moves), so a flip is an XOR on the address;
// the coordinate the lane's own flip bit moves sits at 16 bytes, rows are 544 bytes apart: the 32 lanes a ds_read_b64 serves
// together then cover the 64 banks, and every read is the lane's base address (one of two, by that coordinate) plus an
// immediate.  The sums leave through a [s][s2][x] image in
// the same LDS and are read back by the lanes in the layout the rest of the kernel works in.
typedef double d4v __attribute__((ext_vector_type(4)));
constexpr int TURN_MRS = 68;          // doubles per chain row of the MFMA images (544 bytes)
constexpr int TURN_CS  = 18;          // doubles per (s, s2) cell of the image the sums leave through
constexpr int TURN_LDS_VALU = 16 * TURN_RS, TURN_LDS_MFMA = 64 * TURN_CS;
template <bool MFMA>
__global__ __launch_bounds__(CNF2_BLOCK, MFMA ? 4 : 2) void turn_rows_kernel(TurnParams q)
{
    __shared__ __attribute__((aligned(16))) double lds[CNF2_WAVES_PER_BLOCK][MFMA ? TURN_LDS_MFMA : TURN_LDS_VALU];
    static_assert(16 * TURN_MRS <= TURN_LDS_MFMA, "the operand images and the image of the sums share the LDS");
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int job  = blockIdx.x;
    const KernelParams& p = q.kp;
    const Job jb  = p.jobs[job];
    const int len = jb.last - jb.first + 1;
    const int ml0 = (blockIdx.y * CNF2_WAVES_PER_BLOCK + wib) * CNF2_TURN_SPAN;
    if (ml0 >= len) return;
    const int ml1 = (ml0 + CNF2_TURN_SPAN < len) ? ml0 + CNF2_TURN_SPAN : len;
    // the fast kernel's butterflies drop a constant per gap: its reported log-likelihood carries the chromosome's sum of
    // their logarithms, the stored alpha / beta do not
    const double factor = p.loglik[(size_t)jb.ind * p.n_chrom + jb.chrom] - (q.scaled_transitions ? p.chrom_logk[jb.chrom] : 0.0);
    const Window& w = p.windows[jb.ind];
    const int  s = lane & 7, sx = lane >> 3, s2 = s ^ sx;
    const bool s_ok = !(s & w.shiftignore) && s < w.shiftend;
    const int  n_ok = __builtin_popcountll(__ballot(s_ok) & 0xFFull);
    double*    L  = lds[wib];
    // where this lane's loads go: it holds chain lane >> 3, position lane & 7, registers 2k, 2k + 1 of the sweep's layout
    // (a chain's row is [k][l][2]: the 8 lanes a ds_write_b128 serves together cover the 32 banks)
    double*    Lw = L + (lane >> 3) * TURN_RS + (lane & 7) * 2;
    const double* Ap = L + s * TURN_RS;
    const double* Bp = L + (8 + s2) * TURN_RS;
    // turn bits 0, 3, 6 come from sx bits 1, 2, 0
    const int tshift = ((sx >> 1) & 1) | (((sx >> 2) & 1) << 3) | ((sx & 1) << 6);
    // MFMA form, byte offsets in the wave's LDS.  Loading role (chain lane >> 3, position l = lane & 7): the coordinates of
    // l that the position flips move -- fp (l ^ 2 flips it), fq (l ^ 7 flips it) -- and the one they leave alone, fu.
    int wA = 0, wB = 0, rAe = 0, rAo = 0, rBe = 0, rBo = 0, wC = 0, rC = 0;
    if (MFMA) {
        const int l = lane & 7, ch = lane >> 3;
        const int fp = ((l >> 1) ^ l) & 1, fq = l & 1, fu = (l ^ (l >> 2)) & 1;
        wA = ch * TURN_MRS * 8 + fp * 16 + fq * 32 + fu * 64;                      // + j1 * 128 + j2 * 256; j0 inside the 16 bytes
        wB = (8 + ch) * TURN_MRS * 8 + fp * 32 + fu * 64 + fq * 128;               // + j1 * 16 + j2 * 256
        // operand role: row / column lane & 15 = (mode lane & 7, low flip bit lane >> 3 & 1), k within the step = lane >> 4
        const int so = lane & 7, xbit = (lane >> 3) & 1, g = lane >> 4;
        const int baseA = so * TURN_MRS * 8 + (g >> 1) * 64 + (g & 1) * 8, baseB = baseA + 8 * TURN_MRS * 8;
        rAe = baseA + xbit * 16;      // slot c even: (c ^ xbit) * 16 = c * 16 + xbit * 16
        rAo = baseA - xbit * 16;      //        odd:                  = c * 16 - xbit * 16
        rBe = baseB + xbit * 16;
        rBo = baseB - xbit * 16;
        // sums: this lane holds column (s2 = lane & 7, xb bit 0 = lane >> 3 & 1), rows (lane >> 4) + 4 reg
        wC = ((g * 8 + so) * TURN_CS + xbit) * 8;
        rC = (s * 8 + s2) * TURN_CS * 8;
    }

    const double floor_r   = (double)CNF2_MINFACTOR_F - factor;
    const double floor_lse = n_ok > 0 ? floor_r + log((double)n_ok) : -INFINITY;

    d2v va[4], vb[4];
    d2v scA, scB;
    auto request = [&](int ml) {
        const double* wp = p.wbuf + ((size_t)job * p.wstride + ml) * CNF2_TURN_ROW;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            va[k] = __builtin_nontemporal_load((const d2v*)(wp + k * 128 + lane * 2));
            vb[k] = __builtin_nontemporal_load((const d2v*)(wp + 512 + k * 128 + lane * 2));
        }
        scA = *(const d2v*)(wp + 1024 + 4 * s);
        scB = *(const d2v*)(wp + 1024 + 4 * s2 + 2);
    };
#pragma unroll 1
    for (int ml = ml0; ml < ml1; ml++) {
        const int m = jb.first + ml;
        request(ml);
        const double K = scA.x * scB.x;         // scale of this lane's pair of modes: K * 2^E
        const int    E = (int)scA.y + (int)scB.y;
        double acc[16];
        if constexpr (MFMA) {
            wave_lds_fence();                   // the previous marker's read-back is done
#pragma unroll
            for (int k = 0; k < 4; k++) {
                *(d2v*)((char*)L + wA + ((k & 1) << 7) + ((k >> 1) << 8))  = va[k];      // j bits 1, 2 at 128, 256
                *(d2v*)((char*)L + wB + ((k & 1) << 4) + ((k >> 1) << 8))  = vb[k];      // j bits 1, 2 at 16, 256
            }
            wave_lds_fence();
            d4v c4[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int nt = 0; nt < 2; nt++) c4[mt][nt] = d4v{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < 16; ks++) {
                // k-step = the four movable state coordinates (fp, fq, j1, j2); the B image orders them (j1, j2, fp, fq)
                const int fp = ks & 1, fq = (ks >> 1) & 1, j1 = (ks >> 2) & 1, j2 = ks >> 3;
                double    a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    // tile t of the operand has its second flip on: fq for A, j2 for B; the first flip (fp / j1) is the lane's
                    // bit, folded into the base address
                    a[t] = *(const double*)((const char*)L + (fp ? rAo : rAe) + fp * 16 + (fq ^ t) * 32 + j1 * 128 + j2 * 256);
                    b[t] = *(const double*)((const char*)L + (j1 ? rBo : rBe) + j1 * 16 + fp * 32 + fq * 128 + (j2 ^ t) * 256);
                }
#pragma unroll
                for (int mt = 0; mt < 2; mt++)
#pragma unroll
                    for (int nt = 0; nt < 2; nt++)
                        c4[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mt], b[nt], c4[mt][nt], 0, 0, 0);
            }
            wave_lds_fence();                   // every lane's operand reads are done: the image of the sums takes the LDS
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int nt = 0; nt < 2; nt++)
#pragma unroll
                    for (int reg = 0; reg < 4; reg++)
                        *(double*)((char*)L + wC + ((reg & 1) * 32 * TURN_CS + ((2 * mt + (reg >> 1)) << 1) + 8 * nt) * 8) = c4[mt][nt][reg];
            wave_lds_fence();
#pragma unroll
            for (int x2 = 0; x2 < 8; x2++) {
                // the image keeps a cell's 16 sums in the order xb0 | xa << 1 | xb1 << 3 (the 16 lanes a ds_write_b64 serves
                // together then fall into different banks); x = xa | xb << 2
                const d2v t = *(const d2v*)((const char*)L + rC + x2 * 16);
                const int xa = x2 & 3, xb1 = x2 >> 2;
                acc[xa | (xb1 << 3)]     = t.x;
                acc[xa | 4 | (xb1 << 3)] = t.y;
            }
        } else {
            wave_lds_fence();                       // the previous marker's reads are done
    #pragma unroll
            for (int k = 0; k < 4; k++) {
                *(d2v*)(Lw + 16 * k)                = va[k];
                *(d2v*)(Lw + 8 * TURN_RS + 16 * k) = vb[k];
            }
            wave_lds_fence();
            double A[8][8];
    #pragma unroll
            for (int l = 0; l < 8; l++)
    #pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    const d2v t = *(const d2v*)(Ap + jj * 16 + l * 2);
                    A[l][2 * jj]     = t.x;
                    A[l][2 * jj + 1] = t.y;
                }
    #pragma unroll
            for (int x = 0; x < 16; x++) acc[x] = 0.0;
            // B of one position (8 doubles) is requested a position ahead; the scheduling barriers keep the compiler from
            // pulling all 32 reads to the front (128 registers it does not have)
            d2v bn[4];
    #pragma unroll
            for (int jj = 0; jj < 4; jj++) bn[jj] = *(const d2v*)(Bp + jj * 16);
    #pragma unroll
            for (int l = 0; l < 8; l++) {
                d2v b[4];
    #pragma unroll
                for (int jj = 0; jj < 4; jj++) b[jj] = bn[jj];
                if (l < 7) {
    #pragma unroll
                    for (int jj = 0; jj < 4; jj++) bn[jj] = *(const d2v*)(Bp + jj * 16 + (l + 1) * 2);
                }
                __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
                for (int jj = 0; jj < 4; jj++) {
    #pragma unroll
                    for (int x = 0; x < 16; x++) {
                        // x bit 0 -> state bit 1 (position ^ 2), 1 -> bit 2 (position ^ 7), 2 -> bit 4, 3 -> bit 5 (registers)
                        const int Lx = ((x & 1) ? 2 : 0) ^ ((x & 2) ? 7 : 0), Jx = ((x >> 2) & 3) << 1;
                        acc[x] = fma(A[l ^ Lx][(2 * jj) ^ Jx], b[jj].x, acc[x]);
                        acc[x] = fma(A[l ^ Lx][(2 * jj + 1) ^ Jx], b[jj].y, acc[x]);
                    }
                }
                // the sums are only used under `if (full)` / `if (lse)`: without this the compiler sinks all 1 024 FMAs below
                // the reads and holds every B value in registers
                asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7]),
                                  "+v"(acc[8]), "+v"(acc[9]), "+v"(acc[10]), "+v"(acc[11]), "+v"(acc[12]), "+v"(acc[13]), "+v"(acc[14]), "+v"(acc[15])
                             : : "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        double* full = q.rawervals ? q.rawervals + ((size_t)jb.ind * p.n_markers + m) * 1024 : nullptr;
        double* lse  = q.turn_lse ? q.turn_lse + ((size_t)jb.ind * p.n_markers + m) * 128 : nullptr;
        if (full) {
            const double base = (double)E * 0.69314718055994530942 - factor;
#pragma unroll
            for (int x = 0; x < 16; x++) {
                const int    turn = tshift | ((x & 1) << 1) | (((x >> 1) & 1) << 2) | (((x >> 2) & 1) << 4) | (((x >> 3) & 1) << 5);
                const double kk   = acc[x] * K;
                full[turn * 8 + s] = (kk > 0.0) ? base + log_pos(kk) : floor_r;
            }
        }
        if (lse) {
            // per flip x: sum over the admissible modes s of kk_s 2^E_s.  Usual case: the terms are scaled to the largest
            // exponent E of the group's admissible modes (one max per marker).  Where a sum comes out below 2^-700 --
            // every term an exact zero, or the mode with the largest E has no likelihood at this flip and the others sit
            // hundreds of binary orders below it -- the flips are redone with a maximum per flip (turn_group_sums<true>).
            double w2[2];
            int    e2[2];
            turn_group_sums<false>(acc, K, E, s_ok, s, w2, e2);
            const bool thin = w2[0] < 0x1p-700 || w2[1] < 0x1p-700;
            if (__any(thin)) {
                double w2r[2];
                int    e2r[2];
                turn_group_sums<true>(acc, K, E, s_ok, s, w2r, e2r);
#pragma unroll
                for (int i = 0; i < 2; i++)
                    if (w2[i] < 0x1p-700) {
                        w2[i] = w2r[i];
                        e2[i] = e2r[i];
                    }
            }
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int    x    = ((s & 1) << 3) | (((s >> 1) & 1) << 2) | (((s >> 2) & 1) << 1) | i;
                const int    turn = tshift | ((x & 1) << 1) | (((x >> 1) & 1) << 2) | (((x >> 2) & 1) << 4) | (((x >> 3) & 1) << 5);
                // no admissible mode with a positive sum: every one of them sits at the floor (cnF2freq.cpp:5802-5812)
                lse[turn] = (w2[i] > 0.0) ? ((double)e2[i] * 0.69314718055994530942 - factor) + log_pos(w2[i]) : floor_lse;
            }
        }
    }
}
void launch_turn_rows(const TurnParams& q, hipStream_t stream)
{
    const int per_block = CNF2_WAVES_PER_BLOCK * CNF2_TURN_SPAN;
    dim3 grid(q.n_jobs, (q.max_len + per_block - 1) / per_block);
    if (q.valu_form) hipLaunchKernelGGL(turn_rows_kernel<false>, grid, dim3(CNF2_BLOCK), 0, stream, q);
    else hipLaunchKernelGGL(turn_rows_kernel<true>, grid, dim3(CNF2_BLOCK), 0, stream, q);
}

// =====================================================================================
// Marker placement (cnf2_sweep_place): place[i][q][m] = log sum_(s, g) gamma_(s, m)(g) e'_(s, q)(g), the growth of individual
// i's log-likelihood when candidate marker q is laid on the map at mapped marker m.  gamma comes from a placement sweep
// (SW_POSTERIOR: 512 doubles per job and marker in p.wbuf), e' from place_emission_kernel in the same (k, lane, register)
// order, so the contraction index needs no permutation.
// =====================================================================================
// Emission tables of the candidates: one wave per (individual, candidate), through the producer / consumer code of
// emission_kernel on the candidate rows (p.n_markers = Q).  null_sum[q] += log of the mean over the individual's analysed
// shift modes of (1 / 64) sum_g e'(s, g), the unlinked baseline; an individual whose mean is 0 is left out.
__global__ __launch_bounds__(64) void place_emission_kernel(KernelParams p, int q0, int qcap, double* emis, double* null_sum)
{
    __shared__ double tab[64];
    const int    lane = threadIdx.x, ind = blockIdx.x, cand = q0 + blockIdx.y;
    const Window w    = p.windows[ind];
    LaneCtx      c;
    make_lane(w, lane, &c.L);
    c.row_root   = w.row[0];
    c.root_attop = (w.flags[0] & SLOT_FOUNDER) != 0;
    const int s  = lane >> 3;
    c.s0 = s & 1;
    c.s1 = (s >> 1) & 1;
    c.s2 = (s >> 2) & 1;
    c.lo = state_lo(lane);
    c.active = true;
    c.n_combo = 1;
    const Slot root = load_slot(p, c.row_root, cand);
    LineTerms  T;
    tab[lane] = produce_entry(p, c, root, cand, &T);
    wave_lds_fence();
    double c0, c1, e[8];
    root_weights(c, root, &c0, &c1);
    emission_from_table(tab, c, c0, c1, e);
    double* out = emis + ((size_t)ind * qcap + blockIdx.y) * 512;
#pragma unroll
    for (int k = 0; k < 4; k++) *(d2v*)(out + k * 128 + lane * 2) = d2v{e[2 * k], e[2 * k + 1]};
    if (null_sum) {
        const bool   on   = !(s & w.shiftignore) && s < w.shiftend;
        const double mine = chain_sum(((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
        const double tot  = across_chains_sum(on ? mine : 0.0);
        const int    n_on = __builtin_popcountll(__ballot(on)) >> 3;
        if (lane == 0 && n_on > 0 && tot > 0.0) atomicAdd(&null_sum[cand], log(tot / (64.0 * n_on)));
    }
}
void launch_place_emission(const KernelParams& cand, int n_ind, int q0, int qn, int qcap, double* emis, double* null_sum,
                           hipStream_t stream)
{
    if (n_ind > 0 && qn > 0)
        hipLaunchKernelGGL(place_emission_kernel, dim3(n_ind, qn), dim3(64), 0, stream, cand, q0, qcap, emis, null_sum);
}

// The contraction.  A wave owns a tile of 16 markers x 32 candidates of a chromosome (the four waves of a block: four
// consecutive marker tiles and the same candidates, so that no wave idles when Q is small and the four read the same
// candidate tables at the same time) and walks `group` consecutive jobs
// (individuals; the batch lists its jobs by chromosome): per job a [32 x 512] x [512 x 16] product as 2 x 128
// v_mfma_f64_16x16x4_f64 (A: row = lane & 15, k = lane >> 4; B: column = lane & 15, k = lane >> 4; D: column = lane & 15,
// row = (lane >> 4) + 4 reg) with the candidates as rows and the markers as columns, so that the 16 lanes of a result
// register hold 16 consecutive markers of one candidate: 128 contiguous bytes of place[] and of the sums.  Then a logarithm
// per cell, the cell into place[] where asked for -- and the tile's sums and
// zero counts stay in registers until the chromosome changes or the group ends: one f64 atomic per cell and group, not per
// cell and job.  The operands go through LDS in chunks of 32 of the 512 (coalesced 16-byte loads, the next chunk requested
// while this one is multiplied; rows 34 doubles apart: the 32 lanes a ds_read_b64 serves cover the 64 banks).  Markers past
// the chromosome's end and candidates past Q are zeros in the operands and masked in the outputs: nothing is padded in HBM.
constexpr int PLACE_KC = 32;                 // of the 512 per chunk
constexpr int PLACE_RS = PLACE_KC + 2;       // doubles per LDS row
constexpr int PLACE_NT = 2;                  // candidate tiles of 16 per wave
__global__ __launch_bounds__(CNF2_BLOCK) void place_rows_kernel(PlaceParams q)
{
    __shared__ __attribute__((aligned(16))) double lds[CNF2_WAVES_PER_BLOCK][16 * (1 + PLACE_NT) * PLACE_RS];
    const KernelParams& p = q.kp;
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qend = (q.q0 + q.qn < q.n_cand) ? q.q0 + q.qn : q.n_cand;
    const int qa   = q.q0 + blockIdx.z * 16 * PLACE_NT;      // the block's candidates; its waves take four marker tiles
    if (qa >= qend) return;
    const int ml0 = (blockIdx.y * CNF2_WAVES_PER_BLOCK + wib) * 16;
    const int j0  = blockIdx.x * q.group;
    const int j1  = (j0 + q.group < q.n_jobs) ? j0 + q.group : q.n_jobs;
    double*   LA  = lds[wib];
    double*   LB  = LA + 16 * PLACE_RS;
    const int lr = lane >> 4, lc = (lane & 15) * 2;      // loading role: row within a group of four, column pair
    const int oi = lane & 15, ok = lane >> 4;            // operand role

    d4v sum[PLACE_NT];
    int nz[PLACE_NT][4];
#pragma unroll
    for (int nt = 0; nt < PLACE_NT; nt++) {
        sum[nt] = d4v{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int reg = 0; reg < 4; reg++) nz[nt][reg] = 0;
    }
    int cur_chrom = -1, cur_first = 0, cur_len = 0;
    auto flush = [&]() {
        if (cur_chrom < 0) return;
#pragma unroll
        for (int nt = 0; nt < PLACE_NT; nt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int m = ml0 + oi, cand = qa + nt * 16 + ok + 4 * reg;
                if (m < cur_len && cand < qend) {
                    const size_t o = (size_t)cand * p.n_markers + cur_first + m;
                    if (sum[nt][reg] != 0.0) atomicAdd(&q.place_sum[o], sum[nt][reg]);
                    if (nz[nt][reg]) atomicAdd(&q.n_zero[o], nz[nt][reg]);
                }
                sum[nt][reg] = 0.0;
                nz[nt][reg]  = 0;
            }
    };
#pragma unroll 1
    for (int job = j0; job < j1; job++) {
        const Job jb  = p.jobs[job];
        const int len = jb.last - jb.first + 1;
        if (jb.chrom != cur_chrom) {
            flush();
            cur_chrom = jb.chrom;
            cur_first = jb.first;
            cur_len   = len;
        }
        if (ml0 >= len) continue;
        // a job without a likelihood is skipped, as the sweep skips it: no sums, CNF2_IGNORED in its cells
        if (p.lexp[(size_t)jb.ind * p.n_chrom + jb.chrom] == CNF2_LEXP_DEAD) {
            if (q.place) {
#pragma unroll
                for (int nt = 0; nt < PLACE_NT; nt++)
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const int m = ml0 + oi, cand = qa + nt * 16 + ok + 4 * reg;
                        if (m < len && cand < qend) q.place[((size_t)jb.ind * q.n_cand + cand) * p.n_markers + jb.first + m] = CNF2_IGNORED_D;
                    }
            }
            continue;
        }
        const double* A = p.wbuf + ((size_t)job * p.wstride + ml0) * 512;
        const double* B = q.emis + ((size_t)jb.ind * q.qcap + (qa - q.q0)) * 512;
        d2v ra[4], rb[4 * PLACE_NT];
        auto request = [&](int c) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = 4 * i + lr;
                ra[i] = d2v{0.0, 0.0};
                if (ml0 + row < len) ra[i] = __builtin_nontemporal_load((const d2v*)(A + (size_t)row * 512 + c * PLACE_KC + lc));
            }
#pragma unroll
            for (int i = 0; i < 4 * PLACE_NT; i++) {
                const int row = 4 * i + lr;
                rb[i] = d2v{0.0, 0.0};
                if (qa + row < qend) rb[i] = *(const d2v*)(B + (size_t)row * 512 + c * PLACE_KC + lc);
            }
        };
        d4v acc[PLACE_NT];
#pragma unroll
        for (int nt = 0; nt < PLACE_NT; nt++) acc[nt] = d4v{0.0, 0.0, 0.0, 0.0};
        request(0);
#pragma unroll 1
        for (int c = 0; c < 512 / PLACE_KC; c++) {
            wave_lds_fence();                   // the previous chunk's operand reads are done
#pragma unroll
            for (int i = 0; i < 4; i++) *(d2v*)(LA + (4 * i + lr) * PLACE_RS + lc) = ra[i];
#pragma unroll
            for (int i = 0; i < 4 * PLACE_NT; i++) *(d2v*)(LB + (4 * i + lr) * PLACE_RS + lc) = rb[i];
            wave_lds_fence();
            if (c + 1 < 512 / PLACE_KC) request(c + 1);
#pragma unroll
            for (int t = 0; t < PLACE_KC / 4; t++) {
                const double a = LA[oi * PLACE_RS + 4 * t + ok];
#pragma unroll
                for (int nt = 0; nt < PLACE_NT; nt++)
                    acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(LB[(nt * 16 + oi) * PLACE_RS + 4 * t + ok], a, acc[nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int nt = 0; nt < PLACE_NT; nt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int m = ml0 + oi, cand = qa + nt * 16 + ok + 4 * reg;
                if (m < len && cand < qend) {
                    const double v = acc[nt][reg];
                    double       r = (double)CNF2_MINFACTOR_F;       // the sum is exactly 0: impossible here
                    if (v > 0.0) {
                        r = v >= 2.2250738585072014e-308 ? log_pos(v) : log(v);
                        sum[nt][reg] += r;
                    } else nz[nt][reg]++;
                    if (q.place) q.place[((size_t)jb.ind * q.n_cand + cand) * p.n_markers + jb.first + m] = r;
                }
            }
    }
    flush();
}
void launch_place_rows(const PlaceParams& q, hipStream_t stream)
{
    const int m_block = CNF2_WAVES_PER_BLOCK * 16, q_block = 16 * PLACE_NT;
    const dim3 grid((q.n_jobs + q.group - 1) / q.group, (q.max_len + m_block - 1) / m_block, (q.qn + q_block - 1) / q_block);
    if (q.n_jobs > 0 && q.qn > 0) hipLaunchKernelGGL(place_rows_kernel, grid, dim3(CNF2_BLOCK), 0, stream, q);
}

int fb_fast_blocks_per_cu()
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fb_fast_kernel<true>, CNF2_BLOCK, 0) != hipSuccess) n = 2;
    return n < 1 ? 1 : n;
}
int fb_fast_uniform_blocks_per_cu()
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fb_fast_kernel<true, SW_PLAIN, false, false, true>, CNF2_BLOCK, 0) != hipSuccess) n = 2;
    return n < 1 ? 1 : n;
}

void launch_crossover_rows(const Stage2Params& q, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(crossover_rows_kernel, dim3(q.len), dim3(64), 0, stream, q, out);
}

void launch_loo_rows(const Stage2Params& q, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(loo_rows_kernel, dim3(q.len), dim3(64), 0, stream, q, out);
}

void launch_origin_rows(const Stage2Params& q, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(origin_rows_kernel, dim3(q.len), dim3(64), 0, stream, q, out);
}
void launch_descent_rows(const Stage2Params& q, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(descent_rows_kernel, dim3(q.len), dim3(64), 0, stream, q, out);
}

void launch_emission(const KernelParams& p, int ind, int marker, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(emission_kernel, dim3(1), dim3(64), 0, stream, p, ind, marker, out);
}

void launch_xor_selftest(double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(xor_selftest_kernel, dim3(1), dim3(64), 0, stream, out);
}

int fb_blocks_per_cu()
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fb_kernel<false>, CNF2_BLOCK, 0) != hipSuccess) n = 2;
    return n < 1 ? 1 : n;
}

// =====================================================================================
// Pair posteriors (cnf2_sweep_pairs): joint[i][p][4 u + v], the joint origin classes (u at marker j, v at marker k) of two
// selected markers j < k of one chromosome.  Per shift mode J_s(u, v) = sum_(g, g') [cls g = u] [cls g' = v] A_j(g)
// Phi(j -> k)(g, g') B_k(g'), Phi the product over the markers j+1 .. k of T diag(e); the modes are normalised each by its own
// total and weighted like the origin rows (origin_rows_kernel's rule).  A and B come from a turn-scan sweep's batch buffer.
// =====================================================================================
// Whether mode s of the window counts, and its weight exp(factors[s] - factor): 0 where it does not
__device__ __forceinline__ double pair_mode_weight(const Window& w, int s, double fs, double factor)
{
    const bool on = !(s & w.shiftignore) && s < w.shiftend && fs > (double)CNF2_MINFACTOR_F && !(factor - fs > 40.0) && !isnan(factor);
    return on ? exp(fs - factor) : 0.0;
}

// One wave per (job, anchor): the anchor is the a-th selected marker of the job's chromosome, a = 0 .. S - 2.  The sweep's lane
// layout (lane = mode x state_lo, register = state bits 3-5): class bit 0 is the lane's state bit 0, class bit 1 the register
// index's bit 0.  Alpha of the anchor is split by class into four vectors; they walk to the chromosome's last selected marker
// through the transition (`transition_scaled`) and the marker's emission (formed once, as emission_kernel forms it) with one
// rescale per mode common to the four, which J_s / Z_s does not see.  At a selected marker the sixteen masked sums against beta: a lane's eight
// partials (u, register parity) are reduced by halving -- over state bit 1, then state bit 2, a lane keeping half of its
// values per step -- so that the chain's eight lanes end with two sums each; after the mode's normalisation and weight one
// more halving step and two plain ones add up the modes, and lanes 0-15 store the row: one 128-byte line.
__global__ __launch_bounds__(CNF2_BLOCK, 2) void pair_sweep_kernel(PairParams q)
{
    __shared__ double tabs[CNF2_WAVES_PER_BLOCK][64];
    const int lane = threadIdx.x & 63;
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int job  = blockIdx.x;
    const KernelParams& p = q.kp;
    const Job jb = p.jobs[job];
    const int sb = q.chrom_sel[jb.chrom], se = q.chrom_sel[jb.chrom + 1];
    const int a  = blockIdx.y * CNF2_WAVES_PER_BLOCK + wib;
    if (a >= se - sb - 1) return;                       // (also a chromosome with fewer than two selected markers)
    const int ja = sb + a;
    double*   tab = tabs[wib];
    const Window w = p.windows[jb.ind];
    LaneCtx   c;
    make_lane(w, lane, &c.L);
    c.row_root   = w.row[0];
    c.root_attop = (w.flags[0] & SLOT_FOUNDER) != 0;
    const int s  = lane >> 3;
    c.s0 = s & 1;
    c.s1 = (s >> 1) & 1;
    c.s2 = (s >> 2) & 1;
    c.lo = state_lo(lane);
    c.active  = true;
    c.n_combo = 1;
    const size_t e_ic = (size_t)jb.ind * p.n_chrom + jb.chrom;
    const double ws   = pair_mode_weight(w, s, p.factors[e_ic * 8 + s], p.loglik[e_ic]);
    const bool   on   = ws != 0.0;
    const bool   b0 = (c.lo & 1) != 0, kA = (c.lo & 2) != 0, kB = (c.lo & 4) != 0, kC = (lane & 8) != 0;
    const int    ma = q.sel[ja], mlast = q.sel[se - 1];
    const double* wrow = p.wbuf + (size_t)job * p.wstride * CNF2_TURN_ROW;

    double V[4][8];
    {
        const double* wp = wrow + (size_t)(ma - jb.first) * CNF2_TURN_ROW;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const d2v t = *(const d2v*)(wp + k * 128 + lane * 2);
            const double x0 = on ? t.x : 0.0, x1 = on ? t.y : 0.0;      // (a chain that is off: 0, whatever the buffer holds)
            // register 2k has class bit 1 clear, register 2k + 1 has it set
            V[0][2 * k] = b0 ? 0.0 : x0;
            V[1][2 * k] = b0 ? x0 : 0.0;
            V[2][2 * k] = V[3][2 * k] = 0.0;
            V[0][2 * k + 1] = V[1][2 * k + 1] = 0.0;
            V[2][2 * k + 1] = b0 ? 0.0 : x1;
            V[3][2 * k + 1] = b0 ? x1 : 0.0;
        }
    }
    int kn = ja + 1;
    int mk = q.sel[kn];
#pragma unroll 1
    for (int m = ma + 1; m <= mlast; m++) {
        // the scaled butterflies of the fast sweep (x' = x + t partner, t = r / (1 - r)): the constant they drop is common to
        // the four vectors and to every mode, and J_s / Z_s does not see it; a gap of rate 0 has t = 0, the identity to the bit
        const double2 tq = p.tq[m - 1];
#pragma unroll
        for (int u = 0; u < 4; u++) transition_scaled(V[u], tq.x, tq.y);
        const Slot root = load_slot(p, c.row_root, m);
        LineTerms  T;
        wave_lds_fence();                               // the previous marker's reads are done
        tab[lane] = produce_entry(p, c, root, m, &T);
        wave_lds_fence();
        double c0, c1, e[8], t[8];
        root_weights(c, root, &c0, &c1);
        emission_from_table(tab, c, c0, c1, e);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            e[j] = on ? e[j] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; u++) V[u][j] *= e[j];
            t[j] = (V[0][j] + V[1][j]) + (V[2][j] + V[3][j]);
        }
        const double sum = chain_total<false>(t);
        const double inv = fast_rcp(sum > 0.0 ? sum : 1.0);
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int j = 0; j < 8; j++) V[u][j] *= inv;
        if (m != mk) continue;
        // a selected marker: the sixteen sums against beta
        const double* wp = wrow + (size_t)(m - jb.first) * CNF2_TURN_ROW + 512;
        double h[8];                                     // [u][parity of the register = class bit 1 of v]
        {
            d2v bq[4];
#pragma unroll
            for (int k = 0; k < 4; k++) bq[k] = *(const d2v*)(wp + k * 128 + lane * 2);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                h[2 * u]     = (V[u][0] * bq[0].x + V[u][2] * bq[1].x) + (V[u][4] * bq[2].x + V[u][6] * bq[3].x);
                h[2 * u + 1] = (V[u][1] * bq[0].y + V[u][3] * bq[1].y) + (V[u][5] * bq[2].y + V[u][7] * bq[3].y);
            }
        }
        // halving: the partner over state bit 1 has the same class bit and the other kA: it keeps the other u >> 1 ...
        double h4[4], h2[2];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double lo = h[i], hi = h[4 + i];
            h4[i] = (kA ? hi : lo) + lane_flip_b1(kA ? lo : hi);
        }
        // ... the partner over state bit 2 has the same class bit, the same kA and the other kB: it keeps the other u & 1
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const double lo = h4[i], hi = h4[2 + i];
            h2[i] = (kB ? hi : lo) + lane_flip_b2(kB ? lo : hi);
        }
        // this lane: J_s(u, v) of u = 2 kA + kB, v = b0 + 2 i
        const double x0 = on ? h2[0] : 0.0, x1 = on ? h2[1] : 0.0;
        const double Z  = chain_sum(x0 + x1);
        const bool   ok = on && Z > 0.0;
        const double f  = ok ? ws / Z : 0.0;
        const double wsum = across_chains_sum(ok ? ws : 0.0);
        const double y0 = x0 * f, y1 = x1 * f;
        double y = (kC ? y1 : y0) + lane_xor8(kC ? y0 : y1);
        y += lane_xor16(y);
        y += lane_xor32(y);
        if (lane < 16) {
            const int u = (kA ? 2 : 0) | (kB ? 1 : 0), v = (b0 ? 1 : 0) | (kC ? 2 : 0);
            double*   row = q.joint + ((size_t)jb.ind * q.n_pairs + q.pair_off[ja] + (kn - ja - 1)) * 16;
            row[4 * u + v] = wsum > 0.0 ? y / wsum : 0.0;
        }
        kn++;
        mk = kn < se ? q.sel[kn] : -1;
    }
}
void launch_pair_sweep(const PairParams& q, hipStream_t stream)
{
    if (q.n_jobs <= 0 || q.max_anchors <= 0) return;
    dim3 grid(q.n_jobs, (q.max_anchors + CNF2_WAVES_PER_BLOCK - 1) / CNF2_WAVES_PER_BLOCK);
    hipLaunchKernelGGL(pair_sweep_kernel, grid, dim3(CNF2_BLOCK), 0, stream, q);
}

// cnt[c] = the individuals of [0, n_ind) with a mode that has a likelihood on chromosome c (those a pair sweep writes rows
// for), counted in one thread per chromosome
__global__ __launch_bounds__(64) void pair_count_kernel(const double* factors, const double* loglik, int n_ind, int n_chrom, int32_t* cnt)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chrom) return;
    int k = 0;
    for (int i = 0; i < n_ind; i++) {
        const size_t e = (size_t)i * n_chrom + c;
        bool any = false;
        for (int s = 0; s < 8; s++) any = any || factors[e * 8 + s] > (double)CNF2_MINFACTOR_F;
        k += (any && !isnan(loglik[e])) ? 1 : 0;
    }
    cnt[c] = k;
}
void launch_pair_count(const double* factors, const double* loglik, int n_ind, int n_chrom, int32_t* cnt, hipStream_t stream)
{
    if (n_chrom > 0)
        hipLaunchKernelGGL(pair_count_kernel, dim3((n_chrom + 63) / 64), dim3(64), 0, stream, factors, loglik, n_ind, n_chrom, cnt);
}

// The pair rows from the store, brute force (the cross-check of the pair sweep): one block per anchor a = 0 .. S - 2 among the
// S selected markers of the chromosome (sel: their local indices, ascending), thread g.  Every mode's four class-restricted
// vectors are carried in LDS from marker to marker with the explicit 64 x 64 transition and the emission of all 8 modes
// through the sweep's producer / consumer code (as crossover_rows_kernel), rescaled per mode by their common total.
// out[S (S - 1) / 2][16]: the pairs in ascending anchor, then ascending target; zeros where no mode has a likelihood.
__global__ __launch_bounds__(64) void pair_rows_kernel(Stage2Params q, const int32_t* sel, int S, double* out)
{
    __shared__ double tab[64];
    __shared__ double E[8][64];
    __shared__ double V[8][4][64];
    const int    g  = threadIdx.x;
    const int    a  = blockIdx.x;
    const Window w  = q.kp.windows[0];
    const double factor = q.loglik[0];
    const int    cls = (g & 1) | ((g >> 2) & 2);
    double ws[8];
    for (int s = 0; s < 8; s++) {
        ws[s] = pair_mode_weight(w, s, q.factors[s], factor);
        for (int u = 0; u < 4; u++) V[s][u][g] = (ws[s] != 0.0 && cls == u) ? s2_fw(q, s, sel[a], 2, g) : 0.0;
    }
    LaneCtx c;
    make_lane(w, g, &c.L);
    c.row_root   = w.row[0];
    c.root_attop = (w.flags[0] & SLOT_FOUNDER) != 0;
    const int sl = g >> 3;
    c.s0 = sl & 1;
    c.s1 = (sl >> 1) & 1;
    c.s2 = (sl >> 2) & 1;
    c.lo = state_lo(g);
    c.active  = true;
    c.n_combo = 1;
    size_t pair = (size_t)a * (2 * S - a - 1) / 2;
    int    kn = a + 1;
    __syncthreads();
    for (int ml = sel[a] + 1; ml <= sel[S - 1]; ml++) {
        const int m = q.first + ml;
        const Slot root = load_slot(q.kp, c.row_root, m);
        LineTerms  T;
        tab[g] = produce_entry(q.kp, c, root, m, &T);
        __syncthreads();
        double c0, c1, e[8];
        root_weights(c, root, &c0, &c1);
        emission_from_table(tab, c, c0, c1, e);
        // e of mode sl, state j * 8 + lo sits in this lane's register j
#pragma unroll
        for (int j = 0; j < 8; j++) E[sl][j * 8 + c.lo] = e[j];
        __syncthreads();
        const double2 r = q.kp.rho[m - 1];
        const double rt[6] = {r.y, r.x, r.x, r.y, r.x, r.x};
        double acc[8][4];
        for (int s = 0; s < 8; s++)
            for (int u = 0; u < 4; u++) acc[s][u] = 0.0;
        for (int g2 = 0; g2 < 64; g2++) {
            const int d = g ^ g2;
            double    tr = 1.0;
#pragma unroll
            for (int t = 0; t < 6; t++) tr *= ((d >> t) & 1) ? rt[t] : 1.0 - rt[t];
            for (int s = 0; s < 8; s++)
                for (int u = 0; u < 4; u++) acc[s][u] += V[s][u][g2] * tr;
        }
        __syncthreads();
        for (int s = 0; s < 8; s++) {
            const double eg = ws[s] != 0.0 ? E[s][g] : 0.0;
            double       mine = 0.0;
            for (int u = 0; u < 4; u++) {
                acc[s][u] *= eg;
                mine += acc[s][u];
            }
            const double tot = across_chains_sum(chain_sum(mine));
            const double inv = tot > 0.0 ? 1.0 / tot : 1.0;
            for (int u = 0; u < 4; u++) V[s][u][g] = acc[s][u] * inv;
        }
        __syncthreads();
        if (ml != sel[kn]) continue;
        double row[16], wsum = 0.0;
        for (int k = 0; k < 16; k++) row[k] = 0.0;
        for (int s = 0; s < 8; s++) {
            if (ws[s] == 0.0) continue;
            const double b = s2_fw(q, s, ml, 1, g);
            double J[16], Z = 0.0;
            for (int u = 0; u < 4; u++)
                for (int v = 0; v < 4; v++) {
                    J[4 * u + v] = across_chains_sum(chain_sum(cls == v ? V[s][u][g] * b : 0.0));
                    Z += J[4 * u + v];
                }
            if (!(Z > 0.0)) continue;
            for (int k = 0; k < 16; k++) row[k] += ws[s] * (J[k] / Z);
            wsum += ws[s];
        }
        if (g < 16) out[(pair + (size_t)(kn - a - 1)) * 16 + g] = wsum > 0.0 ? row[g] / wsum : 0.0;
        kn++;
        if (kn >= S) break;
    }
}
void launch_pair_rows(const Stage2Params& q, const int32_t* sel, int S, double* out, hipStream_t stream)
{
    if (S >= 2) hipLaunchKernelGGL(pair_rows_kernel, dim3(S - 1), dim3(64), 0, stream, q, sel, S, out);
}

} // namespace cnf2
