// cnf2_lane.h -- mapping of the 64 emission-table entries of one (individual, marker) onto
// the 64 lanes of a wavefront, shared by the HIP kernels and the host unit-test shim.
//   lane = P<<5 | f<<4 | sp<<3 | k
//     P  parent side (0: state bits 0-2, 1: state bits 3-5)
//     f  root allele index handed to parent 0 (the other one goes to parent 1)
//     sp shift bit of that parent (shift bit 1 for P=0, bit 2 for P=1; cnF2freq.cpp:986)
//     k  the parent's 3 state bits: bit0 = which grandparent is traced, bits 1-2 the
//        grandparents' own bits (upflagit, cnF2freq.cpp:321-329,984)
#ifndef CNF2_LANE_H
#define CNF2_LANE_H

#include "cnf2_emission.h"
#include "cnf2_window.h"

namespace cnf2 {

struct LaneJob {
    LineCfg cfg;
    int32_t row_par, row_tr, row_ot;   // genotype rows (blank row 0 when the slot is missing)
    int8_t  tie_par, tie_tr, tie_ot;   // tie group per slot or -1
    int     P, f;
};

CNF2_HD void make_lane(const Window& w, int lane, LaneJob* L)
{
    const int P = lane >> 5, f = (lane >> 4) & 1, sp = (lane >> 3) & 1, k = lane & 7;
    const int firstpar = k & 1, upflag = k >> 1;
    const int slot_par = 1 + 3 * P;
    const int slot_tr  = slot_par + 1 + firstpar;
    const int slot_ot  = slot_par + 1 + (firstpar ^ 1);
    L->P = P;
    L->f = f;
    L->cfg.par      = w.flags[slot_par];
    L->cfg.tr       = w.flags[slot_tr];
    L->cfg.ot       = w.flags[slot_ot];
    L->cfg.firstpar = firstpar;
    L->cfg.bit_tr   = (upflag >> firstpar) & 1;
    L->cfg.bit_ot   = (upflag >> (firstpar ^ 1)) & 1;
    L->cfg.sp       = sp;
    L->row_par = w.row[slot_par] < 0 ? 0 : w.row[slot_par];
    L->row_tr  = w.row[slot_tr] < 0 ? 0 : w.row[slot_tr];
    L->row_ot  = w.row[slot_ot] < 0 ? 0 : w.row[slot_ot];
    L->tie_par = w.tie[slot_par];
    L->tie_tr  = w.tie[slot_tr];
    L->tie_ot  = w.tie[slot_ot];
}

// The fast kernels' lane order within a chain of 8 lanes: the low state bits (b0, b1, b2) sit in lane b0 ^ 2 b1 ^ 7 b2
// (flipping b2 is then a row_half_mirror move, see cnf2_kernels.hip).  The map is its own inverse.
CNF2_HD constexpr int state_lo(int lane) { return (lane & 7) ^ ((lane & 4) ? 3 : 0); }

// Spill row of the uniform-state sweep with two registers per lane.  Alpha does not depend on state bits 1, 2, 4, 5 there, so
// the 8 lanes of a chain hold two distinct register pairs, told apart by state bit 0: a row keeps each once.
//   [chain 0..7][b0][2] = 32 doubles of values (registers 0, 1 of the lanes with state bit 0 = b0), then
//   [chain][2]          = 16 doubles: reciprocal normaliser of the (even) marker and of an odd last marker
// = 48 doubles, three lines of 128 bytes.  The lanes with state bits 1 and 2 clear (lanes 0 and 1 of a chain) write, one
// 16-byte store each, 256 contiguous bytes a wave; every lane reads the 16 bytes of its class, four lanes an address.
enum { UNI_SPILL_INV = 32, UNI_SPILL_ROW = 48 };
CNF2_HD bool uni_spill_writer(int lane) { return (state_lo(lane) & 6) == 0; }
// offset (doubles) of the lane's register pair in the row: where a writer stores and where every lane loads
CNF2_HD int uni_spill_value(int lane) { return (lane >> 3) * 4 + (state_lo(lane) & 1) * 2; }
// offset (doubles) of a chain's two reciprocals
CNF2_HD int uni_spill_inv(int chain) { return UNI_SPILL_INV + 2 * chain; }

// Four uniform windows to a wave (fb_unipack_kernel).  The four lanes of a chain that differ only in state bits 1 and 2 run the
// uniform recursion on the same numbers, so each of them carries another job: a lane's job is those two bits, its class state
// bit 0, its chain lane >> 3 as ever.  For the rows a lane stands for the four lanes of its job's own sweep that share its chain
// and class: virtual lane v = 0..3 has state bits 1 and 2 = v (the lane number under state_lo, which is its own inverse).
CNF2_HD int upk_job(int lane) { return (state_lo(lane) >> 1) & 3; }
CNF2_HD int upk_virtual_lane(int lane, int v) { return (lane & ~7) | state_lo((state_lo(lane) & 1) | (v << 1)); }
// Spill row of that kernel: the four jobs' compact rows side by side.
//   [lane 0..63][2]     = 128 doubles of values: every lane stores and loads its own register pair, one 16-byte access each
//   [job][chain][2]     = 64 doubles: the reciprocal normalisers of UNI_SPILL_INV, per job
// = 192 doubles, four times UNI_SPILL_ROW.
enum { UPK_SPILL_INV = 128, UPK_SPILL_ROW = 192 };
CNF2_HD int upk_spill_value(int lane) { return 2 * lane; }
CNF2_HD int upk_spill_inv(int job, int chain) { return UPK_SPILL_INV + 2 * (8 * job + chain); }

// Eight uniform windows to a wave (fb_unipack8_kernel), for windows with all eight shift modes analysed.  The unrestricted table
// of a window on line records does not depend on a parent's shift bit, so the chains of a job with equal s0 run the recursion
// on the same numbers as well: the lanes that differ in s1 carry another job, too.  A lane is (job 0..7, s0, s2, b0):
//   lane = job_hi << 5 | s2 << 4 | s0 << 3 | l,  state_lo(l) = b0 | job_lo << 1     (lane ^ 1 flips b0, as the recursion needs it)
// For the rows a lane forms the B-side class sums of (s0, s2) once and then stands for the eight lanes (s1, v) of the job's own
// sweep with its s0, s2 and class: virtual lane (s1, v) is lane s * 8 + state_lo(b0 | v << 1) of chain s = s0 | s1 << 1 | s2 << 2.
CNF2_HD int up8_job(int lane) { return ((lane >> 3) & 4) | ((state_lo(lane) >> 1) & 3); }
CNF2_HD int up8_s0(int lane) { return (lane >> 3) & 1; }
CNF2_HD int up8_s2(int lane) { return (lane >> 4) & 1; }
CNF2_HD int up8_b0(int lane) { return state_lo(lane) & 1; }
CNF2_HD int up8_virtual_lane(int lane, int s1, int v)
{
    return (up8_s0(lane) | (s1 << 1) | (up8_s2(lane) << 2)) * 8 + state_lo(up8_b0(lane) | (v << 1));
}
// Row sums in registers (CNF2_UP8_ROW_SUMS, the default).  A partial depends on the lane's class only through the B-side class
// sums, and the two lanes of a b0 pair (lane, lane ^ 1) between them form the eight partials of chain (s0, s1 = 1, s2) and the
// eight of chain (s0, s1 = 0, s2).  So the pair exchanges its class sums and each lane adds up one whole chain: lane `lane`
// forms the virtual lanes s * 8 + 0..7 of chain s = s0 | up8_sum_s1(lane) << 1 | s2 in ascending place, place i2 being the
// partial (b, v) = (up8_place_b(i2), up8_place_v(i2)) with the class sums of class b: the one-job sweep's order inside a chain.
// The chains of a job are then added as chain_sum adds them, ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)): level 0 pairs
// s0, level 1 s1, level 2 s2, every level between two lanes that both hold what they add (up8_partner), so all eight lanes of a
// job end with the job's sum.  The A-side entries of a chain are the eight doubles from up8_sum_run(f, s1) on in the restricted
// totals and in the class-2 parts: 16-byte aligned runs.
CNF2_HD int up8_sum_s1(int lane) { return up8_b0(lane); }
CNF2_HD constexpr int up8_place_b(int i2) { return state_lo(i2) & 1; }
CNF2_HD constexpr int up8_place_v(int i2) { return state_lo(i2) >> 1; }
CNF2_HD constexpr int up8_partner(int lane, int level) { return lane ^ (level == 0 ? 8 : (level == 1 ? 1 : 16)); }
CNF2_HD int up8_sum_run(int f, int s1) { return (f << 4) | (s1 << 3); }
// The parked form (CNF2_UP8_ROW_SUMS == 0, kept for A/B timing): a lane forms the partials (s1, v) of its own class for both s1
// and parks them in the row for the lanes of a tile epilogue.
// Where the partial of class cls (0..2) of virtual lane vl is parked in the job's table row (TAB_STRIDE doubles: [0,64) the
// unrestricted table, [64,72) root weights and gap, [72,136) restricted totals, [136,200) class-2 parts; the A side is the
// lower half of a table).  The partials of s1 = 1 are parked first, while the A-side entries of s1 = 0 are still to be
// read: they go over the unrestricted table and the B side of the restricted totals; those of s1 = 0 then go over the rest.
// The tile epilogue reads chain s of class cls at up8_park(cls, s * 8) + 0..7, in the order it adds them in a one-job sweep.
CNF2_HD int up8_park(int cls, int vl)
{
    const int s = vl >> 3, s1 = (s >> 1) & 1, i4 = (s & 1) | ((s >> 2) << 1);
    const int base = s1 ? (cls == 0 ? 0 : (cls == 1 ? 32 : 104)) : (cls == 0 ? 72 : (cls == 1 ? 136 : 168));
    return base + i4 * 8 + (vl & 7);
}
// Spill row of that kernel, per marker pair.  What a lane carries does not depend on s2: the lanes with s2 = 0 store, every lane
// loads by its class w = job_hi << 4 | s0 << 3 | l.
//   [w 0..31][2]        = 64 doubles: alpha in front of the even marker
//   [w 0..31][2]        = 64 doubles: that alpha times the even marker's emission (what the odd marker's rebuild starts from)
//   [job][s0][2]        = 32 doubles: the reciprocal normalisers of the even marker and of an odd last marker
// = 160 doubles, ten lines of 128 bytes.
enum { UP8_SPILL_EMIT = 64, UP8_SPILL_INV = 128, UP8_SPILL_ROW = 160 };
CNF2_HD bool up8_spill_writer(int lane) { return up8_s2(lane) == 0; }
CNF2_HD int up8_spill_value(int lane) { return 2 * (((lane >> 5) << 4) | (lane & 15)); }
CNF2_HD int up8_spill_emit(int lane) { return UP8_SPILL_EMIT + up8_spill_value(lane); }
CNF2_HD int up8_spill_inv(int job, int s0) { return UP8_SPILL_INV + 2 * (2 * job + s0); }

// Forward tile of that kernel: the forward step of (marker, job) needs 14 doubles -- one value per part (on line records the
// unrestricted table is one value a part), the root weights c_f(s0) and the gap's two butterfly factors -- and takes them from
// a compact slot instead of a table row.  A tile is T markers x 8 jobs; a slot is 14 values padded to UP8_FWD_SLOT = 16, kept
// job-minor: value i of (t, job) sits at (t * 16 + i) * 8 + job, so that the 64 producer lanes (part, job) of a marker store 64
// consecutive doubles and the recursion lanes of the eight jobs read eight consecutive ones (no bank is asked twice).
//   i = 0..7  part (P << 2 | f << 1 | firstpar);  8 + 2 f + s0  root weight c_f(s0);  12, 13  the gap's factors;  14, 15  unused
// The wave's region (8 table rows) holds two tiles where 2 T x 128 doubles fit: a tile is produced into the buffer the previous
// one was not read from, and one fence a tile orders it all (up8_fwd_buffers, up8_fwd_tile).
enum { UP8_FWD_SLOT = 16, UP8_FWD_VALUES = 14, UP8_FWD_MARKER = 8 * UP8_FWD_SLOT };
CNF2_HD constexpr int up8_fwd_buffers(int T, int region) { return 2 * T * UP8_FWD_MARKER <= region ? 2 : 1; }
// first double of tile number `tile` (its buffer) in the wave's region
CNF2_HD constexpr int up8_fwd_tile(int T, int region, int tile) { return up8_fwd_buffers(T, region) == 2 ? (tile & 1) * T * UP8_FWD_MARKER : 0; }
// value i of (marker t of the tile, job), from the tile's first double
CNF2_HD constexpr int up8_fwd_at(int t, int job, int i) { return (t * UP8_FWD_SLOT + i) * 8 + job; }
CNF2_HD constexpr int up8_fwd_part(int part) { return part; }
CNF2_HD constexpr int up8_fwd_weight(int f, int s0) { return 8 + 2 * f + s0; }
CNF2_HD constexpr int up8_fwd_gap(int k) { return 12 + k; }

// Root staging of that kernel (CNF2_UP8_ROOT_STAGE): the eight producer lanes (part, job) of a marker all need the root's
// sure (two doubles), hw and allele byte of (marker, job), and eight consecutive markers share a line of each array.  So once a
// tile of UP8_STAGE_T = 8 markers lane (t = lane >> 3, job = lane & 7) loads them for (marker t of the tile, job) and stores them
// in the wave's LDS region, where the producer lanes read them, eight lanes an address.  Two buffers: tile k sits in buffer k & 1.
//   forward:  behind the forward tiles; entry (t, job) is UP8_STAGE_ENTRY = 4 doubles: sure, hw, the allele byte (a 32-bit word)
//   backward: the rows fill the region, but of a row's 64 unrestricted entries the packed producer stores and the eights read
//             only 8 k + 0, 1 (cnf2_emtab.h packed_reads_unrestricted): the six doubles behind them hold marker t = k of the
//             job's two buffers (sure 16-byte aligned in both), and the tile's eight allele bytes are the bytes of one double
//             a buffer, behind the gap's factors (doubles 70, 71 of the row, which nobody else uses)
enum { UP8_STAGE_T = 8, UP8_STAGE_ENTRY = 4, UP8_STAGE_BUFFER = UP8_STAGE_T * 8 * UP8_STAGE_ENTRY };
// doubles of the region the forward tiles of T markers leave for staging
CNF2_HD constexpr int up8_stage_fwd_room(int T, int region) { return region - up8_fwd_buffers(T, region) * T * UP8_FWD_MARKER; }
// first double of entry (t, job) of buffer buf in the wave's region, forward
CNF2_HD constexpr int up8_stage_fwd_at(int T, int region, int buf, int t, int job)
{
    return up8_fwd_buffers(T, region) * T * UP8_FWD_MARKER + buf * UP8_STAGE_BUFFER + (t * 8 + job) * UP8_STAGE_ENTRY;
}
enum { UP8_STAGE_SURE = 0, UP8_STAGE_HW = 2, UP8_STAGE_ALLELE = 3 };       // doubles from an entry's first, forward
// backward, in the job's table row: double of sure (two) and of hw of (buffer, marker t), and the double of a buffer's allele bytes
CNF2_HD constexpr int up8_stage_bwd_sure(int buf, int t) { return 8 * t + (buf ? 6 : 2); }
CNF2_HD constexpr int up8_stage_bwd_hw(int buf, int t) { return 8 * t + (buf ? 5 : 4); }
CNF2_HD constexpr int up8_stage_bwd_alleles(int buf) { return 70 + buf; }

CNF2_HD int tie_force(int8_t tie, int combo)
{
    return tie < 0 ? -1 : ((combo >> tie) & 1);
}

CNF2_HD Slot unpack_slot(uint8_t allele_pair, double s0, double s1, double hw)
{
    Slot d;
    d.a0 = allele_pair & 15;
    d.a1 = allele_pair >> 4;
    d.s0 = s0;
    d.s1 = s1;
    d.hw = hw;
    return d;
}

} // namespace cnf2
#endif
