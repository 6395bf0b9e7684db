// C interface for tests/test_uniform_pack8_fwd_host.py: the layout of the eights' forward tiles (cnf2_lane.h up8_fwd_*), the
// lane helpers they are read with, and which unrestricted entries the packed kernels' producer stores (cnf2_emtab.h).  Host
// code only.
#include "cnf2_lane.h"
// (behind cnf2_lane.h: it wants Window)
#include "cnf2_emtab.h"

using namespace cnf2;

extern "C" {

int up8f_shim_state_lo(int lane) { return state_lo(lane); }
int up8f_shim_job(int lane) { return up8_job(lane); }
int up8f_shim_s0(int lane) { return up8_s0(lane); }
int up8f_shim_s2(int lane) { return up8_s2(lane); }
int up8f_shim_b0(int lane) { return up8_b0(lane); }
int up8f_shim_slot() { return UP8_FWD_SLOT; }
int up8f_shim_values() { return UP8_FWD_VALUES; }
int up8f_shim_marker() { return UP8_FWD_MARKER; }
int up8f_shim_buffers(int T, int region) { return up8_fwd_buffers(T, region); }
int up8f_shim_tile(int T, int region, int tile) { return up8_fwd_tile(T, region, tile); }
int up8f_shim_at(int t, int job, int i) { return up8_fwd_at(t, job, i); }
int up8f_shim_part(int part) { return up8_fwd_part(part); }
int up8f_shim_weight(int f, int s0) { return up8_fwd_weight(f, s0); }
int up8f_shim_gap(int k) { return up8_fwd_gap(k); }
int up8f_shim_part_entry_index(int part, int e) { return part_entry_index(part, e); }
int up8f_shim_packed_reads_unrestricted(int e) { return packed_reads_unrestricted(e) ? 1 : 0; }

// what emtab_part_rec hands to `out` for the unrestricted table: bit e of the result, for the packed form or the full one
int up8f_shim_entries_stored(int packed)
{
    Slot root;
    root.a0 = 1;
    root.a1 = 2;
    root.s0 = 0.01;
    root.s1 = 0.02;
    root.hw = 0.5;
    LineRec r;
    r.Bp = 0.9, r.Cp = 0.05, r.Kp = 0.05, r.t0 = 0.8, r.t1 = 0.2, r.oo = 0.7;
    r.bits = LR_LIVE | 0xffffu;
    r.pad[0] = r.pad[1] = r.pad[2] = 0;
    int    seen = 0;
    double cw[2];
    auto   out = [&](int kind, int e, double) {
        if (kind == 0) seen |= 1 << e;
    };
    if (packed) emtab_part_rec<false, true>(0, 0, root, r, out, cw);
    else emtab_part_rec<false, false>(0, 0, root, r, out, cw);
    return seen;
}
}
