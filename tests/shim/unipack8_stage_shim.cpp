// C interface for tests/test_uniform_pack8_stage_host.py: where the eights stage the root's data of a tile in the wave's LDS
// region (cnf2_lane.h up8_stage_*), beside the forward tiles' layout and the entries the packed producer stores.  Host code only.
#include "cnf2_lane.h"
// (behind cnf2_lane.h: it wants Window)
#include "cnf2_emtab.h"

using namespace cnf2;

extern "C" {

int up8s_shim_tile() { return UP8_STAGE_T; }
int up8s_shim_entry() { return UP8_STAGE_ENTRY; }
int up8s_shim_buffer() { return UP8_STAGE_BUFFER; }
int up8s_shim_sure() { return UP8_STAGE_SURE; }
int up8s_shim_hw() { return UP8_STAGE_HW; }
int up8s_shim_allele() { return UP8_STAGE_ALLELE; }
int up8s_shim_fwd_room(int T, int region) { return up8_stage_fwd_room(T, region); }
int up8s_shim_fwd_at(int T, int region, int buf, int t, int job) { return up8_stage_fwd_at(T, region, buf, t, job); }
int up8s_shim_fwd_buffers(int T, int region) { return up8_fwd_buffers(T, region); }
int up8s_shim_fwd_marker() { return UP8_FWD_MARKER; }
int up8s_shim_bwd_sure(int buf, int t) { return up8_stage_bwd_sure(buf, t); }
int up8s_shim_bwd_hw(int buf, int t) { return up8_stage_bwd_hw(buf, t); }
int up8s_shim_bwd_alleles(int buf) { return up8_stage_bwd_alleles(buf); }
int up8s_shim_part_entry_index(int part, int e) { return part_entry_index(part, e); }
int up8s_shim_packed_reads_unrestricted(int e) { return packed_reads_unrestricted(e) ? 1 : 0; }
}
