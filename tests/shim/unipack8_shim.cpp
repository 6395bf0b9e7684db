// C interface for tests/test_uniform_pack8_host.py: the lane helpers of the eight-windows-to-a-wave sweep (cnf2_lane.h up8_*) and
// the pairing of the groups of four (cnf2_plan.h pair_uniform_groups).  Host code only.
#include <cstring>
#include <vector>

#include "cnf2_lane.h"
#include "cnf2_plan.h"

using namespace cnf2;

extern "C" {

int up8_shim_state_lo(int lane) { return state_lo(lane); }
int up8_shim_job(int lane) { return up8_job(lane); }
int up8_shim_s0(int lane) { return up8_s0(lane); }
int up8_shim_s2(int lane) { return up8_s2(lane); }
int up8_shim_b0(int lane) { return up8_b0(lane); }
int up8_shim_virtual_lane(int lane, int s1, int v) { return up8_virtual_lane(lane, s1, v); }
int up8_shim_park(int cls, int vl) { return up8_park(cls, vl); }
int up8_shim_spill_writer(int lane) { return up8_spill_writer(lane) ? 1 : 0; }
int up8_shim_spill_value(int lane) { return up8_spill_value(lane); }
int up8_shim_spill_emit(int lane) { return up8_spill_emit(lane); }
int up8_shim_spill_inv(int job, int s0) { return up8_spill_inv(job, s0); }
int up8_shim_spill_row() { return UP8_SPILL_ROW; }
int up8_shim_plan_spill_row() { return (int)PLAN_SPILL_ROW; }
int up8_shim_sizeof_window() { return (int)sizeof(Window); }

// groups [n_groups][8] (ind[4], first, last, chrom, homleaf) in and out; windows [..] of 64 bytes, indexed by ind; waves: the
// resident waves of the packed grid (0 = no whole-rounds rule).  Returns the number of eights.
int up8_shim_pair(int32_t* groups, int n_groups, const void* windows, int waves)
{
    static_assert(sizeof(PackedJob) == 8 * sizeof(int32_t), "a group is eight ints");
    std::vector<PackedJob> g(n_groups);
    if (n_groups > 0) std::memcpy(g.data(), groups, sizeof(PackedJob) * (size_t)n_groups);
    const size_t n8 = pair_uniform_groups(g, (const Window*)windows, (size_t)waves);
    if ((int)g.size() != n_groups) return -1;
    if (n_groups > 0) std::memcpy(groups, g.data(), sizeof(PackedJob) * (size_t)n_groups);
    return (int)n8;
}
}
