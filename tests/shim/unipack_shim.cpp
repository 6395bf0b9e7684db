// C interface for tests/test_uniform_pack_host.py: the lane helpers of the four-windows-to-a-wave sweep (cnf2_lane.h) and the
// grouping of its jobs (cnf2_plan.h group_uniform_jobs).  Host code only.
#include <cstring>
#include <vector>

#include "cnf2_lane.h"
#include "cnf2_plan.h"

using namespace cnf2;

extern "C" {

int upk_shim_state_lo(int lane) { return state_lo(lane); }
int upk_shim_job(int lane) { return upk_job(lane); }
int upk_shim_virtual_lane(int lane, int v) { return upk_virtual_lane(lane, v); }
int upk_shim_spill_value(int lane) { return upk_spill_value(lane); }
int upk_shim_spill_inv(int job, int chain) { return upk_spill_inv(job, chain); }
int upk_shim_spill_row() { return UPK_SPILL_ROW; }
int upk_shim_sizeof_window() { return (int)sizeof(Window); }

// jobs [n_jobs][4] (ind, first, last, chrom) in and out, the first n_fast of them the fast jobs; windows [..] of 64 bytes, indexed
// by ind; line_keys [..][2] or NULL.  groups_out [n_fast / 4][8] (ind[4], first, last, chrom, homleaf).  Returns the groups' number.
int upk_shim_group(int32_t* jobs, int n_jobs, int n_fast, const void* windows, const int32_t* line_keys, int32_t* groups_out,
                   int32_t* n_single_out)
{
    std::vector<Job> v(n_jobs);
    std::memcpy(v.data(), jobs, sizeof(Job) * (size_t)n_jobs);
    size_t                       n_single = 0;
    const std::vector<PackedJob> g = group_uniform_jobs(v, (size_t)n_fast, (const Window*)windows, line_keys, &n_single);
    std::memcpy(jobs, v.data(), sizeof(Job) * (size_t)n_jobs);
    static_assert(sizeof(PackedJob) == 8 * sizeof(int32_t), "a group is eight ints");
    if (!g.empty()) std::memcpy(groups_out, g.data(), sizeof(PackedJob) * g.size());
    *n_single_out = (int32_t)n_single;
    return (int)g.size();
}
}
