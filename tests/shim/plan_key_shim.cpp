// Host build of the kept plan's key (cnf2_plan.h: PlanKey, plan_key_same_jobs, plan_key_same) for tests/test_plan_cache_host.py.
#include <stdint.h>

#include "cnf2_plan.h"

using namespace cnf2;

namespace {
// field order of the test: windows_gen, map_gen, ind_begin, n, flags, uniform_mode, n_lines, lines_cap, lines_fit, pack_cap,
// reserve_blocks, uni_blocks_per_cu
PlanKey make(const int64_t* v)
{
    PlanKey k;
    k.windows_gen       = (unsigned)v[0];
    k.map_gen           = (unsigned)v[1];
    k.ind_begin         = (int)v[2];
    k.n                 = (int)v[3];
    k.flags             = (uint32_t)v[4];
    k.uniform_mode      = (int)v[5];
    k.n_lines           = (int)v[6];
    k.lines_cap         = (int)v[7];
    k.lines_fit         = (int)v[8];
    k.pack_cap          = (int)v[9];
    k.reserve_blocks    = (int)v[10];
    k.uni_blocks_per_cu = (int)v[11];
    return k;
}
}  // namespace

extern "C" int shim_plan_key_fields() { return 12; }
extern "C" uint32_t shim_plan_key_flags() { return PLAN_KEY_FLAGS; }
// bit 0: plan_key_same_jobs(a, b), bit 1: plan_key_same(a, b)
extern "C" int shim_plan_key_compare(const int64_t* a, const int64_t* b)
{
    const PlanKey ka = make(a), kb = make(b);
    return (plan_key_same_jobs(ka, kb) ? 1 : 0) | (plan_key_same(ka, kb) ? 2 : 0);
}
