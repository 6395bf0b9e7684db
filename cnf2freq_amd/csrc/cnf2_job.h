// cnf2_job.h -- the units of work of a sweep launch, shared by the kernels (cnf2_device.h) and the host-side planner
// (cnf2_plan.h).  Plain C++ (no HIP) so that the planner is unit-testable without a GPU.
#ifndef CNF2_JOB_H
#define CNF2_JOB_H

#include <stdint.h>

namespace cnf2 {

#define CNF2_BLOCK 256
#define CNF2_WAVES_PER_BLOCK (CNF2_BLOCK / 64)

// One unit of sequential work: an analysed individual on one chromosome
// (the body of the loops at cnF2freq.cpp:5283 and 5294).
struct Job {
    int32_t ind;     // index into windows[] / output rows (local to the call)
    int32_t first;   // chromstarts[c]
    int32_t last;    // chromstarts[c+1] - 1
    int32_t chrom;
};

// Four jobs of the same chromosome swept by one wavefront (fb_packed_kernel).
struct PackedJob {
    int32_t ind[4];
    int32_t first, last, chrom;
    int32_t homleaf;   // all four jobs: the grandparents are present and homozygous everywhere too (HOMLEAF)
};

} // namespace cnf2
#endif
