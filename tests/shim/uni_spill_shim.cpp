// Host build of the compact spill row's offset arithmetic (cnf2_lane.h) for tests/test_uniform_spill_host.py: what each of a
// wave's 64 lanes does with a row of the uniform-state sweep.
#include <stdint.h>

#include "cnf2_lane.h"

using namespace cnf2;

// out[lane] = {writes, value offset (doubles), reciprocal offset of the lane's chain (doubles), state_lo}; returns the row size
extern "C" int shim_uni_spill_layout(int32_t* out)
{
    for (int lane = 0; lane < 64; lane++) {
        out[4 * lane + 0] = uni_spill_writer(lane) ? 1 : 0;
        out[4 * lane + 1] = uni_spill_value(lane);
        out[4 * lane + 2] = uni_spill_inv(lane >> 3);
        out[4 * lane + 3] = state_lo(lane);
    }
    return UNI_SPILL_ROW;
}
