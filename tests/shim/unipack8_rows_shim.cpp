// C interface for tests/test_uniform_pack8_rows_host.py: the lane helpers of the eights' row sums in registers (cnf2_lane.h
// up8_sum_*, up8_place_*, up8_partner) beside the ones they are held to (up8_virtual_lane and the lane's coordinates).  Host code only.
#include "cnf2_lane.h"

using namespace cnf2;

extern "C" {

int up8r_state_lo(int lane) { return state_lo(lane); }
int up8r_job(int lane) { return up8_job(lane); }
int up8r_s0(int lane) { return up8_s0(lane); }
int up8r_s2(int lane) { return up8_s2(lane); }
int up8r_b0(int lane) { return up8_b0(lane); }
int up8r_virtual_lane(int lane, int s1, int v) { return up8_virtual_lane(lane, s1, v); }
int up8r_sum_s1(int lane) { return up8_sum_s1(lane); }
int up8r_place_b(int i2) { return up8_place_b(i2); }
int up8r_place_v(int i2) { return up8_place_v(i2); }
int up8r_partner(int lane, int level) { return up8_partner(lane, level); }
int up8r_sum_run(int f, int s1) { return up8_sum_run(f, s1); }
}
