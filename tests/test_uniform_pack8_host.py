"""CPU suite: the host-testable parts of the sweep that takes eight uniform windows to a wave: the lane
helpers of cnf2freq_amd/csrc/cnf2_lane.h (up8_*: which job, chains and class a lane carries, which lanes of a job's own sweep
it stands for, where their partials are parked in the job's table row, where it spills) and the pairing of the groups of four
(cnf2_plan.h pair_uniform_groups), compiled into a small shim of their own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WINDOW = np.dtype(dict(names=["row", "flags", "tie", "shiftignore", "shiftend", "n_groups", "flag2ignore", "rec"],
                       formats=[("<i4", 7), ("u1", 7), ("i1", 7), "u1", "u1", "u1", "u1", "<i4"],
                       offsets=[0, 28, 35, 42, 43, 44, 45, 48], itemsize=64))
# the table row of the sweep kernels (cnf2_kernels.hip): doubles per row, and where its parts begin
TAB_STRIDE, TAB_C, TAB_R, TAB_2 = 202, 64, 72, 136


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g
    g.build()
    shim_dir = os.path.join(ROOT, "tests", "shim")
    csrc = os.path.join(ROOT, "cnf2freq_amd", "csrc")
    so = os.path.join(shim_dir, "libcnf2unipack8shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(shim_dir, "unipack8_shim.cpp")])
    s = C.CDLL(so)
    s.up8_shim_pair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert s.up8_shim_sizeof_window() == WINDOW.itemsize
    return s


# ---------------------------------------------------------------------------------------------- lanes
def test_lane_map_is_a_bijection(shim):
    seen = {}
    for lane in range(64):
        key = (shim.up8_shim_job(lane), shim.up8_shim_s0(lane), shim.up8_shim_s2(lane), shim.up8_shim_b0(lane))
        assert 0 <= key[0] < 8 and all(0 <= k < 2 for k in key[1:])
        assert key not in seen, "lanes %d and %d carry the same (job, s0, s2, class)" % (seen[key], lane)
        seen[key] = lane
    assert len(seen) == 64
    for lane in range(64):
        job, s0, s2, b0 = (shim.up8_shim_job(lane), shim.up8_shim_s0(lane), shim.up8_shim_s2(lane), shim.up8_shim_b0(lane))
        # the exchange of the uniform recursion stays inside a job and a chain: lane ^ 1 flips the class only
        o = lane ^ 1
        assert (shim.up8_shim_job(o), shim.up8_shim_s0(o), shim.up8_shim_s2(o), shim.up8_shim_b0(o)) == (job, s0, s2, b0 ^ 1)
        # lane ^ 8 is the job's other distinct chain (the likelihoods add the two), lane ^ 16 its copy with the other s2
        o = lane ^ 8
        assert (shim.up8_shim_job(o), shim.up8_shim_s0(o), shim.up8_shim_s2(o), shim.up8_shim_b0(o)) == (job, s0 ^ 1, s2, b0)
        o = lane ^ 16
        assert (shim.up8_shim_job(o), shim.up8_shim_s0(o), shim.up8_shim_s2(o), shim.up8_shim_b0(o)) == (job, s0, s2 ^ 1, b0)
        # the producer's and the epilogue's row of a job is the job: the lanes of one half of the wave hold jobs 0..3 or 4..7
        assert job >> 2 == lane >> 5


def test_virtual_lanes_cover_each_jobs_partial_slots_once(shim):
    for job in range(8):
        slots, places = [], []
        for lane in range(64):
            if shim.up8_shim_job(lane) != job:
                continue
            s0, s2, b0 = shim.up8_shim_s0(lane), shim.up8_shim_s2(lane), shim.up8_shim_b0(lane)
            for s1 in range(2):
                for v in range(4):
                    vl = shim.up8_shim_virtual_lane(lane, s1, v)
                    # the lane of the job's own sweep in chain s0 | s1 << 1 | s2 << 2 with this class and state bits 1, 2 = v
                    assert vl >> 3 == s0 | (s1 << 1) | (s2 << 2)
                    assert vl == (vl >> 3) * 8 + shim.up8_shim_state_lo(b0 | (v << 1))
                    lo = shim.up8_shim_state_lo(vl)
                    assert lo & 1 == b0 and lo >> 1 == v
                    slots.append(vl)
                    places += [shim.up8_shim_park(cls, vl) for cls in range(3)]
        assert sorted(slots) == list(range(64)), (job, sorted(slots))
        # 3 x 64 partials, each at a place of its own inside the row
        assert len(set(places)) == 192 and min(places) >= 0 and max(places) < TAB_STRIDE


def test_parking_overwrites_nothing_that_is_still_read(shim):
    # A-side entries of the restricted and class-2 tables that the partials of s1 read: index f << 4 | s1 << 3 | k
    def a_side(s1):
        return {t + (f << 4) + (s1 << 3) + k for t in (TAB_R, TAB_2) for f in range(2) for k in range(8)}

    first = {shim.up8_shim_park(cls, vl) for cls in range(3) for vl in range(64) if (vl >> 4) & 1}      # s1 = 1: parked first
    second = {shim.up8_shim_park(cls, vl) for cls in range(3) for vl in range(64) if not (vl >> 4) & 1}
    assert len(first) == len(second) == 96 and not first & second
    assert not first & a_side(0), "the partials of s1 = 1 are parked while the A side of s1 = 0 is still to be read"
    # the epilogue reads a chain's eight partials of a class side by side, aligned to 16 bytes
    for cls in range(3):
        for s in range(8):
            base = shim.up8_shim_park(cls, s * 8)
            assert base % 2 == 0 and (TAB_STRIDE % 2) == 0
            assert [shim.up8_shim_park(cls, s * 8 + k) for k in range(8)] == list(range(base, base + 8))


def test_spill_offsets_are_disjoint_aligned_and_inside_the_row(shim):
    row = shim.up8_shim_spill_row()
    assert row == 160 and row <= shim.up8_shim_plan_spill_row() and row % 2 == 0
    used = []
    for lane in range(64):
        o, w = shim.up8_shim_spill_value(lane), shim.up8_shim_spill_emit(lane)
        assert o % 2 == 0 and w % 2 == 0, "16-byte accesses"
        # every lane loads what the writer of its job, s0 and class stored
        twin = lane & ~16
        assert shim.up8_shim_spill_writer(twin) and shim.up8_shim_s2(twin) == 0
        assert (shim.up8_shim_spill_value(twin), shim.up8_shim_spill_emit(twin)) == (o, w)
        assert shim.up8_shim_spill_writer(lane) == (shim.up8_shim_s2(lane) == 0)
        if shim.up8_shim_spill_writer(lane):
            used += [o, o + 1, w, w + 1]
    for job in range(8):
        for s0 in range(2):
            o = shim.up8_shim_spill_inv(job, s0)
            assert o % 2 == 0
            used += [o, o + 1]
    assert len(used) == len(set(used)) == row and min(used) == 0 and max(used) == row - 1


# ---------------------------------------------------------------------------------------------- pairing
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _windows(n, partial=()):
    """n windows with all eight modes analysed, but for those of `partial`: {ind: (shiftignore, shiftend)}."""
    w = np.zeros(n, WINDOW)
    w["shiftend"] = 8
    for i, (ign, end) in dict(partial).items():
        w["shiftignore"][i] = ign
        w["shiftend"][i] = end
    return w


def _groups(chroms, n_ind_fours):
    """The list group_uniform_jobs makes: chromosome by chromosome, the fours of the individuals in order."""
    g = []
    for c in chroms:
        for k in range(n_ind_fours):
            g.append([4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3, 100 * c, 100 * c + 99, c, 1])
    return np.array(g, np.int32).reshape(-1, 8)


def _pair(shim, groups, win, waves):
    g = groups.copy()
    n8 = shim.up8_shim_pair(_p(g), len(g), _p(win), waves)
    assert n8 >= 0
    return n8, [tuple(r) for r in g.tolist()]


def test_no_pair_across_chromosomes(shim):
    groups = _groups([2, 0, 1], 3)              # three fours a chromosome: one pair and one four left, per chromosome
    rows = [tuple(r) for r in groups.tolist()]
    n8, got = _pair(shim, groups, _windows(12), 0)
    assert n8 == 3
    assert got[:6] == [rows[0], rows[1], rows[3], rows[4], rows[6], rows[7]]
    assert all(got[2 * e][6] == got[2 * e + 1][6] for e in range(n8))
    assert got[6:] == [rows[2], rows[5], rows[8]]


@pytest.mark.parametrize("partial", [(1, 8), (0, 4), (2, 6)])
def test_a_four_with_a_window_short_of_modes_stays_a_four(shim, partial):
    groups = _groups([0], 5)
    rows = [tuple(r) for r in groups.tolist()]
    win = _windows(20, {6: partial})            # individual 6 sits in the second four
    n8, got = _pair(shim, groups, win, 0)
    assert n8 == 2
    assert got[:4] == [rows[0], rows[2], rows[3], rows[4]]
    assert got[4:] == [rows[1]]


def test_fours_behind_keep_their_order_and_nothing_is_lost(shim):
    groups = _groups([3, 1], 6)
    rows = [tuple(r) for r in groups.tolist()]
    win = _windows(24, {0: (4, 8), 13: (0, 2)})   # the first and the fourth four of each chromosome stay fours
    n8, got = _pair(shim, groups, win, 0)
    assert n8 == 4
    assert got[:8] == [rows[1], rows[2], rows[4], rows[5], rows[7], rows[8], rows[10], rows[11]]
    assert got[8:] == [rows[0], rows[3], rows[6], rows[9]]
    assert sorted(got) == sorted(rows)
    # nothing to pair: the list stays as it is
    n8, got = _pair(shim, groups[:1], win, 0)
    assert n8 == 0 and got == rows[:1]
    n8, got = _pair(shim, groups, _windows(24, {i: (1, 8) for i in range(0, 24, 4)}), 0)
    assert n8 == 0 and got == rows


def test_whole_rounds_of_eights(shim):
    groups = _groups([0], 28)                   # 14 pairs
    rows = [tuple(r) for r in groups.tolist()]
    win = _windows(4 * 28)
    n8, got = _pair(shim, groups, win, 4)       # 4 waves: 3 rounds of eights, 2 pairs handed back
    assert n8 == 12
    assert got == rows
    assert got[24:] == rows[24:]
    # fewer pairs than waves: all are kept
    n8, got = _pair(shim, groups, win, 15)
    assert n8 == 14 and got == rows
    n8, got = _pair(shim, groups[:6], win, 4)
    assert n8 == 3
    # as many as waves, and a multiple
    assert _pair(shim, groups, win, 14)[0] == 14
    assert _pair(shim, groups, win, 7)[0] == 14
    assert _pair(shim, groups, win, 5)[0] == 10
