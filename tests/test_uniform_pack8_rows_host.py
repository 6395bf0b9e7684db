"""CPU suite: the lane helpers of the eights' row sums in registers (*Row sums in registers*;
cnf2freq_amd/csrc/cnf2_lane.h up8_sum_*, up8_place_*, up8_partner), compiled into a small shim of their own.

A lane of fb_unipack8_kernel adds up the eight row partials of one chain of its job and the job's chains are then added across
lanes.  The results keep their bits only if a lane adds exactly the partials the tile epilogue's lane (row, chain) added, in
its order, formed from the class sums of the lane that formed them before, and if the exchange adds the chains as chain_sum
did: that is what is held here, on the helpers the kernel uses."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the table row of the sweep kernels (cnf2_kernels.hip): doubles per row, and where its parts begin
TAB_STRIDE, TAB_R, TAB_2 = 202, 72, 136


@pytest.fixture(scope="module")
def shim():
    shim_dir = os.path.join(ROOT, "tests", "shim")
    csrc = os.path.join(ROOT, "cnf2freq_amd", "csrc")
    so = os.path.join(shim_dir, "libcnf2unipack8rowsshim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(shim_dir, "unipack8_rows_shim.cpp")])
    return C.CDLL(so)


def _chain(s, lane):
    return s.up8r_s0(lane) | (s.up8r_sum_s1(lane) << 1) | (s.up8r_s2(lane) << 2)


def test_places_are_one_chain_in_ascending_place(shim):
    for lane in range(64):
        s = _chain(shim, lane)
        got = [s * 8 + shim.up8r_state_lo(shim.up8r_place_b(i2) | (shim.up8r_place_v(i2) << 1)) for i2 in range(8)]
        assert got == [s * 8 + i2 for i2 in range(8)], (lane, got)
    # the table of the places, written out
    assert [(shim.up8r_place_b(i), shim.up8r_place_v(i)) for i in range(8)] == [(0, 0), (1, 0), (0, 1), (1, 1), (1, 3), (0, 3), (1, 2), (0, 2)]
    # two places that follow each other are the two classes of one v: one 16-byte read a run
    for ip in range(4):
        assert shim.up8r_place_v(2 * ip) == shim.up8r_place_v(2 * ip + 1)
        assert {shim.up8r_place_b(2 * ip), shim.up8r_place_b(2 * ip + 1)} == {0, 1}


def test_virtual_lanes_of_each_job_are_covered_once(shim):
    for job in range(8):
        seen = []
        for lane in range(64):
            if shim.up8r_job(lane) == job:
                seen += [_chain(shim, lane) * 8 + i2 for i2 in range(8)]
        assert sorted(seen) == list(range(64)), (job, sorted(seen))


def test_class_at_a_place_is_the_forming_lanes_class(shim):
    """Virtual lane (chain, place) is formed, in the parked form, by the lane with the chain's s0 and s2 whose class is the
    place's: the lane of the b0 pair whose class sums the new form uses there."""
    for lane in range(64):
        s1 = shim.up8r_sum_s1(lane)
        for i2 in range(8):
            b, v = shim.up8r_place_b(i2), shim.up8r_place_v(i2)
            owner = [l for l in (lane, shim.up8r_partner(lane, 1)) if shim.up8r_b0(l) == b]
            assert len(owner) == 1, (lane, i2, owner)
            o = owner[0]
            assert (shim.up8r_job(o), shim.up8r_s0(o), shim.up8r_s2(o)) == (shim.up8r_job(lane), shim.up8r_s0(lane), shim.up8r_s2(lane))
            assert shim.up8r_virtual_lane(o, s1, v) == _chain(shim, lane) * 8 + i2, (lane, i2)
    # the pair splits the two s1 between its lanes
    for lane in range(64):
        assert shim.up8r_sum_s1(lane) ^ shim.up8r_sum_s1(lane ^ 1) == 1


def test_partners_reproduce_chain_sums_tree(shim):
    coords = lambda l: (shim.up8r_job(l), shim.up8r_s0(l), shim.up8r_sum_s1(l), shim.up8r_s2(l))
    for lane in range(64):
        job, s0, s1, s2 = coords(lane)
        assert coords(shim.up8r_partner(lane, 0)) == (job, s0 ^ 1, s1, s2)
        assert coords(shim.up8r_partner(lane, 1)) == (job, s0, s1 ^ 1, s2)
        assert coords(shim.up8r_partner(lane, 2)) == (job, s0, s1, s2 ^ 1)
    # symbolic operands: a sum is the unordered pair of what it adds (IEEE addition commutes, it does not associate)
    val = [("c", shim.up8r_job(l), _chain(shim, l)) for l in range(64)]
    for level in range(3):
        val = [frozenset((val[l], val[shim.up8r_partner(l, level)])) for l in range(64)]
        assert all(len(x) == 2 for x in val)
    for lane in range(64):
        c = [("c", shim.up8r_job(lane), s) for s in range(8)]
        add = lambda a, b: frozenset((a, b))
        want = add(add(add(c[0], c[1]), add(c[2], c[3])), add(add(c[4], c[5]), add(c[6], c[7])))
        assert val[lane] == want, lane


def test_a_side_runs_are_16_byte_aligned_and_hold_the_chains_entries(shim):
    assert TAB_STRIDE % 2 == 0 and TAB_R % 2 == 0 and TAB_2 % 2 == 0
    for s1 in range(2):
        for f in range(2):
            run = shim.up8r_sum_run(f, s1)
            assert run == (f << 4) | (s1 << 3)
            for tab in (TAB_R, TAB_2):
                assert (tab + run) % 2 == 0
                for i2 in range(8):
                    b, v = shim.up8r_place_b(i2), shim.up8r_place_v(i2)
                    ia = (f << 4) | (s1 << 3) | b | (v << 1)           # the parked form's index
                    assert ia == run + (v << 1) + b and (tab + run + (v << 1)) % 2 == 0
                    assert run <= ia < run + 8
    # the A side is the lower half of a table: the runs stay inside it
    assert max(shim.up8r_sum_run(f, s1) + 8 for f in range(2) for s1 in range(2)) == 32
