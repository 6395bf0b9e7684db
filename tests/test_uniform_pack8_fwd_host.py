"""CPU suite: the host-testable parts of the eights' forward pass on compact tiles ("Forward tiles"): the
layout helpers of cnf2freq_amd/csrc/cnf2_lane.h (up8_fwd_*: where value i of (marker t, job) sits in a tile, where a tile sits
in the wave's LDS region) against the lanes that write and read them in fb_unipack8_kernel, and the unrestricted entries the
packed kernels' producer still stores (cnf2_emtab.h packed_reads_unrestricted) against the indices emission_from_row reads.
Compiled into a small shim of their own."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TAB_STRIDE, TAB_C = 202, 64
REGION = 8 * TAB_STRIDE                  # doubles of a wave's LDS region: eight table rows
# every value CNF2_UP8_FWD_TILE may take beside 1 (the row form): even, and one tile must fit the region
TILES = [T for T in range(2, 64, 2) if T * 128 <= REGION]


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g
    g.build()
    shim_dir = os.path.join(ROOT, "tests", "shim")
    csrc = os.path.join(ROOT, "cnf2freq_amd", "csrc")
    so = os.path.join(shim_dir, "libcnf2unipack8fwdshim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(shim_dir, "unipack8_fwd_shim.cpp")])
    return C.CDLL(so)


def _producer_places(s, lane):
    """What producer lane (part = lane >> 3, job = lane & 7) stores for a marker, from the marker's first double:
    {place: what}, as produce_slot_rec does."""
    part, job = lane >> 3, lane & 7
    f = (part >> 1) & 1
    out = {s.up8f_shim_at(0, job, s.up8f_shim_part(part)): ("part", part, job)}
    if part & 5 == 0:                        # P == 0, firstpar == 0: one writer per f
        for s0 in range(2):
            out[s.up8f_shim_at(0, job, s.up8f_shim_weight(f, s0))] = ("weight", f, s0, job)
    if part == 0:
        for k in range(2):
            out[s.up8f_shim_at(0, job, s.up8f_shim_gap(k))] = ("gap", k, job)
    return out


def _reader_places(s, lane):
    """What recursion lane (job, s0, s2, class) reads for a marker, from the marker's first double: {place: what}, as
    fb_unipack8_kernel's Up8FwdSlot does from its three lane pointers."""
    job, s0, b0 = s.up8f_shim_job(lane), s.up8f_shim_s0(lane), s.up8f_shim_b0(lane)
    F = s.up8f_shim_at(0, 0, 2)
    qa = s.up8f_shim_at(0, job, s.up8f_shim_part(b0))
    qc = s.up8f_shim_at(0, job, s.up8f_shim_weight(0, s0))
    qb = s.up8f_shim_at(0, job, s.up8f_shim_part(4))
    out = {}
    for f in range(2):
        out[qa + f * F] = ("part", (0 << 2) | (f << 1) | b0, job)           # A side: the part of (f, firstpar = class)
        out[qc + f * F] = ("weight", f, s0, job)
        for j in range(2):
            out[qb + f * F + s.up8f_shim_at(0, 0, j)] = ("part", (1 << 2) | (f << 1) | j, job)      # B side: firstpar = register
    for k in range(2):
        out[qb + s.up8f_shim_at(0, 0, s.up8f_shim_gap(k) - 4)] = ("gap", k, job)
    assert len(out) == 10            # 2 + 4 parts, 2 weights, 2 factors: the slot's other 4 values are the other class's and s0's
    return out


def test_tile_sizes():
    assert TILES == [2, 4, 6, 8, 10, 12]


def test_constants(shim):
    assert shim.up8f_shim_values() == 14 and shim.up8f_shim_slot() == 16
    assert shim.up8f_shim_marker() == 8 * 16 == shim.up8f_shim_at(1, 0, 0)
    used = sorted({shim.up8f_shim_part(p) for p in range(8)} | {shim.up8f_shim_weight(f, s0) for f in range(2) for s0 in range(2)}
                  | {shim.up8f_shim_gap(k) for k in range(2)})
    assert used == list(range(14)), "a slot's 14 values, each at an index of its own"


@pytest.mark.parametrize("T", TILES)
def test_producer_lanes_write_distinct_places_inside_the_region(shim, T):
    nb = shim.up8f_shim_buffers(T, REGION)
    assert nb == (2 if 2 * T * 128 <= REGION else 1)
    for tile in range(4):
        base = shim.up8f_shim_tile(T, REGION, tile)
        seen = {}
        for t in range(T):
            m = base + shim.up8f_shim_at(t, 0, 0)
            for lane in range(64):
                for place, what in _producer_places(shim, lane).items():
                    assert 0 <= m + place < REGION, (T, tile, t, lane, place)
                    assert m + place not in seen, "lanes %r and %r write %d" % (seen[m + place], (t, lane), m + place)
                    seen[m + place] = (t, lane)
        assert len(seen) == T * 8 * 14
        # the 64 part values of a marker are 64 consecutive doubles, lane by lane: no two lanes of a store share a bank
        for t in range(T):
            assert [shim.up8f_shim_at(t, lane & 7, shim.up8f_shim_part(lane >> 3)) for lane in range(64)] == \
                list(range(shim.up8f_shim_at(t, 0, 0), shim.up8f_shim_at(t, 0, 0) + 64))


@pytest.mark.parametrize("T", TILES)
def test_every_read_is_written_by_the_lane_of_its_part_and_job(shim, T):
    writers = [_producer_places(shim, lane) for lane in range(64)]
    for t in range(T):
        for lane in range(64):
            for place, what in _reader_places(shim, lane).items():
                who = [w for w in range(64) if place in writers[w]]
                assert len(who) == 1, (T, t, lane, place, who)
                assert writers[who[0]][place] == what, (lane, place, what, writers[who[0]][place])
                if what[0] == "part":
                    assert (who[0] >> 3, who[0] & 7) == (what[1], what[2])
                # (the place of marker t is the same offset from up8_fwd_at(t, 0, 0) for every t)
                assert shim.up8f_shim_at(t, 0, 0) + place < (t + 1) * shim.up8f_shim_marker()
    # the eight jobs' lanes read eight consecutive doubles where they ask for the same value
    for i in range(14):
        assert [shim.up8f_shim_at(0, job, i) for job in range(8)] == list(range(shim.up8f_shim_at(0, 0, i), shim.up8f_shim_at(0, 0, i) + 8))


@pytest.mark.parametrize("T", TILES)
def test_two_buffers_do_not_overlap(shim, T):
    size = T * shim.up8f_shim_marker()
    if shim.up8f_shim_buffers(T, REGION) == 1:
        assert size <= REGION and 2 * size > REGION
        assert {shim.up8f_shim_tile(T, REGION, k) for k in range(6)} == {0}
        return
    b = [shim.up8f_shim_tile(T, REGION, k) for k in range(6)]
    assert b[0::2] == [b[0]] * 3 and b[1::2] == [b[1]] * 3, "tile k + 2 goes where tile k was"
    lo, hi = sorted(b[:2])
    assert lo >= 0 and lo + size <= hi and hi + size <= REGION


def test_trimmed_entries_are_the_ones_the_packed_kernels_read(shim):
    kept = [e for e in range(8) if shim.up8f_shim_packed_reads_unrestricted(e)]
    assert kept == [0, 4]
    assert shim.up8f_shim_entries_stored(1) == (1 << 0) | (1 << 4) and shim.up8f_shim_entries_stored(0) == 0xff
    stored = {shim.up8f_shim_part_entry_index(part, e) for part in range(8) for e in kept}
    assert len(stored) == 16

    def reads(s1, lo, s2):
        """emission_from_row with N = 2: the table indices of one lane."""
        a = {(0 << 5) | (f << 4) | (s1 << 3) | lo for f in range(2)}
        b = {(1 << 5) | (f << 4) | (s2 << 3) | j for f in range(2) for j in range(2)}
        return a | b

    eights = set().union(*(reads(0, b0, s2) for b0 in range(2) for s2 in range(2)))
    fours = set().union(*(reads(s1, b0, s2) for s1 in range(2) for b0 in range(2) for s2 in range(2)))
    assert eights <= stored and fours == stored
    # what the eights leave unread of it: the A side at the parent's shift bit set, which the fours' chains with s1 = 1 read
    assert stored - eights == {(f << 4) | (1 << 3) | k for f in range(2) for k in range(2)}
    # and of a part's entries the eights read e = 0, and e = 4 on the B side only
    for part in range(8):
        mine = {e for e in range(8) if shim.up8f_shim_part_entry_index(part, e) in eights}
        assert mine == ({0, 4} if part >> 2 else {0}), (part, mine)
    assert max(stored) < TAB_C
