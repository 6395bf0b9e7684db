"""CPU suite: where the eights stage the root's data of a tile of markers in the wave's LDS region ("Root
staging"; cnf2freq_amd/csrc/cnf2_lane.h up8_stage_*), against the lanes that write and read the staging places in
fb_unipack8_kernel and against everything else that lives in the region: the forward tile's slots, and in the backward pass the
places of a table row that the packed producer writes and `marker()` / `emission_from_row` read.  The macros allow one tile
length (eight markers, the forward tile's) and two buffers in either pass.  Compiled into a small shim of their own."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TAB_STRIDE, TAB_C, TAB_T, TAB_R = 202, 64, 68, 72
REGION = 8 * TAB_STRIDE                  # doubles of a wave's LDS region: eight table rows
BUFFERS = (0, 1)


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g
    g.build()
    shim_dir = os.path.join(ROOT, "tests", "shim")
    csrc = os.path.join(ROOT, "cnf2freq_amd", "csrc")
    so = os.path.join(shim_dir, "libcnf2unipack8stageshim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(shim_dir, "unipack8_stage_shim.cpp")])
    return C.CDLL(so)


def test_constants(shim):
    T = shim.up8s_shim_tile()
    assert T == 8, "a tile is the eight markers that share a line of `sure`"
    assert shim.up8s_shim_entry() == 4 and shim.up8s_shim_buffer() == T * 8 * 4
    # sure is a 16-byte read: an even double; the allele word sits behind hw
    assert (shim.up8s_shim_sure(), shim.up8s_shim_hw(), shim.up8s_shim_allele()) == (0, 2, 3)
    # the forward tiles of eight markers take one buffer of the region and leave room for both staging buffers
    assert shim.up8s_shim_fwd_buffers(T, REGION) == 1
    assert shim.up8s_shim_fwd_room(T, REGION) == REGION - T * shim.up8s_shim_fwd_marker() == 592 >= 2 * shim.up8s_shim_buffer()


# ---------------------------------------------------------------- forward: behind the tile
def _fwd_written(s, buf, lane):
    """The doubles staging lane (t = lane >> 3, job = lane & 7) writes in buffer buf: {place: what} (store_stage_fwd)."""
    T, t, job = s.up8s_shim_tile(), lane >> 3, lane & 7
    e = s.up8s_shim_fwd_at(T, REGION, buf, t, job)
    return {e + s.up8s_shim_sure(): ("sure0", t, job), e + s.up8s_shim_sure() + 1: ("sure1", t, job),
            e + s.up8s_shim_hw(): ("hw", t, job), e + s.up8s_shim_allele(): ("allele", t, job)}


def _fwd_read(s, buf, lane, t):
    """What producer lane (part = lane >> 3, job = lane & 7) reads for marker t of the tile in buffer buf."""
    T, job = s.up8s_shim_tile(), lane & 7
    e = s.up8s_shim_fwd_at(T, REGION, buf, 0, job) + t * 8 * s.up8s_shim_entry()      # (the kernel steps from marker to marker)
    return {e + s.up8s_shim_sure(): ("sure0", t, job), e + s.up8s_shim_sure() + 1: ("sure1", t, job),
            e + s.up8s_shim_hw(): ("hw", t, job), e + s.up8s_shim_allele(): ("allele", t, job)}


def test_forward_places_are_distinct_inside_the_region_and_behind_the_tile(shim):
    T = shim.up8s_shim_tile()
    tile_end = shim.up8s_shim_fwd_buffers(T, REGION) * T * shim.up8s_shim_fwd_marker()
    seen = {}
    for buf in BUFFERS:
        for lane in range(64):
            for place, what in _fwd_written(shim, buf, lane).items():
                assert tile_end <= place < REGION, (buf, lane, place)
                assert place not in seen, "%r and %r share %d" % (seen[place], (buf,) + what, place)
                seen[place] = (buf,) + what
            assert shim.up8s_shim_fwd_at(T, REGION, buf, lane >> 3, lane & 7) % 2 == 0, "sure is read 16 bytes at a time"
    assert len(seen) == 2 * 64 * 4


def test_forward_reads_are_written_by_the_lane_of_their_marker_and_job(shim):
    T = shim.up8s_shim_tile()
    for buf in BUFFERS:
        writers = [_fwd_written(shim, buf, lane) for lane in range(64)]
        for lane in range(64):
            for t in range(T):
                for place, what in _fwd_read(shim, buf, lane, t).items():
                    who = [w for w in range(64) if place in writers[w]]
                    assert who == [t * 8 + (lane & 7)], (buf, lane, t, place, who)
                    assert writers[who[0]][place] == what
        # the eight part lanes of a job read one address, the eight jobs consecutive entries
        for t in range(T):
            assert len({min(_fwd_read(shim, buf, part * 8 + 3, t)) for part in range(8)}) == 1
            firsts = [min(_fwd_read(shim, buf, job, t)) for job in range(8)]
            assert firsts == list(range(firsts[0], firsts[0] + 8 * 4, 4))


def test_forward_buffers_do_not_overlap(shim):
    T = shim.up8s_shim_tile()
    spans = []
    for buf in BUFFERS:
        places = sorted(p for lane in range(64) for p in _fwd_written(shim, buf, lane))
        assert places == list(range(places[0], places[0] + shim.up8s_shim_buffer())), "a buffer is one run of doubles"
        spans.append((places[0], places[-1]))
    assert spans[0][1] < spans[1][0] and spans[1][1] < REGION


# ---------------------------------------------------------------- backward: in the job's own table row
def _row_places_in_use(s):
    """The doubles of a table row that the packed producer (produce_row_rec<true, true>) writes; marker() and emission_from_row
    read a subset of them: the unrestricted entries the packed kernels keep, the root weights, the gap's factors and the two
    restricted tables."""
    kept = [e for e in range(8) if s.up8s_shim_packed_reads_unrestricted(e)]
    used = {s.up8s_shim_part_entry_index(part, e) for part in range(8) for e in kept}
    assert len(used) == 16 and max(used) < TAB_C
    used |= set(range(TAB_C, TAB_C + 4)) | {TAB_T, TAB_T + 1} | set(range(TAB_R, TAB_R + 128))
    # what the eights' marker() and emission_from_row (s1 = 0) read of the unrestricted table is among them
    reads = {(f << 4) | lo for f in range(2) for lo in range(2)} | {32 | (f << 4) | (s2 << 3) | j for f in range(2) for s2 in range(2) for j in range(2)}
    assert reads <= used
    return used


def _bwd_written(s, buf, lane):
    """Staging lane (t = lane >> 3, job = lane & 7): the doubles it writes in its job's row, and the byte of the allele double."""
    t = lane >> 3
    su, hw = s.up8s_shim_bwd_sure(buf, t), s.up8s_shim_bwd_hw(buf, t)
    return {su: ("sure0", t), su + 1: ("sure1", t), hw: ("hw", t)}, (s.up8s_shim_bwd_alleles(buf), t)


def test_backward_places_are_distinct_and_free(shim):
    T = shim.up8s_shim_tile()
    used = _row_places_in_use(shim)
    doubles, bytes_ = {}, set()
    for buf in BUFFERS:
        for t in range(T):
            d, (slot, byte) = _bwd_written(shim, buf, t * 8)
            assert d == _bwd_written(shim, buf, t * 8 + 5)[0], "a job's places do not depend on the job: each has its own row"
            for place, what in d.items():
                assert 0 <= place < TAB_STRIDE and place not in used, (buf, t, place)
                assert place not in doubles, "%r and %r share %d" % (doubles[place], (buf,) + what, place)
                doubles[place] = (buf,) + what
            assert shim.up8s_shim_bwd_sure(buf, t) % 2 == 0, "sure is read 16 bytes at a time (TAB_STRIDE is even)"
            assert 0 <= slot < TAB_STRIDE and slot not in used and 0 <= byte < 8
            assert (slot, byte) not in bytes_
            bytes_.add((slot, byte))
    assert len(doubles) == 2 * T * 3 and len(bytes_) == 2 * T
    assert not ({slot for slot, _ in bytes_} & set(doubles)), "the allele bytes have doubles of their own"
    # the kernel steps from marker to marker by eight doubles and from buffer to buffer by one allele double
    for buf in BUFFERS:
        assert [shim.up8s_shim_bwd_sure(buf, t) - shim.up8s_shim_bwd_sure(buf, 0) for t in range(T)] == [8 * t for t in range(T)]
        assert [shim.up8s_shim_bwd_hw(buf, t) - shim.up8s_shim_bwd_hw(buf, 0) for t in range(T)] == [8 * t for t in range(T)]
    assert shim.up8s_shim_bwd_alleles(1) == shim.up8s_shim_bwd_alleles(0) + 1


def test_backward_reads_are_written_by_the_lane_of_their_marker_and_job(shim):
    """A producer lane (part, job) reads marker t's places of row `job`: the staging lane t * 8 + job wrote them."""
    T = shim.up8s_shim_tile()
    for buf in BUFFERS:
        for lane in range(64):
            job = lane & 7
            for t in range(T):
                want = _bwd_written(shim, buf, t * 8 + job)
                who = [w for w in range(64) if (w & 7) == job and _bwd_written(shim, buf, w) == want]
                assert who == [t * 8 + job], (buf, lane, t, who)


def test_backward_buffers_do_not_overlap(shim):
    T = shim.up8s_shim_tile()
    a = {p for t in range(T) for p in _bwd_written(shim, 0, t * 8)[0]} | {shim.up8s_shim_bwd_alleles(0)}
    b = {p for t in range(T) for p in _bwd_written(shim, 1, t * 8)[0]} | {shim.up8s_shim_bwd_alleles(1)}
    assert len(a) == len(b) == 3 * T + 1 and not (a & b)
