"""CPU suite: the compact spill row of the uniform-state sweep (cnf2_lane.h) on the host.

In the uniform instantiation with two registers per lane, alpha does not depend on state bits 1, 2, 4, 5: the 8 lanes of a
chain hold two distinct register pairs, told apart by the lane's state bit 0.  A row keeps each pair once -- 8 chains x 2
classes x 2 doubles -- and the chains' reciprocals behind them.  The kernel takes every offset from the functions checked
here; the GPU suite (test_gpu_uniform_spill.py) checks the bits that come out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def layout():
    shim_dir = os.path.join(ROOT, "tests", "shim")
    so = os.path.join(shim_dir, "libcnf2unispill.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "cnf2freq_amd", "csrc"), "-o", so, os.path.join(shim_dir, "uni_spill_shim.cpp")])
    lib = C.CDLL(so)
    lib.shim_uni_spill_layout.argtypes = [C.c_void_p]
    lib.shim_uni_spill_layout.restype = C.c_int
    out = np.zeros((64, 4), np.int32)
    row = lib.shim_uni_spill_layout(out.ctypes.data)
    return row, out[:, 0].astype(bool), out[:, 1], out[:, 2], out[:, 3]


def test_row_is_48_doubles(layout):
    row = layout[0]
    assert row == 48
    assert row * 8 % 128 == 0, "rows stay aligned to 128-byte lines"


def test_state_lo_is_the_kernels_lane_order(layout):
    lo = layout[4]
    lane = np.arange(64)
    assert np.array_equal(lo, (lane & 7) ^ np.where(lane & 4, 3, 0))
    assert np.array_equal(lo.reshape(8, 8), np.tile(lo[:8], (8, 1))) and sorted(lo[:8]) == list(range(8))


def test_sixteen_writers_fill_the_values_exactly(layout):
    _, writes, value, _, lo = layout
    assert writes.sum() == 16
    assert np.array_equal(writes, (lo & 6) == 0)
    assert np.array_equal(np.flatnonzero(writes) & 7, np.tile([0, 1], 8)), "lanes 0 and 1 of each chain"
    # 16-byte stores: a permutation of 0..15 x 16 B, the wave's 256 contiguous bytes
    assert np.all(value[writes] % 2 == 0)
    assert sorted(value[writes] // 2) == list(range(16))


def test_every_lane_reads_what_its_class_wrote(layout):
    _, writes, value, _, lo = layout
    lane = np.arange(64)
    written = {(int(l) >> 3, int(lo[l]) & 1): int(value[l]) for l in lane[writes]}
    assert len(written) == 16
    for l in lane:
        assert value[l] == written[(l >> 3, int(lo[l]) & 1)], "lane %d" % l
    # four lanes share an address
    assert np.all(np.bincount(value, minlength=32)[::2] == 4)


def test_reciprocals_sit_behind_the_values(layout):
    row, _, value, inv, _ = layout
    lane = np.arange(64)
    assert np.array_equal(inv, 32 + 2 * (lane >> 3))
    cells = set()
    for l in lane:
        cells.update((int(inv[l]), int(inv[l]) + 1))
    assert cells == set(range(32, 48))
    vals = set()
    for l in lane:
        vals.update((int(value[l]), int(value[l]) + 1))
    assert vals == set(range(32)) and not (vals & cells)
    assert max(cells) < row
