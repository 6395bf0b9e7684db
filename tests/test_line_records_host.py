"""CPU suite: the line records of the uniform windows (cnf2_emtab.h) on the host.

A record holds what a parent and its two grandparents contribute to a lane's emission entries; `emtab_part_rec` combines it
with the root's own terms.  Over every homozygous (parent, traced grandparent, other grandparent) triple with alleles
{0, 1, 2, 3, 9} and sure {0, 0.02, 0.37, 0.5, 1}, every combination of SLOT_RESTRICT0, all 8 parts and random roots
(heterozygous ones, every sure and haploweight), records + consumer must equal the general producer `emtab_part<CLASSES>` to
the bit -- the host build has no fused multiply-add, so this checks the algebra and the masks, and the GPU suite
(test_gpu_line_records.py) the device's rounding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ROOTS_PER_LINE = 3       # 25^3 triples x 8 restriction masks x 8 parts x 3 roots = 3.0e6 parts, 24 entries each


@pytest.fixture(scope="module")
def shim():
    shim_dir = os.path.join(ROOT, "tests", "shim")
    so = os.path.join(shim_dir, "libcnf2linerec.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "cnf2freq_amd", "csrc"), "-o", so, os.path.join(shim_dir, "line_records_shim.cpp")])
    lib = C.CDLL(so)
    lib.shim_line_records_grid.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.shim_line_records_grid.restype = None
    return lib


@pytest.mark.parametrize("classes", [0, 1], ids=["tot_only", "classes"])
def test_records_and_consumer_equal_the_general_producer(shim, classes):
    counts = np.zeros(4, np.int64)
    first_bad = np.zeros(10, np.int32)
    shim.shim_line_records_grid(classes, ROOTS_PER_LINE, 12345 + classes, counts.ctypes.data, first_bad.ctypes.data)
    assert counts[0] == 25 ** 3 * 8 * 8 * ROOTS_PER_LINE
    assert counts[1] == 0, "%d of %d parts differ; first (ip, it, io, restrict, part, root a0 a1 is0 is1 ihw) = %s" % (
        counts[1], counts[0], first_bad.tolist())
    if classes:
        assert counts[3] > counts[0] // 20, "the grid should reach nonzero restricted / class-2 entries"


def test_one_value_per_part(shim):
    """The property the consumer rests on: within a part every entry of the three tables is 0 or the bits of one value."""
    counts = np.zeros(4, np.int64)
    first_bad = np.zeros(10, np.int32)
    shim.shim_line_records_grid(1, 1, 777, counts.ctypes.data, first_bad.ctypes.data)
    assert counts[2] == 0, "%d of %d parts hold two different nonzero values" % (counts[2], counts[0])
