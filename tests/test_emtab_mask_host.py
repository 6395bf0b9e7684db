"""CPU suite: the record consumer's bit masks (cnf2_emtab.h keep_if_bit, emtab_part_rec) against the select form.

`keep_if_bit(bits, e, v)` stands for `((bits >> e) & 1) ? v : 0.0` in emtab_part_rec: the value's bit pattern or all zero bits,
whatever the value.  The select form is restated here, in Python, and bit patterns (uint64) are compared, not values: -0.0, a
NaN's payload and a denormal must come through as they are, and a cleared entry must be +0.0."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LR_LIVE_BIT = 16
UNSET = 0x7FF8DEADBEEF0001          # an entry the consumer does not hand over (a NaN no product forms)


@pytest.fixture(scope="module")
def shim():
    shim_dir = os.path.join(ROOT, "tests", "shim")
    so = os.path.join(shim_dir, "libcnf2emtabmask.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "cnf2freq_amd", "csrc"), "-o", so, os.path.join(shim_dir, "emtab_mask_shim.cpp")])
    lib = C.CDLL(so)
    lib.shim_keep_if_bit.argtypes = [C.c_uint32, C.c_int, C.c_uint64]
    lib.shim_keep_if_bit.restype = C.c_uint64
    lib.shim_part_rec.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64,
                                  C.c_void_p, C.c_void_p]
    lib.shim_part_rec.restype = None
    return lib


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


VALUES = {
    "+x": _bits(0.8125),
    "-0.0": 0x8000000000000000,
    "NaN with payload": 0x7FF800000BADC0DE,
    "+inf": _bits(float("inf")),
    "-inf": _bits(float("-inf")),
    "denormal": 0x0000000000000123,
}


@pytest.mark.parametrize("name", sorted(VALUES))
def test_helper_against_the_select(shim, name):
    v = VALUES[name]
    for e in range(17):
        for others in (0, 0xFFFFFFFF):                      # the other bits clear, or all set
            set_, clear = (others | (1 << e)) & 0xFFFFFFFF, others & ~(1 << e) & 0xFFFFFFFF
            assert shim.shim_keep_if_bit(set_, e, v) == v, (name, e, hex(set_))          # select: bit set -> v
            assert shim.shim_keep_if_bit(clear, e, v) == 0, (name, e, hex(clear))        # select: bit clear -> +0.0


def _select_form(classes, packed, P, f, root, rec, bits):
    """emtab_part_rec's entries as the select form gives them: [n][3][8] bit patterns."""
    a0, a1, s0, s1, _ = root
    Bp, Cp, Kp, t0, t1, oo = rec
    mf = a1 if f else a0
    sf, so_r = (s1, s0) if f else (s0, s1)
    msv_r = sf if mf != 0 else 0.0
    u0 = 1.0 - so_r if P else 1.0 - sf
    u1 = so_r if P else msv_r
    alpha = u0 * Bp
    beta = u0 * Cp + u1 * Kp
    va = oo * (alpha * t0 + beta * t1)
    vb = oo * (beta * t1 + alpha * t0)
    out = np.full((len(bits), 3, 8), UNSET, np.uint64)
    b = np.asarray(bits, np.uint64)
    ua, ub, zero = np.uint64(_bits(va)), np.uint64(_bits(vb)), np.uint64(_bits(0.0))
    sel = lambda e, u: np.where((b >> np.uint64(e)) & np.uint64(1) != 0, u, zero)      # ((bits >> e) & 1) ? u : 0.0
    for e in range(8):
        if not packed or (e & 3) == 0:
            out[:, 0, e] = sel(LR_LIVE_BIT, ua)
        if classes:
            out[:, 1, e] = sel(e, ua if e & 1 else ub)
            out[:, 2, e] = sel(8 + e, ua)
    return out


def _all_bits():
    rng = np.random.default_rng(20240611)
    single = [1 << e for e in range(32)]
    return np.array(single + [0xFFFFFFFF, 0] + [int(x) for x in rng.integers(0, 1 << 32, 10000, dtype=np.uint64)], np.uint32)


ROOTS = [(1, 2, 0.02, 0.37, 0.31), (2, 0, 0.0, 0.5, 0.5), (0, 1, 0.37, 0.02, 1.0)]
# (a record of ordinary numbers, and one whose value is negative zero: oo = -0.0 times a positive term)
RECS = [(0.98, 0.0, 0.63, 0.5, 0.41, 0.77), (0.63, 0.37, 0.98, 1.0, 0.02, -0.0)]


@pytest.mark.parametrize("packed", [0, 1], ids=["all entries", "PACKED"])
@pytest.mark.parametrize("classes", [0, 1], ids=["tot", "CLASSES"])
def test_part_rec_against_the_select_form(shim, classes, packed):
    bits = _all_bits()
    n = len(bits)
    for root in ROOTS:
        for rec in RECS:
            for P in (0, 1):
                for f in (0, 1):
                    got = np.empty((n, 3, 8), np.uint64)
                    cw = np.empty((n, 2), np.uint64)
                    r5, r6 = np.array(root, np.float64), np.array(rec, np.float64)
                    shim.shim_part_rec(classes, packed, P, f, r5.ctypes.data, r6.ctypes.data, bits.ctypes.data, n, UNSET,
                                       got.ctypes.data, cw.ctypes.data)
                    want = _select_form(classes, packed, P, f, root, rec, bits)
                    bad = np.argwhere(got != want)
                    assert bad.size == 0, (root, rec, P, f, hex(int(bits[bad[0][0]])), bad[0], hex(int(got[tuple(bad[0])])),
                                           hex(int(want[tuple(bad[0])])))
                    assert (cw == cw[0]).all(), "the root weights do not depend on the record's bits"
    # the fixture reaches what it is for: kept values, cleared entries, a kept negative zero
    assert (want == np.uint64(0)).any() and (want == np.uint64(0x8000000000000000)).any()
