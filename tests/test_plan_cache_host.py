"""CPU suite: the key of the plan a context keeps across sweeps (cnf2_plan.h PlanKey, plan_key_same_jobs, plan_key_same).

A sweep takes the kept job list, groups and device copies as they stand only if everything they depend on is unchanged: each
field of the key must break the equality on its own, the fields that only the pairing into eights reads must leave the job list's
equality alone, and of the flags word exactly the flags that route windows count."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ["windows_gen", "map_gen", "ind_begin", "n", "flags", "uniform_mode", "n_lines", "lines_cap", "lines_fit", "pack_cap",
          "reserve_blocks", "uni_blocks_per_cu"]
PAIRING_ONLY = {"pack_cap", "reserve_blocks", "uni_blocks_per_cu"}      # read by pair_uniform_groups alone


@pytest.fixture(scope="module")
def shim():
    shim_dir = os.path.join(ROOT, "tests", "shim")
    so = os.path.join(shim_dir, "libcnf2plankey.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-I" + os.path.join(ROOT, "cnf2freq_amd", "csrc"),
                           "-o", so, os.path.join(shim_dir, "plan_key_shim.cpp")])
    lib = C.CDLL(so)
    lib.shim_plan_key_compare.argtypes = [C.c_void_p, C.c_void_p]
    lib.shim_plan_key_flags.restype = C.c_uint32
    assert lib.shim_plan_key_fields() == len(FIELDS)
    return lib


def _key(**kw):
    from cnf2freq_amd import capi
    base = dict(windows_gen=3, map_gen=1, ind_begin=0, n=21, flags=capi.NO_TIES, uniform_mode=1, n_lines=2, lines_cap=1 << 30,
                lines_fit=1 << 30, pack_cap=6, reserve_blocks=0, uni_blocks_per_cu=3)
    base.update(kw)
    return np.array([base[f] for f in FIELDS], np.int64)


def _cmp(shim, a, b):
    r = shim.shim_plan_key_compare(a.ctypes.data, b.ctypes.data)
    return bool(r & 1), bool(r & 2)


def test_equal_keys(shim):
    assert _cmp(shim, _key(), _key()) == (True, True)


@pytest.mark.parametrize("field", FIELDS)
def test_every_field_counts(shim, field):
    a = _key()
    b = a.copy()
    b[FIELDS.index(field)] += 1 if field != "flags" else 0
    if field == "flags":
        from cnf2freq_amd import capi
        b[FIELDS.index("flags")] ^= capi.NO_UNIFORM_PACK
    jobs, whole = _cmp(shim, a, b)
    assert not whole, field
    assert jobs == (field in PAIRING_ONLY), field
    assert _cmp(shim, b, a) == (jobs, whole)


def test_the_flags_that_enter_the_plan(shim):
    from cnf2freq_amd import capi
    routing = {"NO_TIES": capi.NO_TIES, "FULL_SPILL": capi.FULL_SPILL, "MERGE_MODES": capi.MERGE_MODES, "XPOSE": capi.XPOSE,
               "FLUSH_TINY": capi.FLUSH_TINY, "ALL_STATES": capi.ALL_STATES, "NO_LINE_RECORDS": capi.NO_LINE_RECORDS,
               "NO_UNIFORM_PACK": capi.NO_UNIFORM_PACK, "NO_UNIFORM_PACK8": capi.NO_UNIFORM_PACK8}
    mask = 0
    for v in routing.values():
        mask |= v
    assert shim.shim_plan_key_flags() == mask
    a = _key(flags=0)
    for name, bit in routing.items():
        jobs, whole = _cmp(shim, a, _key(flags=bit))
        assert not whole, name
        assert jobs == (name == "NO_UNIFORM_PACK8"), name          # the eights' switch leaves the list and the fours alone
    # flags that change what a sweep writes or how its waves take jobs, not which lists it sweeps
    for name in ("OUT_DEVICE", "NO_DOSAGE", "RAW_DOSAGE", "LOG_PATHS", "TIES_GENERAL", "STATIC_JOBS"):
        assert _cmp(shim, a, _key(flags=getattr(capi, name))) == (True, True), name
