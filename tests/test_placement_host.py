"""CPU suite of the marker placement: reading the profile (cnf2freq_amd/placement.py), the C ABI's declaration and export,
and the command line's option checks."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import placement

LN10 = np.log(10.0)


def profile(lod, null=None):
    """place_sum and null that give the LOD profile `lod`"""
    lod = np.asarray(lod, np.float64)
    null = np.full(lod.shape[0], -3.0) if null is None else np.asarray(null, np.float64)
    return lod * LN10 + null[:, None], null


def test_peak_among_the_fewest_impossible():
    # the highest LOD (marker 2) has an impossible individual; among the markers with none, marker 5 wins
    lod = [[0.0, 1.0, 9.0, 2.0, 3.0, 4.0, 1.0, 0.5]]
    nz = np.array([[0, 0, 1, 0, 0, 0, 0, 2]], np.int32)
    ps, null = profile(lod)
    b = placement.best_positions(ps, nz, null, np.arange(8) * 2.0, [0, 8])
    assert b["marker"][0] == 5 and b["chrom"][0] == 0 and b["pos"][0] == 10.0 and b["n_zero"][0] == 0
    assert b["lod"][0] == pytest.approx(4.0)
    # within 1 LOD of 4.0 and eligible: markers 4 and 5 (3 is 2.0 below, 6 is 3.0 below)
    assert (b["support_lo_marker"][0], b["support_hi_marker"][0]) == (4, 5)
    assert (b["support_lo"][0], b["support_hi"][0]) == (8.0, 10.0)
    assert b["other_lod"][0] == -np.inf
    # every marker has impossible individuals: the fewest (1) are eligible
    nz2 = np.array([[3, 1, 1, 2, 5, 5, 5, 5]], np.int32)
    b = placement.best_positions(ps, nz2, null, np.arange(8) * 2.0, [0, 8])
    assert b["marker"][0] == 2 and b["n_zero"][0] == 1
    assert (b["support_lo_marker"][0], b["support_hi_marker"][0]) == (2, 2)      # marker 1 is 8 LOD below
    # ties: the first of equals
    ps, null = profile([[1.0, 5.0, 5.0, 0.0]])
    b = placement.best_positions(ps, np.zeros((1, 4), np.int32), null, np.arange(4.0), [0, 4])
    assert b["marker"][0] == 1 and (b["support_lo_marker"][0], b["support_hi_marker"][0]) == (1, 2)


def test_support_interval_stops_at_chromosome_ends_and_other_chromosome_lod():
    # two chromosomes [0, 4) and [4, 9); candidate 0 peaks at the first marker of the second, candidate 1 at the last of the first
    lod = [[2.5, 2.6, 2.7, 2.9, 3.0, 2.8, 2.5, 1.0, 0.0],
           [0.0, 5.0, 5.5, 6.0, 5.9, 5.8, 1.0, 1.0, 1.0]]
    ps, null = profile(lod, [-1.0, -20.0])
    pos = np.array([0, 5, 10, 15, 0, 4, 8, 12, 16], np.float64)
    b = placement.best_positions(ps, np.zeros((2, 9), np.int32), null, pos, [0, 4, 9])
    assert list(b["marker"]) == [4, 3] and list(b["chrom"]) == [1, 0]
    assert (b["support_lo_marker"][0], b["support_hi_marker"][0]) == (4, 6)     # does not run back into chromosome 0
    assert (b["support_lo_marker"][1], b["support_hi_marker"][1]) == (1, 3)     # does not run on into chromosome 1
    assert (b["support_lo"][1], b["support_hi"][1]) == (5.0, 15.0)
    assert b["other_lod"][0] == pytest.approx(2.9) and b["other_lod"][1] == pytest.approx(5.9)
    np.testing.assert_allclose(placement.lod_profile(ps, null), lod, rtol=1e-12, atol=1e-12)
    # a wider drop widens the interval
    b = placement.best_positions(ps, np.zeros((2, 9), np.int32), null, pos, [0, 4, 9], drop=2.5)
    assert (b["support_lo_marker"][0], b["support_hi_marker"][0]) == (4, 7)
    # the other chromosome's markers count only where they are eligible
    nz = np.zeros((2, 9), np.int32)
    nz[1, 4:] = 1
    b = placement.best_positions(ps, nz, null, pos, [0, 4, 9])
    assert b["other_lod"][1] == -np.inf


def test_symbol_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi
    hdr = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    assert re.search(r"\bint\s+cnf2_sweep_place\s*\(", hdr)
    assert "cnf2_sweep_place" in capi.SYMBOLS
    L = capi.load()
    assert hasattr(L, "cnf2_sweep_place")
    assert hasattr(capi.Context, "sweep_place")


EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def run_cli(tmp_path, *extra):
    import __graft_entry__ as g
    g.build()
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))


@pytest.mark.parametrize("extra", [("--place", "p.txt"), ("--place", "p.txt", "--place-genfile", "g.gen"),
                                   ("--place", "p.txt", "--place-markers", "3"),
                                   ("--place-genfile", "g.gen", "--place-markers", "3")])
def test_cli_place_needs_its_companions(tmp_path, extra):
    r = run_cli(tmp_path, *extra)
    assert r.returncode == 2
    assert "go together" in r.stderr
    assert not (tmp_path / "p.txt").exists()


def test_cli_place_refuses_two_gpus(tmp_path):
    r = run_cli(tmp_path, "--gpus", "2", "--place", "p.txt", "--place-genfile", "g.gen", "--place-markers", "3")
    assert r.returncode == 2
    assert "single GPU" in r.stderr
