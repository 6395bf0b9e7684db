"""CPU suite of the pair sweep (cnf2_sweep_pairs): its yardstick (tests/pairs_reference.py) on the CPU oracle's store -- the
margins are the origin rows, adjacent loci give the crossover posteriors, and the joint is far from the product of its
margins --, reading the output (cnf2freq_amd/origins.py), the C ABI's declaration and export, and the command line's
option check."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import origins
from pairs_reference import linked, margins, oracle_pairs_of, recombinant_mass
from test_gpu_crossovers import oracle_xi_all
from test_origins_host import oracle_origins

CASES = ["f2_implicit_f1", "outbred3_missing", "ail_ties", "outbred3_two_chrom"]


@pytest.mark.parametrize("case", CASES)
def test_yardstick_margins_and_crossovers(case):
    ped, joint, pairs, compared = oracle_pairs_of(case)
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    assert compared == n * C, "no individual of these fixtures is skipped"
    assert len(pairs) == sum(k * (k - 1) // 2 for k in np.diff(ped.chromstarts))
    first, second = margins(joint)
    # a product of the margins would be wrong, not approximate: the test below would catch it
    product = (first[..., :, None] * second[..., None, :]).reshape(joint.shape)
    gap = np.abs(joint - product).max()
    print("%s: %d pairs; the joint differs from the product of its margins by up to %.3f" % (case, len(pairs), gap))
    assert gap > 0.2
    np.testing.assert_allclose(joint.sum(axis=2), 1.0, rtol=0, atol=1e-12)
    assert joint.min() >= 0.0
    org = oracle_origins(ped)[0]
    e1, e2 = np.abs(first - org[:, pairs[:, 0]]).max(), np.abs(second - org[:, pairs[:, 1]]).max()
    print("margins against oracle_origins: %.3g, %.3g" % (e1, e2))
    assert e1 <= 1e-12 and e2 <= 1e-12
    xi = oracle_xi_all(ped)
    adj = np.flatnonzero(pairs[:, 1] == pairs[:, 0] + 1)
    assert len(adj) == M - C
    r0, r3 = recombinant_mass(joint[:, adj])
    e0, e3 = np.abs(r0 - xi[:, pairs[adj, 0], 0]).max(), np.abs(r3 - xi[:, pairs[adj, 0], 3]).max()
    print("adjacent pairs against oracle_xi: %.3g, %.3g" % (e0, e3))
    assert e0 <= 1e-12 and e3 <= 1e-12


def test_linked_pairs():
    cs = [0, 4, 5, 9]
    p = origins.linked_pairs([0, 2, 3, 4, 6, 8], cs)
    assert p.dtype == np.int32
    assert p.tolist() == [[0, 1], [0, 2], [1, 2], [4, 5]]
    assert p.tolist() == [list(x) for x in linked([0, 2, 3, 4, 6, 8], cs)]
    assert origins.linked_pairs([1, 4, 7], cs).shape == (0, 2)
    assert origins.linked_pairs(np.arange(9), cs).shape == (6 + 0 + 6, 2)
    for bad in ([2, 1], [1, 1], [-1, 2], [0, 9]):
        with pytest.raises(ValueError):
            origins.linked_pairs(bad, cs)


def test_pair_recombination_on_hand_made_sums():
    cs, sel = [0, 3, 5], [0, 2, 3, 4]
    pairs = origins.linked_pairs(sel, cs)
    assert pairs.tolist() == [[0, 1], [2, 3]]
    s = np.zeros((2, 16))
    # pair 0, 10 contributors: 6 stay in class 0, 2 move 0 -> 1 (first side), 1 moves 0 -> 2 (second side), 1 moves 0 -> 3 (both)
    s[0, [0, 1, 2, 3]] = [6.0, 2.0, 1.0, 1.0]
    # pair 1: no contributors
    r = origins.pair_recombination(s, [10, 0], pairs, sel, cs)
    assert r["marker1"].tolist() == [0, 3] and r["marker2"].tolist() == [2, 4] and r["chrom"].tolist() == [0, 1]
    assert r["n"].tolist() == [10, 0]
    np.testing.assert_allclose(r["first"][0], 0.3, rtol=1e-15)
    np.testing.assert_allclose(r["second"][0], 0.2, rtol=1e-15)
    np.testing.assert_allclose(r["table"][0, 0], [0.6, 0.2, 0.1, 0.1], rtol=1e-15)
    assert np.isnan(r["first"][1]) and np.isnan(r["second"][1]) and np.isnan(r["table"][1]).all()
    # a diagonal table: nothing recombines
    d = np.zeros((1, 16))
    d[0, [0, 5, 10, 15]] = 1.0
    r = origins.pair_recombination(d, [4], [[0, 1]], [0, 1], [0, 2])
    assert r["first"][0] == 0.0 and r["second"][0] == 0.0
    with pytest.raises(ValueError):
        origins.pair_recombination(s, [10, 0], [[1, 2], [2, 3]], sel, cs)      # markers 2 and 3 lie on two chromosomes
    with pytest.raises(ValueError):
        origins.pair_recombination(s[:1], [10, 0], pairs, sel, cs)


def test_symbols_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi, host
    hdr = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    L = capi.load()
    for sym, method in (("cnf2_sweep_pairs", "sweep_pairs"), ("cnf2_pair_rows", "pair_rows"), ("cnf2_linked_pairs", "linked_pairs"),
                        ("cnf2_qtl_scan2_linked", "qtl_scan2_linked")):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        assert sym in capi.SYMBOLS
        assert hasattr(L, sym)
        assert hasattr(capi.Context, method)
    assert hasattr(capi.Context, "sweep_pairs_device") and hasattr(capi.Context, "qtl_scan2_linked_device")
    assert "CNF2_QTL_JOINT_DEVICE" in hdr
    hh = open(os.path.join(ROOT, "include", "cnf2host.h")).read()
    assert re.search(r"\bint\s+cnf2h_qtl2_pair_linked\s*\(", hh) and "cnf2h_qtl2_pair_linked" in host.SYMBOLS
    assert hasattr(host.load(), "cnf2h_qtl2_pair_linked")


EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def test_cli_qtl2_linked_needs_qtl2(tmp_path):
    import __graft_entry__ as g
    g.build()
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", "--qtl2-linked"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2
    assert "--qtl2-linked" in r.stderr and "--qtl2 FILE" in r.stderr
