"""CPU suite of the descent rows (cnf2_sweep_descent): reading them (origins.DESCENT_MASK, descent_columns, descent_calls), the
host library's twin of the column map, the fixture synth.make_founder_cross, the C ABI's declaration and export, the command
line's option check, and -- on the CPU oracle's store (tests/descent_reference.py) -- the identities with the origin rows,
the labelling of the strands by the grandparent's hw and the planted truth."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import origins, synth
from descent_reference import FOUNDER_ARGS, check_identities, founder_cross, oracle_descent, truth_shares
from test_origins_host import oracle_origins


# ---------------------------------------------------------------------------------------------- origins.py
def test_descent_mask_partitions_the_states_per_side():
    m = origins.DESCENT_MASK
    assert m.shape == (8, 64) and m.dtype == bool
    assert np.all(m[:4].sum(axis=0) == 1) and np.all(m[4:].sum(axis=0) == 1)
    assert np.all(m.sum(axis=1) == 16)
    g = np.arange(64)
    bit = lambda t: (g >> t) & 1
    # class 2 w + b: w the parent's own meiosis, b the meiosis of the grandparent it selected
    for k in range(4):
        w, b = k >> 1, k & 1
        assert np.array_equal(m[k], (bit(0) == w) & (np.where(w == 1, bit(2), bit(1)) == b))
        assert np.array_equal(m[4 + k], (bit(3) == w) & (np.where(w == 1, bit(5), bit(4)) == b))


def test_descent_calls():
    d = np.array([[0.1, 0.6, 0.2, 0.1, 0.25, 0.25, 0.25, 0.25], [0.0] * 8, [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.7, 0.3]])
    cls, prob = origins.descent_calls(d)
    assert cls.tolist() == [[1, 0], [-1, -1], [3, 2]]
    np.testing.assert_allclose(prob, [[0.6, 0.25], [0.0, 0.0], [1.0, 0.7]], rtol=1e-15)
    assert origins.descent_calls(np.zeros((2, 3, 8)))[0].shape == (2, 3, 2)


def hand_columns(par, dous, by):
    """the column map, slot by slot"""
    gps = set()
    for i in dous:
        for s in range(2):
            p = par[i][s]
            if p >= 0 and par[p][0] >= 0 and par[p][1] >= 0:
                gps.update(int(v) for v in par[p])
    grand = sorted(gps)
    col = np.full((len(dous), 8), -1, np.int32)
    for j, i in enumerate(dous):
        for s in range(2):
            p = par[i][s]
            if p < 0 or par[p][0] < 0 or par[p][1] < 0:
                continue
            for w in range(2):
                g = grand.index(int(par[p][w]))
                for b in range(2):
                    col[j, 4 * s + 2 * w + b] = {"haplotype": 2 * g + b, "founder": g, "line": w}[by]
    return col, grand


def column_pedigrees():
    out = {}
    ped = synth.make_outbred3(3, 4, 5, 1, seed=3)
    out["outbred3"] = (ped.par, ped.dous)
    # a sire (record 4, parents 0 1) with two dams (5: parents 2 3; 6: no recorded parents); children 7..10
    par = np.full((11, 2), -1, np.int32)
    par[4], par[5] = (0, 1), (2, 3)
    par[7], par[8], par[9], par[10] = (4, 5), (4, 5), (4, 6), (6, 4)
    out["sire_two_dams"] = (par, np.array([7, 8, 9, 10], np.int32))
    f2 = synth.make_f2(3, 4, 1, seed=1)
    out["f2"] = (f2.par, f2.dous)
    return out


@pytest.mark.parametrize("by", ["haplotype", "founder", "line"])
def test_descent_columns(by):
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host
    for name, (par, dous) in column_pedigrees().items():
        want, grand = hand_columns(par, dous, by)
        col, got_grand = origins.descent_columns(par, dous, by)
        assert col.dtype == np.int32 and np.array_equal(col, want), name
        assert got_grand.tolist() == grand, name
        hcol, G = host.descent_columns(par, dous, by)
        assert np.array_equal(hcol, want) and G == len(grand), name
    par, dous = column_pedigrees()["sire_two_dams"]
    col, grand = origins.descent_columns(par, dous, by)
    assert grand.tolist() == [0, 1, 2, 3]
    assert np.all(col[2, 4:] == -1) and np.all(col[2, :4] >= 0), "the dam without recorded parents: -1 on her side only"
    assert np.all(col[3, :4] == -1) and np.all(col[3, 4:] >= 0)
    if by == "haplotype":
        assert col[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and col[3, 4:].tolist() == [0, 1, 2, 3]
    if by == "founder":
        assert col[0].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    if by == "line":
        assert col[0].tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    # three families of make_outbred3: twelve grandparents, H = 24 haplotype columns
    par, dous = column_pedigrees()["outbred3"]
    col, grand = origins.descent_columns(par, dous, by)
    assert len(grand) == 12 and col.max() == {"haplotype": 23, "founder": 11, "line": 1}[by] and col.min() == 0


def test_descent_columns_refusals():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host
    par, dous = column_pedigrees()["sire_two_dams"]
    with pytest.raises(ValueError):
        origins.descent_columns(par, dous, "strand")
    L = host.load()
    p = lambda a: a.ctypes.data
    col, G = np.full((len(dous), 8), 7, np.int32), np.full(1, 7, np.int32)
    par32, dous32 = np.ascontiguousarray(par, np.int32), np.ascontiguousarray(dous, np.int32)
    bad_par = par32.copy()
    bad_par[4, 0] = 11
    bad_dous = dous32.copy()
    bad_dous[1] = 11
    calls = [(0, p(par32), 4, p(dous32), 0, p(col), p(G)), (11, None, 4, p(dous32), 0, p(col), p(G)),
             (11, p(par32), 0, p(dous32), 0, p(col), p(G)), (11, p(par32), 4, None, 0, p(col), p(G)),
             (11, p(par32), 4, p(dous32), 3, p(col), p(G)), (11, p(par32), 4, p(dous32), -1, p(col), p(G)),
             (11, p(par32), 4, p(dous32), 0, None, p(G)), (11, p(par32), 4, p(dous32), 0, p(col), None),
             (11, p(bad_par), 4, p(dous32), 0, p(col), p(G)), (11, p(par32), 4, p(bad_dous), 0, p(col), p(G))]
    for args in calls:
        assert L.cnf2h_descent_columns(*args) == -2
        assert np.all(col == 7) and np.all(G == 7)


# ---------------------------------------------------------------------------------------------- the fixture
def test_make_founder_cross():
    ped, truth = synth.make_founder_cross(*FOUNDER_ARGS)
    n_fam, kids, mpc, n_chrom = FOUNDER_ARGS[:4]
    per = 6 + kids
    assert len(ped.dous) == n_fam * kids and ped.n_markers == n_chrom * (mpc + 1)
    assert truth.shape == (n_fam * kids, 2, ped.n_markers) and truth.dtype == np.uint8 and truth.max() == 3
    for f in range(n_fam):
        assert ped.par[f * per + 4].tolist() == [0, 1] and ped.par[f * per + 5].tolist() == [2, 3]
    col, grand = origins.descent_columns(ped.par, ped.dous)
    assert grand.tolist() == [0, 1, 2, 3] and np.all(col == np.arange(8))
    # the grandparents' hw says which strand carries the first stored allele; everybody else's is 0.5
    hw = ped.hw[ped.row_of]
    assert set(np.unique(hw[:4])) <= {1.0 - 0.98, 0.5, 0.98} and (hw[:4] == 0.98).any() and (hw[:4] == 1.0 - 0.98).any()
    assert np.all(hw[4:] == 0.5)
    flipped, t2 = synth.make_founder_cross(*FOUNDER_ARGS[:6], 0.02)
    assert np.array_equal(t2, truth) and np.array_equal(flipped.allele, ped.allele)
    np.testing.assert_allclose(flipped.hw, 1.0 - ped.hw, rtol=0, atol=1e-15)
    # the same law and streams as make_outbred3: family 0 is that generator's family 0 up to the phase
    base = synth.make_outbred3(*FOUNDER_ARGS[:6])
    assert np.array_equal(base.allele[:1 + 6], ped.allele[:1 + 6]) and np.array_equal(base.pos, ped.pos)
    # each side of the truth follows one strand between crossovers
    changes = (np.diff(truth[:, :, :mpc + 1].astype(int), axis=2) != 0).mean()
    assert 0.0 < changes < 0.3


# ---------------------------------------------------------------------------------------------- C ABI
def test_symbols_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi, host
    hdr = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    L = capi.load()
    for sym, method in (("cnf2_sweep_descent", "sweep_descent"), ("cnf2_descent_rows", "descent_rows")):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        assert sym in capi.SYMBOLS
        assert hasattr(L, sym)
        assert hasattr(capi.Context, method)
    assert hasattr(capi.Context, "sweep_descent_device")
    assert "THE STRAND IS LABELLED BY THE GRANDPARENT'S OWN RECORD" in hdr
    hhdr = open(os.path.join(ROOT, "include", "cnf2host.h")).read()
    assert re.search(r"\bint\s+cnf2h_descent_columns\s*\(", hhdr) and "cnf2h_descent_columns" in host.SYMBOLS
    assert hasattr(host.load(), "cnf2h_descent_columns")


# ---------------------------------------------------------------------------------------------- on the oracle
def test_identities_with_the_origin_rows_on_the_oracle():
    ped, _, ref = founder_cross()
    assert ref["compared"] == len(ped.dous) * 2
    org, bits, _, compared = oracle_origins(ped)
    assert compared == ref["compared"]
    check_identities(ref["descent"], bits)
    d = ref["descent"]
    np.testing.assert_allclose(d[:, :, 0] + d[:, :, 1] + d[:, :, 4] + d[:, :, 5] - 1.0, org[:, :, 0] - org[:, :, 3], rtol=0, atol=1e-12)
    # an outbred pedigree with grandparents of every family's own, random hw
    ped = synth.make_outbred3(3, 12, 17, 2, seed=777, random_hw=True)
    ref = oracle_descent(ped)
    assert ref["compared"] == len(ped.dous) * 2
    check_identities(ref["descent"], oracle_origins(ped)[1])


def test_hw_labels_the_strands_on_the_oracle():
    """hw and 1 - hw of one grandparent exchanged along a chromosome: its two strand cells change places there, and nothing
    else moves"""
    ped, _, ref = founder_cross()
    cs = ped.chromstarts
    base = ref["descent"]
    for g, chrom in ((1, 0), (2, 1)):
        other, _ = synth.make_founder_cross(*FOUNDER_ARGS)
        sl = slice(int(cs[chrom]), int(cs[chrom + 1]))
        other.hw[other.row_of[g], sl] = 1.0 - other.hw[other.row_of[g], sl]
        got = oracle_descent(other)["descent"]
        side, w = g >> 1, g & 1                  # grandparent g is par[parent `side`][w] of every child
        lo = 4 * side + 2 * w
        want = base.copy()
        want[:, sl, lo], want[:, sl, lo + 1] = base[:, sl, lo + 1], base[:, sl, lo]
        moved = np.abs(base[:, sl, lo] - base[:, sl, lo + 1]).max()
        print("grandparent %d, chromosome %d: largest difference %.3g; the cells differ by up to %.3g" % (g, chrom, np.abs(got - want).max(), moved))
        assert moved > 0.5, "the fixture should tell the strands apart"
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


def test_planted_truth_on_the_oracle():
    ped, truth, ref = founder_cross()
    shares = truth_shares(ref["descent"], truth)
    print("arg-max class is the true (grandparent, strand) in %.3f / %.3f of the cells of the two sides" % tuple(shares))
    assert min(shares) >= 0.8
    # with the phase the other way round the strands take each other's names
    flipped, t2 = synth.make_founder_cross(*FOUNDER_ARGS[:6], 0.02)
    other = truth_shares(oracle_descent(flipped)["descent"], t2 ^ 1)
    assert min(other) >= 0.8
    # the origin classes alone name the grandparent, never the strand
    grandparent_only = [float(((ref["descent"][:, :, 4 * s + 2:4 * s + 4].sum(axis=2) > 0.5) == (truth[:, s] >> 1)).mean()) for s in range(2)]
    assert min(grandparent_only) >= min(shares)


# ---------------------------------------------------------------------------------------------- command line
EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def test_cli_descent_refuses_two_gpus(tmp_path):
    import __graft_entry__ as g
    g.build()
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", "--gpus", "2", "--descent", "d.txt"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2
    assert "single GPU" in r.stderr and "--descent" in r.stderr
    assert not (tmp_path / "d.txt").exists()
