"""CPU suite of the origin sweep: reading its output (cnf2freq_amd/origins.py), the C ABI's declaration and export, the command
line's option check, and -- on the CPU oracle's store -- the absolute frame of the rows and the grid positions of
origins.with_positions.  The helpers that form the rows from the oracle, and the frame fixture, are shared with the GPU suite
(tests/test_gpu_origins.py)."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT, oracle_ped
from cnf2freq_amd import origins, synth

G = np.arange(64)
ORIGIN_MASK = np.stack([((G & 1) + 2 * ((G >> 3) & 1)) == k for k in range(4)]).astype(np.float64)      # [4][64]
BIT_MASK = np.stack([(G >> t) & 1 for t in range(6)]).astype(np.float64)                                  # [6][64]


def oracle_origins(ped, threads=None):
    """(origin[n][M][4], bits[n][M][6], loglik[n][C], pairs compared) from the oracle's alpha / beta store in numpy: per mode
    gam = fw[s,:,2] * fw[s,:,1] (alpha after the emission x beta) normalised per marker, the modes weighted with
    exp(factors[s] - factor) -- masked modes, modes without a likelihood and modes more than 40 below the total dropped --
    and renormalised, then the masked sums over g.  Zeros where the oracle skips the individual."""
    o = oracle_ped(ped)
    cs = np.asarray(ped.chromstarts)
    n, M, C = len(ped.dous), ped.n_markers, len(cs) - 1
    org, bits = np.zeros((n, M, 4)), np.zeros((n, M, 6))
    ll = np.zeros((n, C))
    ok = np.zeros((n, C), bool)

    def work(j):
        ind = int(ped.dous[j])
        for c in range(C):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            res = o.sweep_ind(ind, int(ped.gen[ind]), first=first, last=last, mode=2, dosage=False, keep_store=True)
            factor = res["factor"]
            ll[j, c] = factor
            if not res["ok"] or not (factor >= -1e15):
                continue
            fw = res["fwbw"]
            sl = slice(first, last + 1)
            gamma = np.zeros((last - first + 1, 64))
            wsum = 0.0
            for s in range(8):
                fs = res["factors"][s]
                if fs < -1e29 or not (fs > -1e14) or factor - fs > 40.0:
                    continue
                gam = fw[s, sl, 2] * fw[s, sl, 1]
                w = np.exp(fs - factor)
                gamma += w * gam / gam.sum(axis=1, keepdims=True)
                wsum += w
            if not wsum > 0:
                continue
            ok[j, c] = True
            gamma /= wsum
            org[j, sl] = gamma @ ORIGIN_MASK.T
            bits[j, sl] = gamma @ BIT_MASK.T

    threads = threads or max(1, min(16, len(os.sched_getaffinity(0)), n))
    with ThreadPoolExecutor(threads) as ex:      # (the oracle's C code is reentrant and ctypes drops the GIL)
        list(ex.map(work, range(n)))
    return org, bits, ll, int(ok.sum())


FRAME_CASES = [(side, order) for side in (0, 1) for order in ((0, 1), (1, 0))]


def frame_ped(side, order):
    """The backcross-like pedigree that shows which way the bits point: the F2 of synth.make_f2(6, 12, 1, seed=7) with the
    F1 parent on `side` (0: par[.][0], 1: par[.][1]) informative -- its own parents listed as `order`, (0, 1) = (A, B) or
    (1, 0) = (B, A) -- and the other F1's parents both record 0 (line A: that side always gives A).  The child's genotype
    is 1/2 where the informative gamete, synth._meiosis(7, 1, ...), carries the B strand and 1/1 elsewhere.
    Returns (pedigree, carries_b[n][M] bool)."""
    ped = synth.make_f2(6, 12, 1, seed=7)
    ped.par, ped.allele, ped.sure = ped.par.copy(), ped.allele.copy(), ped.sure.copy()
    n = len(ped.dous)
    g = synth._meiosis(7, 1, n, ped.pos, ped.chromstarts)
    for i, r in enumerate(ped.dous):
        ped.par[ped.par[r, side]] = order
        ped.par[ped.par[r, 1 - side]] = (0, 0)
        row = ped.row_of[r]
        ped.allele[row, :, 0] = 1
        ped.allele[row, :, 1] = 1 + g[i]
        ped.sure[row] = 0.02
    ped.founder_flags()
    return ped, g.astype(bool)


_FRAME = {}


def frame_oracle(side, order):
    """(pedigree, carries_b, oracle origin, oracle bits), computed once per case and left unchanged"""
    if (side, order) not in _FRAME:
        ped, b = frame_ped(side, order)
        org, bits, _, compared = oracle_origins(ped)
        assert compared == len(ped.dous)
        _FRAME[(side, order)] = (ped, b, org, bits)
    return _FRAME[(side, order)]


# ---------------------------------------------------------------------------------------------- origins.py
def test_line_genotypes_collapses_the_heterozygotes():
    o = np.array([[0.1, 0.2, 0.3, 0.4], [1.0, 0.0, 0.0, 0.0]])
    np.testing.assert_allclose(origins.line_genotypes(o), [[0.1, 0.5, 0.4], [1.0, 0.0, 0.0]], rtol=1e-15)
    assert origins.line_genotypes(np.zeros((3, 5, 4))).shape == (3, 5, 3)


def test_segregation_report_on_hand_made_sums():
    # chromosome [0, 3) with 40 contributors, [3, 4) with none
    s = np.array([[10.0, 10.0, 10.0, 10.0],      # 1:1:1:1
                  [10.0, 14.0, 6.0, 10.0],       # 1:2:1 collapsed, the two heterozygotes unequal
                  [16.0, 8.0, 8.0, 8.0],
                  [0.0, 0.0, 0.0, 0.0]])
    r = origins.segregation_report(s, [40, 0], [0, 3, 4])
    assert list(r["n"]) == [40, 40, 40, 0]
    assert r["chi2_4"][0] == 0.0 and r["chi2_3"][0] == 0.0 and r["p_4"][0] == 1.0 and r["p_3"][0] == 1.0
    assert r["chi2_3"][1] == 0.0                                    # a 1:2:1 table
    np.testing.assert_allclose(r["chi2_4"][1], (16 + 16) / 10.0, rtol=1e-14)
    np.testing.assert_allclose(r["chi2_4"][2], (36 + 4 + 4 + 4) / 10.0, rtol=1e-14)
    np.testing.assert_allclose(r["chi2_3"][2], 36 / 10.0 + 16 / 20.0 + 4 / 10.0, rtol=1e-14)
    np.testing.assert_allclose(r["p_3"][2], np.exp(-r["chi2_3"][2] / 2), rtol=1e-14)
    # 3 d.f.: P(chi2 > 7.814728) = 0.05
    r5 = origins.segregation_report(np.array([[10.0 + np.sqrt(7.814728 * 10 / 2), 10.0 - np.sqrt(7.814728 * 10 / 2), 10.0, 10.0]]), [40], [0, 1])
    np.testing.assert_allclose(r5["p_4"], 0.05, rtol=1e-5)
    np.testing.assert_allclose(r["ratio_first"][:3], [0.5, 0.6, 0.4], rtol=1e-15)
    np.testing.assert_allclose(r["ratio_second"][:3], [0.5, 0.4, 0.4], rtol=1e-15)
    np.testing.assert_allclose(r["collapsed"][1], [10.0, 20.0, 10.0], rtol=1e-15)
    for k in ("expected", "collapsed", "ratio_first", "ratio_second", "chi2_4", "p_4", "chi2_3", "p_3"):
        assert np.isnan(r[k][3]).all(), k
        assert not np.isnan(r[k][:3]).any(), k


def test_information_content():
    # known origins in 1:2:1: a = -1, 0, 0, 1 -> variance 0.5 -> 1; no information: every row (1/4, 1/4, 1/4, 1/4) -> 0
    known = np.zeros((4, 2, 4))
    known[0, :, 0] = known[1, :, 1] = known[2, :, 2] = known[3, :, 3] = 1.0
    np.testing.assert_allclose(origins.information_content(known), [1.0, 1.0], rtol=1e-15)
    assert np.all(origins.information_content(np.full((5, 3, 4), 0.25)) == 0.0)
    # a skipped individual (all-zero rows) is left out
    with_skip = np.concatenate([known, np.zeros((1, 2, 4))])
    np.testing.assert_allclose(origins.information_content(with_skip), [1.0, 1.0], rtol=1e-15)
    assert np.isnan(origins.information_content(np.zeros((2, 1, 4)))).all()


# ---------------------------------------------------------------------------------------------- C ABI
def test_symbols_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi
    hdr = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    L = capi.load()
    for sym, method in (("cnf2_sweep_origins", "sweep_origins"), ("cnf2_origin_rows", "origin_rows")):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        assert sym in capi.SYMBOLS
        assert hasattr(L, sym)
        assert hasattr(capi.Context, method)
    assert hasattr(capi.Context, "sweep_origins_device")
    assert "THE FRAME IS ABSOLUTE" in hdr


# ---------------------------------------------------------------------------------------------- the frame, on the oracle
@pytest.mark.parametrize("side,order", FRAME_CASES)
def test_frame_is_absolute_on_the_oracle(side, order):
    """bit 0 (side 0) / bit 3 (side 1) = 1 means "from the informative parent's par[.][1]": listed (A, B) that is "the child
    carries B", listed (B, A) its opposite; the other side, whose grandparents are one record, sits at 0.5"""
    ped, carries_b, org, bits = frame_oracle(side, order)
    assert carries_b.shape == (6, 13) and 0.2 < carries_b.mean() < 0.8
    t_inf, t_other = (0, 3) if side == 0 else (3, 0)
    agree = ((bits[:, :, t_inf] > 0.5) == carries_b).mean()
    print("side %d, grandparents listed %s: P(bit %d = 1) > 0.5 agrees with 'carries B' in %.3f of %d cells"
          % (side, order, t_inf, agree, carries_b.size))
    if order == (0, 1):
        assert agree >= 0.95
    else:
        assert agree <= 0.05
    assert np.abs(bits[:, :, t_other] - 0.5).max() <= 1e-9
    np.testing.assert_allclose(org.sum(axis=2), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(bits[:, :, 0], org[:, :, 1] + org[:, :, 3], rtol=0, atol=1e-12)
    np.testing.assert_allclose(bits[:, :, 3], org[:, :, 2] + org[:, :, 3], rtol=0, atol=1e-12)


def test_swapping_the_grandparents_flips_the_bit_on_the_oracle():
    for side in (0, 1):
        t = 0 if side == 0 else 3
        a, b = frame_oracle(side, (0, 1))[3], frame_oracle(side, (1, 0))[3]
        np.testing.assert_allclose(a[:, :, t] + b[:, :, t], 1.0, rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------- grid positions
def grid_positions(ped, every=3):
    """a position in the middle of every `every`-th gap of non-zero length, per chromosome"""
    cs = np.asarray(ped.chromstarts)
    out = []
    for c in range(len(cs) - 1):
        p = np.asarray(ped.pos[cs[c]:cs[c + 1]], np.float64)
        mids = [(p[k] + p[k + 1]) / 2 for k in range(0, len(p) - 1, every) if p[k + 1] > p[k]]
        out.append(mids)
    return out


def test_with_positions_on_the_oracle():
    ped = synth.make_outbred3(2, 2, 11, 2, seed=5, random_hw=True, random_sure=True)
    base_o, base_b, _, compared = oracle_origins(ped)
    assert compared == len(ped.dous) * 2
    add = grid_positions(ped)
    assert sum(len(a) for a in add) >= 5
    ped2, is_marker = origins.with_positions(ped, add)
    assert ped2.n_markers == ped.n_markers + sum(len(a) for a in add) and is_marker.sum() == ped.n_markers
    assert list(ped2.chromstarts) == [0, 12 + len(add[0]), 24 + len(add[0]) + len(add[1])]
    assert np.all(np.diff(ped2.pos[:ped2.chromstarts[1]]) >= 0)
    np.testing.assert_array_equal(ped2.pos[is_marker], ped.pos)
    np.testing.assert_array_equal(ped2.allele[:, is_marker], ped.allele)
    assert not ped2.allele[:, ~is_marker].any() and not ped2.sure[:, ~is_marker].any() and np.all(ped2.hw[:, ~is_marker] == 0.5)
    assert ped.n_markers == 24 and ped.allele.shape[1] == 24, "the input is left as it was"
    o2, b2, _, _ = oracle_origins(ped2)
    print("rows at the real markers move by %.3g" % max(np.abs(o2[:, is_marker] - base_o).max(), np.abs(b2[:, is_marker] - base_b).max()))
    np.testing.assert_allclose(o2[:, is_marker], base_o, rtol=0, atol=1e-9)
    np.testing.assert_allclose(b2[:, is_marker], base_b, rtol=0, atol=1e-9)
    np.testing.assert_allclose(o2[:, ~is_marker].sum(axis=2), 1.0, rtol=0, atol=1e-12)
    assert np.all(o2[:, ~is_marker] >= -1e-15)


def test_with_positions_refusals():
    ped = synth.make_f2(3, 5, 2, seed=3)
    cs = ped.chromstarts
    lo, hi = ped.pos[cs[1]], ped.pos[cs[2] - 1]
    origins.with_positions(ped, [[], [(lo + hi) / 2]])
    for bad in ([[], [lo - 1.0]], [[], [hi + 0.5]], [[ped.pos[2]], []], [[1.5, 1.5], []], [[1.0]], [[float("nan")], []]):
        with pytest.raises(ValueError):
            origins.with_positions(ped, bad)


# ---------------------------------------------------------------------------------------------- command line
EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def test_cli_origins_refuses_two_gpus(tmp_path):
    import __graft_entry__ as g
    g.build()
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", "--gpus", "2", "--origins", "o.txt"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2
    assert "single GPU" in r.stderr and "--origins" in r.stderr
    assert not (tmp_path / "o.txt").exists()


def test_run_from_files_refuses_a_file_it_cannot_read(tmp_path):
    """host.Run.from_files reads before it opens a device: a missing genotype file is an error, not an empty run"""
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host
    paths = [os.path.join(DEMO, "demoplantimpute." + e) for e in ("map", "ped")] + [str(tmp_path / "none.gen")]
    with pytest.raises(RuntimeError, match="cannot read .*none.gen"):
        host.Run.from_files(*paths)
