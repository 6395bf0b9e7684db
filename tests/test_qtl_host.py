"""CPU suite of the QTL scan's host side: the permutations of cnf2freq_amd/qtl.py and their twin in the host library, the
null-model residuals, thresholds and peaks on hand-made profiles, the symbols, and the command line's usage errors.  The scan
itself needs a GPU (tests/test_gpu_qtl.py)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import qtl, synth

EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    return h


# ---------------------------------------------------------------------------------------------- permutations
def test_permutations_are_permutations_that_respect_use_and_strata():
    n, P = 23, 7
    use = np.ones(n, bool)
    use[[2, 9, 22]] = False
    strata = np.arange(n) % 3
    perm = qtl.permutations(n, P, 5, use=use, strata=strata)
    assert perm.shape == (P, n) and perm.dtype == np.int32
    for row in perm:
        assert np.array_equal(np.sort(row), np.arange(n))
        assert np.array_equal(row[~use], np.flatnonzero(~use)), "unused individuals map to themselves"
        assert use[row[use]].all(), "used stays used"
        assert np.array_equal(strata[row], strata), "strata are kept"
    assert len({row.tobytes() for row in perm}) == P, "p gives distinct rows"
    assert not np.array_equal(perm, qtl.permutations(n, P, 6, use=use, strata=strata)), "the seed matters"
    assert np.array_equal(perm, qtl.permutations(n, P, 5, use=use, strata=strata))
    # the rule, spelled out for one row without strata
    row = qtl.permutations(n, 3, 11)[2]
    keys = synth.splitmix64(11, 2 * n + np.arange(n))
    assert np.array_equal(row, np.argsort(keys, kind="stable"))
    assert qtl.permutations(4, 0, 1).shape == (0, 4)
    assert np.array_equal(qtl.permutations(3, 2, 1, use=np.zeros(3)), [[0, 1, 2]] * 2)


def test_permutations_equal_the_host_library(host):
    for n, P, seed, masked, strat in ((1, 2, 0, False, False), (17, 5, 3, True, False), (64, 9, 2 ** 63 + 5, True, True),
                                      (200, 3, 7, False, True)):
        use = None
        if masked:
            use = synth.uniform(seed % 1000, np.arange(n)) < 0.8
        strata = (np.arange(n) * 7) % 4 if strat else None
        want = qtl.permutations(n, P, seed, use=use, strata=strata)
        got = host.qtl_permutations(n, P, seed, use=use, strata=strata)
        assert np.array_equal(got, want), (n, P, seed)


# ---------------------------------------------------------------------------------------------- residuals
def test_null_residuals_against_lstsq(host):
    n, T, K = 31, 3, 2
    y = synth.uniform(1, np.arange(n * T)).reshape(n, T) * 3.0 + 10.0
    cov = synth.uniform(2, np.arange(n * K)).reshape(n, K)
    use = np.ones(n, bool)
    use[[0, 7]] = False
    y[0] = np.nan
    X = np.concatenate([np.ones((n, 1)), cov], axis=1)[use]
    want = np.zeros((n, T))
    want[use] = y[use] - X @ np.linalg.lstsq(X, y[use], rcond=None)[0]
    got = qtl.null_residuals(y, cov, use)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    assert np.all(got[~use] == 0.0)
    np.testing.assert_allclose(X.T @ got[use], 0.0, atol=1e-12)                       # orthogonal to the null design
    np.testing.assert_allclose(host.qtl_null_residuals(np.where(use[:, None], y, 0.0), cov, use), want, rtol=0, atol=1e-12)
    # without covariates: the deviations from the mean of the used
    np.testing.assert_allclose(qtl.null_residuals(y[:, 0], None, use)[use, 0], y[use, 0] - y[use, 0].mean(), atol=1e-13)
    np.testing.assert_allclose(host.qtl_null_residuals(np.where(use, y[:, 0], 0.0), None, use)[use, 0],
                               y[use, 0] - y[use, 0].mean(), atol=1e-13)


# ---------------------------------------------------------------------------------------------- thresholds, peaks
def test_thresholds_on_hand_made_maxima():
    P, T, C = 100, 2, 3
    pm = np.zeros((P, T, C))
    pm[:, 0, 0] = np.arange(P)                      # trait 0: the maxima are 0 .. 99 on chromosome 0
    pm[:, 0, 1] = np.arange(P)[::-1] / 2.0          #          and 49.5 .. 0 on chromosome 1
    pm[:, 1, 2] = 1.0
    thr = qtl.thresholds(pm)
    assert thr["alpha"] == (0.05, 0.01)
    # genome-wide: max(p, (99 - p) / 2) over p: sorted, the 95th and 99th order statistics
    genome0 = np.sort(np.maximum(np.arange(P), np.arange(P)[::-1] / 2.0))
    assert thr["genome"].shape == (2, T) and list(thr["genome"][:, 0]) == [genome0[94], genome0[98]]
    assert list(thr["genome"][:, 1]) == [1.0, 1.0]
    assert thr["chromosome"].shape == (2, T, C) and list(thr["chromosome"][:, 0, 0]) == [94.0, 98.0]
    assert list(thr["chromosome"][:, 0, 1]) == [47.0, 49.0] and np.all(thr["chromosome"][:, 0, 2] == 0.0)
    assert (pm.max(axis=2)[:, 0] > thr["genome"][0, 0]).sum() <= 0.05 * P         # at most alpha P maxima exceed a threshold
    assert qtl.thresholds(pm[:1])["genome"].shape == (2, T)
    with pytest.raises(ValueError):
        qtl.thresholds(np.zeros((0, 1, 1)))


def test_peaks_on_hand_made_profiles():
    cs = [0, 5, 9, 12]
    pos = np.array([0, 10, 20, 30, 40, 0, 5, 10, 15, 0, 1, 2], np.float64)
    lod = np.array([[0.5, 2.0, 4.0, 2.6, 0.1,       # a peak inside chromosome 0: interval markers 2 .. 3
                     0.2, 1.0, 2.9, 2.0,            # nothing above the threshold
                     1.0, 3.2, 5.0],                # the peak at the end of chromosome 2
                    [0.0] * 12])
    coef = np.zeros((2, 12, 2))
    coef[0, 2], coef[0, 11] = (0.7, -0.1), (np.nan, 0.3)
    found = qtl.peaks(lod, pos, cs, 3.0, coef=coef)
    assert [(p["trait"], p["chrom"], p["marker"]) for p in found] == [(0, 0, 2), (0, 2, 11)]
    a, b = found
    assert (a["lod"], a["lo"], a["hi"], a["pos_lo"], a["pos_hi"], a["additive"], a["dominance"]) == (4.0, 2, 3, 20.0, 30.0, 0.7, -0.1)
    assert (b["lod"], b["lo"], b["hi"], b["pos"], b["pos_hi"]) == (5.0, 11, 11, 2.0, 2.0) and np.isnan(b["additive"])
    wide = qtl.peaks(lod[0], pos, cs, 3.0, drop=2.0)
    assert (wide[0]["lo"], wide[0]["hi"]) == (1, 3) and (wide[1]["lo"], wide[1]["hi"]) == (10, 11)
    # a threshold per trait; a LOD equal to the threshold is not above it
    assert qtl.peaks(lod, pos, cs, [5.0, -1.0]) == [dict(trait=1, chrom=c, marker=m, lod=0.0, lo=m, hi=hi, pos=0.0, pos_lo=0.0,
                                                         pos_hi=pos[hi]) for c, m, hi in ((0, 0, 4), (1, 5, 8), (2, 9, 11))]


# ---------------------------------------------------------------------------------------------- symbols
def test_symbols_declared_exported_and_bound(host):
    from cnf2freq_amd import capi
    hdr = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    L = capi.load()
    for sym, method in (("cnf2_qtl_scan", "qtl_scan"), ("cnf2_sweep_qtl", "sweep_qtl"), ("cnf2_set_qtl_columns", "set_qtl_columns")):
        assert sym + "(" in hdr and hasattr(L, sym) and sym in capi.SYMBOLS and hasattr(capi.Context, method), sym
    assert hasattr(capi.Context, "qtl_scan_device") and hasattr(capi.Context, "sweep_qtl_device")
    for flag, name in ((capi.QTL_ADDITIVE, "CNF2_QTL_ADDITIVE"), (capi.QTL_ORIGIN_DEVICE, "CNF2_QTL_ORIGIN_DEVICE")):
        shift = flag.bit_length() - 1
        assert "%s = 1u << %d," % (name, shift) in " ".join(hdr.split()), name
        assert hdr.count("1u << %d," % shift) == 1, "the bit is taken once"
    hh = open(os.path.join(ROOT, "include", "cnf2host.h")).read()
    for sym in ("cnf2h_qtl_permutations", "cnf2h_qtl_null_residuals"):
        assert sym + "(" in hh and hasattr(host.load(), sym) and sym in host.SYMBOLS


# ---------------------------------------------------------------------------------------------- command line
def run_cli(tmp_path, *extra):
    import __graft_entry__ as g
    g.build()
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "1", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))


def test_cli_usage_errors(tmp_path):
    """every one of these ends with status 2 and a message before a GPU is asked for"""
    ph = tmp_path / "p.txt"
    ph.write_text("id weight age\nC 1.0 3\nD NA 4\nF 2.5 -\n")
    for extra, text in ((["--qtl", "q.txt"], "--qtl FILE needs --phenofile FILE"),
                        (["--phenofile", str(ph)], "need --qtl FILE"),
                        (["--qtl-permutations", "10"], "need --qtl FILE"),
                        (["--qtl-seed", "3"], "need --qtl FILE"),
                        (["--qtl-additive"], "need --qtl FILE"),
                        (["--qtl-covariates", "age"], "need --qtl FILE"),
                        (["--qtl", "q.txt", "--phenofile", str(ph), "--gpus", "2"], "--qtl needs a single GPU"),
                        (["--qtl", "q.txt", "--phenofile", str(ph), "--qtl-permutations", "-1"], "must not be negative"),
                        (["--qtl", "q.txt", "--phenofile", str(ph), "--qtl-covariates", "age,height,sex"], "not a column of .*: height sex"),
                        (["--qtl", "q.txt", "--phenofile", str(ph), "--qtl-covariates", "age,weight"], "no trait is left"),
                        (["--qtl", "q.txt", "--phenofile", str(tmp_path / "none.txt")], "cannot read .*none.txt")):
        r = run_cli(tmp_path, *extra)
        assert r.returncode == 2, (extra, r.returncode, r.stderr[-300:])
        import re
        assert re.search(text, r.stderr), (extra, r.stderr[-300:])
        assert not (tmp_path / "q.txt").exists()
    bad = tmp_path / "bad.txt"
    bad.write_text("id weight\nC 1.0\nnobody 2.0\nD 1.5\nstranger 0.5\n")
    r = run_cli(tmp_path, "--qtl", "q.txt", "--phenofile", str(bad))
    assert r.returncode == 2 and "not in the pedigree: nobody stranger" in r.stderr
    for text, msg in (("id weight\nC 1.0 2.0\n", "line 2 has 3 fields"), ("id weight\nC heavy\n", '"heavy" is not a number'), ("id\nC\n", "at least one name")):
        bad.write_text(text)
        r = run_cli(tmp_path, "--qtl", "q.txt", "--phenofile", str(bad))
        assert r.returncode == 2 and msg in r.stderr, r.stderr[-300:]
