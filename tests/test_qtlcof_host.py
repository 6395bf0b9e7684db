"""CPU suite of the cofactor scan's host side: the algebra of cnf2freq_amd/csrc/cnf2_qtlcof.h compiled for the host (through
cnf2h_qtlcof_marker) against the least-squares yardstick of tests/qtlcof_reference.py on Gram matrices formed in numpy;
cofactor_windows on a hand-made map; what read_multi, fit_multi and forward_select read off hand-made scan outputs; the
refusals of the host entry; the symbols; the command line's usage errors.  The scan itself needs a GPU
(tests/test_gpu_qtlcof.py)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import qtl
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, columns
from qtlcof_reference import CASES, WORST_PIVOT, case_id, case_reference, compared_markers, gram_of, make_case, worst_pivot

EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    return h


def host_scan_cof(host, origin, cs, pheno, cof, excl, use=None, cov=None, perm=None, additive=False):
    """what cnf2_qtl_scan_cof computes, with numpy forming the sums the kernels form (the normal matrix of a marker's design
    with every cofactor, X'y, sum c y^2) and cnf2_qtlcof.h, compiled for the host, deciding everything else"""
    o = np.asarray(origin, np.float64)
    n, M = o.shape[:2]
    K = 0 if cov is None else np.asarray(cov).reshape(n, -1).shape[1]
    u = np.ones(n, bool) if use is None else np.asarray(use) != 0
    Y = columns(np.where(u[:, None], np.asarray(pheno, np.float64).reshape(n, -1), 0.0), perm)
    B, T = Y.shape[1], Y.shape[2]
    ne = 1 if additive else 2
    out = dict(lod=np.zeros((B, T, M)), lod_base=np.zeros((B, T, M)), coef=np.zeros((T, M, ne)), rank=np.zeros(M, np.int32),
               rank_cof=np.zeros(M, np.int32))
    for m in range(M):
        gram, xty, yy, n_c = gram_of(o, cs, m, Y.reshape(n, B * T), cof, use, cov, additive)
        skip = sum(1 << q for q in range(len(cof)) if excl[0][q] <= m <= excl[1][q])
        r = host.qtlcof_marker(gram, xty, yy, n_c, K, len(cof), skip, additive)
        out["lod"][:, :, m] = r["lod"].reshape(B, T)
        out["lod_base"][:, :, m] = r["lod_base"].reshape(B, T)
        out["coef"][:, m] = r["coef"][:T]
        out["rank"][m], out["rank_cof"][m] = r["rank"], r["rank_cof"]
    return out


# ---------------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_marker_algebra_against_lstsq(host, case):
    n, K, cof, hw, additive, seed, T, P, mask, skipped = case
    origin, pheno, cov, use, perm, excl = make_case(*case)
    cs = chromstarts_of(CHROM_LENS)
    ref = case_reference(case)
    compared = compared_markers(ref, cs)
    assert compared.all() and abs(worst_pivot(ref, cs) - WORST_PIVOT[CASES.index(case)]) <= 0.006
    got = host_scan_cof(host, origin, cs, pheno, cof, excl, use, cov, perm, additive)
    err_l, err_b = np.abs(got["lod"] - ref["lod"]).max(), np.abs(got["lod_base"] - ref["lod_base"]).max()
    assert np.array_equal(np.isnan(got["coef"]), np.isnan(ref["coef"]))
    both = ~np.isnan(ref["coef"])
    err_c = (np.abs(got["coef"][both] - ref["coef"][both]) / np.maximum(1.0, np.abs(ref["coef"][both]))).max()
    print("%s: lod %.3g, lod_base %.3g over %d cells, coef %.3g" % (case_id(case), err_l, err_b, got["lod"].size, err_c))
    assert np.array_equal(got["rank"], ref["rank"]) and np.array_equal(got["rank_cof"], ref["rank_cof"])
    assert err_l <= ATOL and err_b <= ATOL and err_c <= ATOL
    assert np.all(got["lod"] >= 0) and np.all(got["lod_base"] >= 0) and np.isfinite(got["lod"]).all()
    assert np.all(got["lod"][:, :, got["rank"] == 0] == 0.0)
    # a cofactor that is left out counts for nothing: ne kept columns fewer per cofactor whose range holds the marker
    ne = 1 if additive else 2
    out_here = np.array([sum(excl[0][q] <= m <= excl[1][q] for q in range(len(cof))) for m in range(origin.shape[1])])
    assert np.array_equal(got["rank_cof"], ne * (len(cof) - out_here))


def test_marker_refusals_on_the_host(host):
    g, b, y = np.eye(16), np.zeros((1, 16)), np.ones(1)
    for kw in (dict(n_cov=0, n_cof=7), dict(n_cov=2, n_cof=6), dict(n_cov=0, n_cof=14, additive=True), dict(n_cov=1, n_cof=13, additive=True),
               dict(n_cov=-1, n_cof=1), dict(n_cov=0, n_cof=-1)):
        with pytest.raises(RuntimeError):
            host.qtlcof_marker(g, b, y, 40, **kw)
    for kw in (dict(n_cov=0, n_cof=6), dict(n_cov=0, n_cof=13, additive=True), dict(n_cov=8, n_cof=2), dict(n_cov=0, n_cof=0)):
        r = host.qtlcof_marker(g, b, y, 40, **kw)
        assert r["usable"] and r["lod"][0] == 0.0 and r["lod_base"][0] == 0.0
    # every cofactor left out: no cofactor column is kept; too few individuals: nothing is
    r = host.qtlcof_marker(g, b, y, 40, n_cov=0, n_cof=3, skip=0b111)
    assert r["rank_cof"] == 0 and r["rank"] == 2
    r = host.qtlcof_marker(g, b, y, 9, n_cov=0, n_cof=3)
    assert not r["usable"] and r["rank_cof"] == 0 and r["rank"] == 0 and np.isnan(r["coef"]).all()
    assert host.qtlcof_marker(g, b, y, 10, n_cov=0, n_cof=3)["usable"]


# ---------------------------------------------------------------------------------------------- reading the scan
def test_cofactor_windows_on_a_hand_made_map():
    pos = np.array([0.0, 1.0, 5.0, 5.0, 9.0, 0.0, 4.0, 0.0, 2.0, 3.0, 10.0])
    cs = np.array([0, 5, 7, 11])
    lo, hi = qtl.cofactor_windows([2, 5, 9], pos, cs, 0.0)
    assert lo.dtype == np.int32 and list(lo) == [2, 5, 9] and list(hi) == [3, 5, 9]          # (3 shares the position of 2)
    lo, hi = qtl.cofactor_windows([2, 5, 9], pos, cs, 4.0)
    assert list(lo) == [1, 5, 7] and list(hi) == [4, 6, 9]                                   # clipped to the chromosome
    lo, hi = qtl.cofactor_windows([0, 10], pos, cs, 100.0)
    assert list(lo) == [0, 7] and list(hi) == [4, 10]
    lo, hi = qtl.cofactor_windows([], pos, cs, 1.0)
    assert len(lo) == 0 and len(hi) == 0
    for bad in ([11], [-1]):
        with pytest.raises(ValueError):
            qtl.cofactor_windows(bad, pos, cs, 1.0)
    with pytest.raises(ValueError):
        qtl.cofactor_windows([1], pos, cs, -1.0)


def hand_made_scan(M=8, T=2):
    lod = np.arange(T * M, dtype=np.float64).reshape(T, M) * 0.5
    base = 10.0 - lod
    coef = np.stack([lod + 1.0, -lod], axis=2)
    return dict(lod=lod, lod_base=base, coef=coef, n_used=np.array([[20, 50], [25, 40]]))


def test_read_multi_on_hand_made_outputs():
    out = hand_made_scan()
    cs = np.array([0, 3, 8])
    r = qtl.read_multi(out, [6, 1], cs)
    assert list(r["loci"]) == [6, 1] and np.array_equal(r["drop_one"], out["lod"][:, [6, 1]])
    assert np.array_equal(r["lod_full"], [10.0, 10.0]) and np.array_equal(r["coef"], out["coef"][:, [6, 1]])
    assert np.array_equal(r["n"], [[50, 20], [40, 25]])
    assert np.allclose(r["var_full"], 1.0 - 10.0 ** (-2.0 * 10.0 / np.array([50.0, 40.0])), rtol=0, atol=1e-15)
    assert np.allclose(r["var_drop"], 1.0 - 10.0 ** (-2.0 * r["drop_one"] / np.array([[50.0, 20.0], [40.0, 25.0]])), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        qtl.read_multi(out, [], cs)
    # fit_multi hands its scanner the loci in ascending order, each left out at its own marker only, and no permutations
    calls = []

    def scanner(cof, excl, permutations, seed):
        calls.append((list(cof), list(excl[0]), list(excl[1]), permutations))
        return out
    f = qtl.fit_multi(None, None, [6, 1], scanner=scanner, chromstarts=cs)
    assert calls == [([1, 6], [1, 6], [1, 6], 0)] and np.array_equal(f["drop_one"], r["drop_one"])


def test_forward_select_on_hand_made_outputs():
    """a scanner that plays three steps: the best candidate enters while it beats the step's threshold; markers inside a range
    are no candidates however large their LOD"""
    M, cs = 10, np.array([0, 6, 10])
    pos = np.array([0.0, 1, 2, 3, 4, 5, 0, 1, 2, 3])
    profiles = {(): [1, 2, 9, 3, 1, 1, 1, 5, 1, 1], (2,): [1, 30, 40, 30, 2, 1, 1, 6, 1, 1], (2, 7): [1, 30, 40, 30, 2.5, 1, 50, 50, 50, 1]}
    thr = {(): 4.0, (2,): 5.0, (2, 7): 3.0}
    calls = []

    def scanner(cof, excl, permutations, seed):
        key = tuple(int(m) for m in cof)
        calls.append((key, list(excl[0]), list(excl[1]), permutations, seed))
        mk = np.arange(M)
        cand = np.ones(M, bool)
        for lo, hi in zip(excl[0], excl[1]):
            cand &= ~((lo <= mk) & (mk <= hi))
        pm = None
        if permutations:
            pm = np.zeros((permutations, 1, 2))
            pm[:, 0, 0] = np.linspace(0.0, thr[key] / 0.95 * (1.0 - 1.0 / permutations), permutations)      # the 95 % order statistic is thr
        lod = np.asarray(profiles[key], np.float64)[None]
        return dict(lod=lod, lod_base=7.0 - lod, coef=np.zeros((1, M, 2)), n_used=np.array([[30, 30]]), perm_max=pm, candidate=cand)
    got = qtl.forward_select(None, np.zeros(30), 5, 1.0, pos, permutations=20, seed=9, scanner=scanner, chromstarts=cs)
    th = [float(qtl.thresholds(scanner(k, ([], []), 20, 0)["perm_max"], (0.05,))["genome"][0, 0]) for k in ((), (2,), (2, 7))]
    assert got["loci"] == [2, 7] and got["lod"] == [9.0, 6.0] and got["threshold"] == th[:2]
    assert got["stopped"] == dict(marker=4, lod=2.5, threshold=th[2]) and th[2] < 3.0 < th[0]
    assert calls[0] == ((), [], [], 20, 9) and calls[1] == ((2,), [1], [3], 20, 9) and calls[2] == ((2, 7), [1, 6], [3, 8], 20, 9)
    assert calls[3] == ((2, 7), [2, 7], [2, 7], 0, 0)
    assert list(got["fit"]["loci"]) == [2, 7] and np.array_equal(got["fit"]["drop_one"], [[40.0, 50.0]]) and got["fit"]["lod_full"][0] == 7.0
    # max_loci stops it before a scan; without loci there is no fit
    one = qtl.forward_select(None, np.zeros(30), 1, 1.0, pos, permutations=20, scanner=scanner, chromstarts=cs)
    assert one["loci"] == [2] and one["stopped"] is None and list(one["fit"]["loci"]) == [2]
    thr[()] = 100.0
    none = qtl.forward_select(None, np.zeros(30), 5, 1.0, pos, permutations=20, scanner=scanner, chromstarts=cs)
    assert none["loci"] == [] and none["fit"] is None and none["stopped"]["marker"] == 2
    with pytest.raises(ValueError):
        qtl.forward_select(None, np.zeros((30, 2)), 5, 1.0, pos, scanner=scanner, chromstarts=cs)
    with pytest.raises(ValueError):
        qtl.forward_select(None, np.zeros(30), 5, 1.0, pos, permutations=0, scanner=scanner, chromstarts=cs)


def test_new_symbols_in_both_libraries(host):
    from cnf2freq_amd import capi
    assert {"cnf2_qtl_scan_cof", "cnf2_set_qtlcof_columns"} <= set(capi.SYMBOLS)
    assert "cnf2h_qtlcof_marker" in host.SYMBOLS
    import ctypes
    hip = ctypes.CDLL(os.path.join(ROOT, "cnf2freq_amd", "libcnf2hip.so"))
    for s in ("cnf2_qtl_scan_cof", "cnf2_set_qtlcof_columns"):
        assert getattr(hip, s)
    assert getattr(host.load(), "cnf2h_qtlcof_marker")
    for name in ("qtl_scan_cof", "qtl_scan_cof_device", "set_qtlcof_columns"):
        assert callable(getattr(capi.Context, name))
    for name in ("cofactor_windows", "scan_cof", "fit_multi", "forward_select", "read_multi"):
        assert callable(getattr(qtl, name))


# ---------------------------------------------------------------------------------------------- command line
def run_cli(tmp_path, *extra):
    import __graft_entry__ as g
    g.build()
    files = [os.path.join(DEMO, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    args = [EXE, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--count", "1", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))


def test_cli_usage_errors(tmp_path):
    """every one of these ends with status 2 and a message before a GPU is asked for; the existing messages keep their text"""
    import re
    ph = tmp_path / "p.txt"
    ph.write_text("id weight " + " ".join("z%d" % k for k in range(7)) + "\nC 1.0 1 2 3 4 5 6 7\nD NA 1 2 3 4 5 6 7\nF 2.5 1 2 3 4 5 6 -\n")
    base = ["--qtlcof", "q.txt", "--phenofile", str(ph)]
    for extra, text in ((["--qtlcof", "q.txt", "--qtl-cofactors", "1"], "^--qtlcof FILE needs --phenofile FILE$"),
                        (base, "^--qtlcof FILE needs --qtl-cofactors LIST$"),
                        (["--qtl-cofactors", "1,2"], "^--qtl-cofactors and --qtl-window need --qtlcof FILE$"),
                        (["--qtl-window", "2.5", "--qtl", "q.txt", "--phenofile", str(ph)], "^--qtl-cofactors and --qtl-window need --qtlcof FILE$"),
                        (base + ["--qtl-cofactors", "1", "--gpus", "2"], r"^--qtlcof needs a single GPU \(--gpus 1\)"),
                        (base + ["--qtl-cofactors", "1,100000"], "--qtl-cofactors: marker 100000 is not on the map"),
                        (base + ["--qtl-cofactors", "3,1,3"], "--qtl-cofactors: marker 3 is given twice"),
                        (base + ["--qtl-cofactors", "1,x"], "--qtl-cofactors: not a marker index: x"),
                        (base + ["--qtl-cofactors", "1", "--qtl-window", "-1"], "--qtl-window must not be negative"),
                        (base + ["--qtl-cofactors", "0,1,2,3,4,5,6"], "--qtlcof: the design has 17 columns"),
                        (base + ["--qtl-cofactors", "0,1,2,3,4,5", "--qtl-covariates", "z0"], "--qtlcof: the design has 16 columns"),
                        # the existing messages, word for word
                        (["--phenofile", str(ph)], "--phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed and --qtl-additive need --qtl FILE or --qtl2 FILE$"),
                        (["--qtl", "q.txt"], "^--qtl FILE needs --phenofile FILE$"),
                        (["--qtlx", "q.txt"], "--qtlx FILE needs --phenofile FILE")):
        r = run_cli(tmp_path, *extra)
        assert r.returncode == 2, (extra, r.returncode, r.stderr[-300:])
        assert re.search(text, r.stderr, re.M), (extra, r.stderr[-300:])
        assert not (tmp_path / "q.txt").exists()
