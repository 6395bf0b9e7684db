"""CPU suite of the pair scan's host side: the algebra of cnf2freq_amd/csrc/cnf2_qtl2.h compiled for the host (through
cnf2h_qtl2_pair) against the least-squares yardstick of tests/qtl2_reference.py on the sums of explicit designs, with every
drop pattern of the degenerate designs; pair_summary and thresholds2 on hand-made matrices; the symbols; the command line's
usage errors.  The scan itself needs a GPU (tests/test_gpu_qtl2.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import qtl
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, columns, noise, soft_rows
from qtl2_reference import (added_columns, chrom_of, compared_pairs, degenerate_case, exact_case, reference_scan2)

EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    return h


def host_scan2(host, origin, cs, sel, pheno, use=None, cov=None, perm=None, additive=False):
    """what cnf2_qtl_scan2 computes, with numpy forming the sums the kernels form (the normal matrix of a pair's design,
    X'y, sum c y^2) and cnf2_qtl2.h, compiled for the host, deciding everything else"""
    o = np.asarray(origin, np.float64)
    n, L = o.shape[0], len(sel)
    sc = chrom_of(sel, cs)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    X0 = np.ones((n, 1)) if cov is None else np.concatenate([np.ones((n, 1)), np.asarray(cov, np.float64).reshape(n, -1)], axis=1)
    K = X0.shape[1] - 1
    Y = columns(np.where(use[:, None], np.asarray(pheno, np.float64).reshape(n, -1), 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    present = o[:, np.asarray(cs)[:-1]].any(axis=2)
    out = dict(lod_add=np.full((Q, T, L, L), np.nan), lod_full=np.full((Q, T, L, L), np.nan),
               rank_add=np.full((L, L), -1, np.int32), rank_full=np.full((L, L), -1, np.int32))
    for j in range(L):
        for k in range(j + 1, L):
            keep = use & present[:, sc[j]] & present[:, sc[k]]
            add, inter = added_columns(o[keep, sel[j]], o[keep, sel[k]], additive, sc[j] == sc[k])
            X = np.column_stack([X0[keep]] + add + inter)
            gram, xty = np.zeros((16, 16)), np.zeros((Q * T, 16))
            gram[:X.shape[1], :X.shape[1]] = X.T @ X
            y = Y[keep].reshape(int(keep.sum()), Q * T)
            xty[:, :X.shape[1]] = (X.T @ y).T
            r = host.qtl2_pair(gram, xty, (y ** 2).sum(axis=0), int(keep.sum()), K, additive, sc[j] == sc[k])
            out["lod_add"][:, :, j, k], out["lod_full"][:, :, j, k] = r["lod_add"].reshape(Q, T), r["lod_full"].reshape(Q, T)
            out["rank_add"][j, k], out["rank_full"][j, k] = r["rank_add"], r["rank_full"]
    return out


def check(got, ref, what):
    compared = compared_pairs(ref, share=0.99 if what[0] != "d" else 0.0)
    cross = ref["cross"] & compared
    err_a = np.abs(got["lod_add"] - ref["lod_add"])[:, :, compared].max()
    err_f = np.abs(got["lod_full"] - ref["lod_full"])[:, :, cross].max() if cross.any() else 0.0
    print("%s: lod_add %.3g, lod_full %.3g over %d / %d pairs" % (what, err_a, err_f, compared.sum(), cross.sum()))
    assert np.array_equal(got["rank_add"], ref["rank_add"]) and np.array_equal(got["rank_full"], ref["rank_full"]), what
    assert np.array_equal(np.isnan(got["lod_full"]), np.isnan(ref["lod_full"])), what
    assert err_a <= ATOL and err_f <= ATOL, what


# ---------------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("n,K,seed,additive", [(40, 2, 5, False), (24, 0, 3, False), (41, 6, 9, True)])
def test_pair_algebra_against_lstsq(host, n, K, seed, additive):
    cs = chromstarts_of(CHROM_LENS)
    sel = np.arange(0, int(cs[-1]), 3)
    origin, _ = soft_rows(n, CHROM_LENS, seed)
    cov = noise(n, K, seed + 1) if K else None
    a = origin[:, :, 3] - origin[:, :, 0]
    pheno = np.stack([noise(n, 1, seed + 2)[:, 0] + a[:, 6] * a[:, 60], noise(n, 1, seed + 3)[:, 0] + a[:, 30]], axis=1)
    perm = qtl.permutations(n, 2, seed)
    ref = reference_scan2(origin, cs, sel, pheno, cov=cov, perm=perm, additive=additive)
    got = host_scan2(host, origin, cs, sel, pheno, cov=cov, perm=perm, additive=additive)
    check(got, ref, "n %d K %d" % (n, K))
    assert ref["rank_full"].max() == (3 if additive else 8) and ref["rank_add"].max() == (2 if additive else 4)


def test_degenerate_designs_on_the_host(host):
    lens, origin, sel, pheno, want = degenerate_case()
    cs = chromstarts_of(lens)
    for additive in (False, True):
        ref = reference_scan2(origin, cs, sel, pheno, additive=additive)
        got = host_scan2(host, origin, cs, sel, pheno, additive=additive)
        check(got, ref, "degenerate designs" + (" additive" if additive else ""))
        for (j, k), (ra, rf) in want[additive].items():
            assert (got["rank_add"][j, k], got["rank_full"][j, k]) == (ra, rf), (additive, j, k)
            if ra == 0:
                assert np.all(got["lod_add"][:, :, j, k] == 0.0)
            if rf == 0:
                assert np.all(got["lod_full"][:, :, j, k] == 0.0)


def test_constant_and_exactly_epistatic_phenotypes_on_the_host(host):
    lens, origin, sel, pheno, clamp = exact_case()
    got = host_scan2(host, origin, chromstarts_of(lens), sel, pheno)
    assert (got["rank_add"][0, 1], got["rank_full"][0, 1]) == (2, 3)
    assert got["lod_add"][0, 0, 0, 1] == 0.0 and got["lod_full"][0, 0, 0, 1] == 0.0           # the constant: RSS0 = 0
    print("clamped lod_full %.12f, expected %.12f" % (got["lod_full"][0, 1, 0, 1], clamp))
    assert got["lod_add"][0, 1, 0, 1] == 0.0 and abs(got["lod_full"][0, 1, 0, 1] - clamp) <= ATOL


def test_random_gram_matrices(host):
    """designs that are plain random matrices (no structure of a cross): widths of every model, columns zeroed or repeated at
    random; ranks and LODs against lstsq on the same columns"""
    from qtl2_reference import lod_of, sequential_pivots
    u = lambda s, shape: noise(int(np.prod(shape)), 1, s)[:, 0].reshape(shape)
    for seed, (K, additive, same) in enumerate([(0, False, False), (6, False, False), (3, True, False), (2, False, True), (1, True, True)]):
        n, nadd = 30 + seed, (2 if additive else 4)
        nint = 0 if same else (1 if additive else 4)
        X0 = np.column_stack([np.ones(n), u(100 + seed, (n, K))]) if K else np.ones((n, 1))
        A = u(200 + seed, (n, nadd + nint))
        if seed % 2:
            A[:, 1] = 0.0                                # a raw diagonal of 0
            A[:, -1] = A[:, 0] * 2.0                     # a repeated direction
        y = u(300 + seed, (n, 3)) + A[:, :1]
        X = np.column_stack([X0, A])
        gram, xty = np.zeros((16, 16)), np.zeros((3, 16))
        gram[:X.shape[1], :X.shape[1]], xty[:, :X.shape[1]] = X.T @ X, (X.T @ y).T
        r = host.qtl2_pair(gram, xty, (y ** 2).sum(axis=0), n, K, additive, same)
        _, kept = sequential_pivots(X0, list(A.T))
        rss = lambda Z: ((y - Z @ np.linalg.lstsq(Z, y, rcond=None)[0]) ** 2).sum(axis=0)
        rss0, rssa, rssf = rss(X0), rss(X[:, :X0.shape[1] + nadd]), rss(X)
        assert r["usable"] and r["rank_add"] == sum(kept[:nadd]) and r["rank_full"] == (-1 if same else sum(kept))
        np.testing.assert_allclose(r["rss0"], rss0, rtol=0, atol=1e-9)
        np.testing.assert_allclose(r["lod_add"], lod_of(rss0, rssa, n), rtol=0, atol=ATOL)
        if same:
            assert np.isnan(r["lod_full"]).all()
        else:
            np.testing.assert_allclose(r["lod_full"], lod_of(rss0, rssf, n), rtol=0, atol=ATOL)
    # not scanned: fewer than K + 10 individuals, or a null design without a Cholesky factor
    gram = np.zeros((16, 16))
    gram[0, 0] = 9.0
    r = host.qtl2_pair(gram, np.ones((1, 16)), [5.0], 9, 0)
    assert (r["usable"], r["rank_add"], r["rank_full"]) == (False, 0, 0) and r["lod_add"][0] == 0.0 and r["lod_full"][0] == 0.0
    gram[0, 0], gram[1, 0], gram[1, 1] = 20.0, 20.0, 20.0            # the covariate is the intercept again
    r = host.qtl2_pair(gram, np.ones((1, 16)), [5.0], 20, 1, same_chrom=True)
    assert (r["usable"], r["rank_add"], r["rank_full"]) == (False, 0, -1) and r["lod_add"][0] == 0.0 and np.isnan(r["lod_full"][0])


# ---------------------------------------------------------------------------------------------- thresholds, summary
def test_thresholds2_on_hand_made_maxima():
    P, T = 100, 2
    pm = np.zeros((P, T, 3))
    pm[:, 0, 0] = np.arange(P)
    pm[:, 0, 1] = np.arange(P)[::-1] * 2.0
    pm[:, 0, 2] = 1.0                                    # ties: every order statistic is the value
    pm[:, 1, 2] = np.arange(P) % 2
    thr = qtl.thresholds2(pm)
    assert thr["alpha"] == (0.05, 0.01) and thr["add"].shape == (2, T)
    assert list(thr["add"][:, 0]) == [94.0, 98.0] and list(thr["full"][:, 0]) == [188.0, 196.0] and list(thr["int"][:, 0]) == [1.0, 1.0]
    assert list(thr["add"][:, 1]) == [0.0, 0.0] and list(thr["int"][:, 1]) == [1.0, 1.0]
    assert list(qtl.thresholds2(pm, alpha=(0.5,))["int"][:, 1]) == [0.0]
    assert qtl.thresholds2(pm[:1])["full"].shape == (2, T)
    for bad in (np.zeros((0, 1, 3)), np.zeros((4, 1, 2))):
        with pytest.raises(ValueError):
            qtl.thresholds2(bad)


def test_pair_summary_on_hand_made_matrices():
    cs = [0, 4, 5, 9, 12]                                 # chromosome 1 has one marker; chromosome 3 has no selected locus
    sel = [0, 2, 4, 5, 7]                                 # chromosomes 0, 0, 1, 2, 2
    L = len(sel)
    la, lf = np.full((L, L), np.nan), np.full((L, L), np.nan)
    up = np.triu_indices(L, 1)
    la[up] = [1.0, 2.0, 3.0, 3.0, 2.5, 0.5, 3.0, 4.0, 4.0, 0.25]      # (0,1) (0,2) (0,3) (0,4) (1,2) (1,3) (1,4) (2,3) (2,4) (3,4)
    lf[up] = [np.nan, 2.5, 5.0, 3.5, 2.5, 5.0, 3.0, 4.0, 6.0, np.nan]
    found = qtl.pair_summary(la, lf, sel, cs)
    assert [(r["chrom1"], r["chrom2"]) for r in found] == [(0, 0), (0, 1), (0, 2), (1, 2), (2, 2)]      # (1, 1) holds no pair
    same = found[0]
    assert same["add"] == (0, 2) and same["lod_add"] == 1.0 and same["full"] is None
    assert np.isnan(same["lod_full"]) and np.isnan(same["lod_int"]) and np.isnan(same["lod_add_at_full"])
    r01 = found[1]
    assert r01["add"] == (2, 4) and r01["lod_add"] == 2.5 and r01["full"] == (0, 4) and r01["lod_full"] == 2.5, "the first pair wins a tie"
    assert r01["lod_add_at_full"] == 2.0 and r01["lod_int"] == 0.0
    r02 = found[2]                                        # best additive pair and best full pair differ; ties in both
    assert r02["add"] == (0, 5) and r02["lod_add"] == 3.0 and r02["full"] == (0, 5) and r02["lod_full"] == 5.0 and r02["lod_int"] == 2.0
    r12 = found[3]
    assert r12["add"] == (4, 5) and r12["full"] == (4, 7) and r12["lod_full"] == 6.0 and r12["lod_add_at_full"] == 4.0 and r12["lod_int"] == 2.0
    assert found[4]["add"] == (5, 7) and found[4]["lod_add"] == 0.25
    both = qtl.pair_summary(np.stack([la, la * 2.0]), np.stack([lf, lf * 2.0]), sel, cs)
    assert len(both) == 10 and [r["trait"] for r in both] == [0] * 5 + [1] * 5 and both[7]["lod_int"] == 4.0
    with pytest.raises(ValueError):
        qtl.pair_summary(la, lf[:4, :4], sel, cs)
    assert list(qtl.select_every(cs, 2)) == [0, 2, 4, 5, 7, 9, 11] and list(qtl.select_every(cs, 1)) == list(range(12))


# ---------------------------------------------------------------------------------------------- symbols
def test_symbols_declared_exported_and_bound(host):
    from cnf2freq_amd import capi
    hdr = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    L = capi.load()
    for sym, method in (("cnf2_qtl_scan2", "qtl_scan2"), ("cnf2_set_qtl2_columns", "set_qtl2_columns")):
        assert sym + "(" in hdr and hasattr(L, sym) and sym in capi.SYMBOLS and hasattr(capi.Context, method), sym
    assert hasattr(capi.Context, "qtl_scan2_device")
    hh = open(os.path.join(ROOT, "include", "cnf2host.h")).read()
    assert "cnf2h_qtl2_pair(" in hh and hasattr(host.load(), "cnf2h_qtl2_pair") and "cnf2h_qtl2_pair" in host.SYMBOLS
    for name in ("scan2", "thresholds2", "pair_summary"):
        assert callable(getattr(qtl, name))


# ---------------------------------------------------------------------------------------------- command line
def run_cli(tmp_path, *extra, files=None):
    import __graft_entry__ as g
    g.build()
    files = files or [os.path.join(DEMO, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    args = [EXE, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--count", "1", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))


def test_cli_usage_errors(tmp_path):
    """every one of these ends with status 2 and a message before a GPU is asked for"""
    ph = tmp_path / "p.txt"
    ph.write_text("id weight " + " ".join("z%d" % k for k in range(7)) + "\nC 1.0 1 2 3 4 5 6 7\nD NA 1 2 3 4 5 6 7\nF 2.5 1 2 3 4 5 6 -\n")
    for extra, text in ((["--qtl2", "q.txt"], "--qtl2 FILE needs --phenofile FILE"),
                        (["--qtl2-every", "2"], "--qtl2-every needs --qtl2 FILE"),
                        (["--qtl2-every", "2", "--qtl", "q.txt", "--phenofile", str(ph)], "--qtl2-every needs --qtl2 FILE"),
                        (["--qtl2", "q.txt", "--phenofile", str(ph), "--gpus", "2"], "--qtl2 needs a single GPU"),
                        (["--qtl2", "q.txt", "--phenofile", str(ph), "--qtl2-every", "0"], "--qtl2-every must be at least 1"),
                        (["--qtl2", "q.txt", "--phenofile", str(ph), "--qtl-permutations", "-1"], "must not be negative"),
                        (["--qtl2", "q.txt", "--phenofile", str(ph), "--qtl-covariates", "z0,z1,z2,z3,z4,z5,z6"], "--qtl2: at most 6 covariates"),
                        (["--qtl2", "q.txt", "--phenofile", str(ph), "--qtl-covariates", "nothing"], "not a column of .*: nothing"),
                        (["--qtl2", "q.txt", "--phenofile", str(ph), "--qtl2-every", "100000"], r"S = 100000 selects 1 loci.*lower S"),
                        (["--qtl2", "q.txt", "--phenofile", str(tmp_path / "none.txt")], "cannot read .*none.txt")):
        r = run_cli(tmp_path, *extra)
        assert r.returncode == 2, (extra, r.returncode, r.stderr[-300:])
        assert re.search(text, r.stderr), (extra, r.stderr[-300:])
        assert not (tmp_path / "q.txt").exists()
    # a selection of more than 4096 loci: the message names S
    big = [tmp_path / ("big." + e) for e in ("map", "ped", "gen")]
    big[0].write_text("".join("%r\n" % (0.01 * m) for m in range(4100)))
    big[1].write_text("A 0 0\nB 0 0\nX A B 2\n")
    big[2].write_text("".join("%s %s\n" % (nm, " ".join(["1"] * 4100)) for nm in ("A", "B", "X")))
    tb = tmp_path / "pb.txt"
    tb.write_text("id w\nX 1.0\n")
    r = run_cli(tmp_path, "--qtl2", "q.txt", "--phenofile", str(tb), files=[str(f) for f in big])
    assert r.returncode == 2 and re.search(r"S = 1 selects 4100 loci.*raise S", r.stderr), r.stderr[-300:]
    assert not (tmp_path / "q.txt").exists()
