"""CPU suite of the extended single-locus scan's host side: the algebra of cnf2freq_amd/csrc/cnf2_qtlx.h compiled for the
host (through cnf2h_qtlx_marker) against the least-squares yardstick of tests/qtlx_reference.py on Gram matrices formed in
numpy, with the drop patterns of the degenerate designs; the column order of qtlx_column for every (ne, Ki); thresholdsx and
coef_names; the symbols; the command line's usage errors.  The scan itself needs a GPU (tests/test_gpu_qtlx.py)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import qtl
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, columns
from qtlx_reference import (CASES, DEGENERATE, case_reference, compared_markers, constant_case, constant_covariate_case,
                            degenerate_case, design_columns, gram_of, make_case, reference_scanx, tiny_imprint_case, width)

EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    return h


def host_scanx(host, origin, cs, pheno, use=None, cov=None, n_int=0, imprint=False, perm=None, additive=False):
    """what cnf2_qtl_scanx computes, with numpy forming the sums the kernels form (the normal matrix of a marker's design,
    X'y, sum c y^2) and cnf2_qtlx.h, compiled for the host, deciding everything else"""
    o = np.asarray(origin, np.float64)
    n, M = o.shape[:2]
    K = 0 if cov is None else np.asarray(cov).reshape(n, -1).shape[1]
    u = np.ones(n, bool) if use is None else np.asarray(use) != 0
    Y = columns(np.where(u[:, None], np.asarray(pheno, np.float64).reshape(n, -1), 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    ncoef = width(K, n_int, additive, imprint) - 1 - K
    out = dict(lod=np.zeros((Q, T, M, 3)), coef=np.zeros((T, M, ncoef)), rank=np.zeros((M, 3), np.int32))
    for m in range(M):
        gram, xty, yy, n_c = gram_of(o, cs, m, Y.reshape(n, Q * T), use, cov, n_int, imprint, additive)
        r = host.qtlx_marker(gram, xty, yy, n_c, K, n_int, additive, imprint)
        out["lod"][:, :, m] = r["lod"].reshape(Q, T, 3)
        out["coef"][:, m] = r["coef"][:T]
        out["rank"][m] = r["rank"]
    return out


def check(got, ref, cs, what, share=0.99):
    compared = compared_markers(ref, cs, share)
    err_l = np.abs(got["lod"] - ref["lod"]).max()
    gc, rc = got["coef"][:, compared], ref["coef"][:, compared]
    assert np.array_equal(np.isnan(gc), np.isnan(rc)), what
    both = ~np.isnan(rc)
    err_c = (np.abs(gc[both] - rc[both]) / np.maximum(1.0, np.abs(rc[both]))).max() if both.any() else 0.0
    print("%s: lod %.3g over %d cells, coef %.3g over %d markers" % (what, err_l, got["lod"].size, err_c, compared.sum()))
    assert np.array_equal(got["rank"], ref["rank"]), what
    assert err_l <= ATOL and err_c <= ATOL, what
    assert np.all(np.diff(got["lod"], axis=3) >= 0) and np.all(got["lod"] >= 0) and np.isfinite(got["lod"]).all(), what
    return err_l, err_c


# ---------------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-K%d-Ki%d-%s%s-T%d-P%d%s" % (
    c[0], c[1], c[2], "i" if c[3] else "m", "-add" if c[4] else "", c[6], c[7], "-mask" if c[8] else "-skip" if c[9] else ""))
def test_marker_algebra_against_lstsq(host, case):
    n, K, Ki, imprint, additive, seed, T, P, mask, skipped = case
    origin, pheno, cov, use, perm = make_case(*case)
    cs = chromstarts_of(CHROM_LENS)
    ref = case_reference(case)
    got = host_scanx(host, origin, cs, pheno, use, cov, Ki, imprint, perm, additive)
    check(got, ref, cs, "n %d K %d Ki %d" % (n, K, Ki))
    ne = 1 + (not additive) + imprint
    assert tuple(ref["rank"].max(axis=0)) == (1 if additive else 2, ne, ne * (1 + Ki))


def test_degenerate_designs_on_the_host(host):
    lens, origin, pheno, cov, want = degenerate_case()
    cs = chromstarts_of(lens)
    kw = dict(cov=cov, n_int=DEGENERATE["Ki"], imprint=True)
    ref = reference_scanx(origin, cs, pheno, **kw)
    got = host_scanx(host, origin, cs, pheno, **kw)
    check(got, ref, cs, "degenerate designs", share=0.0)
    names = qtl.coef_names(1, True)
    for c, ranks in want.items():
        for m in range(cs[c], cs[c + 1]):
            assert tuple(got["rank"][m]) == ranks, (c, m)
            if ranks[2] == 0:
                assert np.all(got["lod"][:, :, m] == 0.0) and np.isnan(got["coef"][:, m]).all()
    m = int(cs[2])
    assert [nm for nm, v in zip(names, got["coef"][0, m]) if np.isnan(v)] == ["d", "i", "d:z1", "i:z1"]
    m = int(cs[3])
    assert np.array_equal(got["lod"][:, :, m, 1], got["lod"][:, :, m, 0]) and np.all(got["lod"][:, :, m, 2] > got["lod"][:, :, m, 1])
    assert [nm for nm, v in zip(names, got["coef"][0, m]) if np.isnan(v)] == ["i", "i:z1"]
    m = int(cs[5])
    assert np.array_equal(got["lod"][:, :, m, 2], got["lod"][:, :, m, 1]) and np.isnan(got["coef"][0, m, 3:]).all()


def test_constant_phenotype_and_constant_covariate_on_the_host(host):
    lens, origin, pheno = constant_case()
    got = host_scanx(host, origin, chromstarts_of(lens), pheno, imprint=True)
    assert np.all(got["lod"][0, 0] == 0.0) and np.isnan(got["coef"][0]).all() and np.all(got["rank"] == (2, 3, 3))
    assert np.all(got["lod"][0, 1, :, 1] > got["lod"][0, 1, :, 0]) and np.isfinite(got["coef"][1]).all()
    lens, origin, pheno, cov = constant_covariate_case()
    got = host_scanx(host, origin, chromstarts_of(lens), pheno, cov=cov, n_int=1)
    assert np.all(got["rank"] == 0) and np.all(got["lod"] == 0.0) and np.isnan(got["coef"]).all()


def test_a_column_of_rounding_noise_is_a_column(host):
    """tiny_imprint_case: i is 1e-17 of the other columns and not 0.  The rank rule is relative to the column's own length, so
    i and i z are kept wherever the noise is not all zero; LODs and effects (of the order of 1e16) agree with the yardstick"""
    lens, origin, pheno = tiny_imprint_case()
    cs = chromstarts_of(lens)
    cov = np.where(np.arange(40) % 3 == 0, 0.5, -0.5)[:, None] + 0.0
    ref = reference_scanx(origin, cs, pheno, cov=cov, n_int=1, imprint=True)
    got = host_scanx(host, origin, cs, pheno, cov=cov, n_int=1, imprint=True)
    i = origin[:, :, 1] - origin[:, :, 2]
    assert 0.0 < np.abs(i).max() < 1e-15
    check(got, ref, cs, "a column of rounding noise", share=0.8)
    assert np.all(got["rank"][1:, 1] - got["rank"][1:, 0] == 1) and np.nanmax(np.abs(got["coef"][0, 1:, 2])) > 1e12


def test_marker_refusals_on_the_host(host):
    g, b, y = np.eye(16), np.zeros((1, 16)), np.ones(1)
    for kw in (dict(n_cov=1, n_int=2), dict(n_cov=3, n_int=3, imprint=True), dict(n_cov=8, n_int=3)):
        with pytest.raises(RuntimeError):
            host.qtlx_marker(g, b, y, 30, **kw)
    assert host.qtlx_marker(g, b, y, 30, n_cov=5, n_int=2, imprint=True)["usable"]           # W = 15


# ---------------------------------------------------------------------------------------------- the column order
def test_column_order_for_every_design(host):
    """qtlx_column, spelled out: X0, then a, d, i (those present), then per interactive covariate the same effects"""
    code = dict(a=1, d=2, i=3)
    seen = set()
    for additive in (False, True):
        for imprint in (False, True):
            ne = 1 + (not additive) + imprint
            for K in range(0, 9):
                for Ki in range(0, K + 1):
                    if width(K, Ki, additive, imprint) > 15:
                        continue
                    want = [(0, j) for j in range(K + 1)] + [(code[e], k) for e, k, _ in design_columns(K, Ki, additive, imprint)]
                    assert host.qtlx_columns(K, Ki, additive, imprint) == want, (K, Ki, additive, imprint)
                    seen.add((ne, Ki))
    assert {(3, 2), (2, 4), (1, 6), (1, 0), (3, 0)} <= seen
    assert host.qtlx_columns(2, 1, False, True) == [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (3, 1)]
    assert host.qtlx_columns(1, 1, True, True) == [(0, 0), (0, 1), (1, 0), (3, 0), (1, 1), (3, 1)]


def test_coef_names():
    assert qtl.coef_names() == ("a", "d")
    assert qtl.coef_names(additive=True) == ("a",)
    assert qtl.coef_names(2, True) == ("a", "d", "i", "a:z1", "d:z1", "i:z1", "a:z2", "d:z2", "i:z2")
    assert qtl.coef_names(1, True, True, cov_names=["sex", "batch"]) == ("a", "i", "a:sex", "i:sex")
    with pytest.raises(ValueError):
        qtl.coef_names(2, cov_names=["sex"])


def test_thresholdsx_on_hand_made_maxima():
    P, T, C = 20, 2, 3
    pm = np.zeros((P, T, C, 5))
    for s in range(5):
        for t in range(T):
            for c in range(C):
                pm[:, t, c, s] = ((np.arange(P) * (3, 7, 9, 11, 13, 17)[2 * c + t]) % P) + 100 * s + 10 * c + 0.5 * t
    th = qtl.thresholdsx(pm, alpha=(0.05, 0.5))
    assert th["alpha"] == (0.05, 0.5)
    for s, key in enumerate(("lod0", "lod1", "lod2", "imprint", "interaction")):
        one = qtl.thresholds(pm[..., s], alpha=(0.05, 0.5))
        assert np.array_equal(th[key]["genome"], one["genome"]) and np.array_equal(th[key]["chromosome"], one["chromosome"])
        assert th[key]["chromosome"].shape == (2, T, C) and th[key]["genome"].shape == (2, T)
        # P = 20: the 5 % threshold is the 19th of the ascending maxima, the 50 % one the 10th
        assert th[key]["chromosome"][0, 0, 0] == 100 * s + 18 and th[key]["chromosome"][1, 1, 2] == 100 * s + 20 + 0.5 + 9
    with pytest.raises(ValueError):
        qtl.thresholdsx(pm[..., :3])
    with pytest.raises(ValueError):
        qtl.thresholdsx(pm[:0])


# ---------------------------------------------------------------------------------------------- symbols
def test_new_symbols_in_both_libraries(host):
    from cnf2freq_amd import capi
    assert {"cnf2_qtl_scanx", "cnf2_set_qtlx_columns"} <= set(capi.SYMBOLS)
    assert {"cnf2h_qtlx_marker", "cnf2h_qtlx_column"} <= set(host.SYMBOLS)
    import ctypes
    hip = ctypes.CDLL(os.path.join(ROOT, "cnf2freq_amd", "libcnf2hip.so"))
    for s in ("cnf2_qtl_scanx", "cnf2_set_qtlx_columns"):
        assert getattr(hip, s)
    lib = host.load()
    for s in ("cnf2h_qtlx_marker", "cnf2h_qtlx_column"):
        assert getattr(lib, s)
    assert capi.QTL_IMPRINT == 1 << 25
    header = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    assert "CNF2_QTL_IMPRINT  = 1u << 25" in header and header.count("1u << 25") == 1


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
    base = ["--qtlx", "q.txt", "--phenofile", str(ph)]
    for extra, text in ((["--qtlx", "q.txt"], "--qtlx FILE needs --phenofile FILE"),
                        (["--qtl-imprint"], "--qtl-imprint and --qtl-interactive need --qtlx FILE"),
                        (["--qtl-interactive", "z0", "--qtl", "q.txt", "--phenofile", str(ph), "--qtl-covariates", "z0"],
                         "--qtl-imprint and --qtl-interactive need --qtlx FILE"),
                        (base + ["--gpus", "2"], "--qtlx needs a single GPU"),
                        (base + ["--qtl-interactive", "z0"], "--qtl-interactive: not among --qtl-covariates: z0"),
                        (base + ["--qtl-covariates", "z0", "--qtl-interactive", "z1,nothing"], "not among --qtl-covariates: z1 nothing"),
                        (base + ["--qtl-covariates", "z0,z1,z2", "--qtl-interactive", "z2,z1,z0", "--qtl-imprint"], "--qtlx: the design has 16 columns"),
                        (base + ["--qtl-covariates", "nothing"], "not a column of .*: nothing"),
                        (base + ["--qtl-permutations", "-1"], "must not be negative"),
                        # the existing messages, word for word
                        (["--phenofile", str(ph)], "--phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed and --qtl-additive need --qtl FILE or --qtl2 FILE$"),
                        (["--qtl-additive"], "--phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed and --qtl-additive need --qtl FILE or --qtl2 FILE$"),
                        (["--qtl", "q.txt"], "^--qtl FILE needs --phenofile FILE$"),
                        (["--qtl2", "q.txt"], "^--qtl2 FILE needs --phenofile FILE$"),
                        (["--qtl2-every", "2"], "^--qtl2-every needs --qtl2 FILE$")):
        r = run_cli(tmp_path, *extra)
        assert r.returncode == 2, (extra, r.returncode, r.stderr[-300:])
        assert re.search(text, r.stderr, re.M), (extra, r.stderr[-300:])
        assert not (tmp_path / "q.txt").exists()
