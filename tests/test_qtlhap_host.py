"""CPU suite: the host side of the founder-haplotype scan (cnf2h_qtlhap_marker of include/cnf2host.h, which fits one marker
serially through cnf2freq_amd/csrc/cnf2_qtlhap.h by the kernels' steps; qtl.hap_fstat; the declarations and exports; the command
line's option check) against tests/qtlhap_reference.py on the CPU oracle's descent rows.  What is compared, and where, is
asserted on the reference before the code under test runs."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import origins, qtl, synth
from descent_reference import founder_cross, oracle_descent
import qtlhap_reference as ref

ATOL = 1e-9
# synth.make_founder_cross arguments at which the reference keeps df = 6 of H = 8 and stays inside the conditioning rule
CROSSES = [(3, 12, 17, 2, 777, 0.2, 0.98), (4, 8, 33, 2, 777, 0.0, 1.0), (2, 9, 9, 2, 777, 0.2, 0.02)]


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    return h


def traits(n, T, seed):
    return np.random.default_rng(seed).normal(size=(n, T))


def serial_scan(host, descent, col, H, y, chromstarts, cov=None, use=None):
    """cnf2h_qtlhap_marker at every marker, assembled as cnf2_qtl_scan_hap reports: traits and covariates minus their means
    over the individuals in the model, the chromosome's mask from its first marker"""
    d = np.asarray(descent)
    n, M = d.shape[:2]
    y = y[:, None] if y.ndim == 1 else y
    cs = np.asarray(chromstarts)
    base = ref.in_model(col, H, use)
    yc = y - y[base].mean(axis=0)
    zc = None if cov is None else cov - cov[base].mean(axis=0)
    out = dict(lod=np.zeros((y.shape[1], M)), df=np.zeros(M, np.int32), coef=np.zeros((y.shape[1], M, H)),
               rss0=np.zeros((y.shape[1], len(cs) - 1)), n_used=np.zeros(len(cs) - 1, np.int32))
    for c in range(len(cs) - 1):
        cm = base & (d[:, cs[c]] != 0).any(axis=1)
        for m in range(cs[c], cs[c + 1]):
            r = host.qtlhap_marker(d[:, m], col, H, yc, zc, cm)
            out["lod"][:, m], out["df"][m], out["coef"][:, m] = r["lod"], r["df"], r["coef"]
            out["rss0"][:, c], out["n_used"][c] = r["rss0"], r["n_used"]
    return out


def compare(got, want, what):
    """df everywhere the reference is inside the rule; LOD and coefficients there; rss0 and n_used everywhere"""
    inside = want["inside"]
    assert np.array_equal(got["n_used"], want["n_used"]), what
    np.testing.assert_allclose(got["rss0"], want["rss0"], rtol=1e-12, atol=ATOL, err_msg=what)
    assert np.array_equal(got["df"][inside], want["df"][inside]), what
    err_lod = np.abs(got["lod"][:, inside] - want["lod"][:, inside]).max()
    gc, wc = got["coef"][:, inside], want["coef"][:, inside]
    assert np.array_equal(np.isnan(gc), np.isnan(wc)), what + ": the dropped columns"
    err_coef = np.nanmax(np.abs(gc - wc)) if np.isfinite(wc).any() else 0.0
    print("%s: %d of %d markers compared; largest difference lod %.3g, coef %.3g" % (what, inside.sum(), len(inside), err_lod, err_coef))
    assert err_lod <= ATOL and err_coef <= ATOL, what
    assert np.all(got["lod"] >= 0) and np.all(np.isfinite(got["lod"]))


@pytest.mark.parametrize("args", CROSSES)
@pytest.mark.parametrize("K", [0, 2])
def test_marker_against_reference_on_founder_crosses(host, args, K):
    ped, _, rows = founder_cross(args)
    d = rows["descent"]
    n = len(ped.dous)
    col, grand = origins.descent_columns(ped.par, ped.dous)
    H = 2 * len(grand)
    assert H == 8
    y = traits(n, 3, 5)
    cov = traits(n, K, 6) if K else None
    want = ref.scan(d, col, H, y, ped.chromstarts, cov)
    # the reference first: df = 6 of the 8 columns (each side's four add up to the intercept), nearly every marker inside the rule
    assert want["inside"].mean() >= 0.9, "at least 0.9 of the markers are compared"
    assert np.all(want["df"][want["inside"]] == 6)
    assert np.all(want["pivots"][want["inside"]][:, [3, 7]] <= ref.DROPPED_MAX), "the last column of each side is the dependent one"
    compare(serial_scan(host, d, col, H, y, ped.chromstarts, cov), want, "founder cross %s, K = %d" % (args[:3], K))


def test_founder_and_line_columns(host):
    ped, _, rows = founder_cross()
    n = len(ped.dous)
    y = traits(n, 2, 8)
    for by, H, df in (("founder", 4, 2), ("line", 2, 1)):
        col, _ = origins.descent_columns(ped.par, ped.dous, by)
        want = ref.scan(rows["descent"], col, H, y, ped.chromstarts)
        assert want["inside"].mean() >= 0.9 and np.all(want["df"][want["inside"]] == df)
        compare(serial_scan(host, rows["descent"], col, H, y, ped.chromstarts), want, "by " + by)


def test_reductions(host):
    """by="line" on an F2: Z_B - Z_A = 2 a and Z_A + Z_B = 2, so the fit is the additive line-cross model with df = 1; with one
    column the design is constant: df 0, lod 0"""
    ped = synth.make_f2(24, 12, 2, seed=4, missing=0.1)
    rows = oracle_descent(ped)
    n = len(ped.dous)
    assert rows["compared"] == n * 2
    y = traits(n, 2, 9)
    col, _ = origins.descent_columns(ped.par, ped.dous, "line")
    got = serial_scan(host, rows["descent"], col, 2, y, ped.chromstarts)
    assert np.all(got["df"] == 1)
    a = rows["origin"][:, :, 3] - rows["origin"][:, :, 0]
    for m in range(ped.n_markers):
        X = np.stack([np.ones(n), a[:, m]], axis=1)
        rss1 = ((y - X @ np.linalg.lstsq(X, y, rcond=None)[0]) ** 2).sum(axis=0)
        rss0 = ((y - y.mean(axis=0)) ** 2).sum(axis=0)
        np.testing.assert_allclose(got["lod"][:, m], 0.5 * n * np.log10(rss0 / rss1), rtol=0, atol=ATOL)
    one = serial_scan(host, rows["descent"], np.zeros((n, 8), np.int32), 1, y, ped.chromstarts)
    assert np.all(one["df"] == 0) and np.all(one["lod"] == 0) and np.isnan(one["coef"]).all()
    assert np.all(one["rss0"] > 0)


def test_no_residual_degree_of_freedom(host):
    """H = 8 keeps 6 columns: with n_c = 7 and K = 0 nothing is left over, with n_c = 8 one degree is"""
    ped, _, rows = founder_cross()
    col, _ = origins.descent_columns(ped.par, ped.dous)
    n = len(ped.dous)
    y = traits(n, 1, 3)
    d = rows["descent"][:, 3]
    for n_c, fitted in ((7, False), (8, True)):
        c = np.zeros(n, np.uint8)
        c[np.arange(n_c) * 4] = 1                # (spread over the three families)
        want = ref.marker(d, col, 8, y, None, c)
        assert want["inside"] and (want["pivots"] >= ref.PIVOT).sum() == 6
        r = host.qtlhap_marker(d, col, 8, y - y[c != 0].mean(axis=0), None, c)
        assert r["n_used"] == n_c and r["df"] == (6 if fitted else 0)
        assert (r["lod"][0] > 0) == fitted and np.isnan(r["coef"]).all() != fitted
        assert want["df"] == r["df"]


def test_unused_and_out_of_model_individuals(host):
    ped, _, rows = founder_cross()
    col, _ = origins.descent_columns(ped.par, ped.dous)
    col = col.copy()
    col[5, 2] = -1
    col[20, 4:] = -1
    n = len(ped.dous)
    use = np.ones(n, bool)
    use[[0, 7, 30]] = False
    y = traits(n, 2, 12)
    y[~use] = np.nan
    want = ref.scan(rows["descent"], col, 8, np.where(use[:, None], y, 0.0), ped.chromstarts, use=use)
    assert np.all(want["n_used"] == n - 5) and want["inside"].mean() >= 0.9
    compare(serial_scan(host, rows["descent"], col, 8, np.where(use[:, None], y, 0.0), ped.chromstarts, use=use), want, "unused and -1")


def test_marker_refusals(host):
    L = host.load()
    n, H, T = 6, 4, 2
    d, col, y = np.full((n, 8), 0.25), np.tile(np.array([0, 1, 2, 3, 0, 1, 2, 3], np.int32), (n, 1)), np.ones((n, T))
    c = np.ones(n, np.uint8)
    lod, df, coef, rss0, nu = np.full(T, 7.0), np.full(1, 7, np.int32), np.full((T, H), 7.0), np.full(T, 7.0), np.full(1, 7, np.int32)
    p = lambda a: a.ctypes.data
    good = [n, p(d), p(col), H, T, p(y), 0, None, p(c), p(lod), p(df), p(coef), p(rss0), p(nu)]
    assert L.cnf2h_qtlhap_marker(*good) == 0 and df[0] != 7
    lod[:], df[:], coef[:], rss0[:], nu[:] = 7, 7, 7, 7, 7
    bad_col = col.copy()
    bad_col[2, 3] = H
    low_col = col.copy()
    low_col[1, 0] = -2
    changes = [(0, 0), (1, None), (2, None), (3, 0), (3, 33), (4, 0), (5, None), (6, 9), (6, 1), (8, None), (9, None), (10, None),
               (12, None), (13, None), (2, p(bad_col)), (2, p(low_col))]
    for k, v in changes:
        args = list(good)
        args[k] = v
        assert L.cnf2h_qtlhap_marker(*args) == -2, (k, v)
        for a in (lod, df, coef, rss0, nu):
            assert np.all(a == 7)


def test_hap_fstat():
    lod = np.array([[0.0, 1.0, 2.0]])
    F, df1, df2 = qtl.hap_fstat(lod, np.array([0, 6, 4]), np.array([36]), 2, chromstarts=[0, 3])
    assert df1.tolist() == [[0, 6, 4]] and df2.tolist() == [[0, 27, 29]]
    assert np.isnan(F[0, 0])
    np.testing.assert_allclose(F[0, 1:], [(10 ** (2 / 36) - 1) * 27 / 6, (10 ** (4 / 36) - 1) * 29 / 4], rtol=1e-14)


def test_symbols_declared_and_exported(host):
    from cnf2freq_amd import capi
    hdr = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    assert re.search(r"\bint\s+cnf2_qtl_scan_hap\s*\(", hdr) and "cnf2_qtl_scan_hap" in capi.SYMBOLS
    assert hasattr(capi.load(), "cnf2_qtl_scan_hap")
    for method in ("qtl_scan_hap", "qtl_scan_hap_device"):
        assert hasattr(capi.Context, method)
    hhdr = open(os.path.join(ROOT, "include", "cnf2host.h")).read()
    assert re.search(r"\bint\s+cnf2h_qtlhap_marker\s*\(", hhdr) and "cnf2h_qtlhap_marker" in host.SYMBOLS
    assert hasattr(host.load(), "cnf2h_qtlhap_marker")
    assert callable(qtl.scan_hap) and callable(qtl.hap_fstat) and callable(qtl.descent_rows)
    assert "16 phased grandparents" in hdr


EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def test_cli_qtlhap_option_checks(host, tmp_path):
    base = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet"]
    pheno = tmp_path / "p.txt"
    pheno.write_text("id\ty\nC\t1.0\nD\t2.0\nF\t0.5\n")
    r = subprocess.run(base + ["--gpus", "2", "--qtlhap", "h.txt", "--phenofile", str(pheno)], capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    assert r.returncode == 2 and "single GPU" in r.stderr and "--qtlhap" in r.stderr
    r = subprocess.run(base + ["--qtlhap", "h.txt"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and "--phenofile" in r.stderr
    r = subprocess.run(base + ["--qtlhap", "h.txt", "--phenofile", str(pheno), "--qtl-hap-by", "strand"], capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and "--qtl-hap-by" in r.stderr
    assert not (tmp_path / "h.txt").exists()
