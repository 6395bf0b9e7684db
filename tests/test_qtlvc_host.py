"""CPU suite: the host side of the variance-component scan (cnf2h_qtlvc_marker of include/cnf2host.h, which fits one marker
serially through cnf2freq_amd/csrc/cnf2_qtlvc.h by the kernels' steps; the declarations and exports; the command line's option
checks) against tests/qtlvc_reference.py on the CPU oracle's descent rows.  Which cells are compared is asserted on the
reference before the code under test runs.  The residual variance is compared at the h the fit returned, as the BLUP is: see
tests/qtlvc_reference.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import origins, qtl, synth
from descent_reference import founder_cross, oracle_descent
import qtlhap_reference as hapref
import qtlvc_reference as ref
from test_qtlhap_host import CROSSES, traits

ATOL = 1e-9


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    return h


def serial_scan(host, descent, col, H, y, chromstarts, cov=None, use=None):
    """cnf2h_qtlvc_marker at every marker, assembled as cnf2_qtl_scan_vc reports: traits and covariates minus their means over
    the individuals in the model, the chromosome's mask from its first marker"""
    d = np.asarray(descent)
    n, M = d.shape[:2]
    y = y[:, None] if y.ndim == 1 else y
    T = y.shape[1]
    cs = np.asarray(chromstarts)
    base = ref.in_model(col, H, use)
    yc = y - y[base].mean(axis=0)
    zc = None if cov is None else cov - cov[base].mean(axis=0)
    out = dict(lod=np.zeros((T, M)), h=np.zeros((T, M)), sigma2=np.zeros((T, M)), blup=np.zeros((T, M, H)), eval=np.zeros((M, H)),
               rank=np.zeros(M, np.int32), rss0=np.zeros((T, len(cs) - 1)), n_used=np.zeros(len(cs) - 1, np.int32))
    for c in range(len(cs) - 1):
        cm = base & (d[:, cs[c]] != 0).any(axis=1)
        for m in range(cs[c], cs[c + 1]):
            r = host.qtlvc_marker(d[:, m], col, H, yc, zc, cm)
            for k in ("lod", "h", "sigma2", "blup"):
                out[k][:, m] = r[k]
            out["eval"][m], out["rank"][m] = r["eval"], r["rank"]
            out["rss0"][:, c], out["n_used"][c] = r["rss0"], r["n_used"]
    return out


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
    assert want["compared"].mean() >= 0.9, "at least 0.9 of the cells are compared"
    got = serial_scan(host, d, col, H, y, ped.chromstarts, cov)
    ref.check(got, want, "founder cross %s, K = %d" % (args[:3], K))
    # the rank is the fixed-effects scan's df wherever that reference is inside its conditioning rule
    hap = hapref.scan(d, col, H, y, ped.chromstarts, cov)
    inside = hap["inside"]
    assert inside.mean() >= 0.9
    cs = ped.chromstarts
    for c in range(len(cs) - 1):
        cm = ref.in_model(col, H) & (d[:, cs[c]] != 0).any(axis=1)
        for m in range(cs[c], cs[c + 1]):
            if inside[m]:
                df = host.qtlhap_marker(d[:, m], col, H, y - y.mean(axis=0), None if cov is None else cov - cov.mean(axis=0), cm)["df"]
                assert got["rank"][m] == df, m


def test_one_column(host):
    """H = 1: Z is 2 c_i, W = 0: rank 0, lod 0, h 0, blup 0"""
    ped, _, rows = founder_cross()
    n = len(ped.dous)
    y = traits(n, 2, 9)
    got = serial_scan(host, rows["descent"], np.zeros((n, 8), np.int32), 1, y, ped.chromstarts)
    assert np.all(got["rank"] == 0) and np.all(got["lod"] == 0) and np.all(got["h"] == 0) and np.all(got["blup"] == 0)
    assert np.all(got["rss0"] > 0) and np.all(np.abs(got["eval"]) <= 1e-12 * 4 * n)
    np.testing.assert_allclose(got["sigma2"], np.repeat(got["rss0"] / (n - 1), np.diff(ped.chromstarts), axis=1), rtol=1e-14)


def test_duplicate_columns_of_an_f2(host):
    """An F2 by "haplotype": the two strands of a founder have equal cells wherever the sweep cannot tell them apart, so
    columns are duplicates and eigenvalues repeat; the iteration converges and agrees with the reference"""
    ped = synth.make_f2(24, 12, 2, seed=4, missing=0.1)
    rows = oracle_descent(ped)
    n = len(ped.dous)
    col, grand = origins.descent_columns(ped.par, ped.dous)
    H = 2 * len(grand)
    y = traits(n, 2, 9)
    want = ref.scan(rows["descent"], col, H, y, ped.chromstarts)
    assert want["compared"].mean() >= 0.9
    got = serial_scan(host, rows["descent"], col, H, y, ped.chromstarts)
    ref.check(got, want, "F2 by haplotype, H = %d" % H)
    assert np.all(got["rank"] < H)


def test_units_and_offsets(host):
    """y -> 3 y + 7 leaves LOD and h unchanged and multiplies the BLUP by 3 (the scan centres the traits: so does serial_scan)"""
    ped, _, rows = founder_cross()
    n = len(ped.dous)
    col, _ = origins.descent_columns(ped.par, ped.dous)
    y = traits(n, 3, 5)
    a = serial_scan(host, rows["descent"], col, 8, y, ped.chromstarts)
    b = serial_scan(host, rows["descent"], col, 8, 3.0 * y + 7.0, ped.chromstarts)
    assert (a["lod"] > 0).any()
    np.testing.assert_allclose(b["lod"], a["lod"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(b["h"], a["h"], rtol=0, atol=1e-5)
    # (the BLUP has a slope in h: compared where both fits stopped at the same h to 1e-9)
    same = np.abs(a["h"] - b["h"]) <= 1e-9
    assert same.mean() >= 0.9
    np.testing.assert_allclose(b["blup"][same], 3.0 * a["blup"][same], rtol=0, atol=ATOL * max(1.0, np.abs(a["blup"]).max()) * 3)
    np.testing.assert_allclose(b["sigma2"][same], 9.0 * a["sigma2"][same], rtol=1e-8)


def test_planted_truth_on_the_oracle_rows(host):
    """The planted trait of the founder-haplotype suite (its cross, effects, noise and seed) on the CPU oracle's descent rows:
    the reference's maximum is at the planted marker -- this is where the seed was chosen -- and so is the serial fit's, with
    the reference's LOD.  tests/test_gpu_qtlvc.py asserts the same of the GPU run through the real sweep."""
    from test_gpu_qtlhap import PLANT_ARGS, PLANT_BETA, PLANT_MARKER, PLANT_NOISE, PLANT_SEED
    ped, truth, rows = founder_cross(PLANT_ARGS)
    n = len(ped.dous)
    Z = np.zeros((n, 8))
    for s in range(2):
        np.add.at(Z, (np.arange(n), 4 * s + truth[:, s, PLANT_MARKER]), 1.0)
    y = Z @ PLANT_BETA + PLANT_NOISE * np.random.default_rng(PLANT_SEED).normal(size=n)
    col, _ = origins.descent_columns(ped.par, ped.dous)
    want = ref.scan(rows["descent"], col, 8, y, ped.chromstarts)
    assert int(want["lod"][0].argmax()) == PLANT_MARKER and want["lod"][0].max() > 10.0
    got = serial_scan(host, rows["descent"], col, 8, y, ped.chromstarts)
    ref.check(got, want, "planted trait")
    assert int(got["lod"][0].argmax()) == PLANT_MARKER


def test_marker_refusals(host):
    L = host.load()
    n, H, T = 6, 4, 2
    d, col, y = np.full((n, 8), 0.25), np.tile(np.array([0, 1, 2, 3, 0, 1, 2, 3], np.int32), (n, 1)), np.ones((n, T))
    c = np.ones(n, np.uint8)
    lod, h, s2, blup, ev = np.full(T, 7.0), np.full(T, 7.0), np.full(T, 7.0), np.full((T, H), 7.0), np.full(H, 7.0)
    rank, rss0, nu = np.full(1, 7, np.int32), np.full(T, 7.0), np.full(1, 7, np.int32)
    outs = (lod, h, s2, blup, ev, rank, rss0, nu)
    p = lambda a: a.ctypes.data
    good = [n, p(d), p(col), H, T, p(y), 0, None, p(c)] + [p(a) for a in outs]
    assert L.cnf2h_qtlvc_marker(*good) == 0 and rank[0] != 7
    for a in outs:
        a[...] = 7
    bad_col = col.copy()
    bad_col[2, 3] = H
    low_col = col.copy()
    low_col[1, 0] = -2
    changes = [(0, 0), (1, None), (2, None), (3, 0), (3, 65), (4, 0), (5, None), (6, 9), (6, 1), (8, None), (9, None), (10, None), (11, None),
               (14, None), (15, None), (16, None), (2, p(bad_col)), (2, p(low_col))]
    for k, v in changes:
        args = list(good)
        args[k] = v
        assert L.cnf2h_qtlvc_marker(*args) == -2, (k, v)
        for a in outs:
            assert np.all(a == 7)
    # 64 columns are taken
    col64 = (col + 4 * (np.arange(n)[:, None] % 16)).astype(np.int32)
    big = np.zeros((T, 64))
    args = list(good)
    args[2], args[3], args[12], args[13] = p(col64), 64, p(big), p(np.zeros(64))
    assert L.cnf2h_qtlvc_marker(*args) == 0


def test_symbols_declared_and_exported(host):
    from cnf2freq_amd import capi
    hdr = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    assert re.search(r"\bint\s+cnf2_qtl_scan_vc\s*\(", hdr) and "cnf2_qtl_scan_vc" in capi.SYMBOLS
    assert hasattr(capi.load(), "cnf2_qtl_scan_vc")
    for method in ("qtl_scan_vc", "qtl_scan_vc_device"):
        assert hasattr(capi.Context, method)
    hhdr = open(os.path.join(ROOT, "include", "cnf2host.h")).read()
    assert re.search(r"\bint\s+cnf2h_qtlvc_marker\s*\(", hhdr) and "cnf2h_qtlvc_marker" in host.SYMBOLS
    assert hasattr(host.load(), "cnf2h_qtlvc_marker")
    assert callable(qtl.scan_vc)


EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def test_cli_qtlvc_option_checks(host, tmp_path):
    base = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet"]
    pheno = tmp_path / "p.txt"
    pheno.write_text("id\ty\nC\t1.0\nD\t2.0\nF\t0.5\n")
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    r = run("--gpus", "2", "--qtlvc", "v.txt", "--phenofile", str(pheno))
    assert r.returncode == 2 and "single GPU" in r.stderr and "--qtlvc" in r.stderr
    r = run("--qtlvc", "v.txt")
    assert r.returncode == 2 and "--phenofile" in r.stderr
    r = run("--qtlvc", "v.txt", "--phenofile", str(pheno), "--qtl-vc-by", "strand")
    assert r.returncode == 2 and "--qtl-vc-by" in r.stderr
    r = run("--qtl-vc-by", "line")
    assert r.returncode == 2 and "--qtl-vc-by needs --qtlvc" in r.stderr
    # --qtl-hap-by and its messages stay as they are
    r = run("--qtlvc", "v.txt", "--phenofile", str(pheno), "--qtl-hap-by", "line")
    assert r.returncode == 2 and "--qtl-hap-by needs --qtlhap" in r.stderr
    assert not (tmp_path / "v.txt").exists()
