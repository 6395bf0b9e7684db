"""CPU tests of the maximum-likelihood scan: cnf2_qtlem.h compiled for the host and run through cnf2h_qtlem_fit, one (marker,
column) cell at a time, against the yardstick tests/qtlem_reference.py; scan_em's argument checks, the command line's usage
errors for the new flags and the exported symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qtlem_reference as R
from conftest import ROOT
from cnf2freq_amd import qtl

EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
CS = R.chromstarts_of(R.CHROM_LENS)


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


class _Lazy:
    """cnf2freq_amd.host / capi once the build has run"""
    def __init__(self, name):
        self.name = name

    def __getattr__(self, key):
        import importlib
        return getattr(importlib.import_module("cnf2freq_amd." + self.name), key)


host, capi = _Lazy("host"), _Lazy("capi")


def host_scan(origin, pheno, use=None, cov=None, perm=None, imprint=False, additive=False, max_iter=1000, tol=1e-6):
    """the scan of cnf2_qtl_scan_em cell by cell through cnf2h_qtlem_fit: the dict Context.qtl_scan_em returns"""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    Cn = len(CS) - 1
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    z = None if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    Y = R.columns(np.where(use[:, None], np.asarray(pheno, np.float64).reshape(n, -1), 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    ne = len(R.effects(additive, imprint))
    out = dict(lod=np.zeros((T, M)), coef=np.zeros((T, M, ne)), sigma2=np.zeros((T, M)), iters=np.zeros((T, M), np.int32),
               status=np.zeros((T, M), np.int32), rank=np.zeros(M, np.int32), rss0=np.zeros((T, Cn)),
               n_used=np.zeros(Cn, np.int32), perm_max=np.zeros((Q - 1, T, Cn)) if Q > 1 else None)
    for c in range(Cn):
        mask = use & (o[:, CS[c]] != 0.0).any(axis=1)
        for m in range(CS[c], CS[c + 1]):
            for q in range(Q):
                for t in range(T):
                    f = host.qtlem_fit(o[:, m], Y[:, q, t], z, mask, additive, imprint, max_iter, tol)
                    if q == 0:
                        for key in ("lod", "sigma2", "iters", "status", "coef"):
                            out[key][t, m] = f[key]
                        out["rank"][m], out["n_used"][c], out["rss0"][t, c] = f["rank"], f["n_used"], f["rss0"]
                    else:
                        out["perm_max"][q - 1, t, c] = max(out["perm_max"][q - 1, t, c], f["lod"])
    return out


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "n%d-K%d-%s%s-it%d" % (c[0], c[1], "i" if c[2] else "", "a" if c[3] else "", c[9]))
def test_fixed_iterations(case):
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    ref = R.case_reference(case)
    R.compared_markers(ref, CS)              # the precondition, on the reference alone, before the product runs
    origin, pheno, cov, use, perm = R.make_case(*case)
    got = host_scan(origin, pheno, use, cov, perm, imprint, additive, max_iter, -1.0)
    R.compare_em(got, ref, CS, "host %s" % (case,))
    fitted = got["rank"] > 0
    assert np.all(got["iters"][:, fitted] == max_iter) and np.all(got["status"][:, fitted] == 1)


def test_stopping_rule_and_not_haley_knott():
    p = R.PLANTED
    ref = R.planted_reference()
    origin, _, pheno, z = R.planted_case()
    # on the reference alone: few cells at the edge of the rule; the method differs from Haley-Knott and finds the locus
    assert ref["near"].mean() <= 0.01
    hk = R.reference_scan(origin, CS, pheno, cov=z)["lod"][0, 0]
    em = ref["lod"][0, 0]
    print("EM peak %.2f at %d, HK peak %.2f at %d, largest difference %.2f, iterations %d .. %d" %
          (em.max(), em.argmax(), hk.max(), hk.argmax(), np.abs(em - hk).max(), ref["iters"].min(), ref["iters"].max()))
    assert np.abs(em - hk).max() > 0.5 and em.argmax() == p["marker"] and hk.argmax() == p["marker"]
    got = host_scan(origin, pheno, None, z, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_em(got, ref, CS, "host planted")
    assert got["lod"][0].argmax() == p["marker"]
    short = host_scan(origin, pheno, None, z, max_iter=p["short"], tol=p["tol"])
    ok = ~ref["near"]
    assert np.array_equal((short["status"] == 1)[ok], (ref["iters"] > p["short"])[ok])


def test_monotone():
    ref = R.monotone_reference()
    steps = ref["trace"][0][:, list(R.MONOTONE)]
    assert np.all(np.diff(steps, axis=1) >= -1e-12)
    origin, _, pheno, z = R.planted_case()
    lods = np.stack([host_scan(origin, pheno, None, z, max_iter=k, tol=-1.0)["lod"][0] for k in R.MONOTONE], axis=1)
    assert np.all(np.diff(lods, axis=1) >= -1e-12)
    assert np.abs(lods - steps).max() <= R.ATOL


def test_degenerate_and_extreme():
    origin, at = R.degenerate_rows()
    n = origin.shape[0]
    y = R.noise(n, 1, 11)[:, 0]
    fit = lambda m, **kw: host.qtlem_fit(origin[:, m], y, **kw)
    f = fit(at["flat"], imprint=True)
    assert f["rank"] == 0 and f["lod"] == 0.0 and f["iters"] == 0 and f["status"] == 0 and np.isnan(f["coef"]).all()
    f = fit(at["homozygous"], imprint=True)
    assert f["rank"] == 1 and np.isfinite(f["coef"][0]) and np.isnan(f["coef"][1:]).all()
    f, g = fit(at["symmetric"], imprint=True), fit(at["symmetric"])
    assert f["rank"] == 2 and np.isnan(f["coef"][2]) and f["lod"] == g["lod"] and np.array_equal(f["coef"][:2], g["coef"])
    f = fit(at["zeros"], imprint=True)
    assert f["rank"] == 3 and np.isfinite([f["lod"], f["sigma2"]]).all() and np.isfinite(f["coef"]).all()
    # n_c = W: not scanned (W = 1 + 1 + 3)
    z = R.noise(n, 1, 12)
    c = np.zeros(n, np.uint8)
    c[:5] = 1
    f = host.qtlem_fit(origin[:, 8], y, z, c, imprint=True)
    assert f["n_used"] == 5 and f["rank"] == 0 and f["lod"] == 0.0 and np.isnan(f["coef"]).all()
    # a constant phenotype: RSS0 exactly 0 (n_c = 16 has an exact square root, so the null design's sums are exact)
    f = host.qtlem_fit(origin[:16, 8], np.full(16, 2.0))
    assert f["rss0"] == 0.0 and f["lod"] == 0.0 and np.isnan(f["coef"]).all() and f["iters"] == 0
    # a covariate that is constant over everybody: X0 is singular
    f = host.qtlem_fit(origin[:16, 8], y[:16], np.full((16, 1), 0.5))
    assert f["rank"] == 0 and f["lod"] == 0.0 and np.isnan(f["coef"]).all()


def test_outlier():
    origin, _ = R.degenerate_rows()
    y = R.outlier_pheno()
    ref = R.reference_scan_em(origin, CS, y, imprint=True, max_iter=50, tol=1e-7)
    got = host_scan(origin, y, imprint=True, max_iter=50, tol=1e-7)
    for key in ("lod", "sigma2", "rss0"):
        assert np.isfinite(got[key][:, got["rank"] > 0] if key != "rss0" else got[key]).all()
    R.compare_em(got, ref, CS, "host outlier", share=0.9, strict=False)


def test_refused_arguments():
    o, y = np.full((8, 4), 0.25), np.arange(8.0)
    for kw in (dict(max_iter=0), dict(max_iter=10001), dict(tol=np.nan), dict(tol=np.inf), dict(cov=np.zeros((8, 9)))):
        with pytest.raises(RuntimeError):
            host.qtlem_fit(o, y, **kw)


class _Ctx:
    n_ind, n_markers, n_chrom = 6, 3, 1


def test_scan_em_argument_checks():
    y = np.zeros((6, 1))
    with pytest.raises(ValueError):
        qtl.scan_em(_Ctx(), np.zeros((5, 1)))
    with pytest.raises(ValueError):
        qtl.scan_em(_Ctx(), y, max_iter=0)
    with pytest.raises(ValueError):
        qtl.scan_em(_Ctx(), y, max_iter=10001)
    with pytest.raises(ValueError):
        qtl.scan_em(_Ctx(), y, tol=np.nan)
    with pytest.raises(ValueError):
        qtl.scan_em(_Ctx(), y, tol=np.inf)


def test_symbols():
    assert "cnf2_qtl_scan_em" in capi.SYMBOLS and "cnf2_set_qtlem_columns" in capi.SYMBOLS and "cnf2h_qtlem_fit" in host.SYMBOLS
    L = C.CDLL(host.LIB_PATH)
    assert hasattr(L, "cnf2h_qtlem_fit")
    G = C.CDLL(capi.LIB_PATH)
    assert hasattr(G, "cnf2_qtl_scan_em") and hasattr(G, "cnf2_set_qtlem_columns")


def test_command_line_usage_errors(tmp_path):
    """every one of these ends with status 2 and a message before a GPU is asked for; the existing messages keep their text"""
    ph = tmp_path / "p.txt"
    ph.write_text("id weight z\nC 1.0 1\nD NA 2\nF 2.5 3\n")
    files = [os.path.join(DEMO, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    base = ["--qtlem", "q.txt", "--phenofile", str(ph)]
    for extra, text in ((["--qtlem", "q.txt"], "--qtlem FILE needs --phenofile FILE"),
                        (["--qtl-em-iterations", "5"], "--qtl-em-iterations and --qtl-em-tol need --qtlem FILE"),
                        (["--qtl-em-tol", "1e-5"], "--qtl-em-iterations and --qtl-em-tol need --qtlem FILE"),
                        (base + ["--qtl-em-iterations", "0"], "--qtl-em-iterations must be 1 .. 10000"),
                        (base + ["--qtl-em-iterations", "10001"], "--qtl-em-iterations must be 1 .. 10000"),
                        (base + ["--qtl-em-tol", "nan"], "--qtl-em-tol needs a finite number"),
                        (base + ["--qtl-em-tol", "inf"], "--qtl-em-tol needs a finite number"),
                        (base + ["--qtl-em-tol", "x"], "--qtl-em-tol needs a finite number"),
                        (base + ["--qtl-interactive", "z", "--qtl-covariates", "z"], "--qtl-imprint and --qtl-interactive need --qtlx FILE"),
                        (base + ["--gpus", "2"], "--qtlem needs a single GPU"),
                        (["--qtl-imprint"], "--qtl-imprint and --qtl-interactive need --qtlx FILE"),
                        (["--phenofile", str(ph)], "--phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed and --qtl-additive need --qtl FILE or --qtl2 FILE")):
        args = [EXE, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--count", "1", "--quiet", *extra]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 2 and text in r.stderr, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "q.txt").exists()
