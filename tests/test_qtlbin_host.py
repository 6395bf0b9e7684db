"""CPU tests of the binary-trait scan: cnf2_qtlbin.h compiled for the host and run through cnf2h_qtlbin_fit, one (marker,
column) cell at a time, against the yardstick tests/qtlbin_reference.py; the yardstick's own anchor, scan_binary's argument
checks, the command line's usage errors for the new flags and the exported symbols; at the end the cases of every width of
X0 and of the design (a, i), and two edges of the walk over the individuals, as tests/test_gpu_qtlbin.py runs them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qtlbin_reference as R
from conftest import ROOT
from cnf2freq_amd import qtl

EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
CS = R.chromstarts_of(R.CHROM_LENS)
HOST_CASES = (R.CASES[0], R.CASES[2])        # n = 41, K = 2, two traits; n = 67, K = 2, imprint, skipped individuals, P = 1


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


def host_scan(origin, pheno, use=None, cov=None, perm=None, imprint=False, additive=False, max_iter=50, tol=1e-7):
    """the scan of cnf2_qtl_scan_binary cell by cell through cnf2h_qtlbin_fit: the dict Context.qtl_scan_binary returns"""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    Cn = len(CS) - 1
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    z = None if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    Y = R.columns(np.where(use[:, None], np.asarray(pheno, np.float64).reshape(n, -1), 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    ne = len(R.effects(additive, imprint))
    out = dict(lod=np.zeros((T, M)), coef=np.zeros((T, M, ne)), iters=np.zeros((T, M), np.int32),
               status=np.zeros((T, M), np.int32), rank=np.zeros(M, np.int32), ll0=np.zeros((T, Cn)),
               n_ones=np.zeros((T, Cn), np.int32), n_used=np.zeros(Cn, np.int32), perm_max=np.zeros((Q - 1, T, Cn)) if Q > 1 else None)
    for c in range(Cn):
        mask = use & (o[:, CS[c]] != 0.0).any(axis=1)
        for m in range(CS[c], CS[c + 1]):
            for q in range(Q):
                for t in range(T):
                    f = host.qtlbin_fit(o[:, m], Y[:, q, t], z, mask, additive, imprint, max_iter, tol)
                    if q == 0:
                        for key in ("lod", "iters", "status", "coef"):
                            out[key][t, m] = f[key]
                        out["rank"][m], out["n_used"][c] = f["rank"], f["n_used"]
                        out["ll0"][t, c], out["n_ones"][t, c] = f["ll0"], f["n_ones"]
                    else:
                        out["perm_max"][q - 1, t, c] = max(out["perm_max"][q - 1, t, c], f["lod"])
    return out


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: "n%d-K%d-%s%s" % (c[0], c[1], "i" if c[2] else "", "a" if c[3] else ""))
@pytest.mark.parametrize("max_iter", (1, 2, 3, 5))
def test_fixed_iterations(case, max_iter):
    n, K, imprint, additive, seed, T, P, mask, skipped, _ = case
    ref = R.case_reference(case, max_iter, -1.0)
    R.compared_cells(ref, CS)                # the precondition, on the reference alone, before the product runs
    origin, pheno, cov, use, perm = R.make_case(*case)
    got = host_scan(origin, pheno, use, cov, perm, imprint, additive, max_iter, -1.0)
    R.compare_bin(got, ref, CS, "host %s at %d iterations" % (case, max_iter))
    fitted = got["rank"] > 0
    assert np.all(got["iters"][:, fitted] == max_iter) and np.all(got["status"][:, fitted] == 1)


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: "n%d-K%d-%s%s" % (c[0], c[1], "i" if c[2] else "", "a" if c[3] else ""))
def test_stopping_rule(case):
    n, K, imprint, additive, seed, T, P, mask, skipped, _ = case
    ref = R.case_reference(case, 50, 1e-7)
    # on the yardstick alone, before the product runs: its converged likelihood is that of the longdouble Newton run from
    # theta = 0, and nearly all cells are compared
    R.assert_anchor(ref, "case n = %d" % n)
    R.assert_conditions([R.case_reference(c, 50, 1e-7) for c in HOST_CASES])
    R.compared_cells(ref, CS)
    origin, pheno, cov, use, perm = R.make_case(*case)
    got = host_scan(origin, pheno, use, cov, perm, imprint, additive, 50, 1e-7)
    R.compare_bin(got, ref, CS, "host %s to tol" % (case,))
    assert np.all(got["status"] == 0) and got["iters"].max() <= 10


def test_planted_not_haley_knott():
    p = R.PLANTED
    ref, hk = R.planted_reference(), R.planted_linear_reference()
    R.assert_anchor(ref, "planted")                        # on the yardstick alone, before the product runs
    R.assert_conditions([ref])
    R.assert_conditions([R.case_reference(case) for case in R.CASES])
    R.assert_planted(ref, hk)
    origin, _, pheno, z = R.planted_case()
    got = host_scan(origin, pheno, None, z, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_bin(got, ref, CS, "host planted")
    assert got["lod"][0].argmax() == p["marker"]
    short = host_scan(origin, pheno, None, z, max_iter=p["short"], tol=p["tol"])
    ok = ~ref["near"]
    assert np.array_equal((short["status"] == 1)[ok], (ref["iters"] > p["short"])[ok])
    assert np.array_equal(short["iters"][ok], np.minimum(ref["iters"], p["short"])[ok])


def test_monotone():
    ref = R.monotone_reference()
    steps = ref["trace"][0][:, list(R.MONOTONE)]
    assert np.all(np.diff(steps, axis=1) >= -1e-12)
    origin, _, pheno, z = R.planted_case()
    lods = np.stack([host_scan(origin, pheno, None, z, max_iter=k, tol=-1.0)["lod"][0] for k in R.MONOTONE], axis=1)
    assert np.all(np.diff(lods, axis=1) >= -1e-12)
    assert np.abs(lods - steps).max() <= R.ATOL


def test_invariant_to_shift_and_rescale_of_the_covariates():
    case = R.CASES[0]
    origin, pheno, cov, use, perm = R.make_case(*case)
    base = host_scan(origin, pheno[:, :1], use, cov)
    moved = host_scan(origin, pheno[:, :1], use, cov * np.array([1e3, 1e-3]) + np.array([1e6, -40.0]))
    err = np.abs(base["lod"] - moved["lod"]).max()
    print("lod under a shift and rescale of the covariates: %.3g" % err)
    err_0 = np.abs(base["ll0"] - moved["ll0"]).max()
    print("ll0 under the same: %.3g" % err_0)
    # (the covariates are centred; what is left is the rounding of cov * s + t itself, 1e6 * 2^-53 against a spread of 1e3:
    # about 1e-13 relative, far inside ATOL)
    assert err <= R.ATOL and err_0 <= R.ATOL
    assert np.array_equal(base["rank"], moved["rank"]) and np.array_equal(base["iters"], moved["iters"])


def test_degenerate_and_extreme():
    origin, at = R.degenerate_rows()
    n = origin.shape[0]
    y = R.bernoulli(np.zeros((n, 1)), 11)[:, 0]
    assert 0 < y.sum() < n
    fit = lambda m, **kw: host.qtlbin_fit(origin[:, m], y, **kw)
    f = fit(at["flat"], imprint=True)
    assert f["rank"] == 0 and f["lod"] == 0.0 and f["iters"] == 0 and f["status"] == 0 and np.isnan(f["coef"]).all() and f["ll0"] < 0
    f = fit(at["homozygous"], imprint=True)
    assert f["rank"] == 1 and np.isfinite(f["coef"][0]) and np.isnan(f["coef"][1:]).all()
    f, g = fit(at["symmetric"], imprint=True), fit(at["symmetric"])
    assert f["rank"] == 2 and np.isnan(f["coef"][2]) and f["lod"] == g["lod"] and np.array_equal(f["coef"][:2], g["coef"])
    f = fit(at["zeros"], imprint=True)
    assert f["rank"] == 3 and np.isfinite(f["lod"]) and f["status"] in (0, 1, 2)
    # K = 0: the null fit is the closed form
    n1 = y.sum()
    assert abs(f["ll0"] - (n1 * np.log(n1 / n) + (n - n1) * np.log((n - n1) / n))) <= R.ATOL
    # n_c = W: not scanned (W = 1 + 1 + 3); n_c = W + 1 is
    z = R.noise(n, 1, 12)
    c = np.zeros(n, np.uint8)
    c[:5] = 1
    yy = y.copy()
    yy[:6] = [0, 1, 0, 1, 1, 0]
    f = host.qtlbin_fit(origin[:, 8], yy, z, c, imprint=True)
    assert f["n_used"] == 5 and f["rank"] == 0 and f["lod"] == 0.0 and np.isnan(f["coef"]).all() and f["ll0"] == 0.0
    c[5] = 1
    assert host.qtlbin_fit(origin[:, 8], yy, z, c, imprint=True)["rank"] == 3
    # additive: W + 1 = K + 3 individuals are enough
    c[:] = 0
    c[:4] = 1
    assert host.qtlbin_fit(origin[:, 8], yy, z, c, additive=True)["rank"] == 1
    # a trait that is constant under the mask: not scanned, but the rank is the design's
    f = host.qtlbin_fit(origin[:16, 8], np.ones(16))
    assert f["ll0"] == 0.0 and f["lod"] == 0.0 and np.isnan(f["coef"]).all() and f["iters"] == 0 and f["n_ones"] == 16 and f["rank"] == 2
    # a covariate that is constant over everybody: X0 is singular
    f = host.qtlbin_fit(origin[:16, 8], y[:16], np.full((16, 1), 0.5))
    assert f["rank"] == 0 and f["lod"] == 0.0 and np.isnan(f["coef"]).all() and f["ll0"] == 0.0
    # a huge covariate: eta of +-700 and beyond gives finite outputs
    big = np.where(y > 0, 1.0, -1.0)[:, None] * 700.0 + R.noise(n, 1, 13)
    f = host.qtlbin_fit(origin[:, 8], y, big)
    assert np.isfinite([f["lod"], f["ll0"]]).all() and f["lod"] >= 0.0 and f["status"] in (0, 1, 2)


def test_separated():
    origin, y, z = R.separated_case()
    ref = R.reference_scan_binary(origin, CS, y, None, z, imprint=True, max_iter=50, tol=1e-7)
    assert (np.abs(np.nan_to_num(ref["coef"])) > 15).any() or (ref["status"] == 2).any(), "the reference shows diverging coefficients"
    got = host_scan(origin, y, None, z, imprint=True, max_iter=50, tol=1e-7)
    scanned = got["ll0"] < 0
    assert scanned.any()
    bound = np.repeat(-got["ll0"] / np.log(10.0) + R.ATOL, np.diff(CS), axis=1)
    assert np.isfinite(got["lod"]).all() and np.all(got["lod"] >= 0) and np.all(got["lod"] <= bound)
    assert np.isin(got["status"], (0, 1, 2)).all()
    # nothing is NaN except the coefficients of dropped effects (read off the reference where its pivots are clear)
    cm = R.compared_cells(dict(ref, maxeta=np.zeros_like(ref["maxeta"])), CS, share=0.9, strict=False)[0]
    assert np.array_equal(np.isnan(got["coef"][:, cm]), np.isnan(ref["coef"][:, cm]))
    sc = np.repeat(scanned, np.diff(CS), axis=1)
    assert np.all((np.isnan(got["coef"]).sum(axis=2) == 3 - got["rank"][None, :])[sc])


def test_refused_arguments():
    o, y = np.full((8, 4), 0.25), np.array([0, 1, 0, 1, 1, 0, 1, 0.0])
    for kw in (dict(max_iter=0), dict(max_iter=1001), dict(tol=np.nan), dict(tol=np.inf), dict(cov=np.zeros((8, 9)))):
        with pytest.raises(RuntimeError):
            host.qtlbin_fit(o, y, **kw)
    for bad in (0.5, 2.0, np.nan, -1.0):
        yb = y.copy()
        yb[3] = bad
        with pytest.raises(RuntimeError):
            host.qtlbin_fit(o, yb)
        c = np.ones(8, np.uint8)
        c[3] = 0
        host.qtlbin_fit(o, yb, c=c)          # the same value at an individual outside the mask is accepted


class _Ctx:
    n_ind, n_markers, n_chrom = 6, 3, 1


def test_scan_binary_argument_checks():
    y = np.array([[0.0], [1.0], [0.0], [1.0], [np.nan], [1.0]])
    with pytest.raises(ValueError):
        qtl.scan_binary(_Ctx(), np.zeros((5, 1)))
    for kw in (dict(max_iter=0), dict(max_iter=1001), dict(tol=np.nan), dict(tol=np.inf)):
        with pytest.raises(ValueError):
            qtl.scan_binary(_Ctx(), y, **kw)
    for bad in (0.5, 2.0, -1.0, 1e-300):
        yb = y.copy()
        yb[2] = bad
        with pytest.raises(ValueError):
            qtl.scan_binary(_Ctx(), yb)


def test_symbols():
    assert "cnf2_qtl_scan_binary" in capi.SYMBOLS and "cnf2_set_qtlbin_columns" in capi.SYMBOLS and "cnf2h_qtlbin_fit" in host.SYMBOLS
    L = C.CDLL(host.LIB_PATH)
    assert hasattr(L, "cnf2h_qtlbin_fit")
    G = C.CDLL(capi.LIB_PATH)
    assert hasattr(G, "cnf2_qtl_scan_binary") and hasattr(G, "cnf2_set_qtlbin_columns")


def test_command_line_usage_errors(tmp_path):
    """every one of these ends with status 2 and a message before a GPU is asked for"""
    ph = tmp_path / "p.txt"
    ph.write_text("id weight z\nC 1.0 1\nD NA 2\nF 2.5 3\n")
    files = [os.path.join(DEMO, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    base = ["--qtlbin", "q.txt", "--phenofile", str(ph)]
    for extra, text in ((["--qtlbin", "q.txt"], "--qtlbin FILE needs --phenofile FILE"),
                        (["--qtl-binary-iterations", "5"], "--qtl-binary-iterations and --qtl-binary-tol need --qtlbin FILE"),
                        (["--qtl-binary-tol", "1e-5"], "--qtl-binary-iterations and --qtl-binary-tol need --qtlbin FILE"),
                        (base + ["--qtl-binary-iterations", "0"], "--qtl-binary-iterations must be 1 .. 1000"),
                        (base + ["--qtl-binary-iterations", "1001"], "--qtl-binary-iterations must be 1 .. 1000"),
                        (base + ["--qtl-binary-tol", "nan"], "--qtl-binary-tol needs a finite number"),
                        (base + ["--qtl-binary-tol", "x"], "--qtl-binary-tol needs a finite number"),
                        (base + ["--gpus", "2"], "--qtlbin needs a single GPU"),
                        (base, "--qtlbin: no column of")):
        args = [EXE, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--count", "1", "--quiet", *extra]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 2 and text in r.stderr, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "q.txt").exists()


# ------------------------------------------------------------------------------------- every width of X0, every design
@pytest.mark.parametrize("stop", (False, True), ids=("fixed", "stop"))
@pytest.mark.parametrize("case", R.WIDTH_CASES, ids=R.case_id)
def test_every_width_and_design(case, stop):
    """K = 3 .. 7 and the design (a, i) through cnf2h_qtlbin_fit, as tests/test_gpu_qtlbin.py runs them on the device: a
    failure there that does not show here is the kernels', not the model's"""
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    how = R.WIDTH_STOP if stop else dict(max_iter=max_iter, tol=-1.0)
    ref = R.case_reference(case, **(R.WIDTH_STOP if stop else {}))
    # on the references alone, before the product runs
    R.assert_conditions([R.case_reference(c, **(R.WIDTH_STOP if stop else {})) for c in R.WIDTH_CASES])
    assert R.compared_cells(ref, CS, share=1.0).all()
    if stop:
        R.assert_anchor(ref, R.case_id(case))
        assert np.all(ref["status"] == 0)
    origin, pheno, cov, use, perm = R.make_case(*case)
    got = host_scan(origin, pheno, use, cov, perm, imprint, additive, **how)
    assert got["coef"].shape[2] == len(R.effects(additive, imprint))
    R.compare_bin(got, ref, CS, "host %s %s" % (R.case_id(case), "to tol 1e-7" if stop else "fixed"), share=1.0)
    if not stop:
        fitted = got["rank"] > 0
        assert np.all(got["iters"][:, fitted] == max_iter) and np.all(got["status"][:, fitted] == 1)


def test_additive_imprint_drops_i():
    """(a, i) on the degenerate rows: i is dropped at the homozygous and the symmetric marker, and lod and a are the additive
    fit's without imprinting"""
    origin, at = R.degenerate_rows()
    n = origin.shape[0]
    y = R.bernoulli(np.zeros((n, 1)), 11)[:, 0]
    z = R.noise(n, 1, 12)
    for m in (at["homozygous"], at["symmetric"]):
        f = host.qtlbin_fit(origin[:, m], y, z, additive=True, imprint=True)
        g = host.qtlbin_fit(origin[:, m], y, z, additive=True)
        assert f["rank"] == 1 and np.isnan(f["coef"][1]) and f["lod"] == g["lod"] > 0.0 and f["coef"][0] == g["coef"][0]
        assert f["iters"] == g["iters"] and len(f["coef"]) == 2 and len(g["coef"]) == 1
    f = host.qtlbin_fit(origin[:, at["zeros"]], y, z, additive=True, imprint=True)
    assert f["rank"] == 2 and np.isfinite(f["coef"]).all()


# ------------------------------------------------------------------------------------- two edges of the walk
def test_a_round_with_nobody_in_it():
    p = R.EMPTY_ROUND
    origin, pheno, z, use = R.empty_round_case()
    ref = R.empty_round_reference()
    R.assert_anchor(ref, "empty round")
    R.compared_cells(ref, CS, share=p["share"])
    assert ref["near"].mean() <= 0.01 and np.all(ref["n_used"] == 66)
    got = host_scan(origin, pheno, use, z, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_bin(got, ref, CS, "host n 130, 64 .. 127 unused", share=p["share"])


@pytest.mark.parametrize("n_c", (7, 6))
def test_scan_threshold_of_the_additive_imprint_design(n_c):
    """(a, i) with K = 3: W = 6, so a chromosome with 7 individuals is scanned and one with 6 is not"""
    origin, y, z = R.threshold_case(n_c)
    ref = R.reference_scan_binary(origin, CS, y, None, z, imprint=True, additive=True, max_iter=50, tol=1e-7)
    assert ref["usable"][R.THRESHOLD["chrom"]] == (n_c == 7) and ref["usable"].sum() == 5 + (n_c == 7)
    got = host_scan(origin, y, None, z, imprint=True, additive=True, max_iter=50, tol=1e-7)
    R.assert_threshold(got, n_c)
    fine = R.compared_cells(dict(ref, maxeta=np.zeros_like(ref["maxeta"])), CS, share=0.9, strict=False)[0]
    assert np.array_equal(got["rank"][fine], ref["rank"][fine])
