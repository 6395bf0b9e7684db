"""CPU tests of the survival-trait scan: cnf2_qtlsurv.h compiled for the host and run through cnf2h_qtlsurv_fit, one (marker,
column) cell at a time, against the yardstick tests/qtlsurv_reference.py (the direct risk-set definition); the yardstick's own
anchor, the closed-form null without covariates, hand-made ties and censoring, the refusals, scan_surv's argument checks, the
exported symbols and the command line's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qtlsurv_reference as R
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


def host_scan(origin, time, status, use=None, cov=None, perm=None, imprint=False, additive=False, max_iter=50, tol=1e-7):
    """the scan of cnf2_qtl_scan_surv cell by cell through cnf2h_qtlsurv_fit: the dict Context.qtl_scan_surv returns"""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    Cn = len(CS) - 1
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    z = None if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    Tm = R.columns(np.where(use[:, None], np.asarray(time, np.float64).reshape(n, -1), 0.0), perm)
    Dm = R.columns(np.where(use[:, None], np.asarray(status, np.float64).reshape(n, -1), 0.0), perm)
    Q, T = Tm.shape[1], Tm.shape[2]
    ne = len(R.effects(additive, imprint))
    out = dict(lod=np.zeros((T, M)), coef=np.zeros((T, M, ne)), iters=np.zeros((T, M), np.int32),
               status=np.zeros((T, M), np.int32), rank=np.zeros(M, np.int32), ll0=np.zeros((T, Cn)),
               n_events=np.zeros((T, Cn), np.int32), n_used=np.zeros(Cn, np.int32), perm_max=np.zeros((Q - 1, T, Cn)) if Q > 1 else None)
    for c in range(Cn):
        mask = use & (o[:, CS[c]] != 0.0).any(axis=1)
        for m in range(CS[c], CS[c + 1]):
            for q in range(Q):
                for t in range(T):
                    f = host.qtlsurv_fit(o[:, m], Tm[:, q, t], Dm[:, q, t], z, mask, additive, imprint, max_iter, tol)
                    if q == 0:
                        for key in ("lod", "iters", "status", "coef"):
                            out[key][t, m] = f[key]
                        out["rank"][m], out["n_used"][c] = f["rank"], f["n_used"]
                        out["ll0"][t, c], out["n_events"][t, c] = f["ll0"], f["n_events"]
                    else:
                        out["perm_max"][q - 1, t, c] = max(out["perm_max"][q - 1, t, c], f["lod"])
    return out


@pytest.mark.parametrize("case", R.HOST_CASES, ids=R.case_id)
@pytest.mark.parametrize("max_iter", (1, 3))
def test_fixed_iterations(case, max_iter):
    n, K, imprint, additive, seed, T, P, mask, skipped, _, grid = case
    ref = R.case_reference(case, max_iter, -1.0)
    R.compared_cells(ref, CS)                # the precondition, on the reference alone, before the product runs
    origin, time, status, cov, use, perm = R.make_case(*case)
    got = host_scan(origin, time, status, use, cov, perm, imprint, additive, max_iter, -1.0)
    R.compare_surv(got, ref, CS, "host %s at %d iterations" % (R.case_id(case), max_iter))
    fitted = got["rank"] > 0
    assert np.all(got["iters"][:, fitted] == max_iter) and np.all(got["status"][:, fitted] == 1)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_every_width_and_design(case):
    """every K = 0 .. 8 and every design through cnf2h_qtlsurv_fit at the case's own fixed iterations, as
    tests/test_gpu_qtlsurv.py runs them on the device: a failure there that does not show here is the kernels', not the model's"""
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter, grid = case
    ref = R.case_reference(case)
    R.assert_conditions([R.case_reference(c) for c in R.CASES])
    origin, time, status, cov, use, perm = R.make_case(*case)
    got = host_scan(origin, time, status, use, cov, perm, imprint, additive, max_iter, -1.0)
    assert got["coef"].shape[2] == len(R.effects(additive, imprint))
    R.compare_surv(got, ref, CS, "host %s" % R.case_id(case))


@pytest.mark.parametrize("case", R.HOST_CASES, ids=R.case_id)
def test_stopping_rule(case):
    n, K, imprint, additive, seed, T, P, mask, skipped, _, grid = case
    ref = R.case_reference(case, **R.STOP)
    # on the yardstick alone, before the product runs: its converged likelihood is that of the longdouble Newton run from
    # theta = 0, and nearly all cells are compared
    R.assert_anchor(ref, R.case_id(case))
    R.assert_conditions([R.case_reference(c, **R.STOP) for c in R.HOST_CASES])
    R.compared_cells(ref, CS)
    origin, time, status, cov, use, perm = R.make_case(*case)
    got = host_scan(origin, time, status, use, cov, perm, imprint, additive, **R.STOP)
    R.compare_surv(got, ref, CS, "host %s to tol" % R.case_id(case))
    assert np.all(got["status"] == 0) and got["iters"].max() <= 10


def test_closed_form_null_without_covariates():
    for case in (R.CASES[2], R.CASES[1]):                 # distinct times; tied times
        origin, time, status, _, _, _ = R.make_case(*case)
        t, d = time[:, 0], status[:, 0]
        want = R.closed_form_null(t, d)
        f = host.qtlsurv_fit(origin[:, 20], t, d)
        print("closed-form null: %.17g against %.17g" % (f["ll0"], want))
        assert abs(f["ll0"] - want) <= R.ATOL and f["ll0"] < 0 and f["n_events"] == d.sum() and f["n_used"] == len(t)
        # ... under a mask too, and the yardstick's null is the same number
        c = np.ones(len(t), bool)
        c[::5] = False
        g = host.qtlsurv_fit(origin[:, 20], t, d, c=c)
        assert abs(g["ll0"] - R.closed_form_null(t[c], d[c])) <= R.ATOL
        assert abs(R.null_fit(np.zeros((c.sum(), 0)), *R.risk_sets(t[c], d[c]))[0] - g["ll0"]) <= R.ATOL


@pytest.mark.parametrize("which", ("span", "censored", "masked", "last", "single", "none", "empty"))
def test_hand_made_ties_and_censoring(which):
    origin, time, status, z, use = R.hand_case(which)
    ref = R.hand_reference(which)
    share = 0.0 if which in ("single", "none") else 0.9
    R.compared_cells(ref, CS, share=share)
    got = host_scan(origin, time, status, use, z, max_iter=R.HAND["max_iter"], tol=R.HAND["tol"])
    assert np.isfinite(got["lod"]).all() and np.isfinite(got["ll0"]).all() and np.isin(got["status"], (0, 1, 2)).all()
    if which == "none":
        assert np.all(got["lod"] == 0.0) and np.all(got["ll0"] == 0.0) and np.all(got["n_events"] == 0)
        assert np.all(got["iters"] == 0) and np.isnan(got["coef"]).all() and np.array_equal(got["rank"], ref["rank"])
    else:
        R.compare_surv(got, ref, CS, "host hand-made: " + which, share=share)


def test_time_enters_by_rank_only():
    case = R.CASES[3]
    n, K, imprint, additive, seed, T, P, mask, skipped, _, grid = case
    origin, time, status, cov, use, perm = R.make_case(*case)
    t, d = time[:, 0], status[:, 0]
    for m in (3, 40, 70):
        f = host.qtlsurv_fit(origin[:, m], t, d, cov)
        for g in (host.qtlsurv_fit(origin[:, m], np.exp(t), d, cov), host.qtlsurv_fit(origin[:, m], 3.0 * t + 7.0, d, cov)):
            assert g["lod"] == f["lod"] and g["ll0"] == f["ll0"] and g["iters"] == f["iters"] and np.array_equal(g["coef"], f["coef"])


def test_monotone_likelihood_ends_finite():
    """the effect of a orders the times perfectly: l has no maximum.  Its gains shrink geometrically, so a positive tol stops
    the fit by the first rule (status 0) at a large effect; with a negative tol it ends by max_iter or by a breakdown"""
    marker = 8
    origin, time, status = R.perfect_order_case(marker=marker)
    f = host.qtlsurv_fit(origin[:, marker], time[:, 0], status[:, 0], additive=True, max_iter=200, tol=-1.0)
    print("monotone likelihood: status %d after %d iterations, lod %.3f, a %.2f" % (f["status"], f["iters"], f["lod"], f["coef"][0]))
    assert f["rank"] == 1 and f["status"] in (1, 2) and np.isfinite([f["lod"], f["ll0"], f["coef"][0]]).all()
    assert f["coef"][0] > 5.0 and 1.0 < f["lod"] <= -f["ll0"] / R.LN10 + R.ATOL


def test_refused_arguments():
    o = np.full((8, 4), 0.25)
    t, d = np.arange(8.0), np.array([0, 1, 0, 1, 1, 0, 1, 0.0])
    for kw in (dict(max_iter=0), dict(max_iter=1001), dict(tol=np.nan), dict(tol=np.inf), dict(cov=np.zeros((8, 9)))):
        with pytest.raises(RuntimeError):
            host.qtlsurv_fit(o, t, d, **kw)
    c = np.ones(8, np.uint8)
    c[3] = 0
    for bad in (0.5, 2.0, np.nan, -1.0):
        db = d.copy()
        db[3] = bad
        with pytest.raises(RuntimeError):
            host.qtlsurv_fit(o, t, db)
        host.qtlsurv_fit(o, t, db, c=c)          # the same value at an individual outside the mask is accepted
    for bad in (np.nan, np.inf, -np.inf):
        tb = t.copy()
        tb[3] = bad
        with pytest.raises(RuntimeError):
            host.qtlsurv_fit(o, tb, d)
        host.qtlsurv_fit(o, tb, d, c=c)


class _Ctx:
    n_ind, n_markers, n_chrom = 6, 3, 1


def test_scan_surv_argument_checks():
    t = np.array([[3.0], [1.0], [2.0], [5.0], [np.nan], [4.0]])
    d = np.array([[0.0], [1.0], [0.0], [1.0], [7.0], [1.0]])       # (the status of a missing time is not looked at)
    with pytest.raises(ValueError):
        qtl.scan_surv(_Ctx(), np.zeros((5, 1)), np.zeros((5, 1)))
    with pytest.raises(ValueError):
        qtl.scan_surv(_Ctx(), t, d[:5])
    for kw in (dict(max_iter=0), dict(max_iter=1001), dict(tol=np.nan), dict(tol=np.inf)):
        with pytest.raises(ValueError):
            qtl.scan_surv(_Ctx(), t, d, **kw)
    for bad in (0.5, 2.0, -1.0, np.nan):
        db = d.copy()
        db[2] = bad
        with pytest.raises(ValueError):
            qtl.scan_surv(_Ctx(), t, db)


def test_symbols():
    for name in ("cnf2_qtl_scan_surv", "cnf2_set_qtlsurv_columns", "cnf2_set_qtlsurv_blocks"):
        assert name in capi.SYMBOLS and hasattr(C.CDLL(capi.LIB_PATH), name)
    assert "cnf2h_qtlsurv_fit" in host.SYMBOLS and hasattr(C.CDLL(host.LIB_PATH), "cnf2h_qtlsurv_fit")


def test_command_line_usage_errors(tmp_path):
    """every one of these ends with status 2 and a message before a GPU is asked for"""
    ph = tmp_path / "p.txt"
    ph.write_text("id days dead z\nC 1.0 1 1\nD NA 0 2\nF 2.5 0 3\n")
    bad = tmp_path / "b.txt"
    bad.write_text("id days dead z\nC 1.0 1 1\nD NA 0 2\nF 2.5 2 3\n")
    files = [os.path.join(DEMO, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    names = ["--qtl-surv-time", "days", "--qtl-surv-status", "dead"]
    base = ["--qtlsurv", "q.txt", "--phenofile", str(ph)] + names
    needs = "--qtl-surv-time, --qtl-surv-status, --qtl-surv-iterations and --qtl-surv-tol need --qtlsurv FILE"
    for extra, text in ((["--qtlsurv", "q.txt"] + names, "--qtlsurv FILE needs --phenofile FILE"),
                        (["--qtlsurv", "q.txt", "--phenofile", str(ph)], "--qtlsurv FILE needs --qtl-surv-time NAME and --qtl-surv-status NAME"),
                        (["--qtlsurv", "q.txt", "--phenofile", str(ph), "--qtl-surv-time", "days"],
                         "--qtlsurv FILE needs --qtl-surv-time NAME and --qtl-surv-status NAME"),
                        (["--qtl-surv-iterations", "5"], needs),
                        (["--qtl-surv-tol", "1e-5"], needs),
                        (["--qtl-surv-time", "days"], needs),
                        (base + ["--qtl-surv-iterations", "0"], "--qtl-surv-iterations must be 1 .. 1000"),
                        (base + ["--qtl-surv-iterations", "1001"], "--qtl-surv-iterations must be 1 .. 1000"),
                        (base + ["--qtl-surv-tol", "nan"], "--qtl-surv-tol needs a finite number"),
                        (base + ["--qtl-surv-tol", "x"], "--qtl-surv-tol needs a finite number"),
                        (base + ["--gpus", "2"], "--qtlsurv needs a single GPU"),
                        (base[:-1] + ["death"], "--qtl-surv-status: \"death\" is not a column"),
                        (base + ["--qtl-covariates", "days"], "--qtl-surv-time: \"days\" is a covariate"),
                        (["--qtlsurv", "q.txt", "--phenofile", str(bad)] + names, "holds a value that is neither 0 nor 1")):
        args = [EXE, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--count", "1", "--quiet", *extra]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 2 and text in r.stderr, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "q.txt").exists()
