"""CPU tests of the variance-QTL scan: cnf2_qtlvar.h compiled for the host and run through cnf2h_qtlvar_fit, one (marker,
column) cell at a time, against the yardstick tests/qtlvar_reference.py (explicit designs, numpy.linalg): fixed iterations
and the stopping rule on soft rows, the yardstick's own anchor, the refusals, the scan threshold, the rank rule with i
dropped, two closed forms, scan_var's argument checks, the exported symbols and the command line's usage errors."""
import os
import subprocess

import numpy as np
import pytest

import qtlvar_reference as R
from conftest import ROOT
from qtlem_reference import degenerate_rows

EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")
CS = R.chromstarts_of(R.CHROM_LENS)
LN10 = np.log(10.0)


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


def host_scan(origin, pheno, use=None, cov=None, n_var=0, perm=None, imprint=False, additive=False, max_iter=50, tol=1e-7):
    """the scan of cnf2_qtl_scan_var cell by cell through cnf2h_qtlvar_fit: the dict Context.qtl_scan_var returns.  The host
    fit centres over the mask it is given; the scan centres over `use`, which differs on a chromosome that skips somebody
    by a shift the intercepts take up."""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    Cn = len(CS) - 1
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    z = None if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    Y = R.columns(np.where(use[:, None], np.nan_to_num(np.asarray(pheno, np.float64).reshape(n, -1)), 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    ne = len(R.effects(additive, imprint))
    out = dict(lod=np.zeros((T, M, 3)), coef_mean=np.zeros((T, M, ne)), coef_var=np.zeros((T, M, ne)),
               iters=np.zeros((T, M, 3), np.int32), status=np.zeros((T, M, 3), np.int32), rank=np.zeros(M, np.int32),
               ll0=np.zeros((T, Cn)), n_used=np.zeros(Cn, np.int32), perm_max=np.zeros((Q - 1, T, Cn, 3)) if Q > 1 else None)
    for c in range(Cn):
        mask = use & (o[:, CS[c]] != 0.0).any(axis=1)
        for m in range(CS[c], CS[c + 1]):
            for q in range(Q):
                for t in range(T):
                    f = host.qtlvar_fit(o[:, m], Y[:, q, t], z, n_var, mask, additive, imprint, max_iter, tol)
                    if q == 0:
                        for key in ("lod", "iters", "status", "coef_mean", "coef_var"):
                            out[key][t, m] = f[key]
                        out["rank"][m], out["n_used"][c], out["ll0"][t, c] = f["rank"], f["n_used"], f["ll0"]
                    else:
                        out["perm_max"][q - 1, t, c] = np.maximum(out["perm_max"][q - 1, t, c], f["lod"])
    return out


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fixed_iterations(case):
    """every K + 1, every n_var and every design through cnf2h_qtlvar_fit at the case's own fixed iterations, as
    tests/test_gpu_qtlvar.py runs them on the device: a failure there that does not show here is the kernels', not the model's"""
    n, K, n_var, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    ref = R.case_reference(case)
    R.assert_conditions([R.case_reference(c) for c in R.CASES])      # on the references alone, before the product runs
    origin, pheno, cov, use, perm = R.make_case(*case)
    got = host_scan(origin, pheno, use, cov, n_var, perm, imprint, additive, max_iter, -1.0)
    assert got["coef_mean"].shape[2] == len(R.effects(additive, imprint))
    R.compare_var(got, ref, CS, "host %s" % R.case_id(case), share=0)
    fitted = got["rank"] > 0
    assert np.all(got["iters"][:, fitted] == max_iter) and np.all(got["status"][:, fitted] == 1)


def test_stopping_rule_and_planted_locus():
    p = R.PLANTED
    ref, hk = R.planted_reference(), R.planted_linear_reference()
    R.assert_anchor(ref, "planted")                        # on the yardstick alone, before anything of the product runs
    R.compared_cells(ref, CS)
    assert ref["near"].mean() <= 0.01 and np.all(ref["status"] == 0)
    R.assert_planted(ref, hk)
    origin, _, pheno, z = R.planted_case()
    got = host_scan(origin, pheno, None, z, 0, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_var(got, ref, CS, "host planted locus, tol %g" % p["tol"])
    short = host_scan(origin, pheno, None, z, 0, max_iter=p["short"], tol=p["tol"])
    ok = ~ref["near"]
    assert np.array_equal((short["status"] == 1)[ok], (ref["iters"] > p["short"])[ok])
    assert np.array_equal(short["iters"][ok], np.minimum(ref["iters"], p["short"])[ok])


def test_step_halving():
    p = R.HALVING
    ref = R.halving_reference()
    cc = R.compared_cells(ref, CS, share=0.9)
    halved = (ref["halvings"] >= 1) & cc[..., None] & ~ref["near"]
    print("halving: %d fits of %d take at least one halving, at most %d" % (halved.sum(), halved.size, ref["halvings"].max()))
    assert halved.sum() >= 1
    origin, pheno, z = R.halving_case()
    got = host_scan(origin, pheno, None, z, p["n_var"], imprint=True, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_var(got, ref, CS, "host halving", share=0.9)


def test_closed_form_haley_knott():
    """n_var = 0: (l_mean-only - l_null) / ln 10 is Haley-Knott's LOD n_c / 2 log10(RSS0 / RSS1) of the same design, at tol
    1e-12.  Measured: the yardstick's own error is 2.5e-14 LOD, the product's bound ten times that, the product's error 2.9e-14."""
    bound = R.hk_identity_bound()
    hk = R.planted_linear_reference()
    origin, _, pheno, z = R.planted_case()
    worst = 0.0
    for m in range(CS[-1]):
        f = host.qtlvar_fit(origin[:, m], pheno[:, 0], z, 0, max_iter=R.PLANTED["max_iter"], tol=1e-12)
        assert np.all(f["status"] == 0)
        # (lod[0] - lod[2] where neither is clipped at 0; the fits' own l are not reported, so cells where the variance LOD
        # is 0 are compared through the joint LOD alone, which then is the mean-only fit's up to its own stopping tolerance)
        if f["lod"][2] > 0.0:
            worst = max(worst, abs(f["lod"][0] - f["lod"][2] - hk["lod"][0, 0, m]))
    print("Haley-Knott identity: the product's error %.3g" % worst)
    assert worst <= bound


def test_closed_form_class_means():
    """certain rows, K = 0, design (a, d, i): the full fit is the four classes' own means and ML variances,
    l = -1/2 sum_k n_k (log 2pi + log s_k^2 + 1), at tol 1e-12.  Measured: the yardstick's own error is 1.2e-14 LOD, the
    product's bound ten times that, the product's error 1.2e-14."""
    n, m = 130, 40
    _, k = R.soft_rows(n, R.CHROM_LENS, 6)
    k = k[:, m]
    assert np.bincount(k, minlength=4).min() >= 8
    y = (0.3 * R.CODES["a"][k] + np.exp(0.4 * R.CODES["a"][k]) * R.gauss((n,), 13))
    closed = sum(-0.5 * (k == g).sum() * (R.LOG2PI + np.log(y[k == g].var()) + 1.0) for g in range(4))
    o = R.certain_rows(k)
    X0 = np.ones((n, 1))
    E = np.column_stack([R.CODES[e][k] for e in "adi"])
    f0 = R.null_fit(X0, X0, y, y.mean())
    full = R.dglm(np.column_stack([X0, E]), np.column_stack([X0, E]), y, np.concatenate([f0["beta"], np.zeros(3)]),
                  np.concatenate([f0["gamma"], np.zeros(3)]), f0["ll"][-1], 200, 1e-12)
    assert full["status"] == 0
    own = abs(full["ll"][-1] - closed) / LN10
    print("class means: the yardstick's own error %.3g LOD, the product's bound %.3g" % (own, 10 * own))
    f = host.qtlvar_fit(o, y, imprint=True, max_iter=200, tol=1e-12)
    assert f["rank"] == 3 and np.all(f["status"] == 0)
    err = abs(f["lod"][0] - (closed - f["ll0"]) / LN10)
    print("class means: the product's error %.3g LOD" % err)
    assert err <= 10 * own
    # the coefficients are the classes' contrasts: a = (mean_3 - mean_0) / 2 in the mean, (log s_3^2 - log s_0^2) / 2 in the variance
    mean, lv = [y[k == g].mean() for g in range(4)], [np.log(y[k == g].var()) for g in range(4)]
    assert abs(f["coef_mean"][0] - (mean[3] - mean[0]) / 2) <= 1e-6 and abs(f["coef_var"][0] - (lv[3] - lv[0]) / 2) <= 1e-5
    assert abs(f["coef_mean"][2] - (mean[1] - mean[2]) / 2) <= 1e-6 and abs(f["coef_var"][2] - (lv[1] - lv[2]) / 2) <= 1e-5


@pytest.mark.parametrize("n_c", (11, 10))
def test_scan_threshold(n_c):
    """(a, i) with K = 3 and n_var = 1 needs (1 + 3 + 2) + (1 + 1 + 2) + 1 = 11 individuals: 11 are scanned, 10 are not"""
    p = R.THRESHOLD
    origin, y, z = R.threshold_case(n_c)
    c = p["chrom"]
    mask = (origin[:, CS[c]] != 0.0).any(axis=1)
    assert mask.sum() == n_c
    for m in range(CS[c], CS[c + 1]):
        f = host.qtlvar_fit(origin[:, m], y[:, 0], z, p["n_var"], mask, additive=True, imprint=True)
        assert f["n_used"] == n_c and np.isfinite(f["lod"]).all() and np.all(f["lod"] >= 0) and np.isin(f["status"], (0, 1, 2)).all()
        if n_c >= p["need"]:
            assert f["rank"] > 0 and f["ll0"] != 0.0 and np.all(f["iters"] > 0)
        else:
            assert f["rank"] == 0 and f["ll0"] == 0.0 and np.all(f["lod"] == 0.0) and np.all(f["iters"] == 0) and np.all(f["status"] == 0)
            assert np.isnan(f["coef_mean"]).all() and np.isnan(f["coef_var"]).all()


def test_additive_imprint_drops_i():
    """The design (a, i) on the degenerate rows: at the homozygous and the symmetric marker i vanishes, the rank is 1 with i
    dropped from both parts, and the LODs and a are those of the additive run without imprinting; at the flat marker nothing
    is fitted"""
    origin, at = degenerate_rows(n=41)
    y = R.gauss((41,), 11)
    z = R.noise(41, 1, 12)
    for m in (at["homozygous"], at["symmetric"]):
        f = host.qtlvar_fit(origin[:, m], y, z, 1, additive=True, imprint=True, tol=1e-9)
        g = host.qtlvar_fit(origin[:, m], y, z, 1, additive=True, imprint=False, tol=1e-9)
        assert f["rank"] == 1 and np.isfinite(f["coef_mean"][0]) and np.isnan(f["coef_mean"][1]) and np.isnan(f["coef_var"][1])
        assert f["lod"].tobytes() == g["lod"].tobytes() and f["coef_var"][0] == g["coef_var"][0] and f["coef_mean"][0] == g["coef_mean"][0]
        assert np.array_equal(f["iters"], g["iters"])
    f = host.qtlvar_fit(origin[:, at["flat"]], y, z, 1, additive=True, imprint=True)
    assert f["rank"] == 0 and np.all(f["lod"] == 0.0) and np.all(f["iters"] == 0) and np.all(f["status"] == 0)
    assert np.isnan(f["coef_mean"]).all() and np.isnan(f["coef_var"]).all() and f["ll0"] != 0.0
    f = host.qtlvar_fit(origin[:, at["zeros"]], y, z, 1, additive=True, imprint=True)
    assert f["rank"] == 2 and np.isfinite(f["coef_var"]).all()


def test_constant_trait_and_zero_class_variance():
    n, m = 41, 40
    origin, k = R.soft_rows(n, R.CHROM_LENS, 6)
    f = host.qtlvar_fit(origin[:, m], np.full(n, 1.25))
    assert f["rank"] == 2 and f["ll0"] == 0.0 and np.all(f["lod"] == 0.0) and np.all(f["iters"] == 0) and np.isnan(f["coef_var"]).all()
    y = R.gauss((n,), 11)
    y[k[:, m] == 3] = 0.5
    f = host.qtlvar_fit(R.certain_rows(k[:, m]), y)
    print("a class variance of 0: status %s, iters %s, lod %s" % (f["status"], f["iters"], f["lod"]))
    assert np.isfinite(f["lod"]).all() and np.all(f["lod"] >= 0) and np.isfinite(f["ll0"]) and np.all(np.isin(f["status"][1:], (1, 2)))
    assert np.isfinite(f["coef_mean"]).all() and np.isfinite(f["coef_var"]).all()


def test_refused_arguments():
    n = 20
    origin, _ = R.soft_rows(n, (3,), 5)
    o, y, z = origin[:, 1], R.gauss((n,), 3), R.noise(n, 2, 4)
    ok = host.qtlvar_fit(o, y, z, 2)
    assert ok["rank"] == 2
    for kw in (dict(max_iter=0), dict(max_iter=1001), dict(tol=np.nan), dict(tol=np.inf), dict(n_var=-1), dict(n_var=3)):
        with pytest.raises(RuntimeError, match=r"failed \(-2\)"):
            host.qtlvar_fit(o, y, z, **dict(dict(n_var=1), **kw))
    with pytest.raises(RuntimeError, match=r"failed \(-2\)"):
        host.qtlvar_fit(o, y, R.noise(n, 4, 4), 4)          # n_var above 3
    with pytest.raises(RuntimeError, match=r"failed \(-2\)"):
        host.qtlvar_fit(o, y, R.noise(n, 9, 4), 0)          # n_cov above 8
    with pytest.raises(RuntimeError, match=r"failed \(-2\)"):
        host.qtlvar_fit(o, y, None, 1)                      # a variance covariate without covariates


def test_scan_var_argument_checks():
    from cnf2freq_amd import qtl

    class Ctx:
        n_ind, n_markers, n_chrom = 12, 5, 1
    y, z = np.zeros((12, 1)), np.zeros((12, 2))
    for kw in (dict(max_iter=0), dict(max_iter=1001), dict(tol=np.nan), dict(var_covariates=(2,)), dict(var_covariates=(0, 0)),
               dict(var_covariates=(-1,)), dict(cov=None, var_covariates=(0,))):
        with pytest.raises(ValueError):
            qtl.scan_var(Ctx(), y, **dict(dict(cov=z), **kw))
    with pytest.raises(ValueError):
        qtl.scan_var(Ctx(), np.zeros((11, 1)), cov=z[:11])
    with pytest.raises(ValueError):
        qtl.scan_var(Ctx(), y, cov=np.zeros((12, 4)), var_covariates=(0, 1, 2, 3))
    with pytest.raises(ValueError):
        qtl.thresholds_var(np.zeros((3, 1, 2)))
    th = qtl.thresholds_var(np.arange(60.0).reshape(10, 1, 2, 3))
    assert set(th) == {"alpha", "joint", "mean", "variance"} and th["variance"]["genome"].shape == (2, 1)
    lod = np.zeros((1, 5, 3))
    lod[0, 2] = [3.0, 0.5, 2.5]
    pk = qtl.peaks_var(dict(lod=lod), np.arange(5.0), [0, 5], dict(joint=1.0, mean=1.0, variance=1.0))
    assert [len(pk[k]) for k in qtl.VAR_KEYS] == [1, 0, 1] and pk["variance"][0]["marker"] == 2


def test_symbols():
    assert "cnf2h_qtlvar_fit" in host.SYMBOLS
    assert {"cnf2_qtl_scan_var", "cnf2_set_qtlvar_columns"} <= set(capi.SYMBOLS)
    L = capi.load()
    assert hasattr(L, "cnf2_qtl_scan_var") and hasattr(L, "cnf2_set_qtlvar_columns")


def test_command_line_usage_errors(tmp_path):
    """every one of these ends with status 2 and a message before a GPU is asked for"""
    ph = tmp_path / "p.txt"
    ph.write_text("id weight z w\nC 1.0 1 2\nD NA 2 1\nF 2.5 3 5\n")
    files = [os.path.join(DEMO, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    base = ["--qtlvar", "q.txt", "--phenofile", str(ph)]
    for extra, text in ((["--qtlvar", "q.txt"], "--qtlvar FILE needs --phenofile FILE"),
                        (["--qtl-var-iterations", "5"], "--qtl-var-covariates, --qtl-var-iterations and --qtl-var-tol need --qtlvar FILE"),
                        (["--qtl-var-tol", "1e-5"], "--qtl-var-covariates, --qtl-var-iterations and --qtl-var-tol need --qtlvar FILE"),
                        (["--qtl-var-covariates", "z"], "--qtl-var-covariates, --qtl-var-iterations and --qtl-var-tol need --qtlvar FILE"),
                        (base + ["--qtl-var-iterations", "0"], "--qtl-var-iterations must be 1 .. 1000"),
                        (base + ["--qtl-var-iterations", "1001"], "--qtl-var-iterations must be 1 .. 1000"),
                        (base + ["--qtl-var-tol", "nan"], "--qtl-var-tol needs a finite number"),
                        (base + ["--qtl-var-tol", "x"], "--qtl-var-tol needs a finite number"),
                        (base + ["--gpus", "2"], "--qtlvar needs a single GPU"),
                        (base + ["--qtl-var-covariates", "z"], "--qtl-var-covariates: not among --qtl-covariates: z"),
                        (base + ["--qtl-covariates", "z", "--qtl-var-covariates", "z,nobody"], "--qtl-var-covariates: not among --qtl-covariates: nobody")):
        args = [EXE, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--count", "1", "--quiet", *extra]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 2 and text in r.stderr, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "q.txt").exists()
