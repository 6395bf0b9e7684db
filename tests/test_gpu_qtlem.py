"""GPU suite: the maximum-likelihood single-locus scan (cnf2_qtl_scan_em, cnf2_set_qtlem_columns, Context.qtl_scan_em,
qtl.scan_em, cnF2freq --qtlem).  EM interval mapping of every marker and phenotype column, checked against the expanded-data
least-squares EM in numpy (tests/qtlem_reference.py): a fixed number of iterations on hand-made rows at the shapes where the
tiling can go wrong, the stopping rule, the monotone likelihood, certain rows against the Haley-Knott scans, a planted locus
where the method must differ from Haley-Knott, degenerate and extreme inputs, bit-equality, refusals, a swept cross and the
command line."""
import numpy as np
import pytest

import qtlem_reference as R
from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, noise, reference_scan

pytestmark = pytest.mark.gpu

OUT_KEYS = R_KEYS = ("lod", "coef", "sigma2", "iters", "status", "rank", "rss0", "n_used", "perm_max")
CS = chromstarts_of(CHROM_LENS)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens=CHROM_LENS):
    """a context that holds a map only: what cnf2_qtl_scan_em needs"""
    cs = chromstarts_of(lens)
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in lens])
    ctx = capi.Context(0)
    ctx.upload_map(pos, cs)
    return ctx, cs


def same_bits(a, b, keys=OUT_KEYS):
    for k in keys:
        if a[k] is None:
            assert b[k] is None
        else:
            assert a[k].tobytes() == b[k].tobytes(), k


def device_outputs(capi, like, fill=77):
    import torch
    dev = torch.device("cuda", 0)
    return {k: None if v is None else torch.full(v.shape, fill, dtype=torch.int32 if v.dtype == np.int32 else torch.float64, device=dev)
            for k, v in like.items()}


# ------------------------------------------------------------------------------------- 1. fixed iterations, 7. the same bits
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "n%d-K%d-%s%s-T%d-P%d-it%d%s" % (
    c[0], c[1], "i" if c[2] else "m", "-add" if c[3] else "", c[5], c[6], c[9], "-mask" if c[7] else "-skip" if c[8] else ""))
def test_fixed_iterations(capi, case):
    """every output after exactly max_iter iterations against the yardstick at all 84 markers; the same bits with column tiles
    of 1 and 4, on a second call, from device rows, into device outputs and with another batching of the sweeps"""
    import torch
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    origin, pheno, cov, use, perm = R.make_case(*case)
    ref = R.case_reference(case)
    assert R.compared_markers(ref, CS).mean() >= 0.99      # the conditions of the comparison, on the reference, before anything runs
    ctx, _ = map_context(capi)
    kw = dict(cov=cov, imprint=imprint, use=use, perm=perm, additive=additive, max_iter=max_iter, tol=-1.0)
    got = ctx.qtl_scan_em(origin, pheno, **kw)
    R.compare_em(got, ref, CS, "n %d K %d imprint %d additive %d T %d P %d max_iter %d" % (n, K, imprint, additive, T, P, max_iter))
    fitted = got["rank"] > 0
    assert np.all(got["iters"][:, fitted] == max_iter) and np.all(got["status"][:, fitted] == 1)
    if skipped:
        assert got["n_used"][3] == n - 2 and got["n_used"][0] == n
    if mask:
        assert np.all(got["n_used"] == n - 2)
    same_bits(got, ctx.qtl_scan_em(origin, pheno, **kw))
    for cap in (1, 4):
        ctx.set_qtlem_columns(cap)
        same_bits(got, ctx.qtl_scan_em(origin, pheno, **kw))
    ctx.set_qtlem_columns(0)
    ctx.set_batch_jobs(5)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan_em_device(n, d_o.data_ptr(), pheno, **kw))
    ctx.set_batch_jobs(0)
    d = device_outputs(capi, got)
    ctx.qtl_scan_em_device(n, d_o.data_ptr(), pheno, out={k: None if v is None else v.data_ptr() for k, v in d.items()},
                           flags=capi.OUT_DEVICE, **kw)
    ctx.sync()
    same_bits(got, {k: None if v is None else v.cpu().numpy() for k, v in d.items()})
    ctx.close()


# ------------------------------------------------------------------------------------- 2. stopping rule, 5. not HK in disguise
def test_stopping_rule_and_not_haley_knott(capi):
    p = R.PLANTED
    ref = R.planted_reference()
    origin, _, pheno, z = R.planted_case()
    R.compared_markers(ref, CS)
    assert ref["near"].mean() <= 0.01                      # on the reference alone: cells at the edge of the rule
    hk = reference_scan(origin, CS, pheno, cov=z)["lod"][0, 0]
    em = ref["lod"][0, 0]
    print("reference: EM peak %.2f at %d, HK peak %.2f at %d, largest difference %.2f LOD, iterations %d .. %d" %
          (em.max(), em.argmax(), hk.max(), hk.argmax(), np.abs(em - hk).max(), ref["iters"].min(), ref["iters"].max()))
    assert np.abs(em - hk).max() > 0.5 and em.argmax() == p["marker"] and hk.argmax() == p["marker"]
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_em(origin, pheno, cov=z, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_em(got, ref, CS, "planted locus, tol %g" % p["tol"])
    assert got["lod"][0].argmax() == p["marker"] and np.all(got["status"] == 0)
    one = ctx.qtl_scan(origin, pheno, cov=z)
    assert np.abs(got["lod"] - one["lod"]).max() > 0.5     # the product's two scans differ as the references do
    short = ctx.qtl_scan_em(origin, pheno, cov=z, max_iter=p["short"], tol=p["tol"])
    ok = ~ref["near"]
    assert np.array_equal((short["status"] == 1)[ok], (ref["iters"] > p["short"])[ok])
    ctx.close()


# ------------------------------------------------------------------------------------- 3. monotone
def test_monotone(capi):
    ref = R.monotone_reference()
    steps = ref["trace"][0][:, list(R.MONOTONE)]
    assert np.all(np.diff(steps, axis=1) >= -1e-12)        # on the yardstick first
    origin, _, pheno, z = R.planted_case()
    ctx, _ = map_context(capi)
    lods = np.stack([ctx.qtl_scan_em(origin, pheno, cov=z, max_iter=k, tol=-1.0)["lod"][0] for k in R.MONOTONE], axis=1)
    ctx.close()
    print("LOD after %s iterations: smallest step %.3g, against the yardstick %.3g" %
          (R.MONOTONE, np.diff(lods, axis=1).min(), np.abs(lods - steps).max()))
    assert np.all(np.diff(lods, axis=1) >= -1e-12)
    assert np.abs(lods - steps).max() <= ATOL


# ------------------------------------------------------------------------------------- 4. certain rows
def test_certain_rows(capi):
    """on one-hot rows the mixture is the regression: two iterations, and the Haley-Knott scans' LOD and effects"""
    n = 41
    _, k = R.soft_rows(n, CHROM_LENS, 6)
    origin = R.certain_rows(k)
    z = noise(n, 2, 7)
    pheno = noise(n, 3, 8) + 0.7 * R.CODES["a"][k][:, [3, 40, 70]] + 0.5 * R.CODES["i"][k][:, [3, 50, 70]] + 0.3 * z[:, :1]
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_em(origin, pheno, cov=z, tol=1e-12)
    one = ctx.qtl_scan(origin, pheno, cov=z)
    fitted = got["rank"] > 0
    assert fitted.mean() > 0.9 and np.all(got["status"] == 0) and np.all(got["iters"][:, fitted] == 2)
    assert np.array_equal(got["rank"], one["rank"])
    full = got["rank"] == 2
    err_l = np.abs(got["lod"] - one["lod"]).max()
    err_c = (np.abs(got["coef"][:, full] - one["coef"][:, full]) / np.maximum(1.0, np.abs(one["coef"][:, full]))).max()
    print("certain rows against cnf2_qtl_scan: lod %.3g, coef %.3g" % (err_l, err_c))
    assert err_l <= ATOL and err_c <= ATOL
    goti = ctx.qtl_scan_em(origin, pheno, cov=z, imprint=True, tol=1e-12)
    x = ctx.qtl_scanx(origin, pheno, cov=z, imprint=True)
    fitted = goti["rank"] > 0
    assert np.all(goti["status"] == 0) and np.all(goti["iters"][:, fitted] == 2) and np.array_equal(goti["rank"], x["rank"][:, 1])
    full = goti["rank"] == 3
    err_l = np.abs(goti["lod"] - x["lod"][..., 1]).max()
    err_c = (np.abs(goti["coef"][:, full] - x["coef"][:, full]) / np.maximum(1.0, np.abs(x["coef"][:, full]))).max()
    print("certain rows with imprinting against cnf2_qtl_scanx: lod %.3g, coef %.3g" % (err_l, err_c))
    assert err_l <= ATOL and err_c <= ATOL and full.mean() > 0.9
    ctx.close()


# ------------------------------------------------------------------------------------- 6. degenerate and extreme inputs
def test_degenerate_and_extreme(capi):
    origin, at = R.degenerate_rows()
    n = origin.shape[0]
    y = noise(n, 1, 11)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_em(origin, y, imprint=True, tol=1e-7)
    plain = ctx.qtl_scan_em(origin, y, tol=1e-7)
    ref = R.reference_scan_em(origin, CS, y, imprint=True, tol=1e-7)
    R.compare_em(got, ref, CS, "degenerate rows", share=0.9)
    m = at["flat"]
    assert got["rank"][m] == 0 and got["lod"][0, m] == 0.0 and got["iters"][0, m] == 0 and np.isnan(got["coef"][0, m]).all()
    m = at["homozygous"]
    assert got["rank"][m] == 1 and np.isfinite(got["coef"][0, m, 0]) and np.isnan(got["coef"][0, m, 1:]).all()
    m = at["symmetric"]
    assert got["rank"][m] == 2 and np.isnan(got["coef"][0, m, 2])
    assert got["lod"][0, m].tobytes() == plain["lod"][0, m].tobytes() and got["coef"][0, m, :2].tobytes() == plain["coef"][0, m].tobytes()
    m = at["zeros"]
    assert got["rank"][m] == 3 and np.isfinite(got["coef"][0, m]).all()
    assert np.isfinite(got["lod"]).all() and np.isfinite(got["sigma2"]).all() and np.isfinite(got["rss0"]).all()
    # one individual 10^3 null standard deviations from the rest
    yo = R.outlier_pheno()
    ref = R.reference_scan_em(origin, CS, yo, imprint=True, max_iter=50, tol=1e-7)
    out = ctx.qtl_scan_em(origin, yo, imprint=True, max_iter=50, tol=1e-7)
    assert all(np.isfinite(out[k]).all() for k in ("lod", "sigma2", "rss0"))
    R.compare_em(out, ref, CS, "outlier", share=0.9)
    # n_c = W (= 1 + 1 + 3) on chromosome 4: not scanned there
    few = origin.copy()
    few[5:, CS[4]:CS[5]] = 0.0
    z = noise(n, 1, 12)
    got = ctx.qtl_scan_em(few, y, cov=z, imprint=True)
    on4 = slice(CS[4], CS[5])
    assert got["n_used"][4] == 5 and np.all(got["rank"][on4] == 0) and np.all(got["lod"][:, on4] == 0.0)
    assert np.isnan(got["coef"][:, on4]).all() and got["rss0"][0, 4] == 0.0 and np.all(got["rank"][CS[5]:] > 0)
    ctx.close()
    # a constant phenotype (n_c = 16 has an exact square root, so the null design's sums are exact) beside an ordinary one
    o16, _ = R.soft_rows(16, (3,), 5)
    ctx, _ = map_context(capi, (3,))
    got = ctx.qtl_scan_em(o16, np.stack([np.full(16, 2.0), noise(16, 1, 4)[:, 0]], axis=1))
    assert got["rss0"][0, 0] == 0.0 and np.all(got["lod"][0] == 0.0) and np.isnan(got["coef"][0]).all() and np.all(got["iters"][0] == 0)
    assert got["rss0"][1, 0] > 0.0 and np.isfinite(got["coef"][1]).all() and np.all(got["iters"][1] > 0)
    # a covariate that is constant over everybody: X0 is singular and nothing is scanned
    got = ctx.qtl_scan_em(o16, noise(16, 1, 4), cov=np.full((16, 1), 0.5))
    assert np.all(got["rank"] == 0) and np.all(got["lod"] == 0.0) and np.isnan(got["coef"]).all() and got["n_used"][0] == 16
    ctx.close()


# ------------------------------------------------------------------------------------- 7. identity permutation, 8. refusals
def test_identity_permutation_and_refusals(capi):
    case = R.CASES[1]
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    origin, pheno, cov, _, _ = R.make_case(*case)
    use = np.ones(n, bool)
    use[4] = False
    ctx, cs = map_context(capi)
    C, M = len(cs) - 1, int(cs[-1])
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3, use=use)[0], ident])
    got = ctx.qtl_scan_em(origin, pheno, cov=cov, imprint=True, use=use, perm=perm, max_iter=30, tol=1e-6)
    observed = np.stack([got["lod"][:, cs[c]:cs[c + 1]].max(axis=1) for c in range(C)], axis=1)          # [T][C]
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed) and np.all(observed > 0.0)
    # refused, with the outputs left alone
    twice = ident.copy()
    twice[3] = 2
    holed = pheno.copy()
    holed[6, 1] = np.nan
    bad_cov = cov.copy()
    bad_cov[7, 0] = np.inf
    base = dict(pheno=pheno, cov=cov, perm=ident[None], max_iter=10, tol=1e-6)
    refusals = [dict(max_iter=0), dict(max_iter=10001), dict(tol=np.nan), dict(tol=np.inf), dict(tol=-np.inf), dict(cov=np.zeros((n, 9))),
                dict(perm=twice[None]), dict(pheno=holed), dict(cov=bad_cov)]
    poisoned = lambda: dict(lod=np.full((T, M), 77.0), coef=np.full((T, M, 3), 77.0), sigma2=np.full((T, M), 77.0),
                            iters=np.full((T, M), 77, np.int32), status=np.full((T, M), 77, np.int32), rank=np.full(M, 77, np.int32),
                            rss0=np.full((T, C), 77.0), n_used=np.full(C, 77, np.int32), perm_max=np.full((1, T, C), 77.0))
    import torch
    d_o = torch.from_numpy(origin).cuda()
    for change in refusals:
        kw = dict(base, **change)
        out = poisoned()
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_em(origin, kw["pheno"], cov=kw["cov"], imprint=True, use=use, perm=kw["perm"], max_iter=kw["max_iter"],
                            tol=kw["tol"], out=out)
        assert all(np.all(v == 77) for v in out.values()), change
        d = device_outputs(capi, out)
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_em_device(n, d_o.data_ptr(), kw["pheno"], cov=kw["cov"], imprint=True, use=use, perm=kw["perm"],
                                   max_iter=kw["max_iter"], tol=kw["tol"], out={k: v.data_ptr() for k, v in d.items()},
                                   flags=capi.OUT_DEVICE)
        ctx.sync()
        assert all(bool((x == 77).all()) for x in d.values()), change
    ctx.close()


# ------------------------------------------------------------------------------------- 9. end to end
def test_end_to_end_on_a_swept_cross(capi):
    """qtl.scan_em on an F2 the product sweeps itself: within 1e-9 of the yardstick on the product's own origin_rows at the
    markers that pass the pivot precondition; the other three scans before and after on the rows a sweep_qtl left in the
    context; CNF2_ERR_STATE for another n and after an upload"""
    ped = synth.make_f2(24, 17, 2, seed=7)
    n, M = len(ped.dous), ped.n_markers
    cs = np.asarray(ped.chromstarts)
    cov = synth.uniform(21, np.arange(n)).reshape(n, 1)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = qtl.origin_rows(ctx)
    o = rows.cpu().numpy()
    a = o[:, :, 3] - o[:, :, 0]
    pheno = np.stack([a[:, 4], 0.8 * a[:, M - 3]], axis=1) + noise(n, 2, 8)
    pheno[3, 1] = np.nan                                   # the second trait has its own pattern of missing values
    kw = dict(cov=cov, permutations=3, seed=4, max_iter=200, tol=1e-7)
    got = qtl.scan_em(ctx, pheno, rows=rows, **kw)
    assert got["coef_names"] == ("a", "d") and set(got) >= {"lod", "coef", "sigma2", "iters", "status", "rank", "n_used", "perm_max"}
    for t in range(2):
        use = np.isfinite(pheno[:, t])
        yk = np.where(use, pheno[:, t], 0.0)[:, None]
        ref = R.reference_scan_em(o, cs, yk, use, cov, max_iter=200, tol=1e-7)
        perm = qtl.permutations(n, 3, 4, use=use)
        ref_p = R.reference_scan_em(o, cs, qtl.null_residuals(yk, cov, use), use, cov, perm=perm, max_iter=200, tol=1e-7)
        cm = R.compared_markers(ref, cs, share=0.9, strict=False)
        print("trait %d: %.0f %% of the markers pass the pivot precondition" % (t, 100 * cm.mean()))
        one = dict(lod=got["lod"][t:t + 1], coef=got["coef"][t:t + 1], sigma2=got["sigma2"][t:t + 1], iters=got["iters"][t:t + 1],
                   status=got["status"][t:t + 1], rank=got["rank"][t], n_used=got["n_used"][t], rss0=ref["rss0"], perm_max=None)
        R.compare_em(one, dict(ref, perm_max=ref["perm_max"]), cs, "qtl.scan_em trait %d" % t, share=0.9, strict=False)
        # (a chromosome's maximum is compared where every marker of it passes)
        whole = np.array([cm[cs[c]:cs[c + 1]].all() for c in range(len(cs) - 1)])
        err_p = np.abs(got["perm_max"][:, t:t + 1] - ref_p["perm_max"])[:, :, whole].max() if whole.any() else 0.0
        print("trait %d perm_max %.3g over %d chromosomes" % (t, err_p, whole.sum()))
        assert err_p <= ATOL and got["n_used"][t, 0] == n - t
    thr = qtl.thresholds(got["perm_max"])
    assert thr["genome"].shape == (2, 2)
    qtl.peaks(got["lod"], ped.pos, cs, thr["genome"][0])
    # the other three scans before and after, on the rows a sweep_qtl left in the context
    y0 = pheno[:, :1]
    sel = qtl.select_every(cs, 4)
    single = ctx.sweep_qtl(y0, cov=cov)
    before = (ctx.qtl_scan_device(n, None, y0, cov=cov), ctx.qtl_scan2_device(n, None, sel, y0, cov=cov),
              ctx.qtl_scanx_device(n, None, y0, cov=cov, imprint=True))
    kept = ctx.qtl_scan_em_device(n, None, y0, cov=cov, max_iter=200, tol=1e-7)
    assert kept["lod"][0].tobytes() == got["lod"][0].tobytes() and kept["iters"][0].tobytes() == got["iters"][0].tobytes()
    after = (ctx.qtl_scan_device(n, None, y0, cov=cov), ctx.qtl_scan2_device(n, None, sel, y0, cov=cov),
             ctx.qtl_scanx_device(n, None, y0, cov=cov, imprint=True))
    assert before[0]["lod"].tobytes() == single["lod"].tobytes()
    for b, a_ in zip(before, after):
        for k in b:
            if b[k] is not None:
                assert b[k].tobytes() == a_[k].tobytes(), k
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_em_device(n - 1, None, y0[:-1], cov=cov[:-1])
    ctx.upload_map(ped.pos, ped.chromstarts)
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_em_device(n, None, y0, cov=cov)
    ctx.close()


def test_cli_qtlem(capi, tmp_path):
    """cnF2freq --qtlem on an F2 of 14 on two chromosomes written to files: two traits of which one has missing values of its
    own, a covariate, imprinting, 5 permutations.  Every figure of the file is qtl.scan_em's on host.Run.from_files of the same
    files, to the printed digits; --output is the same bytes with and without --qtlem; --qtl and --qtlem together write the
    files they write alone."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    from test_gpu_qtl2 import write_f2_files
    ped = synth.make_f2(14, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n, M, cs = 14, ped.n_markers, np.asarray(ped.chromstarts)
    g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
    age = np.round(synth.uniform(5, np.arange(n)) * 10.0, 3)
    y = np.stack([g(4) + noise(n, 1, 2)[:, 0], noise(n, 1, 3)[:, 0] * 4.0 + g(12)], axis=1)
    y[3, 1] = np.nan
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id w age h"] + ["%s %s %s %s" % (names[i], cell(y[i, 0]), cell(age[i]), cell(y[i, 1])) for i in range(n)]
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--phenofile", str(ph),
            "--qtl-covariates", "age", "--qtl-permutations", "5", "--qtl-seed", "4"]
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    p = lambda name: str(tmp_path / name)
    eopts = ["--qtl-em-iterations", "300", "--qtl-em-tol", "1e-7"]
    run("--output", p("a.out"), "--qtl", p("q1.txt"))
    run("--output", p("b.out"), "--qtlem", p("qe.txt"), *eopts)
    run("--output", p("c.out"), "--qtl", p("q1b.txt"), "--qtlem", p("qeb.txt"), *eopts)
    subprocess.run(base[:10] + ["--output", p("d.out")], capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    read = lambda name: open(p(name), "rb").read()
    assert read("a.out") == read("b.out") == read("c.out") == read("d.out")
    assert read("q1.txt") == read("q1b.txt") and read("qe.txt") == read("qeb.txt")
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    want = qtl.scan_em(ctx, y, cov=age[:, None], permutations=5, seed=4, max_iter=300, tol=1e-7)
    ctx.close()
    r.close()
    thr = qtl.thresholds(want["perm_max"])
    tables = read("qe.txt").decode().strip("\n").split("\n\n")
    assert len(tables) == 2
    worst, big = 0.0, 0.0
    for t, tab in enumerate(tables):
        lines = [ln.split("\t") for ln in tab.split("\n")]
        assert lines[0] == ["trait", ["w", "h"][t]] and len(lines) == 1 + M + 1
        for m, x in enumerate(lines[1:1 + M]):
            c = int(np.searchsorted(cs, m, side="right") - 1)
            assert len(x) == 8 + 2 and int(x[0]) == c + 1 and int(x[2]) == want["n_used"][t, c] == n - t
            assert int(x[3]) == want["rank"][t, m] and int(x[6]) == want["iters"][t, m] and int(x[7]) == want["status"][t, m]
            figures = [(x[1], ped.pos[m]), (x[4], want["lod"][t, m])]
            for text, v in zip([x[5]] + x[8:], [want["sigma2"][t, m]] + list(want["coef"][t, m])):
                assert (text == "-") == bool(np.isnan(v))
                if text != "-":
                    figures.append((text, v))
            for text, value in figures:
                assert len(text.split(".")[1]) == 5
                worst = max(worst, abs(float(text) - value) / max(1.0, abs(value)))
            big = max(big, want["lod"][t, m])
        x = lines[1 + M]
        assert x[:2] == ["threshold", "lod"] and float(x[2]) > 0.0
        for a in range(2):
            worst = max(worst, abs(float(x[2 + a]) - thr["genome"][a, t]))
    print("file against qtl.scan_em: %.3g; largest LOD %.2f" % (worst, big))
    assert worst <= 0.51e-5 and big > 1.0
