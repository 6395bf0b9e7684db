"""GPU suite: the binary-trait single-locus scan (cnf2_qtl_scan_binary, cnf2_set_qtlbin_columns, Context.qtl_scan_binary,
qtl.scan_binary, cnF2freq --qtlbin).  Logistic regression of every marker and 0/1 phenotype column by Newton's method, checked
against the explicit-design IRLS in numpy (tests/qtlbin_reference.py): a fixed number of iterations on hand-made rows at the
shapes where the lane walk of 64 can go wrong, the stopping rule, a planted locus where the model must differ from the linear
scan of the same 0/1 column, the monotone likelihood, certain rows with the closed-form null, degenerate, separated and extreme
inputs, bit-equality, permutations, refusals, a swept cross and the command line.

The fit kernel is compiled once per width of X0 (qtlbin_fit_kernel<K + 1>) and the design decides the stride and the order of
coef.  Which test compares which instance and design with the yardstick's values:

    instance  K  case                                               design
    <1>       0  CASES[1] n 64;  WIDTH_CASES[6] n 64                (a, d); (a, i)
    <2>       1  planted, monotone, empty round (n 130, 66 used);   (a, d)
                 WIDTH_CASES[5] n 41, T 2                           (a, i)
    <3>       2  CASES[0] n 41; CASES[2] n 67 skipped; CASES[4]     (a, d); (a, d, i); (a)
    <4>       3  WIDTH_CASES[0] n 63                                (a, i)
    <5>       4  WIDTH_CASES[1] n 65                                (a, d)
    <6>       5  WIDTH_CASES[2] n 96, skipped                       (a, d, i)
    <7>       6  WIDTH_CASES[3] n 127, mask                         (a)
    <8>       7  WIDTH_CASES[4] n 129                               (a, i)
    <9>       8  CASES[3] n 130, T 2, P 5                           (a, d, i)

CASES run in test_fixed_iterations, WIDTH_CASES in test_every_width_and_design (fixed iterations and the stopping rule); the
column tiles across the observed/permuted boundary, the design (a, i) with i dropped, a round of the lane walk with nobody in
it and the threshold n_c = W + 1 of the design (a, i) have tests of their own at the end."""
import numpy as np
import pytest

import qtlbin_reference as R
from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, noise

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod", "coef", "iters", "status", "rank", "ll0", "n_ones", "n_used", "perm_max")
CS = chromstarts_of(CHROM_LENS)
LN10 = np.log(10.0)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens=CHROM_LENS):
    """a context that holds a map only: what cnf2_qtl_scan_binary needs"""
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


# ------------------------------------------------------------------------------------- 2. fixed iterations, the same bits
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "n%d-K%d-%s%s-T%d-P%d-it%d%s" % (
    c[0], c[1], "i" if c[2] else "m", "-add" if c[3] else "", c[5], c[6], c[9], "-mask" if c[7] else "-skip" if c[8] else ""))
def test_fixed_iterations(capi, case):
    """every output after exactly max_iter iterations against the yardstick at all 84 markers; rank as cnf2_qtl_scanx's; the
    same bits with column tiles of 1 and 4, on a second call, from device rows, into device outputs and with another batching
    of the sweeps"""
    import torch
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    origin, pheno, cov, use, perm = R.make_case(*case)
    ref = R.case_reference(case)
    # the conditions of the comparison, on the references alone, before anything runs: over the cases together at least 0.99
    # of the cells are compared and at most 0.01 are near
    R.assert_conditions([R.case_reference(c) for c in R.CASES])
    R.compared_cells(ref, CS)
    ctx, _ = map_context(capi)
    kw = dict(cov=cov, imprint=imprint, use=use, perm=perm, additive=additive, max_iter=max_iter, tol=-1.0)
    got = ctx.qtl_scan_binary(origin, pheno, **kw)
    R.compare_bin(got, ref, CS, "n %d K %d imprint %d additive %d T %d P %d max_iter %d" % (n, K, imprint, additive, T, P, max_iter))
    fitted = got["rank"] > 0
    assert np.all(got["iters"][:, fitted] == max_iter) and np.all(got["status"][:, fitted] == 1)
    x = ctx.qtl_scanx(origin, np.nan_to_num(pheno), cov=cov, imprint=imprint, use=use, additive=additive)
    assert np.array_equal(got["rank"], x["rank"][:, 1 if imprint else 0]) and np.array_equal(got["n_used"], x["n_used"])
    if skipped:
        assert got["n_used"][3] == n - 2 and got["n_used"][0] == n
    if mask:
        assert np.all(got["n_used"] == n - 2)
    same_bits(got, ctx.qtl_scan_binary(origin, pheno, **kw))
    for cap in (1, 4):
        ctx.set_qtlbin_columns(cap)
        same_bits(got, ctx.qtl_scan_binary(origin, pheno, **kw))
    ctx.set_qtlbin_columns(0)
    ctx.set_batch_jobs(5)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan_binary_device(n, d_o.data_ptr(), pheno, **kw))
    ctx.set_batch_jobs(0)
    d = device_outputs(capi, got)
    ctx.qtl_scan_binary_device(n, d_o.data_ptr(), pheno, out={k: None if v is None else v.data_ptr() for k, v in d.items()},
                               flags=capi.OUT_DEVICE, **kw)
    ctx.sync()
    same_bits(got, {k: None if v is None else v.cpu().numpy() for k, v in d.items()})
    ctx.close()


# ------------------------------------------------------------------------------------- 3. stopping rule, not HK in disguise
def test_stopping_rule_and_not_haley_knott(capi):
    p = R.PLANTED
    ref, hk = R.planted_reference(), R.planted_linear_reference()
    origin, _, pheno, z = R.planted_case()
    R.assert_anchor(ref, "planted")                        # on the yardstick alone, before anything of the product runs
    R.compared_cells(ref, CS)
    assert ref["near"].mean() <= 0.01
    R.assert_planted(ref, hk)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_binary(origin, pheno, cov=z, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_bin(got, ref, CS, "planted locus, tol %g" % p["tol"])
    assert got["lod"][0].argmax() == p["marker"] and np.all(got["status"] == 0)
    one = ctx.qtl_scan(origin, pheno, cov=z)
    err = np.abs(one["lod"] - hk["lod"][0]).max()
    print("the linear scan of the same column against its reference: %.3g" % err)
    assert err <= ATOL and one["lod"][0].argmax() == p["marker"]
    assert np.abs(got["lod"] - one["lod"]).max() > 0.2     # the product's two scans differ as the references do
    short = ctx.qtl_scan_binary(origin, pheno, cov=z, max_iter=p["short"], tol=p["tol"])
    ok = ~ref["near"]
    assert np.array_equal((short["status"] == 1)[ok], (ref["iters"] > p["short"])[ok])
    assert np.array_equal(short["iters"][ok], np.minimum(ref["iters"], p["short"])[ok])
    ctx.close()


# ------------------------------------------------------------------------------------- 4. monotone
def test_monotone(capi):
    ref = R.monotone_reference()
    steps = ref["trace"][0][:, list(R.MONOTONE)]
    assert np.all(np.diff(steps, axis=1) >= -1e-12)        # on the yardstick first
    origin, _, pheno, z = R.planted_case()
    ctx, _ = map_context(capi)
    lods = np.stack([ctx.qtl_scan_binary(origin, pheno, cov=z, max_iter=k, tol=-1.0)["lod"][0] for k in R.MONOTONE], axis=1)
    ctx.close()
    print("LOD after %s iterations: smallest step %.3g, against the yardstick %.3g" %
          (R.MONOTONE, np.diff(lods, axis=1).min(), np.abs(lods - steps).max()))
    assert np.all(np.diff(lods, axis=1) >= -1e-12)
    assert np.abs(lods - steps).max() <= ATOL


# ------------------------------------------------------------------------------------- 5. certain rows and K = 0
def test_certain_rows_and_no_covariates(capi):
    n = 41
    _, k = R.soft_rows(n, CHROM_LENS, 6)
    origin = R.certain_rows(k)
    y = R.bernoulli(0.3 + 1.0 * R.CODES["a"][k][:, [3, 40]], 9)
    ref = R.reference_scan_binary(origin, CS, y, max_iter=50, tol=1e-7)
    assert R.compared_cells(ref, CS, share=1.0).all()      # on the reference alone: every cell stays within ETA_MAX (2.3 here)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_binary(origin, y)
    ctx.close()
    n1 = y.sum(axis=0)[:, None]
    closed = n1 * np.log(n1 / n) + (n - n1) * np.log((n - n1) / n)
    print("ll0 against the closed form: %.3g" % np.abs(got["ll0"] - closed).max())
    assert np.abs(got["ll0"] - closed).max() <= ATOL and np.array_equal(got["n_ones"], np.broadcast_to(n1, got["n_ones"].shape))
    R.compare_bin(got, ref, CS, "certain rows, K = 0", share=1.0)


# ------------------------------------------------------------------------------------- 6. degenerate and extreme inputs
def test_degenerate_and_extreme(capi):
    origin, at = R.degenerate_rows()
    n = origin.shape[0]
    y = R.bernoulli(np.zeros((n, 1)), 11)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_binary(origin, y, imprint=True)
    plain = ctx.qtl_scan_binary(origin, y)
    ref = R.reference_scan_binary(origin, CS, y, imprint=True)
    # (24 individuals separate at some markers; those cells lie outside ETA_MAX, so no share of compared cells is asked for)
    R.compare_bin(got, ref, CS, "degenerate rows", share=0)
    m = at["flat"]
    assert got["rank"][m] == 0 and got["lod"][0, m] == 0.0 and got["iters"][0, m] == 0 and np.isnan(got["coef"][0, m]).all()
    m = at["homozygous"]
    assert got["rank"][m] == 1 and np.isfinite(got["coef"][0, m, 0]) and np.isnan(got["coef"][0, m, 1:]).all()
    m = at["symmetric"]
    assert got["rank"][m] == 2 and np.isnan(got["coef"][0, m, 2])
    assert got["lod"][0, m].tobytes() == plain["lod"][0, m].tobytes() and got["coef"][0, m, :2].tobytes() == plain["coef"][0, m].tobytes()
    m = at["zeros"]
    assert got["rank"][m] == 3 and np.isfinite(got["coef"][0, m]).all()
    assert np.isfinite(got["lod"]).all() and np.all(got["ll0"] < 0)
    # n_c = W (= 1 + 1 + 3) on chromosome 4: not scanned there
    few = origin.copy()
    few[5:, CS[4]:CS[5]] = 0.0
    z = noise(n, 1, 12)
    y5 = y.copy()
    y5[:5, 0] = [0, 1, 0, 1, 1]
    got = ctx.qtl_scan_binary(few, y5, cov=z, imprint=True)
    on4 = slice(CS[4], CS[5])
    assert got["n_used"][4] == 5 and np.all(got["rank"][on4] == 0) and np.all(got["lod"][:, on4] == 0.0)
    assert np.isnan(got["coef"][:, on4]).all() and got["ll0"][0, 4] == 0.0 and got["n_ones"][0, 4] == 3 and np.all(got["rank"][CS[5]:] > 0)
    # a trait that is constant on chromosome 4 (its five individuals there) is not scanned there, the column beside it is
    few[5:7, CS[4]:CS[5]] = origin[5:7, CS[4]:CS[5]]
    two = np.concatenate([y5, y5], axis=1)
    two[:7, 0] = 1.0
    two[:7, 1] = [0, 1, 0, 1, 1, 0, 1]
    got = ctx.qtl_scan_binary(few, two, additive=True)
    assert got["n_used"][4] == 7 and np.all(got["rank"][on4] == 1)
    assert got["ll0"][0, 4] == 0.0 and np.all(got["lod"][0, on4] == 0.0) and np.isnan(got["coef"][0, on4]).all() and np.all(got["iters"][0, on4] == 0)
    assert got["ll0"][1, 4] < 0.0 and np.all(got["iters"][1, on4] > 0) and np.isfinite(got["coef"][1, on4]).all()
    assert np.all(got["ll0"][0, :4] < 0.0) and got["n_ones"][0, 4] == 7
    ctx.close()
    # a covariate that is constant over everybody: X0 is singular and nothing is scanned
    o16, _ = R.soft_rows(16, (3,), 5)
    ctx, _ = map_context(capi, (3,))
    y16 = R.bernoulli(np.zeros((16, 1)), 4)
    got = ctx.qtl_scan_binary(o16, y16, cov=np.full((16, 1), 0.5))
    assert np.all(got["rank"] == 0) and np.all(got["lod"] == 0.0) and np.isnan(got["coef"]).all() and got["n_used"][0] == 16
    assert got["ll0"][0, 0] == 0.0 and 0 < got["n_ones"][0, 0] < 16
    # eta of +-700 and more through a huge covariate: finite outputs
    big = np.where(y16 > 0, 1.0, -1.0) * 700.0 + noise(16, 1, 13)
    got = ctx.qtl_scan_binary(o16, y16, cov=big)
    assert np.isfinite(got["lod"]).all() and np.all(got["lod"] >= 0) and np.isfinite(got["ll0"]).all() and np.isin(got["status"], (0, 1, 2)).all()
    ctx.close()


def test_separated(capi):
    """n = 17, K = 1, imprint: the reference shows diverging coefficients at several markers"""
    origin, y, z = R.separated_case()
    ref = R.reference_scan_binary(origin, CS, y, None, z, imprint=True, max_iter=50, tol=1e-7)
    wild = (np.abs(np.nan_to_num(ref["coef"])).max(axis=2) > 15) | (ref["status"] == 2)
    print("separated: %d markers with |coef| > 15 or a breakdown in the reference" % wild.sum())
    assert wild.sum() >= 2
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_binary(origin, y, cov=z, imprint=True, max_iter=50, tol=1e-7)
    ctx.close()
    assert np.all(got["ll0"] < 0)
    bound = np.repeat(-got["ll0"] / LN10 + ATOL, np.diff(CS), axis=1)
    assert np.isfinite(got["lod"]).all() and np.all(got["lod"] >= 0) and np.all(got["lod"] <= bound)
    assert np.isin(got["status"], (0, 1, 2)).all()
    assert np.all(np.isnan(got["coef"]).sum(axis=2) == 3 - got["rank"][None, :])       # nothing is NaN but a dropped effect
    R.compare_bin(got, ref, CS, "separated", share=0, strict=False)


# ------------------------------------------------------------------------------------- 7. permutations and refusals
def test_identity_permutation_and_refusals(capi):
    case = R.CASES[0]
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    origin, pheno, cov, _, _ = R.make_case(*case)
    use = np.ones(n, bool)
    use[4] = False
    ctx, cs = map_context(capi)
    C, M = len(cs) - 1, int(cs[-1])
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3, use=use)[0], ident])
    got = ctx.qtl_scan_binary(origin, pheno, cov=cov, imprint=True, use=use, perm=perm)
    observed = np.stack([got["lod"][:, cs[c]:cs[c + 1]].max(axis=1) for c in range(C)], axis=1)          # [T][C]
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed) and np.all(observed > 0.0)
    # refused, with the outputs left alone
    twice = ident.copy()
    twice[3] = 2
    bad_cov = cov.copy()
    bad_cov[7, 0] = np.inf

    def with_value(v):
        y = pheno.copy()
        y[6, 1] = v
        return y
    base = dict(pheno=pheno, cov=cov, perm=ident[None], max_iter=10, tol=1e-6)
    refusals = [dict(max_iter=0), dict(max_iter=1001), dict(tol=np.nan), dict(tol=np.inf), dict(tol=-np.inf), dict(cov=np.zeros((n, 9))),
                dict(perm=twice[None]), dict(cov=bad_cov), dict(pheno=with_value(0.5)), dict(pheno=with_value(2.0)),
                dict(pheno=with_value(np.nan))]
    poisoned = lambda: dict(lod=np.full((T, M), 77.0), coef=np.full((T, M, 3), 77.0), iters=np.full((T, M), 77, np.int32),
                            status=np.full((T, M), 77, np.int32), rank=np.full(M, 77, np.int32), ll0=np.full((T, C), 77.0),
                            n_ones=np.full((T, C), 77, np.int32), n_used=np.full(C, 77, np.int32), perm_max=np.full((1, T, C), 77.0))
    import torch
    d_o = torch.from_numpy(origin).cuda()
    for change in refusals:
        kw = dict(base, **change)
        out = poisoned()
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_binary(origin, kw["pheno"], cov=kw["cov"], imprint=True, use=use, perm=kw["perm"], max_iter=kw["max_iter"],
                                tol=kw["tol"], out=out)
        assert all(np.all(v == 77) for v in out.values()), change
        d = device_outputs(capi, out)
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_binary_device(n, d_o.data_ptr(), kw["pheno"], cov=kw["cov"], imprint=True, use=use, perm=kw["perm"],
                                       max_iter=kw["max_iter"], tol=kw["tol"], out={k: v.data_ptr() for k, v in d.items()},
                                       flags=capi.OUT_DEVICE)
        ctx.sync()
        assert all(bool((x == 77).all()) for x in d.values()), change
    # the same values at an individual that is not used are accepted
    for v in (0.5, 2.0, np.nan):
        y = pheno.copy()
        y[4, 1] = v
        same_bits(got, ctx.qtl_scan_binary(origin, y, cov=cov, imprint=True, use=use, perm=perm))
    ctx.close()


# ------------------------------------------------------------------------------------- 8. end to end
def test_end_to_end_on_a_swept_cross(capi):
    """qtl.scan_binary on an F2 the product sweeps itself: within 1e-9 of the yardstick on the product's own origin_rows at the
    cells that pass the conditions; thresholds and peaks read it; the other four scans before and after on the rows a sweep_qtl
    left in the context; CNF2_ERR_STATE for another n"""
    ped = synth.make_f2(24, 17, 2, seed=7)
    n, M = len(ped.dous), ped.n_markers
    cs = np.asarray(ped.chromstarts)
    cov = synth.uniform(21, np.arange(n)).reshape(n, 1)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = qtl.origin_rows(ctx)
    o = rows.cpu().numpy()
    a = o[:, :, 3] - o[:, :, 0]
    # (24 individuals separate easily: of the strengths tried on the yardstick alone, this one leaves 0.97 and 0.94 of the two
    # traits' cells within ETA_MAX; 1.5 and 1.2 left 0.89 and 0.56)
    pheno = R.bernoulli(np.stack([0.6 * a[:, 4], 0.6 * a[:, M - 3] + 0.2], axis=1), 8)
    pheno[3, 1] = np.nan                                   # the second trait has its own pattern of missing values
    assert np.all(np.nansum(pheno, axis=0) >= 6) and np.all(np.nansum(1 - pheno, axis=0) >= 6)      # both classes, everywhere
    kw = dict(cov=cov, permutations=3, seed=4, max_iter=50, tol=1e-7)
    got = qtl.scan_binary(ctx, pheno, rows=rows, **kw)
    assert got["coef_names"] == ("a", "d") and set(got) >= {"lod", "coef", "iters", "status", "rank", "ll0", "n_ones", "n_used", "perm_max"}
    for t in range(2):
        use = np.isfinite(pheno[:, t])
        yk = np.where(use, pheno[:, t], 0.0)[:, None]
        perm = qtl.permutations(n, 3, 4, use=use)
        ref = R.reference_scan_binary(o, cs, yk, use, cov, perm=perm, max_iter=50, tol=1e-7)
        cc = R.compared_cells(ref, cs, share=0.9, strict=False)
        print("trait %d: %.0f %% of the cells pass the conditions" % (t, 100 * cc.mean()))
        one = dict(lod=got["lod"][t:t + 1], coef=got["coef"][t:t + 1], iters=got["iters"][t:t + 1], status=got["status"][t:t + 1],
                   rank=got["rank"][t], n_used=got["n_used"][t], ll0=got["ll0"][t:t + 1], n_ones=got["n_ones"][t:t + 1], perm_max=None)
        R.compare_bin(one, dict(ref, perm_max=ref["perm_max"][:0]), cs, "qtl.scan_binary trait %d" % t, share=0.9, strict=False)
        # (a chromosome's maximum is compared where every marker of it passes, in every permuted column too)
        fine = cc[0] & (ref["maxeta_all"][:, 0] <= R.ETA_MAX).all(axis=0)
        whole = np.array([fine[cs[c]:cs[c + 1]].all() for c in range(len(cs) - 1)])
        err_p = np.abs(got["perm_max"][:, t:t + 1] - ref["perm_max"])[:, :, whole].max() if whole.any() else 0.0
        print("trait %d perm_max %.3g over %d chromosomes" % (t, err_p, whole.sum()))
        assert err_p <= ATOL and got["n_used"][t, 0] == n - t
    thr = qtl.thresholds(got["perm_max"])
    assert thr["genome"].shape == (2, 2)
    qtl.peaks(got["lod"], ped.pos, cs, thr["genome"][0])
    # the other four scans before and after, on the rows a sweep_qtl left in the context
    y0 = pheno[:, :1]
    sel = qtl.select_every(cs, 4)
    single = ctx.sweep_qtl(y0, cov=cov)
    others = lambda: (ctx.qtl_scan_device(n, None, y0, cov=cov), ctx.qtl_scan2_device(n, None, sel, y0, cov=cov),
                      ctx.qtl_scanx_device(n, None, y0, cov=cov, imprint=True),
                      ctx.qtl_scan_em_device(n, None, y0, cov=cov, max_iter=50, tol=1e-7))
    before = others()
    kept = ctx.qtl_scan_binary_device(n, None, y0, cov=cov, max_iter=50, tol=1e-7)
    assert kept["lod"][0].tobytes() == got["lod"][0].tobytes() and kept["iters"][0].tobytes() == got["iters"][0].tobytes()
    after = others()
    assert before[0]["lod"].tobytes() == single["lod"].tobytes()
    for b, a_ in zip(before, after):
        for k in b:
            if b[k] is not None:
                assert b[k].tobytes() == a_[k].tobytes(), k
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_binary_device(n - 1, None, y0[:-1], cov=cov[:-1])
    ctx.upload_map(ped.pos, ped.chromstarts)
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_binary_device(n, None, y0, cov=cov)
    ctx.close()


def test_cli_qtlbin(capi, tmp_path):
    """cnF2freq --qtlbin on an F2 of 14 on two chromosomes written to files: two 0/1 traits of which one has missing values of
    its own, a continuous trait that --qtlbin leaves out, a covariate, 5 permutations.  Every figure of the file is
    qtl.scan_binary's on host.Run.from_files of the same files, to the printed digits; --output is the same bytes with and
    without --qtlbin; --qtl and --qtlbin together write the files they write alone."""
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
    y = R.bernoulli(np.stack([0.8 * g(4), 0.8 * g(12) + 0.3], axis=1), 2)
    y[3, 1] = np.nan
    w = noise(n, 1, 3)[:, 0]
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id b age w h"] + ["%s %d %s %s %s" % (names[i], int(y[i, 0]), cell(age[i]), cell(w[i]), cell(y[i, 1])) for i in range(n)]
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--phenofile", str(ph),
            "--qtl-covariates", "age", "--qtl-permutations", "5", "--qtl-seed", "4"]
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    p = lambda name: str(tmp_path / name)
    bopts = ["--qtl-binary-iterations", "30", "--qtl-binary-tol", "1e-6"]
    run("--output", p("a.out"), "--qtl", p("q1.txt"))
    run("--output", p("b.out"), "--qtlbin", p("qb.txt"), *bopts)
    run("--output", p("c.out"), "--qtl", p("q1b.txt"), "--qtlbin", p("qbb.txt"), *bopts)
    subprocess.run(base[:10] + ["--output", p("d.out")], capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    read = lambda name: open(p(name), "rb").read()
    assert read("a.out") == read("b.out") == read("c.out") == read("d.out")
    assert read("q1.txt") == read("q1b.txt") and read("qb.txt") == read("qbb.txt")
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    want = qtl.scan_binary(ctx, y, cov=age[:, None], permutations=5, seed=4, max_iter=30, tol=1e-6)
    ctx.close()
    r.close()
    thr = qtl.thresholds(want["perm_max"])
    tables = read("qb.txt").decode().strip("\n").split("\n\n")
    assert len(tables) == 2
    worst = 0.0
    for t, tab in enumerate(tables):
        lines = [ln.split("\t") for ln in tab.split("\n")]
        assert lines[0] == ["trait", ["b", "h"][t]] and len(lines) == 1 + M + 1
        for m, x in enumerate(lines[1:1 + M]):
            c = int(np.searchsorted(cs, m, side="right") - 1)
            assert len(x) == 7 + 2 and int(x[0]) == c + 1 and int(x[2]) == want["n_used"][t, c] == n - t
            assert int(x[3]) == want["rank"][t, m] and int(x[5]) == want["iters"][t, m] and int(x[6]) == want["status"][t, m]
            figures = [(x[1], ped.pos[m]), (x[4], want["lod"][t, m])]
            for text, v in zip(x[7:], want["coef"][t, m]):
                assert (text == "-") == bool(np.isnan(v))
                if text != "-":
                    figures.append((text, v))
            for text, value in figures:
                assert len(text.split(".")[1]) == 5
                worst = max(worst, abs(float(text) - value) / max(1.0, abs(value)))
        x = lines[1 + M]
        assert x[:2] == ["threshold", "lod"]
        for a in range(2):
            worst = max(worst, abs(float(x[2 + a]) - thr["genome"][a, t]))
    print("file against qtl.scan_binary: %.3g; largest LOD %.2f" % (worst, want["lod"].max()))
    assert worst <= 0.51e-5 and want["lod"].max() > 0.5


# ------------------------------------------------------------------------------------- 9. every width of X0, every design
def width_reference(case, stop):
    return R.case_reference(case, **(R.WIDTH_STOP if stop else {}))


def assert_i_dropped_as_plain(got, plain):
    """wherever the (a, i) run reports rank 1 with i dropped, lod and the effect a have the bits of the run without imprinting;
    returns the number of such markers"""
    dropped = (got["rank"] == 1) & np.isnan(got["coef"][:, :, 1]).all(axis=0) & np.isfinite(got["coef"][:, :, 0]).any(axis=0)
    assert plain["coef"].shape[2] == 1
    assert got["lod"][:, dropped].tobytes() == plain["lod"][:, dropped].tobytes()
    assert got["coef"][:, dropped, 0].tobytes() == plain["coef"][:, dropped, 0].tobytes()
    assert got["iters"][:, dropped].tobytes() == plain["iters"][:, dropped].tobytes()
    return int(dropped.sum())


@pytest.mark.parametrize("stop", (False, True), ids=("fixed", "stop"))
@pytest.mark.parametrize("case", R.WIDTH_CASES, ids=R.case_id)
def test_every_width_and_design(capi, case, stop):
    """K = 3 .. 7 and the design (a, i), after exactly max_iter iterations and under the stopping rule (tol 1e-7): every output
    against the yardstick at all 84 markers, rank and n_used as cnf2_qtl_scanx's, the same bits on a second call.  No marker of
    these draws drops i (every rank of the (a, i) cases is 2, asserted on the reference), so the run without imprinting is
    compared at no marker here: test_additive_imprint_drops_i does that on the degenerate rows."""
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    origin, pheno, cov, use, perm = R.make_case(*case)
    ref = width_reference(case, stop)
    # on the references alone, before anything runs: over the seven cases together at least 0.99 of the cells are compared
    # and at most 0.01 are near; this case's own cells are all compared
    R.assert_conditions([width_reference(c, stop) for c in R.WIDTH_CASES])
    assert R.compared_cells(ref, CS, share=1.0).all()
    if stop:
        R.assert_anchor(ref, R.case_id(case))
        assert np.all(ref["status"] == 0)
    ai = imprint and additive
    if ai:
        assert np.all(ref["rank"] == 2)
    ctx, _ = map_context(capi)
    kw = dict(cov=cov, imprint=imprint, use=use, perm=perm, additive=additive)
    kw.update(R.WIDTH_STOP if stop else dict(max_iter=max_iter, tol=-1.0))
    got = ctx.qtl_scan_binary(origin, pheno, **kw)
    assert got["coef"].shape == (T, CS[-1], len(R.effects(additive, imprint)))
    R.compare_bin(got, ref, CS, "%s %s" % (R.case_id(case), "to tol 1e-7" if stop else "fixed"), share=1.0)
    if not stop:
        fitted = got["rank"] > 0
        assert np.all(got["iters"][:, fitted] == max_iter) and np.all(got["status"][:, fitted] == 1)
    x = ctx.qtl_scanx(origin, np.nan_to_num(pheno), cov=cov, imprint=imprint, use=use, additive=additive)
    assert np.array_equal(got["rank"], x["rank"][:, 1 if imprint else 0]) and np.array_equal(got["n_used"], x["n_used"])
    if skipped:
        assert got["n_used"][3] == n - 2 and got["n_used"][0] == n
    if mask:
        assert np.all(got["n_used"] == n - 2)
    same_bits(got, ctx.qtl_scan_binary(origin, pheno, **kw))
    if ai:
        assert assert_i_dropped_as_plain(got, ctx.qtl_scan_binary(origin, pheno, **dict(kw, imprint=False))) == 0
    ctx.close()


def test_additive_imprint_drops_i(capi):
    """The design (a, i) on the degenerate rows, with a covariate: at the homozygous and the symmetric marker i vanishes, the
    rank is 1 with i dropped (coef[..., 1] NaN), and lod and a have the bits of the additive run without imprinting; where
    both effects are kept, coef place 1 is i: the yardstick's."""
    origin, at = R.degenerate_rows()
    n = origin.shape[0]
    y = R.bernoulli(np.zeros((n, 1)), 11)
    z = noise(n, 1, 12)
    ref = R.reference_scan_binary(origin, CS, y, None, z, imprint=True, additive=True)
    for m in (at["homozygous"], at["symmetric"]):         # on the reference alone
        assert ref["rank"][m] == 1 and np.isfinite(ref["coef"][0, m, 0]) and np.isnan(ref["coef"][0, m, 1])
    assert ref["rank"][at["flat"]] == 0 and ref["rank"][at["zeros"]] == 2
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_binary(origin, y, cov=z, imprint=True, additive=True)
    plain = ctx.qtl_scan_binary(origin, y, cov=z, additive=True)
    ctx.close()
    # (24 individuals separate at some markers; those cells lie outside ETA_MAX, so no share of compared cells is asked for)
    R.compare_bin(got, ref, CS, "degenerate rows, (a, i)", share=0)
    for m in (at["homozygous"], at["symmetric"]):
        assert got["rank"][m] == 1 and np.isfinite(got["coef"][0, m, 0]) and np.isnan(got["coef"][0, m, 1]) and got["lod"][0, m] > 0.0
    assert assert_i_dropped_as_plain(got, plain) >= 2
    m = at["flat"]
    assert got["rank"][m] == 0 and got["lod"][0, m] == 0.0 and np.isnan(got["coef"][0, m]).all()


# ------------------------------------------------------------------------------------- 10. column tiles across T
def test_column_tiles_across_the_permuted_boundary(capi):
    """T = 2, P = 5: 12 columns, the first two observed.  Caps of 3 and 5 put observed and permuted columns into one launch
    (columns 0 .. 2, resp. 0 .. 4), a cap of 12 all of them; the bits are those of the default tiling, and of the yardstick."""
    case = R.CASES[3]
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    assert (T, P) == (2, 5)
    origin, pheno, cov, use, perm = R.make_case(*case)
    ref = R.case_reference(case)
    R.compared_cells(ref, CS)
    ctx, _ = map_context(capi)
    kw = dict(cov=cov, imprint=imprint, use=use, perm=perm, additive=additive, max_iter=max_iter, tol=-1.0)
    got = ctx.qtl_scan_binary(origin, pheno, **kw)
    R.compare_bin(got, ref, CS, "12 columns, default tiling")
    for cap in (3, 5, 12):
        ctx.set_qtlbin_columns(cap)
        same_bits(got, ctx.qtl_scan_binary(origin, pheno, **kw))
    ctx.set_qtlbin_columns(0)
    same_bits(got, ctx.qtl_scan_binary(origin, pheno, **kw))
    ctx.close()


# ------------------------------------------------------------------------------------- 11. two edges of the lane walk
def test_a_round_with_nobody_in_it(capi):
    """n = 130 with individuals 64 .. 127 unused: every lane's second step is masked, the third round holds two individuals"""
    p = R.EMPTY_ROUND
    origin, pheno, z, use = R.empty_round_case()
    ref = R.empty_round_reference()
    R.assert_anchor(ref, "empty round")                    # on the yardstick alone, before anything of the product runs
    cc = R.compared_cells(ref, CS, share=p["share"])
    print("empty round: %.3f of the cells compared, %d near" % (cc.mean(), ref["near"].sum()))
    assert ref["near"].mean() <= 0.01 and np.all(ref["n_used"] == 66)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_binary(origin, pheno, cov=z, use=use, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_bin(got, ref, CS, "n 130, 64 .. 127 unused", share=p["share"])
    assert np.all(got["n_used"] == 66)
    same_bits(got, ctx.qtl_scan_binary(origin, pheno, cov=z, use=use, max_iter=p["max_iter"], tol=p["tol"]))
    ctx.close()


@pytest.mark.parametrize("n_c", (7, 6))
def test_scan_threshold_of_the_additive_imprint_design(capi, n_c):
    """(a, i) with K = 3, W = 6: a chromosome with 7 individuals is scanned, one with 6 is not.  Seven individuals on six
    columns separate, so no values are compared: what test_separated asserts"""
    origin, y, z = R.threshold_case(n_c)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_binary(origin, y, cov=z, imprint=True, additive=True, max_iter=50, tol=1e-7)
    x = ctx.qtl_scanx(origin, y, cov=z, imprint=True, additive=True)
    ctx.close()
    R.assert_threshold(got, n_c)
    assert np.array_equal(got["rank"], x["rank"][:, 1]) and np.array_equal(got["n_used"], x["n_used"])
