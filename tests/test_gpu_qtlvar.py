"""GPU suite: the variance-QTL single-locus scan (cnf2_qtl_scan_var, cnf2_set_qtlvar_columns, Context.qtl_scan_var,
qtl.scan_var, cnF2freq --qtlvar).  The double generalised linear model of every marker and phenotype column -- mean-only,
variance-only and full fit from the null fit -- checked against the explicit-design iteration in numpy
(tests/qtlvar_reference.py): a fixed number of iterations on hand-made rows at the shapes where the lane walk of 64 and the
instances can go wrong, the stopping rule, a planted variance locus that a mean scan does not see, the monotone likelihood,
a step that is halved, degenerate and extreme inputs, bit-equality, permutations, refusals, a swept cross and the command
line.

The null and the fit kernel are compiled once per width of X0 (qtlvar_fit_kernel<K + 1>); n_var and the design are runtime
matters.  Which test compares which instance, n_var and design with the yardstick's values:

    instance  K  n_var  case                                          design
    <1>       0  0      CASES[3] n 64                                 (a, d)
    <2>       1  0      planted, monotone (n 130)                     (a, d)
              1  1      halving (n 41); empty round (n 130, 66 used)  (a, d, i); (a, d)
    <3>       2  0      CASES[0] n 41                                 (a, d)
              2  1      CASES[1] n 41                                 (a, d, i)
              2  2      CASES[5] n 67, skipped                        (a, d, i)
    <4>       3  3      CASES[2] n 63                                 (a, i)
              3  1      threshold n_c = 11, 10                        (a, i)
    <5>       4  2      CASES[4] n 65                                 (a, d)
    <6>       5  1      CASES[6] n 96                                 (a, d, i)
    <7>       6  0      CASES[7] n 127, mask                          (a)
    <8>       7  3      CASES[8] n 129                                (a, i)
    <9>       8  3      CASES[9] n 130, T 2, P 5                      (a, d, i)

CASES run in test_fixed_iterations."""
import numpy as np
import pytest

import qtlvar_reference as R
from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, noise

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod", "coef_mean", "coef_var", "iters", "status", "rank", "ll0", "n_used", "perm_max")
CS = chromstarts_of(CHROM_LENS)
LN10 = np.log(10.0)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens=CHROM_LENS):
    """a context that holds a map only: what cnf2_qtl_scan_var needs"""
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


# ------------------------------------------------------------------------------------- 1. fixed iterations, the same bits
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fixed_iterations(capi, case):
    """every output after exactly max_iter iterations against the yardstick at all 84 markers; rank as cnf2_qtl_scanx's; the
    same bits on a second call, with column caps 1, 4 and 0, from device rows, into device outputs and with another batching
    of the sweeps"""
    import torch
    n, K, n_var, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    origin, pheno, cov, use, perm = R.make_case(*case)
    ref = R.case_reference(case)
    # the conditions of the comparison, on the references alone, before anything runs: over the cases together at least 0.99
    # of the cells are compared and at most 0.01 are near
    R.assert_conditions([R.case_reference(c) for c in R.CASES])
    R.compared_cells(ref, CS, share=0)
    ctx, _ = map_context(capi)
    kw = dict(cov=cov, n_var=n_var, imprint=imprint, use=use, perm=perm, additive=additive, max_iter=max_iter, tol=-1.0)
    got = ctx.qtl_scan_var(origin, pheno, **kw)
    assert got["coef_mean"].shape == got["coef_var"].shape == (T, CS[-1], len(R.effects(additive, imprint)))
    R.compare_var(got, ref, CS, R.case_id(case), share=0)
    x = ctx.qtl_scanx(origin, np.nan_to_num(pheno), cov=cov, imprint=imprint, use=use, additive=additive)
    assert np.array_equal(got["rank"], x["rank"][:, 1 if imprint else 0]) and np.array_equal(got["n_used"], x["n_used"])
    if skipped:
        assert got["n_used"][3] == n - 2 and got["n_used"][0] == n
    if mask:
        assert np.all(got["n_used"] == n - 2)
    same_bits(got, ctx.qtl_scan_var(origin, pheno, **kw))
    for cap in (1, 4, 0):
        ctx.set_qtlvar_columns(cap)
        same_bits(got, ctx.qtl_scan_var(origin, pheno, **kw))
    ctx.set_batch_jobs(5)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan_var_device(n, d_o.data_ptr(), pheno, **kw))
    ctx.set_batch_jobs(0)
    d = device_outputs(capi, got)
    ctx.qtl_scan_var_device(n, d_o.data_ptr(), pheno, out={k: None if v is None else v.data_ptr() for k, v in d.items()},
                            flags=capi.OUT_DEVICE, **kw)
    ctx.sync()
    same_bits(got, {k: None if v is None else v.cpu().numpy() for k, v in d.items()})
    ctx.close()


# ------------------------------------------------------------------------------------- 2. stopping rule, not a mean scan in disguise
def test_stopping_rule_and_not_a_mean_scan(capi):
    p = R.PLANTED
    ref, hk = R.planted_reference(), R.planted_linear_reference()
    origin, _, pheno, z = R.planted_case()
    R.assert_anchor(ref, "planted")                        # on the yardstick alone, before anything of the product runs
    R.compared_cells(ref, CS)
    assert ref["near"].mean() <= 0.01 and np.all(ref["status"] == 0)
    R.assert_planted(ref, hk)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_var(origin, pheno, cov=z, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_var(got, ref, CS, "planted locus, tol %g" % p["tol"])
    assert abs(int(got["lod"][0, :, 2].argmax()) - p["marker"]) <= 1 and np.all(got["status"] == 0)
    x = ctx.qtl_scanx(origin, pheno, cov=z)
    err = np.abs(got["lod"][..., 0] - got["lod"][..., 2] - x["lod"][..., 0]).max()
    print("joint - variance LOD against qtl_scanx's LOD of the same design: %.3g" % err)
    assert x["lod"][0, p["marker"], 0] <= 1.0
    # (n_var = 0: mean-only against null is Haley-Knott's LOD; both sides stopped by 1e-7 LOD, which is what separates them)
    assert err <= 2 * p["tol"]
    tight = ctx.qtl_scan_var(origin, pheno, cov=z, max_iter=p["max_iter"], tol=1e-12)
    err = np.abs(tight["lod"][..., 0] - tight["lod"][..., 2] - x["lod"][..., 0]).max()
    print("... at tol 1e-12: %.3g" % err)
    assert err <= R.hk_identity_bound()
    short = ctx.qtl_scan_var(origin, pheno, cov=z, max_iter=p["short"], tol=p["tol"])
    ok = ~ref["near"]
    assert np.array_equal((short["status"] == 1)[ok], (ref["iters"] > p["short"])[ok])
    assert np.array_equal(short["iters"][ok], np.minimum(ref["iters"], p["short"])[ok])
    ctx.close()


# ------------------------------------------------------------------------------------- 3. monotone
def test_monotone(capi):
    ref = R.monotone_reference()
    steps = ref["trace"][0][:, list(R.MONOTONE)]
    assert np.all(np.diff(steps, axis=1) >= -1e-12)        # on the yardstick first
    origin, _, pheno, z = R.planted_case()
    ctx, _ = map_context(capi)
    lods = np.stack([ctx.qtl_scan_var(origin, pheno, cov=z, max_iter=k, tol=-1.0)["lod"][0, :, 0] for k in R.MONOTONE], axis=1)
    ctx.close()
    print("joint LOD after %s iterations: smallest step %.3g, against the yardstick %.3g" %
          (R.MONOTONE, np.diff(lods, axis=1).min(), np.abs(lods - steps).max()))
    assert np.all(np.diff(lods, axis=1) >= -1e-12)
    assert np.abs(lods - steps).max() <= ATOL


# ------------------------------------------------------------------------------------- 4. step halving
def test_step_halving(capi):
    """t(4) noise on 41 individuals: the yardstick's traces halve a step at some fits; the iterates agree"""
    p = R.HALVING
    ref = R.halving_reference()
    origin, pheno, z = R.halving_case()
    cc = R.compared_cells(ref, CS, share=0.9)
    halved = (ref["halvings"] >= 1) & cc[..., None] & ~ref["near"]
    print("halving: %d fits of %d take at least one halving, at most %d; %d near" %
          (halved.sum(), halved.size, ref["halvings"].max(), ref["near"].sum()))
    assert halved.sum() >= 1 and np.all(ref["status"][halved] == 0)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_var(origin, pheno, cov=z, n_var=p["n_var"], imprint=True, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_var(got, ref, CS, "halving", share=0.9)
    # the iterates: every fixed number of iterations up to the longest halved fit's
    for k in (1, 2, 3):
        rk = R.reference_scan_var(origin, CS, pheno, None, z, p["n_var"], imprint=True, max_iter=k, tol=-1.0)
        gk = ctx.qtl_scan_var(origin, pheno, cov=z, n_var=p["n_var"], imprint=True, max_iter=k, tol=-1.0)
        R.compare_var(gk, rk, CS, "halving, %d iterations" % k, share=0.9)
    ctx.close()


# ------------------------------------------------------------------------------------- 5. degenerate and extreme inputs
def test_degenerate_and_extreme(capi):
    n = 41
    origin, k = R.soft_rows(n, CHROM_LENS, 6)
    z = noise(n, 1, 12)
    y = R.gauss((n, 2), 11)
    ctx, _ = map_context(capi)
    # a trait that is constant on chromosome 4's mask (its 20 individuals there) is not scanned there, the column beside it is
    few = origin.copy()
    few[20:, CS[4]:CS[5]] = 0.0
    two = y.copy()
    two[:20, 0] = 1.25
    got = ctx.qtl_scan_var(few, two, cov=z, n_var=1)
    on4 = slice(CS[4], CS[5])
    assert got["n_used"][4] == 20 and np.all(got["rank"][on4] == 2)
    assert got["ll0"][0, 4] == 0.0 and np.all(got["lod"][0, on4] == 0.0) and np.all(got["iters"][0, on4] == 0)
    assert np.isnan(got["coef_mean"][0, on4]).all() and np.isnan(got["coef_var"][0, on4]).all() and np.all(got["status"][0, on4] == 0)
    assert got["ll0"][1, 4] != 0.0 and np.all(got["iters"][1, on4] > 0) and np.isfinite(got["coef_var"][1, on4]).all()
    assert np.all(got["ll0"][0, :4] != 0.0)
    # certain rows where every BB individual has the same trait value: the class variance goes to 0.  A numerical breakdown,
    # not a fault: every output finite, no LOD negative, status 1 or 2 at the fits with a variance part
    cert = R.certain_rows(k)
    yb = y[:, :1].copy()
    m = 40
    yb[k[:, m] == 3, 0] = 0.5
    assert 3 <= (k[:, m] == 3).sum() <= n - 6
    got = ctx.qtl_scan_var(cert, yb, max_iter=50, tol=1e-7)
    for key in ("lod", "ll0"):
        assert np.isfinite(got[key]).all(), key
    assert np.all(got["lod"] >= 0) and np.isin(got["status"], (0, 1, 2)).all()
    fitted = got["rank"] > 0
    assert np.isfinite(got["coef_mean"][0, fitted]).sum() == got["rank"].sum() == np.isfinite(got["coef_var"][0, fitted]).sum()
    print("a class variance of 0 at marker %d: status %s, iters %s, lod %s" % (m, got["status"][0, m], got["iters"][0, m], got["lod"][0, m]))
    assert np.all(np.isin(got["status"][0, m, 1:], (1, 2)))
    # Traits scaled by 1e150 and by 1e-150: log sigma^2 moves by +-690.8, next to QTLVAR_ETA_MAX = 700 (an individual whose
    # log variance lies 9.2 further out is a breakdown by the model's own rule) and, for 1e-150, squares of residuals next to
    # the smallest normal number.  So there: the call returns, every output is finite, no LOD is negative.  Scaled by 1e100
    # and by 1e-100 (log sigma^2 moves by +-460.5, squares stay normal) nothing but the units may move.
    base = ctx.qtl_scan_var(origin, y, cov=z, n_var=1, imprint=True, max_iter=50, tol=1e-9)
    for s in (1e150, 1e-150, 1e100, 1e-100):
        sc = ctx.qtl_scan_var(origin, y * s, cov=z, n_var=1, imprint=True, max_iter=50, tol=1e-9)
        assert np.isfinite(sc["lod"]).all() and np.all(sc["lod"] >= 0) and np.isfinite(sc["ll0"]).all(), s
        assert np.isin(sc["status"], (0, 1, 2)).all() and np.array_equal(sc["rank"], base["rank"]), s
        assert np.isfinite(sc["coef_mean"]).all() and np.isfinite(sc["coef_var"]).all(), s
        e_l = np.abs(sc["lod"] - base["lod"]).max()
        e_v = np.abs(sc["coef_var"] - base["coef_var"]).max()
        e_m = (np.abs(sc["coef_mean"] / s - base["coef_mean"]) / np.maximum(1.0, np.abs(base["coef_mean"]))).max()
        e_0 = np.abs(sc["ll0"] + sc["n_used"][None, :] * np.log(s) - base["ll0"]).max()
        print("trait times %g: lod %.3g, coef_var %.3g, coef_mean %.3g, ll0 %.3g, statuses %s" %
              (s, e_l, e_v, e_m, e_0, np.bincount(sc["status"].reshape(-1), minlength=3)))
        if s in (1e100, 1e-100):
            # (ll0 is of the order of n ln s = 1e4, so ATOL is taken relative to it)
            assert max(e_l, e_v, e_m) <= ATOL and e_0 <= ATOL * 1e4
            assert np.array_equal(sc["status"], base["status"])
    ctx.close()
    # a covariate that is constant over everybody: X0 is singular and nothing is scanned
    o16, _ = R.soft_rows(16, (3,), 5)
    ctx, _ = map_context(capi, (3,))
    got = ctx.qtl_scan_var(o16, R.gauss((16, 1), 4), cov=np.full((16, 1), 0.5))
    assert np.all(got["rank"] == 0) and np.all(got["lod"] == 0.0) and np.isnan(got["coef_mean"]).all() and got["n_used"][0] == 16
    assert got["ll0"][0, 0] == 0.0
    ctx.close()


# ------------------------------------------------------------------------------------- 6. permutations and refusals
def test_identity_permutation_and_refusals(capi):
    case = R.CASES[1]
    n, K, n_var, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    origin, pheno, cov, _, _ = R.make_case(*case)
    use = np.ones(n, bool)
    use[4] = False
    ctx, cs = map_context(capi)
    C, M = len(cs) - 1, int(cs[-1])
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3, use=use)[0], ident])
    got = ctx.qtl_scan_var(origin, pheno, cov=cov, n_var=n_var, imprint=True, use=use, perm=perm)
    observed = np.stack([got["lod"][:, cs[c]:cs[c + 1]].max(axis=1) for c in range(C)], axis=1)          # [T][C][3]
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed) and np.all(observed[..., 0] > 0.0)
    # refused, with the outputs left alone
    twice = ident.copy()
    twice[3] = 2
    bad_cov = cov.copy()
    bad_cov[7, 0] = np.inf
    bad_y = pheno.copy()
    bad_y[6, 0] = np.nan
    base = dict(pheno=pheno, cov=cov, n_var=1, perm=ident[None], max_iter=10, tol=1e-6)
    refusals = [dict(max_iter=0), dict(max_iter=1001), dict(tol=np.nan), dict(tol=np.inf), dict(tol=-np.inf), dict(cov=np.zeros((n, 9))),
                dict(n_var=-1), dict(n_var=3), dict(n_var=4), dict(cov=None, n_var=1), dict(perm=twice[None]), dict(cov=bad_cov),
                dict(pheno=bad_y)]
    poisoned = lambda: dict(lod=np.full((T, M, 3), 77.0), coef_mean=np.full((T, M, 3), 77.0), coef_var=np.full((T, M, 3), 77.0),
                            iters=np.full((T, M, 3), 77, np.int32), status=np.full((T, M, 3), 77, np.int32),
                            rank=np.full(M, 77, np.int32), ll0=np.full((T, C), 77.0), n_used=np.full(C, 77, np.int32),
                            perm_max=np.full((1, T, C, 3), 77.0))
    import torch
    d_o = torch.from_numpy(origin).cuda()
    for change in refusals:
        kw = dict(base, **change)
        out = poisoned()
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_var(origin, kw["pheno"], cov=kw["cov"], n_var=kw["n_var"], imprint=True, use=use, perm=kw["perm"],
                             max_iter=kw["max_iter"], tol=kw["tol"], out=out)
        assert all(np.all(v == 77) for v in out.values()), change
        d = device_outputs(capi, out)
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_var_device(n, d_o.data_ptr(), kw["pheno"], cov=kw["cov"], n_var=kw["n_var"], imprint=True, use=use,
                                    perm=kw["perm"], max_iter=kw["max_iter"], tol=kw["tol"],
                                    out={k: v.data_ptr() for k, v in d.items()}, flags=capi.OUT_DEVICE)
        ctx.sync()
        assert all(bool((x == 77).all()) for x in d.values()), change
    # the same value at an individual that is not used is accepted
    y = pheno.copy()
    y[4, 0] = np.nan
    same_bits(got, ctx.qtl_scan_var(origin, y, cov=cov, n_var=n_var, imprint=True, use=use, perm=perm))
    ctx.close()


# ------------------------------------------------------------------------------------- 7. column tiles across T
def test_column_tiles_across_the_permuted_boundary(capi):
    """T = 2, P = 5: 12 columns, the first two observed.  Caps of 3 and 5 put observed and permuted columns into one launch
    (columns 0 .. 2, resp. 0 .. 4), a cap of 12 all of them; the bits are those of the default tiling."""
    case = R.CASES[9]
    n, K, n_var, imprint, additive, seed, T, P, mask, skipped, max_iter = case
    assert (T, P) == (2, 5)
    origin, pheno, cov, use, perm = R.make_case(*case)
    ctx, _ = map_context(capi)
    kw = dict(cov=cov, n_var=n_var, imprint=imprint, use=use, perm=perm, additive=additive, max_iter=max_iter, tol=-1.0)
    got = ctx.qtl_scan_var(origin, pheno, **kw)
    for cap in (3, 5, 12):
        ctx.set_qtlvar_columns(cap)
        same_bits(got, ctx.qtl_scan_var(origin, pheno, **kw))
    ctx.set_qtlvar_columns(0)
    same_bits(got, ctx.qtl_scan_var(origin, pheno, **kw))
    ctx.close()


# ------------------------------------------------------------------------------------- 8. edges of the lane walk and of n_c
def test_a_round_with_nobody_in_it(capi):
    """n = 130 with individuals 64 .. 127 unused: every lane's second step is masked, the third round holds two individuals"""
    p = R.EMPTY_ROUND
    origin, pheno, z, use = R.empty_round_case()
    ref = R.empty_round_reference()
    cc = R.compared_cells(ref, CS)
    print("empty round: %.3f of the cells compared, %d near" % (cc.mean(), ref["near"].sum()))
    assert ref["near"].mean() <= 0.01 and np.all(ref["n_used"] == 66)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_var(origin, pheno, cov=z, n_var=1, use=use, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_var(got, ref, CS, "n 130, 64 .. 127 unused")
    assert np.all(got["n_used"] == 66)
    same_bits(got, ctx.qtl_scan_var(origin, pheno, cov=z, n_var=1, use=use, max_iter=p["max_iter"], tol=p["tol"]))
    ctx.close()


@pytest.mark.parametrize("n_c", (11, 10))
def test_scan_threshold(capi, n_c):
    """(a, i) with K = 3 and n_var = 1 needs 6 + 4 + 1 individuals: a chromosome with 11 is scanned, one with 10 is not"""
    p = R.THRESHOLD
    origin, y, z = R.threshold_case(n_c)
    c = p["chrom"]
    on = slice(CS[c], CS[c + 1])
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_var(origin, y, cov=z, n_var=p["n_var"], imprint=True, additive=True, max_iter=50, tol=1e-7)
    ctx.close()
    assert got["n_used"][c] == n_c and np.all(np.delete(got["n_used"], c) == p["n"])
    assert np.isfinite(got["lod"]).all() and np.all(got["lod"] >= 0) and np.isin(got["status"], (0, 1, 2)).all()
    assert np.all(np.delete(got["rank"], np.arange(CS[c], CS[c + 1])) > 0)
    if n_c >= p["need"]:
        assert np.all(got["rank"][on] > 0) and got["ll0"][0, c] != 0.0 and np.all(got["iters"][0, on] > 0)
    else:
        assert np.all(got["rank"][on] == 0) and got["ll0"][0, c] == 0.0
        assert np.all(got["lod"][:, on] == 0.0) and np.all(got["iters"][:, on] == 0) and np.all(got["status"][:, on] == 0)
        assert np.isnan(got["coef_mean"][:, on]).all() and np.isnan(got["coef_var"][:, on]).all()


# ------------------------------------------------------------------------------------- 9. end to end
def test_end_to_end_on_a_swept_cross(capi):
    """qtl.scan_var on an F2 the product sweeps itself: within 1e-9 of the yardstick on the product's own origin_rows at the
    cells that pass the conditions; thresholds_var and peaks_var read it; var_covariates moves a covariate to the front; the
    scan on the rows a sweep_qtl left in the context (origin NULL) leaves them valid; CNF2_ERR_STATE for another n"""
    ped = synth.make_f2(80, 17, 2, seed=7)
    n, M = len(ped.dous), ped.n_markers
    cs = np.asarray(ped.chromstarts)
    cov = np.stack([synth.uniform(21, np.arange(n)), synth.uniform(22, np.arange(n))], axis=1)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = qtl.origin_rows(ctx)
    o = rows.cpu().numpy()
    a = o[:, :, 3] - o[:, :, 0]
    e = R.gauss((n, 2), 8)
    pheno = np.stack([0.8 * a[:, 4] + e[:, 0], np.exp(0.5 * 0.9 * a[:, M - 3]) * e[:, 1] + cov[:, 1]], axis=1)
    pheno[3, 1] = np.nan                                   # the second trait has its own pattern of missing values
    kw = dict(cov=cov, var_covariates=(1,), permutations=3, seed=4, max_iter=50, tol=1e-7)
    got = qtl.scan_var(ctx, pheno, rows=rows, **kw)
    assert got["coef_names"] == ("a", "d") and set(got) >= set(OUT_KEYS) | {"lod_joint", "lod_mean", "lod_variance"}
    moved = cov[:, [1, 0]]
    for t in range(2):
        use = np.isfinite(pheno[:, t])
        yk = np.where(use, pheno[:, t], 0.0)[:, None]
        perm = qtl.permutations(n, 3, 4, use=use)
        ref = R.reference_scan_var(o, cs, yk, use, moved, 1, perm=perm, max_iter=50, tol=1e-7)
        cc = R.compared_cells(ref, cs, share=0, strict=False)
        print("trait %d: %.0f %% of the cells pass the conditions (smallest pivot %.3g, largest |eta| %.3g)" %
              (t, 100 * cc.mean(), ref["minpivot"].min(), ref["maxeta"].max()))
        one = {k: got[k][t:t + 1] for k in ("lod", "coef_mean", "coef_var", "iters", "status", "ll0")}
        one.update(rank=got["rank"][t], n_used=got["n_used"][t], perm_max=None)
        R.compare_var(one, dict(ref, perm_max=ref["perm_max"][:0]), cs, "qtl.scan_var trait %d" % t, share=0.9, strict=False)
        assert got["n_used"][t, 0] == n - t
    thr = qtl.thresholds_var(got["perm_max"])
    assert thr["joint"]["genome"].shape == (2, 2) and set(thr) == {"alpha", "joint", "mean", "variance"}
    pk = qtl.peaks_var(got, ped.pos, cs, 0.0)
    assert set(pk) == set(qtl.VAR_KEYS) and all(len(v) > 0 for v in pk.values())
    assert pk["variance"] == qtl.peaks(got["lod_variance"], ped.pos, cs, 0.0)
    # on the rows a sweep_qtl left in the context
    y0 = pheno[:, :1]
    single = ctx.sweep_qtl(y0, cov=cov)
    before = ctx.qtl_scan_device(n, None, y0, cov=cov)
    kept = ctx.qtl_scan_var_device(n, None, y0, cov=moved, n_var=1, max_iter=50, tol=1e-7)
    assert kept["lod"][0].tobytes() == got["lod"][0].tobytes() and kept["iters"][0].tobytes() == got["iters"][0].tobytes()
    after = ctx.qtl_scan_device(n, None, y0, cov=cov)
    assert before["lod"].tobytes() == single["lod"].tobytes() == after["lod"].tobytes()
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_var_device(n - 1, None, y0[:-1], cov=cov[:-1])
    ctx.close()


def test_cli_qtlvar(capi, tmp_path):
    """cnF2freq --qtlvar on an F2 of 30 on two chromosomes written to files: two traits of which one has missing values of its
    own, two covariates of which the second is a variance covariate, 5 permutations.  Every figure of the file is
    qtl.scan_var's on host.Run.from_files of the same files, to the printed digits; --output is the same bytes with and
    without --qtlvar."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    from test_gpu_qtl2 import write_f2_files
    ped = synth.make_f2(30, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n, M, cs = 30, ped.n_markers, np.asarray(ped.chromstarts)
    g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
    age = np.round(synth.uniform(5, np.arange(n)) * 10.0, 3)
    w = np.round(noise(n, 1, 3)[:, 0], 4)
    e = R.gauss((n, 2), 2)
    y = np.round(np.stack([0.8 * g(4) + e[:, 0], np.exp(0.4 * g(12) + 0.5 * w) * e[:, 1]], axis=1), 4)
    y[3, 1] = np.nan
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id b age w h"] + ["%s %s %s %s %s" % (names[i], cell(y[i, 0]), cell(age[i]), cell(w[i]), cell(y[i, 1])) for i in range(n)]
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1"]
    qopts = ["--phenofile", str(ph), "--qtl-covariates", "age,w", "--qtl-permutations", "5", "--qtl-seed", "4", "--qtl-imprint",
             "--qtl-var-covariates", "w", "--qtl-var-iterations", "30", "--qtl-var-tol", "1e-6"]
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    p = lambda name: str(tmp_path / name)
    run("--output", p("a.out"), "--qtlvar", p("qv.txt"), *qopts)
    run("--output", p("b.out"))
    read = lambda name: open(p(name), "rb").read()
    assert read("a.out") == read("b.out")
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    want = qtl.scan_var(ctx, y, cov=np.stack([age, w], axis=1), var_covariates=(1,), imprint=True, permutations=5, seed=4, max_iter=30,
                        tol=1e-6)
    ctx.close()
    r.close()
    thr = qtl.thresholds_var(want["perm_max"])
    tables = read("qv.txt").decode().strip("\n").split("\n\n")
    assert len(tables) == 2
    worst = 0.0
    for t, tab in enumerate(tables):
        lines = [ln.split("\t") for ln in tab.split("\n")]
        assert lines[0] == ["trait", ["b", "h"][t]] and len(lines) == 1 + M + 3
        for m, x in enumerate(lines[1:1 + M]):
            c = int(np.searchsorted(cs, m, side="right") - 1)
            assert len(x) == 4 + 9 + 6 and int(x[0]) == c + 1 and int(x[2]) == want["n_used"][t, c] == n - t
            assert int(x[3]) == want["rank"][t, m]
            assert [int(v) for v in x[7:10]] == list(want["iters"][t, m]) and [int(v) for v in x[10:13]] == list(want["status"][t, m])
            figures = [(x[1], ped.pos[m])] + list(zip(x[4:7], want["lod"][t, m]))
            for text, v in zip(x[13:], np.concatenate([want["coef_mean"][t, m], want["coef_var"][t, m]])):
                assert (text == "-") == bool(np.isnan(v))
                if text != "-":
                    figures.append((text, v))
            for text, value in figures:
                assert len(text.split(".")[1]) == 5
                worst = max(worst, abs(float(text) - value) / max(1.0, abs(value)))
        for k, key in enumerate(qtl.VAR_KEYS):
            x = lines[1 + M + k]
            assert x[:2] == ["threshold", key]
            for a in range(2):
                worst = max(worst, abs(float(x[2 + a]) - thr[key]["genome"][a, t]))
    print("file against qtl.scan_var: %.3g; largest LOD %.2f" % (worst, want["lod"].max()))
    assert worst <= 0.51e-5 and want["lod"].max() > 0.5
