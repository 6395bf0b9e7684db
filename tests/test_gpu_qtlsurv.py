"""GPU suite: the survival-trait single-locus scan (cnf2_qtl_scan_surv, cnf2_set_qtlsurv_columns, cnf2_set_qtlsurv_blocks,
Context.qtl_scan_surv, qtl.scan_surv, cnF2freq --qtlsurv).  Cox's regression of every marker and (time, status) column by
Newton's method on Breslow's partial likelihood, checked against the direct risk-set definition in numpy
(tests/qtlsurv_reference.py): a fixed number of iterations and the stopping rule at the shapes where the rounds of 64 positions
and the wave scans can go wrong, hand-made ties and censoring, the invariance to a monotone change of the times, a planted
locus where the model must differ from the linear scan of the times and the logistic scan of the status, the monotone
likelihood, bit-equality, refusals, a swept cross and the command line.

The kernels are compiled once per K + 1.  Which case runs which instance and design:

    K  case                         design      |  K  case                          design
    0  CASES[2] n 64                (a, d)      |  5  CASES[7] n 67, skipped, ties  (a, d, i)
    1  CASES[8] n 41, T 2           (a, i)      |  6  CASES[4] n 127, mask          (a)
    2  CASES[0] n 41, T 2           (a, d)      |  7  CASES[5] n 129, ties          (a, i)
    3  CASES[1] n 63, ties          (a, i)      |  8  CASES[6] n 130, T 2, P 5      (a, d, i)
    4  CASES[3] n 65, skipped, ties (a, d)      |

The hand-made cases (n 130) and the planted locus (n 60) run K = 1 with (a, d)."""
import numpy as np
import pytest

import qtlsurv_reference as R
from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, noise

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod", "coef", "iters", "status", "rank", "ll0", "n_events", "n_used", "perm_max")
CS = chromstarts_of(CHROM_LENS)
LN10 = np.log(10.0)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens=CHROM_LENS):
    """a context that holds a map only: what cnf2_qtl_scan_surv needs"""
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


# ------------------------------------------------------------------------------------- fixed iterations, the same bits
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fixed_iterations(capi, case):
    """every output after exactly max_iter passes against the yardstick at all 84 markers; rank as cnf2_qtl_scanx's; the same
    bits with column tiles of 1 and 4 (across the observed/permuted boundary where T = 2, P = 5), with block caps of 1 and 7,
    on a second call, from device rows, into device outputs and with another batching of the sweeps"""
    import torch
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter, grid = case
    origin, time, status, cov, use, perm = R.make_case(*case)
    ref = R.case_reference(case)
    # the conditions of the comparison, on the references alone, before anything runs
    R.assert_conditions([R.case_reference(c) for c in R.CASES])
    R.compared_cells(ref, CS)
    if grid:
        t0 = time[np.isfinite(time[:, 0]), 0]
        assert len(np.unique(t0)) < len(t0), "the case has tied times"
    ctx, _ = map_context(capi)
    kw = dict(cov=cov, imprint=imprint, use=use, perm=perm, additive=additive, max_iter=max_iter, tol=-1.0)
    got = ctx.qtl_scan_surv(origin, time, status, **kw)
    assert got["coef"].shape[2] == len(R.effects(additive, imprint))
    R.compare_surv(got, ref, CS, R.case_id(case))
    fitted = got["rank"] > 0
    assert np.all(got["iters"][:, fitted] == max_iter) and np.all(got["status"][:, fitted] == 1)
    x = ctx.qtl_scanx(origin, np.nan_to_num(time), cov=cov, imprint=imprint, use=use, additive=additive)
    assert np.array_equal(got["rank"], x["rank"][:, 1 if imprint else 0]) and np.array_equal(got["n_used"], x["n_used"])
    if skipped:
        assert got["n_used"][3] == n - 2 and got["n_used"][0] == n
    if mask:
        assert np.all(got["n_used"] == n - 2)
    same_bits(got, ctx.qtl_scan_surv(origin, time, status, **kw))
    for cap in (1, 4):
        ctx.set_qtlsurv_columns(cap)
        same_bits(got, ctx.qtl_scan_surv(origin, time, status, **kw))
    ctx.set_qtlsurv_columns(0)
    for cap in (1, 7):
        ctx.set_qtlsurv_blocks(cap)
        same_bits(got, ctx.qtl_scan_surv(origin, time, status, **kw))
    ctx.set_qtlsurv_blocks(0)
    ctx.set_batch_jobs(5)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan_surv_device(n, d_o.data_ptr(), time, status, **kw))
    ctx.set_batch_jobs(0)
    d = device_outputs(capi, got)
    ctx.qtl_scan_surv_device(n, d_o.data_ptr(), time, status, out={k: None if v is None else v.data_ptr() for k, v in d.items()},
                             flags=capi.OUT_DEVICE, **kw)
    ctx.sync()
    same_bits(got, {k: None if v is None else v.cpu().numpy() for k, v in d.items()})
    ctx.close()


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_stopping_rule(capi, case):
    """the same cases to tol 1e-7: the yardstick agrees with its longdouble anchor, then every output against it"""
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter, grid = case
    ref = R.case_reference(case, **R.STOP)
    R.assert_anchor(ref, R.case_id(case))
    R.assert_conditions([R.case_reference(c, **R.STOP) for c in R.CASES])
    R.compared_cells(ref, CS)
    origin, time, status, cov, use, perm = R.make_case(*case)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_surv(origin, time, status, cov=cov, imprint=imprint, use=use, perm=perm, additive=additive, **R.STOP)
    R.compare_surv(got, ref, CS, R.case_id(case) + " to tol 1e-7")
    assert np.all(got["status"] == 0) and got["iters"].max() <= 10
    ctx.close()


# ------------------------------------------------------------------------------------- ties and censoring, hand-made
@pytest.mark.parametrize("which", R.HAND_CASES)
def test_hand_made_ties_and_censoring(capi, which):
    origin, time, status, z, use = R.hand_case(which)
    ref = R.hand_reference(which)
    n = R.HAND["n"]
    # what the case is about, on its data and the reference alone
    t, d = time[:, 0], status[:, 0]
    if which == "span":
        assert np.all(t[60:71] == t[60]) and (t == t[60]).sum() == 11
    if which == "censored":
        assert np.all(d[20:26] == 0) and (t == t[20]).sum() == 6
    if which == "masked":
        assert ref["n_used"][3] == n - 2 and ref["n_used"][0] == n - 1 and ref["n_events"][0, 3] == ref["n_events"][0, 0] - 1
    if which == "first":
        assert d[np.argmax(t)] == 1
    if which == "last":
        assert d[np.argmin(t)] == 1 and d[np.argmax(t)] == 0
    if which == "single":
        assert np.all(ref["n_events"] == 1)
    if which == "ninety":
        assert d.mean() <= 0.12
    if which == "empty":
        assert np.all(ref["n_used"] == 66)
    share = 0.0 if which in ("single", "none") else 0.9
    R.compared_cells(ref, CS, share=share)
    assert ref["near"].mean() <= 0.02
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_surv(origin, time, status, cov=z, use=use, max_iter=R.HAND["max_iter"], tol=R.HAND["tol"])
    assert np.isfinite(got["lod"]).all() and np.isfinite(got["ll0"]).all() and np.isin(got["status"], (0, 1, 2)).all()
    if which == "none":
        assert np.all(got["lod"] == 0.0) and np.all(got["ll0"] == 0.0) and np.all(got["n_events"] == 0)
        assert np.all(got["iters"] == 0) and np.all(got["status"] == 0) and np.isnan(got["coef"]).all()
        assert np.array_equal(got["rank"], ref["rank"]) and np.all(got["rank"] > 0)
    else:
        R.compare_surv(got, ref, CS, "hand-made: " + which, share=share)
    ctx.close()


# ------------------------------------------------------------------------------------- time enters by rank only
def test_time_enters_by_rank_only(capi):
    case = R.CASES[3]                         # n 65, K 4, skipped individuals, tied times, one permutation
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter, grid = case
    origin, time, status, cov, use, perm = R.make_case(*case)
    ctx, _ = map_context(capi)
    kw = dict(cov=cov, imprint=imprint, use=use, perm=perm, additive=additive, **R.STOP)
    got = ctx.qtl_scan_surv(origin, time, status, **kw)
    for f in (np.exp, lambda t: 3.0 * t + 7.0):
        moved = f(time)
        assert len(np.unique(moved)) == len(np.unique(time)), "the change keeps distinct times distinct"
        same_bits(got, ctx.qtl_scan_surv(origin, moved, status, **kw))
    assert got["lod"].max() > 0.5
    ctx.close()


# ------------------------------------------------------------------------------------- not a linear scan in disguise
def test_planted_locus_is_not_a_linear_or_a_binary_scan(capi):
    p = R.PLANTED
    ref, hk, bn = R.planted_references()
    R.assert_anchor(ref, "planted")           # on the yardsticks alone, before anything of the product runs
    R.compared_cells(ref, CS)
    assert ref["near"].mean() <= 0.01
    R.assert_planted(ref, hk, bn)
    origin, time, status, z = R.planted_case()
    assert abs(1.0 - status.mean() - p["censored"]) <= 0.1
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_surv(origin, time, status, cov=z, max_iter=p["max_iter"], tol=p["tol"])
    R.compare_surv(got, ref, CS, "planted locus")
    assert got["lod"][0].argmax() == p["marker"] and np.all(got["status"] == 0)
    lin = ctx.qtl_scan(origin, time, cov=z)["lod"][0]
    logit = ctx.qtl_scan_binary(origin, status, cov=z, max_iter=50, tol=1e-7)["lod"][0]
    assert np.abs(lin - hk["lod"][0, 0]).max() <= ATOL
    assert np.abs(got["lod"][0] - lin).max() > 0.2 and np.abs(got["lod"][0] - logit).max() > 0.2
    ctx.close()


# ------------------------------------------------------------------------------------- other properties
def test_monotone_over_iterations(capi):
    ref = R.monotone_reference()
    steps = ref["trace"][0][:, list(R.MONOTONE)]
    assert np.all(np.diff(steps, axis=1) >= -1e-12)
    origin, time, status, z = R.planted_case()
    ctx, _ = map_context(capi)
    lods = np.stack([ctx.qtl_scan_surv(origin, time, status, cov=z, max_iter=k, tol=-1.0)["lod"][0] for k in R.MONOTONE], axis=1)
    ctx.close()
    assert np.all(np.diff(lods, axis=1) >= -1e-12)
    assert np.abs(lods - steps).max() <= ATOL


def test_monotone_likelihood_ends_finite(capi):
    """a marker whose effect orders the times perfectly: the partial likelihood has no maximum; the fit ends by max_iter or by
    a breakdown with finite outputs (tol is negative: the gains shrink geometrically, and a positive tol would stop the fit by
    the first rule), and its LOD reaches at least what five iterations reach"""
    marker = 8
    origin, time, status = R.perfect_order_case(marker=marker)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_surv(origin, time, status, additive=True, max_iter=200, tol=-1.0)
    five = ctx.qtl_scan_surv(origin, time, status, additive=True, max_iter=5, tol=-1.0)
    ctx.close()
    assert got["rank"][marker] == 1 and got["status"][0, marker] in (1, 2)
    assert np.isfinite(got["lod"]).all() and np.isfinite(got["ll0"]).all() and np.all(got["lod"] >= 0)
    assert np.isfinite(got["coef"][0, got["rank"] > 0]).all() and np.isin(got["status"], (0, 1, 2)).all()
    assert got["lod"][0, marker] >= five["lod"][0, marker] > 1.0 and got["coef"][0, marker, 0] > 5.0
    bound = np.repeat(-got["ll0"] / LN10 + ATOL, np.diff(CS), axis=1)
    assert np.all(got["lod"] <= bound)


@pytest.mark.parametrize("n_c", (7, 6))
def test_scan_threshold(capi, n_c):
    """(a, i) with K = 3: W = 6, so a chromosome with 7 individuals is scanned and one with 6 is not"""
    p = R.THRESHOLD
    origin, time, status, z = R.threshold_case(n_c)
    ref = R.reference_scan_surv(origin, CS, time, status, None, z, imprint=True, additive=True, max_iter=50, tol=1e-7)
    c = p["chrom"]
    assert ref["usable"][c] == (n_c == 7) and ref["usable"].sum() == 5 + (n_c == 7)
    ctx, _ = map_context(capi)
    got = ctx.qtl_scan_surv(origin, time, status, cov=z, imprint=True, additive=True, max_iter=50, tol=1e-7)
    ctx.close()
    on = slice(CS[c], CS[c + 1])
    assert got["n_used"][c] == n_c and np.all(np.delete(got["n_used"], c) == p["n"])
    assert got["n_events"][0, c] == (5 if n_c == 7 else 4) and np.isfinite(got["lod"]).all() and np.isin(got["status"], (0, 1, 2)).all()
    assert np.all(np.delete(got["rank"], np.arange(CS[c], CS[c + 1])) > 0)
    if n_c == 7:
        assert np.all(got["rank"][on] > 0)
    else:
        assert np.all(got["rank"][on] == 0) and got["ll0"][0, c] == 0.0 and np.isnan(got["coef"][0, on]).all()
        assert np.all(got["lod"][:, on] == 0.0) and np.all(got["iters"][:, on] == 0) and np.all(got["status"][:, on] == 0)
    fine = R.compared_cells(dict(ref, maxeta=np.zeros_like(ref["maxeta"])), CS, share=0.9, strict=False)[0]
    assert np.array_equal(got["rank"][fine], ref["rank"][fine])


def test_a_dropped_effect(capi):
    """(a, i) on the degenerate rows: i is dropped at the homozygous and the symmetric marker (NaN), and lod and a are the
    additive fit's without imprinting, to the bit"""
    origin, at = R.degenerate_rows()
    n = origin.shape[0]
    z = noise(n, 1, 12)
    time, status = R.draw_times(np.zeros((n, 1)), 11)
    ctx, _ = map_context(capi)
    f = ctx.qtl_scan_surv(origin, time, status, cov=z, additive=True, imprint=True)
    g = ctx.qtl_scan_surv(origin, time, status, cov=z, additive=True)
    ctx.close()
    for m in (at["homozygous"], at["symmetric"]):
        assert f["rank"][m] == 1 and np.isnan(f["coef"][0, m, 1]) and f["lod"][0, m] == g["lod"][0, m] > 0.0
        assert f["coef"][0, m, 0] == g["coef"][0, m, 0] and f["iters"][0, m] == g["iters"][0, m]
    assert f["rank"][at["flat"]] == 0 and f["lod"][0, at["flat"]] == 0.0 and np.isnan(f["coef"][0, at["flat"]]).all()
    assert f["rank"][at["zeros"]] == 2 and np.isfinite(f["coef"][0, at["zeros"]]).all()


# ------------------------------------------------------------------------------------- permutations and refusals
def test_identity_permutation_and_refusals(capi):
    case = R.CASES[0]
    n, K, imprint, additive, seed, T, P, mask, skipped, max_iter, grid = case
    origin, time, status, cov, _, _ = R.make_case(*case)
    use = np.ones(n, bool)
    use[4] = False
    ctx, cs = map_context(capi)
    C, M = len(cs) - 1, int(cs[-1])
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3, use=use)[0], ident])
    got = ctx.qtl_scan_surv(origin, time, status, cov=cov, imprint=True, use=use, perm=perm)
    observed = np.stack([got["lod"][:, cs[c]:cs[c + 1]].max(axis=1) for c in range(C)], axis=1)          # [T][C]
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed) and np.all(observed > 0.0)
    # refused, with the outputs left alone
    twice = ident.copy()
    twice[3] = 2
    bad_cov = cov.copy()
    bad_cov[7, 0] = np.inf

    def with_value(a, v):
        b = a.copy()
        b[6, 1] = v
        return b
    base = dict(time=time, status=status, cov=cov, perm=ident[None], max_iter=10, tol=1e-6)
    refusals = [dict(max_iter=0), dict(max_iter=1001), dict(tol=np.nan), dict(tol=np.inf), dict(tol=-np.inf), dict(cov=np.zeros((n, 9))),
                dict(perm=twice[None]), dict(cov=bad_cov), dict(status=with_value(status, 0.5)), dict(status=with_value(status, 2.0)),
                dict(status=with_value(status, np.nan)), dict(time=with_value(time, np.nan)), dict(time=with_value(time, np.inf))]
    poisoned = lambda: dict(lod=np.full((T, M), 77.0), coef=np.full((T, M, 3), 77.0), iters=np.full((T, M), 77, np.int32),
                            status=np.full((T, M), 77, np.int32), rank=np.full(M, 77, np.int32), ll0=np.full((T, C), 77.0),
                            n_events=np.full((T, C), 77, np.int32), n_used=np.full(C, 77, np.int32), perm_max=np.full((1, T, C), 77.0))
    import torch
    d_o = torch.from_numpy(origin).cuda()
    for change in refusals:
        kw = dict(base, **change)
        out = poisoned()
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_surv(origin, kw["time"], kw["status"], cov=kw["cov"], imprint=True, use=use, perm=kw["perm"],
                              max_iter=kw["max_iter"], tol=kw["tol"], out=out)
        assert all(np.all(v == 77) for v in out.values()), change
        d = device_outputs(capi, out)
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_surv_device(n, d_o.data_ptr(), kw["time"], kw["status"], cov=kw["cov"], imprint=True, use=use, perm=kw["perm"],
                                     max_iter=kw["max_iter"], tol=kw["tol"], out={k: v.data_ptr() for k, v in d.items()},
                                     flags=capi.OUT_DEVICE)
        ctx.sync()
        assert all(bool((x == 77).all()) for x in d.values()), change
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
        ctx.set_qtlsurv_blocks(-1)
    # the same values at an individual that is not used are accepted
    for v in (0.5, np.nan):
        s = status.copy()
        s[4, 1] = v
        t = time.copy()
        t[4, 0] = np.nan
        same_bits(got, ctx.qtl_scan_surv(origin, t, s, cov=cov, imprint=True, use=use, perm=perm))
    ctx.close()


# ------------------------------------------------------------------------------------- through the stack
def test_end_to_end_on_a_swept_cross(capi):
    """qtl.scan_surv on an F2 the product sweeps itself: within 1e-9 of the yardstick on the product's own origin_rows at the
    cells that pass the conditions, permutations included; thresholds and peaks read it; CNF2_ERR_STATE for another n"""
    ped = synth.make_f2(24, 17, 2, seed=7)
    n, M = len(ped.dous), ped.n_markers
    cs = np.asarray(ped.chromstarts)
    cov = synth.uniform(21, np.arange(n)).reshape(n, 1)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = qtl.origin_rows(ctx)
    o = rows.cpu().numpy()
    a = o[:, :, 3] - o[:, :, 0]
    time, status = R.draw_times(np.stack([0.6 * a[:, 4], 0.6 * a[:, M - 3]], axis=1), 8)
    time[3, 1] = np.nan                                    # the second trait has its own pattern of missing values
    kw = dict(cov=cov, permutations=3, seed=4, max_iter=50, tol=1e-7)
    got = qtl.scan_surv(ctx, time, status, rows=rows, **kw)
    assert got["coef_names"] == ("a", "d") and set(got) >= set(OUT_KEYS)
    for t in range(2):
        use = np.isfinite(time[:, t])
        perm = qtl.permutations(n, 3, 4, use=use)
        ref = R.reference_scan_surv(o, cs, np.where(use, time[:, t], 0.0)[:, None], status[:, t:t + 1], use, cov, perm=perm, max_iter=50,
                                    tol=1e-7)
        cc = R.compared_cells(ref, cs, share=0.9, strict=False)
        print("trait %d: %.0f %% of the cells pass the conditions" % (t, 100 * cc.mean()))
        one = dict(lod=got["lod"][t:t + 1], coef=got["coef"][t:t + 1], iters=got["iters"][t:t + 1], status=got["status"][t:t + 1],
                   rank=got["rank"][t], n_used=got["n_used"][t], ll0=got["ll0"][t:t + 1], n_events=got["n_events"][t:t + 1],
                   perm_max=got["perm_max"][:, t:t + 1])
        R.compare_surv(one, ref, cs, "qtl.scan_surv trait %d" % t, share=0.9, strict=False)
        assert got["n_used"][t, 0] == n - t
    thr = qtl.thresholds(got["perm_max"])
    assert thr["genome"].shape == (2, 2)
    qtl.peaks(got["lod"], ped.pos, cs, thr["genome"][0])
    with pytest.raises(ValueError):
        qtl.scan_surv(ctx, time, np.where(status == 1.0, 2.0, status), rows=rows)
    # on the rows a sweep_qtl left in the context
    single = ctx.sweep_qtl(time[:, :1], cov=cov)
    kept = ctx.qtl_scan_surv_device(n, None, time[:, :1], status[:, :1], cov=cov, max_iter=50, tol=1e-7)
    assert kept["lod"][0].tobytes() == got["lod"][0].tobytes() and kept["iters"][0].tobytes() == got["iters"][0].tobytes()
    assert ctx.qtl_scan_device(n, None, time[:, :1], cov=cov)["lod"].tobytes() == single["lod"].tobytes()
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_surv_device(n - 1, None, time[:-1, :1], status[:-1, :1], cov=cov[:-1])
    ctx.close()


def test_cli_qtlsurv(capi, tmp_path):
    """cnF2freq --qtlsurv on an F2 of 14 on two chromosomes written to files: a time with a missing value, its status, a
    covariate, 5 permutations.  Every figure of the file is qtl.scan_surv's on host.Run.from_files of the same files, to the
    printed digits; --output is the same bytes with and without --qtlsurv."""
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
    time, status = R.draw_times(0.8 * g(4)[:, None], 2)
    time = np.round(time[:, 0], 4)
    status = status[:, 0]
    time[3] = np.nan
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id days age dead"] + ["%s %s %s %d" % (names[i], cell(time[i]), cell(age[i]), int(status[i])) for i in range(n)]
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1"]
    opts = ["--phenofile", str(ph), "--qtl-covariates", "age", "--qtl-permutations", "5", "--qtl-seed", "4", "--qtl-surv-time", "days",
            "--qtl-surv-status", "dead", "--qtl-surv-iterations", "30", "--qtl-surv-tol", "1e-6"]
    p = lambda name: str(tmp_path / name)
    run = lambda *args: subprocess.run(base + list(args), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    run("--output", p("a.out"), "--qtlsurv", p("qs.txt"), *opts)
    run("--output", p("d.out"))
    read = lambda name: open(p(name), "rb").read()
    assert read("a.out") == read("d.out")
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    want = qtl.scan_surv(ctx, time, status, cov=age[:, None], permutations=5, seed=4, max_iter=30, tol=1e-6)
    ctx.close()
    r.close()
    thr = qtl.thresholds(want["perm_max"])
    lines = [ln.split("\t") for ln in read("qs.txt").decode().strip("\n").split("\n")]
    assert lines[0] == ["trait", "days", "dead"] and len(lines) == 1 + M + 1
    worst = 0.0
    for m, x in enumerate(lines[1:1 + M]):
        c = int(np.searchsorted(cs, m, side="right") - 1)
        assert len(x) == 7 + 2 and int(x[0]) == c + 1 and int(x[2]) == want["n_used"][0, c] == n - 1
        assert int(x[3]) == want["rank"][0, m] and int(x[5]) == want["iters"][0, m] and int(x[6]) == want["status"][0, m]
        figures = [(x[1], ped.pos[m]), (x[4], want["lod"][0, m])]
        for text, v in zip(x[7:], want["coef"][0, m]):
            assert (text == "-") == bool(np.isnan(v))
            if text != "-":
                figures.append((text, v))
        for text, value in figures:
            assert len(text.split(".")[1]) == 5
            worst = max(worst, abs(float(text) - value) / max(1.0, abs(value)))
    x = lines[1 + M]
    assert x[:2] == ["threshold", "lod"]
    for k in range(2):
        worst = max(worst, abs(float(x[2 + k]) - thr["genome"][k, 0]))
    print("file against qtl.scan_surv: %.3g; largest LOD %.2f" % (worst, want["lod"].max()))
    assert worst <= 0.51e-5 and want["lod"].max() > 0.5
