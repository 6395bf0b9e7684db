"""GPU suite: the cofactor scan (cnf2_qtl_scan_cof, cnf2_set_qtlcof_columns, Context.qtl_scan_cof, qtl.scan_cof /
cofactor_windows / fit_multi / forward_select, cnF2freq --qtlcof).  Composite interval mapping: every marker fitted together
with the cofactors, each left out inside its own window, checked against a per-marker least-squares fit in numpy
(tests/qtlcof_reference.py): on hand-made rows at the shapes of the issue, against the existing scan, as a multiple-QTL fit,
on degenerate designs, for its permutations and refusals, on planted effects, on the rows a sweep left in the context and
through the command line.

Measured on an MI355X (largest absolute error against the reference): hand-made rows 2.5e-13 on the LODs,
1.8e-14 on coef; against cnf2_qtl_scan 5.4e-15; the drop-one identity 1.3e-14; planted effects 7.2e-14; the swept F2 2.9e-14;
the command line's file 4.97e-6."""
import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, PIVOT_WELL, chromstarts_of, noise, soft_rows
from qtlx_reference import certain_rows
from qtlcof_reference import (CASES, PLANTED, WORST_PIVOT, case_id, case_reference, compare_cof, compared_markers, explicit_multi,
                              make_case, planted_case, planted_pos, planted_reference, reference_scan_cof, windows, worst_pivot)

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod", "lod_base", "coef", "rank", "rank_cof", "rss0", "n_used", "perm_max")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens):
    """a context that holds a map only: what cnf2_qtl_scan_cof needs"""
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
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def raw_call(capi, ctx, n, origin_ptr, pheno, cof, excl, cov, use, perm, outs, flags):
    """cnf2_qtl_scan_cof itself: outs maps OUT_KEYS to pointers (c_void_p); returns the status"""
    p = lambda a: None if a is None else a.ctypes.data_as(capi.C.c_void_p)
    ph, cv, us, pm = ctx._qtl_inputs(n, pheno, cov, use, perm)
    cf, lo, hi = (np.ascontiguousarray(v, np.int32) for v in (cof, excl[0], excl[1]))
    return ctx.L.cnf2_qtl_scan_cof(ctx.h, n, origin_ptr, ph.shape[1], p(ph), p(us), 0 if cv is None else cv.shape[1], p(cv), len(cf),
                                   p(cf), p(lo), p(hi), 0 if pm is None else len(pm), p(pm), *[outs[k] for k in OUT_KEYS], flags)


def device_outputs(like, fill=77):
    import torch
    dev = torch.device("cuda", 0)
    return {k: None if v is None else torch.full(v.shape, fill, dtype=torch.int32 if v.dtype == np.int32 else torch.float64, device=dev)
            for k, v in like.items()}


def pointers(capi, tensors):
    return {k: None if v is None else capi.C.c_void_p(v.data_ptr()) for k, v in tensors.items()}


# ------------------------------------------------------------------------------------- 1. values on hand-made rows
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scan_cof_on_hand_made_rows(capi, case):
    """every output against the least-squares fit at all 84 markers; the same bits on a second call, with column caps of 1 and
    16, from device rows, into device outputs and with another batching of the sweeps"""
    import torch
    n, K, cof, hw, additive, seed, T, P, mask, skipped = case
    origin, pheno, cov, use, perm, excl = make_case(*case)
    cs = chromstarts_of(CHROM_LENS)
    ref = case_reference(case)
    compared = compared_markers(ref, cs)         # the conditions of the comparison, on the reference, before anything runs
    assert compared.all()
    wp = worst_pivot(ref, cs)
    print("worst kept relative pivot %.4g" % wp)
    assert wp >= PIVOT_WELL and abs(wp - WORST_PIVOT[CASES.index(case)]) <= 0.006
    ctx, _ = map_context(capi, CHROM_LENS)
    kw = dict(excl=excl, cov=cov, use=use, perm=perm, additive=additive)
    got = ctx.qtl_scan_cof(origin, pheno, cof, **kw)
    compare_cof(got, ref, cs, case_id(case))
    if skipped:
        on3 = any(18 <= m < 34 for m in cof)
        assert got["n_used"][3] == n - 2 and got["n_used"][0] == (n - 2 if on3 else n)
    if mask:
        assert np.all(got["n_used"] == n - 2)
    same_bits(got, ctx.qtl_scan_cof(origin, pheno, cof, **kw))
    for cap in (1, 16):
        ctx.set_qtlcof_columns(cap)
        same_bits(got, ctx.qtl_scan_cof(origin, pheno, cof, **kw))
    ctx.set_qtlcof_columns(0)
    ctx.set_batch_jobs(5)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan_cof_device(n, d_o.data_ptr(), pheno, cof, **kw))
    ctx.set_batch_jobs(0)
    d = device_outputs(got)
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    rc = raw_call(capi, ctx, n, p(origin), pheno, cof, excl, cov, use, perm, pointers(capi, d),
                  capi.OUT_DEVICE | (capi.QTL_ADDITIVE if additive else 0))
    ctx.sync()
    assert rc == 0
    same_bits(got, {k: None if v is None else v.cpu().numpy() for k, v in d.items()})
    ctx.close()


# ------------------------------------------------------------------------------------- 2. without cofactors: the existing scan
def test_no_cofactors_is_qtl_scan(capi):
    """Q = 0: lod, coef, rank, rss0, n_used, perm_max are cnf2_qtl_scan's within 1e-9, the counts equal; lod_base is exactly 0"""
    ctx, cs = map_context(capi, CHROM_LENS)
    for case in (CASES[1], CASES[4]):
        n, K, _, hw, additive, seed, T, P, mask, skipped = case
        origin, pheno, cov, use, perm, _ = make_case(*case)
        one = ctx.qtl_scan(origin, pheno, cov=cov, use=use, perm=perm, additive=additive)
        got = ctx.qtl_scan_cof(origin, pheno, [], cov=cov, use=use, perm=perm, additive=additive)
        ne = got["coef"].shape[2]
        errs = dict(lod=np.abs(got["lod"] - one["lod"]).max(),
                    coef=(np.abs(got["coef"] - one["coef"][..., :ne]) / np.maximum(1.0, np.abs(one["coef"][..., :ne]))).max(),
                    rss0=np.abs(got["rss0"] - one["rss0"]).max(), perm_max=np.abs(got["perm_max"] - one["perm_max"]).max())
        print("n %d K %d additive %d against cnf2_qtl_scan: %s" % (n, K, additive, ", ".join("%s %.3g" % kv for kv in errs.items())))
        assert np.array_equal(got["rank"], one["rank"]) and np.array_equal(got["n_used"], one["n_used"])
        assert np.all(got["rank_cof"] == 0) and np.all(got["lod_base"] == 0.0)
        assert ne == (1 if additive else 2) and all(e <= ATOL for e in errs.values()), errs
    ctx.close()


# ------------------------------------------------------------------------------------- 3. cofactors as covariates
def test_whole_chromosome_ranges_against_covariates(capi):
    """case 8: on a chromosome without cofactors the conditional LOD is cnf2_qtl_scan's with the cofactor columns appended to
    the covariates"""
    case = CASES[7]
    n, K, cof, hw, additive, seed, T, P, mask, skipped = case
    origin, pheno, cov, use, perm, excl = make_case(*case)
    ctx, cs = map_context(capi, CHROM_LENS)
    assert additive and excl[0][0] == cs[2] and excl[1][0] == cs[3] - 1          # the range of cofactor 8 is all of chromosome 2
    got = ctx.qtl_scan_cof(origin, pheno, cof, excl=excl, cov=cov, use=use, additive=True)
    a = origin[:, :, 3] - origin[:, :, 0]
    one = ctx.qtl_scan(origin, pheno, cov=np.concatenate([cov, a[:, list(cof)]], axis=1), use=use, additive=True)
    ctx.close()
    free = np.concatenate([np.arange(cs[c], cs[c + 1]) for c in (0, 1, 3, 4)])
    err = np.abs(got["lod"][:, free] - one["lod"][:, free]).max()
    print("against cnf2_qtl_scan with the cofactors as covariates: lod %.3g over %d markers" % (err, len(free)))
    assert err <= ATOL and np.array_equal(got["rank"][free], one["rank"][free])
    # ... and inside a range that covers its chromosome the only cofactor left is the other one
    only = ctx_free_scan(capi, origin, pheno, cov, use, a[:, [cof[1]]])
    on2 = np.arange(cs[2], cs[3])
    err = np.abs(got["lod"][:, on2] - only["lod"][:, on2]).max()
    print("inside the range of cofactor %d: lod %.3g" % (cof[0], err))
    assert err <= ATOL


def ctx_free_scan(capi, origin, pheno, cov, use, extra):
    ctx, _ = map_context(capi, CHROM_LENS)
    out = ctx.qtl_scan(origin, pheno, cov=np.concatenate([cov, extra], axis=1), use=use, additive=True)
    ctx.close()
    return out


# ------------------------------------------------------------------------------------- 4. the multiple-QTL fit
def test_drop_one_identity(capi):
    """ranges of the cofactor alone: lod and coef at cof[q] are the explicit fit of the Q-locus model with and without locus
    q, and lod_base + lod is one and the same full-model LOD at every cofactor"""
    n, K, cof, _, additive, seed, T, P, mask, skipped = CASES[1]
    origin, pheno, cov, use, _, _ = make_case(n, K, cof, 0, additive, seed, T, 0, mask, skipped)
    cs = chromstarts_of(CHROM_LENS)
    full, drop, beta = explicit_multi(origin, cs, pheno, cof, use, cov, additive)
    ctx, _ = map_context(capi, CHROM_LENS)
    got = ctx.qtl_scan_cof(origin, pheno, cof, cov=cov, use=use)
    ctx.close()
    at = list(cof)
    err_d = np.abs(got["lod"][:, at] - drop).max()
    err_f = np.abs(got["lod_base"][:, at] + got["lod"][:, at] - full[:, None]).max()
    err_c = (np.abs(got["coef"][:, at] - beta) / np.maximum(1.0, np.abs(beta))).max()
    print("drop-one LOD %.3g, full-model LOD %.3g, effects %.3g; full LODs %s" % (err_d, err_f, err_c, full))
    assert err_d <= ATOL and err_f <= ATOL and err_c <= ATOL and np.all(full > 5.0)
    read = qtl.read_multi(got, cof[::-1], cs)
    assert np.abs(read["lod_full"] - full).max() <= ATOL and np.abs(read["drop_one"] - drop[:, ::-1]).max() <= ATOL
    assert np.all(read["n"] == n - 2)


# ------------------------------------------------------------------------------------- 5. degenerate designs
def degenerate_rows():
    """(origin, pheno, cof): 40 individuals on CHROM_LENS; marker 20 carries no information (0.25 each: a = 0, d constant),
    marker 31 repeats marker 30's rows, at marker 50 everybody is certain and homozygous (d = 0); trait 1 is constant"""
    origin, _ = soft_rows(40, CHROM_LENS, 8)
    origin[:, 20] = 0.25
    origin[:, 31] = origin[:, 30]
    origin[:, 50] = certain_rows(np.where(synth.uniform(3, np.arange(40)) < 0.5, 0, 3))
    a = origin[:, :, 3] - origin[:, :, 0]
    pheno = np.stack([0.7 * a[:, 5] + 0.5 * a[:, 70] + 0.4 * a[:, 30] + noise(40, 1, 9)[:, 0], np.full(40, 2.0)], axis=1)
    return origin, pheno, (5, 20, 30, 31, 70)


def test_degenerate_designs(capi):
    origin, pheno, cof = degenerate_rows()
    cs = chromstarts_of(CHROM_LENS)
    excl = windows(cof, 1, cs)
    ref = reference_scan_cof(origin, cs, pheno[:, :1], cof, excl[0], excl[1])       # (the constant trait is not one for least squares)
    M = origin.shape[1]
    active = np.array([[not excl[0][q] <= m <= excl[1][q] for q in range(5)] for m in range(M)])
    # on the reference first: the uninformative cofactor loses both columns, of the twins the second is dropped -- unless the
    # first is left out --, the homozygous marker keeps a alone
    want_cof = 2 * (active[:, 0].astype(int) + (active[:, 2] | active[:, 3]) + active[:, 4])
    assert np.array_equal(ref["rank_cof"], want_cof) and ref["rank"][50] == 1 and ref["rank"][20] == 0
    assert np.all(ref["rank"][[19, 21, 29, 30, 31, 32, 49, 51]] == 2) and np.all(ref["rank_cof"][[30, 31]] == 4)
    ctx, _ = map_context(capi, CHROM_LENS)
    got = ctx.qtl_scan_cof(origin, pheno, cof, excl=excl)
    compare_cof(dict(got, lod=got["lod"][:1], lod_base=got["lod_base"][:1], coef=got["coef"][:1], rss0=got["rss0"][:1]), ref, cs,
                "degenerate designs")
    assert np.isfinite(got["coef"][0, 50, 0]) and np.isnan(got["coef"][0, 50, 1])
    assert np.all(got["lod"][:, 20] == 0.0) and np.isnan(got["coef"][:, 20]).all()
    # a constant phenotype: RSS0 = 0 exactly, LODs 0, effects NaN, beside an ordinary column
    assert np.all(got["rss0"][1] == 0.0) and np.all(got["lod"][1] == 0.0) and np.all(got["lod_base"][1] == 0.0)
    assert np.isnan(got["coef"][1]).all() and np.all(got["rss0"][0] > 0.0) and got["lod"][0].max() > 1.0
    # without the uninformative cofactor and the twin: the same LODs, rank_cof the same count of kept columns
    less = ctx.qtl_scan_cof(origin, pheno, (5, 30, 70), excl=windows((5, 30, 70), 1, cs))
    same = np.ones(M, bool)
    same[[29, 32]] = False                   # (there the twin 31 is still in the design where 30 is left out)
    err = max(np.abs(got["lod"][:, same] - less["lod"][:, same]).max(), np.abs(got["lod_base"][:, same] - less["lod_base"][:, same]).max())
    print("against the call without the degenerate cofactors: %.3g" % err)
    assert err <= ATOL and np.array_equal(got["rank_cof"][same], less["rank_cof"][same])
    ctx.close()
    # n_c = W is not scanned, n_c = W + 1 is: one cofactor with dominance, W = 5
    lens = (3, 2, 2)
    cs3 = chromstarts_of(lens)
    o3, _ = soft_rows(12, lens, 4)
    o3[5:, 3:5] = 0.0
    o3[6:, 5:7] = 0.0
    y3 = noise(12, 1, 6) + (o3[:, 1, 3] - o3[:, 1, 0])[:, None]
    ref3 = reference_scan_cof(o3, cs3, y3, (1,), (1,), (1,))
    assert list(ref3["n_used"]) == [12, 5, 6] and list(ref3["usable"]) == [True, False, True]
    ctx, _ = map_context(capi, lens)
    got3 = ctx.qtl_scan_cof(o3, y3, (1,))
    ctx.close()
    assert list(got3["n_used"]) == [12, 5, 6] and got3["rss0"][0, 1] == 0.0 and got3["rss0"][0, 2] > 0.0
    assert np.all(got3["rank"][3:5] == 0) and np.all(got3["rank_cof"][3:5] == 0) and np.all(got3["lod"][:, 3:5] == 0.0)
    assert np.all(got3["lod_base"][:, 3:5] == 0.0) and np.isnan(got3["coef"][:, 3:5]).all()
    assert np.array_equal(got3["rank"], ref3["rank"]) and np.array_equal(got3["rank_cof"], ref3["rank_cof"]) and np.all(got3["rank_cof"][5:7] == 2)
    well = np.all(np.isnan(ref3["relpivot"]) | (ref3["relpivot"] >= PIVOT_WELL), axis=1)
    err3 = np.abs(got3["lod"][:, well] - ref3["lod"][0][:, well]).max()
    print("n_c = W + 1: lod %.3g over the %d well-conditioned markers" % (err3, well.sum()))
    assert err3 <= ATOL and well[:3].all()


# ------------------------------------------------------------------------------------- 6. permutations
def test_identity_permutation_and_candidates(capi):
    """the identity permutation gives the observed maxima over the candidate markers to the bit; a marker inside a range
    never sets perm_max, though the chromosome's largest LOD sits there"""
    origin, pheno = planted_case()
    n, m0, hw = PLANTED["n"], PLANTED["loci"][0], PLANTED["hw"]
    cs = chromstarts_of(CHROM_LENS)
    C = len(cs) - 1
    excl = windows([m0], hw, cs)
    plain, cond, _ = planted_reference()
    c0 = int(np.searchsorted(cs, m0, side="right") - 1)
    seg = cond["lod"][0, cs[c0]:cs[c0 + 1]]
    inside = excl[0][0] <= cs[c0] + int(np.argmax(seg)) <= excl[1][0]
    assert inside and not cond["candidate"][m0], "on the reference the chromosome's largest LOD sits inside the range"
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3)[0], ident])
    ctx, _ = map_context(capi, CHROM_LENS)
    got = ctx.qtl_scan_cof(origin, pheno, [m0], excl=excl, perm=perm)
    ctx.close()
    cand = cond["candidate"]
    observed = np.zeros((1, C))
    for c in range(C):
        k = np.flatnonzero(cand[cs[c]:cs[c + 1]]) + cs[c]
        observed[0, c] = got["lod"][0, k].max() if k.size else 0.0
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed)
    assert got["perm_max"][0, 0, c0] < got["lod"][0, cs[c0]:cs[c0 + 1]].max() - 1.0
    assert np.abs(got["lod"] - cond["lod"]).max() <= ATOL


# ------------------------------------------------------------------------------------- 7. refusals
def test_refusals(capi):
    """everything the entry point refuses returns CNF2_ERR_ARG and leaves host and device outputs alone"""
    case = CASES[1]
    n, K, cof, hw, additive, seed, T, P, mask, skipped = case
    origin, pheno, cov, use, perm, excl = make_case(*case)
    ctx, cs = map_context(capi, CHROM_LENS)
    M, C = int(cs[-1]), len(cs) - 1
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    lo, hi = excl
    holed = pheno.copy()
    holed[6, 1] = np.nan
    twice = perm.copy()
    twice[0, 3] = twice[0, 2]
    swap = lambda v, i, x: np.concatenate([v[:i], [x], v[i + 1:]]).astype(np.int32)
    base = dict(pheno=pheno, cov=cov, perm=perm, cof=np.asarray(cof, np.int32), lo=lo, hi=hi, flags=0)
    refusals = [dict(flags=capi.QTL_IMPRINT), dict(cof=swap(base["cof"], 1, 5)), dict(cof=np.asarray(cof, np.int32)[::-1].copy()),
                dict(cof=swap(base["cof"], 2, M), hi=swap(hi, 2, M)), dict(cof=swap(base["cof"], 0, -1)),
                dict(hi=swap(hi, 1, int(cs[4]))), dict(lo=swap(lo, 1, int(cs[3]) - 1)), dict(lo=swap(lo, 1, 27)), dict(hi=swap(hi, 1, 25)),
                dict(cov=np.zeros((n, 7))),                                             # W = 1 + 7 + 2 * 4 = 16
                dict(pheno=holed), dict(perm=twice), dict(cov=np.zeros((n, 9)))]
    for change in refusals:
        kw = dict(base, **change)
        ne = 2
        out = dict(lod=np.full((T, M), 77.0), lod_base=np.full((T, M), 77.0), coef=np.full((T, M, ne), 77.0), rank=np.full(M, 77, np.int32),
                   rank_cof=np.full(M, 77, np.int32), rss0=np.full((T, C), 77.0), n_used=np.full(C, 77, np.int32),
                   perm_max=np.full((P, T, C), 77.0))
        rc = raw_call(capi, ctx, n, p(origin), kw["pheno"], kw["cof"], (kw["lo"], kw["hi"]), kw["cov"], None, kw["perm"],
                      {k: p(v) for k, v in out.items()}, kw["flags"])
        assert rc == -2 and all(np.all(v == 77) for v in out.values()), change
        d = device_outputs(out)
        rc = raw_call(capi, ctx, n, p(origin), kw["pheno"], kw["cof"], (kw["lo"], kw["hi"]), kw["cov"], None, kw["perm"],
                      pointers(capi, d), kw["flags"] | capi.OUT_DEVICE)
        ctx.sync()
        assert rc == -2 and all(bool((x == 77).all()) for x in d.values()), change
    # the widest design is taken: six cofactors with dominance, W = 15; a seventh is not, nor are fourteen additive ones
    wide = (10, 25, 40, 45, 60, 75)
    assert ctx.qtl_scan_cof(origin, pheno, wide)["rank_cof"].max() == 12
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
        ctx.qtl_scan_cof(origin, pheno, wide + (80,))
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
        ctx.qtl_scan_cof(origin, pheno, tuple(range(3, 17)), additive=True)
    assert ctx.qtl_scan_cof(origin, pheno, tuple(range(3, 16)), additive=True)["lod"].shape == (T, M)      # thirteen additive: W = 15
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_cof_device(n, None, pheno, cof)              # no rows in the context
    ctx.close()


# ------------------------------------------------------------------------------------- 8. planted effects
def test_planted_loci_forward_selection(capi):
    """planted_case: effects at markers 42 and 67.  The reference alone must show that conditioning on 42 raises the LOD at 67
    and that forward selection enters 42, then 67, then stops; qtl.scan_cof, forward_select and fit_multi then agree with it"""
    import torch
    p = PLANTED
    origin, pheno = planted_case()
    cs = chromstarts_of(CHROM_LENS)
    plain, cond, sel = planted_reference()
    m0, m1 = p["loci"]
    print("reference: LOD at %d plain %.2f, given %d %.2f; forward selection %s at %s against %s, then %s" % (
        m1, plain["lod"][0, m1], m0, cond["lod"][0, m1], sel["loci"], np.round(sel["lod"], 2), np.round(sel["threshold"], 2), sel["stopped"]))
    assert cond["lod"][0, m1] > plain["lod"][0, m1] + 5.0
    assert sel["loci"] == [m0, m1] and sel["stopped"] is not None and sel["stopped"]["lod"] < sel["stopped"]["threshold"]
    assert sel["fit"]["drop_one"][0, 0] > plain["lod"][0, m0] + 5.0
    ctx, _ = map_context(capi, CHROM_LENS)
    ctx.n_ind = p["n"]                             # (qtl.scan_cof asks for a row per analysed individual; the rows are handed to it)
    rows = torch.from_numpy(origin).cuda()
    excl = qtl.cofactor_windows([m0], planted_pos(), cs, 2.0 * p["hw"])
    assert np.array_equal(excl[0], windows([m0], p["hw"], cs)[0]) and np.array_equal(excl[1], windows([m0], p["hw"], cs)[1])
    got = qtl.scan_cof(ctx, pheno, [m0], excl=excl, rows=rows)
    err = np.abs(got["lod"] - cond["lod"]).max()
    gsel = qtl.forward_select(ctx, pheno, 5, 2.0 * p["hw"], planted_pos(), permutations=p["permutations"], seed=p["perm_seed"], rows=rows)
    fit = qtl.fit_multi(ctx, pheno, sel["loci"], rows=rows)
    ctx.close()
    errs = dict(scan=err, entry=np.abs(np.array(gsel["lod"]) - np.array(sel["lod"])).max(),
                threshold=np.abs(np.array(gsel["threshold"]) - np.array(sel["threshold"])).max(),
                stopped=abs(gsel["stopped"]["lod"] - sel["stopped"]["lod"]) + abs(gsel["stopped"]["threshold"] - sel["stopped"]["threshold"]),
                full=np.abs(fit["lod_full"] - sel["fit"]["lod_full"]).max(), drop=np.abs(fit["drop_one"] - sel["fit"]["drop_one"]).max(),
                coef=np.abs(fit["coef"] - sel["fit"]["coef"]).max())
    print("qtl.scan_cof, forward_select, fit_multi against the reference: %s" % ", ".join("%s %.3g" % kv for kv in errs.items()))
    assert gsel["loci"] == sel["loci"] and gsel["stopped"]["marker"] == sel["stopped"]["marker"]
    assert all(e <= ATOL for e in errs.values()), errs
    assert np.array_equal(gsel["fit"]["drop_one"], fit["drop_one"]) and 0.0 < fit["var_drop"][0, 1] < fit["var_drop"][0, 0] < fit["var_full"][0] < 1.0


# ------------------------------------------------------------------------------------- 9. end to end
def test_end_to_end_on_a_swept_cross(capi):
    """qtl.scan_cof on an F2 the product sweeps itself: within 1e-9 of the reference on the product's own origin_rows, two
    traits of which one has a missing value, 3 permutations; the other scans on the same context keep their bits"""
    ped = synth.make_f2(24, 17, 2, seed=7)
    n, M = len(ped.dous), ped.n_markers
    cs = np.asarray(ped.chromstarts)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = qtl.origin_rows(ctx)
    o = rows.cpu().numpy()
    a = o[:, :, 3] - o[:, :, 0]
    cof = (4, M - 3)
    pheno = np.stack([a[:, 4] + 0.8 * a[:, M - 3], a[:, 2] + 0.5 * a[:, M - 3]], axis=1) + noise(n, 2, 8)
    pheno[3, 1] = np.nan                                   # the second trait has its own pattern of missing values
    excl = qtl.cofactor_windows(cof, ped.pos, cs, 0.25 * (ped.pos[cs[1] - 1] - ped.pos[0]))
    assert excl[0][0] < 4 < excl[1][0]
    before = (ctx.qtl_scan_device(n, rows.data_ptr(), pheno[:, :1]), ctx.qtl_scanx_device(n, rows.data_ptr(), pheno[:, :1], imprint=True))
    kw = dict(excl=excl, permutations=3, seed=4)
    got = qtl.scan_cof(ctx, pheno, cof, rows=rows, **kw)
    after = (ctx.qtl_scan_device(n, rows.data_ptr(), pheno[:, :1]), ctx.qtl_scanx_device(n, rows.data_ptr(), pheno[:, :1], imprint=True))
    for b, c in zip(before, after):
        same_bits(b, c, ("lod", "coef", "rank", "rss0", "n_used"))
    for t in range(2):
        use = np.isfinite(pheno[:, t])
        yk = np.where(use, pheno[:, t], 0.0)[:, None]
        ref = reference_scan_cof(o, cs, yk, cof, excl[0], excl[1], use)
        perm = qtl.permutations(n, 3, 4, use=use)
        res = qtl.null_residuals(yk, qtl.cofactor_columns(o, cof), use)
        ref_pm = reference_scan_cof(o, cs, res, cof, excl[0], excl[1], use, perm=perm)["perm_max"]
        one = dict(lod=got["lod"][t:t + 1], lod_base=got["lod_base"][t:t + 1], coef=got["coef"][t:t + 1], rank=got["rank"][t],
                   rank_cof=got["rank_cof"][t], n_used=got["n_used"][t], rss0=ref["rss0"], perm_max=None)
        compare_cof(one, dict(ref, perm_max=ref["perm_max"]), cs, "qtl.scan_cof trait %d" % t, share=0.9, strict=False)
        err_p = np.abs(got["perm_max"][:, t:t + 1] - ref_pm).max()
        print("trait %d perm_max %.3g" % (t, err_p))
        assert err_p <= ATOL and got["n_used"][t, 0] == n - t
    keys = ("lod", "lod_base", "coef", "rank", "rank_cof", "n_used", "perm_max")
    same_bits(got, qtl.scan_cof(ctx, pheno, cof, **kw), keys)      # a sweep of its own
    ctx.set_batch_jobs(5)
    same_bits(got, qtl.scan_cof(ctx, pheno, cof, **kw), keys)
    ctx.set_batch_jobs(0)
    # the rows a sweep_qtl left in the context: read in place and left valid
    y0 = pheno[:, :1]
    direct = ctx.qtl_scan_cof_device(n, rows.data_ptr(), y0, cof, excl=excl)
    single = ctx.sweep_qtl(y0)
    kept = ctx.qtl_scan_cof_device(n, None, y0, cof, excl=excl)
    same_bits(direct, kept, ("lod", "lod_base", "coef", "rank", "rank_cof", "rss0", "n_used"))
    assert direct["lod"][0].tobytes() == got["lod"][0].tobytes()
    again = ctx.qtl_scan_device(n, None, y0)               # the call left the rows valid
    assert again["lod"].tobytes() == single["lod"].tobytes()
    # ... and fetched at the cofactors as the device rows hold them
    assert ctx.qtl_kept_rows(n, cof).tobytes() == np.ascontiguousarray(o[:, list(cof)].transpose(1, 0, 2)).tobytes()
    ctx.upload_map(ped.pos, ped.chromstarts)
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_cof_device(n, None, y0, cof, excl=excl)
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_kept_rows(n, cof)
    ctx.close()


# ------------------------------------------------------------------------------------- 10. command line
def test_cli_qtlcof(capi, tmp_path):
    """cnF2freq --qtlcof on an F2 of 14 on two chromosomes written to files: two traits of which one has missing values of its
    own, a covariate, two cofactors with a window, 25 permutations.  Every figure of the file is qtl.scan_cof's on
    host.Run.from_files of the same files, to the printed digits; --output and the --qtl and --qtlx files are the same bytes
    with and without --qtlcof."""
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
    y = np.stack([g(4) + 0.5 * g(12) + noise(n, 1, 2)[:, 0], noise(n, 1, 3)[:, 0] * 4.0 + g(12)], axis=1)
    y[3, 1] = np.nan                                 # the second trait has its own pattern of missing values
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id w age h"] + ["%s %s %s %s" % (names[i], cell(y[i, 0]), cell(age[i]), cell(y[i, 1])) for i in range(n)]
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    cof = (4, 12)
    window = 0.3 * float(ped.pos[cs[1] - 1] - ped.pos[0])
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--phenofile", str(ph),
            "--qtl-covariates", "age", "--qtl-permutations", "25", "--qtl-seed", "4"]
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    p = lambda name: str(tmp_path / name)
    copts = ["--qtl-cofactors", "12,4", "--qtl-window", repr(window)]
    run("--output", p("a.out"), "--qtl", p("q1.txt"), "--qtlx", p("qx.txt"))
    run("--output", p("b.out"), "--qtlcof", p("qc.txt"), *copts)
    run("--output", p("c.out"), "--qtl", p("q1b.txt"), "--qtlx", p("qxb.txt"), "--qtlcof", p("qcb.txt"), *copts)
    read = lambda name: open(p(name), "rb").read()
    assert read("a.out") == read("b.out") == read("c.out")
    assert read("q1.txt") == read("q1b.txt") and read("qx.txt") == read("qxb.txt") and read("qc.txt") == read("qcb.txt")
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    excl = qtl.cofactor_windows(cof, ped.pos, cs, window)
    want = qtl.scan_cof(ctx, y, cof, excl=excl, cov=age[:, None], permutations=25, seed=4)
    ctx.close()
    r.close()
    assert excl[1][0] > 4 and excl[0][1] < 12
    thr = qtl.thresholds(want["perm_max"])
    tables = read("qc.txt").decode().strip("\n").split("\n\n")
    assert len(tables) == 2
    worst, big = 0.0, 0.0
    for t, tab in enumerate(tables):
        lines = [ln.split("\t") for ln in tab.split("\n")]
        assert lines[0] == ["trait", ["w", "h"][t]] and len(lines) == 2 + M
        assert lines[1][:2] == ["threshold", "lod"] and float(lines[1][2]) > 0.0
        for a in range(2):
            worst = max(worst, abs(float(lines[1][2 + a]) - thr["genome"][a, t]))
        for m, x in enumerate(lines[2:]):
            c = int(np.searchsorted(cs, m, side="right") - 1)
            assert len(x) == 9 and int(x[0]) == c + 1 and int(x[2]) == want["n_used"][t, c] == n - t
            assert int(x[3]) == want["rank_cof"][t, m] and int(x[5]) == want["rank"][t, m]
            figures = [(x[1], ped.pos[m]), (x[4], want["lod_base"][t, m]), (x[6], want["lod"][t, m])]
            for text, v in zip(x[7:], want["coef"][t, m]):
                assert (text == "-") == bool(np.isnan(v))
                if text != "-":
                    figures.append((text, v))
            for text, value in figures:
                assert len(text.split(".")[1]) == 5
                worst = max(worst, abs(float(text) - value) / max(1.0, abs(value)))
            big = max(big, want["lod"][t, m])
    print("file against qtl.scan_cof: %.3g; largest conditional LOD %.2f" % (worst, big))
    assert worst <= 0.51e-5 and big > 0.5
