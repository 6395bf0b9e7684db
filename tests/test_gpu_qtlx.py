"""GPU suite: the extended single-locus scan (cnf2_qtl_scanx, cnf2_set_qtlx_columns, Context.qtl_scanx, qtl.scanx /
thresholdsx / coef_names, cnF2freq --qtlx).  The nested Haley-Knott models Mendelian, imprinting and QTL x covariate
interaction of every marker, checked against a per-marker least-squares fit in numpy (tests/qtlx_reference.py): on hand-made
rows at the shapes where the tiling can go wrong, against the existing scan, on degenerate designs, for its permutations and
refusals, on planted effects, on the rows a sweep left in the context and through the command line.

Measured on an MI355X (largest absolute error against the reference): hand-made rows 8.9e-14 on the LODs,
1.1e-13 on coef; against cnf2_qtl_scan 5.8e-15; planted effects 3.2e-14; the swept F2 8.7e-12; the command line's file 5.0e-6."""
import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, noise
from qtlx_reference import (CASES, DEGENERATE, PLANTED, case_reference, compared_markers, comparex, constant_case,
                            constant_covariate_case, degenerate_case, make_case, planted_case, planted_findings,
                            planted_reference, reference_scanx)

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod", "coef", "rank", "rss0", "n_used", "perm_max")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens):
    """a context that holds a map only: what cnf2_qtl_scanx needs"""
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


# ------------------------------------------------------------------------------------- 1. values on hand-made rows
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-K%d-Ki%d-%s%s-T%d-P%d%s" % (
    c[0], c[1], c[2], "i" if c[3] else "m", "-add" if c[4] else "", c[6], c[7], "-mask" if c[8] else "-skip" if c[9] else ""))
def test_scanx_on_hand_made_rows(capi, case):
    """every output against the least-squares fit at all 84 markers; the same bits with column tiles of 16, on a second call
    and from device rows"""
    import torch
    n, K, Ki, imprint, additive, seed, T, P, mask, skipped = case
    origin, pheno, cov, use, perm = make_case(*case)
    cs = chromstarts_of(CHROM_LENS)
    ref = case_reference(case)
    compared = compared_markers(ref, cs)         # the conditions of the comparison, on the reference, before anything runs
    assert compared.all()
    ctx, _ = map_context(capi, CHROM_LENS)
    kw = dict(cov=cov, interactive=Ki, imprint=imprint, use=use, perm=perm, additive=additive)
    got = ctx.qtl_scanx(origin, pheno, **kw)
    comparex(got, ref, cs, "n %d K %d Ki %d imprint %d additive %d T %d P %d" % (n, K, Ki, imprint, additive, T, P))
    if skipped:
        assert got["n_used"][3] == n - 2 and got["n_used"][0] == n
    if mask:
        assert np.all(got["n_used"] == n - 2)
    same_bits(got, ctx.qtl_scanx(origin, pheno, **kw))
    ctx.set_qtlx_columns(16)
    same_bits(got, ctx.qtl_scanx(origin, pheno, **kw))
    ctx.set_qtlx_columns(0)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scanx_device(n, d_o.data_ptr(), pheno, **kw))
    ctx.close()


# ------------------------------------------------------------------------------------- 2. agreement with the existing scan
def test_agreement_with_qtl_scan(capi):
    """Ki = 0 and no flag: stage 0 is cnf2_qtl_scan's model -- lod, coef, rank, rss0, n_used, perm_max within 1e-9, the counts
    exact; with the flag and an interactive covariate lod[..., 0] is still that scan's"""
    cs = chromstarts_of(CHROM_LENS)
    ctx, _ = map_context(capi, CHROM_LENS)
    for case in (CASES[4], CASES[5], CASES[8]):
        n, K, Ki, imprint, additive, seed, T, P, mask, skipped = case
        origin, pheno, cov, use, perm = make_case(*case)
        one = ctx.qtl_scan(origin, pheno, cov=cov, use=use, perm=perm, additive=additive)
        got = ctx.qtl_scanx(origin, pheno, cov=cov, use=use, perm=perm, additive=additive)
        errs = dict(lod=np.abs(got["lod"][..., 0] - one["lod"]).max(),
                    coef=(np.abs(got["coef"] - one["coef"][..., :got["coef"].shape[2]]) / np.maximum(1.0, np.abs(one["coef"][..., :got["coef"].shape[2]]))).max(),
                    rss0=np.abs(got["rss0"] - one["rss0"]).max(), perm_max=np.abs(got["perm_max"][..., 0] - one["perm_max"]).max())
        print("n %d K %d additive %d against cnf2_qtl_scan: %s" % (n, K, additive, ", ".join("%s %.3g" % kv for kv in errs.items())))
        assert np.array_equal(got["rank"][:, 0], one["rank"]) and np.array_equal(got["n_used"], one["n_used"])
        assert np.array_equal(got["lod"][..., 1], got["lod"][..., 0]) and np.array_equal(got["lod"][..., 2], got["lod"][..., 0])
        assert np.array_equal(got["perm_max"][..., 1], got["perm_max"][..., 0]) and np.all(got["perm_max"][..., 3:] == 0.0)
        assert all(e <= ATOL for e in errs.values()), errs
        if additive:
            assert np.isnan(one["coef"][..., 1]).all() and got["coef"].shape[2] == 1
        full = ctx.qtl_scanx(origin, pheno, cov=cov, interactive=Ki, imprint=True, use=use, perm=perm, additive=additive)
        err = np.abs(full["lod"][..., 0] - one["lod"]).max()
        print("... with imprinting and %d interactive: lod[..., 0] %.3g" % (Ki, err))
        assert err <= ATOL and Ki > 0
    ctx.close()


# ------------------------------------------------------------------------------------- 3. degenerate designs
def test_degenerate_designs(capi):
    """rows without information, certain homozygotes, o[1] == o[2], an interactive covariate that is constant wherever the
    rows carry information, a chromosome with n_c = W: the ranks the rule must give, NaN for the dropped effects, LOD exactly
    0 where the rank is 0, a stage without kept columns repeating the previous LOD to the bit"""
    lens, origin, pheno, cov, want = degenerate_case()
    cs = chromstarts_of(lens)
    ctx, _ = map_context(capi, lens)
    perm = qtl.permutations(24, 2, 3)
    kw = dict(cov=cov, n_int=DEGENERATE["Ki"], imprint=True)
    ref = reference_scanx(origin, cs, pheno, perm=perm, **kw)
    got = ctx.qtl_scanx(origin, pheno, cov=cov, interactive=1, imprint=True, perm=perm)
    comparex(got, ref, cs, "degenerate designs", share=0.0)
    names = qtl.coef_names(1, True)
    nan_names = lambda m: [nm for nm, v in zip(names, got["coef"][0, m]) if np.isnan(v)]
    for c, ranks in want.items():
        for m in range(cs[c], cs[c + 1]):
            assert tuple(got["rank"][m]) == ranks, (c, m)
            if ranks[2] == 0:
                assert np.all(got["lod"][:, m] == 0.0) and nan_names(m) == list(names)
    assert got["n_used"][4] == 8 and np.all(got["rss0"][:, 4] == 0.0) and np.all(got["rss0"][:, [0, 1, 2, 3, 5]] > 0.0)
    assert np.all(got["perm_max"][:, :, [1, 4]] == 0.0)
    m = int(cs[2])
    assert nan_names(m) == ["d", "i", "d:z1", "i:z1"]
    m = int(cs[3])
    assert nan_names(m) == ["i", "i:z1"]
    assert np.array_equal(got["lod"][:, m:m + 2, 1], got["lod"][:, m:m + 2, 0]) and np.all(got["lod"][:, m, 2] > got["lod"][:, m, 1])
    assert np.all(got["perm_max"][:, :, 3, 3] == 0.0)
    m = int(cs[5])
    assert nan_names(m) == ["a:z1", "d:z1", "i:z1"]
    assert np.array_equal(got["lod"][:, m:m + 2, 2], got["lod"][:, m:m + 2, 1]) and np.all(got["perm_max"][:, :, 5, 4] == 0.0)
    ctx.close()
    # a covariate that is constant over everybody: X0 has no factor and nothing is scanned
    lens, origin, pheno, cov = constant_covariate_case()
    ctx, _ = map_context(capi, lens)
    got = ctx.qtl_scanx(origin, pheno, cov=cov, interactive=1)
    assert np.all(got["rank"] == 0) and np.all(got["lod"] == 0.0) and np.isnan(got["coef"]).all() and np.all(got["rss0"] == 0.0)
    assert got["n_used"][0] == 16
    ctx.close()
    # a constant phenotype
    lens, origin, pheno = constant_case()
    ctx, _ = map_context(capi, lens)
    got = ctx.qtl_scanx(origin, pheno, imprint=True)
    ctx.close()
    assert got["rss0"][0, 0] == 0.0 and got["rss0"][1, 0] > 0.0 and np.all(got["rank"] == (2, 3, 3))
    assert np.all(got["lod"][0] == 0.0) and np.isnan(got["coef"][0]).all()
    assert np.all(got["lod"][1, :, 1] > got["lod"][1, :, 0]) and np.isfinite(got["coef"][1]).all()


# ------------------------------------------------------------------------------------- 4. identity permutation, 5. refusals
def test_identity_permutation_and_refusals(capi):
    import torch
    case = CASES[5]
    n, K, Ki, imprint, additive, seed, T, P, mask, skipped = case
    origin, pheno, cov, _, _ = make_case(*case)
    use = np.ones(n, bool)
    use[4] = False
    ctx, cs = map_context(capi, CHROM_LENS)
    C, M = len(cs) - 1, int(cs[-1])
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3, use=use)[0], ident])
    got = ctx.qtl_scanx(origin, pheno, cov=cov, interactive=Ki, imprint=True, use=use, perm=perm)
    l = got["lod"]
    stat = np.concatenate([l, l[..., 1:2] - l[..., 0:1], l[..., 2:3] - l[..., 1:2]], axis=2)
    observed = np.stack([stat[:, cs[c]:cs[c + 1]].max(axis=1) for c in range(C)], axis=1)          # [T][C][5]
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed) and np.all(observed[:, 1:] > 0.0)
    # refused, with the outputs left alone
    twice = ident.copy()
    twice[3] = 2
    holed = pheno.copy()
    holed[6, 1] = np.nan
    bad_cov = cov.copy()
    bad_cov[7, 0] = np.inf
    base = dict(pheno=pheno, cov=cov, perm=ident[None], n_int=Ki, flags=capi.QTL_IMPRINT)
    refusals = [dict(n_int=K + 1), dict(n_int=-1), dict(cov=np.zeros((n, 3)), n_int=3),                # W = 1 + 3 + 3 * 4 = 16
                dict(cov=np.zeros((n, 8)), n_int=2, flags=0),                                         # W = 1 + 8 + 2 * 3 = 15 is taken ...
                dict(perm=twice[None]), dict(pheno=holed), dict(cov=bad_cov), dict(cov=np.zeros((n, 9)))]
    dev = torch.device("cuda", 0)
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    for change in refusals:
        kw = dict(base, **change)
        ne = 3 if kw["flags"] else 2
        ncoef = ne * (1 + max(kw["n_int"], 0))
        out = dict(lod=np.full((T, M, 3), 77.0), coef=np.full((T, M, ncoef), 77.0), rank=np.full((M, 3), 77, np.int32),
                   rss0=np.full((T, C), 77.0), n_used=np.full(C, 77, np.int32), perm_max=np.full((1, T, C, 5), 77.0))
        ph, cv, us, pm = ctx._qtl_inputs(n, kw["pheno"], kw["cov"], use, kw["perm"])
        args = lambda o: (ctx.h, n, p(origin), T, p(ph), p(us), cv.shape[1], p(cv), kw["n_int"], 1, p(pm))
        rc = ctx.L.cnf2_qtl_scanx(*args(out), *[p(out[k]) for k in OUT_KEYS], kw["flags"])
        if change == refusals[3]:
            assert rc == 0 and not any(np.any(v == 77) for v in out.values())                          # ... the widest design
            continue
        assert rc == -2 and all(np.all(v == 77) for v in out.values()), change
        d = {k: torch.full(v.shape, 77, dtype=torch.int32 if v.dtype == np.int32 else torch.float64, device=dev) for k, v in out.items()}
        rc = ctx.L.cnf2_qtl_scanx(*args(d), *[capi.C.c_void_p(d[k].data_ptr()) for k in OUT_KEYS], kw["flags"] | capi.OUT_DEVICE)
        ctx.sync()
        assert rc == -2 and all(bool((x == 77).all()) for x in d.values()), change
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
        ctx.qtl_scanx(origin, pheno, cov=cov, interactive=K + 1)
    # device outputs of a good call are the host outputs, to the bit
    d = {k: torch.full(v.shape, 77, dtype=torch.int32 if v.dtype == np.int32 else torch.float64, device=dev) for k, v in got.items()}
    ph, cv, us, pm = ctx._qtl_inputs(n, pheno, cov, use, perm)
    rc = ctx.L.cnf2_qtl_scanx(ctx.h, n, p(origin), T, p(ph), p(us), K, p(cv), Ki, len(pm), p(pm),
                              *[capi.C.c_void_p(d[k].data_ptr()) for k in OUT_KEYS], capi.QTL_IMPRINT | capi.OUT_DEVICE)
    assert rc == 0
    same_bits(got, {k: v.cpu().numpy() for k, v in d.items()})
    ctx.close()


# ------------------------------------------------------------------------------------- 6. planted effects
def test_planted_imprinting_and_interaction(capi):
    """planted_case: an imprinting effect at one marker and an a x z effect at a marker of another chromosome.  First the
    reference alone must find both (planted_findings, with 200 permutations of its own); then qtl.scanx on the same rows
    agrees on all of it"""
    import torch
    origin, pheno, cov = planted_case()
    cs = chromstarts_of(CHROM_LENS)
    ref, ref_pm = planted_reference()
    compared_markers(ref, cs)
    want = planted_findings(ref["lod"][0], ref_pm, "reference")
    ctx, _ = map_context(capi, CHROM_LENS)
    ctx.n_ind = PLANTED["n"]                       # (qtl.scanx asks for a row per analysed individual; the rows are handed to it)
    rows = torch.from_numpy(origin).cuda()
    got = qtl.scanx(ctx, pheno, cov=cov, interactive=1, imprint=True, permutations=PLANTED["permutations"], seed=PLANTED["perm_seed"],
                    rows=rows)
    ctx.close()
    err_l, err_p = np.abs(got["lod"] - ref["lod"][0]).max(), np.abs(got["perm_max"] - ref_pm).max()
    print("qtl.scanx against the reference: lod %.3g, perm_max %.3g" % (err_l, err_p))
    assert err_l <= ATOL and err_p <= ATOL
    assert planted_findings(got["lod"], got["perm_max"], "qtl.scanx") == want
    assert np.array_equal(got["lod_imprint"], got["lod"][..., 1] - got["lod"][..., 0])
    assert np.array_equal(got["lod_interaction"], got["lod"][..., 2] - got["lod"][..., 1])
    assert got["coef_names"] == ("a", "d", "i", "a:z1", "d:z1", "i:z1")
    ci, cz = got["coef"][0, PLANTED["m_imprint"], 2], got["coef"][0, PLANTED["m_interaction"], 3]
    print("estimated effects at the planted markers: i %.3f (planted %.1f), a:z1 %.3f (planted %.1f)" % (ci, PLANTED["e_imprint"], cz, PLANTED["e_interaction"]))
    assert abs(ci - ref["coef"][0, PLANTED["m_imprint"], 2]) <= ATOL and ci > 0.3 and cz > 0.6


# ------------------------------------------------------------------------------------- 7. end to end
def test_end_to_end_on_a_swept_cross(capi):
    """qtl.scanx on an F2 the product sweeps itself: within 1e-9 of the reference on the product's own origin_rows, the same
    bits with another batching of the sweep and from the rows a sweep_qtl left in the context, CNF2_ERR_STATE after an
    upload"""
    ped = synth.make_f2(24, 17, 2, seed=7)
    n, M = len(ped.dous), ped.n_markers
    cov = synth.uniform(21, np.arange(n)).reshape(n, 1)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = qtl.origin_rows(ctx)
    o = rows.cpu().numpy()
    a, im = o[:, :, 3] - o[:, :, 0], o[:, :, 1] - o[:, :, 2]
    pheno = np.stack([a[:, 4] + 0.8 * im[:, M - 3], a[:, 2] * (cov[:, 0] - 0.5) * 2.0], axis=1) + noise(n, 2, 8)
    pheno[3, 1] = np.nan                                   # the second trait has its own pattern of missing values
    kw = dict(cov=cov, interactive=1, imprint=True, permutations=3, seed=4)
    got = qtl.scanx(ctx, pheno, rows=rows, **kw)
    for t in range(2):
        use = np.isfinite(pheno[:, t])
        yk = np.where(use, pheno[:, t], 0.0)[:, None]
        ref = reference_scanx(o, ped.chromstarts, yk, use, cov, 1, True)
        perm = qtl.permutations(n, 3, 4, use=use)
        ref_pm = reference_scanx(o, ped.chromstarts, qtl.null_residuals(yk, cov, use), use, cov, 1, True, perm)["perm_max"]
        one = dict(lod=got["lod"][t:t + 1], coef=got["coef"][t:t + 1], rank=got["rank"][t], n_used=got["n_used"][t],
                   rss0=ref["rss0"], perm_max=None)
        comparex(one, dict(ref, perm_max=ref["perm_max"]), ped.chromstarts, "qtl.scanx trait %d" % t, share=0.9, strict=False)
        err_p = np.abs(got["perm_max"][:, t:t + 1] - ref_pm).max()
        print("trait %d perm_max %.3g" % (t, err_p))
        assert err_p <= ATOL and got["n_used"][t, 0] == n - t
    keys = ("lod", "coef", "rank", "n_used", "perm_max")
    same_bits(got, qtl.scanx(ctx, pheno, **kw), keys)      # a sweep of its own
    ctx.set_batch_jobs(5)
    same_bits(got, qtl.scanx(ctx, pheno, **kw), keys)
    ctx.set_batch_jobs(0)
    # the rows a sweep_qtl left in the context
    use = np.isfinite(pheno[:, 0])
    y0 = pheno[:, :1]
    direct = ctx.qtl_scanx_device(n, rows.data_ptr(), y0, cov=cov, interactive=1, imprint=True)
    single = ctx.sweep_qtl(y0, cov=cov)
    kept = ctx.qtl_scanx_device(n, None, y0, cov=cov, interactive=1, imprint=True)
    same_bits(direct, kept, ("lod", "coef", "rank", "rss0", "n_used"))
    assert direct["lod"][0].tobytes() == got["lod"][0].tobytes()
    again = ctx.qtl_scan_device(n, None, y0, cov=cov)      # the call left the rows valid
    assert again["lod"].tobytes() == single["lod"].tobytes()
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scanx_device(n - 1, None, y0[:-1], cov=cov[:-1], interactive=1)
    ctx.upload_map(ped.pos, ped.chromstarts)
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scanx_device(n, None, y0, cov=cov, interactive=1, imprint=True)
    ctx.close()


# ------------------------------------------------------------------------------------- 8. command line
def test_cli_qtlx(capi, tmp_path):
    """cnF2freq --qtlx on an F2 of 14 on two chromosomes written to files: two traits of which one has missing values of its
    own, two covariates of which the second is interactive, imprinting, 25 permutations.  Every figure of the file is
    qtl.scanx's on host.Run.from_files of the same files, to the printed digits; --output is the same bytes with and without
    --qtlx; --qtl and --qtlx together write the files they write alone."""
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
    sex = np.where(synth.uniform(6, np.arange(n)) < 0.5, 0.0, 1.0)
    y = np.stack([g(4) * (sex - 0.5) + noise(n, 1, 2)[:, 0], noise(n, 1, 3)[:, 0] * 4.0 + g(12)], axis=1)
    y[3, 1] = np.nan                                 # the second trait has its own pattern of missing values
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id w age sex h"] + ["%s %s %s %s %s" % (names[i], cell(y[i, 0]), cell(age[i]), cell(sex[i]), cell(y[i, 1])) for i in range(n)]
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--phenofile", str(ph),
            "--qtl-covariates", "age,sex", "--qtl-permutations", "25", "--qtl-seed", "4"]
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    p = lambda name: str(tmp_path / name)
    xopts = ["--qtl-imprint", "--qtl-interactive", "sex"]
    run("--output", p("a.out"), "--qtl", p("q1.txt"))
    run("--output", p("b.out"), "--qtlx", p("qx.txt"), *xopts)
    run("--output", p("c.out"), "--qtl", p("q1b.txt"), "--qtlx", p("qxb.txt"), *xopts)
    subprocess.run(base[:10] + ["--output", p("d.out")], capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    read = lambda name: open(p(name), "rb").read()
    assert read("a.out") == read("b.out") == read("c.out") == read("d.out")
    assert read("q1.txt") == read("q1b.txt") and read("qx.txt") == read("qxb.txt")
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    want = qtl.scanx(ctx, y, cov=np.stack([sex, age], axis=1), interactive=1, imprint=True, permutations=25, seed=4)
    ctx.close()
    r.close()
    thr = qtl.thresholdsx(want["perm_max"])
    tables = read("qx.txt").decode().strip("\n").split("\n\n")
    assert len(tables) == 2 and want["coef_names"] == ("a", "d", "i", "a:z1", "d:z1", "i:z1")
    worst, big = 0.0, 0.0
    for t, tab in enumerate(tables):
        lines = [ln.split("\t") for ln in tab.split("\n")]
        assert lines[0] == ["trait", ["w", "h"][t]] and len(lines) == 1 + M + 5
        for m, x in enumerate(lines[1:1 + M]):
            c = int(np.searchsorted(cs, m, side="right") - 1)
            assert len(x) == 11 + 6 and int(x[0]) == c + 1 and int(x[2]) == want["n_used"][t, c] == n - t
            assert [int(v) for v in x[8:11]] == list(want["rank"][t, m])
            l = want["lod"][t, m]
            figures = [(x[1], ped.pos[m]), (x[3], l[0]), (x[4], l[1]), (x[5], l[2]), (x[6], want["lod_imprint"][t, m]),
                       (x[7], want["lod_interaction"][t, m])]
            for text, v in zip(x[11:], want["coef"][t, m]):
                assert (text == "-") == bool(np.isnan(v))
                if text != "-":
                    figures.append((text, v))
            for text, value in figures:
                assert len(text.split(".")[1]) == 5
                worst = max(worst, abs(float(text) - value) / max(1.0, abs(value)))
            big = max(big, l[2])
        for s, (x, key) in enumerate(zip(lines[1 + M:], ("lod0", "lod1", "lod2", "imprint", "interaction"))):
            assert x[0] == "threshold" and x[1] == ("lod_mendelian", "lod_imprinting", "lod_full", "lod_imprint", "lod_interaction")[s]
            for a in range(2):
                worst = max(worst, abs(float(x[2 + a]) - thr[key]["genome"][a, t]))
            assert float(x[2]) > 0.0
    print("file against qtl.scanx: %.3g; largest full LOD %.2f" % (worst, big))
    assert worst <= 0.51e-5 and big > 1.0
