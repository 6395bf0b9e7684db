"""GPU suite: the two-QTL pair scan (cnf2_qtl_scan2, cnf2_set_qtl2_columns, Context.qtl_scan2, qtl.scan2 / thresholds2 /
pair_summary, cnF2freq --qtl2).  The additive-pair and the full Haley-Knott model of every pair of selected loci, checked
against a per-pair least-squares fit in numpy (tests/qtl2_reference.py): on hand-made rows at the shapes where the tiling can
go wrong, on selections, on degenerate designs, for its permutations, on the rows a sweep left in the context, on planted
epistasis and through the command line.

Measured on an MI355X (largest absolute error against the reference over the compared pairs): see DESIGN.md section 8i."""
import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, noise, skip, soft_rows
from qtl2_reference import compare2, compared_pairs, degenerate_case, exact_case, reference_scan2

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod_add", "lod_full", "rank_add", "rank_full", "rss0", "n_used", "perm_max")
ALL = np.arange(sum(CHROM_LENS), dtype=np.int32)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens):
    """a context that holds a map only: what cnf2_qtl_scan2 needs"""
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
#        n    K  seed  T   P  mask   skip   additive       (n mod 4 = 0, 3, 2, 0, 1; columns 1, 6, 17, 34, 18, 102)
CASES = [(40, 2, 5, 1, 0, False, False, False),
         (67, 2, 7, 3, 1, True, True, False),
         (130, 6, 9, 17, 0, False, False, False),
         (24, 0, 3, 1, 33, False, False, False),
         (41, 2, 6, 3, 5, True, False, True),
         (67, 2, 7, 17, 5, False, True, True)]


def make_case(n, K, seed, T, P, mask, skipped):
    """(origin, pheno, cov, use, perm) on the map CHROM_LENS: the rows and covariates of the issue's conditioning check, and
    phenotypes with additive and epistatic effects plus noise.  Unused individuals carry NaN phenotypes and covariates."""
    origin, _ = soft_rows(n, CHROM_LENS, seed)
    M = origin.shape[1]
    if skipped:
        origin = skip(origin, [1, n - 2], 3, CHROM_LENS)
    use = np.ones(n, bool)
    if mask:
        use[[0, n // 2]] = False
    cov = noise(n, K, seed + 1) if K else None
    a = origin[:, :, 3] - origin[:, :, 0]
    d = origin[:, :, 1] + origin[:, :, 2]
    at = [(7 * t + 3) % M for t in range(T)]
    to = [(11 * t + 40) % M for t in range(T)]
    pheno = 0.6 * a[:, at] + 0.3 * d[:, to] + 0.8 * a[:, at] * a[:, to] + noise(n, T, seed + 2)
    if K:
        pheno = pheno + 0.3 * cov[:, :1]
        cov = np.where(use[:, None], cov, np.nan)
    pheno = np.where(use[:, None], pheno, np.nan)
    perm = qtl.permutations(n, P, seed, use=use) if P else None
    return origin, pheno, cov, (use if mask else None), perm


@pytest.mark.parametrize("n,K,seed,T,P,mask,skipped,additive", CASES)
def test_scan2_on_hand_made_rows(capi, n, K, seed, T, P, mask, skipped, additive):
    """every output against the least-squares fit with all 84 markers selected (3 486 pairs, 2 596 on different
    chromosomes); the same bits with column tiles of 16, on a second call and from device rows"""
    import torch
    origin, pheno, cov, use, perm = make_case(n, K, seed, T, P, mask, skipped)
    cs = chromstarts_of(CHROM_LENS)
    ref = reference_scan2(origin, cs, ALL, pheno, use, cov, perm, additive)
    compared_pairs(ref)                          # the conditions of the comparison, on the reference, before anything runs
    ctx, _ = map_context(capi, CHROM_LENS)
    got = ctx.qtl_scan2(origin, ALL, pheno, cov=cov, use=use, perm=perm, additive=additive)
    compare2(got, ref, "n %d K %d T %d P %d" % (n, K, T, P))
    if skipped:
        assert got["n_used"][3, 3] == got["n_used"][0, 0] - 2 and got["n_used"][0, 3] == got["n_used"][3, 0] == got["n_used"][3, 3]
    same_bits(got, ctx.qtl_scan2(origin, ALL, pheno, cov=cov, use=use, perm=perm, additive=additive))
    ctx.set_qtl2_columns(16)
    same_bits(got, ctx.qtl_scan2(origin, ALL, pheno, cov=cov, use=use, perm=perm, additive=additive))
    ctx.set_qtl2_columns(0)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan2_device(n, d_o.data_ptr(), ALL, pheno, cov=cov, use=use, perm=perm, additive=additive))
    ctx.close()


# ------------------------------------------------------------------------------------- 2. selections
def test_selections(capi):
    """every third marker; two loci on one chromosome (one pair, full = NaN); two loci on two chromosomes; a selection with
    the single marker of the one-marker chromosome.  compare2 checks the unwritten triangle and the diagonal: NaN / -1"""
    n, K, seed = 40, 2, 5
    origin, pheno, cov, _, perm = make_case(n, K, seed, 3, 1, False, False)
    cs = chromstarts_of(CHROM_LENS)
    ctx, _ = map_context(capi, CHROM_LENS)
    for sel in (ALL[::3], [20, 30], [5, 70], [0, 1, 2, 18, 83]):
        sel = np.asarray(sel, np.int32)
        ref = reference_scan2(origin, cs, sel, pheno, None, cov, perm)
        got = ctx.qtl_scan2(origin, sel, pheno, cov=cov, perm=perm)
        compare2(got, ref, "sel of %d" % len(sel), share=0.99 if len(sel) > 5 else 0.0)
        L = len(sel)
        low = ~ref["upper"]
        assert np.isnan(got["lod_add"][:, low]).all() and np.isnan(got["lod_full"][:, low]).all()
        assert np.all(got["rank_add"][low] == -1) and np.all(got["rank_full"][low] == -1)
        assert got["lod_add"].shape == (3, L, L) and got["rss0"].shape == (3, 6, 6) and np.array_equal(got["rss0"], got["rss0"].transpose(0, 2, 1))
    one = ctx.qtl_scan2(origin, [20, 30], pheno, cov=cov)
    assert np.isnan(one["lod_full"]).all() and one["rank_full"][0, 1] == -1 and np.isfinite(one["lod_add"][:, 0, 1]).all()
    assert one["rank_add"][0, 1] == 4 and np.all(one["lod_add"][:, 0, 1] > 0)
    two = ctx.qtl_scan2(origin, [5, 70], pheno, cov=cov)
    assert two["rank_full"][0, 1] == 8 and np.all(two["lod_full"][:, 0, 1] > two["lod_add"][:, 0, 1])
    ctx.close()


# ------------------------------------------------------------------------------------- 3. degenerate designs, 4. nesting
def test_degenerate_designs(capi):
    """rows without information, a certain homozygous locus, a repeated locus, a chromosome pair with n_c < K + 10: the ranks
    the rule must give, LOD exactly 0 where the rank is 0; lod_full >= lod_add (compare2); and the additive-pair LOD of a
    pair whose second locus carries no information is the single-locus LOD of cnf2_qtl_scan at the first"""
    lens, origin, sel, pheno, want = degenerate_case()
    cs = chromstarts_of(lens)
    ctx, _ = map_context(capi, lens)
    for additive in (False, True):
        ref = reference_scan2(origin, cs, sel, pheno, additive=additive)
        got = ctx.qtl_scan2(origin, sel, pheno, additive=additive)
        compare2(got, ref, "degenerate designs" + (" additive" if additive else ""), share=0.0)
        for (j, k), (ra, rf) in want[additive].items():
            assert (got["rank_add"][j, k], got["rank_full"][j, k]) == (ra, rf), (additive, j, k)
            if ra == 0:
                assert np.all(got["lod_add"][:, j, k] == 0.0)
            if rf == 0:
                assert np.all(got["lod_full"][:, j, k] == 0.0)
        assert got["n_used"][0, 6] == got["n_used"][6, 6] == 9 and got["n_used"][0, 0] == 24
        assert np.all(got["rss0"][:, 6, :] == 0.0) and np.all(got["rss0"][:, :6, :6] > 0.0)
        single = ctx.qtl_scan(origin, pheno, additive=additive)
        err = np.abs(got["lod_add"][:, 0, 1:4] - single["lod"][:, 0:1]).max()
        print("additive-pair LOD beside a locus without information against the single scan: %.3g" % err)
        assert err <= ATOL
    ctx.close()


def test_constant_and_exactly_epistatic_phenotypes(capi):
    """exact_case: a constant phenotype has RSS0 = 0 and LOD 0; y = 1 + 2 a1 a2 on certain individuals has lod_add = 0 exactly
    and lod_full = lod_int = the clamp's value"""
    lens, origin, sel, pheno, clamp = exact_case()
    ctx, _ = map_context(capi, lens)
    got = ctx.qtl_scan2(origin, sel, pheno)
    ctx.close()
    assert (got["rank_add"][0, 1], got["rank_full"][0, 1]) == (2, 3) and list(got["rss0"][:, 0, 1]) == [0.0, 64.0]
    assert got["lod_add"][0, 0, 1] == 0.0 and got["lod_full"][0, 0, 1] == 0.0
    print("clamped lod_int %.12f, expected %.12f" % (got["lod_full"][1, 0, 1] - got["lod_add"][1, 0, 1], clamp))
    assert got["lod_add"][1, 0, 1] == 0.0 and abs(got["lod_full"][1, 0, 1] - clamp) <= ATOL and np.isfinite(got["lod_full"][:, 0, 1]).all()


# ------------------------------------------------------------------------------------- 5. permutations and refusals
def test_identity_permutation_and_refusals(capi):
    import torch
    n, T, K = 40, 3, 2
    origin, pheno, cov, _, _ = make_case(n, K, 5, T, 0, False, False)
    use = np.ones(n, bool)
    use[4] = False
    sel = np.ascontiguousarray(ALL[::4])
    L = len(sel)
    ctx, cs = map_context(capi, CHROM_LENS)
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3, use=use)[0], ident])
    got = ctx.qtl_scan2(origin, sel, pheno, cov=cov, use=use, perm=perm)
    ref = reference_scan2(origin, cs, sel, pheno, use, cov, perm)
    compare2(got, ref, "identity permutation", share=0.98)
    cross = ref["cross"]
    observed = np.stack([got["lod_add"][:, ref["upper"]].max(axis=1), got["lod_full"][:, cross].max(axis=1),
                         (got["lod_full"] - got["lod_add"])[:, cross].max(axis=1)], axis=1)
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed)
    # refused, with the outputs left alone: everything cnf2_qtl_scan refuses, then K = 7 and the selections that are no
    # strictly ascending list of markers of the map
    moved = ident.copy()
    moved[[4, 5]] = [5, 4]
    twice = ident.copy()
    twice[3] = 2
    holed = pheno.copy()
    holed[6, 1] = np.nan
    bad_cov = cov.copy()
    bad_cov[7, 0] = np.inf
    M = int(cs[-1])
    base = dict(pheno=pheno, cov=cov, perm=ident[None], sel=sel)
    refusals = [dict(perm=moved[None]), dict(perm=twice[None]), dict(pheno=holed), dict(cov=bad_cov), dict(cov=np.zeros((n, 9))),
                dict(cov=np.zeros((n, 7))), dict(sel=[3, 2, 10]), dict(sel=[2, 2, 10]), dict(sel=[2, 10, M]), dict(sel=[-1, 2]),
                dict(sel=[5])]
    dev = torch.device("cuda", 0)
    for change in refusals:
        kw = dict(base, **change)
        s = np.asarray(kw["sel"], np.int32)
        out = {k: np.full_like(v, 77) for k, v in got.items()}
        out["perm_max"] = np.full((1, T, 3), 77.0)
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx._qtl2_call(n, origin.ctypes.data_as(capi.C.c_void_p), s, kw["pheno"], kw["cov"], use, kw["perm"], 0, out=out)
        assert all(np.all(v == 77) for v in out.values()), change
        # ... and device outputs
        d = {k: torch.full(v.shape, 77, dtype=torch.int32 if v.dtype == np.int32 else torch.float64, device=dev) for k, v in out.items()}
        ph, cv, us, pm = ctx._qtl_inputs(n, kw["pheno"], kw["cov"], use, kw["perm"])
        p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
        rc = ctx.L.cnf2_qtl_scan2(ctx.h, n, p(origin), len(s), p(s), T, p(ph), p(us), cv.shape[1], p(cv), 1, p(pm),
                                  *[capi.C.c_void_p(d[k].data_ptr()) for k in OUT_KEYS], capi.OUT_DEVICE)
        ctx.sync()
        assert rc == -2 and all(bool((x == 77).all()) for x in d.values()), change
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):            # perm without perm_max
        out = {k: np.full_like(v, 77) for k, v in got.items()}
        out["perm_max"] = None
        ctx._qtl2_call(n, origin.ctypes.data_as(capi.C.c_void_p), sel, pheno, cov, use, ident[None], 0, out=out)
    # device outputs of a good call are the host outputs, to the bit
    d = {k: torch.full(v.shape, 77, dtype=torch.int32 if v.dtype == np.int32 else torch.float64, device=dev) for k, v in got.items()}
    ph, cv, us, pm = ctx._qtl_inputs(n, pheno, cov, use, perm)
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    rc = ctx.L.cnf2_qtl_scan2(ctx.h, n, p(origin), L, p(sel), T, p(ph), p(us), K, p(cv), len(pm), p(pm),
                              *[capi.C.c_void_p(d[k].data_ptr()) for k in OUT_KEYS], capi.OUT_DEVICE)
    assert rc == 0
    same_bits(got, {k: v.cpu().numpy() for k, v in d.items()})
    ctx.close()


# ------------------------------------------------------------------------------------- 6. the rows a sweep left
def test_context_rows(capi):
    import torch
    ped = synth.make_f2(24, 17, 2, seed=7)
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    cov = synth.uniform(21, np.arange(n)).reshape(n, 1)
    use = np.ones(n, bool)
    use[2] = False
    perm = qtl.permutations(n, 3, 9, use=use)
    sel = qtl.select_every(ped.chromstarts, 2)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = ctx.sweep_origins()["origin"]
    a = rows[:, :, 3] - rows[:, :, 0]
    pheno = np.stack([a[:, 4] * a[:, M - 3], a[:, 2]], axis=1) + noise(n, 2, 8)
    single = ctx.sweep_qtl(pheno, cov=cov, use=use)
    kept = ctx.qtl_scan2_device(n, None, sel, pheno, cov=cov, use=use, perm=perm)
    dev = torch.device("cuda", 0)
    t = lambda *shape, dtype=torch.float64: torch.full(shape, 77, dtype=dtype, device=dev)
    d_f, d_l, d_o, d_s, d_c = t(n, C, 8), t(n, C), t(n, M, 4), t(M, 4), t(C, dtype=torch.int32)
    other = capi.Context(0)
    other.upload(ped)
    other.sweep_origins_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_o.data_ptr(), None, d_s.data_ptr(), d_c.data_ptr())
    other.sync()
    same_bits(kept, other.qtl_scan2_device(n, d_o.data_ptr(), sel, pheno, cov=cov, use=use, perm=perm))
    other.close()
    # the call leaves the context's rows valid: a single scan and another pair scan follow
    again = ctx.qtl_scan_device(n, None, pheno, cov=cov, use=use)
    for k in ("lod", "coef", "rank", "rss0", "n_used"):
        assert again[k].tobytes() == single[k].tobytes(), k
    same_bits(kept, ctx.qtl_scan2_device(n, None, sel, pheno, cov=cov, use=use, perm=perm))
    # qtl.scan and qtl.scan2 from one sweep
    d_rows = qtl.origin_rows(ctx)
    s2 = qtl.scan2(ctx, pheno, sel, cov=cov, use=use, permutations=3, seed=4, rows=d_rows)
    assert s2["lod_add"].tobytes() == kept["lod_add"].tobytes() and s2["lod_full"].tobytes() == kept["lod_full"].tobytes()
    assert np.array_equal(qtl.scan(ctx, pheno, cov=cov, use=use, rows=d_rows)["lod"], single["lod"])

    # refused (CNF2_ERR_STATE, -3) for another n, and once an upload or another call has used the buffer
    def kept_is_refused(k=n):
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
            ctx.qtl_scan2_device(k, None, sel, pheno[:k], cov=cov[:k], use=use[:k])
    kept_is_refused()                     # (qtl.origin_rows ran a sweep of its own in this context)
    for spoil in (lambda: ctx.upload_map(ped.pos, ped.chromstarts), lambda: ctx.sweep_origins(),
                  lambda: ctx.qtl_scan2(rows, sel, pheno), lambda: ctx.upload_rows(ped.allele, ped.sure, ped.hw),
                  lambda: ctx.upload_pedigree(ped.par, ped.empty, ped.gen, ped.row_of, ped.dous)):
        ctx.sweep_qtl(pheno, cov=cov, use=use)
        same_bits(kept, ctx.qtl_scan2_device(n, None, sel, pheno, cov=cov, use=use, perm=perm))
        kept_is_refused(n - 1)
        spoil()
        kept_is_refused()
    fresh = capi.Context(0)
    fresh.upload_map(ped.pos, ped.chromstarts)
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        fresh.qtl_scan2_device(n, None, sel, pheno, use=use)
    fresh.close()
    ctx.close()


# ------------------------------------------------------------------------------------- 7. planted epistasis
def test_planted_epistasis(capi):
    """An F2 of 200 with a pure a1 a2 effect of the true genotypes at one marker on each chromosome: the reference, on the
    product's rows, has its largest lod_int on that chromosome pair with the planted markers within two loci of the best
    full pair; qtl.scan2 agrees and its lod_int exceeds the 5 % threshold of 100 permutations"""
    ped = synth.make_f2(200, 30, 2, seed=7)
    n = len(ped.dous)
    m1, m2 = 11, 30 + 17
    g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0          # -1, 0, 1 = AA, AB, BB (no missing data)
    pheno = (1.5 * g(m1) * g(m2) + 2.0 * noise(n, 1, 31)[:, 0])[:, None]
    sel = qtl.select_every(ped.chromstarts, 2)                                        # 30 loci, 435 pairs, 225 on (0, 1)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = ctx.sweep_origins()["origin"]
    ref = reference_scan2(rows, ped.chromstarts, sel, pheno)
    cmp = compared_pairs(ref, share=0.9)
    rs = qtl.pair_summary(ref["lod_add"][0], ref["lod_full"][0], sel, ped.chromstarts)
    cross = [r for r in rs if r["chrom1"] != r["chrom2"]]
    assert len(cross) == 1 and (cross[0]["chrom1"], cross[0]["chrom2"]) == (0, 1)
    assert abs(cross[0]["full"][0] - m1) <= 4 and abs(cross[0]["full"][1] - m2) <= 4, cross       # two selected loci = 4 markers
    got = qtl.scan2(ctx, pheno, sel, permutations=100, seed=5)
    ctx.close()
    err_a = np.abs(got["lod_add"] - ref["lod_add"][0])[:, cmp].max()
    err_f = np.abs(got["lod_full"] - ref["lod_full"][0])[:, cmp & ref["cross"]].max()
    print("qtl.scan2 against the reference: lod_add %.3g, lod_full %.3g" % (err_a, err_f))
    assert err_a <= ATOL and err_f <= ATOL
    gs = [r for r in qtl.pair_summary(got["lod_add"], got["lod_full"], sel, ped.chromstarts) if r["chrom1"] != r["chrom2"]]
    assert gs[0]["full"] == cross[0]["full"] and gs[0]["add"] == cross[0]["add"] and abs(gs[0]["lod_int"] - cross[0]["lod_int"]) <= ATOL
    thr = qtl.thresholds2(got["perm_max"])
    print("lod_full %.2f lod_add %.2f lod_int %.2f at %s; 5 %% thresholds add %.2f full %.2f int %.2f" % (
        gs[0]["lod_full"], gs[0]["lod_add"], gs[0]["lod_int"], gs[0]["full"], thr["add"][0, 0], thr["full"][0, 0], thr["int"][0, 0]))
    assert gs[0]["lod_int"] > thr["int"][0, 0] > 0.0 and gs[0]["lod_full"] > thr["full"][0, 0] > 0.0


# ------------------------------------------------------------------------------------- 8. command line
def write_f2_files(ped, tmp_path):
    """an F2 of synth.make_f2 as PlantImpute files (as tests/test_gpu_qtl.py writes them); returns the paths and the names"""
    n = len(ped.dous)
    names = ["F2_%d" % i for i in range(n)]
    files = [tmp_path / ("f2." + e) for e in ("map", "ped", "gen")]
    files[0].write_text("".join("%r\n" % float(p) for p in ped.pos))
    files[1].write_text("A 0 0\nB 0 0\n" + "".join("%s A B 2\n" % nm for nm in names))
    dos = np.where(ped.allele.min(axis=2) == 0, 9, ped.allele.astype(int).sum(axis=2) - 2)
    files[2].write_text("".join("%s %s\n" % (nm, " ".join(str(v) for v in dos[r])) for nm, r in [("A", 1), ("B", 2)] + [(names[i], 3 + i) for i in range(n)]))
    return [str(f) for f in files], names


def test_cli_qtl2(capi, tmp_path):
    """cnF2freq --qtl2 on an F2 of 30 on two chromosomes written to files: two traits with different missing values, a
    covariate, an individual absent from the table, 25 permutations, --qtl2-every 2.  With --count 1 every figure of the
    file is qtl.scan2's (through pair_summary and thresholds2) on host.Run.from_files of the same files, to the printed
    digits; --output is the same bytes with and without --qtl2; --qtl and --qtl2 together write the files they write alone."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    ped = synth.make_f2(30, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n, M, cs = 30, ped.n_markers, np.asarray(ped.chromstarts)
    g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
    y = np.stack([g(4) * g(13) + noise(n, 1, 2)[:, 0], noise(n, 1, 3)[:, 0] * 4.0 + g(2)], axis=1)
    y[3, 1] = y[8, 1] = np.nan                       # the second trait has its own pattern of missing values
    age = np.round(synth.uniform(5, np.arange(n)) * 10.0, 3)
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id w age h"] + ["%s %s %s %s" % (names[i], cell(y[i, 0]), cell(age[i]), cell(y[i, 1])) for i in range(n) if i != 6]
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--phenofile", str(ph),
            "--qtl-covariates", "age", "--qtl-permutations", "25", "--qtl-seed", "4"]
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    p = lambda name: str(tmp_path / name)
    run("--output", p("a.out"), "--qtl", p("q1.txt"))
    run("--output", p("b.out"), "--qtl2", p("q2.txt"), "--qtl2-every", "2")
    run("--output", p("c.out"), "--qtl", p("q1b.txt"), "--qtl2", p("q2b.txt"), "--qtl2-every", "2")
    subprocess.run(base[:10] + ["--output", p("d.out")], capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    read = lambda name: open(p(name), "rb").read()
    assert read("a.out") == read("b.out") == read("c.out") == read("d.out")
    assert read("q1.txt") == read("q1b.txt") and read("q2.txt") == read("q2b.txt")
    blocks = read("q2.txt").decode().split("\n\n")
    rows = [ln.split("\t") for ln in blocks[0].split("\n")]
    thr = [ln.split("\t") for ln in blocks[1].strip("\n").split("\n")]
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    use = np.ones(n, bool)
    use[6] = False
    sel = qtl.select_every(cs, 2)
    want = qtl.scan2(ctx, y, sel, cov=np.where(use, age, 0.0), use=use, permutations=25, seed=4)
    ctx.close()
    r.close()
    summary = qtl.pair_summary(want["lod_add"], want["lod_full"], sel, cs)
    assert len(rows) == len(summary) == 2 * 3 and all(len(x) == 16 for x in rows)
    worst = 0.0
    for x, s in zip(rows, summary):
        assert (x[0], int(x[1]), int(x[2])) == (["w", "h"][s["trait"]], s["chrom1"] + 1, s["chrom2"] + 1)
        assert int(x[3]) == want["n_used"][s["trait"], s["chrom1"], s["chrom2"]] == (29 if s["trait"] == 0 else 27)
        assert (int(x[4]), int(x[5])) == s["add"]
        figures = [(x[6], ped.pos[s["add"][0]]), (x[7], ped.pos[s["add"][1]]), (x[8], s["lod_add"])]
        if s["full"] is None:
            assert x[9:] == ["-"] * 7
        else:
            assert (int(x[9]), int(x[10])) == s["full"]
            figures += [(x[11], ped.pos[s["full"][0]]), (x[12], ped.pos[s["full"][1]]), (x[13], s["lod_full"]),
                        (x[14], s["lod_add_at_full"]), (x[15], s["lod_int"])]
        for text, value in figures:
            assert len(text.split(".")[1]) == 5
            worst = max(worst, abs(float(text) - value))
    wthr = qtl.thresholds2(want["perm_max"])
    assert [t[0] for t in thr] == ["w", "h"] and all(len(t) == 7 for t in thr)
    for t, line in enumerate(thr):
        for s, key in enumerate(("add", "full", "int")):
            for a in range(2):
                worst = max(worst, abs(float(line[1 + 2 * s + a]) - wthr[key][a, t]))
    print("file against qtl.scan2: %.3g; largest lod_full %.2f, thresholds %s" % (
        worst, max(s["lod_full"] for s in summary if s["full"]), [line[1:] for line in thr]))
    assert worst <= 0.51e-5
    assert max(s["lod_full"] for s in summary if s["full"]) > 1.0 and all(float(v) > 0.0 for line in thr for v in line[1:])
