"""GPU suite: the QTL scan (cnf2_qtl_scan, cnf2_sweep_qtl, cnf2_set_qtl_columns, Context.qtl_scan / sweep_qtl,
cnf2freq_amd/qtl.py).  Haley-Knott regression on the origin rows, checked against a per-marker least-squares fit in numpy
(tests/qtl_reference.py) on hand-made rows at the shapes where the tiling can go wrong, on degenerate markers, for its
permutations, through the sweep on two pedigrees and on a planted QTL."""
import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import (ATOL, CHROM_LENS, CLAMP, chromstarts_of, compare, compared_markers, noise, reference_scan, skip,
                           soft_rows)

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod", "coef", "rank", "rss0", "n_used", "perm_max")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens):
    """a context that holds a map only: what cnf2_qtl_scan needs"""
    cs = chromstarts_of(lens)
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in lens])
    ctx = capi.Context(0)
    ctx.upload_map(pos, cs)
    return ctx, cs, pos


def same_bits(a, b, keys=OUT_KEYS):
    for k in keys:
        if a[k] is None:
            assert b[k] is None
        else:
            assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------- 1. the scan on hand-made rows
#        n   T   P  K  mask   skip   additive
CASES = [(5, 1, 0, 0, False, False, False),
         (13, 3, 1, 2, True, True, False),
         (17, 17, 5, 0, False, False, True),
         (64, 1, 33, 2, False, True, False),
         (67, 3, 33, 0, True, True, False),
         (67, 17, 5, 2, False, False, False),        # R = 102: the second wave of a block, a partial column tile of 16
         (64, 17, 33, 0, True, False, True)]         # R = 578: three column groups of 256


# With five individuals many draws of the rows have a marker at which only two genotypes occur and the three columns of the
# design come close to one plane; this seed's rows keep every relative pivot above 5e-3 (compared_markers asserts it)
ROW_SEEDS = {5: 2}


def make_case(n, T, P, K, mask, skipped, seed=11):
    """(origin, pheno, cov, use, perm) on the map CHROM_LENS.  Unused individuals carry NaN phenotypes and covariates."""
    origin, _ = soft_rows(n, CHROM_LENS, ROW_SEEDS.get(n, seed + n))
    M = origin.shape[1]
    if skipped:
        origin = skip(origin, [1, n - 2], 3, CHROM_LENS)
    use = np.ones(n, bool)
    if mask:
        use[[0, n // 2]] = False
    cov = None
    if K:
        cov = synth.uniform(seed * 16 + 9, np.arange(n * K)).reshape(n, K) * 2.0 - 1.0
    a = origin[:, :, 3] - origin[:, :, 0]
    d = origin[:, :, 1] + origin[:, :, 2]
    at = [(7 * t + 3) % M for t in range(T)]
    pheno = 0.8 * a[:, at] + 0.4 * d[:, at] + noise(n, T, seed)
    if K:
        pheno = pheno + 0.3 * cov[:, :1]
        cov = np.where(use[:, None], cov, np.nan)
    pheno = np.where(use[:, None], pheno, np.nan)
    perm = qtl.permutations(n, P, seed, use=use) if P else None
    return origin, pheno, cov, (use if mask else None), perm


@pytest.mark.parametrize("n,T,P,K,mask,skipped,additive", CASES)
def test_scan_on_hand_made_rows(capi, n, T, P, K, mask, skipped, additive):
    """lod, coef, rank, rss0, n_used and perm_max against the least-squares fit; the same bits with column tiles of 16, on a
    second call and from device rows"""
    import torch
    origin, pheno, cov, use, perm = make_case(n, T, P, K, mask, skipped)
    cs = chromstarts_of(CHROM_LENS)
    ref = reference_scan(origin, cs, pheno, use, cov, perm, additive)
    compared_markers(ref, cs, additive)          # the conditions of the comparison, on the reference, before anything runs
    ctx, _, _ = map_context(capi, CHROM_LENS)
    got = ctx.qtl_scan(origin, pheno, cov=cov, use=use, perm=perm, additive=additive)
    compare(got, ref, cs, additive, "n %d T %d P %d K %d" % (n, T, P, K))
    assert (got["perm_max"] is None) == (P == 0)
    same_bits(got, ctx.qtl_scan(origin, pheno, cov=cov, use=use, perm=perm, additive=additive))
    ctx.set_qtl_columns(16)
    same_bits(got, ctx.qtl_scan(origin, pheno, cov=cov, use=use, perm=perm, additive=additive))
    ctx.set_qtl_columns(0)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan_device(n, d_o.data_ptr(), pheno, cov=cov, use=use, perm=perm, additive=additive))
    ctx.close()


# ------------------------------------------------------------------------------------- 2. degenerate markers
def certain_rows(classes):
    """origin[n][M][4] with every individual certain of its class"""
    k = np.asarray(classes)
    o = np.zeros(k.shape + (4,))
    np.put_along_axis(o, k[..., None], 1.0, axis=2)
    return o


def test_degenerate_designs(capi):
    """one map of four chromosomes of 3 markers: [0] rows without information, [1] everybody certain and homozygous, [2] a
    chromosome with n_c < K + 4, [3] ordinary rows"""
    lens, n = (3, 3, 3, 3), 12
    origin, _ = soft_rows(n, lens, 5)
    origin[:, 0:3] = 0.25
    origin[:, 3:6] = certain_rows(np.where(synth.uniform(3, np.arange(n * 3)).reshape(n, 3) < 0.5, 0, 3))
    origin[3:, 6:9] = 0.0                                    # three individuals left on chromosome 2
    pheno = noise(n, 2, 4)
    cs = chromstarts_of(lens)
    ref = reference_scan(origin, cs, pheno)
    assert list(ref["rank"]) == [0] * 3 + [1] * 3 + [0] * 3 + [2] * 3 and list(ref["usable"]) == [True, True, False, True]
    ctx, _, _ = map_context(capi, lens)
    got = ctx.qtl_scan(origin, pheno)
    compare(got, ref, cs, what="degenerate designs", share=0)
    assert list(got["n_used"]) == [12, 12, 3, 12]
    assert np.all(got["lod"][:, 0:3] == 0.0) and np.isnan(got["coef"][:, 0:3]).all()          # rank 0: exactly 0
    assert np.isfinite(got["coef"][:, 3:6, 0]).all() and np.isnan(got["coef"][:, 3:6, 1]).all() and np.all(got["lod"][:, 3:6] > 0)
    assert np.all(got["lod"][:, 6:9] == 0.0) and np.isnan(got["coef"][:, 6:9]).all()          # n_c < K + 4
    # the additive model on the same rows: the dominance column is dropped everywhere
    add = ctx.qtl_scan(origin, pheno, additive=True)
    assert list(add["rank"]) == [0] * 3 + [1] * 3 + [0] * 3 + [1] * 3 and np.isnan(add["coef"][:, :, 1]).all()
    assert np.array_equal(add["lod"][:, 3:6], got["lod"][:, 3:6])
    ctx.close()


def test_constant_and_exactly_linear_phenotypes(capi):
    """16 certain individuals, 4 AA, 4 BB, 8 heterozygous: every sum of the model is a small dyadic number, so both cases
    are exact.  A constant phenotype has RSS0 = 0: lod 0, coef NaN.  y = 1 + 2 a has dRSS = RSS0 = 32: the clamp's value"""
    k = np.array([0] * 4 + [3] * 4 + [1] * 4 + [2] * 4)
    origin = certain_rows(np.stack([k, np.roll(k, 1)], axis=1))              # two markers, one chromosome
    a = origin[:, 0, 3] - origin[:, 0, 0]
    pheno = np.stack([np.full(16, 2.0), 1.0 + 2.0 * a], axis=1)
    ctx, _, _ = map_context(capi, (2,))
    got = ctx.qtl_scan(origin, pheno)
    ctx.close()
    assert list(got["rank"]) == [2, 2] and list(got["rss0"][:, 0]) == [0.0, 32.0]
    assert np.all(got["lod"][0] == 0.0) and np.isnan(got["coef"][0]).all()
    clamp = 0.5 * 16 * np.log10(32.0 / (32.0 - 32.0 * CLAMP))
    print("clamped lod %.12f, expected %.12f" % (got["lod"][1, 0], clamp))
    assert np.isfinite(got["lod"]).all() and abs(got["lod"][1, 0] - clamp) <= ATOL
    assert list(got["coef"][1, 0]) == [2.0, 0.0]
    assert 0.0 <= got["lod"][1, 1] < clamp


# ------------------------------------------------------------------------------------- 3. permutations
def test_identity_permutation_and_refusals(capi):
    n, T = 17, 3
    origin, pheno, _, _, _ = make_case(n, T, 0, 0, False, False)
    use = np.ones(n, bool)
    use[4] = False
    cs = chromstarts_of(CHROM_LENS)
    ctx, _, _ = map_context(capi, CHROM_LENS)
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3, use=use)[0], ident])
    got = ctx.qtl_scan(origin, pheno, use=use, perm=perm)
    observed = np.stack([got["lod"][:, cs[c]:cs[c + 1]].max(axis=1) for c in range(len(cs) - 1)], axis=1)
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed)
    # refused, with the outputs left alone: a permutation that moves an unused individual, a row that is no permutation,
    # a phenotype that is used and not finite, too many covariates
    moved = ident.copy()
    moved[[4, 5]] = [5, 4]
    twice = ident.copy()
    twice[3] = 2
    holed = pheno.copy()
    holed[6, 1] = np.nan
    for kw in (dict(pheno=pheno, perm=moved[None]), dict(pheno=pheno, perm=twice[None]), dict(pheno=holed, perm=ident[None]),
               dict(pheno=pheno, perm=ident[None], cov=np.zeros((n, 9)))):
        out = {k: np.full_like(v, 77) for k, v in got.items()}
        out["perm_max"] = np.full((1, T, len(cs) - 1), 77.0)
        with pytest.raises(capi.Cnf2Error):
            ctx._qtl_call(n, origin.ctypes.data_as(capi.C.c_void_p), kw["pheno"], kw.get("cov"), use, kw["perm"], 0, out=out)
        assert all(np.all(v == 77) for v in out.values())
    ctx.close()


# ------------------------------------------------------------------------------------- 4. through the sweep
def sweep_peds():
    return [("f2", synth.make_f2(24, 17, 2, seed=7)),
            ("outbred3", synth.make_outbred3(3, 4, 9, 2, seed=5, missing=0.2, random_hw=True, random_sure=True))]


@pytest.mark.parametrize("which", [0, 1])
def test_sweep_qtl(capi, which):
    import torch
    name, ped = sweep_peds()[which]
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    T, P, K = 2, 3, 1
    cov = synth.uniform(21, np.arange(n * K)).reshape(n, K)
    use = np.ones(n, bool)
    use[2] = False
    perm = qtl.permutations(n, P, 9, use=use)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = ctx.sweep_origins()["origin"]
    a = rows[:, :, 3] - rows[:, :, 0]
    pheno = np.stack([a[:, 4], a[:, M - 3]], axis=1) + noise(n, T, 8)
    got = ctx.sweep_qtl(pheno, cov=cov, use=use, perm=perm)
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(got["factors"], plain["factors"]) and np.array_equal(got["loglik"], plain["loglik"])
    # the reference on the product's own rows
    ref = reference_scan(rows, ped.chromstarts, pheno, use, cov, perm)
    compare(got, ref, ped.chromstarts, what="sweep_qtl " + name)
    # sweep_origins with device rows, then the scan on them: the same bits
    dev = torch.device("cuda", 0)
    t = lambda *shape, dtype=torch.float64: torch.full(shape, 77, dtype=dtype, device=dev)
    d_f, d_l, d_o, d_s, d_c = t(n, C, 8), t(n, C), t(n, M, 4), t(M, 4), t(C, dtype=torch.int32)
    ctx.sweep_origins_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_o.data_ptr(), None, d_s.data_ptr(), d_c.data_ptr())
    ctx.sync()
    same_bits(got, ctx.qtl_scan_device(n, d_o.data_ptr(), pheno, cov=cov, use=use, perm=perm))
    # device outputs
    d = dict(lod=t(T, M), coef=t(T, M, 2), rank=t(M, dtype=torch.int32), rss0=t(T, C), n_used=t(C, dtype=torch.int32),
             perm_max=t(P, T, C))
    ctx.sweep_qtl_device(0, n, d_f.data_ptr(), d_l.data_ptr(), pheno, cov, use, perm, *[d[k].data_ptr() for k in OUT_KEYS])
    ctx.sync()
    same_bits(got, {k: v.cpu().numpy() for k, v in d.items()})
    assert np.array_equal(d_f.cpu().numpy(), plain["factors"]) and np.array_equal(d_l.cpu().numpy(), plain["loglik"])
    # the column cap and the batch cap change nothing
    ctx.set_qtl_columns(3)
    ctx.set_batch_jobs(5)
    same_bits(got, ctx.sweep_qtl(pheno, cov=cov, use=use, perm=perm))
    ctx.set_qtl_columns(0)
    ctx.set_batch_jobs(0)
    # the rows that call left in the context: the same bits without a second sweep, and other traits on them
    same_bits(got, ctx.qtl_scan_device(n, None, pheno, cov=cov, use=use, perm=perm))
    other = pheno[:, ::-1] * 2.0 + 1.0
    same_bits(ctx.qtl_scan_device(n, d_o.data_ptr(), other, use=use, additive=True), ctx.qtl_scan_device(n, None, other, use=use, additive=True))
    # ... refused (CNF2_ERR_STATE, -3) for another n, and once an upload or another call has used the buffer

    def kept_is_refused(k=n):
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
            ctx.qtl_scan_device(k, None, pheno[:k], cov=cov[:k], use=use[:k], perm=None)
    kept_is_refused(n - 1)
    for spoil in (lambda: ctx.upload_map(ped.pos, ped.chromstarts), lambda: ctx.sweep_origins(),
                  lambda: ctx.qtl_scan(rows, pheno), lambda: ctx.upload_rows(ped.allele, ped.sure, ped.hw),
                  lambda: ctx.upload_pedigree(ped.par, ped.empty, ped.gen, ped.row_of, ped.dous)):
        same_bits(got, ctx.sweep_qtl(pheno, cov=cov, use=use, perm=perm))
        ctx.qtl_scan_device(n, None, pheno, use=use)
        spoil()
        kept_is_refused()
    fresh = capi.Context(0)
    fresh.upload_map(ped.pos, ped.chromstarts)
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        fresh.qtl_scan_device(n, None, pheno, use=use)
    fresh.close()
    # bad arguments leave the device buffers alone
    for x in list(d.values()) + [d_f, d_l]:
        x.fill_(77)
    bad_perm = perm.copy()
    bad_perm[0, [2, 3]] = perm[0, [3, 2]]                     # still a permutation; individual 3, used, gets the unused 2
    bad_pheno = pheno.copy()
    bad_pheno[5, 0] = np.inf
    longer = (np.concatenate([pheno, pheno[:1]]), np.concatenate([cov, cov[:1]]), np.append(use, True),
              np.concatenate([perm, np.full((P, 1), n, np.int32)], axis=1))
    for args in ((0, n, pheno, cov, use, bad_perm), (0, n, bad_pheno, cov, use, perm), (0, n + 1) + longer,
                 (3, 3, pheno[:0], cov[:0], use[:0], perm[:, :0]), (0, n, pheno, np.where(use[:, None], np.nan, cov), use, perm)):
        b, e, ph, cv, us, pm = args
        with pytest.raises(capi.Cnf2Error):
            ctx.sweep_qtl_device(b, e, d_f.data_ptr(), d_l.data_ptr(), ph, cv, us, pm, *[d[k].data_ptr() for k in OUT_KEYS])
        ctx.sync()
        assert all(bool((x == 77).all()) for x in list(d.values()) + [d_f, d_l])
    ctx.close()


# ------------------------------------------------------------------------------------- 5. a planted QTL
def test_planted_qtl(capi):
    """An F2 of 200 with an additive effect of the true genotype at one marker of chromosome 0: the peak lies on that
    chromosome with the planted marker inside its support interval -- by the reference first -- above the 5 % genome-wide
    threshold of 200 permutations, and no marker of the other chromosome is"""
    ped = synth.make_f2(200, 30, 2, seed=7)
    n, M = len(ped.dous), ped.n_markers
    planted = 11
    truth = ped.allele[3:, planted, :].astype(np.float64).sum(axis=1) - 3.0          # -1, 0, 1 = AA, AB, BB (no missing data)
    assert set(np.unique(truth)) == {-1.0, 0.0, 1.0}
    pheno = (0.6 * truth + 2.0 * noise(n, 1, 31)[:, 0])[:, None]
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = ctx.sweep_origins()["origin"]
    ref = reference_scan(rows, ped.chromstarts, pheno)
    ref_peaks = qtl.peaks(ref["lod"][0], ped.pos, ped.chromstarts, 3.0)
    assert [p["chrom"] for p in ref_peaks] == [0] and ref_peaks[0]["lo"] <= planted <= ref_peaks[0]["hi"], ref_peaks
    got = qtl.scan(ctx, pheno, permutations=200, seed=5)
    ctx.close()
    assert np.abs(got["lod"] - ref["lod"][0]).max() <= ATOL
    thr = qtl.thresholds(got["perm_max"])
    t5 = thr["genome"][0]
    print("peak %.2f at marker %d, 5 %% threshold %.2f, 1 %% %.2f" % (ref_peaks[0]["lod"], ref_peaks[0]["marker"], t5[0], thr["genome"][1][0]))
    # above the pointwise 5 % point of two degrees of freedom (LOD 1.3); a map of 2 x 100 cM stays far below 5
    assert 1.3 < t5[0] < 5.0 and thr["genome"][1][0] >= t5[0]
    found = qtl.peaks(got["lod"], ped.pos, ped.chromstarts, t5, coef=got["coef"])
    assert [p["chrom"] for p in found] == [0] and found[0]["lo"] <= planted <= found[0]["hi"]
    assert found[0]["marker"] == ref_peaks[0]["marker"] and found[0]["additive"] > 0.3
    cs = ped.chromstarts
    assert got["lod"][0, cs[1]:cs[2]].max() < t5[0]


# ------------------------------------------------------------------------------------- 6. command line
def test_cli_qtl(capi, tmp_path):
    """cnF2freq --qtl on the demo inputs with a phenotype file written here.  --output is the same bytes with and without
    it; the file parses; with --count 1 (the state the call sees is the readers' after postmarkerdata, which
    host.Run.from_files reaches through the same readers) its figures are qtl.scan's to the printed digits and its
    thresholds qtl.thresholds' for the same seed.  The demo analyses three individuals, fewer than K + 4: every LOD is 0 and
    every effect "-", which is what the file must say; the covariate, the missing value and the absent individual take the
    table through its paths."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    exe, demo = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq"), os.path.join(ROOT, "tests", "golden", "demo")
    files = [os.path.join(demo, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    ph = tmp_path / "pheno.txt"
    ph.write_text("id weight age height\nC 1.25 3 10\nA 9 9 9\nD 2.5 4 NA\n")             # F is absent; A is not analysed
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet"]
    qargs = ["--phenofile", str(ph), "--qtl-covariates", "age", "--qtl-permutations", "20", "--qtl-seed", "9"]
    out_a, out_b, q2, q1 = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "q2.txt", tmp_path / "q1.txt"
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    run("--count", "2", "--output", str(out_a))
    run("--count", "2", "--output", str(out_b), "--qtl", str(q2), *qargs)
    assert out_a.read_bytes() == out_b.read_bytes()
    run("--count", "1", "--output", str(out_b), "--qtl", str(q1), *qargs)
    pos = [float(v) for v in open(files[0]).read().split()]
    M, traits = len(pos), ["weight", "height"]

    def parse(path):
        blocks = path.read_text().split("\n\n")
        assert len(blocks) == 2
        rows = [ln.split("\t") for ln in blocks[0].split("\n")]
        assert len(rows) == M and all(len(r) == 4 + 3 * len(traits) for r in rows)
        assert all(int(r[0]) == 1 for r in rows) and [float(r[1]) for r in rows] == pos
        assert all(len(v.split(".")[1]) == 5 for r in rows for v in r[4:] if v != "-")
        num = lambda v: np.nan if v == "-" else float(v)
        lod = np.array([[float(r[4 + 3 * t]) for r in rows] for t in range(len(traits))])
        coef = np.array([[[num(r[5 + 3 * t]), num(r[6 + 3 * t])] for r in rows] for t in range(len(traits))])
        thr = [ln.split("\t") for ln in blocks[1].strip("\n").split("\n")]
        assert [r[0] for r in thr] == traits and all(len(r) == 3 for r in thr)
        return (np.array([int(r[2]) for r in rows]), np.array([int(r[3]) for r in rows]), lod, coef,
                np.array([[float(r[1]), float(r[2])] for r in thr]))

    parse(q2)
    n_used, rank, lod, coef, thr = parse(q1)
    r = host.Run.from_files(*files)
    assert (r.M, r.n_chrom, r.n_dous) == (M, 1, 3)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, [0, M], 3)
    pheno = np.array([[1.25, 10.0], [2.5, np.nan], [np.nan, np.nan]])                        # C, D, F
    use = np.array([True, True, False])
    want = qtl.scan(ctx, pheno, cov=np.array([3.0, 4.0, 0.0]), use=use, permutations=20, seed=9)
    ctx.close()
    r.close()
    wthr = qtl.thresholds(want["perm_max"])["genome"]
    print("file against qtl.scan: lod %.3g, thresholds %.3g" % (np.abs(lod - want["lod"]).max(), np.abs(thr - wthr.T).max()))
    assert np.array_equal(n_used, np.repeat(want["n_used"][0], M)) and np.array_equal(rank, want["rank"][0])
    np.testing.assert_allclose(lod, want["lod"], rtol=0, atol=0.51e-5)
    assert np.array_equal(np.isnan(coef), np.isnan(want["coef"]))
    np.testing.assert_allclose(thr, wthr.T, rtol=0, atol=0.51e-5)
    assert list(n_used) == [2] * M and np.all(lod == 0.0) and np.isnan(coef).all() and np.all(thr == 0.0)


def write_f2_files(ped, tmp_path):
    """an F2 of synth.make_f2 as PlantImpute files (map: positions, a chromosome starts where they fall; pedigree: name,
    parents, generation; genotypes: name and a dosage 0 / 1 / 2 per marker, 9 = missing); returns the paths and the names"""
    n = len(ped.dous)
    names = ["F2_%d" % i for i in range(n)]
    files = [tmp_path / ("f2." + e) for e in ("map", "ped", "gen")]
    files[0].write_text("".join("%r\n" % float(p) for p in ped.pos))
    files[1].write_text("A 0 0\nB 0 0\n" + "".join("%s A B 2\n" % nm for nm in names))
    dos = np.where(ped.allele.min(axis=2) == 0, 9, ped.allele.astype(int).sum(axis=2) - 2)
    files[2].write_text("".join("%s %s\n" % (nm, " ".join(str(v) for v in dos[r])) for nm, r in [("A", 1), ("B", 2)] + [(names[i], 3 + i) for i in range(n)]))
    return [str(f) for f in files], names


def test_cli_qtl_figures(capi, tmp_path):
    """The command line's figures on a cross that has some: an F2 of 14 on two chromosomes written to files, two traits with
    different missing values, a third with the first one's, a covariate that one individual lacks, an individual absent from
    the table, 25 permutations.  With --count 1 every LOD, effect, rank, n and threshold of the file is qtl.scan's on
    host.Run.from_files of the same files, to the printed digits."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    ped = synth.make_f2(14, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n, M, cs = 14, ped.n_markers, np.asarray(ped.chromstarts)
    truth = ped.allele[3:, 4, :].astype(np.float64).sum(axis=1) - 3.0
    y = np.stack([truth + noise(n, 1, 2)[:, 0], noise(n, 1, 3)[:, 0] * 4.0, -0.5 * truth + noise(n, 1, 4)[:, 0]], axis=1)
    y[3, 1] = y[8, 1] = np.nan                       # the second trait has its own pattern of missing values
    age = np.round(synth.uniform(5, np.arange(n)) * 10.0, 3)
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id w age h z"]
    for i in range(n):
        if i == 6:
            continue                                 # absent from the table: not used
        table.append("%s %s %s %s %s" % (names[i], cell(y[i, 0]), "-" if i == 11 else cell(age[i]), cell(y[i, 1]), cell(y[i, 2])))
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    q = tmp_path / "q.txt"
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    args = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--output",
            str(tmp_path / "out.txt"), "--qtl", str(q), "--qtl-covariates", "age", "--qtl-permutations", "25", "--qtl-seed", "4"]
    subprocess.run(args + ["--phenofile", str(ph)], capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    blocks = q.read_text().split("\n\n")
    rows = [ln.split("\t") for ln in blocks[0].split("\n")]
    assert len(rows) == M and all(len(r) == 4 + 9 for r in rows)
    assert [int(r[0]) for r in rows] == list(np.repeat([1, 2], np.diff(cs))) and np.allclose([float(r[1]) for r in rows], ped.pos, atol=0.51e-5)
    num = lambda v: np.nan if v == "-" else float(v)
    lod = np.array([[float(r[4 + 3 * t]) for r in rows] for t in range(3)])
    coef = np.array([[[num(r[5 + 3 * t]), num(r[6 + 3 * t])] for r in rows] for t in range(3)])
    thr = [ln.split("\t") for ln in blocks[1].strip("\n").split("\n")]
    assert [r[0] for r in thr] == ["w", "h", "z"]
    thr = np.array([[float(r[1]), float(r[2])] for r in thr])
    r = host.Run.from_files(*files)
    assert (r.M, r.n_chrom, r.n_dous) == (M, 2, n)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    use = np.ones(n, bool)
    use[[6, 11]] = False
    want = qtl.scan(ctx, y, cov=np.where(use, age, 0.0), use=use, permutations=25, seed=4)
    ctx.close()
    r.close()
    wthr = qtl.thresholds(want["perm_max"])["genome"].T
    print("file against qtl.scan: lod %.3g (largest %.2f), coef %.3g, thresholds %.3g (%s)" % (
        np.abs(lod - want["lod"]).max(), want["lod"].max(), np.nanmax(np.abs(coef - want["coef"])), np.abs(thr - wthr).max(), wthr.round(2).tolist()))
    assert list(want["n_used"][0]) == [12, 12] and list(want["n_used"][1]) == [10, 10] and want["lod"].max() > 1.0
    assert [int(x[2]) for x in rows] == [12] * M and np.array_equal([int(x[3]) for x in rows], want["rank"][0])
    np.testing.assert_allclose(lod, want["lod"], rtol=0, atol=0.51e-5)
    assert np.array_equal(np.isnan(coef), np.isnan(want["coef"])) and np.isfinite(coef).mean() > 0.9
    np.testing.assert_allclose(coef, want["coef"], rtol=0, atol=0.51e-5)
    np.testing.assert_allclose(thr, wthr, rtol=0, atol=0.51e-5)
    assert np.all(thr > 0.5) and len({tuple(t) for t in thr}) == 3, "every trait has thresholds of its own"
    # a covariate that is constant over the used individuals: the permutation test has no null model to take residuals
    # from, and the run ends with a message instead of thresholds of 0
    flat = tmp_path / "flat.txt"
    flat.write_text("\n".join([table[0]] + [" ".join(ln.split()[:2] + ["1"] + ln.split()[3:]) for ln in table[1:]]) + "\n")
    bad = subprocess.run(args + ["--phenofile", str(flat)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert bad.returncode != 0 and "has no full rank" in bad.stderr, bad.stderr[-300:]
