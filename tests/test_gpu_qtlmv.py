"""GPU suite: the multi-trait QTL scan (cnf2_qtl_scan_mv, cnf2_set_qtlmv_groups, Context.qtl_scan_mv / qtl_scan_mv_device,
qtl.scan_mv, cnF2freq --qtlmv).  The joint Wilks' lambda LOD on the origin rows against least-squares determinants in numpy
(tests/qtlmv_reference.py) at the shapes where the row map and the group tiling can go wrong, against the single scan for
T = 1, under the changes of the traits that must not matter, on degenerate designs, its refusals, on planted pleiotropy
and through the command line."""
import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, noise, soft_rows
from qtlmv_reference import CASES, case_reference, compare, conditions, make_case, reference_scan_mv

pytestmark = pytest.mark.gpu

KEYS = ("lod", "rank", "trait_rank", "n_used", "perm_max")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens):
    """a context that holds a map only: what cnf2_qtl_scan_mv needs"""
    cs = chromstarts_of(lens)
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in lens])
    ctx = capi.Context(0)
    ctx.upload_map(pos, cs)
    return ctx, cs


def same_bits(a, b):
    for k in KEYS:
        if a[k] is None:
            assert b[k] is None
        else:
            assert a[k].tobytes() == b[k].tobytes(), k


def device_outputs(M, C, P):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda *shape, dtype=torch.float64: torch.full(shape, 77, dtype=dtype, device=dev)
    return dict(lod=t(M), rank=t(M, dtype=torch.int32), trait_rank=t(C, dtype=torch.int32), n_used=t(C, dtype=torch.int32),
                perm_max=t(P, C) if P else None)


def pointers(d):
    return {k: (None if v is None else v.data_ptr()) for k, v in d.items()}


def host_copy(d):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}


# ------------------------------------------------------------------------------------- 1. the scan on hand-made rows
@pytest.mark.parametrize("case", CASES, ids=["n%d-T%d" % c[:2] for c in CASES])
def test_scan_on_hand_made_rows(capi, case):
    """lod, rank, trait_rank, n_used and perm_max against the determinants of least squares; the same bits with group tiles
    of 3, on a second call, from device rows and into device outputs"""
    import torch
    n, T, P, K, additive = case
    (origin, pheno, cov, use, perm), ref = case_reference(case)
    cs = chromstarts_of(CHROM_LENS)
    conditions(ref, cs, additive)                # on the reference alone, before anything runs
    ctx, _ = map_context(capi, CHROM_LENS)
    kw = dict(cov=cov, use=use, perm=perm, additive=additive)
    got = ctx.qtl_scan_mv(origin, pheno, **kw)
    compare(got, ref, "n %d T %d P %d K %d" % (n, T, P, K))
    assert (got["perm_max"] is None) == (P == 0)
    same_bits(got, ctx.qtl_scan_mv(origin, pheno, **kw))
    ctx.set_qtlmv_groups(3)
    same_bits(got, ctx.qtl_scan_mv(origin, pheno, **kw))
    ctx.set_qtlmv_groups(0)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan_mv_device(n, d_o.data_ptr(), pheno, **kw))
    d = device_outputs(origin.shape[1], len(CHROM_LENS), P)
    ctx.qtl_scan_mv_device(n, d_o.data_ptr(), pheno, d_out=pointers(d), **kw)
    ctx.sync()
    same_bits(got, host_copy(d))
    ctx.close()


# ------------------------------------------------------------------------------------- 2. one trait is the single scan
@pytest.mark.parametrize("n,P,K", [(5, 0, 0), (17, 6, 2), (67, 33, 0)])
def test_one_trait_is_the_single_scan(capi, n, P, K):
    origin, pheno, cov, use, perm = make_case(n, 1, P, K)
    cs = chromstarts_of(CHROM_LENS)
    ctx, _ = map_context(capi, CHROM_LENS)
    if P:
        perm[0] = np.arange(n)                                   # the identity among them
    one = ctx.qtl_scan(origin, pheno, cov=cov, use=use, perm=perm)
    got = ctx.qtl_scan_mv(origin, pheno, cov=cov, use=use, perm=perm)
    ctx.close()
    err_l = np.abs(got["lod"] - one["lod"][0]).max()
    err_p = np.abs(got["perm_max"] - one["perm_max"][:, 0]).max() if P else 0.0
    print("n %d P %d K %d against cnf2_qtl_scan: lod %.3g (largest %.2f), perm_max %.3g" % (n, P, K, err_l, one["lod"].max(), err_p))
    assert err_l <= ATOL and err_p <= ATOL and one["lod"].max() > 0.5
    assert np.array_equal(got["rank"], one["rank"]) and np.array_equal(got["n_used"], one["n_used"])
    assert np.array_equal(got["trait_rank"], (one["rss0"][0] > 0).astype(np.int32))
    if P:
        observed = np.array([got["lod"][cs[c]:cs[c + 1]].max() for c in range(len(cs) - 1)])
        assert got["perm_max"][0].tobytes() == observed.tobytes()
        assert not np.array_equal(got["perm_max"][1], observed)


# ------------------------------------------------------------------------------------- 3. what must not matter
def test_invariances(capi):
    """Y -> Y B + 3 with B = 2 I + 0.25 (strict upper triangle), the traits in reversed order, a covariate shifted and
    rescaled: the statistic is the same, held to ATOL against the base result"""
    case = CASES[4]
    n, T, P, K, additive = case
    (origin, pheno, cov, use, perm), ref = case_reference(case)
    conditions(ref, chromstarts_of(CHROM_LENS), additive)
    ctx, _ = map_context(capi, CHROM_LENS)
    base = ctx.qtl_scan_mv(origin, pheno, cov=cov, use=use, perm=perm)
    B = 2.0 * np.eye(T) + 0.25 * np.triu(np.ones((T, T)), 1)
    cov2 = cov.copy()
    cov2[:, 0] = 1000.0 + 64.0 * cov[:, 0]
    for what, y, z in (("Y B + 3", pheno @ B + 3.0, cov), ("reversed traits", pheno[:, ::-1], cov), ("covariate units", pheno, cov2)):
        got = ctx.qtl_scan_mv(origin, y, cov=z, use=use, perm=perm)
        err_l, err_p = np.abs(got["lod"] - base["lod"]).max(), np.abs(got["perm_max"] - base["perm_max"]).max()
        print("%s: lod %.3g, perm_max %.3g" % (what, err_l, err_p))
        assert err_l <= ATOL and err_p <= ATOL
        for k in ("rank", "trait_rank", "n_used"):
            assert np.array_equal(got[k], base[k]), (what, k)
    ctx.close()


# ------------------------------------------------------------------------------------- 4. degenerate designs
def certain_rows(classes):
    """origin[n][M][4] with every individual certain of its class"""
    k = np.asarray(classes)
    o = np.zeros(k.shape + (4,))
    np.put_along_axis(o, k[..., None], 1.0, axis=2)
    return o


def test_degenerate_traits(capi):
    """a copy of a trait and a constant trait are dropped and leave the LOD of the scan without them; only constant traits:
    every LOD exactly 0"""
    n, T, P, K = 64, 5, 3, 0
    origin, pheno, cov, use, perm = make_case(n, T, P, K)
    C = len(CHROM_LENS)
    ctx, _ = map_context(capi, CHROM_LENS)
    without = ctx.qtl_scan_mv(origin, pheno[:, [0, 1, 2, 4]], use=use, perm=perm)
    assert list(without["trait_rank"]) == [4] * C and without["lod"].max() > 1.0
    copied = pheno.copy()
    copied[:, 3] = copied[:, 1]
    flat = pheno.copy()
    flat[:, 3] = 7.0
    for what, y in (("trait 3 a copy of trait 1", copied), ("trait 3 constant", flat)):
        got = ctx.qtl_scan_mv(origin, y, use=use, perm=perm)
        err_l, err_p = np.abs(got["lod"] - without["lod"]).max(), np.abs(got["perm_max"] - without["perm_max"]).max()
        print("%s: lod %.3g, perm_max %.3g against the scan without it" % (what, err_l, err_p))
        assert list(got["trait_rank"]) == [T - 1] * C and np.array_equal(got["rank"], without["rank"])
        assert err_l <= ATOL and err_p <= ATOL
    ref = reference_scan_mv(origin, chromstarts_of(CHROM_LENS), copied, use, None, perm)
    assert list(ref["trait_rank"]) == [T - 1] * C and np.abs(ref["lod"][0] - without["lod"]).max() <= ATOL
    const = np.where(np.isfinite(pheno), np.arange(1.0, T + 1.0)[None, :], np.nan)
    got = ctx.qtl_scan_mv(origin, const, use=use, perm=perm)
    ctx.close()
    assert np.all(got["lod"] == 0.0) and np.all(got["perm_max"] == 0.0) and np.all(got["trait_rank"] == 0) and np.all(got["rank"] == 0)
    assert np.array_equal(got["n_used"], without["n_used"])


def test_degenerate_designs(capi):
    """one map of four chromosomes of 3 markers: [0] rows without information, [1] everybody certain and homozygous, [2] a
    chromosome with K + 4 <= n_c < K + 3 + T, which the single scan fits and this one does not, [3] ordinary rows"""
    lens, n, T = (3, 3, 3, 3), 12, 3
    origin, _ = soft_rows(n, lens, 5)
    origin[:, 0:3] = 0.25
    origin[:, 3:6] = certain_rows(np.where(synth.uniform(3, np.arange(n * 3)).reshape(n, 3) < 0.5, 0, 3))
    origin[5:, 6:9] = 0.0                                    # five individuals left on chromosome 2: K + 3 + T = 6
    pheno = noise(n, T, 4)
    cs = chromstarts_of(lens)
    ref = reference_scan_mv(origin, cs, pheno)
    assert list(ref["rank"]) == [0] * 3 + [1] * 3 + [0] * 3 + [2] * 3 and list(ref["trait_rank"]) == [3, 3, 0, 3]
    ctx, _ = map_context(capi, lens)
    got = ctx.qtl_scan_mv(origin, pheno)
    compare(got, ref, "degenerate designs")
    assert list(got["n_used"]) == [12, 12, 5, 12]
    assert np.all(got["lod"][0:3] == 0.0) and np.all(got["lod"][3:6] > 0) and np.all(got["lod"][6:9] == 0.0) and np.all(got["lod"][9:] > 0)
    assert np.all(ctx.qtl_scan(origin, pheno)["lod"][:, 6:9] > 0)          # the single scan fits chromosome 2
    add = ctx.qtl_scan_mv(origin, pheno, additive=True)
    assert list(add["rank"]) == [0] * 3 + [1] * 3 + [0] * 3 + [1] * 3 and np.array_equal(add["lod"][3:6], got["lod"][3:6])
    ctx.close()


def test_exactly_linear_trait(capi):
    """16 certain individuals, 4 AA, 4 BB, 8 heterozygous, y = 1 + 2 a: every sum is a small dyadic number, Lambda is exactly
    0 and the LOD the clamp's 8 log10(2^52)"""
    k = np.array([0] * 4 + [3] * 4 + [1] * 4 + [2] * 4)
    origin = certain_rows(np.stack([k, np.roll(k, 1)], axis=1))              # two markers, one chromosome
    a = origin[:, 0, 3] - origin[:, 0, 0]
    ctx, _ = map_context(capi, (2,))
    got = ctx.qtl_scan_mv(origin, 1.0 + 2.0 * a)
    ctx.close()
    clamp = 8.0 * np.log10(2.0 ** 52)
    print("clamped lod %.12f, expected %.12f" % (got["lod"][0], clamp))
    assert list(got["rank"]) == [2, 2] and list(got["trait_rank"]) == [1]
    assert abs(got["lod"][0] - clamp) <= ATOL and 0.0 <= got["lod"][1] < clamp


# ------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_outputs_alone(capi):
    import torch
    n, T, P = 17, 3, 1
    origin, pheno, _, use, _ = make_case(n, T, 0, 0)
    use = use.copy()
    use[4] = False                                              # (beside individual 2, which carries NaN)
    M, C = origin.shape[1], len(CHROM_LENS)
    ctx, _ = map_context(capi, CHROM_LENS)
    d_o = torch.from_numpy(origin).cuda()
    ident = np.arange(n, dtype=np.int32)
    moved = ident.copy()
    moved[[4, 5]] = [5, 4]
    twice = ident.copy()
    twice[3] = 2
    holed = pheno.copy()
    holed[6, 1] = np.nan
    assert ctx.qtl_scan_mv(origin, pheno, use=use, perm=ident[None])["lod"].max() > 0.0
    for what, kw in (("T = 17", dict(pheno=np.tile(pheno, (1, 6))[:, :17], perm=ident[None])),
                     ("nine covariates", dict(pheno=pheno, perm=ident[None], cov=noise(n, 9, 3))),
                     ("not a permutation", dict(pheno=pheno, perm=twice[None])),
                     ("an unused individual moved", dict(pheno=pheno, perm=moved[None])),
                     ("a phenotype not finite", dict(pheno=holed, perm=ident[None]))):
        out = dict(lod=np.full(M, 77.0), rank=np.full(M, 77, np.int32), trait_rank=np.full(C, 77, np.int32),
                   n_used=np.full(C, 77, np.int32), perm_max=np.full((P, C), 77.0))
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_mv(origin, kw["pheno"], cov=kw.get("cov"), use=use, perm=kw["perm"], out=out)
        assert all(np.all(v == 77) for v in out.values()), what
        d = device_outputs(M, C, P)
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_mv_device(n, d_o.data_ptr(), kw["pheno"], cov=kw.get("cov"), use=use, perm=kw["perm"], d_out=pointers(d))
        ctx.sync()
        assert all(bool((v == 77).all()) for v in d.values()), what
    ctx.close()
    # the rows a sweep_qtl left: the same bits as from the caller's; of another n: CNF2_ERR_STATE, outputs left alone
    ped = synth.make_f2(24, 17, 2, seed=7)
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    y = noise(n, 3, 8)
    ctx = capi.Context(0)
    ctx.upload(ped)
    ctx.sweep_qtl(y[:, :1])
    rows = ctx.sweep_origins()["origin"]
    ctx.sweep_qtl(y[:, :1])
    kept = ctx.qtl_scan_mv_device(n, None, y)
    same_bits(kept, ctx.qtl_scan_mv_device(n, None, y))                      # ... which the call leaves valid
    d = device_outputs(M, C, 0)
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_mv_device(n - 1, None, y[:n - 1], d_out=pointers(d))
    ctx.sync()
    assert all(bool((v == 77).all()) for v in d.values() if v is not None)
    same_bits(kept, ctx.qtl_scan_mv(rows, y))
    ctx.close()


# ------------------------------------------------------------------------------------- 6. planted pleiotropy
def test_planted_pleiotropy(capi):
    """An F2 of 200 and four traits, each with an additive effect of 0.5 of the true genotype at marker 11 of chromosome 0
    beside uniform noise of width 2 (an effect of 0.43 residual standard deviations: about 9 % of a trait's variance).  The
    reference alone first: the only joint peak above LOD 5 -- P(chi2 with 8 d.f. > 2 ln 10 x 5) = 0.003 pointwise -- lies on
    chromosome 0 with the planted marker inside its 1.5-LOD interval.  Then qtl.scan_mv agrees, the peak clears the 5 %
    genome-wide threshold of 200 permutations, and no marker of the other chromosome does."""
    ped = synth.make_f2(200, 30, 2, seed=7)
    n, planted, effect = len(ped.dous), 11, 0.5
    truth = ped.allele[3:, planted, :].astype(np.float64).sum(axis=1) - 3.0          # -1, 0, 1 = AA, AB, BB (no missing data)
    assert set(np.unique(truth)) == {-1.0, 0.0, 1.0}
    pheno = effect * truth[:, None] + 2.0 * noise(n, 4, 31)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = ctx.sweep_origins()["origin"]
    ref = reference_scan_mv(rows, ped.chromstarts, pheno)
    ref_peaks = qtl.peaks(ref["lod"][0], ped.pos, ped.chromstarts, 5.0)
    assert [p["chrom"] for p in ref_peaks] == [0] and ref_peaks[0]["lo"] <= planted <= ref_peaks[0]["hi"], ref_peaks
    got = qtl.scan_mv(ctx, pheno, permutations=200, seed=5)
    single = qtl.scan(ctx, pheno)
    ctx.close()
    assert np.abs(got["lod"] - ref["lod"][0]).max() <= ATOL
    assert got["perm_max"].shape == (200, 1, 2)
    thr = qtl.thresholds(got["perm_max"])
    t5 = thr["genome"][0]
    print("joint peak %.2f at marker %d (single traits at most %.2f), 5 %% threshold %.2f, 1 %% %.2f" %
          (ref_peaks[0]["lod"], ref_peaks[0]["marker"], single["lod"].max(), t5[0], thr["genome"][1][0]))
    # above the pointwise 5 % point of eight degrees of freedom (LOD 3.4); a map of 2 x 100 cM stays far below 8
    assert 3.4 < t5[0] < 8.0 and thr["genome"][1][0] >= t5[0]
    found = qtl.peaks(got["lod"], ped.pos, ped.chromstarts, t5)
    assert [p["chrom"] for p in found] == [0] and found[0]["lo"] <= planted <= found[0]["hi"]
    assert found[0]["marker"] == ref_peaks[0]["marker"] and found[0]["lod"] > single["lod"].max()
    cs = ped.chromstarts
    assert got["lod"][cs[1]:cs[2]].max() < t5[0]


# ------------------------------------------------------------------------------------- 7. command line
def test_cli_qtlmv(capi, tmp_path):
    """cnF2freq --qtlmv on an F2 of 14 on two chromosomes written to files: three traits, one of them with a missing value, a
    covariate that one individual lacks, an individual absent from the table, --qtl-traits choosing two, 25 permutations.
    With --count 1 every LOD, rank and threshold of the file is qtl.scan_mv's on host.Run.from_files of the same files, to the
    printed digits; without --qtl-traits all three traits are scanned.  The usage errors are refused."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    from test_gpu_qtl import write_f2_files
    ped = synth.make_f2(14, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n, M, cs = 14, ped.n_markers, np.asarray(ped.chromstarts)
    truth = ped.allele[3:, 4, :].astype(np.float64).sum(axis=1) - 3.0
    y = np.stack([truth + noise(n, 1, 2)[:, 0], noise(n, 1, 3)[:, 0] * 4.0, -0.5 * truth + noise(n, 1, 4)[:, 0]], axis=1)
    y[3, 2] = np.nan                                 # the third trait lacks a value: individual 3 is no complete case with it
    age = np.round(synth.uniform(5, np.arange(n)) * 10.0, 3)
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id w age h z"]
    for i in range(n):
        if i == 6:
            continue                                 # absent from the table: not used
        table.append("%s %s %s %s %s" % (names[i], cell(y[i, 0]), "-" if i == 11 else cell(age[i]), cell(y[i, 1]), cell(y[i, 2])))
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--output",
            str(tmp_path / "out.txt"), "--phenofile", str(ph), "--qtl-covariates", "age", "--qtl-permutations", "25", "--qtl-seed", "4"]

    def run_and_parse(name, *extra):
        q = tmp_path / name
        subprocess.run(base + ["--qtlmv", str(q), *extra], capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
        blocks = q.read_text().split("\n\n")
        assert len(blocks) == 2
        rows = [ln.split("\t") for ln in blocks[0].split("\n")]
        assert len(rows) == M and all(len(r) == 5 for r in rows) and [int(r[0]) for r in rows] == list(range(M))
        assert [int(r[1]) for r in rows] == list(np.repeat([1, 2], np.diff(cs))) and np.allclose([float(r[2]) for r in rows], ped.pos, atol=0.51e-5)
        assert all(len(r[3].split(".")[1]) == 5 for r in rows)
        thr = blocks[1].strip("\n").split("\t")
        assert thr[0] == "joint" and len(thr) == 3
        return np.array([float(r[3]) for r in rows]), np.array([int(r[4]) for r in rows]), np.array([float(thr[1]), float(thr[2])])

    two = run_and_parse("two.txt", "--qtl-traits", "w,h")
    three = run_and_parse("three.txt")
    r = host.Run.from_files(*files)
    assert (r.M, r.n_chrom, r.n_dous) == (M, 2, n)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    use = np.ones(n, bool)
    use[[6, 11]] = False
    for what, (lod, rank, thr), cols, n_used in (("w,h", two, [0, 1], 12), ("all traits", three, [0, 1, 2], 11)):
        want = qtl.scan_mv(ctx, y[:, cols], cov=np.where(use, age, 0.0), use=use, permutations=25, seed=4)
        wthr = qtl.thresholds(want["perm_max"])["genome"][:, 0]
        print("%s, file against qtl.scan_mv: lod %.3g (largest %.2f), thresholds %.3g (%s)" % (
            what, np.abs(lod - want["lod"]).max(), want["lod"].max(), np.abs(thr - wthr).max(), wthr.round(2).tolist()))
        assert list(want["n_used"]) == [n_used] * 2 and list(want["trait_rank"]) == [len(cols)] * 2 and want["lod"].max() > 1.0
        assert np.array_equal(rank, want["rank"])
        np.testing.assert_allclose(lod, want["lod"], rtol=0, atol=0.51e-5)
        np.testing.assert_allclose(thr, wthr, rtol=0, atol=0.51e-5)
        assert np.all(thr > 0.5)
    ctx.close()
    r.close()
    assert not np.array_equal(two[0], three[0])
    # usage errors: an absent trait, more than 16 traits
    wide = tmp_path / "wide.txt"
    wide.write_text("id " + " ".join("t%d" % t for t in range(17)) + "\n" + "".join(
        "%s %s\n" % (names[i], " ".join(repr(float(v)) for v in noise(17, 1, 40 + i)[:, 0])) for i in range(n)))
    for args, text in ((base + ["--qtlmv", "bad.txt", "--qtl-traits", "w,girth"], "--qtl-traits: the phenotype file has no trait girth"),
                       ([a if a != str(ph) else str(wide) for a in base[:-6]] + ["--qtlmv", "bad.txt"], "--qtlmv takes 1 .. 16 traits, not 17")):
        bad = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert bad.returncode == 2 and text in bad.stderr, bad.stderr[-300:]
        assert not (tmp_path / "bad.txt").exists()
