"""GPU suite: the bootstrap scan (cnf2_qtl_scan_boot, Context.qtl_scan_boot / qtl_scan_boot_device, qtl.scan_boot and
qtl.boot_interval).  The scan of resampled individuals in one call, checked against least squares on literally repeated rows
(tests/qtlboot_reference.py) at the smallest shapes that cross every edge of the kernel -- partial and several replicate
groups, n no multiple of 4, every instantiation by design width, model and trait chunk --, for its bits, its two properties,
its documented cells, its refusals, on the rows a sweep left in the context and on a planted QTL."""
import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, noise, soft_rows
from qtlboot_reference import CASES, case_reference, compare, conditions, reference_boot, sub_range

pytestmark = pytest.mark.gpu

KEYS = ("boot_max", "boot_arg", "n_boot", "boot_lod")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens):
    cs = chromstarts_of(lens)
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in lens])
    ctx = capi.Context(0)
    ctx.upload_map(pos, cs)
    return ctx, cs, pos


def same_bits(a, b, keys=KEYS):
    for k in keys:
        if a[k] is None or b[k] is None:
            continue
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------- 1. the cases of the issue
@pytest.mark.parametrize("case", CASES, ids=["n%d" % c[0] for c in CASES])
def test_boot_on_hand_made_rows(capi, case):
    """boot_lod, boot_max, boot_arg and n_boot against the resampled least-squares fit on the full range and on a sub-range
    with chrom_begin > 0; the same bits on a second call, without the profile and from device rows"""
    import torch
    n, T, K, B, additive, lens, seed = case
    (origin, pheno, cov, use, count), ref = case_reference(case)
    cs = chromstarts_of(lens)
    C = len(lens)
    compared = conditions(ref, K, additive, "n %d" % n)              # on the reference, before anything runs
    ctx, _, _ = map_context(capi, lens)
    kw = dict(cov=cov, use=use, additive=additive)
    got = ctx.qtl_scan_boot(origin, pheno, count, profile=True, **kw)
    compare(got, ref, compared, "n %d T %d K %d B %d" % (n, T, K, B))
    same_bits(got, ctx.qtl_scan_boot(origin, pheno, count, profile=True, **kw))
    lean = ctx.qtl_scan_boot(origin, pheno, count, **kw)
    assert lean["boot_lod"] is None
    same_bits(got, lean)
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan_boot_device(n, d_o.data_ptr(), pheno, count, profile=True, **kw))
    # a sub-range: the same cells, their markers still global indices
    c0, c1 = (1, 2) if C == 2 else (2, 5)
    part = ctx.qtl_scan_boot(origin, pheno, count, c0, c1, profile=True, **kw)
    rsub = sub_range(ref, cs, c0, c1)
    compare(part, rsub, compared[:, :, c0:c1], "n %d chromosomes %d .. %d" % (n, c0, c1 - 1))
    assert part["boot_arg"].min() >= cs[c0] and part["boot_arg"].max() < cs[c1]
    same_bits(part, dict(boot_max=got["boot_max"][:, :, c0:c1].copy(), boot_arg=got["boot_arg"][:, :, c0:c1].copy(),
                         n_boot=got["n_boot"][:, c0:c1].copy(), boot_lod=got["boot_lod"][:, :, cs[c0]:cs[c1]].copy()))
    ctx.close()


# The cases above run the instantiations (design width up to 2 / up to 9, full / additive, one trait / chunks of four)
# (2, full, 1), (9, full, 4), (2, additive, 4) and (9, full, 1).  The other four, and a T that takes two trait chunks:
#         n   T  K  B  additive lens      seed
EXTRA = [(40, 6, 0, 3, False, (17, 5), 21),        # (2, full, 4), chunks of 4 + 2
         (40, 5, 3, 3, True, (17, 5), 22),         # (9, additive, 4), chunks of 4 + 1
         (30, 1, 1, 3, True, (17, 5), 23),         # (2, additive, 1)
         (40, 1, 3, 3, True, (17, 5), 24)]         # (9, additive, 1)


@pytest.mark.parametrize("case", EXTRA, ids=["T%d-K%d-%s" % (c[1], c[2], "add" if c[4] else "full") for c in EXTRA])
def test_boot_every_instantiation_and_trait_chunks(capi, case):
    """the remaining instantiations against the reference; with more than four traits, to the bit what calls on subsets of
    the traits give, in which every trait falls into another chunk and another place of its chunk"""
    n, T, K, B, additive, lens, seed = case
    (origin, pheno, cov, use, count), ref = case_reference(case)
    compared = conditions(ref, K, additive, "extra n %d" % n)
    ctx, _, _ = map_context(capi, lens)
    kw = dict(cov=cov, use=use, additive=additive, profile=True)
    got = ctx.qtl_scan_boot(origin, pheno, count, **kw)
    compare(got, ref, compared, "extra T %d K %d" % (T, K))
    if T > 4:
        for lo, hi in ((4, T), (1, 5), (2, 4)):
            sub = ctx.qtl_scan_boot(origin, pheno[:, lo:hi], count, **kw)
            for k in ("boot_max", "boot_arg", "boot_lod"):
                assert sub[k].tobytes() == got[k][:, lo:hi].copy().tobytes(), (k, lo, hi)
    ctx.close()


# ------------------------------------------------------------------------------------- 2. properties
def test_counts_of_one_are_the_scan_and_doubled_counts_double_it(capi):
    case = CASES[1]
    n, T, K, B, additive, lens, seed = case
    (origin, pheno, cov, use, count), _ = case_reference(case)
    ctx, cs, _ = map_context(capi, lens)
    ones = use.astype(np.int32)[None, :]
    plain = ctx.qtl_scan(origin, pheno, cov=cov, use=use)
    got = ctx.qtl_scan_boot(origin, pheno, ones, cov=cov, use=use, profile=True)
    err = np.abs(got["boot_lod"][0] - plain["lod"]).max()
    print("counts of one against cnf2_qtl_scan: lod %.3g" % err)
    assert err <= ATOL and np.array_equal(got["n_boot"][0], plain["n_used"])
    for c in range(len(lens)):
        assert np.abs(got["boot_max"][0, :, c] - plain["lod"][:, cs[c]:cs[c + 1]].max(axis=1)).max() <= ATOL
    once = ctx.qtl_scan_boot(origin, pheno, count, cov=cov, use=use, profile=True)
    twice = ctx.qtl_scan_boot(origin, pheno, 2 * count, cov=cov, use=use, profile=True)
    err = np.abs(twice["boot_lod"] - 2.0 * once["boot_lod"]).max()
    print("doubled counts: lod %.3g" % err)
    assert err <= ATOL and np.abs(twice["boot_max"] - 2.0 * once["boot_max"]).max() <= ATOL
    assert np.array_equal(twice["boot_arg"], once["boot_arg"]) and np.array_equal(twice["n_boot"], 2 * once["n_boot"])
    ctx.close()


# ------------------------------------------------------------------------------------- 3. documented cells
def test_documented_cells(capi):
    """one call on a map of (1, 3, 3) markers, K = 1 with a binary covariate.  Replicate 0: everybody once; 1: all the weight
    on K + 3 individuals; 2: only individuals of one covariate class.  Chromosome 2 carries rows without information."""
    lens, n = (1, 3, 3), 24
    origin, _ = soft_rows(n, lens, 6)
    origin[:, 4:7] = 0.25
    pheno = 0.7 * (origin[:, 2, 3] - origin[:, 2, 0])[:, None] + noise(n, 1, 6)
    z = (np.arange(n) % 2).astype(np.float64)[:, None]
    count = np.ones((3, n), np.int32)
    count[1] = 0
    count[1, :4] = 1
    count[2] = np.where(np.arange(n) % 2 == 0, 2, 0)
    ctx, cs, _ = map_context(capi, lens)
    got = ctx.qtl_scan_boot(origin, pheno, count, cov=z, profile=True)
    ref = reference_boot(origin, cs, pheno, count, cov=z)
    assert list(ref["usable"][0]) == [True] * 3 and not ref["usable"][1:].any()
    assert np.array_equal(got["n_boot"], [[n] * 3, [4] * 3, [n] * 3])
    # not fitted: -1, 0 and a profile of zeros
    assert np.all(got["boot_arg"][1:] == -1) and np.all(got["boot_max"][1:] == 0.0) and np.all(got["boot_lod"][1:] == 0.0)
    # a single-marker chromosome gives that marker; an all-zero profile its chromosome's first marker
    assert got["boot_arg"][0, 0, 0] == 0 and got["boot_max"][0, 0, 0] == got["boot_lod"][0, 0, 0]
    assert np.all(got["boot_lod"][0, 0, 4:7] == 0.0) and got["boot_arg"][0, 0, 2] == 4 and got["boot_max"][0, 0, 2] == 0.0
    assert np.abs(got["boot_lod"][0] - ref["lod"][0]).max() <= ATOL
    assert got["boot_arg"][0, 0, 1] == ref["boot_arg"][0, 0, 1] and got["boot_max"][0, 0, 1] > 0.0
    ctx.close()


# ------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_outputs_untouched(capi):
    case = CASES[0]
    n, T, K, B, additive, lens, seed = case
    (origin, pheno, cov, use, count), _ = case_reference(case)
    ctx, cs, _ = map_context(capi, lens)
    M, C = int(cs[-1]), len(lens)
    fresh = lambda: dict(boot_max=np.full((B, T, C), 77.0), boot_arg=np.full((B, T, C), 77, np.int32),
                         n_boot=np.full((B, C), 77, np.int32), boot_lod=np.full((B, T, M), 77.0))
    mask = np.ones(n, bool)
    mask[2] = False
    neg = count.copy()
    neg[1, 3] = -1
    nan_y = pheno.copy()
    nan_y[5] = np.nan
    on_unused = count.copy()
    on_unused[:, 2] = 1
    wide = np.zeros((n, 9))
    bad = [dict(count=neg), dict(pheno=nan_y), dict(count=on_unused, use=mask), dict(cov=wide),
           dict(cov=np.full((n, 1), np.inf))]
    for b in bad:
        out = fresh()
        a = dict(pheno=pheno, count=count, cov=None, use=None)
        a.update(b)
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx.qtl_scan_boot(origin, a["pheno"], a["count"], cov=a["cov"], use=a["use"], out=out)
        assert all(np.all(v == 77) for v in out.values()), sorted(b)
    # through the library itself: the chromosome range, B = 0, NULL pointers
    import ctypes as Ct
    p = lambda a: a.ctypes.data_as(Ct.c_void_p)
    out = fresh()
    y, cnt = np.ascontiguousarray(pheno), np.ascontiguousarray(count, np.int32)
    outs = [p(out[k]) for k in KEYS]
    call = lambda o, ph, c0, c1, nb, ct, os: ctx.L.cnf2_qtl_scan_boot(ctx.h, n, o, T, ph, None, 0, None, c0, c1, nb, ct, *os, 0)
    for args in ((p(origin), p(y), 2, 2, B, p(cnt), outs), (p(origin), p(y), -1, 2, B, p(cnt), outs),
                 (p(origin), p(y), 0, C + 1, B, p(cnt), outs), (p(origin), p(y), 0, C, 0, p(cnt), outs),
                 (None, p(y), 0, C, B, p(cnt), outs), (p(origin), None, 0, C, B, p(cnt), outs),
                 (p(origin), p(y), 0, C, B, None, outs), (p(origin), p(y), 0, C, B, p(cnt), [None] + outs[1:]),
                 (p(origin), p(y), 0, C, B, p(cnt), outs[:2] + [None] + outs[3:])):
        assert call(*args) == -2
        assert all(np.all(v == 77) for v in out.values())
    assert call(p(origin), p(y), 0, C, B, p(cnt), outs[:3] + [None]) == 0            # (boot_lod alone may be NULL)
    ctx.close()


# ------------------------------------------------------------------------------------- 5. the rows a sweep left in the context
def test_context_rows(capi):
    ped = synth.make_f2(60, 20, 2, seed=7)
    n = len(ped.dous)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = ctx.sweep_origins()["origin"]
    pheno = (rows[:, 5, 3] - rows[:, 5, 0])[:, None] + noise(n, 1, 8)
    count = qtl.bootstrap_counts(n, 20, 3)
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_boot_device(n, None, pheno, count)
    swept = ctx.sweep_qtl(pheno)
    kept = ctx.qtl_scan_boot_device(n, None, pheno, count, profile=True)
    # ... which leaves the rows valid: again, and the scan itself on them
    ctx.qtl_scan_boot_device(n, None, pheno, count, 1, 2)
    same_bits(kept, ctx.qtl_scan_boot_device(n, None, pheno, count, profile=True))
    assert ctx.qtl_scan_device(n, None, pheno)["lod"].tobytes() == swept["lod"].tobytes()
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):
        ctx.qtl_scan_boot_device(n - 1, None, pheno[:-1], count[:, :-1])
    same_bits(kept, ctx.qtl_scan_boot(rows, pheno, count, profile=True))                 # the same rows from the host
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-3\)"):                          # ... which took the buffer
        ctx.qtl_scan_boot_device(n, None, pheno, count)
    # qtl.scan_boot: a sweep of its own, these counts, this result for each chromosome
    for chrom in (0, 1):
        full = qtl.scan_boot(ctx, pheno, chrom, replicates=20, seed=3, profile=True)
        assert np.array_equal(full["count"][0], count)
        cs = ped.chromstarts
        assert full["boot_max"].tobytes() == kept["boot_max"][:, :, chrom:chrom + 1].copy().tobytes()
        assert np.array_equal(full["boot_arg"], kept["boot_arg"][:, :, chrom:chrom + 1])
        assert full["boot_lod"].tobytes() == kept["boot_lod"][:, :, cs[chrom]:cs[chrom + 1]].copy().tobytes()
    both = qtl.scan_boot(ctx, pheno, (0, 2), replicates=20, seed=3)
    assert both["boot_max"].tobytes() == kept["boot_max"].tobytes() and both["boot_lod"] is None
    ctx.close()


# ------------------------------------------------------------------------------------- 6. a planted QTL
def test_planted_qtl_interval(capi):
    """soft_rows(67, CHROM_LENS, 3), an additive effect at marker 20 of the chromosome of 33, B = 200: the reference's 95 %
    interval holds the planted marker, and the product's interval is the same markers"""
    n, B, chrom = 67, 200, 5
    origin, _ = soft_rows(n, CHROM_LENS, 3)
    cs = chromstarts_of(CHROM_LENS)
    planted = int(cs[chrom]) + 20
    pheno = 0.35 * (origin[:, planted, 3] - origin[:, planted, 0])[:, None] + noise(n, 1, 3)
    count = qtl.bootstrap_counts(n, B, 3)
    ref = reference_boot(origin, cs, pheno, count, chrom_begin=chrom, chrom_end=chrom + 1)
    ctx, _, pos = map_context(capi, CHROM_LENS)
    want = qtl.boot_interval(ref["boot_arg"][:, 0, 0], pos)
    print("reference: markers %d .. %d of %d usable replicates, %.2f on the planted marker" %
          (want["lo"], want["hi"], want["V"], want["share"][planted]))
    assert want["V"] == B and want["lo"] <= planted <= want["hi"] and want["lo"] < want["hi"]
    assert ref["gap"].min() >= 1e-6 and ref["distinct"].min() >= 6          # every replicate has a clear best marker
    got = ctx.qtl_scan_boot(origin, pheno, count, chrom, chrom + 1)
    assert np.abs(got["boot_max"] - ref["boot_max"]).max() <= ATOL
    mine = qtl.boot_interval(got["boot_arg"][:, 0, 0], pos)
    assert (mine["lo"], mine["hi"], mine["V"]) == (want["lo"], want["hi"], want["V"])
    ctx.close()


# ------------------------------------------------------------------------------------- 7. command line
def write_f2_files(ped, tmp_path):
    """an F2 of synth.make_f2 as PlantImpute files (map, pedigree, genotypes as dosages with 9 = missing)"""
    n = len(ped.dous)
    names = ["F2_%d" % i for i in range(n)]
    files = [tmp_path / ("f2." + e) for e in ("map", "ped", "gen")]
    files[0].write_text("".join("%r\n" % float(p) for p in ped.pos))
    files[1].write_text("A 0 0\nB 0 0\n" + "".join("%s A B 2\n" % nm for nm in names))
    dos = np.where(ped.allele.min(axis=2) == 0, 9, ped.allele.astype(int).sum(axis=2) - 2)
    files[2].write_text("".join("%s %s\n" % (nm, " ".join(str(v) for v in dos[r])) for nm, r in [("A", 1), ("B", 2)] + [(names[i], 3 + i) for i in range(n)]))
    return [str(f) for f in files], names


def test_cli_qtlboot(capi, tmp_path):
    """cnF2freq --qtlboot on an F2 of 14 on two chromosomes written to files: two traits with different missing values, a
    covariate that one individual lacks, an individual absent from the table, 40 replicates on chromosome 2.  --output is the
    same bytes with and without it; the file parses; its peak is qtl.scan's, its interval, V and shares qtl.scan_boot's and
    qtl.boot_interval's on host.Run.from_files of the same files, to the printed digits."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    ped = synth.make_f2(14, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n, M, cs = 14, ped.n_markers, np.asarray(ped.chromstarts)
    truth = ped.allele[3:, cs[1] + 4, :].astype(np.float64).sum(axis=1) - 3.0
    y = np.stack([truth + noise(n, 1, 2)[:, 0], -0.5 * truth + noise(n, 1, 3)[:, 0] * 2.0], axis=1)
    y[3, 1] = y[8, 1] = np.nan
    age = np.round(synth.uniform(5, np.arange(n)) * 10.0, 3)
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id w age h"]
    for i in range(n):
        if i != 6:
            table.append("%s %s %s %s" % (names[i], cell(y[i, 0]), "-" if i == 11 else cell(age[i]), cell(y[i, 1])))
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1"]
    out_a, out_b, q = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "boot.txt"
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    run("--output", str(out_a))
    run("--output", str(out_b), "--qtlboot", str(q), "--phenofile", str(ph), "--qtl-covariates", "age", "--qtl-seed", "4",
        "--qtl-boot-chrom", "2", "--qtl-boot-replicates", "40")
    assert out_a.read_bytes() == out_b.read_bytes()
    blocks = q.read_text().split("\n\n")
    assert len(blocks) == 2
    head = [ln.split("\t") for ln in blocks[0].split("\n")]
    rows = [ln.split("\t") for ln in blocks[1].strip("\n").split("\n")]
    L = int(cs[2] - cs[1])
    assert [h[0] for h in head] == ["w", "h"] and all(len(h) == 8 for h in head)
    assert len(rows) == L and all(len(r) == 4 and int(r[0]) == 2 for r in rows)
    assert np.allclose([float(r[1]) for r in rows], ped.pos[cs[1]:cs[2]], atol=0.51e-5)
    assert all(len(v.split(".")[1]) == 5 for r in rows for v in r[1:])
    share = np.array([[float(r[2 + t]) for r in rows] for t in range(2)])
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    use = np.ones(n, bool)
    use[[6, 11]] = False
    cov = np.where(use, age, 0.0)
    want = qtl.scan_boot(ctx, y, 1, replicates=40, seed=4, cov=cov, use=use)
    plain = qtl.scan(ctx, y, cov=cov, use=use)
    ctx.close()
    r.close()
    for t in range(2):
        iv = qtl.boot_interval(want["boot_arg"][:, t, 0], ped.pos)
        assert iv["V"] > 0 and int(head[t][7]) == iv["V"]
        assert (int(head[t][5]), int(head[t][6])) == (iv["lo"], iv["hi"])
        assert np.allclose([float(head[t][3]), float(head[t][4])], [iv["pos_lo"], iv["pos_hi"]], rtol=0, atol=0.51e-5)
        np.testing.assert_allclose(share[t], iv["share"][cs[1]:cs[2]], rtol=0, atol=0.51e-5)
        assert np.all(iv["share"][:cs[1]] == 0.0)
        assert int(head[t][1]) == cs[1] + int(np.argmax(plain["lod"][t, cs[1]:cs[2]]))
        assert abs(float(head[t][2]) - ped.pos[int(head[t][1])]) <= 0.51e-5
    assert np.abs(share.sum(axis=1) - 1.0).max() < 1e-4 and not np.array_equal(share[0], share[1])
