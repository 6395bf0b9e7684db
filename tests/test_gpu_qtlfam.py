"""GPU suite: the within-family scan (cnf2_qtl_scan_fam, Context.qtl_scan_fam / qtl_scan_fam_device, families, scan_fam and
fam_fstat of cnf2freq_amd/qtl.py).  The nested half-sib model on the origin rows, checked against the dense least-squares
design of tests/qtlfam_reference.py on hand-made rows at the shapes where the gather list, the 4-slot step and the tiling can
go wrong, on degenerate designs, for its permutations and bookkeeping, against the column scan where the two models
coincide, and on a planted within-family QTL through the sweep."""
import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import CHROM_LENS, chromstarts_of, noise, skip, soft_rows
from qtlfam_reference import ATOL, CASES, SKIP_CHROM, compare, compared_markers, make_case, reference_scan, regressor, sized_families

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod", "df", "slope", "rss0", "n_used", "n_cells", "perm_max")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens):
    """a context that holds a map only: what cnf2_qtl_scan_fam needs"""
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
@pytest.mark.parametrize("T,P,K,side,fine,mask,skipped", CASES)
def test_scan_on_hand_made_rows(capi, T, P, K, side, fine, mask, skipped):
    """families of 1, 2, 3, 4, 5, 8 and 9 on the map CHROM_LENS: lod, df, slopes, rss0, n_used, n_cells and perm_max against
    the least-squares design; the same bits with column tiles of 16, on a second call, from device rows and into device
    outputs"""
    import torch
    origin, grp, cell, F, pheno, cov, use, perm = make_case(T, P, K, side, fine, mask, skipped)
    n = len(grp)
    cs = chromstarts_of(CHROM_LENS)
    ref = reference_scan(origin, cs, side, grp, cell, F, pheno, use, cov, perm)
    compared_markers(ref, cs)                    # the conditions of the comparison, on the reference, before anything runs
    ctx, _, _ = map_context(capi, CHROM_LENS)
    kw = dict(cell=cell, cov=cov, use=use, perm=perm, slopes=True)
    got = ctx.qtl_scan_fam(origin, side, grp, F, pheno, **kw)
    compare(got, ref, cs, "T %d P %d K %d side %d fine %d" % (T, P, K, side, fine))
    assert (got["perm_max"] is None) == (P == 0)
    assert not ref["fitted"][:, 0].any() and np.isnan(got["slope"][:, :, 0]).all()          # a family of one is never fitted
    if skipped:
        on = slice(cs[SKIP_CHROM], cs[SKIP_CHROM + 1])
        assert np.isnan(got["slope"][:, on, 1:3]).all() and np.isfinite(got["slope"][:, :cs[SKIP_CHROM], 2]).all()
        assert got["n_cells"][SKIP_CHROM] == got["n_cells"][0] - 1 and got["n_used"][SKIP_CHROM] == got["n_used"][0] - 4
    same_bits(got, ctx.qtl_scan_fam(origin, side, grp, F, pheno, **kw))
    ctx.set_qtl_columns(16)
    same_bits(got, ctx.qtl_scan_fam(origin, side, grp, F, pheno, **kw))
    ctx.set_qtl_columns(0)
    # without slopes everything else is the same
    bare = ctx.qtl_scan_fam(origin, side, grp, F, pheno, cell=cell, cov=cov, use=use, perm=perm)
    assert bare["slope"] is None
    same_bits(got, bare, [k for k in OUT_KEYS if k != "slope"])
    d_o = torch.from_numpy(origin).cuda()
    same_bits(got, ctx.qtl_scan_fam_device(n, d_o.data_ptr(), side, grp, F, pheno, **kw))
    # device outputs
    M, C = origin.shape[1], len(cs) - 1
    t = lambda *shape, dtype=torch.float64: torch.full(shape, 77, dtype=dtype, device="cuda")
    d = dict(lod=t(T, M), df=t(M, dtype=torch.int32), slope=t(T, M, F), rss0=t(T, C), n_used=t(C, dtype=torch.int32),
             n_cells=t(C, dtype=torch.int32), perm_max=t(P, T, C) if P else None)
    assert ctx.qtl_scan_fam_device(n, d_o.data_ptr(), side, grp, F, pheno, d_out={k: v.data_ptr() for k, v in d.items() if v is not None},
                                   **{k: v for k, v in kw.items() if k != "slopes"}) is None
    ctx.sync()
    same_bits(got, {k: None if v is None else v.cpu().numpy() for k, v in d.items()})
    ctx.close()


# ------------------------------------------------------------------------------------- 2. one family; the column scan
def test_one_family_is_the_column_scan(capi):
    """F = 1 with one cell and no covariate is the regression of y on [1, x]: the LOD of cnf2_qtl_scan_cols on the single
    regressor x with the null design of ones"""
    n, T = 21, 3
    origin, _ = soft_rows(n, CHROM_LENS, 40)
    cs = chromstarts_of(CHROM_LENS)
    pheno = regressor(origin, 0)[:, [5, 40, 70]] + noise(n, T, 2)
    grp = np.zeros(n, np.int32)
    ref = reference_scan(origin, cs, 0, grp, None, 1, pheno)
    ctx, _, _ = map_context(capi, CHROM_LENS)
    got = ctx.qtl_scan_fam(origin, 0, grp, 1, pheno, slopes=True)
    compare(got, ref, cs, "one family")
    assert np.all(got["df"] == 1) and list(got["n_cells"]) == [1] * len(CHROM_LENS)
    cols = ctx.qtl_scan_cols(regressor(origin, 0)[:, :, None], np.ones((n, 1)), pheno)
    ctx.close()
    err_l = np.abs(got["lod"] - cols["lod"]).max()
    err_s = (np.abs(got["slope"][:, :, 0] - cols["coef"][:, :, 0]) / np.maximum(1.0, np.abs(cols["coef"][:, :, 0]))).max()
    print("against cnf2_qtl_scan_cols: lod %.3g, slope %.3g" % (err_l, err_s))
    assert err_l <= ATOL and err_s <= ATOL


# ------------------------------------------------------------------------------------- 3. degenerate designs
def test_covariate_constant_within_cells(capi):
    """the covariate takes one value per cell but for two individuals, which are skipped on chromosome 2: there it is
    constant within every cell, S11 has no factor and the chromosome is not scanned; the others are"""
    lens = (3, 4, 3)
    grp, _ = sized_families((4, 5, 6))
    n = len(grp)
    origin, _ = soft_rows(n, lens, 8)
    movers = [np.flatnonzero(grp == 0)[1], np.flatnonzero(grp == 2)[3]]
    origin = skip(origin, movers, 2, lens)
    cov = (3.0 + grp).astype(np.float64)[:, None] / 7.0
    cov[movers, 0] += [0.5, -0.25]
    pheno = regressor(origin, 1)[:, [1, 5]] + noise(n, 2, 6)
    cs = chromstarts_of(lens)
    ref = reference_scan(origin, cs, 1, grp, None, 3, pheno, cov=cov)
    assert list(ref["scanned"]) == [True, True, False]
    ctx, _, _ = map_context(capi, lens)
    got = ctx.qtl_scan_fam(origin, 1, grp, 3, pheno, cov=cov, slopes=True)
    ctx.close()
    compare(got, ref, cs, "covariate constant within cells", share=0)
    on = slice(cs[2], cs[3])
    assert np.all(got["df"][on] == 0) and np.all(got["lod"][:, on] == 0.0) and np.isnan(got["slope"][:, on]).all()
    assert np.all(got["rss0"][:, 2] == 0.0) and np.all(got["df"][:cs[2]] == 3) and list(got["n_used"]) == [n, n, n - 2]


def test_residual_df_underflow(capi):
    """six families of two with one cell each: n_c - cells - K = 6, so the chromosome is scanned, but six fitted slopes leave
    no residual degree of freedom: df 0, lod 0, slopes NaN.  At the markers where the two rows of family 0 are identical it
    is not fitted, five slopes leave one degree of freedom, and the marker is fitted"""
    lens = (6,)
    grp, _ = sized_families((2,) * 6)
    n = len(grp)
    origin, _ = soft_rows(n, lens, 12)
    pair = np.flatnonzero(grp == 0)
    origin[pair[1], [1, 4]] = origin[pair[0], [1, 4]]
    pheno = noise(n, 2, 9)
    cs = chromstarts_of(lens)
    ref = reference_scan(origin, cs, 0, grp, None, 6, pheno)
    assert list(ref["df"]) == [0, 5, 0, 0, 5, 0] and list(ref["scanned"]) == [True]
    ctx, _, _ = map_context(capi, lens)
    got = ctx.qtl_scan_fam(origin, 0, grp, 6, pheno, slopes=True)
    ctx.close()
    compare(got, ref, cs, "residual df underflow", share=0)
    assert np.all(got["lod"][:, [0, 2, 3, 5]] == 0.0) and np.isnan(got["slope"][:, [0, 2, 3, 5]]).all()
    assert np.all(got["lod"][:, [1, 4]] > 0.0) and np.isnan(got["slope"][:, [1, 4], 0]).all()
    assert np.isfinite(got["slope"][:, [1, 4], 1:]).all() and np.all(got["rss0"] > 0.0)


# ------------------------------------------------------------------------------------- 4. permutations and refusals
def test_permutations_and_refusals(capi):
    """perm_max is the maximum of the explicitly permuted columns scanned as observed traits, to the bit: the phenotypes are
    multiples of 2^-8 that add up to exactly 0 over the used individuals, so that a column's mean, and with it every centred
    value, does not depend on the order in which a permutation lists the individuals.  Bad arguments leave poisoned buffers
    alone"""
    T, P, K, side = 2, 3, 1, 0
    origin, grp, cell, F, pheno, cov, use, perm = make_case(T, P, K, side, True, True, False)
    pheno = np.round(pheno * 256.0) / 256.0
    pheno[np.flatnonzero(use)[0]] -= np.nansum(pheno, axis=0)
    assert np.all(np.nansum(pheno, axis=0) == 0.0)
    n, cs = len(grp), chromstarts_of(CHROM_LENS)
    C = len(cs) - 1
    ctx, _, _ = map_context(capi, CHROM_LENS)
    got = ctx.qtl_scan_fam(origin, side, grp, F, pheno, cell=cell, cov=cov, use=use, perm=perm, slopes=True)
    moved = np.concatenate([np.where(use[:, None], np.nan_to_num(pheno)[perm[p]], np.nan) for p in range(P)], axis=1)
    explicit = ctx.qtl_scan_fam(origin, side, grp, F, moved, cell=cell, cov=cov, use=use)
    want = np.stack([explicit["lod"][:, cs[c]:cs[c + 1]].max(axis=1) for c in range(C)], axis=1).reshape(P, T, C)
    assert got["perm_max"].tobytes() == want.tobytes()
    ident = np.arange(n, dtype=np.int32)
    same = ctx.qtl_scan_fam(origin, side, grp, F, pheno, cell=cell, cov=cov, use=use, perm=ident[None])
    observed = np.stack([got["lod"][:, cs[c]:cs[c + 1]].max(axis=1) for c in range(C)], axis=1)
    assert same["perm_max"][0].tobytes() == observed.tobytes()
    # refused: a permutation across two cells of one family, one that takes an unused individual, a cell with members of two
    # groups, a group of n_fam, a negative cell of a used individual, a side of 2, a phenotype that is used and not finite,
    # nine covariates
    a, b = np.flatnonzero((grp == 5) & use)[0], np.flatnonzero((grp == 5) & use & (cell != cell[np.flatnonzero(grp == 5)[0]]))[0]
    assert cell[a] != cell[b]
    across = ident.copy()
    across[[a, b]] = [b, a]
    unused = np.flatnonzero(~use)[0]
    mate = np.flatnonzero(use & (cell == cell[unused]))[0]
    takes = ident.copy()
    takes[[unused, mate]] = [mate, unused]
    split = cell.copy()
    split[np.flatnonzero(grp == 3)[0]] = cell[np.flatnonzero(grp == 5)[0]]
    holed = pheno.copy()
    holed[mate, 1] = np.nan
    base = dict(side=side, grp=grp, cell=cell, n_fam=F, pheno=pheno, cov=cov, perm=ident[None])
    for kw in (dict(perm=across[None]), dict(perm=takes[None]), dict(cell=split), dict(grp=np.where(grp == 6, F, grp)),
               dict(cell=np.where(grp == 2, -1, cell)), dict(side=2), dict(pheno=holed), dict(cov=np.zeros((n, 9))), dict(n_fam=0)):
        out = {k: np.full_like(got[k], 77) for k in OUT_KEYS if k != "perm_max"}
        out["perm_max"] = np.full((1, T, C), 77.0)
        arg = dict(base, **kw)
        with pytest.raises(capi.Cnf2Error):
            ctx._qtlfam_call(n, origin.ctypes.data_as(capi.C.c_void_p), arg["side"], arg["grp"], arg["cell"], arg["n_fam"], arg["pheno"],
                             arg["cov"], use, arg["perm"], True, 0, out=out)
        assert all(np.all(v == 77) for v in out.values()), kw.keys()
    ctx.close()


# ------------------------------------------------------------------------------------- 5. a planted within-family QTL
PLANTED = dict(n_fam=16, kids=12, markers=17, chroms=2, seed=5, marker=8, noise=1.5, noise_seed=31, permutations=200, perm_seed=5)


def planted_trait(rows, grp, p=PLANTED):
    """s_f x_i(m*) + noise with s_f = +-1 alternating by family, on side 0"""
    x = regressor(rows, 0)[:, p["marker"]]
    return (np.where(grp % 2 == 0, 1.0, -1.0) * x + p["noise"] * 2.0 * noise(len(grp), 1, p["noise_seed"])[:, 0])[:, None]


def test_planted_within_family_qtl(capi):
    """make_outbred3, 16 families of 12 children, two chromosomes of 17 markers, through the real sweep: the sign of the
    planted effect alternates between the families, so the line-cross scan sees nothing and the within-family scan finds
    it.  The reference first, on the product's own rows (the seed and the noise were chosen on the oracle's rows so that both
    statements hold there)"""
    p = PLANTED
    ped = synth.make_outbred3(p["n_fam"], p["kids"], p["markers"], p["chroms"], seed=p["seed"], missing=0.2)
    ctx = capi.Context(0)
    ctx.upload(ped)
    d_o = qtl.origin_rows(ctx)
    rows = d_o.cpu().numpy()
    grp, cell, F = qtl.families(ped, 0)
    assert F == p["n_fam"] and np.array_equal(grp, cell)
    pheno = planted_trait(rows, grp)
    ref = reference_scan(rows, ped.chromstarts, 0, grp, cell, F, pheno)
    got = qtl.scan_fam(ctx, pheno, side="first", permutations=p["permutations"], seed=p["perm_seed"], rows=d_o, slopes=True)
    line = qtl.scan(ctx, pheno, permutations=p["permutations"], seed=p["perm_seed"], rows=d_o)
    ctx.close()
    err = np.abs(got["lod"] - ref["lod"][0]).max()
    print("scan_fam against the reference: lod %.3g" % err)
    assert err <= ATOL and np.array_equal(got["df"][0], ref["df"])
    t_fam, t_line = qtl.thresholds(got["perm_max"], alpha=(0.05,))["genome"][0, 0], qtl.thresholds(line["perm_max"], alpha=(0.05,))["genome"][0, 0]
    top = int(np.argmax(got["lod"][0]))
    print("within-family: peak %.2f at marker %d (planted %d), LOD there %.2f, 5 %% threshold %.2f; line cross: LOD at the planted "
          "marker %.2f, 5 %% threshold %.2f" % (got["lod"][0, top], top, p["marker"], got["lod"][0, p["marker"]], t_fam,
                                               line["lod"][0, p["marker"]], t_line))
    assert got["lod"][0, top] - got["lod"][0, p["marker"]] <= 1.5 and ped.chromstarts[0] <= top < ped.chromstarts[1]
    assert got["lod"][0, top] > t_fam
    assert line["lod"][0, p["marker"]] < t_line
    found = qtl.peaks(got["lod"], ped.pos, ped.chromstarts, t_fam)
    assert found and found[0]["lo"] <= p["marker"] <= found[0]["hi"]
    # the slopes at the peak carry the alternating sign
    s = got["slope"][0, top]
    assert np.isfinite(s).sum() == got["df"][0, top] and np.nanmean(s * np.where(np.arange(F) % 2 == 0, 1.0, -1.0)) > 0.5
    Fs, d1, d2 = qtl.fam_fstat(got["lod"], got["df"], got["n_used"], got["n_cells"], 0, chromstarts=ped.chromstarts)
    assert d1[0, top] == got["df"][0, top] and d2[0, top] == got["n_used"][0, 0] - got["n_cells"][0, 0] - d1[0, top] and Fs[0, top] > 1.0


# ------------------------------------------------------------------------------------- 6. command line
def test_cli_qtlfam(capi, tmp_path):
    """cnF2freq --qtlfam on the demo inputs with a phenotype file written here.  --output is the same bytes with and without
    it; the file parses; with --count 1 its figures are qtl.scan_fam's on host.Run.from_files of the same files, to the
    printed digits.  Of the demo's three analysed individuals only F has a parent with recorded parents (E, its first): one
    nested individual on the first side and none on the second, so every LOD is 0 and df 0, which is what the file must say;
    the covariate, the missing value and both sides take the table through its paths."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    exe, demo = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq"), os.path.join(ROOT, "tests", "golden", "demo")
    files = [os.path.join(demo, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    ph = tmp_path / "pheno.txt"
    ph.write_text("id weight age height\nC 1.25 3 10\nA 9 9 9\nD 2.5 4 NA\nF 3.5 5 12\n")             # A is not analysed
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet"]
    qargs = ["--phenofile", str(ph), "--qtl-covariates", "age", "--qtl-permutations", "20", "--qtl-seed", "9"]
    out_a, out_b, q2, q1, qs = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "q2.txt", tmp_path / "q1.txt", tmp_path / "qs.txt"
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    run("--count", "2", "--output", str(out_a))
    run("--count", "2", "--output", str(out_b), "--qtlfam", str(q2), *qargs)
    assert out_a.read_bytes() == out_b.read_bytes()
    run("--count", "1", "--output", str(out_b), "--qtlfam", str(q1), *qargs)
    run("--count", "1", "--output", str(out_b), "--qtlfam", str(qs), "--qtl-fam-side", "first", "--qtl-cell", "parent", *qargs)
    pos = [float(v) for v in open(files[0]).read().split()]
    M, traits = len(pos), ["weight", "height"]

    def parse(path, sides):
        blocks = path.read_text().split("\n\n")
        assert len(blocks) == 2
        rows = [ln.split("\t") for ln in blocks[0].split("\n")]
        w = 3 + len(traits)
        assert len(rows) == M and all(len(r) == 2 + w * sides for r in rows)
        assert all(int(r[0]) == 1 for r in rows) and [float(r[1]) for r in rows] == pos
        ints = np.array([[[int(r[2 + w * s + k]) for r in rows] for k in range(3)] for s in range(sides)])       # [side][n_used, n_cells, df][M]
        lod = np.array([[[float(r[5 + w * s + t]) for r in rows] for t in range(len(traits))] for s in range(sides)])
        assert all(len(r[5 + w * s + t].split(".")[1]) == 5 for r in rows for s in range(sides) for t in range(len(traits)))
        thr = [ln.split("\t") for ln in blocks[1].strip("\n").split("\n")]
        assert [r[0] for r in thr] == traits and all(len(r) == 1 + 2 * sides for r in thr)
        return ints, lod, np.array([[[float(r[1 + 2 * s]), float(r[2 + 2 * s])] for r in thr] for s in range(sides)])

    parse(q2, 2)
    ints, lod, thr = parse(q1, 2)
    ints1, lod1, thr1 = parse(qs, 1)
    assert np.array_equal(ints1[0], ints[0]) and np.array_equal(lod1[0], lod[0]) and np.array_equal(thr1[0], thr[0])
    r = host.Run.from_files(*files)
    assert (r.M, r.n_chrom, r.n_dous) == (M, 1, 3)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, [0, M], 3)
    pheno = np.array([[1.25, 10.0], [2.5, np.nan], [3.5, 12.0]])                        # C, D, F
    grp = (np.array([0, 1, 2], np.int32), np.array([0, 1, -1], np.int32))
    want = qtl.scan_fam(ctx, pheno, side="both", grp=grp, cell=grp, cov=np.array([3.0, 4.0, 5.0]), permutations=20, seed=9)
    ctx.close()
    r.close()
    for s, name in enumerate(("first", "second")):
        w = want[name]
        assert np.array_equal(ints[s, 0], np.repeat(w["n_used"][0], M)) and np.array_equal(ints[s, 1], np.repeat(w["n_cells"][0], M))
        assert np.array_equal(ints[s, 2], w["df"][0])
        np.testing.assert_allclose(lod[s], w["lod"], rtol=0, atol=0.51e-5)
        np.testing.assert_allclose(thr[s], qtl.thresholds(w["perm_max"])["genome"].T, rtol=0, atol=0.51e-5)
    assert list(ints[0, 0]) == [3] * M and list(ints[1, 0]) == [2] * M and list(ints[0, 1]) == [3] * M and list(ints[1, 1]) == [2] * M and np.all(ints[:, 2] == 0) and np.all(lod == 0.0) and np.all(thr == 0.0)
