"""GPU suite: the founder-haplotype scan (cnf2_qtl_scan_hap, Context.qtl_scan_hap / qtl_scan_hap_device, qtl.scan_hap,
cnF2freq --qtlhap) on the descent rows of the real sweep.  Against tests/qtlhap_reference.py where that reference is inside its
conditioning rule (asserted on the reference first) and against the host library's serial fit of the same header; on the
gather list's padding, the chromosome lengths, column counts under a cap, covariates, column numbers, masks; for its
bookkeeping, the permutation maxima to the bit, the reductions to the line-cross scan, the refusals, planted truth and the
command line."""
import numpy as np
import pytest

from cnf2freq_amd import origins, qtl, synth
from descent_reference import founder_cross
import qtlhap_reference as ref
from test_qtlhap_host import CROSSES, serial_scan, traits

pytestmark = pytest.mark.gpu

ATOL = 1e-9


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


@pytest.fixture(scope="module")
def host():
    from cnf2freq_amd import host as h
    return h


_ROWS = {}


def swept(capi, args):
    """(pedigree, truth, the product's descent rows on the host), one sweep per founder cross"""
    if args not in _ROWS:
        ped, truth = synth.make_founder_cross(*args)
        ctx = capi.Context(0)
        ctx.upload(ped)
        _ROWS[args] = (ped, truth, ctx.sweep_descent()["descent"])
        ctx.close()
    return _ROWS[args]


@pytest.fixture(scope="module")
def cross(capi):
    """the first founder cross with a context that has its map: (ctx, ped, rows, col)"""
    ped, _, rows = swept(capi, CROSSES[0])
    ctx = capi.Context(0)
    ctx.upload(ped)
    col, _ = origins.descent_columns(ped.par, ped.dous)
    yield ctx, ped, rows, col
    ctx.close()


def compare(got, want, what, coef=True, inside=None):
    """against a reference dict: n_used, rss0 and df where compared, LOD and coefficients at the project's bar"""
    inside = np.ones(len(want["df"]), bool) if inside is None else inside
    assert inside.any(), what
    assert np.array_equal(got["n_used"], want["n_used"]), what
    np.testing.assert_allclose(got["rss0"], want["rss0"], rtol=1e-12, atol=ATOL, err_msg=what)
    assert np.array_equal(got["df"][inside], want["df"][inside]), what
    err_lod = np.abs(got["lod"][:, inside] - want["lod"][:, inside]).max()
    err_coef = 0.0
    if coef:
        gc, wc = got["coef"][:, inside], want["coef"][:, inside]
        assert np.array_equal(np.isnan(gc), np.isnan(wc)), what + ": the dropped columns"
        err_coef = np.nanmax(np.abs(gc - wc)) if np.isfinite(wc).any() else 0.0
    print("%s: %d of %d markers compared; largest difference lod %.3g, coef %.3g" % (what, inside.sum(), len(inside), err_lod, err_coef))
    assert err_lod <= ATOL and err_coef <= ATOL, what
    assert np.all(got["lod"] >= 0) and np.all(np.isfinite(got["lod"]))


def same_bits(a, b, keys=("lod", "df", "coef", "rss0", "n_used", "perm_max")):
    for k in keys:
        if a.get(k) is not None and b.get(k) is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---------------------------------------------------------------------------------------------- 1. the founder crosses
@pytest.mark.parametrize("args", CROSSES)
def test_founder_crosses_through_the_sweep(capi, host, args):
    ped, _, rows = swept(capi, args)
    n = len(ped.dous)
    col, grand = origins.descent_columns(ped.par, ped.dous)
    y, cov = traits(n, 3, 5), traits(n, 2, 6)
    want = ref.scan(rows, col, 8, y, ped.chromstarts, cov)
    assert want["inside"].mean() >= 0.9 and np.all(want["df"][want["inside"]] == 6), "asserted on the reference first"
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.qtl_scan_hap(rows, col, 8, y, cov=cov)
    ctx.close()
    compare(got, want, "founder cross %s against the reference" % (args[:3],), inside=want["inside"])
    compare(got, serial_scan(host, rows, col, 8, y, ped.chromstarts, cov), "against the serial fit", inside=want["inside"])


# ---------------------------------------------------------------------------------------------- 2. patterns and shapes
def test_patterns_dealt_out_in_shuffled_order(capi, host, cross):
    """patterns of 1, 2, 3, 4, 5, 8 and 9 individuals, their members scattered over the individuals: the padding of every
    pattern to four slots, a pattern of one step and of three.  The model does not care what a column means."""
    ctx, ped, rows, _ = cross
    n = len(ped.dous)
    sizes = [1, 2, 3, 4, 5, 8, 9]
    rng = np.random.default_rng(17)
    pat = np.array([rng.permutation(8) for _ in sizes], np.int32)
    assert len({tuple(p) for p in pat}) == len(sizes)
    member = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    col = np.full((n, 8), -1, np.int32)
    who = rng.permutation(n)[:len(member)]
    col[who] = pat[member]
    y = traits(n, 2, 21)
    want = ref.scan(rows, col, 8, y, ped.chromstarts)
    assert np.all(want["n_used"] == sum(sizes))
    got = ctx.qtl_scan_hap(rows, col, 8, y)
    compare(got, want, "seven patterns against the reference", inside=want["inside"])
    compare(got, serial_scan(host, rows, col, 8, y, ped.chromstarts), "seven patterns against the serial fit", inside=want["inside"])


CHROM_LENS = (1, 2, 15, 16, 17, 33)


def test_chromosome_lengths(capi, host):
    """tiles of two markers at odd and even chromosome lengths, the single marker"""
    M = sum(CHROM_LENS)
    ped, _ = synth.make_founder_cross(3, 12, M - 1, 1, 777, 0.2, 0.98)
    ped.chromstarts = np.cumsum((0,) + CHROM_LENS).astype(np.int32)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = ctx.sweep_descent()["descent"]
    n = len(ped.dous)
    col, _ = origins.descent_columns(ped.par, ped.dous)
    y = ref.exact_phenotypes(n, 2, 4)
    perm = qtl.permutations(n, 3, 5)
    want = ref.scan(rows, col, 8, y, ped.chromstarts)
    assert want["inside"].mean() >= 0.9
    got = ctx.qtl_scan_hap(rows, col, 8, y, perm=perm)
    compare(got, want, "six chromosome lengths against the reference", inside=want["inside"])
    compare(got, serial_scan(host, rows, col, 8, y, ped.chromstarts), "against the serial fit", inside=want["inside"])
    explicit = ctx.qtl_scan_hap(rows, col, 8, np.concatenate([y[perm[p]] for p in range(3)], axis=1), coef=False)["lod"].reshape(3, 2, M)
    cs = ped.chromstarts
    for c in range(len(CHROM_LENS)):
        assert np.array_equal(got["perm_max"][:, :, c], explicit[:, :, cs[c]:cs[c + 1]].max(axis=2)), c
    ctx.close()


@pytest.mark.parametrize("T,P", [(1, 0), (16, 0), (17, 0), (6, 16)])
def test_columns_under_a_cap(cross, T, P):
    """1, 16, 17 and 102 columns: a column's bits do not depend on the tile, the cap or the call"""
    ctx, ped, rows, col = cross
    n = len(ped.dous)
    y = ref.exact_phenotypes(n, T, 30 + T)
    perm = qtl.permutations(n, P, 3) if P else None
    ctx.set_qtl_columns(0)
    base = ctx.qtl_scan_hap(rows, col, 8, y, perm=perm)
    ctx.set_qtl_columns(16)
    capped = ctx.qtl_scan_hap(rows, col, 8, y, perm=perm)
    ctx.set_qtl_columns(0)
    same_bits(base, capped)
    one = ctx.qtl_scan_hap(rows, col, 8, y[:, T - 1])
    assert np.array_equal(one["lod"][0], base["lod"][T - 1]) and np.array_equal(one["coef"][0], base["coef"][T - 1], equal_nan=True)
    if P:
        # perm_max against explicitly permuted columns, to the bit: phenotypes that are multiples of 2^-8 adding up to 0
        cs = ped.chromstarts
        for p in (0, P - 1):
            explicit = ctx.qtl_scan_hap(rows, col, 8, y[perm[p]], coef=False)["lod"]
            for c in range(len(cs) - 1):
                assert np.array_equal(base["perm_max"][p, :, c], explicit[:, cs[c]:cs[c + 1]].max(axis=1))
        assert base["perm_max"].shape == (P, T, 2) and np.all(base["perm_max"] > 0)


@pytest.mark.parametrize("K", [0, 1, 2, 8])
def test_covariates(host, cross, K):
    ctx, ped, rows, col = cross
    n = len(ped.dous)
    y = traits(n, 2, 40)
    cov = traits(n, K, 41) * 3.0 + 100.0 if K else None
    want = ref.scan(rows, col, 8, y, ped.chromstarts, cov)
    assert want["inside"].mean() >= 0.9
    got = ctx.qtl_scan_hap(rows, col, 8, y, cov=cov)
    compare(got, want, "K = %d against the reference" % K, inside=want["inside"])
    compare(got, serial_scan(host, rows, col, 8, y, ped.chromstarts, cov), "K = %d against the serial fit" % K, inside=want["inside"])


@pytest.mark.parametrize("H", [1, 8, 9, 16, 17, 32])
def test_column_numbers(capi, host, H):
    """the larger values by splitting the founders' columns arbitrarily among the individuals"""
    ped, _, rows = swept(capi, (6, 16, 9, 2, 777, 0.2, 0.98))
    n = len(ped.dous)
    base, _ = origins.descent_columns(ped.par, ped.dous)
    i = np.arange(n)[:, None]
    if H == 1:
        col = np.zeros((n, 8), np.int32)
    elif H in (8, 16, 32):
        col = (base + 8 * (i % (H // 8))).astype(np.int32)
    else:
        col = (base + 8 * (i % (H // 8))).astype(np.int32)
        col[(i[:, 0] % 5 == 0)[:, None] & (base == 0)] = H - 1
    assert col.max() == H - 1
    y = traits(n, 2, 50 + H)
    want = ref.scan(rows, col, H, y, ped.chromstarts)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.qtl_scan_hap(rows, col, H, y)
    ctx.close()
    ser = serial_scan(host, rows, col, H, y, ped.chromstarts)
    if H == 1:
        assert np.array_equal(got["df"], ser["df"])
        assert np.all(got["df"] == 0) and np.all(got["lod"] == 0) and np.isnan(got["coef"]).all() and np.all(got["rss0"] > 0)
        return
    print("H = %d: df %d .. %d, %d of %d markers inside the rule" % (H, got["df"].min(), got["df"].max(), want["inside"].sum(), len(want["inside"])))
    assert got["df"].max() >= min(H, 8) - 2
    compare(got, ser, "H = %d against the serial fit" % H, inside=want["inside"])
    compare(got, want, "H = %d against the reference" % H, inside=want["inside"])


def test_masks_and_a_skipped_chromosome(host, cross):
    """unused individuals, individuals with a -1 cell, an individual whose rows are all zero on one chromosome"""
    ctx, ped, rows, col = cross
    n = len(ped.dous)
    col = col.copy()
    col[5, 2] = -1
    col[20, 4:] = -1
    use = np.ones(n, bool)
    use[[0, 7, 30]] = False
    cs = ped.chromstarts
    rows = rows.copy()
    rows[11, cs[1]:cs[2]] = 0.0
    y = traits(n, 2, 12)
    y[~use] = np.nan
    yz = np.where(use[:, None], y, 0.0)
    want = ref.scan(rows, col, 8, yz, cs, use=use)
    assert want["n_used"].tolist() == [n - 5, n - 6] and want["inside"].mean() >= 0.9
    got = ctx.qtl_scan_hap(rows, col, 8, yz, use=use)
    compare(got, want, "masks against the reference", inside=want["inside"])
    compare(got, serial_scan(host, rows, col, 8, yz, cs, use=use), "masks against the serial fit", inside=want["inside"])


# ---------------------------------------------------------------------------------------------- 3. bookkeeping
def test_bookkeeping(capi, cross):
    import torch
    ctx, ped, rows, col = cross
    n, M, C = len(ped.dous), ped.n_markers, 2
    y, cov = ref.exact_phenotypes(n, 3, 60), traits(n, 1, 61)
    perm = qtl.permutations(n, 5, 8)
    base = ctx.qtl_scan_hap(rows, col, 8, y, cov=cov, perm=perm)
    same_bits(base, ctx.qtl_scan_hap(rows, col, 8, y, cov=cov, perm=perm))
    nocoef = ctx.qtl_scan_hap(rows, col, 8, y, cov=cov, perm=perm, coef=False)
    assert nocoef["coef"] is None
    same_bits(base, nocoef)
    dev = torch.device("cuda:0")
    d_rows = torch.tensor(rows, dtype=torch.float64, device=dev)
    same_bits(base, ctx.qtl_scan_hap_device(n, d_rows.data_ptr(), col, 8, y, cov=cov, perm=perm))
    # rows from the sweep's device form, outputs on the device
    t = lambda *shape, dtype=torch.float64: torch.full(shape, 7, dtype=dtype, device=dev)
    d_f, d_l, d_d, d_c = t(n, C, 8), t(n, C), t(n, M, 8), t(C, dtype=torch.int32)
    ctx.sweep_descent_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_d.data_ptr(), d_c.data_ptr())
    out = dict(lod=t(3, M), df=t(M, dtype=torch.int32), coef=t(3, M, 8), rss0=t(3, C), n_used=t(C, dtype=torch.int32), perm_max=t(5, 3, C))
    assert ctx.qtl_scan_hap_device(n, d_d.data_ptr(), col, 8, y, cov=cov, perm=perm, d_out={k: v.data_ptr() for k, v in out.items()}) is None
    ctx.sync()
    torch.cuda.synchronize()
    assert np.array_equal(d_d.cpu().numpy(), rows)
    same_bits(base, {k: v.cpu().numpy() for k, v in out.items()})
    # qtl.scan_hap: patterns of missing phenotypes, its own sweep, its own column map
    ym = y.copy()
    ym[3, 1] = np.nan
    whole = qtl.scan_hap(ctx, ped, ym, cov=cov, permutations=4, seed=2)
    assert whole["n_columns"] == 8 and np.array_equal(whole["col"], col)
    assert np.array_equal(whole["lod"][[0, 2]], base["lod"][[0, 2]]) and np.array_equal(whole["df"][0], base["df"])
    assert whole["n_used"].tolist() == [[n, n], [n - 1, n - 1], [n, n]] and whole["perm_max"].shape == (4, 3, C)
    use = np.ones(n, bool)
    use[3] = False
    one = ctx.qtl_scan_hap(rows, col, 8, np.where(use, ym[:, 1], 0.0), cov=cov, use=use)
    assert np.array_equal(whole["lod"][1], one["lod"][0])
    F, df1, df2 = qtl.hap_fstat(whole["lod"], whole["df"], whole["n_used"], 1, chromstarts=ped.chromstarts)
    assert np.all(df2[whole["df"] > 0] == (np.repeat(whole["n_used"], np.diff(ped.chromstarts), axis=1) - 2 - whole["df"])[whole["df"] > 0])
    assert np.all(F[whole["df"] > 0] >= 0)


def test_reductions_to_the_line_cross_scan(capi):
    """by="line" on an F2: Z_B - Z_A = 2 a and Z_A + Z_B = 2, so the LOD is cnf2_qtl_scan's additive one on the origin rows of
    the same context, with df = 1"""
    ped = synth.make_f2(40, 20, 2, seed=6, missing=0.1)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n = len(ped.dous)
    y, cov = traits(n, 3, 70), traits(n, 1, 71)
    line = qtl.scan_hap(ctx, ped, y, cov=cov, by="line")
    add = ctx.qtl_scan(ctx.sweep_origins()["origin"], y, cov=cov, additive=True)
    ctx.close()
    assert line["n_columns"] == 2 and np.all(line["df"] == 1) and np.all(add["rank"] == 1)
    print("by line against the additive scan: largest difference %.3g" % np.abs(line["lod"] - add["lod"]).max())
    np.testing.assert_allclose(line["lod"], add["lod"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(line["rss0"], add["rss0"], rtol=1e-12)
    # Z_A = 1 - a: the coefficient of the kept column A is minus the additive effect
    np.testing.assert_allclose(line["coef"][:, :, 0], -add["coef"][:, :, 0], rtol=0, atol=ATOL)
    assert np.isnan(line["coef"][:, :, 1]).all()


def test_no_residual_degree_of_freedom(cross):
    ctx, ped, rows, col = cross
    n = len(ped.dous)
    y = traits(n, 1, 3)
    for n_c, fitted in ((7, False), (8, True)):
        use = np.zeros(n, bool)
        use[np.arange(n_c) * 4] = True
        got = ctx.qtl_scan_hap(rows, col, 8, y, use=use)
        want = ref.marker(rows[:, 3], col, 8, y, None, use)
        assert want["inside"] and (want["pivots"] >= ref.PIVOT).sum() == 6
        assert got["n_used"].tolist() == [n_c, n_c] and got["df"][3] == (6 if fitted else 0)
        assert (got["lod"][0, 3] > 0) == fitted and np.isnan(got["coef"][0, 3]).all() != fitted


def test_refusals_write_nothing(cross):
    ctx, ped, rows, col = cross
    n, M = len(ped.dous), ped.n_markers
    rows = np.ascontiguousarray(rows)
    y, cov, use = np.ones((n, 2)), np.ones((n, 1)), np.ones(n, np.uint8)
    perm = np.ascontiguousarray(qtl.permutations(n, 2, 1), np.int32)
    lod, df, coef = np.full((2, M), 7.0), np.full(M, 7, np.int32), np.full((2, M, 8), 7.0)
    rss0, nu, pm = np.full((2, 2), 7.0), np.full(2, 7, np.int32), np.full((2, 2, 2), 7.0)
    p = lambda a: a.ctypes.data
    good = [n, p(rows), p(col), 8, 2, p(y), p(use), 1, p(cov), 2, p(perm), p(lod), p(df), p(coef), p(rss0), p(nu), p(pm), 0]
    high, low, nan_y, bad_perm = col.copy(), col.copy(), y.copy(), perm.copy()
    high[4, 1], low[4, 1], nan_y[2, 0] = 8, -2, np.nan
    bad_perm[1, 0] = bad_perm[1, 1]
    changes = [(0, 0), (1, None), (2, None), (3, 0), (3, 33), (4, 0), (5, None), (7, 9), (7, -1), (8, None), (9, -1), (10, None), (16, None),
               (11, None), (12, None), (14, None), (15, None), (2, p(high)), (2, p(low)), (5, p(nan_y)), (10, p(bad_perm)), (17, 1 << 23)]
    for k, v in changes:
        args = list(good)
        args[k] = v
        if (k, v) == (17, 1 << 23):
            args[1] = p(rows) + 8          # device rows must be aligned to 16 bytes (refused before anything is read)
        assert ctx.L.cnf2_qtl_scan_hap(ctx.h, *args) == -2, (k, v)
        for a in (lod, df, coef, rss0, nu, pm):
            assert np.all(a == 7)
    assert ctx.L.cnf2_qtl_scan_hap(ctx.h, *good) == 0 and not np.any(lod == 7)
    empty = capi_context_without_map(ctx)
    assert empty.L.cnf2_qtl_scan_hap(empty.h, *good) == -3      # CNF2_ERR_STATE: no map
    empty.close()


def capi_context_without_map(ctx):
    return type(ctx)(0)


# ---------------------------------------------------------------------------------------------- 4. planted truth
PLANT_ARGS, PLANT_SEED, PLANT_NOISE, PLANT_MARKER = (8, 15, 17, 2, 777, 0.2, 0.98), 2, 1.0, 8
PLANT_BETA = np.array([1.0, -1.0, -1.0, 1.0, -1.0, 1.0, 1.0, -1.0])      # mixed sign inside each line: no line effect


def test_planted_truth(capi):
    """The trait is sum_h beta_h Z_m*[i][h] + noise with the true dosages of the founder haplotypes at marker 8, the effects
    of mixed sign inside each line.  Seed and noise were chosen on the oracle's rows: there the founder-haplotype LOD is 16.2 at
    marker 8 against a 0.95 quantile of 4.03 over its own 200 permutations, and the line-cross scan has 1.29 there against
    2.23."""
    ped, truth = synth.make_founder_cross(*PLANT_ARGS)
    n, m_star = len(ped.dous), PLANT_MARKER
    Z = np.zeros((n, 8))
    for s in range(2):
        np.add.at(Z, (np.arange(n), 4 * s + truth[:, s, m_star]), 1.0)
    y = Z @ PLANT_BETA + PLANT_NOISE * np.random.default_rng(PLANT_SEED).normal(size=n)
    ctx = capi.Context(0)
    ctx.upload(ped)
    hap = qtl.scan_hap(ctx, ped, y, permutations=200, seed=PLANT_SEED)
    line = qtl.scan(ctx, y, permutations=200, seed=PLANT_SEED)
    ctx.close()
    lod = hap["lod"][0]
    peak = int(lod.argmax())
    thr = qtl.thresholds(hap["perm_max"], alpha=(0.05,))["genome"][0, 0]
    thr_line = qtl.thresholds(line["perm_max"], alpha=(0.05,))["genome"][0, 0]
    cs = ped.chromstarts
    c = int(np.searchsorted(cs, peak, side="right")) - 1
    seg = np.arange(cs[c], cs[c + 1])
    support = seg[lod[seg] >= lod[peak] - 1.5]
    print("founder-haplotype LOD %.2f at marker %d (threshold %.2f), 1.5-LOD interval %d .. %d; line-cross LOD at marker %d: %.2f (threshold %.2f)"
          % (lod[peak], peak, thr, support.min(), support.max(), m_star, line["lod"][0, m_star], thr_line))
    assert support.min() <= m_star <= support.max()
    assert lod[peak] > thr
    assert line["lod"][0, m_star] < thr_line
    assert np.all(hap["df"][0] >= 5)


# ---------------------------------------------------------------------------------------------- 5. command line
def test_cli_qtlhap(capi, tmp_path):
    """cnF2freq --qtlhap on the demo inputs with a phenotype file written here.  --output is the same bytes with and without
    it; the file parses; with --count 1 its figures are qtl.scan_hap's on host.Run.from_files of the same files, to the
    printed digits.  Of the demo's three analysed individuals C and D descend on both sides from the founders A and B (through
    the implicit F1 parents the reader gives them) and F has a parent without recorded parents: two individuals are in the
    model, too few to scan a chromosome, so n_used is 2 and df and every LOD are 0, which is what the file must say; the
    covariate, the missing value and the permutations take the table through its paths."""
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
    out_a, out_b, q2, q1, qf = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "q2.txt", tmp_path / "q1.txt", tmp_path / "qf.txt"
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    run("--count", "2", "--output", str(out_a))
    run("--count", "2", "--output", str(out_b), "--qtlhap", str(q2), *qargs)
    assert out_a.read_bytes() == out_b.read_bytes()
    run("--count", "1", "--output", str(out_b), "--qtlhap", str(q1), *qargs)
    run("--count", "1", "--output", str(out_b), "--qtlhap", str(qf), "--qtl-hap-by", "founder", *qargs)
    pos = [float(v) for v in open(files[0]).read().split()]
    M, names = len(pos), ["weight", "height"]

    def parse(path):
        blocks = path.read_text().split("\n\n")
        assert len(blocks) == 2
        rows = [ln.split("\t") for ln in blocks[0].split("\n")]
        assert len(rows) == M and all(len(r) == 4 + len(names) for r in rows)
        assert all(int(r[0]) == 1 for r in rows) and [float(r[1]) for r in rows] == pos
        assert all(len(v.split(".")[1]) == 5 for r in rows for v in r[4:])
        thr = [ln.split("\t") for ln in blocks[1].strip("\n").split("\n")]
        assert [r[0] for r in thr] == names and all(len(r) == 3 for r in thr)
        return (np.array([[int(r[2]), int(r[3])] for r in rows]), np.array([[float(v) for v in r[4:]] for r in rows]).T,
                np.array([[float(r[1]), float(r[2])] for r in thr]))

    parse(q2)
    parse(qf)
    ints, lod, thr = parse(q1)
    r = host.Run.from_files(*files)
    assert (r.M, r.n_chrom, r.n_dous) == (M, 1, 3)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, [0, M], 3)
    pheno = np.array([[1.25, 10.0], [2.5, np.nan], [3.5, 12.0]])                        # C, D, F
    col = np.array([[0, 1, 2, 3, 0, 1, 2, 3], [0, 1, 2, 3, 0, 1, 2, 3], [0, 1, 2, 3, -1, -1, -1, -1]], np.int32)
    want = qtl.scan_hap(ctx, None, pheno, cov=np.array([3.0, 4.0, 5.0]), col=col, n_columns=4, permutations=20, seed=9)
    ctx.close()
    r.close()
    assert np.array_equal(ints[:, 0], np.repeat(want["n_used"][0], M)) and np.array_equal(ints[:, 1], want["df"][0])
    np.testing.assert_allclose(lod, want["lod"], rtol=0, atol=0.51e-5)
    np.testing.assert_allclose(thr, qtl.thresholds(want["perm_max"])["genome"].T, rtol=0, atol=0.51e-5)
    assert np.all(ints[:, 0] == 2) and np.all(ints[:, 1] == 0) and np.all(lod == 0.0) and np.all(thr == 0.0)
