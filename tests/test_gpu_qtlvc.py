"""GPU suite: the variance-component scan (cnf2_qtl_scan_vc, Context.qtl_scan_vc / qtl_scan_vc_device, qtl.scan_vc,
cnF2freq --qtlvc) on the descent rows of the real sweep.  Against tests/qtlvc_reference.py on the cells that reference compares
(asserted on the reference first) and against the host library's serial fit of the same header; on 1 to 64 columns, the
chromosome lengths, column counts under a cap, covariates, shuffled patterns, masks; for its bookkeeping, the permutation
maxima to the bit, the refusals, planted truth and the command line.  No marker may report rank -1.  The residual variance is
compared at the h the run returned, as the BLUP is: see tests/qtlvc_reference.py.

Largest differences seen on the MI355X are recorded in DESIGN.md (8w)."""
import numpy as np
import pytest

from cnf2freq_amd import origins, qtl, synth
import qtlvc_reference as ref
from qtlhap_reference import exact_phenotypes
from test_qtlhap_host import CROSSES, traits
from test_qtlvc_host import serial_scan

pytestmark = pytest.mark.gpu

ATOL = 1e-9
KEYS = ("lod", "h", "sigma2", "blup", "eval", "rank", "rss0", "n_used", "perm_max")


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


def reference(rows, col, H, y, cs, cov=None, use=None):
    want = ref.scan(rows, col, H, y, cs, cov, use)
    assert want["compared"].mean() >= 0.9, "asserted on the reference first: at least 0.9 of the cells are compared"
    return want


def against_serial(got, ser, what):
    """the serial fit takes the same steps: the project's bar on everything, h included (1e-7 is the search's own width)"""
    assert np.array_equal(got["rank"], ser["rank"]) and np.array_equal(got["n_used"], ser["n_used"]), what
    dmax = max(np.abs(ser["eval"]).max(), 1e-300)
    err = {k: float(np.abs(got[k] - ser[k]).max()) for k in ("lod", "h", "eval", "rss0")}
    same = np.abs(got["h"] - ser["h"]) <= 1e-9            # (sigma2 and the BLUP have a slope in h)
    err["sigma2"] = float(np.abs(got["sigma2"] - ser["sigma2"])[same].max())
    err["blup"] = float(np.abs(got["blup"] - ser["blup"])[same].max() / max(np.abs(ser["blup"]).max(), 1e-300))
    print("%s: largest difference lod %.3g, h %.3g, sigma2 %.3g, blup (relative) %.3g, eigenvalues (of d_max) %.3g; %d of %d cells at the same h"
          % (what, err["lod"], err["h"], err["sigma2"], err["blup"], err["eval"] / dmax, same.sum(), same.size))
    assert err["lod"] <= ATOL and err["h"] <= 1e-7 and err["sigma2"] <= ATOL and err["blup"] <= ATOL and err["eval"] <= 1e-12 * dmax, what
    assert same.mean() >= 0.9, what


def same_bits(a, b, keys=KEYS):
    for k in keys:
        if a.get(k) is not None and b.get(k) is not None:
            assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- 1. the founder crosses
@pytest.mark.parametrize("args", CROSSES)
def test_founder_crosses_through_the_sweep(capi, host, args):
    ped, _, rows = swept(capi, args)
    n = len(ped.dous)
    col, grand = origins.descent_columns(ped.par, ped.dous)
    y, cov = traits(n, 3, 5), traits(n, 2, 6)
    want = reference(rows, col, 8, y, ped.chromstarts, cov)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.qtl_scan_vc(rows, col, 8, y, cov=cov)
    ctx.close()
    ref.check(got, want, "founder cross %s against the reference" % (args[:3],))
    against_serial(got, serial_scan(host, rows, col, 8, y, ped.chromstarts, cov), "against the serial fit")


# ---------------------------------------------------------------------------------------------- 2. patterns and shapes
def test_patterns_dealt_out_in_shuffled_order(capi, host, cross):
    """patterns of 1, 2, 3, 4, 5, 8 and 9 individuals, their members scattered over the individuals"""
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
    want = reference(rows, col, 8, y, ped.chromstarts)
    assert np.all(want["n_used"] == sum(sizes))
    got = ctx.qtl_scan_vc(rows, col, 8, y)
    ref.check(got, want, "seven patterns against the reference")
    against_serial(got, serial_scan(host, rows, col, 8, y, ped.chromstarts), "seven patterns against the serial fit")


CHROM_LENS = (1, 2, 3, 17)


def test_chromosome_lengths(capi, host):
    """tiles of two markers at odd and even chromosome lengths, the single marker; perm_max against explicit columns"""
    M = sum(CHROM_LENS)
    ped, _ = synth.make_founder_cross(3, 12, M - 1, 1, 777, 0.2, 0.98)
    ped.chromstarts = np.cumsum((0,) + CHROM_LENS).astype(np.int32)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = ctx.sweep_descent()["descent"]
    n = len(ped.dous)
    col, _ = origins.descent_columns(ped.par, ped.dous)
    y = exact_phenotypes(n, 2, 4)
    perm = qtl.permutations(n, 3, 5)
    want = reference(rows, col, 8, y, ped.chromstarts)
    got = ctx.qtl_scan_vc(rows, col, 8, y, perm=perm)
    ref.check(got, want, "four chromosome lengths against the reference")
    against_serial(got, serial_scan(host, rows, col, 8, y, ped.chromstarts), "against the serial fit")
    explicit = ctx.qtl_scan_vc(rows, col, 8, np.concatenate([y[perm[p]] for p in range(3)], axis=1), blup=False)["lod"].reshape(3, 2, M)
    cs = ped.chromstarts
    for c in range(len(CHROM_LENS)):
        assert np.array_equal(got["perm_max"][:, :, c], explicit[:, :, cs[c]:cs[c + 1]].max(axis=2)), c
    ctx.close()


@pytest.mark.parametrize("T,P", [(1, 0), (16, 0), (17, 0), (6, 16)])
def test_columns_under_a_cap(cross, T, P):
    """1, 16, 17 and 102 columns: a column's bits do not depend on the tile, the cap or the call"""
    ctx, ped, rows, col = cross
    n = len(ped.dous)
    y = exact_phenotypes(n, T, 30 + T)
    perm = qtl.permutations(n, P, 3) if P else None
    ctx.set_qtl_columns(0)
    base = ctx.qtl_scan_vc(rows, col, 8, y, perm=perm)
    ctx.set_qtl_columns(16)
    capped = ctx.qtl_scan_vc(rows, col, 8, y, perm=perm)
    ctx.set_qtl_columns(0)
    same_bits(base, capped)
    assert np.all(base["rank"] >= 0)
    one = ctx.qtl_scan_vc(rows, col, 8, y[:, T - 1])
    for k in ("lod", "h", "sigma2", "blup"):
        assert np.array_equal(one[k][0], base[k][T - 1]), k
    if P:
        # perm_max against explicitly permuted columns, to the bit: phenotypes that are multiples of 2^-8 adding up to 0
        cs = ped.chromstarts
        for p in (0, P - 1):
            explicit = ctx.qtl_scan_vc(rows, col, 8, y[perm[p]], blup=False)["lod"]
            for c in range(len(cs) - 1):
                assert np.array_equal(base["perm_max"][p, :, c], explicit[:, cs[c]:cs[c + 1]].max(axis=1))
        assert base["perm_max"].shape == (P, T, 2) and np.all(base["perm_max"] >= 0) and np.any(base["perm_max"] > 0)


@pytest.mark.parametrize("K", [0, 2, 8])
def test_covariates(host, cross, K):
    ctx, ped, rows, col = cross
    n = len(ped.dous)
    y = traits(n, 2, 40)
    cov = traits(n, K, 41) * 3.0 + 100.0 if K else None
    want = reference(rows, col, 8, y, ped.chromstarts, cov)
    got = ctx.qtl_scan_vc(rows, col, 8, y, cov=cov)
    ref.check(got, want, "K = %d against the reference" % K)
    against_serial(got, serial_scan(host, rows, col, 8, y, ped.chromstarts, cov), "K = %d against the serial fit" % K)


@pytest.mark.parametrize("H", [1, 8, 9, 16, 17, 32, 33, 64])
def test_column_numbers(capi, host, H):
    """the larger values by splitting the founders' columns arbitrarily among the individuals"""
    ped, _, rows = swept(capi, (6, 16, 9, 2, 777, 0.2, 0.98))
    n = len(ped.dous)
    assert n == 96
    base, _ = origins.descent_columns(ped.par, ped.dous)
    i = np.arange(n)[:, None]
    if H == 1:
        col = np.zeros((n, 8), np.int32)
    else:
        col = (base + 8 * (i % (H // 8))).astype(np.int32)
        if H % 8:
            col[(i[:, 0] % 5 == 0)[:, None] & (base == 0)] = H - 1
    assert col.max() == H - 1
    y = traits(n, 2, 50 + H)
    want = reference(rows, col, H, y, ped.chromstarts)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.qtl_scan_vc(rows, col, H, y)
    ctx.close()
    ser = serial_scan(host, rows, col, H, y, ped.chromstarts)
    if H == 1:
        assert np.all(got["rank"] == 0) and np.all(got["lod"] == 0) and np.all(got["h"] == 0) and np.all(got["blup"] == 0)
        assert np.all(got["rss0"] > 0)
        return
    print("H = %d: rank %d .. %d" % (H, got["rank"].min(), got["rank"].max()))
    assert got["rank"].min() >= 1 and got["rank"].max() >= min(H, 8) - 2
    against_serial(got, ser, "H = %d against the serial fit" % H)
    ref.check(got, want, "H = %d against the reference" % H)


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
    want = reference(rows, col, 8, yz, cs, use=use)
    assert want["n_used"].tolist() == [n - 5, n - 6]
    got = ctx.qtl_scan_vc(rows, col, 8, yz, use=use)
    ref.check(got, want, "masks against the reference")
    against_serial(got, serial_scan(host, rows, col, 8, yz, cs, use=use), "masks against the serial fit")


# ---------------------------------------------------------------------------------------------- 3. bookkeeping
def test_bookkeeping(capi, cross):
    import torch
    ctx, ped, rows, col = cross
    n, M, C = len(ped.dous), ped.n_markers, 2
    y, cov = exact_phenotypes(n, 3, 60), traits(n, 1, 61)
    perm = qtl.permutations(n, 5, 8)
    base = ctx.qtl_scan_vc(rows, col, 8, y, cov=cov, perm=perm)
    same_bits(base, ctx.qtl_scan_vc(rows, col, 8, y, cov=cov, perm=perm))
    bare = ctx.qtl_scan_vc(rows, col, 8, y, cov=cov, perm=perm, blup=False, evals=False)
    assert bare["blup"] is None and bare["eval"] is None
    same_bits(base, bare)
    dev = torch.device("cuda:0")
    d_rows = torch.tensor(rows, dtype=torch.float64, device=dev)
    same_bits(base, ctx.qtl_scan_vc_device(n, d_rows.data_ptr(), col, 8, y, cov=cov, perm=perm))
    # rows from the sweep's device form, outputs on the device
    t = lambda *shape, dtype=torch.float64: torch.full(shape, 7, dtype=dtype, device=dev)
    d_f, d_l, d_d, d_c = t(n, C, 8), t(n, C), t(n, M, 8), t(C, dtype=torch.int32)
    ctx.sweep_descent_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_d.data_ptr(), d_c.data_ptr())
    out = dict(lod=t(3, M), h=t(3, M), sigma2=t(3, M), blup=t(3, M, 8), eval=t(M, 8), rank=t(M, dtype=torch.int32), rss0=t(3, C),
               n_used=t(C, dtype=torch.int32), perm_max=t(5, 3, C))
    assert ctx.qtl_scan_vc_device(n, d_d.data_ptr(), col, 8, y, cov=cov, perm=perm, d_out={k: v.data_ptr() for k, v in out.items()}) is None
    ctx.sync()
    torch.cuda.synchronize()
    assert np.array_equal(d_d.cpu().numpy(), rows)
    same_bits(base, {k: v.cpu().numpy() for k, v in out.items()})
    # qtl.scan_vc: patterns of missing phenotypes, its own sweep, its own column map
    ym = y.copy()
    ym[3, 1] = np.nan
    whole = qtl.scan_vc(ctx, ped, ym, cov=cov, permutations=4, seed=2)
    assert whole["n_columns"] == 8 and np.array_equal(whole["col"], col)
    for k, w in (("lod", "lod"), ("h", "h"), ("sigma2", "sigma2_e"), ("blup", "blup")):
        assert np.array_equal(whole[w][[0, 2]], base[k][[0, 2]]), k
    assert np.array_equal(whole["rank"][0], base["rank"]) and np.array_equal(whole["eval"][2], base["eval"])
    np.testing.assert_array_equal(whole["sigma2_u"], whole["h"] / (1 - whole["h"]) * whole["sigma2_e"])
    assert whole["n_used"].tolist() == [[n, n], [n - 1, n - 1], [n, n]] and whole["perm_max"].shape == (4, 3, C)
    use = np.ones(n, bool)
    use[3] = False
    one = ctx.qtl_scan_vc(rows, col, 8, np.where(use, ym[:, 1], 0.0), cov=cov, use=use)
    assert np.array_equal(whole["lod"][1], one["lod"][0])
    thr = qtl.thresholds(whole["perm_max"])["genome"]
    assert thr.shape == (2, 3) and np.all(thr >= 0)
    found = qtl.peaks(whole["lod"], np.arange(M, dtype=np.float64), ped.chromstarts, thr[0])
    assert all(0 <= f["marker"] < M for f in found)


def test_refusals_write_nothing(cross):
    ctx, ped, rows, col = cross
    n, M = len(ped.dous), ped.n_markers
    rows = np.ascontiguousarray(rows)
    y, cov, use = np.ones((n, 2)), np.ones((n, 1)), np.ones(n, np.uint8)
    perm = np.ascontiguousarray(qtl.permutations(n, 2, 1), np.int32)
    outs = [np.full((2, M), 7.0), np.full((2, M), 7.0), np.full((2, M), 7.0), np.full((2, M, 8), 7.0), np.full((M, 8), 7.0),
            np.full(M, 7, np.int32), np.full((2, 2), 7.0), np.full(2, 7, np.int32), np.full((2, 2, 2), 7.0)]
    p = lambda a: a.ctypes.data
    good = [n, p(rows), p(col), 8, 2, p(y), p(use), 1, p(cov), 2, p(perm)] + [p(a) for a in outs] + [0]
    high, low, nan_y, bad_perm = col.copy(), col.copy(), y.copy(), perm.copy()
    high[4, 1], low[4, 1], nan_y[2, 0] = 8, -2, np.nan
    bad_perm[1, 0] = bad_perm[1, 1]
    changes = [(0, 0), (1, None), (2, None), (3, 0), (3, 65), (4, 0), (5, None), (7, 9), (7, -1), (8, None), (9, -1), (10, None), (19, None),
               (11, None), (12, None), (13, None), (16, None), (17, None), (18, None), (2, p(high)), (2, p(low)), (5, p(nan_y)),
               (10, p(bad_perm)), (20, 1 << 23)]
    for k, v in changes:
        args = list(good)
        args[k] = v
        if (k, v) == (20, 1 << 23):
            args[1] = p(rows) + 8          # device rows must be aligned to 16 bytes (refused before anything is read)
        assert ctx.L.cnf2_qtl_scan_vc(ctx.h, *args) == -2, (k, v)
        for a in outs:
            assert np.all(a == 7)
    assert ctx.L.cnf2_qtl_scan_vc(ctx.h, *good) == 0 and not np.any(outs[0] == 7)
    empty = type(ctx)(0)
    assert empty.L.cnf2_qtl_scan_vc(empty.h, *good) == -3      # CNF2_ERR_STATE: no map
    empty.close()


# ---------------------------------------------------------------------------------------------- 4. planted truth
from test_gpu_qtlhap import PLANT_ARGS, PLANT_BETA, PLANT_MARKER, PLANT_NOISE, PLANT_SEED      # noqa: E402


def test_planted_truth(capi):
    """The founder-haplotype suite's planted trait: sum_h beta_h Z_m*[i][h] + noise at marker 8; the seed was chosen on the
    oracle's rows (tests/test_qtlvc_host.py asserts the reference's maximum there).  Here the reference's maximum on the swept
    rows is at the planted marker, asserted first, and so is the GPU run's, with the reference's LOD; it is above the 0.95
    quantile of its own 200 permutations; its LOD and threshold are printed beside scan_hap's (recorded in DESIGN.md, not
    asserted against each other)."""
    ped, truth = synth.make_founder_cross(*PLANT_ARGS)
    n, m_star = len(ped.dous), PLANT_MARKER
    Z = np.zeros((n, 8))
    for s in range(2):
        np.add.at(Z, (np.arange(n), 4 * s + truth[:, s, m_star]), 1.0)
    y = Z @ PLANT_BETA + PLANT_NOISE * np.random.default_rng(PLANT_SEED).normal(size=n)
    # the reference first, on the swept rows: its maximum is at the planted marker
    col, _ = origins.descent_columns(ped.par, ped.dous)
    want = ref.scan(swept(capi, PLANT_ARGS)[2], col, 8, y, ped.chromstarts)
    assert int(want["lod"][0].argmax()) == m_star and want["compared"][0, m_star]
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = qtl.descent_rows(ctx)
    vc = qtl.scan_vc(ctx, ped, y, permutations=200, seed=PLANT_SEED, rows=rows)
    hap = qtl.scan_hap(ctx, ped, y, permutations=200, seed=PLANT_SEED, rows=rows)
    ctx.close()
    lod = vc["lod"][0]
    peak = int(lod.argmax())
    thr = qtl.thresholds(vc["perm_max"], alpha=(0.05,))["genome"][0, 0]
    thr_hap = qtl.thresholds(hap["perm_max"], alpha=(0.05,))["genome"][0, 0]
    cs = ped.chromstarts
    c = int(np.searchsorted(cs, peak, side="right")) - 1
    seg = np.arange(cs[c], cs[c + 1])
    support = seg[lod[seg] >= lod[peak] - 1.5]
    print("variance-component LOD %.2f at marker %d (threshold %.2f), h %.3f, 1.5-LOD interval %d .. %d; founder-haplotype LOD %.2f at marker %d "
          "(threshold %.2f)" % (lod[peak], peak, thr, vc["h"][0, peak], support.min(), support.max(), hap["lod"][0].max(),
                                int(hap["lod"][0].argmax()), thr_hap))
    print("BLUP at the peak:", np.round(vc["blup"][0, peak], 3), "planted:", PLANT_BETA)
    assert np.all(vc["rank"] >= 0)
    assert peak == m_star, "the maximum of the GPU run is at the planted marker, as the reference's is"
    assert abs(lod[peak] - want["lod"][0, m_star]) <= ATOL and abs(vc["h"][0, peak] - want["h"][0, m_star]) <= 1e-5
    assert support.min() <= m_star <= support.max()
    assert lod[peak] > thr
    # the BLUPs show which founder alleles differ: their signs are the planted ones inside each side
    u = vc["blup"][0, peak]
    for s in range(2):
        b = u[4 * s:4 * s + 4] - u[4 * s:4 * s + 4].mean()
        assert np.array_equal(np.sign(b), np.sign(PLANT_BETA[4 * s:4 * s + 4])), s


# ---------------------------------------------------------------------------------------------- 5. command line
def test_cli_qtlvc_figures_and_too_many_founders(capi, tmp_path):
    """The command line's figures on a cross that has some: two families of ten from eight grandparents of their own (16
    columns) on two chromosomes written to files, a trait that follows a marker's dosage and one of noise with a missing
    value, a covariate, 20 permutations.  With --count 1 every n, rank, LOD, h and threshold of the file is qtl.scan_vc's on
    host.Run.from_files of the same files, to the printed digits; the LODs and the h are not all zero and differ from each other
    and between the traits.  Nine families have 36 grandparents: 72 columns are refused with the count, 36 by founder run."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    from test_gpu_cli_multi import write_plantimpute
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    ped = synth.make_outbred3(2, 10, 7, 2, seed=41, missing=0.15)
    d = tmp_path / "two"
    d.mkdir()
    files = write_plantimpute(ped, d)
    n, M, cs = len(ped.dous), ped.n_markers, np.asarray(ped.chromstarts)
    kids = ped.truth[ped.dous].astype(np.float64)                # the children's true dosages: the marker where they vary most
    dos = kids[:, int(kids.var(axis=0).argmax())]
    assert dos.var() > 0.2
    rng = np.random.default_rng(8)
    y = np.stack([2.0 * dos + 0.3 * rng.normal(size=n), rng.normal(size=n)], axis=1)
    y[4, 1] = np.nan
    age = np.round(rng.uniform(size=n) * 10.0, 3)
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    ph = tmp_path / "pheno.txt"
    ph.write_text("id w age z\n" + "".join("%s %s %s %s\n" % (ped.names[ped.dous[i]], cell(y[i, 0]), cell(age[i]), cell(y[i, 1])) for i in range(n)))
    q = tmp_path / "q.txt"
    tail = ["--quiet", "--count", "1", "--phenofile", str(ph), "--qtl-covariates", "age", "--qtl-permutations", "20", "--qtl-seed", "9"]
    subprocess.run([exe] + files + ["--output", str(tmp_path / "o.txt"), "--qtlvc", str(q)] + tail, capture_output=True, text=True, timeout=600,
                   check=True, cwd=str(tmp_path))
    blocks = q.read_text().split("\n\n")
    rows = [ln.split("\t") for ln in blocks[0].split("\n")]
    assert len(rows) == M and all(len(r) == 4 + 2 * 2 for r in rows)
    assert [int(r[0]) for r in rows] == list(np.repeat([1, 2], np.diff(cs)))
    vals = np.array([[float(v) for v in r[4:]] for r in rows])
    lod, h = vals[:, 0::2].T, vals[:, 1::2].T
    thr = [ln.split("\t") for ln in blocks[1].strip("\n").split("\n")]
    assert [r[0] for r in thr] == ["w", "z"]
    thr = np.array([[float(r[1]), float(r[2])] for r in thr])
    r = host.Run.from_files(*files[1::2])
    assert (r.M, r.n_chrom, r.n_dous) == (M, 2, n)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    col, grand = origins.descent_columns(ped.par, ped.dous)
    assert len(grand) == 8
    want = qtl.scan_vc(ctx, None, y, cov=age, col=col, n_columns=16, permutations=20, seed=9)
    ctx.close()
    r.close()
    wthr = qtl.thresholds(want["perm_max"])["genome"].T
    print("file against qtl.scan_vc: lod %.3g (largest %.2f), h %.3g (largest %.3f), thresholds %.3g (%s)"
          % (np.abs(lod - want["lod"]).max(), want["lod"].max(), np.abs(h - want["h"]).max(), want["h"].max(), np.abs(thr - wthr).max(), wthr.round(2).tolist()))
    assert want["n_used"].tolist() == [[n, n], [n - 1, n - 1]] and (want["lod"][0] > 0).any() and (want["lod"][1] > 0).any()
    assert [int(x[2]) for x in rows] == [n] * M and np.array_equal([int(x[3]) for x in rows], want["rank"][0]) and want["rank"].min() >= 1
    np.testing.assert_allclose(lod, want["lod"], rtol=0, atol=0.51e-5)
    np.testing.assert_allclose(h, want["h"], rtol=0, atol=0.51e-5)
    np.testing.assert_allclose(thr, wthr, rtol=0, atol=0.51e-5)
    # (a hundred times the last printed digit: a swap of the LOD and h columns, or of the traits, would show)
    assert np.abs(lod - h).max() > 1e-3 and np.abs(lod[0] - lod[1]).max() > 1e-3 and np.abs(h[0] - h[1]).max() > 1e-3
    assert np.all(thr > 0) and not np.array_equal(thr[0], thr[1])
    # more than 32 phased grandparents
    big = synth.make_outbred3(9, 2, 5, 1, seed=42, missing=0.1)
    d9 = tmp_path / "nine"
    d9.mkdir()
    files9 = write_plantimpute(big, d9)
    ph9 = tmp_path / "pheno9.txt"
    ph9.write_text("id w\n" + "".join("%s %r\n" % (big.names[k], float(i % 5)) for i, k in enumerate(big.dous)))
    args9 = [exe] + files9 + ["--output", str(tmp_path / "o9.txt"), "--quiet", "--count", "1", "--phenofile", str(ph9)]
    bad = subprocess.run(args9 + ["--qtlvc", str(tmp_path / "q9.txt")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert bad.returncode != 0 and "36 grandparents give 72 columns" in bad.stderr and "64" in bad.stderr, bad.stderr[-400:]
    assert not (tmp_path / "q9.txt").exists()
    subprocess.run(args9 + ["--qtlvc", str(tmp_path / "q9f.txt"), "--qtl-vc-by", "founder"], capture_output=True, text=True, timeout=600,
                   check=True, cwd=str(tmp_path))
    assert len((tmp_path / "q9f.txt").read_text().strip("\n").split("\n")) == big.n_markers


def test_cli_qtlvc(capi, tmp_path):
    """cnF2freq --qtlvc on the demo inputs with a phenotype file written here, as the founder-haplotype suite runs --qtlhap:
    --output is the same bytes with and without it; the file parses; with --count 1 its figures are qtl.scan_vc's on
    host.Run.from_files of the same files, to the printed digits.  Two of the demo's three individuals are in the model, too
    few to scan a chromosome: n_used 2, rank 0 and every LOD 0 is what the file must say."""
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
    out_a, out_b, q1, qf = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "q1.txt", tmp_path / "qf.txt"
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    run("--count", "1", "--output", str(out_a))
    run("--count", "1", "--output", str(out_b), "--qtlvc", str(q1), *qargs)
    assert out_a.read_bytes() == out_b.read_bytes()
    run("--count", "1", "--output", str(out_b), "--qtlvc", str(qf), "--qtl-vc-by", "founder", *qargs)
    pos = [float(v) for v in open(files[0]).read().split()]
    M, names = len(pos), ["weight", "height"]

    def parse(path):
        blocks = path.read_text().split("\n\n")
        assert len(blocks) == 2
        rows = [ln.split("\t") for ln in blocks[0].split("\n")]
        assert len(rows) == M and all(len(r) == 4 + 2 * len(names) for r in rows)
        assert all(int(r[0]) == 1 for r in rows) and [float(r[1]) for r in rows] == pos
        assert all(len(v.split(".")[1]) == 5 for r in rows for v in r[4:])
        thr = [ln.split("\t") for ln in blocks[1].strip("\n").split("\n")]
        assert [r[0] for r in thr] == names and all(len(r) == 3 for r in thr)
        vals = np.array([[float(v) for v in r[4:]] for r in rows])
        return (np.array([[int(r[2]), int(r[3])] for r in rows]), vals[:, 0::2].T, vals[:, 1::2].T,
                np.array([[float(r[1]), float(r[2])] for r in thr]))

    parse(qf)
    ints, lod, h, thr = parse(q1)
    r = host.Run.from_files(*files)
    assert (r.M, r.n_chrom, r.n_dous) == (M, 1, 3)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, [0, M], 3)
    pheno = np.array([[1.25, 10.0], [2.5, np.nan], [3.5, 12.0]])                        # C, D, F
    col = np.array([[0, 1, 2, 3, 0, 1, 2, 3], [0, 1, 2, 3, 0, 1, 2, 3], [0, 1, 2, 3, -1, -1, -1, -1]], np.int32)
    want = qtl.scan_vc(ctx, None, pheno, cov=np.array([3.0, 4.0, 5.0]), col=col, n_columns=4, permutations=20, seed=9)
    ctx.close()
    r.close()
    assert np.array_equal(ints[:, 0], np.repeat(want["n_used"][0], M)) and np.array_equal(ints[:, 1], want["rank"][0])
    np.testing.assert_allclose(lod, want["lod"], rtol=0, atol=0.51e-5)
    np.testing.assert_allclose(h, want["h"], rtol=0, atol=0.51e-5)
    np.testing.assert_allclose(thr, qtl.thresholds(want["perm_max"])["genome"].T, rtol=0, atol=0.51e-5)
    assert np.all(ints[:, 0] == 2) and np.all(ints[:, 1] == 0) and np.all(lod == 0.0) and np.all(thr == 0.0)
