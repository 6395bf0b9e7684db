"""GPU suite: the descent sweep (cnf2_sweep_descent, cnf2_descent_rows, Context.sweep_descent, origins.descent_calls,
cnF2freq --descent).  descent[i][m][0..7], per side the four classes "grandparent w, strand b" as masked sums of the state
posterior over the modes the dosage rows count, are checked against the oracle's alpha / beta store in numpy
(tests/descent_reference.py), against the brute-force rows from the product's own store on the shapes at which the kernel
takes another path, against the origin sweep of the same context, for their bookkeeping, on a skipped individual, on the
phased founder cross and through the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import origins, synth
from descent_reference import check_identities, founder_cross, oracle_descent, truth_shares
from test_loo_host import fixture_ped

pytestmark = pytest.mark.gpu

ATOL = 1e-9      # the bar the project asserts on likelihoods
ALL_CASES = ["f2_implicit_f1", "outbred3_missing", "random_windows", "f2_ungenotyped", "ail_ties", "outbred3_two_chrom"]
KEYS = ("factors", "loglik", "descent", "n_contrib")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def has_lik(ll):
    return np.isfinite(ll) & (ll > -1e14)


def has_ties(ctx, n):
    return (np.array([ctx.window_info(j)["tie"] for j in range(n)]) >= 0).any()


def close(got, want, what, atol=ATOL):
    err = np.abs(got - want).max()
    print("%s: largest difference %.3g over %d cells" % (what, err, got.size))
    assert got.shape == want.shape and err <= atol, what


def all_descent_rows(ctx, ped):
    """cnf2_descent_rows of every individual and chromosome: [n][M][8]"""
    cs = np.asarray(ped.chromstarts)
    rows = np.zeros((len(ped.dous), ped.n_markers, 8))
    for j in range(len(ped.dous)):
        for c in range(len(cs) - 1):
            rows[j, cs[c]:cs[c + 1]] = ctx.descent_rows(j, c)
    return rows


_ORACLE = {}


def oracle_of(case):
    """(pedigree, oracle rows), computed once per fixture and left unchanged"""
    if case not in _ORACLE:
        ped = fixture_ped(case)
        _ORACLE[case] = (ped, oracle_descent(ped))
    return _ORACLE[case]


# ---------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("case", ALL_CASES)
def test_against_oracle(capi, case):
    """the rows against the oracle's; cnf2_descent_rows against both; the identities with the origin sweep of the same
    context; the likelihoods are cnf2_sweep's, to the bit"""
    ped, ref = oracle_of(case)
    n, C = len(ped.dous), len(ped.chromstarts) - 1
    assert ref["compared"] == n * C, "no individual of these fixtures is skipped"
    ctx = capi.Context(0)
    ctx.upload(ped)
    if case == "ail_ties":
        assert has_ties(ctx, n), "the fixture should hold tied windows"
    if case == "outbred3_two_chrom":
        assert C == 2, "the fixture should have two chromosomes"
    got = ctx.sweep_descent()
    close(got["descent"], ref["descent"], case + " rows against the oracle")
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(got["factors"], plain["factors"]) and np.array_equal(got["loglik"], plain["loglik"])
    assert np.array_equal(got["n_contrib"], [n] * C)
    check_identities(got["descent"], ctx.sweep_origins()["bits"])
    rows = all_descent_rows(ctx, ped)
    close(rows, got["descent"], case + " cnf2_descent_rows against the sweep")
    close(rows, ref["descent"], case + " cnf2_descent_rows against the oracle")
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. shapes
LENGTHS = [1, 1, 2, 2, 3, 3, 7, 7, 8, 8, 9, 9, 17, 17]


def shaped(kind):
    """8 analysed individuals on two chromosomes each of 1, 2, 3, 7, 8, 9 and 17 markers: the tile edge at 8, the even and
    the odd last marker of the half spill's rebuild, the single marker"""
    M = sum(LENGTHS)
    ped = synth.make_f2(8, M - 1, 1, seed=21, missing=0.1) if kind == "f2" else \
        synth.make_outbred3(2, 4, M - 1, 1, seed=23, random_hw=True, random_sure=True)
    assert ped.n_markers == M and len(ped.dous) == 8
    ped.chromstarts = np.cumsum([0] + LENGTHS).astype(np.int32)
    return ped


@pytest.mark.parametrize("kind", ["f2", "outbred3"])
def test_chromosome_lengths_and_flags(capi, kind):
    ped = shaped(kind)
    n, C = 8, len(LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = all_descent_rows(ctx, ped)
    got = ctx.sweep_descent()
    assert np.array_equal(got["n_contrib"], [n] * C)
    close(got["descent"], rows, kind + " rows against cnf2_descent_rows")
    check_identities(got["descent"], ctx.sweep_origins()["bits"])
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(got["factors"], plain["factors"]) and np.array_equal(got["loglik"], plain["loglik"])
    if kind == "f2":
        # inbred grandparents: nothing tells their strands apart
        d = got["descent"]
        for lo in (0, 2, 4, 6):
            np.testing.assert_allclose(d[:, :, lo], d[:, :, lo + 1], rtol=0, atol=1e-12)
    other = ctx.sweep_descent(full_spill=True)
    close(other["descent"], rows, kind + " full_spill rows against cnf2_descent_rows")
    assert np.array_equal(other["loglik"], ctx.sweep(dosage=False, full_spill=True)["loglik"])
    assert np.array_equal(other["n_contrib"], got["n_contrib"])
    static = ctx.sweep_descent(static_jobs=True)
    for k in KEYS:
        assert np.array_equal(static[k], got[k]), k
    ctx.close()


def test_ties_general_on_tied_windows(capi):
    ped, ref = oracle_of("ail_ties")
    ctx = capi.Context(0)
    ctx.upload(ped)
    assert has_ties(ctx, len(ped.dous)), "the fixture should hold tied windows"
    rows = all_descent_rows(ctx, ped)
    base = ctx.sweep_descent()
    got = ctx.sweep_descent(ties_general=True)
    assert np.array_equal(got["loglik"], ctx.sweep(dosage=False, ties_general=True)["loglik"])
    close(got["descent"], rows, "rows with CNF2_TIES_GENERAL against cnf2_descent_rows")
    close(got["descent"], ref["descent"], "rows with CNF2_TIES_GENERAL against the oracle")
    assert np.array_equal(got["n_contrib"], base["n_contrib"])
    ctx.close()


# ---------------------------------------------------------------------------------------------- 3. bookkeeping
@pytest.mark.parametrize("tied", [False, True])
def test_bookkeeping(capi, tied):
    import torch
    ped = fixture_ped("ail_ties") if tied else synth.make_outbred3(6, 4, 60, 2, seed=31, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    assert has_ties(ctx, n) == tied
    base = ctx.sweep_descent()
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(base["factors"], plain["factors"]) and np.array_equal(base["loglik"], plain["loglik"])
    assert np.array_equal(base["n_contrib"], has_lik(base["loglik"]).sum(axis=0))
    # the four identities against the origin sweep of the same context
    org = ctx.sweep_origins()
    check_identities(base["descent"], org["bits"])
    # a repeated call, also after the origin sweep: the same bits
    again = ctx.sweep_descent()
    for k in KEYS:
        assert np.array_equal(again[k], base[k]), k
    # rows NULL: they stay in the context; the counts are the same
    r = ctx.sweep_descent(rows=False)
    assert r["descent"] is None and np.array_equal(r["n_contrib"], base["n_contrib"]) and np.array_equal(r["loglik"], base["loglik"])
    # a split range: rows and counts exactly
    a, b = ctx.sweep_descent(0, n // 3), ctx.sweep_descent(n // 3, n)
    assert np.array_equal(np.concatenate([a["descent"], b["descent"]]), base["descent"])
    assert np.array_equal(a["n_contrib"] + b["n_contrib"], base["n_contrib"])
    # an empty range: zeros
    e = ctx.sweep_descent(2, 2)
    assert e["descent"].shape == (0, M, 8) and np.all(e["n_contrib"] == 0)
    # CNF2_OUT_DEVICE, with the rows and without
    dev = torch.device("cuda:0")
    d_f = torch.zeros((n, C, 8), dtype=torch.float64, device=dev)
    d_l = torch.zeros((n, C), dtype=torch.float64, device=dev)
    for rows in (True, False):
        d_d = torch.full((n, M, 8), 7.0, dtype=torch.float64, device=dev)
        d_c = torch.full((C,), 7, dtype=torch.int32, device=dev)
        ctx.sweep_descent_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_d.data_ptr() if rows else None, d_c.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        if rows:
            assert np.array_equal(d_d.cpu().numpy(), base["descent"])
        else:
            assert bool((d_d == 7.0).all())
        assert np.array_equal(d_l.cpu().numpy(), base["loglik"]) and np.array_equal(d_f.cpu().numpy(), base["factors"])
        assert np.array_equal(d_c.cpu().numpy(), base["n_contrib"])
    ctx.close()


def test_bad_arguments_write_nothing(capi):
    ped = synth.make_f2(4, 10, 1, seed=3)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n, M = len(ped.dous), ped.n_markers
    f, l = np.full((n, 1, 8), 7.0), np.full((n, 1), 7.0)
    d, c = np.full((n, M, 8), 7.0), np.full(1, 7, np.int32)
    p = lambda a: a.ctypes.data
    full = [p(f), p(l), p(d), p(c)]
    calls = [(0, n, full[:k] + [None] + full[k + 1:]) for k in (0, 1, 3)]
    calls += [(-1, n, full), (0, n + 1, full), (3, 2, full)]
    for b0, e0, ptrs in calls:
        rc = ctx.L.cnf2_sweep_descent(ctx.h, b0, e0, *ptrs, 0)
        assert rc == -2     # CNF2_ERR_ARG
        for a in (f, l, d, c):
            assert np.all(a == 7)
    rows = np.full((M, 8), 7.0)
    for ind, chrom in ((-1, 0), (n, 0), (0, 1)):
        assert ctx.L.cnf2_descent_rows(ctx.h, ind, chrom, p(rows)) == -2
        assert np.all(rows == 7)
    assert ctx.L.cnf2_descent_rows(ctx.h, 0, 0, None) == -2
    ctx.close()


# ---------------------------------------------------------------------------------------------- 4. a skipped individual
def test_skipped_individual(capi):
    """F2 without genotyping error: a child with an allele neither founder carries has no likelihood: all-zero rows, one
    contributor fewer"""
    n, M = 12, 20
    ped = synth.make_f2(n, M, 1, seed=11, sure=0.0)
    skipped = 4
    ped.allele[3 + skipped, 7] = 3
    ctx = capi.Context(0)
    ctx.upload(ped)
    ll = ctx.sweep(dosage=False)["loglik"]
    assert np.isnan(ll[skipped, 0]) or ll[skipped, 0] <= capi.MINFACTOR + 16
    others = np.delete(np.arange(n), skipped)
    got = ctx.sweep_descent()
    assert np.array_equal(got["loglik"], ll, equal_nan=True)
    assert np.all(got["descent"][skipped] == 0)
    np.testing.assert_allclose(got["descent"][others].reshape(n - 1, -1, 2, 4).sum(axis=3), 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(got["n_contrib"], [n - 1])
    assert np.all(ctx.descent_rows(skipped, 0) == 0)
    close(ctx.descent_rows(others[0], 0), got["descent"][others[0]], "a neighbour's rows")
    cls, prob = origins.descent_calls(got["descent"])
    assert np.all(cls[skipped] == -1) and np.all(prob[skipped] == 0) and np.all(cls[others] >= 0)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 5. planted truth, positions
def test_phased_founder_cross(capi):
    """synth.make_founder_cross(3, 12, 17, 2, 777, 0.2, 0.98): the rows are the oracle's, and their arg-max names the true
    (grandparent, strand) as often as the oracle's rows do"""
    ped, truth, ref = founder_cross()
    want = truth_shares(ref["descent"], truth)
    assert min(want) >= 0.8, "the fixture should be informative (asserted on the oracle alone)"
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_descent()
    close(got["descent"], ref["descent"], "founder cross rows against the oracle")
    shares = truth_shares(got["descent"], truth)
    print("arg-max class is the true one in %.4f / %.4f of the cells; the oracle's rows: %.4f / %.4f" % (*shares, *want))
    assert shares[0] >= want[0] and shares[1] >= want[1]
    # positions between the markers: blank columns are ordinary markers to the sweep, the real markers' rows stay
    cs = ped.chromstarts
    add = [[(ped.pos[cs[c] + k] + ped.pos[cs[c] + k + 1]) / 2 for k in (1, 6, 11)] for c in range(2)]
    ped2, is_marker = origins.with_positions(ped, add)
    ctx2 = capi.Context(0)
    ctx2.upload(ped2)
    got2 = ctx2.sweep_descent()["descent"]
    ctx2.close()
    close(got2[:, is_marker], got["descent"], "rows at the real markers with positions added")
    np.testing.assert_allclose(got2.reshape(len(ped.dous), -1, 2, 4).sum(axis=3), 1.0, rtol=0, atol=1e-12)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 6. command line
EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def demo_args(count, *extra):
    return [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", str(count), "--quiet", *extra]


def test_cli_descent(capi, tmp_path):
    """cnF2freq --descent on the demo inputs.  --output is the same bytes with and without the flag.  The file parses: per
    analysed individual a header and a row of eight per marker, then a line per chromosome with the contributors.  With
    --count 1 its rows are the call's on the readers' state after postmarkerdata, to the printed digits."""
    import ctypes as C
    from cnf2freq_amd import host
    out_a, out_b, df2 = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "descent2.txt"
    run = lambda args: subprocess.run(args, capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    run(demo_args(2, "--output", str(out_a)))
    run(demo_args(2, "--output", str(out_b), "--descent", str(df2)))
    assert out_a.read_bytes() == out_b.read_bytes()
    M = len(open(os.path.join(DEMO, "demoplantimpute.map")).read().split())

    def parse(path):
        blocks = path.read_text().split("\n\n")
        assert len(blocks) == 4, "three analysed individuals on one chromosome, then the summary"
        rows, names = np.zeros((3, M, 8)), []
        for j, blk in enumerate(blocks[:3]):
            lines = blk.split("\n")
            name, chrom = lines[0].rsplit(":", 1)
            assert int(chrom) == 1 and name not in names and len(lines) == 1 + M
            names.append(name)
            cells = [ln.split("\t") for ln in lines[1:]]
            assert all(len(c) == 8 and len(v.split(".")[1]) == 6 for c in cells for v in c), "no individual of the demo is skipped"
            rows[j] = [[float(v) for v in c] for c in cells]
        assert blocks[3] == "1\t3\n"
        return names, rows

    names, rows2 = parse(df2)
    assert names == ["C", "D", "F"]
    np.testing.assert_allclose(rows2.reshape(3, M, 2, 4).sum(axis=3), 1.0, rtol=0, atol=2.1e-6)      # (four figures rounded to 6 decimals)
    df1 = tmp_path / "descent1.txt"
    run(demo_args(1, "--output", str(out_b), "--descent", str(df1)))
    names, rows1 = parse(df1)
    r = host.Run.from_files(*[os.path.join(DEMO, "demoplantimpute." + e) for e in ("map", "ped", "gen")])
    assert (r.M, r.n_chrom, r.n_dous) == (M, 1, 3)
    r.postmarkerdata()
    f, ll, ds, cnt = np.zeros((3, 1, 8)), np.zeros((3, 1)), np.zeros((3, M, 8)), np.zeros(1, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = capi.load().cnf2_sweep_descent(C.c_void_p(r.context()), 0, 3, vp(f), vp(ll), vp(ds), vp(cnt), 0)
    assert rc == 0
    r.close()
    assert np.array_equal(cnt, [3])
    print("rows of the file against the call: largest difference %.3g" % np.abs(rows1 - ds).max())
    np.testing.assert_allclose(rows1, ds, rtol=0, atol=0.51e-6)
