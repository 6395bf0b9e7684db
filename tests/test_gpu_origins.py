"""GPU suite: the origin sweep (cnf2_sweep_origins, cnf2_origin_rows, Context.sweep_origins, cnf2freq_amd/origins.py,
cnF2freq --origins).  origin[i][m][k] and bits[i][m][t], masked sums of the state posterior over the modes the dosage rows
count, are checked against the oracle's alpha / beta store in numpy, against the brute-force rows from the product's own
store, on the fixture that shows the frame to be absolute, on the shapes at which the kernel takes another path, for their
bookkeeping, on a skipped individual, at grid positions, on planted truth and through the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import origins, synth
from test_loo_host import fixture_ped
from test_origins_host import FRAME_CASES, frame_oracle, grid_positions, oracle_origins

pytestmark = pytest.mark.gpu

ATOL = 1e-9      # the bar the project asserts on likelihoods
ALL_CASES = ["f2_implicit_f1", "outbred3_missing", "random_windows", "f2_ungenotyped", "ail_ties", "outbred3_two_chrom"]
KEYS = ("factors", "loglik", "origin", "bits", "origin_sum", "n_contrib")


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


def all_origin_rows(ctx, ped):
    """cnf2_origin_rows of every individual and chromosome: (origin[n][M][4], bits[n][M][6])"""
    cs = np.asarray(ped.chromstarts)
    n, M = len(ped.dous), ped.n_markers
    rows = np.zeros((n, M, 10))
    for j in range(n):
        for c in range(len(cs) - 1):
            rows[j, cs[c]:cs[c + 1]] = ctx.origin_rows(j, c)
    return rows[:, :, :4], rows[:, :, 4:]


_ORACLE = {}


def oracle_of(case):
    """(pedigree, oracle origin, oracle bits, oracle loglik, pairs compared), computed once per fixture and left unchanged"""
    if case not in _ORACLE:
        ped = fixture_ped(case)
        _ORACLE[case] = (ped,) + oracle_origins(ped)
    return _ORACLE[case]


def check_identities(got):
    np.testing.assert_allclose(got["origin"].sum(axis=2), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["bits"][:, :, 0], got["origin"][:, :, 1] + got["origin"][:, :, 3], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["bits"][:, :, 3], got["origin"][:, :, 2] + got["origin"][:, :, 3], rtol=0, atol=1e-12)
    assert np.all(got["origin"] >= 0) and np.all(got["bits"] >= 0) and np.all(got["bits"] <= 1 + 1e-12)


# ---------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("case", ALL_CASES)
def test_against_oracle(capi, case):
    """origin and bits from the oracle's store in numpy; cnf2_origin_rows against the sweep and the oracle, for every
    individual and chromosome; the likelihoods are cnf2_sweep's, to the bit"""
    ped, want_o, want_b, _, compared = oracle_of(case)
    n, C = len(ped.dous), len(ped.chromstarts) - 1
    assert compared == n * C, "no individual of these fixtures is skipped"
    ctx = capi.Context(0)
    ctx.upload(ped)
    if case == "ail_ties":
        assert has_ties(ctx, n), "the fixture should hold tied windows"
    if case == "outbred3_two_chrom":
        assert C == 2, "the fixture should have two chromosomes"
    got = ctx.sweep_origins()
    close(got["origin"], want_o, case + " origin against the oracle")
    close(got["bits"], want_b, case + " bits against the oracle")
    check_identities(got)
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(got["factors"], plain["factors"]) and np.array_equal(got["loglik"], plain["loglik"])
    assert np.array_equal(got["n_contrib"], [n] * C)
    ro, rb = all_origin_rows(ctx, ped)
    close(ro, got["origin"], case + " cnf2_origin_rows origin against the sweep")
    close(rb, got["bits"], case + " cnf2_origin_rows bits against the sweep")
    close(ro, want_o, case + " cnf2_origin_rows origin against the oracle")
    close(rb, want_b, case + " cnf2_origin_rows bits against the oracle")
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. the frame
@pytest.mark.parametrize("side,order", FRAME_CASES)
def test_frame_fixture(capi, side, order):
    """the fixture of tests/test_origins_host.py, where the oracle shows which way the bits point: the product agrees with
    the oracle, and decides "> 0.5" the same way in every cell where the oracle is more than 1e-6 from 0.5"""
    ped, carries_b, want_o, want_b = frame_oracle(side, order)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_origins()
    ctx.close()
    close(got["origin"], want_o, "frame fixture origin")
    close(got["bits"], want_b, "frame fixture bits")
    decided = np.abs(want_b - 0.5) > 1e-6
    assert decided[:, :, 0 if side == 0 else 3].all()
    assert np.array_equal((got["bits"] > 0.5)[decided], (want_b > 0.5)[decided])
    t = 0 if side == 0 else 3
    agree = ((got["bits"][:, :, t] > 0.5) == carries_b).mean()
    assert agree >= 0.95 if order == (0, 1) else agree <= 0.05


# ---------------------------------------------------------------------------------------------- 3. shapes
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
    ro, rb = all_origin_rows(ctx, ped)
    got = ctx.sweep_origins()
    assert np.array_equal(got["n_contrib"], [n] * C)
    close(got["origin"], ro, kind + " origin against cnf2_origin_rows")
    close(got["bits"], rb, kind + " bits against cnf2_origin_rows")
    check_identities(got)
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(got["factors"], plain["factors"]) and np.array_equal(got["loglik"], plain["loglik"])
    for flag in ("full_spill", "all_states"):
        other = ctx.sweep_origins(**{flag: True})
        close(other["origin"], ro, "%s %s origin against cnf2_origin_rows" % (kind, flag))
        close(other["bits"], rb, "%s %s bits against cnf2_origin_rows" % (kind, flag))
        assert np.array_equal(other["loglik"], ctx.sweep(dosage=False, **{flag: True})["loglik"])
        assert np.array_equal(other["n_contrib"], got["n_contrib"])
    static = ctx.sweep_origins(static_jobs=True)
    for k in KEYS:
        assert np.array_equal(static[k], got[k]), k
    ctx.close()


def test_ties_general_on_tied_windows(capi):
    ped, want_o, want_b, _, _ = oracle_of("ail_ties")
    ctx = capi.Context(0)
    ctx.upload(ped)
    assert has_ties(ctx, len(ped.dous)), "the fixture should hold tied windows"
    ro, rb = all_origin_rows(ctx, ped)
    ref = ctx.sweep_origins()
    got = ctx.sweep_origins(ties_general=True)
    assert np.array_equal(got["loglik"], ctx.sweep(dosage=False, ties_general=True)["loglik"])
    close(got["origin"], ro, "origin with CNF2_TIES_GENERAL against cnf2_origin_rows")
    close(got["bits"], rb, "bits with CNF2_TIES_GENERAL against cnf2_origin_rows")
    close(got["origin"], want_o, "origin with CNF2_TIES_GENERAL against the oracle")
    close(got["origin_sum"], ref["origin_sum"], "sums with CNF2_TIES_GENERAL", atol=1e-9)
    assert np.array_equal(got["n_contrib"], ref["n_contrib"])
    ctx.close()


# ---------------------------------------------------------------------------------------------- 4., 5. likelihoods, bookkeeping
def host_sums(rows):
    """the columns added up over the individuals in ascending order: what the device does"""
    s = np.zeros(rows.shape[1:])
    for r in rows:
        s = s + r
    return s


@pytest.mark.parametrize("tied", [False, True])
def test_bookkeeping(capi, tied):
    import torch
    ped = fixture_ped("ail_ties") if tied else synth.make_outbred3(6, 4, 60, 2, seed=31, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    assert has_ties(ctx, n) == tied
    base = ctx.sweep_origins()
    # factors / loglik: cnf2_sweep's, to the bit
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(base["factors"], plain["factors"])
    assert np.array_equal(base["loglik"], plain["loglik"])
    # rows sum to 1, the identities between bits and origin
    check_identities(base)
    # the sums: the rows added up in ascending order, to the bit
    assert np.array_equal(base["origin_sum"], host_sums(base["origin"]))
    assert np.array_equal(base["n_contrib"], has_lik(base["loglik"]).sum(axis=0))
    # a repeated call: the same bits, the sums included
    again = ctx.sweep_origins()
    for k in KEYS:
        assert np.array_equal(again[k], base[k]), k
    # rows NULL: the sums alone, the same bits
    r = ctx.sweep_origins(rows=False)
    assert r["origin"] is None and r["bits"] is None
    assert np.array_equal(r["origin_sum"], base["origin_sum"]) and np.array_equal(r["n_contrib"], base["n_contrib"])
    # a split range: rows and counts exactly, sums to rounding
    a, b = ctx.sweep_origins(0, n // 3), ctx.sweep_origins(n // 3, n)
    assert np.array_equal(np.concatenate([a["origin"], b["origin"]]), base["origin"])
    assert np.array_equal(np.concatenate([a["bits"], b["bits"]]), base["bits"])
    np.testing.assert_allclose(a["origin_sum"] + b["origin_sum"], base["origin_sum"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(a["n_contrib"] + b["n_contrib"], base["n_contrib"])
    # an empty range: zeros
    e = ctx.sweep_origins(2, 2)
    assert np.all(e["origin_sum"] == 0) and np.all(e["n_contrib"] == 0)
    # CNF2_OUT_DEVICE, with the rows and without
    dev = torch.device("cuda:0")
    d_f = torch.zeros((n, C, 8), dtype=torch.float64, device=dev)
    d_l = torch.zeros((n, C), dtype=torch.float64, device=dev)
    for rows in (True, False):
        d_o = torch.full((n, M, 4), 7.0, dtype=torch.float64, device=dev)
        d_b = torch.full((n, M, 6), 7.0, dtype=torch.float64, device=dev)
        d_s = torch.full((M, 4), 7.0, dtype=torch.float64, device=dev)
        d_c = torch.full((C,), 7, dtype=torch.int32, device=dev)
        ctx.sweep_origins_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_o.data_ptr() if rows else None,
                                 d_b.data_ptr() if rows else None, d_s.data_ptr(), d_c.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        if rows:
            assert np.array_equal(d_o.cpu().numpy(), base["origin"]) and np.array_equal(d_b.cpu().numpy(), base["bits"])
        else:
            assert bool((d_o == 7.0).all()) and bool((d_b == 7.0).all())
        assert np.array_equal(d_l.cpu().numpy(), base["loglik"]) and np.array_equal(d_f.cpu().numpy(), base["factors"])
        assert np.array_equal(d_s.cpu().numpy(), base["origin_sum"])
        assert np.array_equal(d_c.cpu().numpy(), base["n_contrib"])
    ctx.close()


def test_bad_arguments_write_nothing(capi):
    ped = synth.make_f2(4, 10, 1, seed=3)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n, M = len(ped.dous), ped.n_markers
    f, l = np.full((n, 1, 8), 7.0), np.full((n, 1), 7.0)
    o, b = np.full((n, M, 4), 7.0), np.full((n, M, 6), 7.0)
    s, c = np.full((M, 4), 7.0), np.full(1, 7, np.int32)
    p = lambda a: a.ctypes.data
    full = [p(f), p(l), p(o), p(b), p(s), p(c)]
    calls = [(0, n, full[:k] + [None] + full[k + 1:]) for k in (0, 1, 4, 5)]
    calls += [(-1, n, full), (0, n + 1, full), (3, 2, full)]
    for b0, e0, ptrs in calls:
        rc = ctx.L.cnf2_sweep_origins(ctx.h, b0, e0, *ptrs, 0)
        assert rc == -2     # CNF2_ERR_ARG
        for a in (f, l, o, b, s, c):
            assert np.all(a == 7)
    rows = np.full((M, 10), 7.0)
    for ind, chrom in ((-1, 0), (n, 0), (0, 1)):
        assert ctx.L.cnf2_origin_rows(ctx.h, ind, chrom, p(rows)) == -2
        assert np.all(rows == 7)
    assert ctx.L.cnf2_origin_rows(ctx.h, 0, 0, None) == -2
    ctx.close()


# ---------------------------------------------------------------------------------------------- 6. a skipped individual
def test_skipped_individual(capi):
    """F2 without genotyping error (sure 0 in every member of the window): a child with an allele neither founder carries has
    no likelihood: all-zero rows, one contributor fewer, and the sums leave it out"""
    n, M = 12, 20
    ped = synth.make_f2(n, M, 1, seed=11, sure=0.0)
    skipped = 4
    ped.allele[3 + skipped, 7] = 3
    ctx = capi.Context(0)
    ctx.upload(ped)
    ll = ctx.sweep(dosage=False)["loglik"]
    # (with no live mode the total is the floor plus the logarithm of the analysed modes, log 8 at most: the bound of
    # test_gpu_parity's impossible individual)
    assert np.isnan(ll[skipped, 0]) or ll[skipped, 0] <= capi.MINFACTOR + 16
    others = np.delete(np.arange(n), skipped)
    assert has_lik(ll[others, 0]).all()
    got = ctx.sweep_origins()
    assert np.array_equal(got["loglik"], ll, equal_nan=True)
    assert np.all(got["origin"][skipped] == 0) and np.all(got["bits"][skipped] == 0)
    np.testing.assert_allclose(got["origin"][others].sum(axis=2), 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(got["n_contrib"], [n - 1])
    assert np.array_equal(got["origin_sum"], host_sums(got["origin"]))
    np.testing.assert_allclose(got["origin_sum"].sum(axis=1), n - 1, rtol=1e-12)
    assert np.all(ctx.origin_rows(skipped, 0) == 0)
    close(ctx.origin_rows(others[0], 0)[:, :4], got["origin"][others[0]], "a neighbour's rows")
    # the report counts the contributors, the information content leaves the skipped rows out
    rep = origins.segregation_report(got["origin_sum"], got["n_contrib"], ped.chromstarts)
    assert np.all(rep["n"] == n - 1)
    np.testing.assert_allclose(origins.information_content(got["origin"]), origins.information_content(got["origin"][others]), rtol=1e-12)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 7. grid positions
def test_grid_positions(capi):
    """origins.with_positions on outbred3_missing, a position in every third gap: the rows at the real markers are the plain
    call's, and all rows are the oracle's on the augmented pedigree"""
    ped = fixture_ped("outbred3_missing")
    ped2, is_marker = origins.with_positions(ped, grid_positions(ped))
    assert (~is_marker).sum() >= (ped.n_markers - 1) // 3 - 2 and (~is_marker).sum() >= 2
    ctx = capi.Context(0)
    ctx.upload(ped)
    base = ctx.sweep_origins()
    ctx.close()
    ctx = capi.Context(0)
    ctx.upload(ped2)
    got = ctx.sweep_origins()
    ctx.close()
    close(got["origin"][:, is_marker], base["origin"], "origin at the real markers against the plain call")
    close(got["bits"][:, is_marker], base["bits"], "bits at the real markers against the plain call")
    want_o, want_b, _, compared = oracle_origins(ped2)
    assert compared == len(ped.dous) * (len(ped.chromstarts) - 1)
    close(got["origin"], want_o, "origin on the augmented pedigree against the oracle")
    close(got["bits"], want_b, "bits on the augmented pedigree against the oracle")
    check_identities(got)


# ---------------------------------------------------------------------------------------------- 8. planted truth
def test_planted_truth(capi):
    """make_f2(40, 30, 1, seed=7): the class with the largest line_genotypes probability is the true class g0 + g1 as
    often as the oracle's own rows say, and no less often; the child is unphased, so origin[1] = origin[2]"""
    ped = synth.make_f2(40, 30, 1, seed=7)
    truth = (synth._meiosis(7, 1, 40, ped.pos, ped.chromstarts).astype(int) + synth._meiosis(7, 2, 40, ped.pos, ped.chromstarts))
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_origins()
    ctx.close()
    want_o, _, _, compared = oracle_origins(ped)
    assert compared == 40
    share = (origins.line_genotypes(got["origin"]).argmax(axis=2) == truth).mean()
    share_oracle = (origins.line_genotypes(want_o).argmax(axis=2) == truth).mean()
    print("arg-max class is the true class in %.4f of %d cells; the oracle's rows: %.4f" % (share, truth.size, share_oracle))
    assert share >= share_oracle
    assert share_oracle > 0.9, "the fixture should be informative"
    close(got["origin"], want_o, "origin against the oracle")
    close(got["origin"][:, :, 1], got["origin"][:, :, 2], "origin[1] against origin[2]")
    ic = origins.information_content(got["origin"])
    assert np.all(ic > 0.5) and np.all(ic < 1.6)
    rep = origins.segregation_report(got["origin_sum"], got["n_contrib"], ped.chromstarts)
    assert np.all(rep["n"] == 40)
    np.testing.assert_allclose(rep["expected"].sum(axis=1), 40.0, rtol=1e-12)


# ---------------------------------------------------------------------------------------------- 9. command line
EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def run_demo(tmp_path, *extra):
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))


def test_cli_origins(capi, tmp_path):
    """cnF2freq --origins on the demo inputs.  --output is the same bytes with and without the flag.  The file parses: per
    analysed individual a header and a row per marker, then a line per marker with position, contributors and sums.  Its
    rows are Context.sweep_origins' to the printed digits: with --count 1 the state the call sees is the readers' after
    postmarkerdata, which host.Run.from_files reaches through the same readers; the summary lines are that call's sums."""
    import ctypes as C
    from cnf2freq_amd import host
    out_a, out_b, of2 = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "origins2.txt"
    run_demo(tmp_path, "--output", str(out_a))
    run_demo(tmp_path, "--output", str(out_b), "--origins", str(of2))
    assert out_a.read_bytes() == out_b.read_bytes()
    pos = [float(v) for v in open(os.path.join(DEMO, "demoplantimpute.map")).read().split()]
    M = len(pos)

    def parse(path):
        blocks = path.read_text().split("\n\n")
        assert len(blocks) == 4, "three analysed individuals on one chromosome, then the summary"
        rows, names = np.zeros((3, M, 4)), []
        for j, blk in enumerate(blocks[:3]):
            lines = blk.split("\n")
            name, chrom = lines[0].rsplit(":", 1)
            assert int(chrom) == 1 and name not in names and len(lines) == 1 + M
            names.append(name)
            cells = [ln.split("\t") for ln in lines[1:]]
            assert all(len(c) == 4 and len(v.split(".")[1]) == 6 for c in cells for v in c), "no individual of the demo is skipped"
            rows[j] = [[float(v) for v in c] for c in cells]
        summary = [ln.split("\t") for ln in blocks[3].strip("\n").split("\n")]
        assert len(summary) == M and all(len(r) == 7 for r in summary)
        assert all(int(r[0]) == 1 and int(r[2]) == 3 for r in summary) and [float(r[1]) for r in summary] == pos
        assert all(len(v.split(".")[1]) == 5 for r in summary for v in r[3:])
        return names, rows, np.array([[float(v) for v in r[3:]] for r in summary])

    names, rows2, sums2 = parse(of2)
    assert names == ["C", "D", "F"]
    np.testing.assert_allclose(rows2.sum(axis=2), 1.0, rtol=0, atol=2.1e-6)      # (four figures rounded to 6 decimals)
    np.testing.assert_allclose(sums2, rows2.sum(axis=0), rtol=0, atol=3 * 0.5e-6 + 0.51e-5)
    # --count 1: no round changes the state before the call
    of1 = tmp_path / "origins1.txt"
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "1", "--quiet", "--output", str(out_b), "--origins", str(of1)]
    subprocess.run(args, capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    names, rows1, sums1 = parse(of1)
    run = host.Run.from_files(*[os.path.join(DEMO, "demoplantimpute." + e) for e in ("map", "ped", "gen")])
    assert (run.M, run.n_chrom, run.n_dous) == (M, 1, 3)
    run.postmarkerdata()
    n, Cn = 3, 1
    f, ll = np.zeros((n, Cn, 8)), np.zeros((n, Cn))
    og, bt, os_, cnt = np.zeros((n, M, 4)), np.zeros((n, M, 6)), np.zeros((M, 4)), np.zeros(Cn, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    L = capi.load()
    rc = L.cnf2_sweep_origins(C.c_void_p(run.context()), 0, n, vp(f), vp(ll), vp(og), vp(bt), vp(os_), vp(cnt), 0)
    assert rc == 0
    run.close()
    assert np.array_equal(cnt, [3])
    print("rows of the file against the call: largest difference %.3g" % np.abs(rows1 - og).max())
    np.testing.assert_allclose(rows1, og, rtol=0, atol=0.51e-6)
    np.testing.assert_allclose(sums1, os_, rtol=0, atol=0.51e-5)
