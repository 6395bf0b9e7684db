"""GPU suite: the leave-one-marker-out sweep (cnf2_sweep_loo, cnf2_loo_rows, Context.sweep_loo, cnf2freq_amd/qc.py,
cnF2freq --loo).  loo[i][m] = log(sum_s L_s,-m) - log L is checked against the product itself (the log-likelihood of a plain
sweep on the map with column m taken off, minus the full map's), against the oracle's alpha / beta store and emission in
numpy, against the brute-force rows from the product's own store, on the shapes at which the kernel takes another path, for
its bookkeeping, and on planted genotype errors."""
import copy
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cnf2freq_amd import qc, synth
from test_loo_host import fixture_ped, oracle_loo, oracle_unlinked, planted_f2

pytestmark = pytest.mark.gpu

ATOL = 1e-9      # the bar the project asserts on likelihoods
ALL_CASES = ["f2_implicit_f1", "outbred3_missing", "random_windows", "f2_ungenotyped", "ail_ties", "outbred3_two_chrom"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def has_lik(ll):
    return np.isfinite(ll) & (ll > -1e14)


def without_column(ped, m):
    """the pedigree on the map without marker column m, the positions of the others kept"""
    keep = np.setdiff1d(np.arange(ped.n_markers), [m])
    base = copy.copy(ped)
    base.allele, base.sure, base.hw = ped.allele[:, keep], ped.sure[:, keep], ped.hw[:, keep]
    base.pos = np.asarray(ped.pos)[keep]
    cs = np.asarray(ped.chromstarts)
    base.chromstarts = (cs - (cs > m)).astype(np.int32)
    return base


def has_ties(ctx, n):
    return (np.array([ctx.window_info(j)["tie"] for j in range(n)]) >= 0).any()


def close(got, want, what):
    """both CNF2_IGNORED in the same cells, the others within ATOL; returns the cells compared in numbers"""
    ign = want == -1e30
    assert np.array_equal(got == -1e30, ign), what
    err = np.abs(got[~ign] - want[~ign]).max() if (~ign).any() else 0.0
    print("%s: largest difference %.3g over %d cells" % (what, err, int((~ign).sum())))
    assert err <= ATOL, what
    return int((~ign).sum())


_ORACLE = {}


def oracle_of(case):
    """(pedigree, oracle loo, oracle loglik, pairs compared), computed once per fixture and left unchanged"""
    if case not in _ORACLE:
        ped = fixture_ped(case)
        _ORACLE[case] = (ped,) + oracle_loo(ped)
    return _ORACLE[case]


# ---------------------------------------------------------------------------------------------- 1. the product itself
@pytest.mark.parametrize("case", ALL_CASES)
def test_removal_identity(capi, case):
    """loo[:, m] = loglik(map without column m) - loglik(full map), plain cnf2_sweep for both; on a chromosome of
    one marker, where nothing is left to sweep, log(the modes with a likelihood) - loglik: each of them has likelihood 1
    without the marker; every (individual, chromosome) pair is compared"""
    ped = fixture_ped(case)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n = len(ped.dous)
    if case == "ail_ties":
        assert has_ties(ctx, n), "the fixture should hold tied windows"
    got = ctx.sweep_loo()
    ll0 = ctx.sweep(dosage=False)["loglik"]
    assert np.array_equal(got["loglik"], ll0)
    assert has_lik(ll0).all(), "every (individual, chromosome) pair of these fixtures has a likelihood"
    cs = np.asarray(ped.chromstarts)
    worst, cells = 0.0, 0
    aux = capi.Context(0)
    for m in range(ped.n_markers):
        c = int(np.searchsorted(cs, m, side="right")) - 1
        if cs[c + 1] - cs[c] == 1:
            want = np.log((got["factors"][:, c] > -1e14).sum(axis=1)) - ll0[:, c]
        else:
            aux.upload(without_column(ped, m))
            ll1 = aux.sweep(dosage=False)["loglik"][:, c]
            assert has_lik(ll1).all()
            want = ll1 - ll0[:, c]
        worst = max(worst, np.abs(got["loo"][:, m] - want).max())
        cells += n
    aux.close()
    ctx.close()
    print("%s: largest |loo - (loglik_without - loglik_full)| = %.3g over %d cells" % (case, worst, cells))
    assert cells == n * ped.n_markers
    assert worst <= ATOL


# ---------------------------------------------------------------------------------------------- 2. the oracle
@pytest.mark.parametrize("case", ALL_CASES)
def test_against_oracle(capi, case):
    """loo from the oracle's store, unlinked from the oracle's emission, both in numpy; cnf2_loo_rows against both"""
    ped, want, _, compared = oracle_of(case)
    n, C = len(ped.dous), len(ped.chromstarts) - 1
    assert compared == n * C, "no individual of these fixtures is skipped"
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_loo()
    close(got["loo"], want, case + " loo against the oracle")
    active = got["factors"][:, 0, :] > -1e29      # (a masked mode's factor is CNF2_IGNORED on every chromosome)
    unl = oracle_unlinked(ped, active)
    close(got["unlinked"], unl, case + " unlinked against the oracle")
    cs = np.asarray(ped.chromstarts)
    for j in range(n):
        for c in range(C):
            rows = ctx.loo_rows(j, c)
            sl = slice(int(cs[c]), int(cs[c + 1]))
            assert np.abs(rows[:, 0] - got["loo"][j, sl]).max() <= ATOL and np.abs(rows[:, 0] - want[j, sl]).max() <= ATOL
            assert np.abs(rows[:, 1] - got["unlinked"][j, sl]).max() <= ATOL and np.abs(rows[:, 1] - unl[j, sl]).max() <= ATOL
    ctx.close()


def test_unlinked_sum_is_minus_the_placement_null(capi):
    """sum_i unlinked[i][q] = -null[q] of cnf2_sweep_place for the same columns as candidates (nobody is skipped)"""
    ped = fixture_ped("outbred3_two_chrom")
    cols = np.arange(0, ped.n_markers, 3)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_loo()
    assert np.array_equal(got["n_contrib"], [len(ped.dous)] * (len(ped.chromstarts) - 1))
    pl = ctx.sweep_place(np.ascontiguousarray(ped.allele[:, cols]), np.ascontiguousarray(ped.sure[:, cols]),
                         np.ascontiguousarray(ped.hw[:, cols]))
    np.testing.assert_allclose(got["unlinked_sum"][cols], -pl["null"], rtol=1e-12)
    np.testing.assert_allclose(got["unlinked"][:, cols].sum(axis=0), -pl["null"], rtol=1e-12)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 3. shapes
def test_chromosome_lengths_zero_gap_and_flags(capi):
    """chromosomes of 1, 2, 3, 8, 9, 17 and 64 markers in one map (the tile edge at 8, the even and the odd last marker of
    the half spill, the single marker) with a zero-length gap inside the longest, against the oracle; the full spill to
    rounding, static jobs to the bit"""
    ped = synth.make_outbred3(3, 3, 103, 1, seed=13, random_hw=True, random_sure=True)
    assert ped.n_markers == 104
    ped.chromstarts = np.cumsum([0, 1, 2, 3, 8, 9, 17, 64]).astype(np.int32)
    ped.pos = np.asarray(ped.pos, np.float64).copy()
    ped.pos[61] = ped.pos[60]                       # markers 40 .. 103 are the longest chromosome
    n, C = len(ped.dous), 7
    want, ll, compared = oracle_loo(ped)
    assert compared == n * C
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_loo()
    close(got["loo"], want, "loo against the oracle")
    np.testing.assert_allclose(got["loglik"], ll, rtol=1e-9, atol=1e-8)
    # one marker: without it every mode with a likelihood has likelihood 1
    modes = (got["factors"][:, 0] > -1e14).sum(axis=1)
    np.testing.assert_allclose(got["loo"][:, 0], np.log(modes) - got["loglik"][:, 0], rtol=0, atol=ATOL)
    close(got["unlinked"], oracle_unlinked(ped, got["factors"][:, 0, :] > -1e29), "unlinked against the oracle")
    full = ctx.sweep_loo(full_spill=True)
    for k in ("loo", "unlinked", "loo_sum", "unlinked_sum"):
        np.testing.assert_allclose(full[k], got[k], rtol=1e-12, atol=1e-12)
    assert np.array_equal(full["loglik"], ctx.sweep(dosage=False, full_spill=True)["loglik"])
    static = ctx.sweep_loo(static_jobs=True)
    for k in ("factors", "loglik", "loo", "unlinked", "loo_sum", "unlinked_sum", "n_contrib"):
        assert np.array_equal(static[k], got[k]), k
    ctx.close()


def test_ties_general_on_tied_windows(capi):
    ped, want, _, _ = oracle_of("ail_ties")
    ctx = capi.Context(0)
    ctx.upload(ped)
    assert has_ties(ctx, len(ped.dous)), "the fixture should hold tied windows"
    ref = ctx.sweep_loo()
    got = ctx.sweep_loo(ties_general=True)
    assert np.array_equal(got["loglik"], ctx.sweep(dosage=False, ties_general=True)["loglik"])
    np.testing.assert_allclose(got["loglik"], ref["loglik"], rtol=1e-12)
    close(got["loo"], want, "loo with CNF2_TIES_GENERAL against the oracle")
    for k in ("loo", "unlinked", "loo_sum", "unlinked_sum"):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=1e-12)
    assert np.array_equal(got["n_contrib"], ref["n_contrib"])
    ctx.close()


def test_long_chromosome_and_sparse_rescaling_guard(capi):
    """20 F2 individuals on one chromosome of 2 000 markers (the scale exponents run into the thousands), and the data of the
    sparse-rescaling guard's test (tests/test_gpu_parity.py: genotypes that contradict the pedigree with tiny certainties,
    ~1e-24 a marker), both against the oracle"""
    f2 = synth.make_f2(20, 2000, 1, seed=3)
    guard = synth.make_outbred3(2, 2, 60, 1, seed=5, missing=0.0)
    guard.allele, guard.sure = guard.allele.copy(), guard.sure.copy()
    kid = int(guard.dous[0])
    p0, p1 = int(guard.par[kid, 0]), int(guard.par[kid, 1])
    for r, al in ((kid, (2, 2)), (p0, (1, 1)), (p1, (1, 1))):
        guard.allele[guard.row_of[r], 10:50] = al
        guard.sure[guard.row_of[r], 10:50] = 1e-6
    for name, ped in (("F2 20 x 2000", f2), ("rescaling guard", guard)):
        want, ll, compared = oracle_loo(ped)
        assert compared == len(ped.dous)
        if ped is guard:
            assert ll[0, 0] < -400, "the fixture should lose hundreds of log units"
        else:
            assert ll.min() < -710, "some likelihood should lie below a double's range: only the scale exponents hold it"
        ctx = capi.Context(0)
        ctx.upload(ped)
        got = ctx.sweep_loo()
        ctx.close()
        np.testing.assert_allclose(got["loglik"], ll, rtol=1e-9, atol=1e-8)
        close(got["loo"], want, name + " loo against the oracle")


# ---------------------------------------------------------------------------------------------- 4. bookkeeping
def host_sums(rows):
    """the columns added up over the individuals in ascending order, CNF2_IGNORED cells left out: what the device does"""
    s = np.zeros(rows.shape[1])
    for r in rows:
        s = s + np.where(r == -1e30, 0.0, r)
    return s


@pytest.mark.parametrize("tied", [False, True])
def test_bookkeeping(capi, tied):
    import torch
    ped = fixture_ped("ail_ties") if tied else synth.make_outbred3(6, 4, 60, 2, seed=31, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    assert has_ties(ctx, n) == tied
    base = ctx.sweep_loo()
    # factors / loglik: cnf2_sweep's, to the bit
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(base["factors"], plain["factors"])
    assert np.array_equal(base["loglik"], plain["loglik"])
    assert np.array_equal(base["factors"], ctx.sweep()["factors"])
    # the sums: the rows added up in ascending order, to the bit
    assert np.array_equal(base["loo_sum"], host_sums(base["loo"]))
    assert np.array_equal(base["unlinked_sum"], host_sums(base["unlinked"]))
    assert np.array_equal(base["n_contrib"], has_lik(base["loglik"]).sum(axis=0))
    assert np.all(base["loo"] >= -1e-12)
    # a repeated call: the same bits, the sums included
    again = ctx.sweep_loo()
    for k in ("factors", "loglik", "loo", "unlinked", "loo_sum", "unlinked_sum", "n_contrib"):
        assert np.array_equal(again[k], base[k]), k
    # rows NULL: the sums alone, the same bits
    r = ctx.sweep_loo(rows=False)
    assert r["loo"] is None and r["unlinked"] is None
    assert np.array_equal(r["loo_sum"], base["loo_sum"]) and np.array_equal(r["unlinked_sum"], base["unlinked_sum"])
    assert np.array_equal(r["n_contrib"], base["n_contrib"])
    # a split range adds up
    a, b = ctx.sweep_loo(0, n // 3), ctx.sweep_loo(n // 3, n)
    assert np.array_equal(np.concatenate([a["loo"], b["loo"]]), base["loo"])
    assert np.array_equal(np.concatenate([a["unlinked"], b["unlinked"]]), base["unlinked"])
    np.testing.assert_allclose(a["loo_sum"] + b["loo_sum"], base["loo_sum"], rtol=1e-12)
    np.testing.assert_allclose(a["unlinked_sum"] + b["unlinked_sum"], base["unlinked_sum"], rtol=1e-12)
    assert np.array_equal(a["n_contrib"] + b["n_contrib"], base["n_contrib"])
    # an empty range: zeros
    e = ctx.sweep_loo(2, 2)
    assert np.all(e["loo_sum"] == 0) and np.all(e["unlinked_sum"] == 0) and np.all(e["n_contrib"] == 0)
    # CNF2_OUT_DEVICE, with the rows and without
    dev = torch.device("cuda:0")
    d_f = torch.zeros((n, C, 8), dtype=torch.float64, device=dev)
    d_l = torch.zeros((n, C), dtype=torch.float64, device=dev)
    for rows in (True, False):
        d_o = torch.full((n, M), 7.0, dtype=torch.float64, device=dev)
        d_u = torch.full((n, M), 7.0, dtype=torch.float64, device=dev)
        d_os = torch.full((M,), 7.0, dtype=torch.float64, device=dev)
        d_us = torch.full((M,), 7.0, dtype=torch.float64, device=dev)
        d_c = torch.full((C,), 7, dtype=torch.int32, device=dev)
        ctx.sweep_loo_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_o.data_ptr() if rows else None,
                             d_u.data_ptr() if rows else None, d_os.data_ptr(), d_us.data_ptr(), d_c.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        if rows:
            assert np.array_equal(d_o.cpu().numpy(), base["loo"]) and np.array_equal(d_u.cpu().numpy(), base["unlinked"])
        else:
            assert bool((d_o == 7.0).all()) and bool((d_u == 7.0).all())
        assert np.array_equal(d_l.cpu().numpy(), base["loglik"]) and np.array_equal(d_f.cpu().numpy(), base["factors"])
        assert np.array_equal(d_os.cpu().numpy(), base["loo_sum"]) and np.array_equal(d_us.cpu().numpy(), base["unlinked_sum"])
        assert np.array_equal(d_c.cpu().numpy(), base["n_contrib"])
    ctx.close()


def test_bad_arguments_write_nothing(capi):
    ped = synth.make_f2(4, 10, 1, seed=3)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n, M = len(ped.dous), ped.n_markers
    f, l = np.full((n, 1, 8), 7.0), np.full((n, 1), 7.0)
    o, u = np.full((n, M), 7.0), np.full((n, M), 7.0)
    so, su, c = np.full(M, 7.0), np.full(M, 7.0), np.full(1, 7, np.int32)
    p = lambda a: a.ctypes.data
    full = [p(f), p(l), p(o), p(u), p(so), p(su), p(c)]
    calls = [(0, n, full[:k] + [None] + full[k + 1:]) for k in (0, 1, 4, 5, 6)]
    calls += [(-1, n, full), (0, n + 1, full), (3, 2, full)]
    for b, e, ptrs in calls:
        rc = ctx.L.cnf2_sweep_loo(ctx.h, b, e, *ptrs, 0)
        assert rc == -2     # CNF2_ERR_ARG
        for a in (f, l, o, u, so, su, c):
            assert np.all(a == 7)
    rows = np.full((M, 2), 7.0)
    for ind, chrom in ((-1, 0), (n, 0), (0, 1)):
        assert ctx.L.cnf2_loo_rows(ctx.h, ind, chrom, p(rows)) == -2
        assert np.all(rows == 7)
    assert ctx.L.cnf2_loo_rows(ctx.h, 0, 0, None) == -2
    ctx.close()


def test_skipped_individual(capi):
    """F2 without genotyping error: a child with an impossible genotype has no likelihood: CNF2_IGNORED in both arrays, one
    contributor fewer, and the sums leave it out"""
    n, M = 12, 20
    ped = synth.make_f2(n, M, 1, seed=11, sure=0.0)
    skipped = 4
    ped.allele[3 + skipped, 7] = 3            # an allele neither founder carries, without error
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_loo()
    ll = ctx.sweep(dosage=False)["loglik"]
    assert np.array_equal(got["loglik"], ll)
    assert not has_lik(ll[skipped, 0]) and has_lik(np.delete(ll[:, 0], skipped)).all()
    assert np.all(got["loo"][skipped] == capi.IGNORED) and np.all(got["unlinked"][skipped] == capi.IGNORED)
    others = np.delete(np.arange(n), skipped)
    assert np.all(got["loo"][others] > -1e-12) and np.all(got["unlinked"][others] > 0)
    assert np.array_equal(got["n_contrib"], [n - 1])
    assert np.array_equal(got["loo_sum"], host_sums(got["loo"]))
    assert np.array_equal(got["unlinked_sum"], host_sums(got["unlinked"]))
    rows = ctx.loo_rows(skipped, 0)
    assert np.all(rows == capi.IGNORED)
    assert not any(i == skipped for i, _, _ in qc.flag_genotypes(got["loo"], -1.0))
    ctx.close()


# ---------------------------------------------------------------------------------------------- 5. planted errors
def test_planted_errors_stand_out(capi):
    """the 12 planted genotype errors of the 40 x 30 F2 (shown sound on the oracle in tests/test_loo_host.py) cost more than
    every other cell, and qc.flag_genotypes at 5 nats returns exactly them"""
    ped, planted = planted_f2(40, 30, 7)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_loo()
    ctx.close()
    loo = got["loo"]
    lo, hi = loo[planted].min(), loo[~planted].max()
    print("smallest planted cost %.2f, largest other cost %.2f" % (lo, hi))
    assert lo > hi
    flagged = qc.flag_genotypes(loo, 5.0)
    assert [(i, m) for i, m, _ in flagged] == [(int(i), int(m)) for i, m in zip(*np.nonzero(planted))]
    rep = qc.marker_report(got["loo_sum"], got["unlinked_sum"], got["n_contrib"], ped.chromstarts)
    assert np.all(rep["n"] == 40) and np.all(rep["lod"] > 0)


# ---------------------------------------------------------------------------------------------- 6. command line
EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def run_demo(tmp_path, *extra):
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))


def test_cli_loo(capi, tmp_path):
    """cnF2freq --loo on the demo inputs: --output unchanged; with a threshold below every cost the file lists every cell
    of the call, and its per-marker lines are qc.marker_report of those rows' sums (to the 5 decimals of the file).
    What this does not show: that the cells themselves are right for the run's last state -- the state after the rounds is
    not available to Python, so the file is checked for agreeing with itself in both of its sections, for its order and
    contributors, and the values of the call by every other test of this file."""
    out_a, out_b, lf = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "loo.txt"
    run_demo(tmp_path, "--output", str(out_a))
    run_demo(tmp_path, "--output", str(out_b), "--loo", str(lf), "--loo-threshold", "-1")
    assert out_a.read_bytes() == out_b.read_bytes()
    pos = [float(v) for v in open(os.path.join(DEMO, "demoplantimpute.map")).read().split()]
    M = len(pos)
    head, cells = lf.read_text().split("\n\n")
    rows = [ln.split("\t") for ln in head.split("\n")]
    assert len(rows) == M and all(len(r) == 5 for r in rows)
    assert all(int(r[0]) == 1 for r in rows) and [float(r[1]) for r in rows] == pos
    flagged = [ln.split("\t") for ln in cells.strip("\n").split("\n")]
    assert all(len(r) == 6 for r in flagged)
    names = []
    for r in flagged:
        if r[0] not in names:
            names.append(r[0])
    assert len(names) == 3 and len(flagged) == 3 * M, "the demo has three analysed individuals, none skipped"
    loo, unl = np.zeros((3, M)), np.zeros((3, M))
    for k, (name, chrom, m, p, cost, off) in enumerate(flagged):
        assert (names.index(name), int(m)) == (k // M, k % M), "by individual, then marker"
        assert int(chrom) == 1 and float(p) == pos[int(m)]
        loo[k // M, k % M], unl[k // M, k % M] = float(cost), float(off)
    assert np.all(loo >= 0) and np.all(unl > 0)
    rep = qc.marker_report(loo.sum(axis=0), unl.sum(axis=0), [3], [0, M])
    assert [int(r[2]) for r in rows] == list(rep["n"])
    # (every figure of the file is rounded to 5 decimals: 3 cells and the line's own rounding)
    np.testing.assert_allclose([float(r[3]) for r in rows], rep["mean_cost"], rtol=0, atol=1.1e-5)
    np.testing.assert_allclose([float(r[4]) for r in rows], rep["lod"], rtol=0, atol=2.5e-5)
    # the default threshold lists exactly the cells at or above 5 nats
    lf2 = tmp_path / "loo2.txt"
    run_demo(tmp_path, "--output", str(out_b), "--loo", str(lf2))
    head2, cells2 = lf2.read_text().split("\n\n")
    assert head2 == head
    want = [r for r in flagged if float(r[4]) >= 5.0]
    assert [ln.split("\t") for ln in cells2.strip("\n").split("\n") if ln] == want
