"""GPU suite: the pair sweep (cnf2_sweep_pairs, cnf2_pair_rows, cnf2_linked_pairs, Context.sweep_pairs).
joint[i][p][4 u + v], the joint distribution of the origin classes of two markers of one chromosome, is checked against the
yardstick on the CPU oracle's store (tests/pairs_reference.py), against the brute-force rows from the product's own store,
for its identities with the origin and the crossover sweeps, on the shapes at which the kernels take another path, for its
bookkeeping and on a skipped individual."""
import numpy as np
import pytest

from cnf2freq_amd import origins, synth
from pairs_reference import linked, margins, oracle_pairs_of, recombinant_mass
from test_gpu_origins import ALL_CASES, ATOL, LENGTHS, close, has_lik, has_ties, host_sums, shaped
from test_loo_host import fixture_ped

pytestmark = pytest.mark.gpu

KEYS = ("factors", "loglik", "joint", "joint_sum", "n_contrib")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def all_pair_rows(ctx, ped, sel):
    """cnf2_pair_rows of every individual and chromosome, in the order of sweep_pairs' rows: [n][n_pairs][16]"""
    n, C = len(ped.dous), len(ped.chromstarts) - 1
    return np.stack([np.concatenate([ctx.pair_rows(j, c, sel) for c in range(C)]) for j in range(n)])


def check_rows(joint):
    np.testing.assert_allclose(joint.sum(axis=2), 1.0, rtol=0, atol=1e-12)
    assert joint.min() >= 0.0


# ---------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("case", ALL_CASES)
def test_against_oracle(capi, case):
    """every marker selected; the sweep and cnf2_pair_rows against the yardstick for every individual and chromosome; the
    likelihoods are cnf2_sweep's, to the bit"""
    ped, want, pairs, compared = oracle_pairs_of(case)
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    assert compared == n * C, "no individual of these fixtures is skipped"
    sel = np.arange(M, dtype=np.int32)
    ctx = capi.Context(0)
    ctx.upload(ped)
    if case == "ail_ties":
        assert has_ties(ctx, n), "the fixture should hold tied windows"
    assert np.array_equal(ctx.linked_pairs(sel), pairs) and np.array_equal(origins.linked_pairs(sel, ped.chromstarts), pairs)
    got = ctx.sweep_pairs(sel)
    close(got["joint"], want, case + " joint against the yardstick")
    check_rows(got["joint"])
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(got["factors"], plain["factors"]) and np.array_equal(got["loglik"], plain["loglik"])
    assert np.array_equal(got["n_contrib"], [n] * C)
    rows = all_pair_rows(ctx, ped, sel)
    close(rows, got["joint"], case + " cnf2_pair_rows against the sweep")
    close(rows, want, case + " cnf2_pair_rows against the yardstick")
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. identities
@pytest.mark.parametrize("case", ["outbred3_two_chrom", "ail_ties"])
def test_identities(capi, case):
    """rows sum to 1; the margins are the origin rows of the same context; for adjacent markers the mass in which a side's
    class bit differs is that side's crossover posterior"""
    ped = fixture_ped(case)
    sel = np.arange(ped.n_markers, dtype=np.int32)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_pairs(sel)
    org = ctx.sweep_origins()["origin"]
    xi = ctx.sweep_crossovers()["xo"]
    pairs = ctx.linked_pairs(sel)
    ctx.close()
    check_rows(got["joint"])
    first, second = margins(got["joint"])
    close(first, org[:, pairs[:, 0]], case + " first margin against sweep_origins")
    close(second, org[:, pairs[:, 1]], case + " second margin against sweep_origins")
    adj = np.flatnonzero(pairs[:, 1] == pairs[:, 0] + 1)
    assert len(adj) == ped.n_markers - (len(ped.chromstarts) - 1)
    r0, r3 = recombinant_mass(got["joint"][:, adj])
    close(r0, xi[:, pairs[adj, 0], 0], case + " adjacent pairs against xi[0]")
    close(r3, xi[:, pairs[adj, 0], 3], case + " adjacent pairs against xi[3]")


# ---------------------------------------------------------------------------------------------- 3. shapes
def selections():
    """selections on chromosomes of 1, 1, 2, 2, 3, 3, 7, 7, 8, 8, 9, 9, 17 and 17 markers"""
    cs = np.cumsum([0] + LENGTHS)
    M = cs[-1]
    ends = np.concatenate([[cs[c], cs[c + 1] - 1] for c in range(len(LENGTHS)) if LENGTHS[c] > 1])
    return {"all": np.arange(M),
            "first and last": ends,
            "two adjacent": np.array([cs[12] + 7, cs[12] + 8]),
            "one marker on a chromosome": np.array([cs[6] + 3, cs[8] + 1, cs[8] + 7, cs[10] + 4]),
            "every third": np.concatenate([np.arange(cs[c], cs[c + 1], 3) for c in range(len(LENGTHS))])}


@pytest.mark.parametrize("kind", ["f2", "outbred3"])
def test_chromosome_lengths_and_selections(capi, kind):
    ped = shaped(kind)
    n, C = 8, len(LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    for name, sel in selections().items():
        sel = sel.astype(np.int32)
        want_pairs = linked(sel, ped.chromstarts)
        pairs = ctx.linked_pairs(sel)
        assert pairs.tolist() == [list(p) for p in want_pairs] and len(pairs) > 0, name
        got = ctx.sweep_pairs(sel)
        assert got["joint"].shape == (n, len(pairs), 16)
        rows = all_pair_rows(ctx, ped, sel)
        close(got["joint"], rows, "%s, %s: joint against cnf2_pair_rows" % (kind, name))
        check_rows(got["joint"])
        assert np.array_equal(got["n_contrib"], [n] * C)
        static = ctx.sweep_pairs(sel, static_jobs=True)
        for k in KEYS:
            assert np.array_equal(static[k], got[k]), (name, k)
    ctx.close()


@pytest.mark.parametrize("kind", ["f2", "outbred3"])
def test_a_gap_of_zero_cM(capi, kind):
    """two markers at one position: nothing recombines between them, so the joint of that pair is diagonal in each class bit,
    and the cells off it are zero to the bit"""
    ped = shaped(kind)
    cs = ped.chromstarts
    ped.pos = np.array(ped.pos, np.float64)
    m = int(cs[12]) + 5
    ped.pos[m + 1] = ped.pos[m]
    sel = np.arange(cs[12], cs[13], dtype=np.int32)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_pairs(sel)["joint"]
    rows = all_pair_rows(ctx, ped, sel)
    pairs = ctx.linked_pairs(sel)
    ctx.close()
    close(got, rows, kind + " with a gap of 0 cM: joint against cnf2_pair_rows")
    check_rows(got)
    p = int(np.flatnonzero((sel[pairs[:, 0]] == m) & (sel[pairs[:, 1]] == m + 1))[0])
    u, v = np.divmod(np.arange(16), 4)
    assert np.all(got[:, p][:, u != v] == 0.0) and np.all(rows[:, p][:, u != v] == 0.0)
    assert np.all(got[:, p][:, u == v].sum(axis=1) > 0.999999)


# ---------------------------------------------------------------------------------------------- 4. bookkeeping
@pytest.mark.parametrize("tied", [False, True])
def test_bookkeeping(capi, tied):
    import torch
    ped = fixture_ped("ail_ties") if tied else synth.make_outbred3(6, 4, 60, 2, seed=31, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    assert has_ties(ctx, n) == tied
    sel = np.arange(0, M, 2 if tied else 5, dtype=np.int32)
    NP = len(origins.linked_pairs(sel, ped.chromstarts))
    base = ctx.sweep_pairs(sel)
    assert base["joint"].shape == (n, NP, 16) and NP > 0
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(base["factors"], plain["factors"]) and np.array_equal(base["loglik"], plain["loglik"])
    check_rows(base["joint"])
    # the sums: the rows added up in ascending order, to the bit
    assert np.array_equal(base["joint_sum"], host_sums(base["joint"]))
    assert np.array_equal(base["n_contrib"], has_lik(base["loglik"]).sum(axis=0))
    # a repeated call and another batch size: the same bits, the sums included
    again = ctx.sweep_pairs(sel)
    ctx.set_batch_jobs(5)
    small = ctx.sweep_pairs(sel)
    ctx.set_batch_jobs(0)
    static = ctx.sweep_pairs(sel, static_jobs=True)
    for k in KEYS:
        assert np.array_equal(again[k], base[k]), k
        assert np.array_equal(small[k], base[k]), k
        assert np.array_equal(static[k], base[k]), k
    # rows NULL: the sums alone, the same bits
    r = ctx.sweep_pairs(sel, rows=False)
    assert r["joint"] is None
    assert np.array_equal(r["joint_sum"], base["joint_sum"]) and np.array_equal(r["n_contrib"], base["n_contrib"])
    # a split range: rows and counts exactly, sums to rounding
    a, b = ctx.sweep_pairs(sel, 0, n // 3), ctx.sweep_pairs(sel, n // 3, n)
    assert np.array_equal(np.concatenate([a["joint"], b["joint"]]), base["joint"])
    np.testing.assert_allclose(a["joint_sum"] + b["joint_sum"], base["joint_sum"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(a["n_contrib"] + b["n_contrib"], base["n_contrib"])
    # an empty range: zeros
    e = ctx.sweep_pairs(sel, 2, 2)
    assert np.all(e["joint_sum"] == 0) and np.all(e["n_contrib"] == 0)
    if tied:
        gen = ctx.sweep_pairs(sel, ties_general=True)
        close(gen["joint"], base["joint"], "joint with CNF2_TIES_GENERAL")
        close(gen["joint_sum"], base["joint_sum"], "sums with CNF2_TIES_GENERAL")
        assert np.array_equal(gen["n_contrib"], base["n_contrib"])
    # CNF2_OUT_DEVICE, with the rows and without
    dev = torch.device("cuda:0")
    d_f = torch.zeros((n, C, 8), dtype=torch.float64, device=dev)
    d_l = torch.zeros((n, C), dtype=torch.float64, device=dev)
    for rows in (True, False):
        d_j = torch.full((n, NP, 16), 7.0, dtype=torch.float64, device=dev)
        d_s = torch.full((NP, 16), 7.0, dtype=torch.float64, device=dev)
        d_c = torch.full((C,), 7, dtype=torch.int32, device=dev)
        ctx.sweep_pairs_device(0, n, sel, d_f.data_ptr(), d_l.data_ptr(), d_j.data_ptr() if rows else None, d_s.data_ptr(),
                               d_c.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        if rows:
            assert np.array_equal(d_j.cpu().numpy(), base["joint"])
        else:
            assert bool((d_j == 7.0).all())
        assert np.array_equal(d_l.cpu().numpy(), base["loglik"]) and np.array_equal(d_f.cpu().numpy(), base["factors"])
        assert np.array_equal(d_s.cpu().numpy(), base["joint_sum"])
        assert np.array_equal(d_c.cpu().numpy(), base["n_contrib"])
    ctx.close()


def test_bad_arguments_write_nothing(capi):
    ped = synth.make_f2(4, 10, 2, seed=3)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n, M, C = len(ped.dous), ped.n_markers, 2
    cs = ped.chromstarts
    good = np.array([0, 3, 5], np.int32)
    NP = 3
    f, l = np.full((n, C, 8), 7.0), np.full((n, C), 7.0)
    j, s, c = np.full((n, NP, 16), 7.0), np.full((NP, 16), 7.0), np.full(C, 7, np.int32)
    p = lambda a: a.ctypes.data
    full = [p(f), p(l), p(j), p(s), p(c)]

    def refused(b0, e0, sel, ptrs):
        sel = np.asarray(sel, np.int32)
        rc = ctx.L.cnf2_sweep_pairs(ctx.h, b0, e0, len(sel), p(sel) if len(sel) else None, *ptrs, 0)
        assert rc == -2, (b0, e0, sel)     # CNF2_ERR_ARG
        for a in (f, l, j, s, c):
            assert np.all(a == 7)

    for k in (0, 1, 3, 4):
        refused(0, n, good, full[:k] + [None] + full[k + 1:])
    for b0, e0 in ((-1, n), (0, n + 1), (3, 2)):
        refused(b0, e0, good, full)
    # what cnf2_qtl_scan2 refuses in sel, and a selection without a linked pair
    for sel in ([3], [3, 3], [5, 3], [-1, 3], [3, M], [], [int(cs[1]) - 1, int(cs[1])]):
        refused(0, n, sel, full)
    assert ctx.L.cnf2_sweep_pairs(ctx.h, 0, n, 2, None, *full, 0) == -2
    rows = np.full((3, 16), 7.0)
    for ind, chrom in ((-1, 0), (n, 0), (0, 2)):
        assert ctx.L.cnf2_pair_rows(ctx.h, ind, chrom, 3, p(good), p(rows)) == -2
    assert ctx.L.cnf2_pair_rows(ctx.h, 0, 0, 3, p(good), None) == -2
    bad = np.array([5, 3], np.int32)
    assert ctx.L.cnf2_pair_rows(ctx.h, 0, 0, 2, p(bad), p(rows)) == -2
    cnt = np.full(1, 7, np.int32)
    assert ctx.L.cnf2_linked_pairs(ctx.h, 2, p(bad), None, p(cnt)) == -2
    assert ctx.L.cnf2_linked_pairs(ctx.h, 3, p(good), None, None) == -2
    assert np.all(rows == 7) and cnt[0] == 7
    # a selection without a linked pair is a valid question to cnf2_linked_pairs: none
    assert ctx.linked_pairs([int(cs[1]) - 1, int(cs[1])]).shape == (0, 2)
    ctx.close()


# ---------------------------------------------------------------------------------------------- a skipped individual
def test_skipped_individual(capi):
    """F2 without genotyping error: a child with an allele neither founder carries has no likelihood: all-zero rows, one
    contributor fewer, and the sums leave it out"""
    n, M = 12, 20
    ped = synth.make_f2(n, M, 1, seed=11, sure=0.0)
    skipped = 4
    ped.allele[3 + skipped, 7] = 3
    sel = np.arange(0, M + 1, 3, dtype=np.int32)
    ctx = capi.Context(0)
    ctx.upload(ped)
    ll = ctx.sweep(dosage=False)["loglik"]
    assert np.isnan(ll[skipped, 0]) or ll[skipped, 0] <= capi.MINFACTOR + 16
    others = np.delete(np.arange(n), skipped)
    assert has_lik(ll[others, 0]).all()
    got = ctx.sweep_pairs(sel)
    assert np.array_equal(got["loglik"], ll, equal_nan=True)
    assert np.all(got["joint"][skipped] == 0)
    check_rows(got["joint"][others])
    assert np.array_equal(got["n_contrib"], [n - 1])
    assert np.array_equal(got["joint_sum"], host_sums(got["joint"]))
    np.testing.assert_allclose(got["joint_sum"].sum(axis=1), n - 1, rtol=1e-12)
    assert np.all(ctx.pair_rows(skipped, 0, sel) == 0)
    close(ctx.pair_rows(int(others[0]), 0, sel), got["joint"][others[0]], "a neighbour's rows")
    rec = origins.pair_recombination(got["joint_sum"], got["n_contrib"], ctx.linked_pairs(sel), sel, ped.chromstarts)
    assert np.all(rec["n"] == n - 1)
    np.testing.assert_allclose(rec["table"].sum(axis=(1, 2)), 1.0, rtol=1e-12)
    assert np.all((rec["first"] >= 0) & (rec["first"] <= 1) & (rec["second"] >= 0) & (rec["second"] <= 1))
    ctx.close()
