"""CPU suite of the linked pair scan (cnf2_qtl_scan2_linked): the synthetic joint of its yardstick
(tests/qtl2_linked_reference.py), the yardstick against the plain one where the two must agree, the host form of one linked
pair (cnf2h_qtl2_pair_linked) against the yardstick, and qtl.pair_summary on a linked scan's arrays."""
import numpy as np
import pytest

from cnf2freq_amd import qtl
from qtl_reference import ATOL, CHROM_LENS, PIVOT_DROP, PIVOT_EXACT, chromstarts_of, noise, soft_rows
from qtl2_reference import reference_scan2
from qtl2_linked_reference import (interaction_columns, linked, product_joint, reference_scan2_linked, synthetic_joint,
                                   zero_cM_case)

SEL = np.arange(sum(CHROM_LENS), dtype=np.int32)[::3]


@pytest.fixture(scope="module")
def case():
    n, K, seed = 40, 2, 5
    origin, _ = soft_rows(n, CHROM_LENS, seed)
    cs = chromstarts_of(CHROM_LENS)
    cov = noise(n, K, seed + 1)
    a = origin[:, :, 3] - origin[:, :, 0]
    pheno = 0.6 * a[:, [3, 40]] + 0.8 * a[:, [20, 40]] * a[:, [30, 60]] + noise(n, 2, seed + 2)
    perm = qtl.permutations(n, 2, seed)
    return origin, cs, cov, pheno, perm, synthetic_joint(origin, cs, SEL)


def test_synthetic_joint(case):
    origin, cs, _, _, _, J = case
    pairs = linked(SEL, cs)
    assert J.shape == (40, len(pairs), 16) and len(pairs) == sum(k * (k - 1) // 2 for k in (1, 1, 5, 5, 6, 11))
    T = J.reshape(40, -1, 4, 4)
    first, second = origin[:, SEL[[p[0] for p in pairs]]], origin[:, SEL[[p[1] for p in pairs]]]
    e = max(np.abs(T.sum(axis=3) - first).max(), np.abs(T.sum(axis=2) - second).max())
    gap = np.abs(J - product_joint(origin, cs, SEL)).max()
    print("margins of the synthetic joint %.3g; it differs from the product by up to %.3f" % (e, gap))
    assert e <= 3e-16 and J.min() >= 0.0 and gap > 0.05
    # the columns of a product joint are the products of the rows' columns
    P = product_joint(origin, cs, SEL)
    o1, o2 = origin[:, SEL[pairs[7][0]]], origin[:, SEL[pairs[7][1]]]
    a1, d1, a2, d2 = o1[:, 3] - o1[:, 0], o1[:, 1] + o1[:, 2], o2[:, 3] - o2[:, 0], o2[:, 1] + o2[:, 2]
    for got, want in zip(interaction_columns(P[:, 7], False), (a1 * a2, a1 * d2, d1 * a2, d1 * d2)):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("additive", [False, True])
def test_linked_reference_against_the_plain_one(case, additive):
    """lod_add, rank_add, rss0, n_used everywhere and lod_full on two chromosomes are the plain reference's; with the product
    as the joint the same-chromosome pairs are fitted what a map with the two loci on two chromosomes would fit them"""
    origin, cs, cov, pheno, perm, J = case
    plain = reference_scan2(origin, cs, SEL, pheno, None, cov, perm, additive)
    ref = reference_scan2_linked(origin, J, cs, SEL, pheno, None, cov, perm, additive)
    for k in ("lod_add", "rank_add", "rss0", "n_used"):
        assert np.array_equal(ref[k], plain[k], equal_nan=True), k
    two = ref["two_chrom"]
    assert np.array_equal(ref["lod_full"][:, :, two], plain["lod_full"][:, :, two]) and np.array_equal(ref["rank_full"][two], plain["rank_full"][two])
    same = ref["upper"] & ~two
    assert same.sum() == len(linked(SEL, cs)) and np.isnan(plain["lod_full"][:, :, same]).all()
    assert np.isfinite(ref["lod_full"][:, :, same]).all() and np.all(ref["lod_full"][:, :, same] >= ref["lod_add"][:, :, same])
    assert np.all(ref["rank_full"][same] >= ref["rank_add"][same])
    assert np.all(ref["perm_max"][:, :, 1] >= plain["perm_max"][:, :, 1])


def fit_pair(origin, J, cs, sel, j, k, pheno, cov, additive):
    from cnf2freq_amd import host
    row = linked(sel, cs).index((j, k))
    return host.qtl2_pair_linked(origin[:, sel[j]], origin[:, sel[k]], J[:, row], pheno, cov=cov, additive=additive)


@pytest.mark.parametrize("additive", [False, True])
def test_host_pair_against_the_yardstick(case, additive):
    import __graft_entry__ as g
    g.build()
    origin, cs, cov, pheno, _, J = case
    ref = reference_scan2_linked(origin, J, cs, SEL, pheno, None, cov, None, additive)
    rp = ref["relpivot"]
    worst = 0.0
    pairs = linked(SEL, cs)
    for j, k in pairs[::3]:
        assert not ((rp[j, k] > PIVOT_EXACT) & (rp[j, k] < 100 * PIVOT_DROP)).any()
        got = fit_pair(origin, J, cs, SEL, j, k, pheno, cov - cov.mean(axis=0), additive)
        assert got["usable"] and (got["rank_add"], got["rank_full"]) == (ref["rank_add"][j, k], ref["rank_full"][j, k])
        worst = max(worst, np.abs(got["lod_add"] - ref["lod_add"][0, :, j, k]).max(), np.abs(got["lod_full"] - ref["lod_full"][0, :, j, k]).max())
    print("cnf2h_qtl2_pair_linked against the yardstick over %d pairs: %.3g" % (len(pairs[::3]), worst))
    assert worst <= ATOL


def test_zero_cM_pair_on_the_host():
    """the pair whose second locus repeats the first, with the diagonal joint: every column the second locus adds is dropped,
    ranks (2, 2), compared with =="""
    import __graft_entry__ as g
    g.build()
    lens, origin, J, sel, pheno = zero_cM_case()
    cs = chromstarts_of(lens)
    ref = reference_scan2_linked(origin, J, cs, sel, pheno)
    rp = ref["relpivot"]
    assert not ((rp > PIVOT_EXACT) & (rp < 100 * PIVOT_DROP)).any()
    assert (ref["rank_add"][0, 1], ref["rank_full"][0, 1]) == (2, 2) and (ref["rank_add"][0, 2], ref["rank_full"][0, 2]) == (4, 8)
    for j, k in ((0, 1), (0, 2), (1, 2)):
        got = fit_pair(origin, J, cs, sel, j, k, pheno, None, False)
        assert (got["rank_add"], got["rank_full"]) == (ref["rank_add"][j, k], ref["rank_full"][j, k])
        assert np.abs(got["lod_full"] - ref["lod_full"][0, :, j, k]).max() <= ATOL


def test_pair_summary_fills_the_diagonal_of_a_linked_scan():
    cs, sel = [0, 3, 5], [0, 2, 3, 4]
    la = np.full((1, 4, 4), np.nan)
    lf = np.full((1, 4, 4), np.nan)
    for (j, k), (a, f) in {(0, 1): (2.0, 5.0), (0, 2): (1.0, 1.5), (0, 3): (3.0, 3.5), (1, 2): (0.5, 0.7), (1, 3): (0.2, 0.9), (2, 3): (1.0, 4.0)}.items():
        la[0, j, k], lf[0, j, k] = a, f
    plain = lf.copy()
    plain[0, 0, 1] = plain[0, 2, 3] = np.nan
    before = qtl.pair_summary(la, plain, sel, cs)
    assert [r["full"] for r in before] == [None, (0, 4), None] and np.isnan(before[0]["lod_int"])
    after = qtl.pair_summary(la, lf, sel, cs)
    assert [(r["chrom1"], r["chrom2"]) for r in after] == [(0, 0), (0, 1), (1, 1)]
    assert after[0]["full"] == (0, 2) and after[0]["lod_full"] == 5.0 and after[0]["lod_add_at_full"] == 2.0 and after[0]["lod_int"] == 3.0
    assert after[2]["full"] == (3, 4) and after[2]["lod_int"] == 3.0
    assert after[1] == before[1]
