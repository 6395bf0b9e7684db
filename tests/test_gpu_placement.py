"""GPU suite: marker placement (cnf2_sweep_place, Context.sweep_place, cnf2freq_amd/placement.py, cnF2freq --place).
place[i][q][m] = log sum_s w_s sum_g gamma_s,m(g) e'_s,q(g) is checked against the product itself (the log-likelihood of a
plain sweep on the map with the candidate inserted at marker m's position, minus the base map's), against an independent
numpy contraction of the oracle's alpha / beta store with the oracle's emission, for its bookkeeping (sums, counts, range
splits, flags, batches, candidate tiles, chromosome lengths) and on planted positions."""
import copy
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_CASES, ROOT, load_golden, load_trajectory, oracle_ped
from cnf2freq_amd import placement, synth

pytestmark = pytest.mark.gpu

ATOL = 1e-9      # the bar the project asserts on likelihoods


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def fixture_ped(case):
    return load_golden(case)[0] if case in GOLDEN_CASES else load_trajectory(case)[0]


def has_lik(ll):
    return np.isfinite(ll) & (ll > -1e14)


def without_columns(ped, cols):
    """(the pedigree on the map without the marker columns `cols`, their rows as candidates with hw 0.5)"""
    cols = np.asarray(cols)
    keep = np.setdiff1d(np.arange(ped.n_markers), cols)
    base = copy.copy(ped)
    base.allele, base.sure, base.hw = ped.allele[:, keep], ped.sure[:, keep], ped.hw[:, keep]
    base.pos = np.asarray(ped.pos)[keep]
    cs = np.asarray(ped.chromstarts)
    base.chromstarts = (cs - np.array([(cols < c).sum() for c in cs])).astype(np.int32)
    assert np.all(np.diff(base.chromstarts) > 0)
    ca, csr = np.ascontiguousarray(ped.allele[:, cols]), np.ascontiguousarray(ped.sure[:, cols])
    return base, ca, csr, np.full(ca.shape[:2], 0.5)


def with_inserted(base, m, a_col, s_col, h_col):
    """the pedigree with one more marker right after marker m, at pos[m]"""
    aug = copy.copy(base)
    aug.allele = np.insert(base.allele, m + 1, a_col, axis=1)
    aug.sure = np.insert(base.sure, m + 1, s_col, axis=1)
    aug.hw = np.insert(base.hw, m + 1, h_col, axis=1)
    aug.pos = np.insert(np.asarray(base.pos, np.float64), m + 1, base.pos[m])
    cs = np.asarray(base.chromstarts)
    aug.chromstarts = (cs + (cs > m)).astype(np.int32)
    return aug


def candidate_columns(ped, count=3):
    """a handful of the pedigree's own columns, spread over the map, never a chromosome's only marker"""
    cs = np.asarray(ped.chromstarts)
    M = ped.n_markers
    cols = []
    for k in range(count):
        m = int((2 * k + 1) * M // (2 * count))
        c = int(np.searchsorted(cs, m, side="right")) - 1
        if cs[c + 1] - cs[c] - sum(1 for x in cols if cs[c] <= x < cs[c + 1]) > 1 and m not in cols:
            cols.append(m)
    assert cols
    return np.array(cols)


def oracle_emission(ped, ca, csr, ch):
    """E[j][q][s][g] of the analysed individuals from the oracle's emission on the candidate rows"""
    from oracle.pyoracle import OraclePed
    ro = ped.row_of
    oc = OraclePed(ca[ro].astype(np.int32), csr[ro], ch[ro], ped.par, ped.empty, np.arange(ca.shape[1], dtype=np.float64))
    Q = ca.shape[1]
    E = np.zeros((len(ped.dous), Q, 8, 64))
    for j, ind in enumerate(ped.dous):
        for q in range(Q):
            for s in range(8):
                for g in range(64):
                    E[j, q, s, g] = oc.emission(int(ind), q, g, -1, s)
    return E


def oracle_place(capi, base, E):
    """place[n][Q][M] by contracting the oracle's store with E: the weights and the 40-log-unit rule of oracle_xi in
    tests/test_gpu_crossovers.py.  Returns (place, the (individual, chromosome) pairs compared in numbers: those the oracle
    does not skip and that have a mode with a likelihood)."""
    o = oracle_ped(base)
    cs = np.asarray(base.chromstarts)
    n, Q, M = len(base.dous), E.shape[1], base.n_markers
    out = np.zeros((n, Q, M))
    compared = 0
    for j, ind in enumerate(base.dous):
        gen = int(base.gen[ind])
        for c in range(len(cs) - 1):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            res = o.sweep_ind(int(ind), gen, first=first, last=last, mode=2, keep_store=True)
            factor = res["factor"]
            if not res["ok"] or not (factor >= -1e15) or not (res["factors"] > -1e14).any():
                out[j, :, first:last + 1] = capi.IGNORED
                continue
            compared += 1
            fw = res["fwbw"]
            val = np.zeros((Q, last - first + 1))
            for s in range(8):
                fs = res["factors"][s]
                if fs < -1e29 or factor - fs > 40.0 or not (fs > -1e14):
                    continue
                gam = fw[s, first:last + 1, 2] * fw[s, first:last + 1, 1]
                gam = gam / gam.sum(axis=1, keepdims=True)
                val += np.exp(fs - factor) * (E[j, :, s] @ gam.T)
            with np.errstate(divide="ignore"):
                out[j, :, first:last + 1] = np.where(val > 0, np.log(np.where(val > 0, val, 1.0)), capi.MINFACTOR)
    return out, compared


def assert_place_close(got, want, capi):
    special = (want == capi.IGNORED) | (want == capi.MINFACTOR)
    assert np.array_equal(got[special], want[special])
    err = np.abs(got[~special] - want[~special]).max() if (~special).any() else 0.0
    print("largest |place - reference| = %.3g over %d cells" % (err, int((~special).sum())))
    assert (~special).any()
    assert err <= ATOL
    return int((~special).sum())


ALL_CASES = GOLDEN_CASES + ["ail_ties", "outbred3_two_chrom"]


@pytest.mark.parametrize("case", ALL_CASES)
def test_insertion_identity(capi, case):
    """place[i][q][m] = loglik(map with q inserted after m at pos[m]) - loglik(base map), plain cnf2_sweep for both"""
    ped = fixture_ped(case)
    base, ca, csr, ch = without_columns(ped, candidate_columns(ped))
    ctx = capi.Context(0)
    ctx.upload(base)
    if case == "ail_ties":
        tab = np.array([ctx.window_info(j)["tie"] for j in range(len(base.dous))])
        assert (tab >= 0).any(), "the fixture should hold tied windows"
    got = ctx.sweep_place(ca, csr, ch, per_individual=True)
    ll0 = ctx.sweep(dosage=False)["loglik"]
    assert np.array_equal(got["loglik"], ll0)
    cs = np.asarray(base.chromstarts)
    worst, cells = 0.0, 0
    aux = capi.Context(0)
    for q in range(ca.shape[1]):
        for m in range(base.n_markers):
            c = int(np.searchsorted(cs, m, side="right")) - 1
            aug = with_inserted(base, m, ca[:, q], csr[:, q], ch[:, q])
            aux.upload(aug)
            ll1 = aux.sweep(dosage=False)["loglik"][:, c]
            pl = got["place"][:, q, m]
            skipped = ~has_lik(ll0[:, c])
            assert np.all(pl[skipped] == capi.IGNORED)
            dead = ~skipped & ~has_lik(ll1)
            assert np.all(pl[dead] == capi.MINFACTOR)
            live = ~skipped & ~dead
            if live.any():
                worst = max(worst, np.abs(pl[live] - (ll1[live] - ll0[live, c])).max())
                cells += int(live.sum())
    aux.close()
    ctx.close()
    print("%s: largest |place - (loglik_aug - loglik_base)| = %.3g over %d cells" % (case, worst, cells))
    assert cells > 0
    assert worst <= ATOL


@pytest.mark.parametrize("case", ALL_CASES)
def test_against_oracle(capi, case):
    """the same values from the oracle's store and the oracle's emission, in numpy; null_out from the same emission"""
    ped = fixture_ped(case)
    base, ca, csr, ch = without_columns(ped, candidate_columns(ped))
    ctx = capi.Context(0)
    ctx.upload(base)
    got = ctx.sweep_place(ca, csr, ch, per_individual=True)
    E = oracle_emission(base, ca, csr, ch)
    want, compared = oracle_place(capi, base, E)
    assert compared == len(base.dous) * (len(base.chromstarts) - 1), "no individual of these fixtures is skipped"
    assert_place_close(got["place"], want, capi)
    # the unlinked baseline: mean over the analysed modes (a masked mode's factor is CNF2_IGNORED on every chromosome)
    active = got["factors"][:, 0, :] > -1e29
    mean = (E.sum(axis=3) / 64.0 * active[:, None, :]).sum(axis=2) / np.maximum(active.sum(axis=1), 1)[:, None]
    null = np.where(mean > 0, np.log(np.where(mean > 0, mean, 1.0)), 0.0).sum(axis=0)
    np.testing.assert_allclose(got["null"], null, rtol=1e-12)
    ctx.close()


def test_impossible_and_skipped(capi):
    """F2 without genotyping error: a candidate that is Mendelian-impossible for chosen children (both founders 1/1, the
    child 2/2) gives CNF2_MINFACTOR there, n_zero counts exactly them and place_sum leaves them out; a child with an
    impossible genotype on the map itself is skipped: CNF2_IGNORED and one contributor fewer"""
    n, M = 12, 20
    ped = synth.make_f2(n, M, 1, seed=11, sure=0.0)
    skipped_child, bad = 4, [1, 6, 9]
    ped.allele[3 + skipped_child, 7] = 3            # an allele neither founder carries, without error
    rows = ped.allele.shape[0]
    ca = np.zeros((rows, 2, 2), np.uint8)
    csr = np.zeros((rows, 2, 2))
    ca[1:3] = 1                                     # A and B: 1/1 at both candidates
    ca[3:] = 1
    for k in bad:
        ca[3 + k, 0] = 2                            # candidate 0: 2/2 from 1/1 x 1/1 grandparents
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_place(ca, csr, None, per_individual=True)
    ll = ctx.sweep(dosage=False)["loglik"]
    assert not has_lik(ll[skipped_child, 0]) and has_lik(np.delete(ll[:, 0], skipped_child)).all()
    pl = got["place"]
    assert np.all(pl[skipped_child] == capi.IGNORED)
    assert np.array_equal(got["n_contrib"], [n - 1])
    for k in bad:
        assert np.all(pl[k, 0] == capi.MINFACTOR)
    others = [k for k in range(n) if k not in bad and k != skipped_child]
    assert np.all(pl[others] > -1e14) and np.all(pl[bad, 1] > -1e14)
    assert np.all(got["n_zero"][0] == len(bad)) and np.all(got["n_zero"][1] == 0)
    np.testing.assert_allclose(got["place_sum"][0], pl[others, 0].sum(axis=0), rtol=1e-12)
    np.testing.assert_allclose(got["place_sum"][1], pl[others + bad, 1].sum(axis=0), rtol=1e-12)
    ctx.close()


def own_columns_as_candidates(ped, Q, seed=0):
    cols = np.random.default_rng(seed).integers(0, ped.n_markers, Q)
    return np.ascontiguousarray(ped.allele[:, cols]), np.ascontiguousarray(ped.sure[:, cols]), np.ascontiguousarray(ped.hw[:, cols])


def host_sum(place, capi):
    ok = (place != capi.IGNORED) & (place != capi.MINFACTOR)
    return np.where(ok, place, 0.0).sum(axis=0), ((place == capi.MINFACTOR).sum(axis=0)).astype(np.int32)


def test_bookkeeping(capi):
    import torch
    ped = synth.make_outbred3(6, 4, 60, 2, seed=31, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n, M, C = len(ped.dous), ped.n_markers, len(ped.chromstarts) - 1
    ca, csr, ch = own_columns_as_candidates(ped, 37)
    base = ctx.sweep_place(ca, csr, ch, per_individual=True)
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(base["factors"], plain["factors"])
    assert np.array_equal(base["loglik"], plain["loglik"])
    assert np.array_equal(base["factors"], ctx.sweep()["factors"])
    hs, hz = host_sum(base["place"], capi)
    np.testing.assert_allclose(base["place_sum"], hs, rtol=1e-12)
    assert np.array_equal(base["n_zero"], hz)
    assert np.array_equal(base["n_contrib"], has_lik(base["loglik"]).sum(axis=0))
    # two identical calls
    again = ctx.sweep_place(ca, csr, ch, per_individual=True)
    assert np.array_equal(again["place"], base["place"])
    # without the per-individual output
    r = ctx.sweep_place(ca, csr, ch)
    assert r["place"] is None
    np.testing.assert_allclose(r["place_sum"], base["place_sum"], rtol=1e-12)
    np.testing.assert_allclose(r["null"], base["null"], rtol=1e-12)
    # the three flags, to rounding
    for kw in (dict(static_jobs=True), dict(full_spill=True), dict(ties_general=True)):
        r = ctx.sweep_place(ca, csr, ch, per_individual=True, **kw)
        np.testing.assert_allclose(r["place"], base["place"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(r["place_sum"], base["place_sum"], rtol=1e-12, atol=1e-12)
        assert np.array_equal(r["n_zero"], base["n_zero"])
        assert np.array_equal(r["loglik"], ctx.sweep(dosage=False, **kw)["loglik"])
    # a split range adds up
    a = ctx.sweep_place(ca, csr, ch, 0, n // 3, per_individual=True)
    b = ctx.sweep_place(ca, csr, ch, n // 3, n, per_individual=True)
    assert np.array_equal(np.concatenate([a["place"], b["place"]]), base["place"])
    np.testing.assert_allclose(a["place_sum"] + b["place_sum"], base["place_sum"], rtol=1e-12)
    np.testing.assert_allclose(a["null"] + b["null"], base["null"], rtol=1e-12)
    assert np.array_equal(a["n_zero"] + b["n_zero"], base["n_zero"])
    assert np.array_equal(a["n_contrib"] + b["n_contrib"], base["n_contrib"])
    # Q = 1 and 16: the same cells as the first candidates of the 37
    for Q in (1, 16):
        r = ctx.sweep_place(ca[:, :Q], csr[:, :Q], ch[:, :Q], per_individual=True)
        assert r["place"].shape == (n, Q, M)
        np.testing.assert_allclose(r["place"], base["place"][:, :Q], rtol=1e-13, atol=0)
        np.testing.assert_allclose(r["place_sum"], base["place_sum"][:Q], rtol=1e-12)
        np.testing.assert_allclose(r["null"], base["null"][:Q], rtol=1e-12)
    # cand_hw = NULL is 0.5
    r = ctx.sweep_place(ca, csr, None, per_individual=True)
    r2 = ctx.sweep_place(ca, csr, np.full(ch.shape, 0.5), per_individual=True)
    assert np.array_equal(r["place"], r2["place"])
    # CNF2_OUT_DEVICE
    dev = torch.device("cuda:0")
    d_f = torch.zeros((n, C, 8), dtype=torch.float64, device=dev)
    d_l = torch.zeros((n, C), dtype=torch.float64, device=dev)
    d_p = torch.full((n, 37, M), 7.0, dtype=torch.float64, device=dev)
    d_s = torch.full((37, M), 7.0, dtype=torch.float64, device=dev)
    d_z = torch.full((37, M), 7, dtype=torch.int32, device=dev)
    d_n = torch.full((37,), 7.0, dtype=torch.float64, device=dev)
    d_c = torch.full((C,), 7, dtype=torch.int32, device=dev)
    ctx.sweep_place_device(ca, csr, ch, 0, n, d_f.data_ptr(), d_l.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_z.data_ptr(),
                           d_n.data_ptr(), d_c.data_ptr())
    ctx.sync()
    assert np.array_equal(d_p.cpu().numpy(), base["place"])
    assert np.array_equal(d_l.cpu().numpy(), base["loglik"])
    np.testing.assert_allclose(d_s.cpu().numpy(), base["place_sum"], rtol=1e-12)
    np.testing.assert_allclose(d_n.cpu().numpy(), base["null"], rtol=1e-12)
    assert np.array_equal(d_z.cpu().numpy(), base["n_zero"])
    assert np.array_equal(d_c.cpu().numpy(), base["n_contrib"])
    # batches of three jobs against the default
    ctx.set_batch_jobs(3)
    r = ctx.sweep_place(ca, csr, ch, per_individual=True)
    assert np.array_equal(r["place"], base["place"])
    np.testing.assert_allclose(r["place_sum"], base["place_sum"], rtol=1e-12)
    np.testing.assert_allclose(r["null"], base["null"], rtol=1e-12)
    assert np.array_equal(r["n_zero"], base["n_zero"])
    assert np.array_equal(r["n_contrib"], base["n_contrib"])
    ctx.close()


def test_ties_general_on_tied_windows(capi):
    """CNF2_TIES_GENERAL changes the launch that gives the tied windows' likelihoods: on the pedigree that holds some"""
    ped = fixture_ped("ail_ties")
    base, ca, csr, ch = without_columns(ped, candidate_columns(ped))
    ctx = capi.Context(0)
    ctx.upload(base)
    tab = np.array([ctx.window_info(j)["tie"] for j in range(len(base.dous))])
    assert (tab >= 0).any(), "the fixture should hold tied windows"
    ref = ctx.sweep_place(ca, csr, ch, per_individual=True)
    got = ctx.sweep_place(ca, csr, ch, per_individual=True, ties_general=True)
    assert np.array_equal(got["loglik"], ctx.sweep(dosage=False, ties_general=True)["loglik"])
    np.testing.assert_allclose(got["loglik"], ref["loglik"], rtol=1e-12)
    np.testing.assert_allclose(got["place"], ref["place"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["place_sum"], ref["place_sum"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(got["n_zero"], ref["n_zero"])
    ctx.close()


def test_bad_arguments_write_nothing(capi):
    ped = synth.make_f2(4, 10, 1, seed=3)
    ctx = capi.Context(0)
    ctx.upload(ped)
    ca, csr, ch = own_columns_as_candidates(ped, 2)
    n, M = len(ped.dous), ped.n_markers
    f, l = np.full((n, 1, 8), 7.0), np.full((n, 1), 7.0)
    s, z, nl, c = np.full((2, M), 7.0), np.full((2, M), 7, np.int32), np.full(2, 7.0), np.full(1, 7, np.int32)
    p = lambda a: a.ctypes.data
    for q, a_ptr, s_ptr in ((0, p(ca), p(csr)), (2, None, p(csr)), (2, p(ca), None)):
        rc = ctx.L.cnf2_sweep_place(ctx.h, 0, n, q, a_ptr, s_ptr, None, p(f), p(l), None, p(s), p(z), p(nl), p(c), 0)
        assert rc == -2     # CNF2_ERR_ARG
        assert np.all(f == 7) and np.all(l == 7) and np.all(s == 7) and np.all(z == 7) and np.all(nl == 7) and np.all(c == 7)
    ctx.close()


def test_many_candidates_tile_over_the_same_weights(capi):
    """more candidates than the tables held at once (256): the tiles of a call give what smaller calls give"""
    ped = synth.make_outbred3(2, 3, 20, 1, seed=5, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    ca, csr, ch = own_columns_as_candidates(ped, 300, seed=2)
    whole = ctx.sweep_place(ca, csr, ch, per_individual=True)
    ctx.set_batch_jobs(2)
    batched = ctx.sweep_place(ca, csr, ch, per_individual=True)
    ctx.set_batch_jobs(0)
    for lo, hi in ((0, 100), (100, 300)):
        part = ctx.sweep_place(ca[:, lo:hi], csr[:, lo:hi], ch[:, lo:hi], per_individual=True)
        for r in (whole, batched):
            np.testing.assert_allclose(r["place"][:, lo:hi], part["place"], rtol=1e-13, atol=0)
            np.testing.assert_allclose(r["place_sum"][lo:hi], part["place_sum"], rtol=1e-12)
            np.testing.assert_allclose(r["null"][lo:hi], part["null"], rtol=1e-12)
            assert np.array_equal(r["n_zero"][lo:hi], part["n_zero"])
    ctx.close()


def test_chromosome_lengths_1_3_17_64(capi):
    """chromosomes of 1, 3, 17 and 64 markers in one map (tiles of 16 markers are masked, not padded), against the oracle"""
    ped = synth.make_outbred3(3, 3, 84, 1, seed=13, random_hw=True, random_sure=True)
    assert ped.n_markers == 85
    ped.chromstarts = np.array([0, 1, 4, 21, 85], np.int32)
    ctx = capi.Context(0)
    ctx.upload(ped)
    ca, csr, ch = own_columns_as_candidates(ped, 5, seed=1)
    got = ctx.sweep_place(ca, csr, ch, per_individual=True)
    want, compared = oracle_place(capi, ped, oracle_emission(ped, ca, csr, ch))
    assert compared == len(ped.dous) * 4
    assert_place_close(got["place"], want, capi)
    hs, hz = host_sum(got["place"], capi)
    np.testing.assert_allclose(got["place_sum"], hs, rtol=1e-12)
    assert np.array_equal(got["n_zero"], hz)
    ctx.close()


def test_planted_small_f2_argmax_matches_oracle(capi):
    """the 40-individual F2 with markers 3, 15 and 27 held out: the GPU profile peaks where the numpy / oracle profile does"""
    ped = synth.make_f2(40, 30, 1, seed=7)
    cols = np.array([3, 15, 27])
    base, ca, csr, ch = without_columns(ped, cols)
    ctx = capi.Context(0)
    ctx.upload(base)
    got = ctx.sweep_place(ca, csr, ch)
    want, _ = oracle_place(capi, base, oracle_emission(base, ca, csr, ch))
    prof = np.where((want == capi.IGNORED) | (want == capi.MINFACTOR), 0.0, want).sum(axis=0)
    assert np.array_equal(np.argmax(got["place_sum"], axis=1), np.argmax(prof, axis=1))
    best = placement.best_positions(got["place_sum"], got["n_zero"], got["null"], base.pos, base.chromstarts)
    for q, m in enumerate(cols):
        # the flanking markers of held-out marker m are m - 1 - q and m - q on the base map
        print("candidate %d (true %.2f cM): placed at marker %d, %.2f cM, LOD %.2f" % (m, ped.pos[m], best["marker"][q], best["pos"][q], best["lod"][q]))
        assert m - q - 2 <= best["marker"][q] <= m - q + 1
    ctx.close()


def test_planted_f2_at_size(capi):
    """2 000 F2 individuals, 100 markers per chromosome at 1 cM, every 10th marker held out: each is placed on its own
    chromosome within 2 cM of its true position"""
    ped = synth.make_f2(2000, 100, 2, seed=19)
    cs = np.asarray(ped.chromstarts)
    cols = np.concatenate([np.arange(cs[c] + 5, cs[c] + 100, 10) for c in range(2)])
    true_pos = np.asarray(ped.pos)[cols]
    true_chrom = np.searchsorted(cs, cols, side="right") - 1
    base, ca, csr, ch = without_columns(ped, cols)
    ctx = capi.Context(0)
    ctx.upload(base)
    got = ctx.sweep_place(ca, csr, ch)
    best = placement.best_positions(got["place_sum"], got["n_zero"], got["null"], base.pos, base.chromstarts)
    err = np.abs(best["pos"] - true_pos)
    print("largest placement error %.2f cM over %d candidates; smallest LOD %.1f, largest LOD on another chromosome %.1f"
          % (err.max(), len(cols), best["lod"].min(), best["other_lod"].max()))
    assert np.array_equal(best["chrom"], true_chrom)
    assert err.max() <= 2.0
    assert np.all(best["lod"] > best["other_lod"])
    ctx.close()


# ---------------------------------------------------------------------------------------------- command line
EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def run_demo(tmp_path, *extra, check=True):
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=600, check=check, cwd=str(tmp_path))


def test_cli_place(capi, tmp_path):
    """candidates = three of the demo's own markers.  The demo has three analysed individuals and 18 markers whose genotype
    columns largely repeat with period 6: most columns are uninformative (both founders alike) or occur again elsewhere
    in the file, and a copy cannot be told from its twin.  The CPU oracle's profile on the files' data (the contraction of
    test_against_oracle with every column as a candidate) peaks at the marker itself, alone, for columns 4, 13 and 16 only
    (by 0.02, 0.15 and 0.38 LOD over the best other marker); column 1 ties with its twin 7, column 10 with 4.  Those three
    are the candidates."""
    cols = [4, 13, 16]
    pos = [float(v) for v in open(os.path.join(DEMO, "demoplantimpute.map")).read().split()]
    M = len(pos)
    gen = tmp_path / "cand.gen"
    with open(gen, "w") as f:
        for ln in open(os.path.join(DEMO, "demoplantimpute.gen")):
            tok = ln.split()
            if tok:
                assert len(tok) == M + 1
                f.write(" ".join([tok[0]] + [tok[1 + c] for c in cols]) + "\n")
    out_a, out_b, pl = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "place.txt"
    run_demo(tmp_path, "--output", str(out_a))
    run_demo(tmp_path, "--output", str(out_b), "--place", str(pl), "--place-genfile", str(gen), "--place-markers", str(len(cols)))
    assert out_a.read_bytes() == out_b.read_bytes()
    head, prof = pl.read_text().split("\n\n")
    rows = [ln.split("\t") for ln in head.split("\n")]
    assert len(rows) == len(cols) and all(len(r) == 8 for r in rows)
    lod = np.array([[float(v) for v in ln.split("\t")] for ln in prof.strip("\n").split("\n")])
    assert lod.shape == (len(cols), M)
    for q, r in enumerate(rows):
        idx, chrom, marker, p, best_lod, lo, hi, nz = int(r[0]), int(r[1]), int(r[2]), float(r[3]), float(r[4]), float(r[5]), float(r[6]), int(r[7])
        print("candidate %d (marker %d): placed at marker %d, LOD %.3f, support [%g, %g], n_zero %d" % (q, cols[q], marker, best_lod, lo, hi, nz))
        assert idx == q and chrom == 1 and p == pos[marker] and lo <= p <= hi and nz >= 0
        assert abs(best_lod - lod[q, marker]) < 1e-4
        assert nz == 0 and best_lod >= lod[q].max() - 1e-4
        assert abs(marker - cols[q]) <= 1
    # the executable's own reading of the profile against placement.best_positions on the file's profile section
    b = placement.best_positions(lod * placement.LN10, np.zeros(lod.shape, np.int32), np.zeros(len(cols)), pos, [0, M])
    for q, r in enumerate(rows):
        assert (int(r[2]), float(r[5]), float(r[6])) == (b["marker"][q], b["support_lo"][q], b["support_hi"][q])
        assert abs(float(r[4]) - b["lod"][q]) < 1e-4
