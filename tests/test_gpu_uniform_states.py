"""GPU suite (-m gpu): the fast kernel's instantiation for uniform windows.

A window whose two parents and four grandparents are homozygous with equal sure at every marker (any cross of inbred lines:
`row_flags_kernel` finds them in the data) has an unrestricted emission table that does not depend on the four grandparental
state bits 1, 2, 4, 5.  Alpha and beta then do not depend on them either, and the plain half-spill sweep of such jobs runs
an instantiation that keeps the equal states once.  It performs the same operations on the same
numbers as the ordinary instantiation, so everything here is compared with `np.array_equal`: `all_states=True`
(CNF2_ALL_STATES) sends every job through the ordinary instantiation."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from conftest import oracle_ped

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ONE_BLOCK = 1 << 20          # more slots than the GPU has: the grid is clamped to one block of 4 waves
OUTPUTS = ("factors", "loglik", "dosage")
# chromosome lengths: a single marker, an even and an odd last marker, exactly one tile of 8, a tile + 1, two tiles +- 1
TILE_EDGE_LENGTHS = (1, 2, 3, 8, 9, 16, 17)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def _cut(ped, lengths):
    """The map of `ped` cut into chromosomes of the given lengths, positions restarting on each."""
    assert sum(lengths) == ped.n_markers
    ped.chromstarts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ped.pos = np.concatenate([np.arange(n) * (0.6 + 0.1 * k) for k, n in enumerate(lengths)])
    return ped


def _same(a, b, what):
    for k in OUTPUTS:
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def _against_oracle(ped, got, what):
    o = oracle_ped(ped)
    for c in range(len(ped.chromstarts) - 1):
        first, last = int(ped.chromstarts[c]), int(ped.chromstarts[c + 1]) - 1
        want = o.sweep_batch(ped.dous, ped.gen[ped.dous], first=first, last=last, mode=2)
        np.testing.assert_allclose(got["factors"][:, c], want["factors"], rtol=RTOL, atol=1e-8, err_msg=what)
        np.testing.assert_allclose(got["dosage"][:, first:last + 1], want["dosage"], rtol=1e-7, atol=1e-11, err_msg=what)


def _three_founder_cross(n_ab, n_ac, markers_per_chrom, seed, missing, het_marker):
    """F2-type individuals with private empty F1 parents over three founders: A and B inbred, C inbred except heterozygous
    at one marker (its row is not homozygous everywhere).  The first n_ab individuals are A x B (uniform windows); the
    other n_ac have one F1 parent from A x C and one from A x B (parents homozygous, grandparents not: the ordinary
    instantiation's `hom == 1`; C in both lines would occupy two slots and make the window a tied one)."""
    ped = synth.make_f2(n_ab + n_ac, markers_per_chrom, 1, seed=seed, chrom_cm=25.0, missing=missing)
    R, rows, M = ped.n_rec, ped.allele.shape[0], ped.n_markers
    c_allele = np.full((1, M, 2), 2, np.uint8)
    c_allele[0, het_marker] = (1, 2)
    ped.names = ped.names + ["C"]
    ped.par = np.concatenate([ped.par, [[-1, -1]]]).astype(np.int32)
    ped.gen = np.concatenate([ped.gen, [0]]).astype(np.int32)
    ped.empty = np.concatenate([ped.empty, [0]]).astype(np.uint8)
    ped.row_of = np.concatenate([ped.row_of, [rows]]).astype(np.int32)
    ped.allele = np.concatenate([ped.allele, c_allele])
    ped.sure = np.concatenate([ped.sure, ped.sure[2:3]])
    ped.hw = np.concatenate([ped.hw, ped.hw[2:3]])
    for i in range(n_ab, n_ab + n_ac):
        r = 2 + 3 * i
        ped.par[r + 1] = (0, R)
    ped.founder_flags()
    return ped


def _append(p1, p2):
    """One pedigree holding the records of both (same map): p2's records and rows behind p1's."""
    assert np.array_equal(p1.pos, p2.pos) and np.array_equal(p1.chromstarts, p2.chromstarts)
    R1, rows1 = p1.n_rec, p1.allele.shape[0]
    ped = synth.Pedigree(list(p1.names) + ["x_" + n for n in p2.names],
                         np.concatenate([p1.par, np.where(p2.par >= 0, p2.par + R1, -1)]).astype(np.int32),
                         np.concatenate([p1.gen, p2.gen]).astype(np.int32),
                         np.concatenate([p1.empty, p2.empty]).astype(np.uint8),
                         np.concatenate([p1.row_of, p2.row_of + rows1]).astype(np.int32),
                         np.concatenate([p1.allele, p2.allele]), np.concatenate([p1.sure, p2.sure]),
                         np.concatenate([p1.hw, p2.hw]), p1.pos, p1.chromstarts,
                         np.concatenate([p1.dous, p2.dous + R1]).astype(np.int32))
    ped.founder_flags()
    return ped


def test_premise_states_that_differ_in_grandparental_bits_are_equal(capi):
    """The alpha-minus and beta rows of an F2 window in the reference layout: states that differ only in state bits 1, 2,
    4, 5 hold the same bits, at every marker and in all 8 shift modes."""
    ped = synth.make_f2(4, 9, 1, missing=0.1)
    ctx = capi.Context(0)
    ctx.upload(ped)
    g = np.arange(64)
    rep = g & 0b001001                       # the state of the same class with the four grandparental bits clear
    for ind in range(len(ped.dous)):
        fw, _ = ctx.fwbw_store(ind)
        assert np.any(fw[:, :, 0] != 0) and np.any(fw[:, :, 1] != 0)
        for slot, name in ((0, "alpha-minus"), (1, "beta")):
            rows = fw[:, :, slot, :]
            assert np.array_equal(rows, rows[:, :, rep]), "%s of individual %d depends on a grandparental bit" % (name, ind)
        # (and the two bits that are kept do matter somewhere: the classes are not coarser than claimed)
        assert any(not np.array_equal(fw[:, :, 0, 0], fw[:, :, 0, k]) for k in (1, 8, 9))
    ctx.close()


@pytest.fixture(scope="module")
def tile_edges(capi):
    ped = _cut(synth.make_f2(10, sum(TILE_EDGE_LENGTHS) - 1, 1, seed=21, chrom_cm=30.0, missing=0.15), TILE_EDGE_LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    yield ped, ctx
    ctx.close()


@pytest.mark.parametrize("kw", [dict(), dict(raw=True), dict(dosage=False), dict(static_jobs=True)],
                         ids=["normalised", "raw", "no_dosage", "static_jobs"])
def test_uniform_jobs_equal_the_ordinary_instantiation_at_tile_edges(tile_edges, kw):
    ped, ctx = tile_edges
    uni = ctx.sweep(log_paths=True, **kw)
    ref = ctx.sweep(all_states=True, log_paths=True, **kw)
    assert set(int(x) for x in uni["paths"].ravel()) == {2}
    assert set(int(x) for x in ref["paths"].ravel()) == {2}
    _same(uni, ref, "tile edges %r" % (kw,))


def test_uniform_jobs_on_one_block_and_against_the_oracle(tile_edges):
    """One block of 4 waves sweeps all 70 jobs (every wave takes many, of every length); and the oracle."""
    ped, ctx = tile_edges
    ref = ctx.sweep(all_states=True)
    ctx.set_grid_reserve(ONE_BLOCK)
    one = ctx.sweep()
    one_static = ctx.sweep(static_jobs=True)
    ctx.set_grid_reserve(0)
    _same(one, ref, "one block")
    _same(one_static, ref, "one block, static jobs")
    _against_oracle(ped, one, "uniform windows")


@pytest.mark.parametrize("with_ties", [False, True], ids=["untied", "with_tied_windows"])
def test_mixed_call_runs_both_instantiations(capi, with_ties):
    n_ab, n_ac = 5, 4
    ped = _three_founder_cross(n_ab, n_ac, 19, seed=33, missing=0.1, het_marker=7)
    if with_ties:
        ped = _append(ped, synth.make_ail(4, 6, 3, 19, 1, seed=5, chrom_cm=25.0))
    ped = _cut(ped, (9, 11))
    ctx = capi.Context(0)
    ctx.upload(ped)
    mixed = ctx.sweep(log_paths=True)
    ref = ctx.sweep(all_states=True, log_paths=True)
    paths = mixed["paths"]
    assert np.all(paths[:n_ab] == 2) and np.all(paths[n_ab:n_ab + n_ac] == 1), paths
    assert np.array_equal(paths, ref["paths"])
    if with_ties:
        assert 16 in set(int(x) for x in paths.ravel()), "the fixture should hold tied windows"
    _same(mixed, ref, "mixed call")
    _same(ctx.sweep(static_jobs=True), ref, "mixed call, static jobs")
    ctx.set_grid_reserve(ONE_BLOCK)
    _same(ctx.sweep(), ref, "mixed call on one block")
    ctx.set_grid_reserve(0)
    # sub-ranges that hold one class only, and one that starts inside the first class
    for b, e in ((0, n_ab), (n_ab, n_ab + n_ac), (2, n_ab + 1)):
        part = ctx.sweep(ind_begin=b, ind_end=e)
        for k in OUTPUTS:
            assert np.array_equal(part[k], ref[k][b:e]), "range [%d, %d): %s differs" % (b, e, k)
    _against_oracle(ped, mixed, "mixed call")
    ctx.close()


def test_nothing_else_moved(capi):
    """A pedigree without uniform windows: the flag changes nothing.  And the modes that do not use the instantiation
    ignore it -- on the outbred pedigree and on an F2, whose Viterbi likelihoods do take the plain sweep's route."""
    out3 = synth.make_outbred3(3, 3, 11, 1)
    f2 = synth.make_f2(5, 11, 1, seed=8, chrom_cm=20.0, missing=0.1)
    for ped, name in ((out3, "outbred"), (f2, "F2")):
        ctx = capi.Context(0)
        ctx.upload(ped)
        a, b = ctx.sweep(log_paths=True), ctx.sweep(all_states=True, log_paths=True)
        _same(a, b, name)
        assert (2 in a["paths"]) == (name == "F2")
        desc = ctx.descendants()
        acc = [ctx.sweep_accumulate(desc, deterministic=True, all_states=f) for f in (False, True)]
        for k in acc[0]:
            assert np.array_equal(acc[0][k], acc[1][k], equal_nan=True), (name, "sweep_accumulate", k)
        # (the accumulate instantiation's rows are not compared with sweep()'s bit for bit: on windows with missing
        # genotypes the two instantiations fuse the class sums' multiply-adds differently, whichever route sweep() takes)
        for k in ("factors", "loglik"):
            assert np.array_equal(acc[0][k], a[k]), (name, "sweep_accumulate against sweep", k)
        np.testing.assert_allclose(acc[0]["dosage"], a["dosage"], rtol=1e-12, atol=1e-15, err_msg=name)
        turn = [ctx.sweep_turn_scan(full=False, lse=True, all_states=f)[1] for f in (False, True)]
        assert np.array_equal(turn[0], turn[1]), (name, "sweep_turn_scan")
        for mode, kw in ((ctx.sweep_crossovers, {}), (ctx.sweep_viterbi, {}), (ctx.sweep_sample, dict(draws=4, seed=5))):
            r = [mode(all_states=f, **kw) for f in (False, True)]
            for k in r[0]:
                if k == "xo_sum":     # added up with f64 atomics in order of arrival: not the same bits from run to run
                    np.testing.assert_allclose(r[0][k], r[1][k], rtol=1e-12, atol=1e-300)
                elif r[0][k] is not None:
                    assert np.array_equal(r[0][k], r[1][k], equal_nan=True), (name, mode.__name__, k)
            assert np.array_equal(r[0]["factors"], a["factors"]) and np.array_equal(r[0]["loglik"], a["loglik"]), (name, mode.__name__)
        ctx.close()
