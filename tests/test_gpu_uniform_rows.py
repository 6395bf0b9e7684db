"""GPU suite (-m gpu): the per-locus rows of the fast kernel's instantiation for uniform windows.

In that instantiation the four lanes of a chain that share state bit 0 would form the same four B-side class sums; each forms
one and fetches the other three from its partners.  A wrong partner or a wrong pick changes a row's
three class sums, so the fixture makes the three classes of a row differ: the analysed individuals' own genotype rows (the
roots of their windows; slots_uniform does not look at them) get unequal certainties at about half the markers and
haploweights away from 0.5.  Rows are compared raw as well: normalisation can hide a common factor, not a swapped class,
but the raw sums are what the exchange hands over.  Everything against the ordinary instantiation (`all_states=True`) is
compared with `np.array_equal`."""
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
N_IND = 12


def _fixture_pedigree():
    ped = synth.make_f2(N_IND, sum(TILE_EDGE_LENGTHS) - 1, 1, missing=0.15)
    assert ped.n_markers == sum(TILE_EDGE_LENGTHS)
    ped.chromstarts = np.concatenate([[0], np.cumsum(TILE_EDGE_LENGTHS)]).astype(np.int32)
    ped.pos = np.concatenate([np.arange(n) * (0.6 + 0.1 * k) for k, n in enumerate(TILE_EDGE_LENGTHS)])
    # rows 3.. are the analysed individuals' own (0 blank, 1 and 2 the inbred founders, which stay as they are)
    rng = np.random.default_rng(20250)
    own = ped.sure[3:]
    typed = ped.allele[3:, :, 0] != 0
    odd = typed & (rng.random(typed.shape) < 0.5)
    own[:, :, 1] = np.where(odd, rng.uniform(0.05, 0.3, typed.shape), own[:, :, 1])
    ped.hw[3:] = rng.uniform(0.1, 0.9, typed.shape)
    share = (own[:, :, 0] != own[:, :, 1]).mean()
    assert 0.3 < share < 0.6, share            # "about half" of all markers (15 % of them are untyped and stay equal)
    return ped


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


@pytest.fixture(scope="module")
def rows(capi):
    ped = _fixture_pedigree()
    ctx = capi.Context(0)
    ctx.upload(ped)
    yield ped, ctx
    ctx.close()


@pytest.fixture(scope="module")
def oracle_rows(rows):
    """Per chromosome: the oracle's factors and its raw (unnormalised) rows, formed once."""
    ped, _ = rows
    o = oracle_ped(ped)
    out = []
    for c in range(len(ped.chromstarts) - 1):
        first, last = int(ped.chromstarts[c]), int(ped.chromstarts[c + 1]) - 1
        r = [o.sweep_ind(int(i), int(ped.gen[i]), first=first, last=last, mode=2) for i in ped.dous]
        out.append((first, last, np.array([x["factors"] for x in r]), np.array([x["dosage"] for x in r])))
    return out


def _same(a, b, what):
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def test_every_job_is_a_uniform_one_and_the_rows_are_not_flat(rows, oracle_rows):
    ped, ctx = rows
    uni = ctx.sweep(log_paths=True)
    assert set(int(x) for x in uni["paths"].ravel()) == {2}
    # the fixture must tell the classes apart: three distinct non-zero raw class sums in at least a quarter of the cells
    raw = np.concatenate([d for _, _, _, d in oracle_rows], axis=1)
    assert raw.shape == (N_IND, ped.n_markers, 3)
    distinct = (raw > 0).all(axis=2) & (raw[:, :, 0] != raw[:, :, 1]) & (raw[:, :, 1] != raw[:, :, 2]) & (raw[:, :, 0] != raw[:, :, 2])
    print("cells with three distinct non-zero raw classes: %.3f" % distinct.mean())
    assert distinct.mean() >= 0.25, distinct.mean()


@pytest.mark.parametrize("kw", [dict(raw=True), dict(), dict(static_jobs=True)], ids=["raw", "normalised", "static_jobs"])
def test_rows_equal_the_ordinary_instantiation(rows, kw):
    ped, ctx = rows
    uni = ctx.sweep(log_paths=True, **kw)
    ref = ctx.sweep(all_states=True, log_paths=True, **kw)
    assert set(int(x) for x in uni["paths"].ravel()) == {2}
    assert set(int(x) for x in ref["paths"].ravel()) == {2}
    assert np.any(ref["dosage"] != 0)
    _same(uni, ref, "rows %r" % (kw,))


def test_rows_on_one_block_and_against_the_oracle(rows, oracle_rows):
    """One block of 4 waves sweeps all 84 jobs (every wave takes many, of every length); and the oracle, raw rows included."""
    ped, ctx = rows
    ref = ctx.sweep(all_states=True)
    ctx.set_grid_reserve(ONE_BLOCK)
    one = ctx.sweep()
    ctx.set_grid_reserve(0)
    _same(one, ref, "one block")
    raw = ctx.sweep(raw=True)
    for c, (first, last, factors, want) in enumerate(oracle_rows):
        np.testing.assert_allclose(one["factors"][:, c], factors, rtol=RTOL, atol=1e-8)
        np.testing.assert_allclose(raw["dosage"][:, first:last + 1], want, rtol=1e-7, atol=1e-12)
        tot = want.sum(axis=2, keepdims=True)
        norm = np.divide(want, tot, out=want.copy(), where=tot > 0)
        np.testing.assert_allclose(one["dosage"][:, first:last + 1], norm, rtol=1e-7, atol=1e-11)
