"""GPU suite (-m gpu): the compact spill row of the uniform-state instantiation (cnf2_lane.h).

The instantiation stores each distinct alpha value once -- 48 doubles a row where the ordinary layout has 528 -- in the
same per-wave slots the ordinary instantiation uses with its own layout.  The yardstick is `sweep(all_states=True)`, the
ordinary instantiation, whose code and layout do not know of the compact row: same operations on the same numbers, so
everything is compared with `np.array_equal`.  The host suite (test_uniform_spill_host.py) checks the offsets themselves."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from conftest import oracle_ped

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ONE_BLOCK = 1 << 20          # more slots than the GPU has: the grid is clamped to one block of 4 waves
OUTPUTS = ("factors", "loglik", "dosage")
# many rows per slot with an even (258) and an odd (257) last marker; short jobs behind long ones in the same slot
LONG_LENGTHS = (258, 1, 257, 2, 23)
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


def _same(a, b, what, keys=OUTPUTS):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def _against_oracle(ped, got, what):
    """The tolerances of test_gpu_uniform_states.py."""
    o = oracle_ped(ped)
    for c in range(len(ped.chromstarts) - 1):
        first, last = int(ped.chromstarts[c]), int(ped.chromstarts[c + 1]) - 1
        want = o.sweep_batch(ped.dous, ped.gen[ped.dous], first=first, last=last, mode=2)
        np.testing.assert_allclose(got["factors"][:, c], want["factors"], rtol=RTOL, atol=1e-8, err_msg=what)
        np.testing.assert_allclose(got["dosage"][:, first:last + 1], want["dosage"], rtol=1e-7, atol=1e-11, err_msg=what)


def _all_uniform(r):
    return set(int(x) for x in r["paths"].ravel()) == {2}


# ---------------------------------------------------------------- case 1: row indexing and slot reuse
@pytest.fixture(scope="module")
def long_chroms(capi):
    ped = _cut(synth.make_f2(6, sum(LONG_LENGTHS) - 1, 1, seed=31, chrom_cm=120.0, missing=0.15), LONG_LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    ref = ctx.sweep(all_states=True, log_paths=True)
    assert _all_uniform(ref)
    yield ped, ctx, ref
    ctx.close()


@pytest.mark.parametrize("kw", [dict(), dict(static_jobs=True), dict(line_records=False)],
                         ids=["records", "static_jobs", "rows_fallback"])
@pytest.mark.parametrize("one_block", [False, True], ids=["full_grid", "one_block"])
def test_many_rows_per_slot_and_short_jobs_behind_long_ones(long_chroms, kw, one_block):
    ped, ctx, ref = long_chroms
    ctx.set_grid_reserve(ONE_BLOCK if one_block else 0)
    try:
        got = ctx.sweep(log_paths=True, **kw)
    finally:
        ctx.set_grid_reserve(0)
    assert _all_uniform(got)
    _same(got, ref, "long chromosomes %r one_block=%r" % (kw, one_block))


def test_long_chromosomes_against_the_oracle(long_chroms):
    ped, ctx, ref = long_chroms
    _against_oracle(ped, ctx.sweep(), "long chromosomes")


# ---------------------------------------------------------------- case 2: both layouts in one context's slots
def _three_founder_cross(n_ab, n_ac, markers_per_chrom, seed, missing, het_marker):
    """F2-type individuals with private empty F1 parents over three founders: A and B inbred, C inbred except heterozygous
    at one marker.  The first n_ab individuals are A x B (uniform windows); the other n_ac have one F1 parent from A x C
    and one from A x B (parents homozygous, grandparents not: the ordinary instantiation)."""
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


def test_layouts_alternate_in_one_contexts_slots(capi):
    """Uniform, ordinary and tied windows in one call, and calls with other layouts (every marker spilled; the Viterbi
    decisions) between the half-spill calls: each instantiation finds its own rows, whatever the slots held before."""
    n_ab, n_ac = 5, 4
    ped = _three_founder_cross(n_ab, n_ac, 19, seed=33, missing=0.1, het_marker=7)
    ped = _cut(_append(ped, synth.make_ail(4, 6, 3, 19, 1, seed=5, chrom_cm=25.0)), (9, 11))
    ctx = capi.Context(0)
    ctx.upload(ped)
    half = [ctx.sweep(log_paths=True)]
    full = ctx.sweep(full_spill=True)
    half.append(ctx.sweep(log_paths=True))
    vit = ctx.sweep_viterbi()
    half.append(ctx.sweep(log_paths=True))
    ref_half = ctx.sweep(all_states=True, log_paths=True)
    ref_full = ctx.sweep(all_states=True, full_spill=True)
    ref_vit = ctx.sweep_viterbi(all_states=True)
    paths = half[0]["paths"]
    assert np.all(paths[:n_ab] == 2) and np.all(paths[n_ab:n_ab + n_ac] == 1), paths
    for k, h in enumerate(half):
        assert np.array_equal(h["paths"], paths)
        _same(h, half[0], "half-spill sweep %d against the first" % k)
        _same(h, ref_half, "half-spill sweep %d against all_states" % k)
    _same(full, ref_full, "full spill against all_states")
    for k in vit:
        if vit[k] is not None:
            assert np.array_equal(vit[k], ref_vit[k], equal_nan=True), "sweep_viterbi against all_states: %s" % k
    _same(vit, half[0], "sweep_viterbi against the sweep", keys=("factors", "loglik"))
    _against_oracle(ped, half[2], "alternating layouts")
    ctx.close()


# ---------------------------------------------------------------- case 3: dense rescaling in a uniform window
def test_dense_rescaling_in_a_uniform_window(capi):
    """The reciprocals are stored with every even marker, and the guard (a stretch that loses more than 150 decades between
    two rescalings) switches the wave to dense rescaling in the middle of a chromosome.  An F2 whose first individual
    contradicts both founders with tiny certainties on markers 10..49: about 23 decades a marker -- over the guard within
    a tile, under a double's range.  The oracle rescales at every marker; loglik and dosage at the tolerances of
    test_gpu_parity.py's guard test."""
    ped = synth.make_f2(3, 60, 1, seed=5, chrom_cm=30.0, missing=0.0)
    ped.allele = ped.allele.copy()
    ped.sure = ped.sure.copy()
    kid = int(ped.row_of[ped.dous[0]])
    ped.allele[kid, 10:50] = (3, 3)
    ped.sure[kid, 10:50] = 1e-12
    ped.sure[1:3, 10:50] = 1e-12
    o = oracle_ped(ped)
    want = o.sweep_batch(ped.dous, ped.gen[ped.dous], mode=2)
    print("oracle factor", want["factor"])
    assert want["factor"][0] < -1000, "the fixture should lose thousands of log units"
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep(log_paths=True)
    ref = ctx.sweep(all_states=True, log_paths=True)
    one = None
    ctx.set_grid_reserve(ONE_BLOCK)
    try:
        one = ctx.sweep()
    finally:
        ctx.set_grid_reserve(0)
    ctx.close()
    assert _all_uniform(got) and _all_uniform(ref)
    _same(got, ref, "dense rescaling")
    _same(one, ref, "dense rescaling on one block")
    print("loglik", got["loglik"][:, 0], "max |dosage - oracle|", np.abs(got["dosage"] - want["dosage"]).max())
    np.testing.assert_allclose(got["loglik"][:, 0], want["factor"], rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(got["dosage"], want["dosage"], rtol=1e-6, atol=1e-10)


# ---------------------------------------------------------------- case 4: launches that stop after the forward pass
def test_forward_only_launches_store_no_rows_and_disturb_nothing(capi):
    """sweep(dosage=False) and the Viterbi likelihood pass stop after the forward pass: the uniform instantiation then
    writes no spill row.  Their likelihoods are the sweep's, and a sweep after them finds its rows as before."""
    ped = _cut(synth.make_f2(10, sum(TILE_EDGE_LENGTHS) - 1, 1, seed=21, chrom_cm=30.0, missing=0.15), TILE_EDGE_LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    first = ctx.sweep(log_paths=True)
    assert _all_uniform(first)
    nod = ctx.sweep(dosage=False, log_paths=True)
    assert _all_uniform(nod)
    _same(nod, first, "sweep(dosage=False)", keys=("factors", "loglik"))
    again = ctx.sweep()
    vit = ctx.sweep_viterbi()
    _same(vit, first, "sweep_viterbi", keys=("factors", "loglik"))
    last = ctx.sweep()
    _same(again, first, "sweep after sweep(dosage=False)")
    _same(last, first, "sweep after sweep_viterbi")
    _same(first, ctx.sweep(all_states=True), "against all_states")
    ctx.close()
