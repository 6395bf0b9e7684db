"""GPU suite (-m gpu): the line records of the uniform windows.

In a window of a cross of inbred lines the instantiation for uniform windows reads what a parent and its two grandparents
contribute to the emission tables from records built once per launch (one per line, marker, grandparent traced and allele
handed down) instead of forming it per individual, part and pass.  Same operations on the same operands in the same order,
so three forms are compared with `np.array_equal`: records (the default), `line_records=False` (CNF2_NO_LINE_RECORDS: the
instantiation with the ordinary tile producer) and `all_states=True` (the ordinary instantiation).  The oracle is compared at
the tolerances of test_gpu_uniform_states.py."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from conftest import oracle_ped
from test_gpu_uniform_states import (ONE_BLOCK, OUTPUTS, RTOL, TILE_EDGE_LENGTHS, _against_oracle, _append, _cut, _same,
                                     _three_founder_cross)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def _three_forms(ctx, what, **kw):
    """(records, no records, ordinary instantiation) of one sweep, equal to the bit; returns the first and its record counts."""
    rec = ctx.sweep(**kw)
    counts = ctx.last_line_records()
    _same(rec, ctx.sweep(line_records=False, **kw), what + ": records against the same instantiation without")
    assert ctx.last_line_records() == dict(lines=0, on_records=0, fallback=counts["on_records"] + counts["fallback"], bytes=0)
    _same(rec, ctx.sweep(all_states=True, **kw), what + ": records against the ordinary instantiation")
    return rec, counts


# ---------------------------------------------------------------- 1: an F2 at the tile edges
@pytest.fixture(scope="module")
def tile_edges(capi):
    ped = _cut(synth.make_f2(10, sum(TILE_EDGE_LENGTHS) - 1, 1, seed=21, chrom_cm=30.0, missing=0.15), TILE_EDGE_LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    yield ped, ctx
    ctx.close()


@pytest.mark.parametrize("kw", [dict(), dict(raw=True), dict(dosage=False), dict(static_jobs=True), dict(one_block=True)],
                         ids=["normalised", "raw", "no_dosage", "static_jobs", "one_block"])
def test_f2_at_tile_edges(tile_edges, kw):
    ped, ctx = tile_edges
    kw = dict(kw)
    if kw.pop("one_block", False):
        ctx.set_grid_reserve(ONE_BLOCK)      # one block of 4 waves sweeps all 70 jobs
    try:
        rec, counts = _three_forms(ctx, "tile edges %r" % (kw,), **kw)
    finally:
        ctx.set_grid_reserve(0)
    n_jobs = len(ped.dous) * len(TILE_EDGE_LENGTHS)
    assert counts["on_records"] == n_jobs and counts["fallback"] == 0, counts
    assert 1 <= counts["lines"] <= 2, counts
    assert counts["bytes"] == counts["lines"] * ped.n_markers * 16 * 2 * 64
    if kw == {}:
        _against_oracle(ped, rec, "F2 on records")


# ---------------------------------------------------------------- 2, 4: several lines in one call, and the cap
def _crosses(seed=41, missing=0.1, markers=19):
    """Three inbred founders (homozygous at every marker, C with its own alleles and sure) and F2-type individuals with private
    empty F1 parents, three each of (A x B) x (A x B), (A x C) x (A x C), (B x C) x (B x C) and (A x B) x (A x C): three
    distinct lines (blank parent over A B, A C, B C)."""
    ped = synth.make_f2(12, markers, 1, seed=seed, chrom_cm=25.0, missing=missing)
    R, rows, M = ped.n_rec, ped.allele.shape[0], ped.n_markers
    c_allele = np.empty((1, M, 2), np.uint8)
    c_allele[0, :, 0] = c_allele[0, :, 1] = np.where(np.arange(M) % 3 == 0, 1, 2)
    ped.names = ped.names + ["C"]
    ped.par = np.concatenate([ped.par, [[-1, -1]]]).astype(np.int32)
    ped.gen = np.concatenate([ped.gen, [0]]).astype(np.int32)
    ped.empty = np.concatenate([ped.empty, [0]]).astype(np.uint8)
    ped.row_of = np.concatenate([ped.row_of, [rows]]).astype(np.int32)
    ped.allele = np.concatenate([ped.allele, c_allele])
    ped.sure = np.concatenate([ped.sure, np.full((1, M, 2), 0.05)])
    ped.hw = np.concatenate([ped.hw, ped.hw[2:3]])
    pairs = [((0, 1), (0, 1)), ((0, R), (0, R)), ((1, R), (1, R)), ((0, 1), (0, R))]
    for i in range(12):
        r = 2 + 3 * i
        ped.par[r + 1], ped.par[r + 2] = pairs[i // 3]
    ped.founder_flags()
    return _cut(ped, (9, 11))


@pytest.fixture(scope="module")
def crosses(capi):
    ped = _crosses()
    ctx = capi.Context(0)
    ctx.upload(ped)
    yield ped, ctx
    ctx.close()


def test_several_lines_in_one_call(crosses):
    ped, ctx = crosses
    rec, counts = _three_forms(ctx, "three crosses", log_paths=True)
    assert np.all(rec["paths"] == 2), rec["paths"]
    assert counts["lines"] >= 3 and counts["fallback"] == 0 and counts["on_records"] == rec["paths"].size, counts
    _against_oracle(ped, rec, "three crosses on records")
    # sub-ranges that start inside a group of equal lines
    for b, e in ((1, 5), (4, 12), (7, 8), (10, 12)):
        part = ctx.sweep(ind_begin=b, ind_end=e)
        assert ctx.last_line_records()["on_records"] == (e - b) * 2
        for k in OUTPUTS:
            assert np.array_equal(part[k], rec[k][b:e]), "range [%d, %d): %s differs" % (b, e, k)


def test_cap_sends_the_other_lines_through_the_ordinary_producer(crosses):
    ped, ctx = crosses
    ref = ctx.sweep(all_states=True)
    try:
        ctx.set_line_records(1)
        one = ctx.sweep()
        c1 = ctx.last_line_records()
        ctx.set_line_records(0)
        none = ctx.sweep()
        c0 = ctx.last_line_records()
    finally:
        ctx.set_line_records(-1)
    assert c1["lines"] == 1 and c1["on_records"] == 3 * 2 and c1["fallback"] == 9 * 2, c1     # the three (A x B) x (A x B)
    assert c0["lines"] == 0 and c0["on_records"] == 0 and c0["fallback"] == 12 * 2 and c0["bytes"] == 0, c0
    _same(one, ref, "cap of one line")
    _same(none, ref, "cap of no line")


def test_line_numbering_follows_range_and_cap(crosses):
    """The context keeps the numbering of the lines while the windows, the call's range and the cap stay the same: alternate
    both and come back, every sweep against the ordinary instantiation and with the counts its range and cap imply."""
    ped, ctx = crosses
    ref = ctx.sweep(all_states=True)
    # (range, cap) -> lines kept; individuals 0-2 A x B twice, 3-5 A x C twice, 6-8 B x C twice, 9-11 A x B and A x C
    steps = [((0, 12), -1), ((3, 9), -1), ((0, 12), 1), ((3, 9), 1), ((0, 12), -1), ((3, 9), 2), ((3, 9), -1), ((0, 12), 1), ((0, 12), -1)]
    try:
        for (b, e), cap in steps:
            ctx.set_line_records(cap)
            got = ctx.sweep(ind_begin=b, ind_end=e)
            c = ctx.last_line_records()
            first = 0 if b == 0 else 1                       # the line of the range's first individuals
            lines_in_range = 3 if b == 0 else 2
            want_lines = lines_in_range if cap < 0 else min(cap, lines_in_range)
            on = sum(1 for i in range(b, e) if all(k < want_lines for k in _lines_of(i, first)))
            assert c["lines"] == want_lines and c["on_records"] == 2 * on and c["fallback"] == 2 * (e - b - on), ((b, e), cap, c)
            for k in OUTPUTS:
                assert np.array_equal(got[k], ref[k][b:e]), "range [%d, %d), cap %d: %s differs" % (b, e, cap, k)
    finally:
        ctx.set_line_records(-1)


def _lines_of(i, first):
    """Numbers, in order of appearance from the cross `first`, of the two lines of individual i of _crosses()."""
    cross = [(0, 0), (1, 1), (2, 2), (0, 1)][i // 3]
    order = {0: [0, 1, 2], 1: [None, 0, 1]}[first]
    return [order[x] if order[x] is not None else 99 for x in cross]


# ---------------------------------------------------------------- 3: every incoming value
def _odd_values(seed=55):
    """An F2 whose roots hold unknown alleles, a third allele 3 and the sentinel 9, heterozygous in every combination, with
    sure 0, 1 and values between; founder B is homozygous 3 and 9 at some markers; the founders' sure differ."""
    ped = _cut(synth.make_f2(8, 26, 1, seed=seed, chrom_cm=30.0, missing=0.1), (17, 10))
    M = ped.n_markers
    rng = np.random.default_rng(seed)
    roots = ped.allele[3:]
    pick = rng.random(roots.shape[:2]) < 0.35
    vals = rng.choice(np.array([0, 1, 2, 3], np.uint8), size=roots.shape)
    roots[pick] = vals[pick]
    # the sentinel fits no unknown allele: where roots hold it, the empty F1 parents' blank row gets a sure above 0, or no path
    # through them stays alive
    nines = [2, 8, 14, 19, 23]
    for m in nines:
        for i in rng.choice(8, size=3, replace=False):
            roots[i, m] = [(9, 9), (9, 1), (2, 9), (0, 9)][int(rng.integers(4))]
    ped.sure[0, nines] = 0.25
    # (a known allele that fits no founder must keep a nonzero sure, or the marker leaves no path alive)
    ped.sure[3:] = np.where(roots != 0, rng.choice([0.02, 0.37, 0.5], size=roots.shape), 0.0)
    ped.allele[3, 4] = ped.allele[4, 9] = (1, 2)
    ped.sure[3, 4] = (1.0, 0.5)                # sure 1: the allele is certainly mistyped; sure 0: certainly right
    ped.sure[4, 9] = (0.0, 0.0)
    ped.allele[2, 3] = ped.allele[2, 12] = (3, 3)
    ped.allele[2, 7] = ped.allele[2, 20] = (9, 9)
    ped.sure[1] = 0.03
    ped.sure[2] = 0.11
    ped.sure[2, 5] = 0.0
    ped.sure[2, 6] = 0.5
    assert M == 27
    return ped


def test_every_incoming_value(capi):
    ped = _odd_values()
    ctx = capi.Context(0)
    ctx.upload(ped)
    rec, counts = _three_forms(ctx, "odd values", log_paths=True)
    assert np.all(rec["paths"] == 2) and counts["fallback"] == 0 and counts["lines"] >= 1, (rec["paths"], counts)
    assert np.isfinite(rec["dosage"]).all() and (rec["loglik"][1:] > -1e14).all(), "the fixture should leave the jobs alive"
    # the oracle divides by a root's 1 - sure (as the reference does): the individual with the sure of 1 is NaN there on its
    # first chromosome and is compared among the three forms only
    o = oracle_ped(ped)
    for c in range(len(ped.chromstarts) - 1):
        first, last = int(ped.chromstarts[c]), int(ped.chromstarts[c + 1]) - 1
        want = o.sweep_batch(ped.dous, ped.gen[ped.dous], first=first, last=last, mode=2)
        ok = np.isfinite(want["factor"])
        assert ok.sum() >= len(ped.dous) - 1 and np.isfinite(want["dosage"][ok]).all()
        np.testing.assert_allclose(rec["factors"][ok, c], want["factors"][ok], rtol=RTOL, atol=1e-8)
        np.testing.assert_allclose(rec["dosage"][ok, first:last + 1], want["dosage"][ok], rtol=1e-7, atol=1e-11)
    ctx.close()


# ---------------------------------------------------------------- founders: uniform windows the records do not cover
def test_founder_parents_keep_the_ordinary_producer(capi):
    """An F2 in which some individuals' F1 parents descend from EMPTY grandparent records (blank row: homozygous, doubly
    unknown): all four grandparents are present and homozygous, so the windows are uniform, but such a parent is a founder
    (no parent of its own is informative) and the producer's founder-parent branch runs.  Those windows must report as
    fallback and equal the ordinary instantiation; the others in the same call run on records."""
    ped = synth.make_f2(6, 19, 1, seed=77, chrom_cm=25.0, missing=0.1)
    R = ped.n_rec
    ped.names = ped.names + ["E0", "E1"]                    # two empty records on the blank row
    ped.par = np.concatenate([ped.par, [[-1, -1], [-1, -1]]]).astype(np.int32)
    ped.gen = np.concatenate([ped.gen, [0, 0]]).astype(np.int32)
    ped.empty = np.concatenate([ped.empty, [1, 1]]).astype(np.uint8)
    ped.row_of = np.concatenate([ped.row_of, [0, 0]]).astype(np.int32)
    for i in (1, 4):                                        # one founder parent; and both
        r = 2 + 3 * i
        ped.par[r + 1] = (R, R + 1)
        if i == 4:
            ped.par[r + 2] = (R, R + 1)
    ped.founder_flags()
    ped = _cut(ped, (9, 11))
    ctx = capi.Context(0)
    ctx.upload(ped)
    rec, counts = _three_forms(ctx, "founder parents", log_paths=True)
    assert np.all(rec["paths"][[0, 2, 3, 5]] == 2), rec["paths"]
    n_uni = int((rec["paths"] == 2).sum())
    assert np.all(rec["paths"][1] == 2), "the fixture's window with one founder parent should be uniform: %r" % (rec["paths"],)
    assert counts["on_records"] == 4 * 2 and counts["fallback"] == n_uni - 4 * 2 and counts["fallback"] >= 2, counts
    _against_oracle(ped, rec, "founder parents")
    ctx.close()


# ---------------------------------------------------------------- 5: the records are rebuilt by every call
def test_records_follow_the_rows(crosses):
    ped, ctx = crosses
    first = ctx.sweep()
    sure = ped.sure[2:3].copy()
    sure[0, [2, 10, 15]] = 0.2                 # founder B, still homozygous with equal sure
    try:
        ctx.update_rows(2, ped.allele[2:3], sure, ped.hw[2:3])
        second = ctx.sweep()
        assert ctx.last_line_records()["fallback"] == 0
        _same(second, ctx.sweep(all_states=True), "after the row update")
        assert not np.array_equal(second["factors"], first["factors"]) and not np.array_equal(second["dosage"], first["dosage"])
    finally:
        ctx.update_rows(2, ped.allele[2:3], ped.sure[2:3], ped.hw[2:3])
    _same(ctx.sweep(), first, "rows restored")


# ---------------------------------------------------------------- 6: a call with every kind of window
def test_mixed_call_and_the_viterbi_likelihoods(capi):
    ped = _append(_crosses(), _append(_cut(_three_founder_cross(2, 3, 19, seed=33, missing=0.1, het_marker=7), (9, 11)),
                                      _cut(synth.make_ail(4, 6, 3, 19, 1, seed=5, chrom_cm=25.0), (9, 11))))
    ctx = capi.Context(0)
    ctx.upload(ped)
    rec, counts = _three_forms(ctx, "mixed call", log_paths=True)
    paths = set(int(x) for x in rec["paths"].ravel())
    assert {1, 2, 16} <= paths, paths
    n_uni = int((rec["paths"] == 2).sum())
    assert counts["on_records"] == n_uni and counts["fallback"] == 0 and counts["lines"] >= 3, counts
    vit = [ctx.sweep_viterbi(), ctx.sweep_viterbi(line_records=False), ctx.sweep_viterbi(all_states=True)]
    for other in vit[1:]:
        for k in vit[0]:
            assert np.array_equal(vit[0][k], other[k], equal_nan=True), ("sweep_viterbi", k)
    assert np.array_equal(vit[0]["factors"], rec["factors"]) and np.array_equal(vit[0]["loglik"], rec["loglik"])
    ctx.close()
