"""GPU suite (-m gpu): four uniform windows to a wave (fb_unipack_kernel).

The jobs of a call that are swept on line records go four to a wavefront, chromosome by chromosome: the lanes that would
repeat a uniform window's recursion carry three more jobs instead.  Per job it is the same operations on the same operands in
the same order, so three forms are compared with `np.array_equal`: packed (the default), `uniform_pack=False`
(CNF2_NO_UNIFORM_PACK: one job to a wave on records) and `all_states=True` (the ordinary instantiation).  Every output array is
filled with NaN before the call, `cnf2_last_uniform_pack` tells that the packed kernel ran, and the oracle is compared at the
tolerances of test_gpu_uniform_states.py."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from test_gpu_line_records import _crosses, _odd_values
from test_gpu_uniform_states import (ONE_BLOCK, OUTPUTS, TILE_EDGE_LENGTHS, _against_oracle, _append, _cut, _same,
                                     _three_founder_cross)

pytestmark = pytest.mark.gpu

# a single marker; tiles of 2 with an even and an odd last marker; the 8 markers between two rescalings -1, +0, +1; two such
# stretches +0, +1; a long run of the compact spill rows ending on an odd and on an even marker
LENGTHS = (1, 2, 3, 7, 8, 9, 16, 17, 257, 258)
DEAD = -1e14          # a likelihood below this: none left (test_gpu_line_records.py)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def _sweep(capi, ctx, ind_begin=0, ind_end=None, dosage=True, raw=False, static_jobs=False, all_states=False, line_records=True,
           uniform_pack=True):
    """ctx.sweep() into arrays filled with NaN; returns the outputs and the call's packed jobs and groups."""
    ind_end = ctx.n_ind if ind_end is None else ind_end
    n = ind_end - ind_begin
    out = dict(factors=np.full((n, ctx.n_chrom, 8), np.nan), loglik=np.full((n, ctx.n_chrom), np.nan),
               dosage=np.full((n, ctx.n_markers, 3), np.nan) if dosage else None)
    flags = ((0 if dosage else capi.NO_DOSAGE) | (capi.RAW_DOSAGE if raw else 0) | (capi.STATIC_JOBS if static_jobs else 0)
             | (capi.ALL_STATES if all_states else 0) | (0 if line_records else capi.NO_LINE_RECORDS)
             | (0 if uniform_pack else capi.NO_UNIFORM_PACK))
    ctx._chk(ctx.L.cnf2_sweep(ctx.h, ind_begin, ind_end, capi._p(out["factors"]), capi._p(out["loglik"]),
                              capi._p(out["dosage"]) if dosage else None, flags), "cnf2_sweep")
    for k, v in out.items():
        assert v is None or not np.isnan(v).any(), "%s: not every cell was written" % k
    return out, ctx.last_uniform_pack()


def _three_forms(capi, ctx, what, groups, **kw):
    """(packed, one job to a wave, ordinary instantiation) of one sweep, equal to the bit; `groups`: the groups the packed call
    must report (None: at least one).  Returns the packed call's outputs."""
    got, pk = _sweep(capi, ctx, **kw)
    if groups is None:
        assert pk["groups"] >= 1 and pk["jobs"] == 4 * pk["groups"], pk
    else:
        assert pk == dict(jobs=4 * groups, groups=groups), (what, pk)
    on = ctx.last_line_records()
    single, pk1 = _sweep(capi, ctx, uniform_pack=False, **kw)
    assert pk1 == dict(jobs=0, groups=0), pk1
    assert ctx.last_line_records() == on, "packed jobs count as swept on records"
    _same(got, single, what + ": four to a wave against one")
    ref, pk2 = _sweep(capi, ctx, all_states=True, **kw)
    assert pk2 == dict(jobs=0, groups=0), pk2
    _same(got, ref, what + ": four to a wave against the ordinary instantiation")
    return got


# ---------------------------------------------------------------- 1: no group, exact groups, leftovers; every tile edge
@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 9])
def test_f2_sizes_and_chromosome_lengths(capi, n):
    ped = _cut(synth.make_f2(n, sum(LENGTHS) - 1, 1, seed=60 + n, chrom_cm=120.0, missing=0.15), LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        got = _three_forms(capi, ctx, "F2 of %d" % n, (n // 4) * len(LENGTHS))
        _sweep(capi, ctx)
        assert ctx.last_line_records()["on_records"] == n * len(LENGTHS)
        if n == 5:
            nd = _three_forms(capi, ctx, "F2 of 5, no rows", len(LENGTHS), dosage=False)
            assert np.array_equal(nd["factors"], got["factors"]) and np.array_equal(nd["loglik"], got["loglik"])
            _three_forms(capi, ctx, "F2 of 5, raw rows", len(LENGTHS), raw=True)
            _same(_three_forms(capi, ctx, "F2 of 5 again", len(LENGTHS)), got, "a sweep after one without rows")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2: a wave takes several groups
@pytest.mark.parametrize("static_jobs", [False, True], ids=["counter", "static_jobs"])
def test_one_block_sweeps_many_groups(capi, static_jobs):
    ped = _cut(synth.make_f2(22, sum(TILE_EDGE_LENGTHS) - 1, 1, seed=21, chrom_cm=30.0, missing=0.15), TILE_EDGE_LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        ref, _ = _sweep(capi, ctx, all_states=True)
        ctx.set_grid_reserve(ONE_BLOCK)          # one block of 4 waves: 35 groups and 14 single jobs
        got, pk = _sweep(capi, ctx, static_jobs=static_jobs)
        assert pk == dict(jobs=4 * 35, groups=35), pk
        _same(got, ref, "one block")
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()


# ---------------------------------------------------------------- 3: groups whose members differ
@pytest.fixture(scope="module")
def crosses(capi):
    ped = _crosses()
    ctx = capi.Context(0)
    ctx.upload(ped)
    yield ped, ctx
    ctx.close()


def test_members_of_several_lines_and_the_cap(capi, crosses):
    ped, ctx = crosses
    got = _three_forms(capi, ctx, "three crosses", 3 * 2)
    _against_oracle(ped, got, "three crosses, four to a wave")
    try:
        ctx.set_line_records(2)                  # individuals 6-8 (B x C) keep the ordinary producer: 9 on records a chromosome
        capped = _three_forms(capi, ctx, "cap of two lines", 2 * 2)
        _sweep(capi, ctx)
        c = ctx.last_line_records()
        assert c["lines"] == 2 and c["on_records"] == 9 * 2 and c["fallback"] == 3 * 2, c
        ctx.set_line_records(1)                  # three on records a chromosome: no group
        one, pk = _sweep(capi, ctx)
        assert pk == dict(jobs=0, groups=0) and ctx.last_line_records()["on_records"] == 3 * 2
    finally:
        ctx.set_line_records(-1)
    _same(capped, got, "cap of two lines")
    _same(one, got, "cap of one line")
    # sub-ranges: other groups of four of the same individuals
    for b, e in ((1, 12), (3, 8), (5, 9)):
        part, pk = _sweep(capi, ctx, ind_begin=b, ind_end=e)
        assert pk["groups"] == (e - b) // 4 * 2, pk
        for k in OUTPUTS:
            assert np.array_equal(part[k], got[k][b:e]), "range [%d, %d): %s differs" % (b, e, k)


def test_every_incoming_value(capi):
    ped = _odd_values()
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        _three_forms(capi, ctx, "odd values", 2 * 2)
    finally:
        ctx.close()


def test_no_live_mode_and_dead_chains_beside_live_jobs(capi):
    """Individual 1 carries, on chromosome 0, an allele no founder has, without genotyping error: no mode has a likelihood.
    Individual 9, (A x B) x (A x C) with a known phase, carries on chromosome 1 an allele only C has: the modes that hand it to
    the A x B parent are dead, the others live.  Both share their waves with ordinary jobs."""
    ped = _crosses()
    ped.allele, ped.sure, ped.hw = ped.allele.copy(), ped.sure.copy(), ped.hw.copy()
    c_row = ped.allele.shape[0] - 1
    root = lambda i: int(ped.row_of[ped.dous[i]])
    m0, m1 = int(ped.chromstarts[0]) + 3, int(ped.chromstarts[1]) + 4
    for m in (m0, m1):
        ped.allele[1, m], ped.allele[2, m], ped.allele[c_row, m] = (1, 1), (2, 2), (3, 3)
        ped.sure[[1, 2, c_row], m] = 0.0
        for i in range(len(ped.dous)):           # (the other roots untyped there: the founders' new alleles contradict nobody)
            ped.allele[root(i), m] = (0, 0)
    ped.allele[root(1), m0] = (3, 3)
    ped.sure[root(1), m0] = 0.0
    ped.allele[root(9), m1] = (3, 1)
    ped.sure[root(9), m1] = 0.0
    ped.hw[root(9), m1] = 0.0
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        got = _three_forms(capi, ctx, "dead jobs and chains", 3 * 2)
    finally:
        ctx.close()
    dead = got["factors"] < DEAD
    print("dead modes per job\n", dead.sum(axis=2))
    assert dead[1, 0].all() and got["loglik"][1, 0] < DEAD and np.all(got["dosage"][1, :int(ped.chromstarts[1])] == 0.0)
    assert 0 < dead[9, 1].sum() < 8 and got["loglik"][9, 1] > DEAD, dead[9, 1]
    others = np.ones(dead.shape[:2], bool)
    others[1, 0] = others[9, 1] = False
    assert not dead[others].any()


def test_dense_rescaling_of_one_member(capi):
    """test_gpu_uniform_spill.py's fixture with four individuals: the first loses about 23 decades a marker on markers 10..49
    and rescales at every second marker from there on, in a wave with three that never do."""
    ped = synth.make_f2(4, 60, 1, seed=5, chrom_cm=30.0, missing=0.0)
    ped.allele, ped.sure = ped.allele.copy(), ped.sure.copy()
    kid = int(ped.row_of[ped.dous[0]])
    ped.allele[kid, 10:50] = (3, 3)
    ped.sure[kid, 10:50] = 1e-12
    ped.sure[1:3, 10:50] = 1e-12
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        got = _three_forms(capi, ctx, "dense rescaling", 1)
    finally:
        ctx.close()
    assert got["loglik"][0, 0] < -1000 and np.all(got["loglik"][1:, 0] > -1000), got["loglik"]


# ---------------------------------------------------------------- 4: the rows change between two sweeps of a context
def test_row_update_between_two_sweeps(capi, crosses):
    ped, ctx = crosses
    first, _ = _sweep(capi, ctx)
    sure = ped.sure[2:3].copy()
    sure[0, [2, 10, 15]] = 0.2                 # founder B, still homozygous with equal sure
    try:
        ctx.update_rows(2, ped.allele[2:3], sure, ped.hw[2:3])
        second = _three_forms(capi, ctx, "after the row update", 3 * 2)
        assert not np.array_equal(second["factors"], first["factors"]) and not np.array_equal(second["dosage"], first["dosage"])
    finally:
        ctx.update_rows(2, ped.allele[2:3], ped.sure[2:3], ped.hw[2:3])
    _same(_sweep(capi, ctx)[0], first, "rows restored")


# ---------------------------------------------------------------- 5: every kind of window in one call; the Viterbi call
def test_mixed_call_and_the_viterbi_likelihoods(capi):
    ped = _append(_crosses(), _append(_cut(_three_founder_cross(2, 3, 19, seed=33, missing=0.1, het_marker=7), (9, 11)),
                                      _cut(synth.make_ail(4, 6, 3, 19, 1, seed=5, chrom_cm=25.0), (9, 11))))
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        paths = ctx.sweep(log_paths=True)["paths"]
        assert {1, 2, 16} <= set(int(x) for x in paths.ravel()), paths
        n_uni = int((paths[:, 0] == 2).sum())
        assert n_uni % 4 != 0, "the fixture should leave single uniform jobs beside the groups"
        got = _three_forms(capi, ctx, "mixed call", n_uni // 4 * 2)
        vit = [ctx.sweep_viterbi(), ctx.sweep_viterbi(uniform_pack=False), ctx.sweep_viterbi(all_states=True)]
        assert ctx.last_uniform_pack() == dict(jobs=0, groups=0)
        ctx.sweep_viterbi()
        assert ctx.last_uniform_pack() == dict(jobs=n_uni // 4 * 8, groups=n_uni // 4 * 2)
        for other in vit[1:]:
            for k in vit[0]:
                assert np.array_equal(vit[0][k], other[k], equal_nan=True), ("sweep_viterbi", k)
        assert np.array_equal(vit[0]["factors"], got["factors"]) and np.array_equal(vit[0]["loglik"], got["loglik"])
    finally:
        ctx.close()
