"""GPU suite (-m gpu): eight uniform windows to a wave (fb_unipack8_kernel).

Two groups of four of a chromosome whose windows have all eight shift modes analysed are swept by one wavefront: on line
records the recursion does not depend on the first parent's shift bit either, and the lanes that would repeat it carry the
second group.  Per job it is the same operations on the same operands in the same order, so three forms are compared with
`np.array_equal`: the default (eights, and fours behind them), `uniform_pack8=False` (CNF2_NO_UNIFORM_PACK8: fours only) and
`uniform_pack=False` or `all_states=True` (one job to a wave; the ordinary instantiation).  Every output array is filled with
NaN before the call, `cnf2_last_uniform_pack8` tells that the kernel ran, and the oracle is compared once at the tolerances
of test_gpu_uniform_states.py."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from test_gpu_line_records import _crosses, _odd_values
from test_gpu_uniform_pack import DEAD, LENGTHS
from test_gpu_uniform_states import (ONE_BLOCK, OUTPUTS, TILE_EDGE_LENGTHS, _against_oracle, _append, _cut, _same,
                                     _three_founder_cross)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def _sweep(capi, ctx, ind_begin=0, ind_end=None, dosage=True, raw=False, static_jobs=False, all_states=False, uniform_pack=True,
           uniform_pack8=True):
    """ctx.sweep() into arrays filled with NaN; returns the outputs, the call's packed jobs and groups, and its eights."""
    ind_end = ctx.n_ind if ind_end is None else ind_end
    n = ind_end - ind_begin
    out = dict(factors=np.full((n, ctx.n_chrom, 8), np.nan), loglik=np.full((n, ctx.n_chrom), np.nan),
               dosage=np.full((n, ctx.n_markers, 3), np.nan) if dosage else None)
    flags = ((0 if dosage else capi.NO_DOSAGE) | (capi.RAW_DOSAGE if raw else 0) | (capi.STATIC_JOBS if static_jobs else 0)
             | (capi.ALL_STATES if all_states else 0) | (0 if uniform_pack else capi.NO_UNIFORM_PACK)
             | (0 if uniform_pack8 else capi.NO_UNIFORM_PACK8))
    ctx._chk(ctx.L.cnf2_sweep(ctx.h, ind_begin, ind_end, capi._p(out["factors"]), capi._p(out["loglik"]),
                              capi._p(out["dosage"]) if dosage else None, flags), "cnf2_sweep")
    for k, v in out.items():
        assert v is None or not np.isnan(v).any(), "%s: not every cell was written" % k
    return out, ctx.last_uniform_pack(), ctx.last_uniform_pack8()


def _three_forms(capi, ctx, what, groups, eights, **kw):
    """(eights, fours only, one job to a wave or the ordinary instantiation) of one sweep, equal to the bit; `groups` and
    `eights`: what the default call must report.  Returns the default call's outputs."""
    got, pk, p8 = _sweep(capi, ctx, **kw)
    assert pk == dict(jobs=4 * groups, groups=groups), (what, pk)
    assert p8 == dict(eights=eights, jobs=8 * eights), (what, p8)
    fours, pk1, p81 = _sweep(capi, ctx, uniform_pack8=False, **kw)
    assert pk1 == pk and p81 == dict(eights=0, jobs=0), (what, pk1, p81)
    _same(got, fours, what + ": eight to a wave against four")
    single, pk2, p82 = _sweep(capi, ctx, uniform_pack=False, **kw)
    assert pk2 == dict(jobs=0, groups=0) and p82 == dict(eights=0, jobs=0), (what, pk2, p82)
    _same(got, single, what + ": eight to a wave against one")
    ref, pk3, p83 = _sweep(capi, ctx, all_states=True, **kw)
    assert pk3 == dict(jobs=0, groups=0) and p83 == dict(eights=0, jobs=0), (what, pk3, p83)
    _same(got, ref, what + ": eight to a wave against the ordinary instantiation")
    return got


# ---------------------------------------------------------------- 1: no eight, exact eights, an eight beside a four, leftovers
@pytest.mark.parametrize("n", [7, 8, 9, 12, 16, 17])
def test_f2_sizes_and_chromosome_lengths(capi, n):
    ped = _cut(synth.make_f2(n, sum(LENGTHS) - 1, 1, seed=80 + n, chrom_cm=120.0, missing=0.15), LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        groups, eights = (n // 4) * len(LENGTHS), (n // 8) * len(LENGTHS)
        got = _three_forms(capi, ctx, "F2 of %d" % n, groups, eights)
        nd = _three_forms(capi, ctx, "F2 of %d, no rows" % n, groups, eights, dosage=False)
        assert np.array_equal(nd["factors"], got["factors"]) and np.array_equal(nd["loglik"], got["loglik"])
        _three_forms(capi, ctx, "F2 of %d, raw rows" % n, groups, eights, raw=True)
        _same(_sweep(capi, ctx)[0], got, "a sweep after one without rows")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2: a wave takes several eights; whole rounds
@pytest.mark.parametrize("static_jobs", [False, True], ids=["counter", "static_jobs"])
def test_one_block_sweeps_whole_rounds_of_eights(capi, static_jobs):
    ped = _cut(synth.make_f2(22, sum(TILE_EDGE_LENGTHS) - 1, 1, seed=21, chrom_cm=30.0, missing=0.15), TILE_EDGE_LENGTHS)
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        ref, _, _ = _sweep(capi, ctx, all_states=True)
        full, pk, p8 = _sweep(capi, ctx)
        assert pk == dict(jobs=4 * 35, groups=35) and p8 == dict(eights=14, jobs=8 * 14), (pk, p8)
        _same(full, ref, "all waves")
        ctx.set_grid_reserve(ONE_BLOCK)          # one block of 4 waves: 14 pairs make 3 rounds of eights, 2 pairs go back to fours
        got, pk, p8 = _sweep(capi, ctx, static_jobs=static_jobs)
        assert pk == dict(jobs=4 * 35, groups=35) and p8 == dict(eights=12, jobs=8 * 12), (pk, p8)
        _same(got, ref, "one block")
        nd, pk, p8 = _sweep(capi, ctx, static_jobs=static_jobs, dosage=False)
        assert p8 == dict(eights=12, jobs=8 * 12), p8
        assert np.array_equal(nd["factors"], ref["factors"]) and np.array_equal(nd["loglik"], ref["loglik"])
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()


# ---------------------------------------------------------------- 3: eights whose members differ
@pytest.fixture(scope="module")
def crosses2(capi):
    ped = _append(_crosses(), _crosses(seed=43))
    ctx = capi.Context(0)
    ctx.upload(ped)
    yield ped, ctx
    ctx.close()


def test_members_of_several_lines_and_the_oracle(capi, crosses2):
    ped, ctx = crosses2
    got = _three_forms(capi, ctx, "three crosses twice", 6 * 2, 3 * 2)
    _against_oracle(ped, got, "three crosses twice, eight to a wave")
    # sub-ranges: other eights of the same individuals
    for b, e in ((1, 24), (3, 12), (5, 22)):
        part, pk, p8 = _sweep(capi, ctx, ind_begin=b, ind_end=e)
        assert pk["groups"] == (e - b) // 4 * 2 and p8["eights"] == (e - b) // 8 * 2, (pk, p8)
        for k in OUTPUTS:
            assert np.array_equal(part[k], got[k][b:e]), "range [%d, %d): %s differs" % (b, e, k)


def test_every_incoming_value(capi):
    ped = _append(_odd_values(), _odd_values(seed=56))
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        _three_forms(capi, ctx, "odd values twice", 4 * 2, 2 * 2)
    finally:
        ctx.close()


def test_no_live_mode_and_dead_chains_beside_live_jobs(capi):
    """test_gpu_uniform_pack.py's fixture, doubled: individual 1 (no mode has a likelihood on chromosome 0) sits in the first
    eight of a chromosome, individual 9 (some modes dead on chromosome 1) in the second; both share their waves with seven
    ordinary jobs."""
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
    ped = _append(ped, _crosses(seed=43))
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        got = _three_forms(capi, ctx, "dead jobs and chains", 6 * 2, 3 * 2)
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
    """test_gpu_uniform_spill.py's fixture with eight individuals: the first loses about 23 decades a marker on markers 10..49
    and rescales at every second marker from there on, in a wave with seven that never do."""
    ped = synth.make_f2(8, 60, 1, seed=5, chrom_cm=30.0, missing=0.0)
    ped.allele, ped.sure = ped.allele.copy(), ped.sure.copy()
    kid = int(ped.row_of[ped.dous[0]])
    ped.allele[kid, 10:50] = (3, 3)
    ped.sure[kid, 10:50] = 1e-12
    ped.sure[1:3, 10:50] = 1e-12
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        got = _three_forms(capi, ctx, "dense rescaling", 2, 1)
    finally:
        ctx.close()
    assert got["loglik"][0, 0] < -1000 and np.all(got["loglik"][1:, 0] > -1000), got["loglik"]


# ---------------------------------------------------------------- 4: the rows change between two sweeps of a context
def test_row_update_between_two_sweeps(capi, crosses2):
    ped, ctx = crosses2
    first, _, _ = _sweep(capi, ctx)
    sure = ped.sure[2:3].copy()
    sure[0, [2, 10, 15]] = 0.2                 # founder B, still homozygous with equal sure
    try:
        ctx.update_rows(2, ped.allele[2:3], sure, ped.hw[2:3])
        second = _three_forms(capi, ctx, "after the row update", 6 * 2, 3 * 2)
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
        assert n_uni // 4 % 2 == 1 and n_uni % 4 != 0, "the fixture should leave a four and single uniform jobs beside the eights"
        got = _three_forms(capi, ctx, "mixed call", n_uni // 4 * 2, n_uni // 8 * 2)
        vit = [ctx.sweep_viterbi(), ctx.sweep_viterbi(uniform_pack8=False), ctx.sweep_viterbi(uniform_pack=False),
               ctx.sweep_viterbi(all_states=True)]
        assert ctx.last_uniform_pack8() == dict(eights=0, jobs=0)
        ctx.sweep_viterbi(uniform_pack8=False)
        assert ctx.last_uniform_pack() == dict(jobs=n_uni // 4 * 8, groups=n_uni // 4 * 2)
        assert ctx.last_uniform_pack8() == dict(eights=0, jobs=0)
        ctx.sweep_viterbi()
        assert ctx.last_uniform_pack() == dict(jobs=n_uni // 4 * 8, groups=n_uni // 4 * 2)
        assert ctx.last_uniform_pack8() == dict(eights=n_uni // 8 * 2, jobs=n_uni // 8 * 16)
        for other in vit[1:]:
            for k in vit[0]:
                assert np.array_equal(vit[0][k], other[k], equal_nan=True), ("sweep_viterbi", k)
        assert np.array_equal(vit[0]["factors"], got["factors"]) and np.array_equal(vit[0]["loglik"], got["loglik"])
    finally:
        ctx.close()
