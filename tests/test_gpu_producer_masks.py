"""GPU suite (-m gpu): the record producer with bit masks in place of selects (cnf2_emtab.h keep_if_bit in emtab_part_rec).

The packed kernels' producer keeps or clears a record's one value per table entry by ANDing a sign-extended bit of the record
into the double; the result must be the value's bits or exact zero, as the select gave.  An F2 of 21 individuals puts two eights,
a four and a single job on every chromosome of one call; chromosomes of 1, 2, 3 and 33 markers; missing genotypes, homozygous and
heterozygous roots, markers where founders and roots are certain (exact zeros in the rows) and one member that rescales densely.
Factors, likelihoods and rows are compared with `np.array_equal` against four routes.  CNF2_NO_LINE_RECORDS is the yardstick: the
ordinary producer never runs this code.  CNF2_NO_UNIFORM_PACK8 (fours), CNF2_NO_UNIFORM_PACK (one job to a wave, on records) and
CNF2_ALL_STATES (the ordinary instantiation) run it in other instantiations or not at all."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from test_gpu_uniform_states import ONE_BLOCK, _cut, _same

pytestmark = pytest.mark.gpu

N_IND = 21
LENGTHS = (1, 2, 3, 33)
C33 = sum(LENGTHS[:3])                  # first marker of the long chromosome
CERTAIN = (C33 + 2, C33 + 31)           # founders and roots typed without error there
DENSE = slice(C33 + 5, C33 + 31)        # where individual 0 contradicts its founders


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def f2_of_21():
    ped = _cut(synth.make_f2(N_IND, sum(LENGTHS) - 1, 1, seed=117, chrom_cm=60.0, missing=0.15), LENGTHS)
    ped.allele, ped.sure, ped.hw = ped.allele.copy(), ped.sure.copy(), ped.hw.copy()
    for m in CERTAIN:
        ped.sure[1:, m] = 0.0
    kid = int(ped.row_of[ped.dous[0]])
    ped.allele[kid, DENSE] = (3, 3)
    ped.sure[kid, DENSE] = 1e-12
    ped.sure[1:3, DENSE] = 1e-12
    return ped


ROUTES = dict(no_line_records=dict(line_records=False), fours=dict(uniform_pack8=False), singles=dict(uniform_pack=False),
              all_states=dict(all_states=True))


def _sweep(capi, ctx, dosage=True, static_jobs=False, line_records=True, uniform_pack=True, uniform_pack8=True, all_states=False,
           ind_begin=0, ind_end=None, extra_flags=0):
    """ctx.sweep() into arrays filled with NaN: every cell must be written."""
    ind_end = ctx.n_ind if ind_end is None else ind_end
    n = ind_end - ind_begin
    out = dict(factors=np.full((n, ctx.n_chrom, 8), np.nan), loglik=np.full((n, ctx.n_chrom), np.nan),
               dosage=np.full((n, ctx.n_markers, 3), np.nan) if dosage else None)
    flags = ((0 if dosage else capi.NO_DOSAGE) | (capi.STATIC_JOBS if static_jobs else 0) | (capi.ALL_STATES if all_states else 0)
             | (0 if line_records else capi.NO_LINE_RECORDS) | (0 if uniform_pack else capi.NO_UNIFORM_PACK)
             | (0 if uniform_pack8 else capi.NO_UNIFORM_PACK8) | extra_flags)
    ctx._chk(ctx.L.cnf2_sweep(ctx.h, ind_begin, ind_end, capi._p(out["factors"]), capi._p(out["loglik"]),
                              capi._p(out["dosage"]) if dosage else None, flags), "cnf2_sweep")
    for k, v in out.items():
        assert v is None or not np.isnan(v).any(), "%s: not every cell was written" % k
    return out


def _against_routes(capi, ctx, what, **kw):
    got = _sweep(capi, ctx, **kw)
    assert ctx.last_uniform_pack() == dict(jobs=4 * 5 * len(LENGTHS), groups=5 * len(LENGTHS)), ctx.last_uniform_pack()
    assert ctx.last_uniform_pack8() == dict(eights=2 * len(LENGTHS), jobs=16 * len(LENGTHS)), ctx.last_uniform_pack8()
    assert ctx.last_line_records()["on_records"] == N_IND * len(LENGTHS)
    for name, route in ROUTES.items():
        other = _sweep(capi, ctx, **dict(kw, **route))
        if name != "fours":
            assert ctx.last_uniform_pack8() == dict(eights=0, jobs=0) and ctx.last_uniform_pack() == dict(jobs=0, groups=0), name
        if name in ("no_line_records", "all_states"):
            assert ctx.last_line_records()["on_records"] == 0, name
        _same(got, other, "%s: the masks' producer against %s" % (what, name))
    return got


@pytest.fixture(scope="module")
def f2ctx(capi):
    ped = f2_of_21()
    ctx = capi.Context(0)
    ctx.upload(ped)
    yield ped, ctx
    ctx.close()


def test_the_four_routes_and_the_fixture(capi, f2ctx):
    ped, ctx = f2ctx
    got = _against_routes(capi, ctx, "F2 of 21")
    # the fixture: missing, homozygous and heterozygous roots ...
    roots = ped.allele[ped.row_of[ped.dous]]
    assert (roots == 0).all(axis=2).any() and (roots[..., 0] == roots[..., 1])[roots[..., 0] != 0].any()
    assert (roots[..., 0] != roots[..., 1]).any()
    # ... rows with exact zeros beside non-zeros (a certain root between certain founders rules genotypes out), on every typed job
    rows = got["dosage"]
    for m in CERTAIN:
        typed = roots[:, m, 0] != 0
        assert typed.any()
        assert (rows[typed, m] == 0.0).any(axis=1).all() and (rows[typed, m] != 0.0).any(axis=1).all(), rows[typed, m]
    # ... and the member that rescales densely, in an eight with seven that never do
    c = len(LENGTHS) - 1
    assert got["loglik"][0, c] < -1000 and np.all(got["loglik"][1:, c] > -1000), got["loglik"][:, c]
    nd = _against_routes(capi, ctx, "F2 of 21, no rows", dosage=False)
    assert np.array_equal(nd["factors"], got["factors"]) and np.array_equal(nd["loglik"], got["loglik"])


def test_static_jobs_and_one_block(capi, f2ctx):
    ped, ctx = f2ctx
    ref = _sweep(capi, ctx, line_records=False)
    _same(_against_routes(capi, ctx, "static jobs", static_jobs=True), ref, "static jobs")
    try:
        ctx.set_grid_reserve(ONE_BLOCK)        # one block of 4 waves takes every job in turn (the 8 eights of the call are two whole rounds)
        for static in (False, True):
            _same(_sweep(capi, ctx, static_jobs=static), ref, "one block, static_jobs=%r" % static)
    finally:
        ctx.set_grid_reserve(0)


def test_after_a_row_update(capi, f2ctx):
    ped, ctx = f2ctx
    first = _sweep(capi, ctx)
    sure = ped.sure[2:3].copy()
    sure[0, [1, 4, C33 + 3, C33 + 32]] = 0.2       # founder B, still homozygous with equal sure
    try:
        ctx.update_rows(2, ped.allele[2:3], sure, ped.hw[2:3])
        second = _against_routes(capi, ctx, "after the row update")
        assert not np.array_equal(second["factors"], first["factors"]) and not np.array_equal(second["dosage"], first["dosage"])
    finally:
        ctx.update_rows(2, ped.allele[2:3], ped.sure[2:3], ped.hw[2:3])
    _same(_sweep(capi, ctx), first, "rows restored")
