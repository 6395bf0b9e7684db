"""GPU suite (-m gpu): the eights read a marker's gap factors through the scalar cache (*The gap's
factors as a scalar load*; cnf2_kernels.hip load_rec<TQ_SHIFT, ONE_MARKER>, fb_unipack8_kernel).

Every lane of a wave of the eights looks at the same marker, so the pair (r / (1 - r) factors) of the gap that the marker's row
carries is one value for the wave: the index is made uniform and the pair is read from the constant address space.  What can
go wrong is the index -- the gap in front of a window's first marker (clamped to the map's first entry), the loads the producer
asks for behind a window's last marker (clamped to it), the forward pass's gap after the marker against the backward pass's
gap before it, a window that does not start at marker 0 -- so the map has chromosomes of 1, 2, 3, 4, 5 and 33 markers with a
spacing of their own each, and the eights are compared with `np.array_equal` against `uniform_pack8=False`
(CNF2_NO_UNIFORM_PACK8), `uniform_pack=False` (CNF2_NO_UNIFORM_PACK) and `all_states=True` (CNF2_ALL_STATES), whose lanes
look at several markers and keep the vector load.

One F2 of 21 individuals: two eights, a four and a single job per chromosome.  Individual 0 loses about 23 decades a marker
from an even marker of the long chromosome on, individual 1 from an odd one (dense rescaling), and individual 5 has no live
mode on the chromosome of 5 markers."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from test_gpu_uniform_pack import DEAD
from test_gpu_uniform_pack8 import _sweep, _three_forms
from test_gpu_uniform_states import ONE_BLOCK, _cut, _same

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 4, 5, 33)
N = 21
GROUPS, EIGHTS = (N // 4) * len(LENGTHS), (N // 8) * len(LENGTHS)
LONG = sum(LENGTHS[:5])             # first marker of the chromosome of 33
DEAD_AT = sum(LENGTHS[:4]) + 2      # a marker of the chromosome of 5


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def _cross():
    ped = _cut(synth.make_f2(N, sum(LENGTHS) - 1, 1, seed=61, chrom_cm=40.0, missing=0.15), LENGTHS)
    ped.allele, ped.sure, ped.hw = ped.allele.copy(), ped.sure.copy(), ped.hw.copy()
    root = lambda i: int(ped.row_of[ped.dous[i]])
    # dense rescaling (test_gpu_uniform_spill.py's way): from local marker 4 (even) and from local marker 5 (odd) on
    ped.sure[1:3, LONG + 4:] = 1e-12
    for i, m in ((0, LONG + 4), (1, LONG + 5)):
        ped.allele[root(i), m:] = (3, 3)
        ped.sure[root(i), m:] = 1e-12
    # no live mode: an allele neither founder has, all three certain (the other roots untyped there)
    ped.sure[1:3, DEAD_AT] = 0.0
    for i in range(N):
        ped.allele[root(i), DEAD_AT] = (0, 0)
        ped.sure[root(i), DEAD_AT] = 0.0
    ped.allele[root(5), DEAD_AT] = (3, 3)
    return ped


@pytest.fixture(scope="module")
def swept(capi):
    """The context and the three references' common value (_three_forms holds them to one another), formed once."""
    ped = _cross()
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = _three_forms(capi, ctx, "F2 of %d" % N, GROUPS, EIGHTS)
    yield ped, ctx, got
    ctx.close()


def test_eights_against_fours_single_jobs_and_all_states(swept):
    ped, ctx, got = swept
    lk = got["loglik"]
    print("loglik of individuals 0, 1, 5\n", lk[[0, 1, 5]])
    assert lk[0, 5] < -500 and lk[1, 5] < -500 and np.all(lk[2:, 5] > -500), "individuals 0 and 1 should rescale densely"
    dead = got["factors"] < DEAD
    assert dead[5, 4].all() and lk[5, 4] < DEAD, "individual 5 should have no live mode on the chromosome of 5"
    first, last = int(ped.chromstarts[4]), int(ped.chromstarts[5])
    assert np.all(got["dosage"][5, first:last] == 0.0)
    dead[5, 4] = False
    assert not dead.any()
    # the gaps count: the chromosomes differ in their spacing, and so do the rows of two typed neighbours on them
    assert len(set(np.round(np.diff(ped.pos)[np.diff(ped.pos) > 0], 6))) >= 4


def test_raw_rows(capi, swept):
    _, ctx, _ = swept
    _three_forms(capi, ctx, "raw rows", GROUPS, EIGHTS, raw=True)


def test_launch_without_rows(capi, swept):
    """dosage=False: the launch of the Viterbi likelihood pass; the forward pass alone reads the gaps."""
    _, ctx, got = swept
    nd = _three_forms(capi, ctx, "no rows", GROUPS, EIGHTS, dosage=False)
    assert np.array_equal(nd["factors"], got["factors"]) and np.array_equal(nd["loglik"], got["loglik"])
    _same(_sweep(capi, ctx)[0], got, "a sweep after one without rows")


@pytest.mark.parametrize("static_jobs", [False, True], ids=["counter", "static_jobs"])
def test_one_block_takes_its_eights_in_turn(capi, swept, static_jobs):
    """A wave sweeps eights of several chromosomes one after the other: the marker its lanes share changes with the job."""
    _, ctx, got = swept
    ctx.set_grid_reserve(ONE_BLOCK)
    try:
        one, pk, p8 = _sweep(capi, ctx, static_jobs=static_jobs)
        assert pk == dict(jobs=4 * GROUPS, groups=GROUPS) and p8["eights"] > 4, (pk, p8)
        _same(one, got, "one block")
    finally:
        ctx.set_grid_reserve(0)
    _same(_sweep(capi, ctx, static_jobs=static_jobs)[0], got, "all waves")


def test_after_a_new_map(capi, swept):
    """The map changes between two sweeps of a context (as the map's EM step changes it): no gap of the old map is seen."""
    ped, ctx, got = swept
    try:
        ctx.upload_map(ped.pos * 1.7, ped.chromstarts)
        second = _three_forms(capi, ctx, "after a new map", GROUPS, EIGHTS)
        assert not np.array_equal(second["loglik"], got["loglik"]) and not np.array_equal(second["dosage"], got["dosage"])
    finally:
        ctx.upload_map(ped.pos, ped.chromstarts)
    _same(_sweep(capi, ctx)[0], got, "map restored")


def test_sub_range_of_individuals(capi, swept):
    """Other eights of the same individuals."""
    _, ctx, got = swept
    part, pk, p8 = _sweep(capi, ctx, ind_begin=3, ind_end=20)
    assert p8["eights"] == 2 * len(LENGTHS), p8
    for k in ("factors", "loglik", "dosage"):
        assert np.array_equal(part[k], got[k][3:20]), k
