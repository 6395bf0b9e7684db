"""GPU suite (-m gpu): the eights load the root's `sure`, `hw` and allele byte once a tile of eight markers and stage them in the
wave's LDS region ("Root staging"; cnf2_lane.h up8_stage_*, fb_unipack8_kernel).

Lane (t, job) loads the root's data of (marker t of a tile, job) a tile or two ahead of its use, and the eight producer lanes of
(marker, job) read it from the LDS -- the allele byte, which forms the record's address, two to four markers ahead of the rest
and so from the next tile's buffer at a tile's end.  What can go wrong is a slot read from the wrong marker, job or buffer, a
clamped load behind a window's end, and a buffer that changes hands too early: between two tiles, between the forward tiles and
the backward rows, between two jobs of a wave.  The bench's rows are the same at every marker, so none of that shows there.
Here **`sure`, `hw` and the alleles of the roots differ for every (individual, marker)**: seeded values, some alleles missing,
some `sure` = 0.

  pedigree   an F2 of 21: per chromosome two eights, one four and one window alone
  map        chromosomes of 1, 2, 3, 7, 8, 9, 15, 16, 17 and 33 markers: one short of, at and past a tile's end for tiles of
             4 and 8; the first starts at marker 0, the last ends at the map's end, and the last individual owns the arrays'
             last row, so the clamped loads touch both ends of the allocations
  rescaling  individual 0 loses about 23 decades a marker from an even marker of the long chromosome on, individual 1 from an
             odd one

Nothing is compared with a tolerance: the default call, CNF2_NO_UNIFORM_PACK8, CNF2_NO_UNIFORM_PACK and CNF2_ALL_STATES -- none
of which runs the staging -- are equal with `np.array_equal`, into outputs filled with NaN of which none may be left
(test_gpu_uniform_pack8.py's helpers)."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from test_gpu_uniform_pack8 import _sweep, _three_forms
from test_gpu_uniform_states import ONE_BLOCK, _cut, _same

pytestmark = pytest.mark.gpu

N = 21
LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33)
GROUPS, EIGHTS = (N // 4) * len(LENGTHS), (N // 8) * len(LENGTHS)
LONG = sum(LENGTHS[:-1])            # first marker of the chromosome of 33
DENSE = ((0, 4), (1, 5))            # (individual, local marker of the long chromosome its dense rescaling starts at)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def _cross():
    ped = _cut(synth.make_f2(N, sum(LENGTHS) - 1, 1, seed=97, chrom_cm=40.0, missing=0.15), LENGTHS)
    ped.allele, ped.sure, ped.hw = ped.allele.copy(), ped.sure.copy(), ped.hw.copy()
    M = ped.n_markers
    roots = np.array([int(ped.row_of[d]) for d in ped.dous])
    assert sorted(roots) == list(range(3, 3 + N)) and roots[-1] == ped.allele.shape[0] - 1, "the last individual owns the last row"
    rng = np.random.default_rng(4242)
    # every (individual, marker) its own sure pair and hw; a sixth of the sure pairs is 0 (a certain genotype)
    sure = rng.uniform(0.001, 0.2, size=(N, M, 2))
    sure[rng.random((N, M)) < 1 / 6] = 0.0
    ped.sure[roots] = sure
    ped.hw[roots] = rng.uniform(0.1, 0.9, size=(N, M))
    # dense rescaling (test_gpu_uniform_spill.py's way): an allele neither founder has, nearly certain, everybody nearly certain of the founders
    ped.sure[1:3, LONG + 4:] = 1e-12
    for i, lo in DENSE:
        ped.allele[roots[i], LONG + lo:] = (3, 3)
        ped.sure[roots[i], LONG + lo:] = 1e-12
    return ped


def _distinct(ped):
    """The fixture does what it is for: no two (individual, marker) share their sure / hw, and the allele bytes vary along a
    row and between the rows."""
    roots = [int(ped.row_of[d]) for d in ped.dous]
    free = np.ones((N, ped.n_markers), bool)
    for i, lo in DENSE:
        free[i, LONG + lo:] = False
    hw = ped.hw[roots][free]
    assert len(np.unique(hw)) == hw.size
    s = ped.sure[roots][free]
    live = s[s[:, 0] > 0]
    assert len(np.unique(live[:, 0])) == len(live) and len(np.unique(live[:, 1])) == len(live)
    assert 0.1 < np.mean(s[:, 0] == 0) < 0.25
    a = ped.allele[roots]
    assert np.any(a == 0) and len({a[i].tobytes() for i in range(N)}) == N
    assert all(len({a[i, m].tobytes() for m in range(ped.n_markers)}) >= 2 for i in range(N))


@pytest.fixture(scope="module")
def swept(capi):
    """The pedigree, its context and the default call's outputs (held to the three other forms once)."""
    ped = _cross()
    assert int(ped.chromstarts[0]) == 0 and int(ped.chromstarts[-1]) == ped.n_markers == ped.allele.shape[1]
    _distinct(ped)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = _three_forms(capi, ctx, "F2 of %d" % N, GROUPS, EIGHTS)
    yield ped, ctx, got
    ctx.close()


def test_eights_against_fours_single_jobs_and_all_states(capi, swept):
    ped, ctx, got = swept
    assert (EIGHTS, GROUPS) == (20, 50)
    paths = ctx.sweep(log_paths=True)["paths"]
    assert np.all(paths == 2), "every window should be a uniform one:\n%r" % paths
    lk = got["loglik"][:, len(LENGTHS) - 1]
    print("loglik of the long chromosome\n", lk)
    assert lk[0] < -500 and lk[1] < -500 and np.all(lk[2:] > -500), "individuals 0 and 1 should rescale densely"
    assert np.all(np.isfinite(got["dosage"])) and np.all(got["dosage"] >= 0.0)
    # the roots' own data counts: with one individual's row in another's place the rows of both change
    assert len({got["dosage"][i].tobytes() for i in range(N)}) == N


def test_raw_rows(capi, swept):
    _, ctx, _ = swept
    _three_forms(capi, ctx, "raw rows", GROUPS, EIGHTS, raw=True)


def test_launch_without_rows(capi, swept):
    """dosage=False: a job's last forward tile is followed by the next job's staging, with no backward pass in between."""
    _, ctx, got = swept
    nd = _three_forms(capi, ctx, "no rows", GROUPS, EIGHTS, dosage=False)
    assert np.array_equal(nd["factors"], got["factors"]) and np.array_equal(nd["loglik"], got["loglik"])
    _same(_sweep(capi, ctx)[0], got, "a sweep after one without rows")


def test_static_jobs(capi, swept):
    """Wave w takes jobs w, w + waves, ...: other windows follow each other in a wave."""
    _, ctx, got = swept
    _same(_three_forms(capi, ctx, "static jobs", GROUPS, EIGHTS, static_jobs=True), got, "static jobs against the counter")


@pytest.mark.parametrize("static_jobs", [False, True], ids=["counter", "static_jobs"])
def test_one_block_takes_its_eights_in_turn(capi, swept, static_jobs):
    """A wave sweeps eights of several chromosomes one after the other: nothing staged for a job may be left for the next
    one's first tile or rows, with rows and without."""
    _, ctx, got = swept
    ctx.set_grid_reserve(ONE_BLOCK)
    try:
        one, pk, p8 = _sweep(capi, ctx, static_jobs=static_jobs)
        assert pk == dict(jobs=4 * GROUPS, groups=GROUPS) and p8["eights"] > 4, (pk, p8)
        _same(one, got, "one block")
        nd, _, p8n = _sweep(capi, ctx, static_jobs=static_jobs, dosage=False)
        assert p8n == p8
        assert np.array_equal(nd["factors"], got["factors"]) and np.array_equal(nd["loglik"], got["loglik"])
    finally:
        ctx.set_grid_reserve(0)
    _same(_sweep(capi, ctx, static_jobs=static_jobs)[0], got, "all waves")


def test_sub_range_of_individuals(capi, swept):
    """Other eights of the same individuals."""
    _, ctx, got = swept
    part, pk, p8 = _sweep(capi, ctx, ind_begin=3, ind_end=20)
    assert p8["eights"] == 2 * len(LENGTHS), p8
    for k in ("factors", "loglik", "dosage"):
        assert np.array_equal(part[k], got[k][3:20]), k


def test_second_sweep_after_a_row_update(capi, swept):
    """One individual's sure, hw and alleles change at the first and last marker of forward and backward tiles of the long
    chromosome (forward tiles start at its local markers 0, 8, ...; backward ones at 32, 24, ...) and of a short one."""
    ped, ctx, got = swept
    ind = 10
    row = int(ped.row_of[ped.dous[ind]])
    at = [LONG + k for k in (0, 7, 8, 15, 16, 17, 24, 25, 32)] + [int(ped.chromstarts[4]), int(ped.chromstarts[5]) - 1]
    allele, sure, hw = ped.allele[row:row + 1].copy(), ped.sure[row:row + 1].copy(), ped.hw[row:row + 1].copy()
    for j, m in enumerate(at):
        allele[0, m] = [a for a in ((1, 1), (1, 2), (2, 2)) if a != tuple(ped.allele[row, m])][j % 2]
        sure[0, m] = (0.011 + 0.001 * j, 0.023 + 0.002 * j)
        hw[0, m] = 0.31 + 0.01 * j
    try:
        ctx.update_rows(row, allele, sure, hw)
        second = _three_forms(capi, ctx, "after the row update", GROUPS, EIGHTS)
        changed = [c for c in range(len(LENGTHS)) if not np.array_equal(second["loglik"][ind, c], got["loglik"][ind, c])]
        assert changed == [4, len(LENGTHS) - 1], changed
        others = np.arange(N) != ind
        assert np.array_equal(second["dosage"][others], got["dosage"][others]), "only the updated individual's rows change"
        for m in at:
            assert not np.array_equal(second["dosage"][ind, m], got["dosage"][ind, m]), m
    finally:
        ctx.update_rows(row, ped.allele[row:row + 1], ped.sure[row:row + 1], ped.hw[row:row + 1])
    _same(_sweep(capi, ctx)[0], got, "rows restored")


def test_after_a_new_map(capi, swept):
    """The map changes between two sweeps of a context: the staged data is the rows', which stay."""
    ped, ctx, got = swept
    try:
        ctx.upload_map(ped.pos * 1.7, ped.chromstarts)
        second = _three_forms(capi, ctx, "after a new map", GROUPS, EIGHTS)
        assert not np.array_equal(second["loglik"], got["loglik"]) and not np.array_equal(second["dosage"], got["dosage"])
    finally:
        ctx.upload_map(ped.pos, ped.chromstarts)
    _same(_sweep(capi, ctx)[0], got, "map restored")
