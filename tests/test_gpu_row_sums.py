"""GPU suite (-m gpu): the eights add up a marker's row partials in registers ("Row sums in registers").

A lane of fb_unipack8_kernel takes its b0 partner's class sums, forms the eight partials of one chain and adds them in the
order of a one-job sweep; the job's eight chains are added across lanes (s0, s1, s2) and the job's lead lane stores the row.
Nothing is parked in the table row any more, and a backward marker keeps two fences: behind the producer and behind the row's
last reader.  The fours and the ordinary instantiation run none of that code, so they are the yardsticks:

  pedigree   an F2 of 21: per chromosome two eights, one four and one window alone
  map        chromosomes of 1, 2, 3, 4 and 33 markers: both parities of last - first, an odd last marker, and a window long
             enough for several hand-overs of the row from its readers to the next marker's producer; the first chromosome
             starts at marker 0 and the last ends on the arrays' end
  values     individual 3 (an eight) holds every incoming allele value, missing and the sentinel included
  dead       individual 5 (an eight) has no live mode on the long chromosome: scale = 0 in all of its lanes
  rescaling  individuals 0 and 9 (two eights) rescale densely on the long chromosome from an even and from an odd marker
  crosses    test_gpu_uniform_pack8.py's three crosses, doubled: individual 9 of (A x B) x (A x C) loses the chains of one s0
             only, beside live ones: scale = 0 in half of the lanes that exchange and add

Nothing is compared with a tolerance: the default call, CNF2_NO_UNIFORM_PACK8, CNF2_NO_UNIFORM_PACK and CNF2_ALL_STATES are
equal with `np.array_equal`, into outputs filled with NaN of which none may be left (test_gpu_uniform_pack8.py's helpers)."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from test_gpu_line_records import _crosses
from test_gpu_uniform_pack import DEAD
from test_gpu_uniform_pack8 import _sweep, _three_forms
from test_gpu_uniform_states import ONE_BLOCK, _append, _cut, _same

pytestmark = pytest.mark.gpu

N_IND = 21
LENGTHS = (1, 2, 3, 4, 33)
GROUPS, EIGHTS = (N_IND // 4) * len(LENGTHS), (N_IND // 8) * len(LENGTHS)
LONG0 = sum(LENGTHS[:-1])          # the long chromosome's first marker
LONG = len(LENGTHS) - 1
DENSE = ((0, 10, 33), (9, 11, 33))          # (individual, first and end marker on the long chromosome) of the dense rescaling
EVERY, NO_MODE, NO_MODE_AT = 3, 5, LONG0 + 5
NINES = (1, 4, LONG0 + 2)                   # where individual 3 holds the sentinel


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def _pedigree():
    ped = _cut(synth.make_f2(N_IND, sum(LENGTHS) - 1, 1, seed=311, chrom_cm=120.0, missing=0.15), LENGTHS)
    ped.allele, ped.sure, ped.hw = ped.allele.copy(), ped.sure.copy(), ped.hw.copy()
    M = ped.n_markers
    root = lambda i: int(ped.row_of[ped.dous[i]])
    # every incoming value: all pairs of (missing, 1, 2, 3) in turn, and the sentinel 9 alone and beside a value (where a root
    # holds it the empty parents' blank row gets a sure above 0, a known allele that fits no founder keeps one: the job lives)
    k = root(EVERY)
    for m in range(M):
        ped.allele[k, m] = ((m + 5) % 16 // 4, (m + 5) % 4)
    for m, pair in zip(NINES, ((9, 9), (9, 1), (2, 9))):
        ped.allele[k, m] = pair
    ped.sure[0, list(NINES)] = 0.25
    ped.sure[k] = np.where(ped.allele[k] != 0, np.array([0.02, 0.37, 0.5])[np.arange(M) % 3][:, None], 0.0)
    # no live mode: the founders are certainly 1 1 and 2 2 at one marker, the root certainly 3 3 (the other roots untyped there)
    ped.allele[1, NO_MODE_AT], ped.allele[2, NO_MODE_AT] = (1, 1), (2, 2)
    ped.sure[[1, 2], NO_MODE_AT] = 0.0
    for i in range(N_IND):
        ped.allele[root(i), NO_MODE_AT] = (0, 0)
        ped.sure[root(i), NO_MODE_AT] = 0.0
    ped.allele[root(NO_MODE), NO_MODE_AT] = (3, 3)
    ped.sure[root(NO_MODE), NO_MODE_AT] = 0.0
    # test_gpu_uniform_spill.py's dense rescaling: about 23 decades lost per marker
    for ind, lo, hi in DENSE:
        ped.allele[root(ind), LONG0 + lo:LONG0 + hi] = (3, 3)
        ped.sure[root(ind), LONG0 + lo:LONG0 + hi] = 1e-12
    ped.sure[1:3, LONG0 + 10:LONG0 + 33] = 1e-12
    return ped


@pytest.fixture(scope="module")
def rows(capi):
    """The pedigree, its context and the default call's outputs (checked against the three other forms once)."""
    ped = _pedigree()
    assert ped.n_markers == 43 == ped.allele.shape[1]
    assert int(ped.chromstarts[0]) == 0 and int(ped.chromstarts[-1]) == ped.n_markers
    assert ped.allele.shape[0] == 24 and int(ped.row_of[ped.dous[-1]]) == 23, "the last individual should own the last row"
    ctx = capi.Context(0)
    ctx.upload(ped)
    ref = _three_forms(capi, ctx, "row sums", GROUPS, EIGHTS)
    yield ped, ctx, ref
    ctx.close()


def test_the_forms_agree_and_the_fixture_does_what_it_is_for(capi, rows):
    ped, ctx, ref = rows
    assert (EIGHTS, GROUPS) == (10, 25)
    paths = ctx.sweep(log_paths=True)["paths"]
    assert np.all(paths == 2), "every window should be a uniform one:\n%r" % paths
    _same(_sweep(capi, ctx)[0], ref, "the same call again")
    assert np.all(np.isfinite(ref["dosage"])) and np.all(ref["dosage"] >= 0.0)
    dead = ref["factors"] < DEAD
    print("dead modes per job\n", dead.sum(axis=2), "\nloglik of the long chromosome\n", ref["loglik"][:, LONG])
    # one job without a live mode, in a wave with seven ordinary ones: its rows are zero, nobody else's
    assert dead[NO_MODE, LONG].all() and ref["loglik"][NO_MODE, LONG] < DEAD and np.all(ref["dosage"][NO_MODE, LONG0:] == 0.0)
    others = np.ones(dead.shape[:2], bool)
    others[NO_MODE, LONG] = False
    assert not dead[others].any()
    dense = np.zeros(N_IND, bool)
    dense[[d[0] for d in DENSE]] = True
    zero = ref["dosage"].sum(axis=2) == 0.0
    print("rows that are zero (individual, marker)\n", np.argwhere(zero).T)
    ordinary = ~dense
    ordinary[NO_MODE] = False
    assert not zero[:, :LONG0].any() and not zero[ordinary].any()
    # the two members rescale densely, nobody else does
    live = np.arange(N_IND) != NO_MODE
    long_ll = ref["loglik"][:, LONG]
    assert np.all(long_ll[dense] < -1000) and np.all(long_ll[~dense & live] > -1000), long_ll
    # the member with every value holds them
    k = int(ped.row_of[ped.dous[EVERY]])
    assert {tuple(x) for x in ped.allele[k].tolist()} >= {(a, b) for a in range(4) for b in range(4)} | {(9, 9), (9, 1), (2, 9)}


@pytest.mark.parametrize("kw", [dict(raw=True), dict(static_jobs=True), dict(raw=True, static_jobs=True)], ids=["raw", "static_jobs", "raw_static"])
def test_raw_rows_and_static_jobs(capi, rows, kw):
    ped, ctx, ref = rows
    got = _three_forms(capi, ctx, "row sums, %r" % kw, GROUPS, EIGHTS, **kw)
    if not kw.get("raw"):
        _same(got, ref, "static jobs against the counter")
    else:
        assert np.array_equal(got["factors"], ref["factors"]) and np.array_equal(got["loglik"], ref["loglik"])
        # raw rows: the sums themselves, positive where a job lives
        tot = got["dosage"].sum(axis=2)
        ordinary = np.ones(N_IND, bool)
        ordinary[[NO_MODE] + [d[0] for d in DENSE]] = False
        assert np.all(tot[ordinary] > 0.0) and np.all(got["dosage"][NO_MODE, LONG0:] == 0.0)
        assert not np.array_equal(got["dosage"], ref["dosage"])
    _same(_sweep(capi, ctx)[0], ref, "the default call afterwards")


@pytest.mark.parametrize("static_jobs", [False, True], ids=["counter", "static_jobs"])
def test_one_block_takes_several_eights_in_turn(capi, rows, static_jobs):
    """A wave's region goes from a job's last backward marker to the next job's first forward tile behind one fence."""
    ped, ctx, ref = rows
    try:
        ctx.set_grid_reserve(ONE_BLOCK)          # one block of 4 waves: 10 pairs make 2 rounds of eights, 2 pairs go back to fours
        got, pk, p8 = _sweep(capi, ctx, static_jobs=static_jobs)
        assert pk == dict(jobs=4 * GROUPS, groups=GROUPS) and p8 == dict(eights=8, jobs=8 * 8), (pk, p8)
        _same(got, ref, "one block")
        raw, _, p8 = _sweep(capi, ctx, static_jobs=static_jobs, raw=True)
        assert p8 == dict(eights=8, jobs=8 * 8), p8
    finally:
        ctx.set_grid_reserve(0)
    _same(_sweep(capi, ctx, raw=True)[0], raw, "raw rows: all waves against one block")
    _same(_sweep(capi, ctx)[0], ref, "all waves again")


def test_second_sweep_after_a_row_update(capi, rows):
    ped, ctx, ref = rows
    sure = ped.sure[2:3].copy()
    sure[0, [0, 1, 2, 5, LONG0, LONG0 + 7, ped.n_markers - 1]] = 0.2          # founder B, still homozygous with equal sure
    try:
        ctx.update_rows(2, ped.allele[2:3], sure, ped.hw[2:3])
        second = _three_forms(capi, ctx, "after the row update", GROUPS, EIGHTS)
        assert not np.array_equal(second["factors"], ref["factors"]) and not np.array_equal(second["dosage"], ref["dosage"])
    finally:
        ctx.update_rows(2, ped.allele[2:3], ped.sure[2:3], ped.hw[2:3])
    _same(_sweep(capi, ctx)[0], ref, "rows restored")


# ---------------------------------------------------------------- dead chains for one s0 only, beside live ones
def _half_dead_crosses():
    """test_gpu_uniform_pack8.py's fixture of dead chains: at one marker of chromosome 1 the founders are certainly 1 1, 2 2 and
    3 3, and individual 9, of (A x B) x (A x C), is certainly 3 1 in that phase: the allele 3 comes through the second parent."""
    ped = _crosses()
    ped.allele, ped.sure, ped.hw = ped.allele.copy(), ped.sure.copy(), ped.hw.copy()
    c_row = ped.allele.shape[0] - 1
    root = lambda i: int(ped.row_of[ped.dous[i]])
    m1 = int(ped.chromstarts[1]) + 4
    ped.allele[1, m1], ped.allele[2, m1], ped.allele[c_row, m1] = (1, 1), (2, 2), (3, 3)
    ped.sure[[1, 2, c_row], m1] = 0.0
    for i in range(len(ped.dous)):
        ped.allele[root(i), m1] = (0, 0)
    ped.allele[root(9), m1] = (3, 1)
    ped.sure[root(9), m1] = 0.0
    ped.hw[root(9), m1] = 0.0
    return _append(ped, _crosses(seed=43))


def test_dead_chains_for_one_s0_only(capi):
    ped = _half_dead_crosses()
    ctx = capi.Context(0)
    ctx.upload(ped)
    try:
        got = _three_forms(capi, ctx, "chains of one s0 dead", 6 * 2, 3 * 2)
        dead = got["factors"] < DEAD
        print("dead modes per job\n", dead.sum(axis=2), "\nindividual 9, chromosome 1:", dead[9, 1])
        # mode = s0 | s1 << 1 | s2 << 2: the modes of one s0 are dead, those of the other live, and so is everybody else
        s0 = np.arange(8) & 1
        assert np.array_equal(dead[9, 1], s0 == 0) or np.array_equal(dead[9, 1], s0 == 1), dead[9, 1]
        assert got["loglik"][9, 1] > DEAD and np.all(got["dosage"][9].sum(axis=1) > 0.0)
        others = np.ones(dead.shape[:2], bool)
        others[9, 1] = False
        assert not dead[others].any()
        _three_forms(capi, ctx, "chains of one s0 dead, raw rows", 6 * 2, 3 * 2, raw=True)
        _same(_three_forms(capi, ctx, "chains of one s0 dead, static jobs", 6 * 2, 3 * 2, static_jobs=True), got, "static jobs")
        try:
            ctx.set_grid_reserve(ONE_BLOCK)      # one block of 4 waves: 6 pairs make 1 round of eights, 2 pairs go back to fours
            one, pk, p8 = _sweep(capi, ctx)
            assert p8 == dict(eights=4, jobs=8 * 4), p8
            _same(one, got, "one block")
        finally:
            ctx.set_grid_reserve(0)
    finally:
        ctx.close()
