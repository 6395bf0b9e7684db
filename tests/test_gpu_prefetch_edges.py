"""GPU suite (-m gpu): the ends of a window in the packed sweep kernels ("Prefetch across a marker").

fb_unipack8_kernel and fb_unipack_kernel ask for the next marker's (the next tile's) root data and line record without a
condition, and the eights ask for the backward pass's spill values at one place, a marker ahead: behind a window's end the
clamps make them read the window's end again.  A clamp that is off by one shows only there, so the shapes are the ends:

  pedigree   an F2 of 21: per chromosome two eights, one four and one window alone (the UNI form of fb_fast_kernel)
  map        chromosomes of 1, 2, 3, 4, 5 and 258 markers: both parities of last - first, the pair index below 0, and on the
             long one two individuals that rescale at every second marker from some marker on (one from an even marker in an
             eight, one from an odd marker in the four), so that the spilled reciprocals differ from pair to pair
  placement  the first chromosome starts at marker 0, the last one ends at the map's last marker, and the last individual owns
             the last row of the genotype arrays: a read past a window's end leaves an allocation, not a neighbour's row

Nothing is compared with a tolerance: the default call, CNF2_NO_UNIFORM_PACK8, CNF2_NO_UNIFORM_PACK and CNF2_ALL_STATES are
equal with `np.array_equal`, into outputs filled with NaN of which none may be left (test_gpu_uniform_pack8.py's helpers)."""
import numpy as np
import pytest

from cnf2freq_amd import synth
from test_gpu_uniform_pack8 import _sweep, _three_forms
from test_gpu_uniform_states import _cut, _same

pytestmark = pytest.mark.gpu

N_IND = 21
LENGTHS = (1, 2, 3, 4, 5, 258)
GROUPS, EIGHTS = (N_IND // 4) * len(LENGTHS), (N_IND // 8) * len(LENGTHS)
LONG0 = sum(LENGTHS[:-1])          # the long chromosome's first marker
DENSE = ((0, 10, 50), (17, 11, 50))          # (individual, first and end marker on the long chromosome) of the dense rescaling


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def _pedigree():
    ped = _cut(synth.make_f2(N_IND, sum(LENGTHS) - 1, 1, seed=211, chrom_cm=120.0, missing=0.15), LENGTHS)
    ped.allele, ped.sure = ped.allele.copy(), ped.sure.copy()
    # test_gpu_uniform_spill.py's dense rescaling: about 23 decades lost per marker
    for ind, lo, hi in DENSE:
        kid = int(ped.row_of[ped.dous[ind]])
        ped.allele[kid, LONG0 + lo:LONG0 + hi] = (3, 3)
        ped.sure[kid, LONG0 + lo:LONG0 + hi] = 1e-12
    ped.sure[1:3, LONG0 + 10:LONG0 + 50] = 1e-12
    return ped


@pytest.fixture(scope="module")
def edges(capi):
    """The pedigree, its context and the default call's outputs (checked against the three other forms once)."""
    ped = _pedigree()
    assert int(ped.chromstarts[0]) == 0 and int(ped.chromstarts[-1]) == ped.n_markers == ped.allele.shape[1]
    assert int(ped.row_of[ped.dous[-1]]) == ped.allele.shape[0] - 1, "the last individual should own the last row"
    ctx = capi.Context(0)
    ctx.upload(ped)
    ref = _three_forms(capi, ctx, "window ends", GROUPS, EIGHTS)
    yield ped, ctx, ref
    ctx.close()


def test_the_call_runs_the_three_kernels_and_the_forms_agree(capi, edges):
    ped, ctx, ref = edges
    got, pk, p8 = _sweep(capi, ctx)
    # 12 eights and 6 fours behind them; 126 - 120 = 6 windows alone: one per chromosome
    assert p8 == dict(eights=EIGHTS, jobs=8 * EIGHTS) and pk == dict(jobs=4 * GROUPS, groups=GROUPS), (pk, p8)
    assert N_IND * len(LENGTHS) - pk["jobs"] == len(LENGTHS)
    paths = ctx.sweep(log_paths=True)["paths"]
    assert np.all(paths == 2), "every window should be a uniform one:\n%r" % paths
    _same(got, ref, "the same call again")
    # the fixture does what it is for: the two individuals rescale densely on the long chromosome, nobody else does
    long_ll = ref["loglik"][:, len(LENGTHS) - 1]
    dense = np.zeros(N_IND, bool)
    dense[[d[0] for d in DENSE]] = True
    print("loglik of the long chromosome\n", long_ll)
    assert np.all(long_ll[dense] < -1000) and np.all(long_ll[~dense] > -1000), long_ll
    assert np.all(np.isfinite(ref["dosage"])) and np.all(ref["dosage"] >= 0.0)


@pytest.mark.parametrize("raw", [False, True], ids=["rows", "raw_rows"])
def test_static_jobs_and_raw_rows(capi, edges, raw):
    """Wave w takes jobs w, w + waves, ...: other windows follow each other in a wave, and its spill slots."""
    ped, ctx, ref = edges
    got = _three_forms(capi, ctx, "static jobs", GROUPS, EIGHTS, static_jobs=True, raw=raw)
    if not raw:
        _same(got, ref, "static jobs against the counter")


def test_likelihood_launches_read_no_spill_row_and_agree(capi, edges):
    ped, ctx, ref = edges
    nd = _three_forms(capi, ctx, "no rows", GROUPS, EIGHTS, dosage=False)
    assert np.array_equal(nd["factors"], ref["factors"]) and np.array_equal(nd["loglik"], ref["loglik"])
    vit = ctx.sweep_viterbi()
    assert ctx.last_uniform_pack8() == dict(eights=EIGHTS, jobs=8 * EIGHTS)
    assert np.array_equal(vit["factors"], ref["factors"]) and np.array_equal(vit["loglik"], ref["loglik"])
    for kw in (dict(uniform_pack8=False), dict(uniform_pack=False)):
        other = ctx.sweep_viterbi(**kw)
        assert np.array_equal(other["factors"], ref["factors"]) and np.array_equal(other["loglik"], ref["loglik"]), kw
    _same(_sweep(capi, ctx)[0], ref, "a sweep after the launches without rows")


def test_second_sweep_after_a_row_update_reuses_the_spill_slots(capi, edges):
    ped, ctx, ref = edges
    sure = ped.sure[2:3].copy()
    sure[0, [0, 1, 2, 5, 14, LONG0, LONG0 + 7, ped.n_markers - 1]] = 0.2          # founder B, still homozygous with equal sure
    try:
        ctx.update_rows(2, ped.allele[2:3], sure, ped.hw[2:3])
        second = _three_forms(capi, ctx, "after the row update", GROUPS, EIGHTS)
        assert not np.array_equal(second["factors"], ref["factors"]) and not np.array_equal(second["dosage"], ref["dosage"])
    finally:
        ctx.update_rows(2, ped.allele[2:3], ped.sure[2:3], ped.hw[2:3])
    _same(_sweep(capi, ctx)[0], ref, "rows restored")
