"""GPU suite (-m gpu): the six analysis sweeps through the persistent job loop.

cnf2_sweep_crossovers, _viterbi, _sample, _place, _loo and _origins each run an instantiation of fb_fast_kernel of their own
(the crossover mode also one of fb_kernel, for tied windows), and a wave of those kernels that finishes a job takes the next:
the Viterbi vector with its exponent and the decision words in the spill slot, a sampling wave's walks, the leave-one-out
ratios, the masked origin sums, the crossover counts, a placement batch's posterior slot -- whatever a wave carries from job
k to job k + 1 has to be rebuilt per job.  A fixture with fewer jobs than resident waves (2 048 and more) gives every wave
one job, so, as tests/test_gpu_persistent.py does for the plain sweep, cnf2_set_grid_reserve leaves all but ONE block free
here: 4 waves sweep every job of small fixtures built so that a wave's consecutive jobs differ in what they leave behind --
a chromosome of 64 markers before chromosomes of 1 to 17, tied after untied passes in the same slots, 2-mode windows between
8-mode ones, a skipped job before a live one.  The assignment of jobs to waves is the planner's (cnf2_plan.h: untied windows'
jobs first, chromosomes longest first, individuals ascending; with CNF2_STATIC_JOBS wave w takes jobs w, w + 4, ...): it is
restated here (job_lists, held against the planner itself by tests/test_host_plan.py) and what the tests rely on is asserted.  One block must equal the full grid to the bit (sums that the header documents as f64 atomics
in order of arrival: to the bar tests/test_gpu_uniform_states.py sets for them) and the oracle at each mode's own tolerance.
The descent and the pair sweep, which came after these six, go through the same loop on the same fixtures in
tests/test_gpu_persistent_rows.py, which imports this file's fixtures and helpers."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_crossovers as xo_suite
import test_gpu_loo as loo_suite
import test_gpu_origins as org_suite
import test_gpu_placement as place_suite
import test_gpu_sampling as smp_suite
import test_gpu_viterbi as vit_suite
from cnf2freq_amd import synth
from conftest import oracle_ped
from test_gpu_origins import LENGTHS
from test_gpu_persistent import ONE_BLOCK, capi  # noqa: F401  (the fixture: builds, and asserts a device)
from test_gpu_uniform_states import _append, _cut, _three_founder_cross
from test_loo_host import oracle_loo, oracle_unlinked
from test_origins_host import oracle_origins

pytestmark = pytest.mark.gpu

WAVES = 4                    # of the one block
PATH_UNIFORM, PATH_HOM, PATH_TIED = 2, 1, 16      # what CNF2_LOG_PATHS reports (tests/test_gpu_uniform_states.py)
MODES = ["crossovers", "viterbi", "sample", "place", "loo", "origins"]
FIXTURES = ["f2", "outbred3", "tied_mixed", "f2_skipped"]
MIXED_LENGTHS = LENGTHS + [64]
TIED_LENGTHS = [1, 2, 8, 9, 17]
DRAWS, SEED = 8, 2027
# added up with f64 atomics in order of arrival (include/cnf2hip.h): not the same bits from run to run
ATOMIC_SUMS = ("xo_sum", "place_sum", "null")
# per mode: what a call returns per individual, summed over the range, and counted
ROWS = dict(crossovers=("xo",), viterbi=("logmax", "state", "shift", "path_logpost"), sample=("state", "shift", "logp"),
            place=("place",), loo=("loo", "unlinked"), origins=("origin", "bits"))
SUMS = dict(crossovers=("xo_sum",), viterbi=(), sample=(), place=("place_sum", "null"), loo=("loo_sum", "unlinked_sum"),
            origins=("origin_sum",))
COUNTS = dict(crossovers=("n_contrib",), viterbi=(), sample=(), place=("n_contrib", "n_zero"), loo=("n_contrib",),
              origins=("n_contrib",))
# a range split adds up "to rounding": the tolerance each mode's own file asserts for it (test_bookkeeping and its like)
SPLIT_TOL = dict(xo_sum=dict(rtol=1e-12, atol=1e-13), place_sum=dict(rtol=1e-12), null=dict(rtol=1e-12),
                 loo_sum=dict(rtol=1e-12), unlinked_sum=dict(rtol=1e-12), origin_sum=dict(rtol=1e-12, atol=1e-12))


# ---------------------------------------------------------------------------------------------- fixtures
class Fixture:
    def __init__(self, name, ped, skipped=()):
        self.name, self.ped = name, ped
        self.skipped = list(skipped)                  # (individual, chromosome) pairs without a likelihood
        self.cand = place_suite.own_columns_as_candidates(ped, 3)
        self.n, self.C = len(ped.dous), len(ped.chromstarts) - 1
        self.oracle = {}


def _mixed_f2():
    ped = synth.make_f2(16, sum(MIXED_LENGTHS) - 1, 1, seed=21, chrom_cm=150.0, missing=0.1)
    return _cut(ped, MIXED_LENGTHS)


def _build(name):
    if name == "f2":
        return Fixture(name, _mixed_f2())
    if name == "outbred3":
        ped = synth.make_outbred3(4, 4, sum(MIXED_LENGTHS) - 1, 1, seed=23, chrom_cm=150.0, random_hw=True, random_sure=True)
        return Fixture(name, _cut(ped, MIXED_LENGTHS))
    if name == "tied_mixed":
        # uniform (A x B) and hom == 1 (A x C) windows, then an advanced intercross with tied and untied windows; two F1s
        # of the intercross (generation 1: two shift modes) are analysed between the 8-mode individuals of the cross
        cross = _three_founder_cross(5, 4, sum(TIED_LENGTHS) - 1, seed=33, missing=0.1, het_marker=7)
        ail = synth.make_ail(4, 6, 4, sum(TIED_LENGTHS) - 1, 1, seed=7, chrom_cm=25.0, missing=0.05)
        ped = _append(cross, ail)
        f1 = [cross.n_rec + 2, cross.n_rec + 3]
        assert ped.names[f1[0]] == "x_F1_0" and np.all(ped.gen[f1] == 1)
        dous = list(ped.dous)
        dous.insert(2, f1[0])
        dous.insert(7, f1[1])
        ped.dous = np.array(dous, np.int32)
        return Fixture(name, _cut(ped, TIED_LENGTHS))
    if name == "f2_skipped":
        # the F2 above; individuals 3 and 10 carry an allele neither founder has, without genotyping error at that marker
        # in the child and both founders, on chromosome 12 (17 markers) and chromosome 6 (7 markers)
        ped = _mixed_f2()
        ped.allele, ped.sure = ped.allele.copy(), ped.sure.copy()
        skipped = [(3, 12), (10, 6)]
        for j, c in skipped:
            m = int(ped.chromstarts[c]) + 3
            ped.allele[3 + j, m] = 3
            ped.sure[[1, 2, 3 + j], m] = 0.0
        return Fixture(name, ped, skipped)
    raise KeyError(name)


_FIXTURES = {}


def fixture(name):
    """built once per module and left unchanged; its oracle results are cached in it"""
    if name not in _FIXTURES:
        _FIXTURES[name] = _build(name)
    return _FIXTURES[name]


def job_lists(fx, paths):
    """the (individual, chromosome) pairs of a call's two launches, untied and tied, in the planner's order: chromosomes longest
    first (equal lengths in map order), individuals ascending (cnf2_plan.h; tests/test_host_plan.py).  paths: what
    CNF2_LOG_PATHS reports, which tells the windows the planner lists as tied (cnf2_window_info does not: it shows the tie
    groups before those of ancestors that are homozygous everywhere are dropped).  The placement sweep lists every window as
    untied, in the same order"""
    lens = np.diff(np.asarray(fx.ped.chromstarts))
    order = sorted(range(fx.C), key=lambda c: -lens[c])
    tied = [bool(np.all(paths[j] == PATH_TIED)) for j in range(fx.n)]
    return [[(j, c) for c in order for j in range(fx.n) if tied[j] == t] for t in (False, True)]


def check_fixture(ctx, fx):
    """the job counts and the job order the tests of this file rely on, under CNF2_STATIC_JOBS on one block"""
    ped = fx.ped
    lens = np.diff(np.asarray(ped.chromstarts))
    paths = ctx.sweep(log_paths=True, dosage=False)["paths"]
    assert np.all((paths == PATH_TIED) == (paths[:, :1] == PATH_TIED)), "an individual's windows are tied on every chromosome or on none"
    untied, tied = job_lists(fx, paths)
    if fx.name in ("f2", "outbred3", "f2_skipped"):
        assert list(lens) == MIXED_LENGTHS and fx.n >= 16 and not tied
        assert len(untied) == fx.n * fx.C >= 240
        for w in range(WAVES):
            mine = [lens[c] for _, c in untied[w::WAVES]]
            assert len(mine) >= 50
            # the 64-marker job's spill rows and decision words outlast the shorter job this wave takes next
            assert any(a == 64 and b < 64 for a, b in zip(mine, mine[1:])), mine
        if fx.name == "outbred3":
            assert not set(int(x) for x in paths.ravel()) & {PATH_UNIFORM, PATH_HOM, PATH_TIED}, "neither homozygous parents nor ties"
        else:
            assert np.all(paths == PATH_UNIFORM), "an F2's windows are uniform"
    if fx.name == "f2_skipped":
        ll = ctx.sweep(dosage=False)["loglik"]
        dead = ~org_suite.has_lik(ll)
        assert sorted(zip(*np.nonzero(dead))) == sorted(fx.skipped)
        inds, chroms = [j for j, _ in fx.skipped], [c for _, c in fx.skipped]
        assert abs(inds[0] - inds[1]) > 1 and fx.C - 1 not in chroms
        for pair in fx.skipped:
            k = untied.index(pair)
            assert k + WAVES < len(untied) and untied[k + WAVES] not in fx.skipped, "the wave's next job is a live one"
    if fx.name == "tied_mixed":
        assert list(lens) == TIED_LENGTHS
        assert len(tied) >= 40 and len(untied) >= 100, (len(tied), len(untied))
        kinds = set(int(x) for x in paths.ravel())
        assert {PATH_UNIFORM, PATH_HOM, PATH_TIED} <= kinds, kinds
        two = [j for j in range(fx.n) if ped.gen[ped.dous[j]] < 2]
        assert len(two) >= 2
        for j in two:
            assert ped.gen[ped.dous[j - 1]] >= 2 and ped.gen[ped.dous[j + 1]] >= 2
            assert np.all(paths[j] != PATH_TIED)
            f = ctx.sweep(ind_begin=j, ind_end=j + 1, dosage=False)["factors"]
            assert np.all((f > -1e29).sum(axis=2) == 2), "two shift modes"
        # a 2-mode job followed by an 8-mode job in the same wave
        follows = 0
        for w in range(WAVES):
            mine = [j in two for j, _ in untied[w::WAVES]]
            follows += sum(1 for a, b in zip(mine, mine[1:]) if a and not b)
        assert follows >= 2, follows
    return untied, tied


def open_ctx(capi, fx):
    ctx = capi.Context(0)
    ctx.upload(fx.ped)
    return ctx


def run(mode, ctx, fx, **kw):
    if mode == "crossovers":
        return ctx.sweep_crossovers(**kw)
    if mode == "viterbi":
        return ctx.sweep_viterbi(**kw)
    if mode == "sample":
        return ctx.sweep_sample(draws=DRAWS, seed=SEED, **kw)
    if mode == "place":
        return ctx.sweep_place(*fx.cand, per_individual=True, **kw)
    if mode == "loo":
        return ctx.sweep_loo(**kw)
    return ctx.sweep_origins(**kw)


def assert_same(got, ref, what):
    """every output key to the bit; the sums in order of arrival to the project's bar for them"""
    assert set(got) == set(ref)
    for k, v in ref.items():
        if k in ATOMIC_SUMS:
            np.testing.assert_allclose(got[k], v, rtol=1e-12, atol=1e-300, err_msg="%s: %s" % (what, k))
        else:
            assert np.array_equal(got[k], v, equal_nan=v.dtype.kind == "f"), "%s: %s differs" % (what, k)


# ---------------------------------------------------------------------------------------------- the oracle, per mode
class CachedOracle:
    """the oracle of a fixture whose sweeps (alpha / beta store included) are made once and left unchanged: the Viterbi check
    and the sampling replay read the same store in every test of this module"""

    def __init__(self, ped):
        self.o, self.kept = oracle_ped(ped), {}

    def sweep_ind(self, ind, gen, **kw):
        key = (ind, gen) + tuple(sorted(kw.items()))
        if key not in self.kept:
            self.kept[key] = self.o.sweep_ind(ind, gen, **kw)
        return self.kept[key]


def stores(fx):
    return oracle(fx, "stores", lambda: CachedOracle(fx.ped))


def gaps(fx):
    return oracle(fx, "gaps", lambda: smp_suite.gap_transitions(fx.ped))


def replayed(fx, got):
    """smp_suite.replay of every individual of the fixture with skipped jobs, of every fourth of the others"""
    inds = list(range(fx.n)) if fx.skipped else list(range(0, fx.n, 4))
    checked = smp_suite.replay(fx.ped, got, SEED, inds=inds, o=stores(fx), Ts=gaps(fx))
    assert checked == len(inds) * fx.C - len([1 for j, _ in fx.skipped if j in inds])
    return len(inds), checked


def oracle(fx, kind, make):
    if kind not in fx.oracle:
        fx.oracle[kind] = make()
    return fx.oracle[kind]


def live_pairs(fx):
    return fx.n * fx.C - len(fx.skipped)


def marker_slice(fx, c):
    return slice(int(fx.ped.chromstarts[c]), int(fx.ped.chromstarts[c + 1]))


def check_oracle(capi, ctx, fx, mode, got, what, rows=False):
    """one call's outputs against the independent reference, with the helper and at the tolerance of the mode's own file:
    every individual and chromosome (sampling: every individual of the fixture with skipped jobs, every fourth of the
    others); rows: the mode's brute-force hook as well (cnf2_crossover_rows, cnf2_loo_rows, cnf2_origin_rows)"""
    ped = fx.ped
    what = "%s %s %s" % (fx.name, mode, what)
    if mode == "crossovers":
        want = oracle(fx, "xi", lambda: xo_suite.oracle_xi_all(ped))
        print(what, end=" ")
        xo_suite.check_against_oracle(ctx, ped, got=got, want=want, rows=rows)
    elif mode == "viterbi":
        print(what, end=" ")
        vit_suite.check_against_oracle(ctx, ped, got=got, o=stores(fx))
    elif mode == "sample":
        n_inds, checked = replayed(fx, got)
        print("%s: every pick of %d draws of %d individuals replayed, %d (individual, chromosome) pairs" % (what, got["state"].shape[1], n_inds, checked))
    elif mode == "place":
        E = oracle(fx, "emission", lambda: place_suite.oracle_emission(ped, *fx.cand))
        want, compared = oracle(fx, "place", lambda: place_suite.oracle_place(capi, ped, E))
        assert compared == live_pairs(fx)
        print(what, end=" ")
        place_suite.assert_place_close(got["place"], want, capi)
        active = got["factors"][:, 0, :] > -1e29
        mean = (E.sum(axis=3) / 64.0 * active[:, None, :]).sum(axis=2) / np.maximum(active.sum(axis=1), 1)[:, None]
        null = np.where(mean > 0, np.log(np.where(mean > 0, mean, 1.0)), 0.0).sum(axis=0)
        np.testing.assert_allclose(got["null"], null, rtol=1e-12)
    elif mode == "loo":
        want, _, compared = oracle(fx, "loo", lambda: oracle_loo(ped))
        assert compared == live_pairs(fx)
        loo_suite.close(got["loo"], want, what + " loo against the oracle")
        active = got["factors"][:, 0, :] > -1e29
        unl = oracle(fx, "unlinked", lambda: np.where(want == capi.IGNORED, capi.IGNORED, oracle_unlinked(ped, active)))
        loo_suite.close(got["unlinked"], unl, what + " unlinked against the oracle")
        if rows:
            for j in range(fx.n):
                for c in range(fx.C):
                    r, sl = ctx.loo_rows(j, c), marker_slice(fx, c)
                    assert np.abs(r[:, 0] - want[j, sl]).max() <= loo_suite.ATOL and np.abs(r[:, 1] - unl[j, sl]).max() <= loo_suite.ATOL
    else:
        want_o, want_b, _, compared = oracle(fx, "origins", lambda: oracle_origins(ped))
        assert compared == live_pairs(fx)
        org_suite.close(got["origin"], want_o, what + " origin against the oracle")
        org_suite.close(got["bits"], want_b, what + " bits against the oracle")
        live = np.ones((fx.n, ped.n_markers), bool)
        for j, c in fx.skipped:
            live[j, marker_slice(fx, c)] = False
        org_suite.check_identities(dict(origin=got["origin"][live][None], bits=got["bits"][live][None]))
        if rows:
            ro, rb = org_suite.all_origin_rows(ctx, ped)
            org_suite.close(ro, want_o, what + " cnf2_origin_rows origin against the oracle")
            org_suite.close(rb, want_b, what + " cnf2_origin_rows bits against the oracle")


def check_sentinels(capi, ctx, fx, mode, got):
    """a skipped job shows what include/cnf2hip.h documents for it, and is not counted"""
    for j, c in fx.skipped:
        sl = marker_slice(fx, c)
        if mode == "crossovers":
            assert np.all(got["xo"][j, sl] == 0.0)
        elif mode == "viterbi":
            assert np.all(got["state"][j, sl] == 0xFF) and got["shift"][j, c] == -1
            assert np.all(got["logmax"][j, c] == capi.IGNORED) and np.isnan(got["path_logpost"][j, c])
        elif mode == "sample":
            assert np.all(got["state"][j, :, sl] == 0xFF) and np.all(got["shift"][j, :, c] == -1)
        elif mode == "place":
            assert np.all(got["place"][j, :, sl] == capi.IGNORED)
        elif mode == "loo":
            assert np.all(got["loo"][j, sl] == capi.IGNORED) and np.all(got["unlinked"][j, sl] == capi.IGNORED)
        else:
            assert np.all(got["origin"][j, sl] == 0.0) and np.all(got["bits"][j, sl] == 0.0)
    if "n_contrib" in got:
        want = np.full(fx.C, fx.n, np.int32)
        for _, c in fx.skipped:
            want[c] -= 1
        assert np.array_equal(got["n_contrib"], want)
    if mode == "sample" and fx.skipped:
        # (Context.sweep_sample turns the logp of a skipped draw into NaN: the call's own value)
        K, M = 2, fx.ped.n_markers
        f, ll = np.zeros((fx.n, fx.C, 8)), np.zeros((fx.n, fx.C))
        st, sh, lp = np.zeros((fx.n, K, M), np.uint8), np.zeros((fx.n, K, fx.C), np.int32), np.zeros((fx.n, K, fx.C))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert ctx.L.cnf2_sweep_sample(ctx.h, 0, fx.n, K, SEED, p(f), p(ll), p(st), p(sh), p(lp), 0) == 0
        for j, c in fx.skipped:
            assert np.all(lp[j, :, c] == capi.IGNORED) and np.all(sh[j, :, c] == -1)
        assert np.array_equal(st, got["state"][:, :K]) and np.array_equal(sh, got["shift"][:, :K])


# ---------------------------------------------------------------------------------------------- a. one block = the full grid
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode", MODES)
def test_one_block_equals_the_full_grid(capi, mode, name):
    """jobs from the counter and strided jobs on one block against the unconstrained launch; the likelihoods are
    cnf2_sweep's to the bit in all three"""
    fx = fixture(name)
    ctx = open_ctx(capi, fx)
    try:
        check_fixture(ctx, fx)
        free = run(mode, ctx, fx)
        plain = ctx.sweep(dosage=False)
        ctx.set_grid_reserve(ONE_BLOCK)
        one = run(mode, ctx, fx)
        one_static = run(mode, ctx, fx, static_jobs=True)
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    assert_same(one, free, "%s %s: one block" % (name, mode))
    assert_same(one_static, free, "%s %s: one block, static jobs" % (name, mode))
    for r in (free, one, one_static):
        assert np.array_equal(r["factors"], plain["factors"], equal_nan=True)
        assert np.array_equal(r["loglik"], plain["loglik"], equal_nan=True)


# ---------------------------------------------------------------------------------------------- b. one block against the oracle
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode", MODES)
def test_one_block_against_the_oracle(capi, mode, name):
    """the one-block outputs themselves, jobs from the counter and strided jobs, against the independent reference; a skipped
    job's sentinels, and the job the same wave takes after it like any other"""
    fx = fixture(name)
    ctx = open_ctx(capi, fx)
    try:
        untied, tied = check_fixture(ctx, fx)
        print("%s: %d analysed individuals x %d chromosomes: %d untied + %d tied jobs on %d waves" % (name, fx.n, fx.C, len(untied), len(tied), WAVES))
        ctx.set_grid_reserve(ONE_BLOCK)
        for static in (False, True):
            got = run(mode, ctx, fx, static_jobs=static)
            check_oracle(capi, ctx, fx, mode, got, "one block, " + ("strided jobs" if static else "jobs from the counter"))
            check_sentinels(capi, ctx, fx, mode, got)
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()


# ---------------------------------------------------------------------------------------------- c. mode-specific edges
@pytest.mark.parametrize("name", FIXTURES)
def test_sampling_two_walks_then_the_next_job(capi, name):
    """65 draws are two backward walks per job (64 lanes), after which the wave takes its next job; draw k depends on (seed,
    individual, k) only, so the first draw of a 65-draw call is the 1-draw call's"""
    fx = fixture(name)
    ctx = open_ctx(capi, fx)
    try:
        free = {K: ctx.sweep_sample(draws=K, seed=SEED) for K in (65, 1)}
        ctx.set_grid_reserve(ONE_BLOCK)
        one = {K: ctx.sweep_sample(draws=K, seed=SEED) for K in (65, 1)}
        one_static = ctx.sweep_sample(draws=65, seed=SEED, static_jobs=True)
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    for K in (65, 1):
        assert_same(one[K], free[K], "%s: %d draws on one block" % (name, K))
    assert_same(one_static, free[65], "%s: 65 draws on one block, static jobs" % name)
    for k in ("state", "shift", "logp"):
        assert np.array_equal(one[65][k][:, :1], one[1][k], equal_nan=True), k
    # every pick of both walks against the oracle
    replayed(fx, one[65])


@pytest.mark.parametrize("name", FIXTURES)
def test_placement_in_batches_of_three_jobs_on_one_block(capi, name):
    """cnf2_set_batch_jobs(3): the posterior buffer's slots are reused batch after batch; uncapped, one batch holds every job
    and each wave of the block fills many slots"""
    fx = fixture(name)
    ctx = open_ctx(capi, fx)
    try:
        ctx.set_grid_reserve(ONE_BLOCK)
        ctx.set_batch_jobs(3)
        three = run("place", ctx, fx)
        ctx.set_batch_jobs(0)
        whole = run("place", ctx, fx)
        check_oracle(capi, ctx, fx, "place", three, "one block, batches of three jobs")
    finally:
        ctx.set_batch_jobs(0)
        ctx.set_grid_reserve(0)
        ctx.close()
    assert np.array_equal(fx.cand[0].shape[1:], (3, 2))
    assert_same(three, whole, "%s: batches of three jobs" % name)


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode", MODES)
def test_full_spill_between_half_spill_calls_on_one_block(capi, mode, name):
    """CNF2_FULL_SPILL lays the rows of a slot out differently and runs another instantiation: its outputs against the oracle,
    and the mode's brute-force hook (cnf2_crossover_rows, cnf2_loo_rows, cnf2_origin_rows) against the same oracle values; a
    half-spill call after it equals the half-spill call before it (every key to the bit but the sums that are added in
    order of arrival, which no two runs promise to the bit: those to the atomics' bar)"""
    fx = fixture(name)
    ctx = open_ctx(capi, fx)
    try:
        ctx.set_grid_reserve(ONE_BLOCK)
        first = run(mode, ctx, fx)
        full = run(mode, ctx, fx, full_spill=True)
        third = run(mode, ctx, fx)
        plain_full = ctx.sweep(dosage=False, full_spill=True)
        check_oracle(capi, ctx, fx, mode, full, "one block, full spill", rows=True)
        check_sentinels(capi, ctx, fx, mode, full)
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    assert_same(third, first, "%s %s: half spill after full spill" % (name, mode))
    assert np.array_equal(full["loglik"], plain_full["loglik"], equal_nan=True)
    assert np.array_equal(full["factors"], plain_full["factors"], equal_nan=True)


@pytest.mark.parametrize("mode", MODES)
def test_ties_general_on_one_block(capi, mode):
    """CNF2_TIES_GENERAL: the general kernel's job loop makes the tied windows' likelihoods, and (crossovers) its crossover
    instantiation their posteriors, on one block of 4 waves"""
    fx = fixture("tied_mixed")
    ctx = open_ctx(capi, fx)
    try:
        free = run(mode, ctx, fx, ties_general=True)
        plain = ctx.sweep(dosage=False, ties_general=True)
        ctx.set_grid_reserve(ONE_BLOCK)
        one = run(mode, ctx, fx, ties_general=True)
        one_static = run(mode, ctx, fx, ties_general=True, static_jobs=True)
        check_oracle(capi, ctx, fx, mode, one, "one block, CNF2_TIES_GENERAL")
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    assert_same(one, free, "%s: CNF2_TIES_GENERAL on one block" % mode)
    assert_same(one_static, free, "%s: CNF2_TIES_GENERAL on one block, static jobs" % mode)
    assert np.array_equal(one["loglik"], plain["loglik"]) and np.array_equal(one["factors"], plain["factors"])


@pytest.mark.parametrize("mode", MODES)
def test_sub_range_across_the_classes_on_one_block(capi, mode):
    """[b, e) from inside the uniform windows to inside the tied ones: the rows and counts of the whole call's slice, and with
    [0, b) and [e, n) the whole call's sums (to rounding, as the header says of a split) and counts"""
    fx = fixture("tied_mixed")
    ctx = open_ctx(capi, fx)
    try:
        untied, tied = check_fixture(ctx, fx)
        tied_inds = sorted(set(j for j, _ in tied))
        b, e = 1, tied_inds[len(tied_inds) // 2] + 1
        paths = ctx.sweep(log_paths=True, dosage=False)["paths"][:, 0]
        assert paths[b - 1] == PATH_UNIFORM and paths[b] == PATH_UNIFORM and paths[e - 1] == PATH_TIED and PATH_TIED in paths[e:]
        ctx.set_grid_reserve(ONE_BLOCK)
        whole = run(mode, ctx, fx)
        parts = [run(mode, ctx, fx, ind_begin=lo, ind_end=hi) for lo, hi in ((0, b), (b, e), (e, fx.n))]
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    for k in ("factors", "loglik") + ROWS[mode]:
        for (lo, hi), part in zip(((0, b), (b, e), (e, fx.n)), parts):
            assert np.array_equal(part[k], whole[k][lo:hi], equal_nan=whole[k].dtype.kind == "f"), "[%d, %d): %s differs" % (lo, hi, k)
    for k in COUNTS[mode]:
        assert np.array_equal(sum(part[k] for part in parts), whole[k]), k
    for k in SUMS[mode]:
        np.testing.assert_allclose(sum(part[k] for part in parts), whole[k], err_msg=k, **SPLIT_TOL[k])
