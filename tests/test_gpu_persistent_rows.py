"""GPU suite (-m gpu): the descent and the pair sweep through the persistent job loop.

tests/test_gpu_persistent_modes.py runs the six older analysis sweeps on ONE block of 4 waves; this file does the same, on
the same four fixtures and with the same helpers, for the two sweeps that came after it.

descent  cnf2_sweep_descent is the SW_DESCENT instantiation of fb_fast_kernel (tied windows: a follow-up launch on the second
         stream with a job counter of its own); its halving epilogue sits inside the marker loop of the persistent kernel, so
         whatever it leaves in registers, LDS or the spill slot meets the wave's next job.
pairs    cnf2_sweep_pairs runs the SW_ALPHA_BETA instantiation in batches (for_each_batch; the tied pass through launch_fb
         under CNF2_TIES_GENERAL) into slots of the batch buffer addressed by the job's index within the batch, and
         pair_sweep_kernel reads those slots, one wave per (job, first locus).  A slot is reused batch after batch: a skipped
         job's slot still holds the alpha and beta of the job that had it before.  Two selections per fixture, and a third
         that stands in for the first against the oracle:
         sel_all     every marker: the 64-marker chromosome of f2, outbred3 and f2_skipped has 63 first loci (16 blocks in y),
                     tied_mixed's longest chromosome 16
         sel_sparse  the first and the last marker of every chromosome of at least 2 markers, the marker of one single-marker
                     chromosome and nothing on another: chromosomes with one selected marker and with none, which
                     pair_sweep_kernel leaves at once.  tied_mixed has one single-marker chromosome only (lengths 1, 2, 8, 9,
                     17): there the chromosome left without a selected marker is the one of 2 markers.
         sel_thin    (f2, outbred3, f2_skipped) sel_all without every 2nd marker of the 64-marker chromosome: 31 first loci, 8
                     blocks in y.  The pair oracle takes a few thousand small matrix products per individual and mode for the
                     63 first loci of that chromosome, which made the tests that form it the only ones of this file to take
                     more than a second; so on these three fixtures the ORACLE is formed for sel_thin and sel_sparse, and the
                     sel_all rows are held at the same bar to cnf2_pair_rows, every pair of them.  Every comparison to the bit
                     is made on sel_all and sel_sparse (the capped batches on sel_thin as well).  tied_mixed's oracle is
                     formed for sel_all itself.
         check_selections asserts these properties against origins.linked_pairs.

References, all independent of the code under test: descent_reference.oracle_descent and pairs_reference.oracle_pairs (numpy
on the CPU oracle's store; computed once per fixture and selection, cached in the fixture and left unchanged; `compared` must
be live_pairs(fx), asserted on the reference alone before anything runs on the GPU), the brute-force hooks cnf2_descent_rows
and cnf2_pair_rows, descent_reference.check_identities against sweep_origins()["bits"] and pairs_reference.margins against
sweep_origins()["origin"].  The tolerance is the project's bar, ATOL = 1e-9 of tests/test_gpu_origins.py, through that file's
close.  "To the bit" is np.array_equal, for every key: both sweeps write their rows without atomics, n_contrib is counted by
one thread per chromosome and joint_sum is added in ascending order by origin_finish_kernel -- include/cnf2hip.h documents no
output of these two calls as added in order of arrival, so none is held to the atomics' bar.  Only a range split's joint_sum
adds up "to rounding": to the bar tests/test_gpu_pairs.py::test_bookkeeping sets for a split."""
import numpy as np
import pytest

from cnf2freq_amd import origins
from descent_reference import check_identities, oracle_descent
from pairs_reference import margins, oracle_pairs
from test_gpu_descent import all_descent_rows
from test_gpu_origins import ATOL, close, host_sums
from test_gpu_pairs import all_pair_rows, check_rows
from test_gpu_persistent_modes import (FIXTURES, MIXED_LENGTHS, ONE_BLOCK, PATH_TIED, PATH_UNIFORM, TIED_LENGTHS, WAVES,
                                       capi,  # noqa: F401  (the fixture: builds, and asserts a device)
                                       check_fixture, fixture, live_pairs, marker_slice, open_ctx, oracle)
from test_origins_host import oracle_origins

pytestmark = pytest.mark.gpu

MODES = ["descent", "pairs"]
MIXED = ("f2", "outbred3", "f2_skipped")         # the fixtures on MIXED_LENGTHS; tied_mixed is on TIED_LENGTHS
KEYS = dict(descent=("factors", "loglik", "descent", "n_contrib"), pairs=("factors", "loglik", "joint", "joint_sum", "n_contrib"))
ROWS = dict(descent="descent", pairs="joint")
SPLIT_TOL = dict(rtol=1e-12, atol=1e-12)         # joint_sum of a split range (tests/test_gpu_pairs.py::test_bookkeeping)
CAPS = (3, 13)                                   # cnf2_set_batch_jobs in test_pairs_in_capped_batches_on_one_block


# ---------------------------------------------------------------------------------------------- selections
def selections(fx):
    """{"sel_all": every marker, "sel_sparse": ends of the chromosomes of 2 and more markers, one marker on one further
    chromosome, none on another; on the fixtures with a 64-marker chromosome "sel_thin": sel_all without every 2nd marker of
    that chromosome} (int32, ascending)"""
    cs = np.asarray(fx.ped.chromstarts)
    lens = np.diff(cs)
    ones = [c for c in range(fx.C) if lens[c] == 1]
    single = ones[0]
    # none: a second single-marker chromosome; a fixture with one only leaves its shortest longer chromosome out
    none = ones[1] if len(ones) > 1 else min((c for c in range(fx.C) if lens[c] >= 2), key=lambda c: lens[c])
    sparse = [int(cs[single])]
    for c in range(fx.C):
        if lens[c] >= 2 and c != none:
            sparse += [int(cs[c]), int(cs[c + 1]) - 1]
    sels = dict(sel_all=np.arange(fx.ped.n_markers, dtype=np.int32), sel_sparse=np.array(sorted(sparse), np.int32))
    if fx.name in MIXED:
        long = int(np.argmax(lens))
        sels["sel_thin"] = np.array([m for m in range(fx.ped.n_markers) if not (cs[long] <= m < cs[long + 1] and (m - cs[long]) & 1)], np.int32)
    return sels


def check_selections(fx):
    """what the tests rely on in the two selections, against origins.linked_pairs; needs no GPU"""
    cs = np.asarray(fx.ped.chromstarts)
    lens = np.diff(cs)
    assert list(lens) == (MIXED_LENGTHS if fx.name in MIXED else TIED_LENGTHS)
    sels = selections(fx)
    per_chrom = lambda sel: np.bincount(np.searchsorted(cs, sel, side="right") - 1, minlength=fx.C)
    # sel_all: every pair of every chromosome; the longest chromosome's first loci fill 16 (tied_mixed: 4) blocks of 4 waves
    sel = sels["sel_all"]
    pairs = origins.linked_pairs(sel, cs)
    assert np.array_equal(per_chrom(sel), lens) and len(pairs) == sum(int(k) * (int(k) - 1) // 2 for k in lens)
    anchors = per_chrom(sel).max() - 1
    assert anchors == (63 if fx.name in MIXED else 16) and -(-anchors // WAVES) == (16 if fx.name in MIXED else 4)
    # sel_thin: the 64-marker chromosome keeps its markers 0, 2, .. 62: 31 first loci in 8 blocks; the others keep all
    if fx.name in MIXED:
        cnt = per_chrom(sels["sel_thin"])
        assert np.array_equal(cnt[:-1], lens[:-1]) and lens[-1] == 64 and cnt[-1] == 32 and -(-(cnt[-1] - 1) // WAVES) == 8
        assert set(sels["sel_thin"]) < set(sels["sel_all"]) and np.all(np.diff(sels["sel_thin"]) > 0)
    else:
        assert "sel_thin" not in sels
    # sel_sparse: one pair, (first, last), per chromosome with two selected markers; one chromosome with one, one with none
    sel = sels["sel_sparse"]
    cnt = per_chrom(sel)
    pairs = origins.linked_pairs(sel, cs)
    assert np.all(np.diff(sel) > 0) and set(cnt) == {0, 1, 2}
    assert (cnt == 1).sum() == 1 and (cnt == 0).sum() == 1 and len(pairs) == (cnt == 2).sum() >= 3
    two = np.flatnonzero(cnt == 2)
    assert np.array_equal(sel[pairs[:, 0]], cs[two]) and np.array_equal(sel[pairs[:, 1]], cs[two + 1] - 1)
    assert lens[cnt == 1][0] == 1, "the chromosome with one selected marker is a single-marker one"
    left_out = [c for c in range(fx.C) if lens[c] >= 2 and cnt[c] != 2]
    if fx.name in MIXED:
        assert not left_out and lens[cnt == 0][0] == 1, "first and last marker of every chromosome of at least 2 markers"
    else:
        assert left_out == [1] and cnt[1] == 0 and lens[1] == 2, "tied_mixed: the 2-marker chromosome has no selected marker"
    return sels


def has_oracle(fx, label):
    """whether the oracle is formed for this selection of the fixture (module docstring)"""
    return label != "sel_all" or fx.name not in MIXED


def cases(mode, fx, want="bits"):
    """[(label, sel)]: the calls of a mode on a fixture.  want: "bits" -- sel_all and sel_sparse; "oracle" -- the selections
    the oracle is formed for; "every" -- all of them"""
    if mode == "descent":
        return [("", None)]
    sels = check_selections(fx)
    order = [k for k in ("sel_all", "sel_thin", "sel_sparse") if k in sels]
    keep = dict(bits=lambda k: k != "sel_thin", oracle=lambda k: has_oracle(fx, k), every=lambda k: True)[want]
    return [(k, sels[k]) for k in order if keep(k)]


def run(mode, ctx, sel, **kw):
    return ctx.sweep_descent(**kw) if mode == "descent" else ctx.sweep_pairs(sel, **kw)


def pair_chroms(fx, sel, pairs):
    """the chromosome of every pair"""
    return np.searchsorted(np.asarray(fx.ped.chromstarts), sel[pairs[:, 0]], side="right") - 1


def live_rows(fx, mode, sel):
    """[n][M] (descent) or [n][n_pairs] (pairs): False on the rows of a skipped (individual, chromosome)"""
    if mode == "descent":
        live = np.ones((fx.n, fx.ped.n_markers), bool)
        for j, c in fx.skipped:
            live[j, marker_slice(fx, c)] = False
        return live
    pc = pair_chroms(fx, sel, origins.linked_pairs(sel, fx.ped.chromstarts))
    live = np.ones((fx.n, len(pc)), bool)
    for j, c in fx.skipped:
        live[j, pc == c] = False
    return live


# ---------------------------------------------------------------------------------------------- the references
def reference(fx, mode, label, sel):
    """the oracle's rows of a mode (and selection), made once per fixture; no (individual, chromosome) is left out"""
    if mode == "descent":
        ref = oracle(fx, "descent", lambda: oracle_descent(fx.ped))
        assert ref["compared"] == live_pairs(fx)
        return ref["descent"]
    kept = oracle(fx, "pair emissions", dict)         # the emission vectors do not depend on the selection
    joint, pairs, compared = oracle(fx, "pairs " + label, lambda: oracle_pairs(fx.ped, sel, emissions=kept))
    assert compared == live_pairs(fx)
    assert np.array_equal(pairs, origins.linked_pairs(sel, fx.ped.chromstarts))
    return joint


def check_reference_alone(fx, modes=MODES):
    """every condition the tests below set, on the references alone (no GPU): nothing left out, rows that sum to 1, exact
    zeros where skipped, the identities and the margins against oracle_origins at ATOL"""
    want_o, want_b, _, compared = oracle(fx, "origins", lambda: oracle_origins(fx.ped))
    assert compared == live_pairs(fx)
    if "descent" in modes:
        des = reference(fx, "descent", "", None)
        live = live_rows(fx, "descent", None)
        assert np.all(des[~live] == 0.0) and np.all(des[live].sum(axis=-1) > 0)
        check_identities(des, want_b)
    for label, sel in cases("pairs", fx, "oracle") if "pairs" in modes else ():
        joint = reference(fx, "pairs", label, sel)
        live = live_rows(fx, "pairs", sel)
        assert np.all(joint[~live] == 0.0)
        check_rows(joint[live][None])
        pairs = origins.linked_pairs(sel, fx.ped.chromstarts)
        first, second = margins(joint)
        close(first, want_o[:, sel[pairs[:, 0]]], "%s %s: the oracle's first margin against oracle_origins" % (fx.name, label))
        close(second, want_o[:, sel[pairs[:, 1]]], "%s %s: the oracle's second margin against oracle_origins" % (fx.name, label))


def check_oracle(ctx, fx, mode, label, sel, got, what, hook=False):
    """one call's rows against the oracle at ATOL; hook: the brute-force rows (cnf2_descent_rows, cnf2_pair_rows) against the
    same oracle values.  A selection the oracle is not formed for (has_oracle): the rows against cnf2_pair_rows at ATOL"""
    what = " ".join(w for w in (fx.name, mode, label, what) if w)
    if not has_oracle(fx, label):
        if hook:
            close(got["joint"], all_pair_rows(ctx, fx.ped, sel), what + " against cnf2_pair_rows")
        return
    want = reference(fx, mode, label, sel)
    close(got[ROWS[mode]], want, what + " against the oracle")
    if hook:
        rows = all_descent_rows(ctx, fx.ped) if mode == "descent" else all_pair_rows(ctx, fx.ped, sel)
        close(rows, want, what + (": cnf2_descent_rows" if mode == "descent" else ": cnf2_pair_rows") + " against the oracle")


def check_sentinels(ctx, fx, mode, sel, got, org):
    """a skipped job's rows are exactly 0.0 and it is not counted; every other row sums to 1; the sums are the rows added in
    ascending order; the identities with the origin sweep of the same context (org)"""
    rows, live = got[ROWS[mode]], live_rows(fx, mode, sel)
    assert (~live).any() == bool(fx.skipped)
    assert np.all(rows[~live] == 0.0), "rows of a skipped job"
    want = np.full(fx.C, fx.n, np.int32)
    for _, c in fx.skipped:
        want[c] -= 1
    assert np.array_equal(got["n_contrib"], want)
    if mode == "descent":
        assert np.all(rows[live].sum(axis=-1) > 0)
        check_identities(rows, org["bits"])
    else:
        check_rows(rows[live][None])
        assert np.array_equal(got["joint_sum"], host_sums(rows))
        pairs = origins.linked_pairs(sel, fx.ped.chromstarts)
        assert np.array_equal(ctx.linked_pairs(sel), pairs)
        first, second = margins(rows)
        close(first, org["origin"][:, sel[pairs[:, 0]]], fx.name + " first margin against sweep_origins")
        close(second, org["origin"][:, sel[pairs[:, 1]]], fx.name + " second margin against sweep_origins")


def assert_same(mode, got, ref, what):
    """every output key to the bit"""
    assert set(got) == set(ref) == set(KEYS[mode])
    for k in KEYS[mode]:
        assert np.array_equal(got[k], ref[k], equal_nan=ref[k].dtype.kind == "f"), "%s: %s differs" % (what, k)


def assert_likelihoods(r, plain):
    assert np.array_equal(r["factors"], plain["factors"], equal_nan=True)
    assert np.array_equal(r["loglik"], plain["loglik"], equal_nan=True)


# ---------------------------------------------------------------------------------------------- 1. one block = the full grid
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode", MODES)
def test_one_block_equals_the_full_grid(capi, mode, name):
    """jobs from the counter and strided jobs on one block against the unconstrained launch, every key to the bit; the
    likelihoods are cnf2_sweep's to the bit in all three"""
    fx = fixture(name)
    todo = cases(mode, fx)
    ctx = open_ctx(capi, fx)
    try:
        check_fixture(ctx, fx)
        free = [run(mode, ctx, sel) for _, sel in todo]
        plain = ctx.sweep(dosage=False)
        ctx.set_grid_reserve(ONE_BLOCK)
        one = [run(mode, ctx, sel) for _, sel in todo]
        one_static = [run(mode, ctx, sel, static_jobs=True) for _, sel in todo]
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    for (label, _), f, o, s in zip(todo, free, one, one_static):
        assert_same(mode, o, f, "%s %s %s: one block" % (name, mode, label))
        assert_same(mode, s, f, "%s %s %s: one block, static jobs" % (name, mode, label))
        for r in (f, o, s):
            assert_likelihoods(r, plain)


# ---------------------------------------------------------------------------------------------- 2. one block against the oracle
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode", MODES)
def test_one_block_against_the_oracle(capi, mode, name):
    """the one-block rows themselves, jobs from the counter and strided jobs, against the oracle (pairs: cnf2_pair_rows too;
    sel_all of the fixtures with a 64-marker chromosome: against cnf2_pair_rows, the oracle on sel_thin); a skipped job's
    zeros and count, the sums, the rows' totals and the identities with the origin sweep"""
    fx = fixture(name)
    todo = cases(mode, fx, "every")
    check_reference_alone(fx, (mode,))                # made, and held to live_pairs, before anything runs on the GPU
    ctx = open_ctx(capi, fx)
    try:
        untied, tied = check_fixture(ctx, fx)
        print("%s: %d analysed individuals x %d chromosomes: %d untied + %d tied jobs on %d waves" % (name, fx.n, fx.C, len(untied), len(tied), WAVES))
        ctx.set_grid_reserve(ONE_BLOCK)
        org = ctx.sweep_origins()
        for label, sel in todo:
            for static in (False, True):
                got = run(mode, ctx, sel, static_jobs=static)
                check_oracle(ctx, fx, mode, label, sel, got, "one block, " + ("strided jobs" if static else "jobs from the counter"),
                             hook=mode == "pairs" and (static or not has_oracle(fx, label)))
                check_sentinels(ctx, fx, mode, sel, got, org)
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()


# ---------------------------------------------------------------------------------------------- 3. full spill (descent)
@pytest.mark.parametrize("name", FIXTURES)
def test_descent_full_spill_between_half_spill_calls_on_one_block(capi, name):
    """CNF2_FULL_SPILL lays the rows of a slot out differently and runs another instantiation: its rows against the oracle,
    cnf2_descent_rows against the same oracle values, its likelihoods those of cnf2_sweep with the flag; the half-spill call
    after it equals the half-spill call before it to the bit"""
    fx = fixture(name)
    reference(fx, "descent", "", None)
    ctx = open_ctx(capi, fx)
    try:
        ctx.set_grid_reserve(ONE_BLOCK)
        first = ctx.sweep_descent()
        full = ctx.sweep_descent(full_spill=True)
        third = ctx.sweep_descent()
        plain_full = ctx.sweep(dosage=False, full_spill=True)
        check_oracle(ctx, fx, "descent", "", None, full, "one block, full spill", hook=True)
        check_sentinels(ctx, fx, "descent", None, full, ctx.sweep_origins())
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    assert_same("descent", third, first, name + ": half spill after full spill")
    assert_likelihoods(full, plain_full)


# ---------------------------------------------------------------------------------------------- 4. CNF2_TIES_GENERAL
@pytest.mark.parametrize("mode", MODES)
def test_ties_general_on_one_block(capi, mode):
    """CNF2_TIES_GENERAL: the general kernel's job loop makes the tied windows' likelihoods, and for the pair sweep (launch_fb
    with SW_ALPHA_BETA) their alpha and beta, with more than one job per wave only here"""
    fx = fixture("tied_mixed")
    todo = cases(mode, fx)
    for label, sel in todo:
        reference(fx, mode, label, sel)
    ctx = open_ctx(capi, fx)
    try:
        _, tied = check_fixture(ctx, fx)
        assert len(tied) >= 10 * WAVES
        free = [run(mode, ctx, sel, ties_general=True) for _, sel in todo]
        plain = ctx.sweep(dosage=False, ties_general=True)
        ctx.set_grid_reserve(ONE_BLOCK)
        one = [run(mode, ctx, sel, ties_general=True) for _, sel in todo]
        one_static = [run(mode, ctx, sel, ties_general=True, static_jobs=True) for _, sel in todo]
        org = ctx.sweep_origins(ties_general=True)
        for (label, sel), o in zip(todo, one):
            check_oracle(ctx, fx, mode, label, sel, o, "one block, CNF2_TIES_GENERAL")
            check_sentinels(ctx, fx, mode, sel, o, org)
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    for (label, _), f, o, s in zip(todo, free, one, one_static):
        assert_same(mode, o, f, "%s %s: CNF2_TIES_GENERAL on one block" % (mode, label))
        assert_same(mode, s, f, "%s %s: CNF2_TIES_GENERAL on one block, static jobs" % (mode, label))
        for r in (f, o, s):
            assert_likelihoods(r, plain)


# ---------------------------------------------------------------------------------------------- 5. capped batches (pairs)
def stale_slots(fx, jobs, cap):
    """[(k, skipped job, the job that had its slot in the batch before)] of one pass's jobs in batches of cap: slot k % cap
    of the batch buffer is job k - cap's before it is job k's.  Kept where that job is live and has at least as many markers,
    so that its alpha and beta lie under every marker the skipped job's waves would read"""
    lens = np.diff(np.asarray(fx.ped.chromstarts))
    out = []
    for k, job in enumerate(jobs):
        if job in fx.skipped and k >= cap and jobs[k - cap] not in fx.skipped and lens[jobs[k - cap][1]] >= lens[job[1]]:
            out.append((k, job, jobs[k - cap]))
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_pairs_in_capped_batches_on_one_block(capi, name):
    """cnf2_set_batch_jobs(3) and (13) against the uncapped call, every key to the bit, with jobs from the counter and strided
    jobs.  3 jobs on 4 waves never give a wave a second job in a launch but reuse every slot many times; 13 is neither a
    multiple of 4 nor below it: waves take 3 or 4 jobs a launch, and slots are reused across batches.  Under the cap of 13 the
    skipped jobs of f2_skipped (jobs 19 and 122 of the planner's order) take slots 6 and 5, which jobs 6 and 109 -- live, 64
    and 8 markers against 17 and 7 -- had in the batch before: asserted from job_lists' order, which check_fixture returns.  The capped rows against the oracle
    on f2_skipped (sel_thin and sel_sparse) and tied_mixed"""
    fx = fixture(name)
    against_oracle = name in ("f2_skipped", "tied_mixed")
    todo = cases("pairs", fx, "every" if against_oracle else "bits")
    if against_oracle:
        for label, sel in cases("pairs", fx, "oracle"):
            reference(fx, "pairs", label, sel)
    ctx = open_ctx(capi, fx)
    try:
        untied, tied = check_fixture(ctx, fx)
        assert len(untied) > 4 * max(CAPS) and [len(range(w, 13, WAVES)) for w in range(WAVES)] == [4, 3, 3, 3]
        if name == "f2_skipped":
            stale = stale_slots(fx, untied, 13)
            print("f2_skipped, batches of 13: (job, skipped, previous occupant of its slot):", stale)
            assert sorted(job for _, job, _ in stale) == sorted(fx.skipped)
        ctx.set_grid_reserve(ONE_BLOCK)
        org = ctx.sweep_origins() if against_oracle else None
        for label, sel in todo:
            for static in (False, True):
                ctx.set_batch_jobs(0)
                whole = ctx.sweep_pairs(sel, static_jobs=static)
                for cap in CAPS:
                    ctx.set_batch_jobs(cap)
                    got = ctx.sweep_pairs(sel, static_jobs=static)
                    what = "%s pairs %s: batches of %d jobs%s" % (name, label, cap, ", static jobs" if static else "")
                    assert_same("pairs", got, whole, what)
                    if against_oracle:
                        check_oracle(ctx, fx, "pairs", label, sel, got, "one block, batches of %d jobs%s" % (cap, ", strided jobs" if static else ""))
                        check_sentinels(ctx, fx, "pairs", sel, got, org)
    finally:
        ctx.set_batch_jobs(0)
        ctx.set_grid_reserve(0)
        ctx.close()


# ---------------------------------------------------------------------------------------------- 6. a sub-range
@pytest.mark.parametrize("mode", MODES)
def test_sub_range_across_the_classes_on_one_block(capi, mode):
    """[b, e) from inside the uniform windows to inside the tied ones: rows and likelihoods of the whole call's slice to the
    bit, and with [0, b) and [e, n) the whole call's counts exactly and joint_sum to rounding"""
    fx = fixture("tied_mixed")
    todo = cases(mode, fx)
    ctx = open_ctx(capi, fx)
    try:
        untied, tied = check_fixture(ctx, fx)
        tied_inds = sorted(set(j for j, _ in tied))
        b, e = 1, tied_inds[len(tied_inds) // 2] + 1
        paths = ctx.sweep(log_paths=True, dosage=False)["paths"][:, 0]
        assert paths[b - 1] == PATH_UNIFORM and paths[b] == PATH_UNIFORM and paths[e - 1] == PATH_TIED and PATH_TIED in paths[e:]
        ranges = ((0, b), (b, e), (e, fx.n))
        ctx.set_grid_reserve(ONE_BLOCK)
        whole = [run(mode, ctx, sel) for _, sel in todo]
        parts = [[run(mode, ctx, sel, ind_begin=lo, ind_end=hi) for lo, hi in ranges] for _, sel in todo]
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    for (label, _), w, ps in zip(todo, whole, parts):
        for k in ("factors", "loglik", ROWS[mode]):
            for (lo, hi), part in zip(ranges, ps):
                assert np.array_equal(part[k], w[k][lo:hi], equal_nan=True), "%s [%d, %d): %s differs" % (label, lo, hi, k)
        assert np.array_equal(sum(part["n_contrib"] for part in ps), w["n_contrib"])
        if mode == "pairs":
            np.testing.assert_allclose(sum(part["joint_sum"] for part in ps), w["joint_sum"], err_msg=label, **SPLIT_TOL)


# ---------------------------------------------------------------------------------------------- 7. what the consumers read
@pytest.mark.parametrize("mode", MODES)
def test_device_rows_on_one_block(capi, mode):
    """sweep_descent_device and sweep_pairs_device (every marker selected) into device tensors, what qtl_scan_hap / _vc and
    qtl_scan2_linked read in place: on one block the host-output call's, to the bit"""
    import torch
    fx = fixture("outbred3")
    n, M, C = fx.n, fx.ped.n_markers, fx.C
    sel = None if mode == "descent" else check_selections(fx)["sel_all"]
    dev = torch.device("cuda:0")
    new = lambda shape, dtype=torch.float64: torch.full(shape, 7, dtype=dtype, device=dev)
    ctx = open_ctx(capi, fx)
    try:
        ctx.set_grid_reserve(ONE_BLOCK)
        host = run(mode, ctx, sel)
        out = dict(factors=new((n, C, 8)), loglik=new((n, C)), n_contrib=new((C,), torch.int32))
        if mode == "descent":
            out["descent"] = new((n, M, 8))
            ctx.sweep_descent_device(0, n, out["factors"].data_ptr(), out["loglik"].data_ptr(), out["descent"].data_ptr(),
                                     out["n_contrib"].data_ptr())
        else:
            NP = len(origins.linked_pairs(sel, fx.ped.chromstarts))
            out["joint"], out["joint_sum"] = new((n, NP, 16)), new((NP, 16))
            ctx.sweep_pairs_device(0, n, sel, out["factors"].data_ptr(), out["loglik"].data_ptr(), out["joint"].data_ptr(),
                                   out["joint_sum"].data_ptr(), out["n_contrib"].data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
    finally:
        ctx.set_grid_reserve(0)
        ctx.close()
    assert_same(mode, got, host, "outbred3 %s: device rows on one block" % mode)
