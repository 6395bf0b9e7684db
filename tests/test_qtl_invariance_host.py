"""CPU suite: the QTL scans on shifted and rescaled traits and covariates (tests/qtl_invariance.py).  The transforms are exact;
the maps that carry a base reference over to a transformed problem are proved on the yardsticks themselves, where those are
accurate (a small shift, pure scalings); the yardsticks' own error on the large shifts is printed, which is why the mapped
base reference is the reference; and the host library's pieces -- one fit of the maximum-likelihood scan
(cnf2h_qtlem_fit, the header the device compiles) and the residuals `cnF2freq --qtl*` permutes (cnf2h_qtl_null_residuals),
with qtl.null_residuals beside them -- are held to ATOL under every transform.

The binary-trait scan: its maps (covariate transforms change nothing; the complement and the relabellings change signs and
n_ones) are proved on the yardstick where that is accurate, the yardstick's own error under the large covariate transforms is
printed, and every cell through cnf2h_qtlbin_fit is held to the mapped base reference by qtlbin_reference.compare_bin.

The cofactor, bootstrap and polygenic scans: their maps are proved on their yardsticks (A, F, G and the four relabellings),
the conditions of each base reference are asserted, the yardsticks' own error on B, D and E is printed; no product scan runs.
The host counterparts of their kernels (qtlcof_marker, qtl_boot_marker, qtl_cols_marker) take sums or columns that their
callers have already centred, so units and offsets do not reach them and they are left out.  host.kinship_sums is checked
under the relabellings, and qtl.est_herit (numpy) against the base problem's likelihood grid under every transform."""
import numpy as np
import pytest

import qtl_invariance as V
import qtlbin_reference as RB
import qtlboot_reference as RO
import qtlcof_reference as RC
import qtlem_reference as RE
import qtllmm_reference as RL
from cnf2freq_amd import host, qtl
from qtl_reference import ATOL, reference_scan

TRANSFORM_IDS = sorted(V.TRANSFORMS)


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_transforms_are_exact(case):
    base = V.make_base(case)
    assert np.all(np.abs(np.nan_to_num(base["pheno"])) < 16) and np.all(np.nan_to_num(base["pheno"]) % V.GRID == 0)
    assert np.all(np.abs(np.nan_to_num(base["cov"])) < 16) and np.all(np.nan_to_num(base["cov"]) % V.GRID == 0)
    for name in TRANSFORM_IDS:
        for tr in (V.TRANSFORMS[name], V.interactive_variant(V.TRANSFORMS[name])):
            t = V.apply(base, tr)               # (asserts that the inverse returns the base bits)
            assert np.array_equal(np.isnan(t["pheno"]), np.isnan(base["pheno"]))
            changed = np.any(tr["alpha"] != 1) or np.any(tr["beta"] != 0) or np.any(tr["gamma"] != 1) or np.any(tr["delta"] != 0)
            assert changed and not (V.same_bits(t["pheno"], base["pheno"]) and V.same_bits(t["cov"], base["cov"]))
    s = V.order_of(case[1])
    assert np.array_equal(np.sort(s), np.arange(case[1])) and not np.array_equal(s, np.arange(case[1]))


# ------------------------------------------------------------------------------------------------ the mapping
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", list(V.SCANS))
def test_mapping_on_the_yardsticks(scan, case):
    """The yardstick on transforms A (a small shift), F and G (pure scalings) agrees with the mapped base reference within
    ATOL, by the scan's own comparison; for F and G also in the base problem's units, where that comparison is relative to
    figures of order 1.  This proves the formulas of map_reference; no product code runs.  (The interactive variant shifts
    the other covariate by 2^4 here, not 2^14: at 2^14 the yardstick's own effects are off by 1e-9 of their size, which the
    comparison of F, relative to effects of order 2^100, would count.)"""
    base, ref, names = V.make_base(case), V.base_reference(case, scan), V.coef_names(scan)
    if "near" in ref:
        assert ref["near"].mean() <= 0.01
    for name in ("A", "F", "G"):
        tr = V.transform_for(scan, V.TRANSFORMS[name], shift=2.0 ** 4)
        yard = V.as_got(scan, V.reference(scan, V.apply(base, tr)))
        want = V.map_reference(ref, tr["alpha"], tr["gamma"], names)
        what = "yardstick %s %s transform %s" % (scan, case[0], name)
        print(V.errors_line(what, V.errors(yard, want)))
        V.check(scan, yard, want, what)
        if name in "FG":
            V.check(scan, V.unmap(yard, tr, names), ref, what + " in base units")


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", ["scan", "scanx-int", "scan2", "em-fixed"])
def test_relabelling_maps_on_the_yardsticks(scan, case):
    """the relabellings do no arithmetic on the inputs: the yardstick on the relabelled problem agrees with the mapped base"""
    base, ref, names = V.make_base(case), V.base_reference(case, scan), V.coef_names(scan)
    for name in V.RELABELLINGS:
        if name == "covswap" and V.SCANS[scan].get("interactive"):
            continue
        inp, flip = V.relabel(base, name)
        what = "yardstick %s %s relabelling %s" % (scan, case[0], name)
        V.check(scan, V.as_got(scan, V.reference(scan, inp)), V.map_reference(ref, names=names, flip=flip), what)


# ------------------------------------------------------------------------------------------------ the yardsticks' own error
@pytest.mark.parametrize("scan", ["scan", "scanx", "scan2", "em-fixed"])
def test_yardstick_error_on_large_shifts(scan):
    """Printed, not asserted: how far the float64 yardsticks themselves are from the mapped base reference on B, D and E.  They
    are no reference there."""
    case = V.CASES[1]
    base, ref, names = V.make_base(case), V.base_reference(case, scan), V.coef_names(scan)
    for name in ("B", "D", "E"):
        tr = V.TRANSFORMS[name]
        yard = V.unmap(V.as_got(scan, V.reference(scan, V.apply(base, tr))), tr, names)
        err = V.errors(yard, ref)
        print(V.errors_line("yardstick's own error %s %s transform %s" % (scan, case[0], name), err))
        assert all(np.isfinite(v) for v in err.values())


# ------------------------------------------------------------------------------------------------ cnf2h_qtlem_fit
FIT_MARKERS = (3, 20, 70)        # on chromosomes 2, 3 (where the second case skips two individuals) and 5
FIT = dict(imprint=True, max_iter=300, tol=1e-7)


def fit_cells(case, inp):
    """host.qtlem_fit at FIT_MARKERS x traits on the inputs `inp`"""
    o = inp["origin"]
    use = np.ones(o.shape[0], bool) if inp["use"] is None else inp["use"]
    cells = {}
    for m in FIT_MARKERS:
        c = int(np.searchsorted(V.CS, m, side="right") - 1)
        mask = use & (o[:, V.CS[c]] != 0.0).any(axis=1)
        for t in range(V.T):
            cells[m, t] = host.qtlem_fit(o[:, m], np.where(mask, inp["pheno"][:, t], 0.0), np.where(mask[:, None], inp["cov"], 0.0),
                                         mask, **FIT)
    return cells


_FIT_BASE = {}


def fit_base(case):
    """(the product's fits on the base problem, near[m, t] of the yardstick on the three markers, each a chromosome of its own)"""
    if case not in _FIT_BASE:
        base = V.make_base(case)
        sub = np.ascontiguousarray(base["origin"][:, list(FIT_MARKERS)])
        ref = RE.reference_scan_em(sub, np.arange(len(FIT_MARKERS) + 1), base["pheno"], base["use"], base["cov"], True, None, False,
                                   FIT["max_iter"], FIT["tol"])
        assert ref["near"].mean() <= 0.01 and np.all(ref["rank"] == 3) and np.all(ref["status"] == 0)
        near = {(m, t): bool(ref["near"][t, j]) for j, m in enumerate(FIT_MARKERS) for t in range(V.T)}
        cells = fit_cells(case, base)
        for (m, t), f in cells.items():          # the base fits themselves are the yardstick's
            j = FIT_MARKERS.index(m)
            assert abs(f["lod"] - ref["lod"][0, t, j]) <= ATOL and f["rank"] == 3 and f["status"] == 0
            assert near[m, t] or f["iters"] == ref["iters"][t, j]
        _FIT_BASE[case] = (cells, near)
    return _FIT_BASE[case]


@pytest.mark.parametrize("name", TRANSFORM_IDS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_qtlem_fit(case, name):
    """one fit of the maximum-likelihood scan under a transform against the same fit of the base problem: lod within ATOL,
    coef and sigma2 in base units relative to max(1, |.|), rank, status and iterations equal"""
    tr = V.TRANSFORMS[name]
    want, near = fit_base(case)
    got = fit_cells(case, V.apply(V.make_base(case), tr))
    worst = dict(lod=0.0, coef=0.0, sigma2=0.0, rss0=0.0)
    for (m, t), g in got.items():
        w, a = want[m, t], tr["alpha"][t]
        worst["lod"] = max(worst["lod"], abs(g["lod"] - w["lod"]))
        worst["coef"] = max(worst["coef"], np.max(np.abs(g["coef"] / a - w["coef"]) / np.maximum(1.0, np.abs(w["coef"]))))
        worst["sigma2"] = max(worst["sigma2"], abs(g["sigma2"] / a ** 2 - w["sigma2"]) / max(1.0, abs(w["sigma2"])))
        worst["rss0"] = max(worst["rss0"], abs(g["rss0"] / a ** 2 - w["rss0"]) / max(1.0, abs(w["rss0"])))
    print(V.errors_line("host.qtlem_fit %s transform %s" % (case[0], name), worst))
    for (m, t), g in got.items():
        w = want[m, t]
        assert (g["rank"], g["status"], g["n_used"]) == (w["rank"], w["status"], w["n_used"]), (m, t)
        assert near[m, t] or g["iters"] == w["iters"], (m, t, g["iters"], w["iters"])
    assert worst["lod"] <= ATOL and worst["coef"] <= ATOL and worst["sigma2"] <= ATOL and worst["rss0"] <= ATOL


# ------------------------------------------------------------------------------------------------ the residuals that are permuted
LENS3 = V.CHROM_LENS[:3]         # the small permuted scan of the thresholds: the first 18 markers


def thresholds_text(case, res):
    """the 5-digit thresholds of a permuted Haley-Knott scan (the yardstick) of the residuals `res` on three chromosomes"""
    base = V.make_base(case)
    cs = V.chromstarts_of(LENS3)
    pm = reference_scan(base["origin"][:, :cs[-1]], cs, res, base["use"], base["cov"], base["perm"])["perm_max"]
    th = qtl.thresholds(pm, alpha=(0.5, 0.05))
    return ["%.5f" % v for v in np.concatenate([th["genome"].ravel(), th["chromosome"].ravel()])]


@pytest.mark.parametrize("name", TRANSFORM_IDS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_null_residuals(case, name):
    """cnf2h_qtl_null_residuals and qtl.null_residuals under a transform: res / alpha within ATOL of the base residuals, and
    the same printed thresholds from them"""
    tr = V.TRANSFORMS[name]
    base = V.make_base(case)
    use = np.ones(case[1], bool) if base["use"] is None else base["use"]
    zero = lambda inp: (np.where(use[:, None], inp["pheno"], 0.0), np.where(use[:, None], inp["cov"], 0.0), use)
    want = qtl.null_residuals(*zero(base))
    np.testing.assert_allclose(host.qtl_null_residuals(*zero(base)), want, rtol=0, atol=1e-12)
    want_text = thresholds_text(case, want)
    t = V.apply(base, tr)
    for what, f in (("host.qtl_null_residuals", host.qtl_null_residuals), ("qtl.null_residuals", qtl.null_residuals)):
        res = f(*zero(t)) / tr["alpha"]
        err = np.abs(res - want).max()
        print("%s %s transform %s: %.3g" % (what, case[0], name, err))
        assert np.all(res[~use] == 0.0)
        assert err <= ATOL, what
        assert thresholds_text(case, res) == want_text, what


# ------------------------------------------------------------------------------------------------ the binary-trait scan
BIN_TRANSFORM_IDS = sorted(V.BIN_TRANSFORMS)
BIN_SCAN_IDS = list(V.BIN_SCANS)


def bin_host_run(scan, inp):
    """cnf2h_qtlbin_fit at every (marker, column) of the inputs `inp`, in the form of Context.qtl_scan_binary's outputs"""
    from test_qtlbin_host import host_scan
    s = V.BIN_SCANS[scan]
    return host_scan(inp["origin"], inp["pheno"], inp["use"], inp["cov"], inp["perm"], s["imprint"], False, s["max_iter"], s["tol"])


def bin_changed(base, change):
    """(inputs, what map_bin_reference needs) of the complement or one of the relabellings"""
    if change == "complement":
        return V.complement(base), dict(complemented=True)
    inp, flip = V.relabel(base, change)
    return inp, dict(flip=flip)


BIN_CHANGES = ("complement",) + V.RELABELLINGS


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_bin_transforms_are_exact(case):
    base = V.make_bin_base(case)
    used = np.ones(case[1], bool) if base["use"] is None else base["use"]
    y = base["pheno"]
    assert np.all(np.isin(y[used], (0.0, 1.0))) and np.isnan(y[~used]).all() and V.same_bits(base["cov"], V.make_base(case)["cov"])
    for t in range(V.T):                         # both classes, so that the complement is a scan too
        assert 5 <= y[used, t].sum() <= used.sum() - 5
    for name in BIN_TRANSFORM_IDS + ["small"]:
        tr = V.BIN_SMALL_SHIFT if name == "small" else V.BIN_TRANSFORMS[name]
        assert np.all(tr["alpha"] == 1.0) and np.all(tr["beta"] == 0.0)
        t = V.apply(base, tr)                    # (asserts that the inverse returns the base bits)
        assert V.same_bits(t["pheno"], y) and not V.same_bits(t["cov"], base["cov"])
    c = V.complement(base)
    assert V.same_bits(1.0 - c["pheno"], y) and np.all(c["pheno"][used] + y[used] == 1.0)


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", BIN_SCAN_IDS)
def test_bin_mapping_on_the_yardstick(scan, case):
    """The yardstick on a small covariate shift (2^4), on the complement and on the four relabellings agrees with the mapped
    base reference by RB.compare_bin at ATOL.  This proves map_bin_reference; no product code runs."""
    V.assert_bin_conditions(case, scan)
    base, ref, names = V.make_bin_base(case), V.bin_base_reference(case, scan), V.bin_coef_names(scan)
    problems = [("shift 2^4", V.apply(base, V.BIN_SMALL_SHIFT), {})] + [(c,) + bin_changed(base, c) for c in BIN_CHANGES]
    for name, inp, how in problems:
        yard = V.as_got(scan, V.bin_reference(scan, inp))
        want = V.map_bin_reference(ref, names=names, **how)
        what = "yardstick %s %s %s" % (scan, case[0], name)
        print(V.errors_line(what, V.bin_errors(yard, want)))
        RB.compare_bin(yard, want, V.CS, what)
        if name == "complement":                 # the map is not the identity
            assert np.array_equal(yard["n_ones"] + ref["n_ones"], np.broadcast_to(ref["n_used"], ref["n_ones"].shape))
            assert np.nanmax(np.abs(yard["coef"] + ref["coef"])) <= ATOL and np.nanmax(np.abs(ref["coef"])) > 0.1


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", BIN_SCAN_IDS)
def test_bin_yardstick_error_on_covariate_transforms(scan, case):
    """Printed, not asserted: how far the float64 yardstick itself is from the mapped base reference under the covariate
    transforms.  It works on the covariates as given, so X'WX loses digits to a mean of 2^14 (effects off by up to 1e-7 of
    their size, by 6e-6 where a spread of 2^-20 sits on a mean of 2^-3) and its rank rule no longer scans anything at
    gamma = 2^+-100.  The yardstick is no reference there: the mapped base reference is."""
    base, ref, names = V.make_bin_base(case), V.bin_base_reference(case, scan), V.bin_coef_names(scan)
    for name in BIN_TRANSFORM_IDS:
        yard = V.as_got(scan, V.bin_reference(scan, V.apply(base, V.BIN_TRANSFORMS[name])))
        err = V.bin_errors(yard, V.map_bin_reference(ref, names=names))
        print(V.errors_line("yardstick's own error %s %s transform %s" % (scan, case[0], name), err))
        assert all(np.isfinite(v) for v in err.values())


_BIN_HOST_BASE = {}


def bin_host_base(case, scan):
    if (case, scan) not in _BIN_HOST_BASE:
        _BIN_HOST_BASE[case, scan] = bin_host_run(scan, V.make_bin_base(case))
    return _BIN_HOST_BASE[case, scan]


def bin_host_check(scan, case, name, inp, how):
    """cnf2h_qtlbin_fit on the inputs `inp` against the mapped base reference: RB.compare_bin, unchanged"""
    V.assert_bin_conditions(case, scan)          # on the reference alone, before the product runs
    ref, names = V.bin_base_reference(case, scan), V.bin_coef_names(scan)
    want = V.map_bin_reference(ref, names=names, **how)
    got = bin_host_run(scan, inp)
    what = "host %s %s %s" % (scan, case[0], name)
    print(V.errors_line("INVARIANCE " + what + " | against the mapped base reference:", V.bin_errors(got, want)))
    back = V.map_bin_reference(got, names=names, **how)          # (each of the maps is its own inverse)
    print(V.errors_line("INVARIANCE " + what + " | against the base run:", V.bin_errors(back, bin_host_base(case, scan))))
    RB.compare_bin(got, want, V.CS, what)
    s = V.BIN_SCANS[scan]
    if s["tol"] < 0:
        fitted = got["rank"] > 0
        assert np.all(got["iters"][:, fitted] == s["max_iter"]) and np.all(got["status"][:, fitted] == 1)
    return got


@pytest.mark.parametrize("name", BIN_TRANSFORM_IDS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", BIN_SCAN_IDS)
def test_bin_host_transform(scan, case, name):
    """every cell of the binary scan through cnf2h_qtlbin_fit on rescaled and shifted covariates: nothing changes"""
    got = bin_host_check(scan, case, "transform " + name, V.apply(V.make_bin_base(case), V.BIN_TRANSFORMS[name]), {})
    if name in "FG":
        print("INVARIANCE host %s %s transform %s | bit-equal to the base run: %s" %
              (scan, case[0], name, V.bin_bit_equal(got, bin_host_base(case, scan))))


@pytest.mark.parametrize("change", BIN_CHANGES)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", BIN_SCAN_IDS)
def test_bin_host_complement_and_relabelling(scan, case, change):
    """y -> 1 - y, classes 0 and 3 or 1 and 2 exchanged, the covariate columns exchanged, the individuals reordered"""
    inp, how = bin_changed(V.make_bin_base(case), change)
    bin_host_check(scan, case, change, inp, how)


# ------------------------------------------------------------------------------------------------ cofactor, bootstrap, polygenic
# The maps of the three newer scans, proved on their yardsticks.  No product scan runs here, and the host counterparts of their
# kernels (qtlcof_marker, qtl_boot_marker, qtl_cols_marker) take sums or columns that their callers have already centred: units
# and offsets do not reach them, so they are left out.  What does run on the host is host.kinship_sums, under the relabellings,
# and qtl.est_herit, which is numpy.
YARD_TRANSFORMS = ("A", "F", "G")
COF_SCAN_IDS = list(V.COF_SCANS)
BOOT_SCAN_IDS = list(V.BOOT_SCANS)


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", COF_SCAN_IDS)
def test_cof_mapping_on_the_yardstick(scan, case):
    """The cofactor scan's yardstick on A, F and G and on the four relabellings agrees with the mapped base reference by
    compare_cof at ATOL (share 0.99, strict: every marker of both cases is compared); for F and G also in base units.  The
    same for the three cofactors of COF3 under A and the reordering.  The conditions of the base references are asserted."""
    base = V.make_base(case)
    for config, names in ((V.COF, YARD_TRANSFORMS + V.RELABELLINGS), (V.COF3, ("A", "reorder"))):
        ref = V.cof_base_reference(case, scan, config)
        assert RC.compared_markers(ref, V.CS, share=0.99, strict=True).all() and RC.worst_pivot(ref, V.CS) >= 0.115
        kept = case[1] - 2
        on3 = [kept if case[3] or c == 3 else case[1] for c in range(len(V.CHROM_LENS))]
        assert list(ref["n_used"]) == ([kept] * len(V.CHROM_LENS) if config is V.COF else on3)
        for name in names:
            if name in V.TRANSFORMS:
                tr, flip = V.TRANSFORMS[name], ()
                inp = V.apply(base, tr)
            else:
                tr = V.IDENTITY
                inp, flip = V.relabel(base, name)
            yard = V.cof_as_got(V.cof_reference(scan, inp, config))
            want = V.map_cof_reference(ref, tr["alpha"], flip)
            what = "yardstick %s %s cofactors %s %s" % (scan, case[0], config[0], name)
            print(V.errors_line(what, V.cof_errors(yard, want)))
            RC.compare_cof(yard, want, V.CS, what, share=0.99, strict=True)
            if name in "FG":
                RC.compare_cof(V.map_cof_reference(yard, 1.0 / tr["alpha"]), ref, V.CS, what + " in base units", share=0.99, strict=True)
            if name == "swap03":                 # the map is not the identity
                assert np.nanmax(np.abs(yard["coef"][:, :, 0] + ref["coef"][:, :, 0])) <= ATOL and np.nanmax(np.abs(ref["coef"][:, :, 0])) > 0.1


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", BOOT_SCAN_IDS)
def test_boot_mapping_on_the_yardstick(scan, case):
    """The bootstrap scan's yardstick on A, F and G and on the four relabellings (the counts reordered with the individuals)
    agrees with the base reference -- the map is the identity -- by qtlboot_reference.compare at ATOL on the cells that
    conditions(base reference, K = 2) gives, which are asserted first."""
    base = V.make_boot_base(case)
    assert base["count"].shape == (V.BOOT_B, case[1]) and np.all(base["count"].sum(axis=1) == case[1] - 2 * case[3])
    ref, compared = V.boot_base_reference(case, scan)
    assert compared.all() and ref["gap"].min() >= 2e-4
    problems = [(name, V.apply(base, V.TRANSFORMS[name])) for name in YARD_TRANSFORMS] + [(name, V.boot_relabel(base, name)) for name in V.RELABELLINGS]
    for name, inp in problems:
        yard = V.boot_as_got(V.boot_reference(scan, inp))
        what = "yardstick %s %s %s" % (scan, case[0], name)
        print(V.errors_line(what, V.boot_errors(yard, ref, compared)))
        RO.compare(yard, ref, compared, what)
    s = V.order_of(case[1])
    re = V.boot_relabel(base, "reorder")
    assert np.array_equal(re["count"], base["count"][:, s]) and V.same_bits(re["pheno"], base["pheno"][s])


def lmm_yardstick(case, inp, kin):
    return V.lmm_reference(inp, kin, V.lmm_given_h2("lmm-given"))


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_lmm_mapping_on_the_yardstick(case):
    """The polygenic scan's Cholesky yardstick at h2 = (0.3, 0.8) with the kinship that leaves a chromosome out, on A, F and G
    and on the four relabellings (the kinship of the relabelled rows), agrees with the mapped base reference by compare_lmm at
    ATOL with at least 0.9 of the cells compared (all are), and in sigma2 and n_used; for F and G also in base units."""
    base = V.make_base(case)
    ref = V.lmm_base_reference(case, "lmm-given")
    assert ref["compared"].mean() >= 0.9 and list(ref["n_used"]) == [case[1] - 2] * V.T
    kin = V.lmm_base_kinship(case, True)
    for name in YARD_TRANSFORMS + V.RELABELLINGS:
        if name in V.TRANSFORMS:
            tr, flip = V.TRANSFORMS[name], ()
            inp, k = V.apply(base, tr), kin
        else:
            tr = V.IDENTITY
            inp, flip = V.relabel(base, name)
            k = np.stack([RL.kinship_ref(inp["origin"], V.CS, leave_out=c) for c in range(len(V.CHROM_LENS))])
        yard = lmm_yardstick(case, inp, k)
        what = "yardstick lmm-given %s %s" % (case[0], name)
        want = V.map_lmm_reference(ref, tr["alpha"], flip)
        print(V.errors_line(what, V.lmm_errors(yard, want)))
        V.lmm_check(yard, want, what)
        if name in "FG":
            V.lmm_check(V.map_lmm_reference(yard, 1.0 / tr["alpha"]), ref, what + " in base units")
        if name == "swap03":
            assert np.nanmax(np.abs(yard["coef"][:, :, 0] + ref["coef"][:, :, 0])) <= ATOL and np.nanmax(np.abs(ref["coef"][:, :, 0])) > 0.1


def test_new_yardsticks_error_on_large_shifts():
    """Printed, not asserted: how far the yardsticks of the cofactor, bootstrap and polygenic scans themselves are from the
    mapped base reference on B, D and E.  They are no reference there."""
    case = V.CASES[1]
    for name in ("B", "D", "E"):
        tr = V.TRANSFORMS[name]
        ref = V.cof_base_reference(case, "cof-full")
        yard = V.map_cof_reference(V.cof_as_got(V.cof_reference("cof-full", V.apply(V.make_base(case), tr))), 1.0 / tr["alpha"])
        err = V.cof_errors(yard, ref)
        print(V.errors_line("yardstick's own error cof-full %s transform %s" % (case[0], name), err))
        assert all(np.isfinite(v) for v in err.values())
        ref, compared = V.boot_base_reference(case, "boot-full")
        err = V.boot_errors(V.boot_as_got(V.boot_reference("boot-full", V.apply(V.make_boot_base(case), tr))), ref, compared)
        print(V.errors_line("yardstick's own error boot-full %s transform %s" % (case[0], name), err))
        assert all(np.isfinite(v) for v in err.values())
        ref = V.lmm_base_reference(case, "lmm-given")
        yard = V.map_lmm_reference(lmm_yardstick(case, V.apply(V.make_base(case), tr), V.lmm_base_kinship(case, True)), 1.0 / tr["alpha"])
        err = V.lmm_errors(yard, ref)
        print(V.errors_line("yardstick's own error lmm-given %s transform %s" % (case[0], name), err))
        assert all(np.isfinite(v) for v in err.values())


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_est_herit_under_transforms(case):
    """qtl.est_herit (numpy) on the eigenvectors of the base kinship, fed the centred traits and covariates of every
    transformed problem as qtl.scan_lmm centres them: h2 within 1e-4, the grid's step, of the maximum of the Cholesky-route
    REML likelihood of the BASE problem on the grid (which has a single local maximum); sigma2 in base units within ATOL,
    relative, of the yardstick's at the returned h2.  How far h2 moves from the base problem's estimate is printed: the
    likelihood is flat to rounding over the 1e-7 that the golden section's end leaves open."""
    keep, y0, X0 = V.lmm_design(V.make_base(case))
    K0 = V.lmm_base_kinship(case, False)[0][np.ix_(keep, keep)]
    lam, U = np.linalg.eigh(K0)
    fit = lambda inp: [qtl.est_herit(V.lmm_design(inp)[1][:, t], V.lmm_design(inp)[2], lam, U, reml=True) for t in range(V.T)]
    at_base = fit(V.make_base(case))
    for name in ["identity"] + TRANSFORM_IDS:
        tr = V.IDENTITY if name == "identity" else V.TRANSFORMS[name]
        for t, (h2, s2, _) in enumerate(fit(V.apply(V.make_base(case), tr))):
            grid = V.lmm_grid_h2(case, t)
            print("est_herit %s trait %d transform %s: h2 %.10f, the grid's maximum at %.4f, from the base estimate %.3g" %
                  (case[0], t, name, h2, grid, abs(h2 - at_base[t][0])))
            assert abs(h2 - grid) <= V.LMM_H2_BOUND
            (ys, xs), _ = RL.chol_whiten(K0, h2, y0[:, t], X0)
            r = ys - xs @ np.linalg.lstsq(xs, ys, rcond=None)[0]
            want = (r @ r) / (len(ys) - X0.shape[1])
            assert abs(s2 / tr["alpha"][t] ** 2 - want) <= ATOL * max(1.0, want)


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_host_kinship_sums_relabelled(case):
    """host.kinship_sums on the base rows over three chromosome ranges: the same bits with classes 0 and 3 or 1 and 2
    exchanged, the reordered matrix within ATOL under the reordering, and symmetric to the bit"""
    V.check_kinship_relabellings(lambda o, c0, c1: host.kinship_sums(o, V.CS, c0, c1), case, "host.kinship_sums")


def test_bin_nearly_collinear_marker_under_a_shift():
    """13 individuals of classes 1 .. 3 with up to 1e-3 of class 0: a + d is the intercept but for that leak, both effects are
    kept (relative pivot between QTL_PIVOT and 1e-3) and their estimates run to thousands.  Such a fit multiplies any change
    of the centred covariate by 1e7 and more: with the mean rounded to one double, age + 16384 moved the effects of 38 of
    these 40 draws, by up to 1.4.  The centred value is now rounded once from a mean carried in two doubles
    (qtl_column_mean2), so an exactly shifted covariate gives the same centred bits, and the fit the same bits."""
    from cnf2freq_amd import synth
    n, cells, differ, wild = 13, 0, 0, 0
    for seed in range(40):
        k = (synth.uniform(3 + seed, np.arange(n)) * 3).astype(int) + 1
        o = np.zeros((n, 4))
        o[np.arange(n), k] = 1.0
        leak = synth.uniform(400 + seed, np.arange(n)) * 1e-3
        o[:, 0] = leak
        o[np.arange(n), k] -= leak
        z = V.on_grid(synth.uniform(50 + seed, np.arange(n)) * 10.0)[:, None]
        y = RB.bernoulli(0.8 * (o[:, 3] - o[:, 0])[:, None], 2 + seed)[:, 0]
        assert np.array_equal((z + 16384.0) - 16384.0, z)
        f = host.qtlbin_fit(o, y, z, max_iter=30, tol=1e-6)
        g = host.qtlbin_fit(o, y, z + 16384.0, max_iter=30, tol=1e-6)
        if f["rank"] != 2 or f["ll0"] == 0.0:
            continue
        cells += 1
        wild += bool(np.abs(f["coef"]).max() > 100.0)
        same = f["lod"] == g["lod"] and V.same_bits(f["coef"], g["coef"]) and (f["iters"], f["status"]) == (g["iters"], g["status"])
        differ += not same
    print("nearly collinear markers: %d fits, %d with an effect beyond 100, %d change under age + 16384" % (cells, wild, differ))
    assert cells >= 30 and wild >= 20 and differ == 0
