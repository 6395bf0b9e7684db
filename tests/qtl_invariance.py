"""What the QTL scans' invariance tests share (tests/test_qtl_invariance_host.py, tests/test_gpu_qtl_invariance.py): base cases
on a binary grid, transforms of traits and covariates that are exact in binary64, relabellings that do no arithmetic, and
the maps that carry a base reference over to the transformed problem.

With an intercept in X0 the model of include/cnf2hip.h does not depend on the units and offsets of the traits
(y -> alpha y + beta) nor on those of a covariate that is not interactive (z_k -> gamma_k z_k + delta_k): LOD, rank, n_used,
iterations, status and perm_max stay, the effects scale with alpha (an interaction with z_k with alpha / gamma_k), rss0 and
sigma2 with alpha^2.  The float64 yardsticks are themselves off by 1e-10 .. 1e-9 on a trait shifted by 2^17, so the reference
of a transformed problem is the yardstick on the base problem, carried over by map_reference.  The binary-trait scan has a
section of its own at the end: covariate transforms, the complement of the trait, the same relabellings, map_bin_reference."""
import numpy as np

import qtl2_reference as R2
import qtlbin_reference as RB
import qtlem_reference as RE
import qtlx_reference as RX
from cnf2freq_amd import qtl
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, compare, noise, reference_scan, skip, soft_rows  # noqa: F401

CS = chromstarts_of(CHROM_LENS)
SEL = qtl.select_every(CS, 4)
GRID = 2.0 ** -16
K, T, P = 2, 2, 3

#         name        n  seed  mask   skipped
CASES = [("n41-mask", 41, 6, True, False),       # two unused individuals carrying NaN
         ("n67-skip", 67, 7, False, True)]       # individuals 1 and 4 skipped on chromosome 3
CASE_IDS = [c[0] for c in CASES]


def on_grid(x):
    """x rounded to multiples of 2^-16 (and -0.0 to 0.0); asserts |x| < 16"""
    r = np.round(np.asarray(x, np.float64) / GRID) * GRID + 0.0
    assert np.all(np.abs(r) < 16.0)
    return r


_BASE = {}


def make_base(case):
    """dict(origin, pheno, cov, use, perm) of one of CASES on the map CHROM_LENS: rows soft_rows(n, CHROM_LENS, seed), two
    covariates, two traits with Mendelian, imprinting and interaction effects of the true classes, every trait and covariate
    value on the grid; use is None without a mask.  Computed once and shared: nobody writes to it."""
    if case not in _BASE:
        _, n, seed, mask, skipped = case
        origin, k = soft_rows(n, CHROM_LENS, seed)
        M = origin.shape[1]
        if skipped:
            origin = skip(origin, [1, 4], 3, CHROM_LENS)
        use = np.ones(n, bool)
        if mask:
            use[[0, n // 2]] = False
        cov = on_grid(noise(n, K, seed + 1))
        a, d, im = RE.CODES["a"][k], RE.CODES["d"][k], RE.CODES["i"][k]
        at = [(7 * t + 3) % M for t in range(T)]
        to = [(11 * t + 40) % M for t in range(T)]
        pheno = on_grid(0.6 * a[:, at] + 0.3 * d[:, to] + 0.5 * im[:, to] + noise(n, T, seed + 2) + 0.3 * cov[:, :1] +
                        0.9 * a[:, at] * cov[:, :1])
        cov = np.where(use[:, None], cov, np.nan)
        pheno = np.where(use[:, None], pheno, np.nan)
        perm = qtl.permutations(n, P, seed, use=use)
        _BASE[case] = dict(origin=origin, pheno=pheno, cov=cov, use=use if mask else None, perm=perm)
    return _BASE[case]


# ------------------------------------------------------------------------------------------------ transforms
def transform(alpha=1.0, beta=0.0, gamma=1.0, delta=0.0):
    b = lambda v, w: np.broadcast_to(np.asarray(v, np.float64), (w,)).copy()
    return dict(alpha=b(alpha, T), beta=b(beta, T), gamma=b(gamma, K), delta=b(delta, K))


TRANSFORMS = dict(A=transform(beta=2.0 ** 10),
                  B=transform(beta=2.0 ** 17),
                  C=transform(delta=2.0 ** 14),
                  D=transform(alpha=2.0 ** 10, beta=2.0 ** 27, gamma=2.0 ** 3, delta=2.0 ** 14),
                  E=transform(alpha=2.0 ** -20, beta=2.0 ** -3, delta=2.0 ** 14),
                  F=transform(alpha=2.0 ** 100),
                  G=transform(alpha=2.0 ** -100),
                  H=transform(beta=(2.0 ** 9, 2.0 ** 15), delta=(2.0 ** 12, 2.0 ** 6)))
IDENTITY = transform()


def interactive_variant(tr, shift=2.0 ** 14):
    """the transform for the extended scan with interactive = 1: the traits as in `tr`, the interactive covariate z_0 only
    scaled (2^3 z_0), the other one shifted by `shift`.  A shift of an interactive covariate changes what the main effects mean
    and the raw columns the rank rule is relative to: that is the model, and not tested."""
    return dict(alpha=tr["alpha"], beta=tr["beta"], gamma=np.array([2.0 ** 3, 1.0]), delta=np.array([0.0, shift]))


def same_bits(a, b):
    """the same values bit for bit, NaN at the same places"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.nan_to_num(a).tobytes() == np.nan_to_num(b).tobytes()


def apply(base, tr):
    """the inputs of the transformed problem; asserts that the transform is exact: its inverse returns the base bits"""
    pheno = tr["alpha"] * base["pheno"] + tr["beta"]
    cov = tr["gamma"] * base["cov"] + tr["delta"]
    assert same_bits((pheno - tr["beta"]) / tr["alpha"], base["pheno"]), "the trait transform is not exact"
    assert same_bits((cov - tr["delta"]) / tr["gamma"], base["cov"]), "the covariate transform is not exact"
    return dict(base, pheno=pheno, cov=cov)


# ------------------------------------------------------------------------------------------------ relabellings
RELABELLINGS = ("swap03", "swap12", "covswap", "reorder")


def order_of(n):
    """the fixed permutation s of the reordering: new row j is old row s[j]"""
    return qtl.permutations(n, 1, 99)[0].astype(np.int64)


def relabel(base, name):
    """(inputs, flip): the relabelled problem and the effects whose sign it changes.  swap03: classes 0 and 3 of every origin
    row exchanged (a changes sign); swap12: classes 1 and 2 (i changes sign); covswap: the two covariate columns exchanged;
    reorder: the individuals in the order order_of(n), the permutations perm'[p][j] = s^-1[perm[p][s[j]]]."""
    if name == "swap03":
        return dict(base, origin=np.ascontiguousarray(base["origin"][:, :, [3, 1, 2, 0]])), ("a",)
    if name == "swap12":
        return dict(base, origin=np.ascontiguousarray(base["origin"][:, :, [0, 2, 1, 3]])), ("i",)
    if name == "covswap":
        return dict(base, cov=np.ascontiguousarray(base["cov"][:, ::-1])), ()
    assert name == "reorder"
    s = order_of(base["origin"].shape[0])
    sinv = np.argsort(s)
    perm = sinv[base["perm"][:, s]].astype(np.int32)
    return dict(origin=np.ascontiguousarray(base["origin"][s]), pheno=base["pheno"][s], cov=base["cov"][s],
                use=None if base["use"] is None else base["use"][s], perm=perm), ()


# ------------------------------------------------------------------------------------------------ the scans
#            name        what runs, and how
SCANS = {"scan": dict(kind="scan", additive=False),
         "scan-add": dict(kind="scan", additive=True),
         "scanx": dict(kind="scanx", imprint=True, interactive=0),
         "scanx-int": dict(kind="scanx", imprint=True, interactive=1),
         "scan2": dict(kind="scan2"),
         "em-fixed": dict(kind="em", imprint=True, tol=-1.0, max_iter=5),
         "em-stop": dict(kind="em", imprint=False, tol=1e-7, max_iter=300, perm=False)}    # (the stopping rule without permutations: the reference's cost)


def transform_for(scan, tr, shift=2.0 ** 14):
    return interactive_variant(tr, shift) if SCANS[scan].get("interactive") else tr


def perm_of(scan, inp):
    return inp["perm"] if SCANS[scan].get("perm", True) else None


def coef_names(scan):
    """the names of the scan's coef entries in their order, as qtl.coef_names gives them (the pair scan reports no effects)"""
    s = SCANS[scan]
    if s["kind"] == "scan":
        return ("a", "d")
    if s["kind"] == "scan2":
        return ()
    return qtl.coef_names(s.get("interactive", 0), s["imprint"], False)


def reference(scan, inp):
    """the scan's float64 yardstick on the inputs `inp`"""
    s = SCANS[scan]
    o, y, z, u, p = inp["origin"], inp["pheno"], inp["cov"], inp["use"], perm_of(scan, inp)
    if s["kind"] == "scan":
        return reference_scan(o, CS, y, u, z, p, s["additive"])
    if s["kind"] == "scanx":
        return RX.reference_scanx(o, CS, y, u, z, s["interactive"], s["imprint"], p, False)
    if s["kind"] == "scan2":
        return R2.reference_scan2(o, CS, SEL, y, u, z, p, False)
    return RE.reference_scan_em(o, CS, y, u, z, s["imprint"], p, False, s["max_iter"], s["tol"])


def run(ctx, scan, inp):
    """the product's scan on the inputs `inp` (ctx: a capi.Context that holds the map)"""
    s = SCANS[scan]
    o, y, kw = inp["origin"], inp["pheno"], dict(cov=inp["cov"], use=inp["use"], perm=perm_of(scan, inp))
    if s["kind"] == "scan":
        return ctx.qtl_scan(o, y, additive=s["additive"], **kw)
    if s["kind"] == "scanx":
        return ctx.qtl_scanx(o, y, interactive=s["interactive"], imprint=s["imprint"], **kw)
    if s["kind"] == "scan2":
        return ctx.qtl_scan2(o, SEL, y, **kw)
    return ctx.qtl_scan_em(o, y, imprint=s["imprint"], max_iter=s["max_iter"], tol=s["tol"], **kw)


def check(scan, got, ref, what):
    """the scan's own comparison (compare, comparex, compare2, compare_em), unchanged, with ATOL unchanged"""
    s = SCANS[scan]
    if s["kind"] == "scan":
        return compare(got, ref, CS, s["additive"], what)
    if s["kind"] == "scanx":
        return RX.comparex(got, ref, CS, what)
    if s["kind"] == "scan2":
        return R2.compare2(got, ref, what)
    return RE.compare_em(got, ref, CS, what)


def as_got(scan, ref):
    """a yardstick's dict in the form of the product's outputs (the observed block of the LODs), for the same comparison"""
    out = dict(ref)
    for key in ("lod", "lod_add", "lod_full"):
        if key in ref:
            out[key] = ref[key][0]
    if ref["perm_max"].shape[0] == 0:
        out["perm_max"] = None
    return out


_REFS = {}


def base_reference(case, scan):
    """the yardstick of a scan on a base case, computed once and shared"""
    if (case, scan) not in _REFS:
        _REFS[case, scan] = reference(scan, make_base(case))
    return _REFS[case, scan]


# ------------------------------------------------------------------------------------------------ the maps
def map_reference(ref, alpha=1.0, gamma=None, names=(), flip=()):
    """The expected outputs of the transformed problem from a base reference (or, with 1 / alpha and 1 / gamma, the base form
    of a transformed problem's outputs): lod, rank, n_used, iters, status, perm_max, relpivot and near stay; coef[T][M][len(names)]
    is multiplied by alpha, an interaction "e:zk" by alpha / gamma[k - 1], and by -1 for an effect in `flip`; rss0 and sigma2 by
    alpha^2.  alpha: a number or one per trait."""
    out = dict(ref)
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (ref["rss0"].shape[0],))
    if ref.get("coef") is not None and len(names):
        f = np.ones((len(alpha), 1, len(names))) * alpha[:, None, None]
        for j, name in enumerate(names):
            e, _, z = name.partition(":z")
            if z and gamma is not None:
                f[:, :, j] /= gamma[int(z) - 1]
            if e in flip:
                f[:, :, j] *= -1.0
        out["coef"] = ref["coef"] * f
    if ref.get("sigma2") is not None:
        out["sigma2"] = ref["sigma2"] * alpha[:, None] ** 2
    out["rss0"] = ref["rss0"] * (alpha ** 2).reshape((-1,) + (1,) * (ref["rss0"].ndim - 1))
    return out


def unmap(got, tr, names):
    """a transformed problem's outputs in the base problem's units"""
    return map_reference(got, 1.0 / tr["alpha"], 1.0 / tr["gamma"], names)


FLOAT_KEYS = ("lod", "lod_add", "lod_full", "coef", "sigma2", "rss0", "perm_max")
INT_KEYS = ("rank", "rank_add", "rank_full", "n_used", "iters", "status")


def errors(got, ref, float_keys=FLOAT_KEYS, int_keys=INT_KEYS):
    """Figures for the log, nothing asserted: per float output the largest |got - ref| / max(1, |ref|) over the cells where both
    are numbers (ref: a yardstick's dict, its LODs with the observed block first, or outputs of the product), and per
    integer output the number of cells that differ (iters: outside ref["near"])."""
    out = {}
    for key in float_keys:
        g, r = got.get(key), ref.get(key)
        if g is None or r is None or np.size(r) == 0:
            continue
        r = r[0] if key.startswith("lod") and r.ndim == g.ndim + 1 else r
        with np.errstate(invalid="ignore"):
            e = np.abs(g - r) / np.maximum(1.0, np.abs(r))
        out[key] = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
    for key in int_keys:
        if key in got and key in ref:
            differ = got[key] != ref[key]
            if key == "iters" and "near" in ref:
                differ = differ & ~ref["near"]
            out[key] = int(np.sum(differ))
    return out


def errors_line(tag, err):
    return tag + "  " + "  ".join("%s %.3g" % (k, v) if isinstance(v, float) else "%s_differ %d" % (k, v) for k, v in err.items())


def bit_equal(a, b, keys=FLOAT_KEYS + INT_KEYS):
    """every output of two runs of the product the same bits"""
    return all((a[k] is None and b[k] is None) or same_bits(a[k], b[k]) for k in keys if k in a)


# ------------------------------------------------------------------------------------------------ the binary-trait scan
# A 0/1 trait has no units: only the covariates are transformed (alpha = 1, beta = 0).  With an intercept in X0 the logistic
# model does not depend on z_k -> gamma_k z_k + delta_k at all (no output changes); under the complement y -> 1 - y of the
# used individuals theta changes sign, so lod, ll0, rank, n_used, iters, status and perm_max stay, every effect changes sign
# and n_ones -> n_used - n_ones; the relabellings change the sign of a (swap03) or of i (swap12) and nothing else.
BIN_TRANSFORMS = dict(C=transform(delta=2.0 ** 14),
                      D=transform(gamma=2.0 ** 3, delta=2.0 ** 14),
                      E=transform(gamma=2.0 ** -20, delta=2.0 ** -3),
                      F=transform(gamma=2.0 ** 100),
                      G=transform(gamma=2.0 ** -100),
                      H=transform(delta=(2.0 ** 12, 2.0 ** 6)))
BIN_SMALL_SHIFT = transform(delta=2.0 ** 4)      # a shift at which the float64 yardstick itself is still accurate

BIN_SCANS = {"bin-fixed": dict(imprint=True, tol=-1.0, max_iter=4),
             "bin-stop": dict(imprint=False, tol=1e-7, max_iter=50)}      # (both with the permutations)

# The strength of the planted effects (log odds per unit of a, d, i and of the first covariate), chosen on the yardstick alone
# so that each base reference passes the conditions of tests/qtlbin_reference.py (strict, compared >= 0.99, near <= 0.01).
# Tried, with the shares of compared cells of (n41 bin-fixed, n41 bin-stop, n67 bin-fixed, n67 bin-stop) and the largest share
# of near cells (41 individuals with two covariates and three effects come close to separation at a marker or two, which
# takes |eta| past ETA_MAX there):
#   (a, d, i, z) = (0.9, 0.5, -0.6, 1.0), tests/qtlbin_reference.make_case's:
#       draw seed + 2: 0.994, 1, 1, 1, near 0.006   seed + 3: 0.994, 1, 1, 1, near 0   seed + 4: 1, 1, 1, 1, near 0.006 (taken)
#   (0.6, 0.3, -0.4, 0.6):  seed + 2: 1, 1, 1, 1, near 0.006   seed + 3: 0.994, 0.994, 1, 1   seed + 4: 1, 1, 1, 1, near 0
#   (0.4, 0.2, -0.3, 0.4):  seed + 2: 1, 1, 1, 1   seed + 3: 0.988 (fails), 0.994, 1, 1   seed + 4: 1, 1, 1, 1
# Every reference was strict.  The taken one leaves the largest |eta| at 7.8 and the iterations of bin-stop at 2 .. 6.
BIN_EFFECT = dict(intercept=0.2, a=0.9, d=0.5, i=-0.6, z=1.0)
BIN_SEED = {"n41-mask": 4, "n67-skip": 4}        # added to the case's seed for the Bernoulli draws

BIN_FLOAT_KEYS = ("lod", "coef", "ll0", "perm_max")
BIN_INT_KEYS = ("rank", "n_used", "n_ones", "iters", "status")

_BIN_BASE = {}


def make_bin_base(case):
    """make_base(case) with 0/1 traits in place of the continuous ones: T columns drawn by RB.bernoulli from a logistic model of
    the true classes (a at one marker, d and i at another) plus the first covariate; NaN at the unused individuals.  Origin
    rows, covariates (on the grid), mask and permutations are make_base's own.  Computed once and shared."""
    if case not in _BIN_BASE:
        name, n, seed, mask, skipped = case
        base = make_base(case)
        _, k = soft_rows(n, CHROM_LENS, seed)
        M = k.shape[1]
        a, d, im = RE.CODES["a"][k], RE.CODES["d"][k], RE.CODES["i"][k]
        at = [(7 * t + 3) % M for t in range(T)]
        to = [(11 * t + 40) % M for t in range(T)]
        e = BIN_EFFECT
        eta = e["intercept"] + e["a"] * a[:, at] + e["d"] * d[:, to] + e["i"] * im[:, to] + e["z"] * np.nan_to_num(base["cov"][:, :1])
        used = np.ones(n, bool) if base["use"] is None else base["use"]
        pheno = np.where(used[:, None], RB.bernoulli(eta, seed + BIN_SEED[name]), np.nan)
        _BIN_BASE[case] = dict(base, pheno=pheno)
    return _BIN_BASE[case]


def complement(base):
    """the inputs with y -> 1 - y (NaN stays at the unused individuals)"""
    return dict(base, pheno=1.0 - base["pheno"])


def bin_coef_names(scan):
    return RB.effects(False, BIN_SCANS[scan]["imprint"])


def bin_reference(scan, inp):
    """the binary scan's float64 yardstick on the inputs `inp`"""
    s = BIN_SCANS[scan]
    return RB.reference_scan_binary(inp["origin"], CS, inp["pheno"], inp["use"], inp["cov"], s["imprint"], inp["perm"], False,
                                    s["max_iter"], s["tol"])


def bin_run(ctx, scan, inp):
    """Context.qtl_scan_binary on the inputs `inp`"""
    s = BIN_SCANS[scan]
    return ctx.qtl_scan_binary(inp["origin"], inp["pheno"], cov=inp["cov"], use=inp["use"], perm=inp["perm"], imprint=s["imprint"],
                               max_iter=s["max_iter"], tol=s["tol"])


_BIN_REFS = {}


def bin_base_reference(case, scan):
    """the yardstick of a binary scan on a base case, computed once and shared"""
    if (case, scan) not in _BIN_REFS:
        _BIN_REFS[case, scan] = bin_reference(scan, make_bin_base(case))
    return _BIN_REFS[case, scan]


def assert_bin_conditions(case, scan):
    """on the base reference alone: strict pivots, at least 0.99 of the cells compared, at most 0.01 near"""
    RB.assert_conditions([bin_base_reference(case, scan)])


def map_bin_reference(ref, names=(), flip=(), complemented=False):
    """The expected outputs of a changed problem from a base reference of the binary scan: under a covariate transform nothing
    changes; an effect in `flip` changes sign; under the complement every effect does and n_ones becomes n_used - n_ones.
    lod, ll0, rank, n_used, iters, status, perm_max, near, maxeta and relpivot stay."""
    out = dict(ref)
    f = np.ones(len(names))
    for j, name in enumerate(names):
        if name in flip:
            f[j] = -f[j]
    if complemented:
        f = -f
        out["n_ones"] = ref["n_used"][None, :] - ref["n_ones"]
    out["coef"] = ref["coef"] * f
    return out


def bin_errors(got, ref):
    return errors(got, ref, BIN_FLOAT_KEYS, BIN_INT_KEYS)


def bin_bit_equal(a, b):
    return bit_equal(a, b, BIN_FLOAT_KEYS + BIN_INT_KEYS)
