"""What the QTL scans' invariance tests share (tests/test_qtl_invariance_host.py, tests/test_gpu_qtl_invariance.py): base cases
on a binary grid, transforms of traits and covariates that are exact in binary64, relabellings that do no arithmetic, and
the maps that carry a base reference over to the transformed problem.

With an intercept in X0 the model of include/cnf2hip.h does not depend on the units and offsets of the traits
(y -> alpha y + beta) nor on those of a covariate that is not interactive (z_k -> gamma_k z_k + delta_k): LOD, rank, n_used,
iterations, status and perm_max stay, the effects scale with alpha (an interaction with z_k with alpha / gamma_k), rss0 and
sigma2 with alpha^2.  The float64 yardsticks are themselves off by 1e-10 .. 1e-9 on a trait shifted by 2^17, so the reference
of a transformed problem is the yardstick on the base problem, carried over by map_reference.  The binary-trait scan has a
section of its own: covariate transforms, the complement of the trait, the same relabellings, map_bin_reference.

Three newer scans follow it, each with the same base cases, the same eight transforms and four relabellings, and a map of its
own.  The cofactor scan (cofactors 22 and 60 with +-3 markers left out; 7, 43 and 70 with +-2 under the largest shifts and the
reordering): map_cof_reference, compared by qtlcof_reference.compare_cof.  The bootstrap scan (21 replicates, a full replicate
tile and a partial one, all six chromosomes with the profile): the map is the identity, the counts go with their individuals
under the reordering, and reversing the replicates reverses every output to the bit; compared by qtlboot_reference.compare
on the cells of its conditions.  The polygenic scan (qtl.scan_lmm with h2 given and a chromosome left out of the kinship, and
with h2 estimated by REML): the reference is the Cholesky yardstick of the base problem at the given h2, or at the h2 the run
returned, carried over by map_lmm_reference; the estimated h2 itself is held to the base problem's likelihood grid, not to
another run (est_herit's golden section ends 1e-8 wide on a likelihood that is flat to rounding over 1e-7).  Last, what the
polygenic scan is made of: the kinship sums under the relabellings (check_kinship_relabellings) and the column scan, which
centres nothing and adds no intercept, under the scalings its model is invariant to (cols_problems)."""
import numpy as np

import qtl2_reference as R2
import qtlbin_reference as RB
import qtlboot_reference as RO
import qtlcof_reference as RC
import qtlem_reference as RE
import qtllmm_reference as RL
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


# ------------------------------------------------------------------------------------------------ the cofactor scan
# Composite interval mapping on the base cases: the cofactors' columns join the design, so the model stays invariant as the
# plain scan's is.  lod, lod_base, rank, rank_cof, n_used and perm_max stay, the marker's effects scale with alpha (a changes
# sign under swap03; the scan has no i, so swap12 changes nothing), rss0 with alpha^2; covariate transforms change nothing.
COF_SCANS = {"cof-full": dict(additive=False), "cof-add": dict(additive=True)}
COF = ((22, 60), 3)              # (cofactors, half-window in markers): chromosomes 4 and 6
COF3 = ((7, 43, 70), 2)          # none on chromosome 3, where n67-skip skips two individuals: n_used differs by chromosome

COF_FLOAT_KEYS = ("lod", "lod_base", "coef", "rss0", "perm_max")
COF_INT_KEYS = ("rank", "rank_cof", "n_used")


def cof_coef_names(scan):
    return ("a",) if COF_SCANS[scan]["additive"] else ("a", "d")


def cof_run(ctx, scan, inp, config=COF):
    """Context.qtl_scan_cof on the inputs `inp` with the cofactors and the half-window of `config`"""
    cof, hw = config
    return ctx.qtl_scan_cof(inp["origin"], inp["pheno"], cof, excl=RC.windows(cof, hw, CS), cov=inp["cov"], use=inp["use"],
                            perm=inp["perm"], additive=COF_SCANS[scan]["additive"])


def cof_reference(scan, inp, config=COF):
    """the cofactor scan's float64 yardstick on the inputs `inp`"""
    cof, hw = config
    lo, hi = RC.windows(cof, hw, CS)
    return RC.reference_scan_cof(inp["origin"], CS, inp["pheno"], cof, lo, hi, inp["use"], inp["cov"], inp["perm"],
                                 COF_SCANS[scan]["additive"])


_COF_REFS = {}


def cof_base_reference(case, scan, config=COF):
    """the yardstick of a cofactor scan on a base case, computed once and shared"""
    if (case, scan, config) not in _COF_REFS:
        _COF_REFS[case, scan, config] = cof_reference(scan, make_base(case), config)
    return _COF_REFS[case, scan, config]


def map_cof_reference(ref, alpha=1.0, flip=()):
    """The expected outputs of the transformed problem from a base reference of the cofactor scan (with 1 / alpha: the base
    form of a transformed problem's outputs): coef[T][M][ne] is multiplied by alpha per trait, and by -1 for a when "a" is in
    `flip`; rss0[T][C] by alpha^2; everything else stays."""
    out = dict(ref)
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (ref["rss0"].shape[0],))
    f = np.ones((len(alpha), 1, ref["coef"].shape[2])) * alpha[:, None, None]
    if "a" in flip:
        f[:, :, 0] *= -1.0
    out["coef"] = ref["coef"] * f
    out["rss0"] = ref["rss0"] * (alpha ** 2)[:, None]
    return out


def cof_as_got(ref):
    """a yardstick's dict in the form of the product's outputs"""
    return dict(ref, lod=ref["lod"][0], lod_base=ref["lod_base"][0], perm_max=ref["perm_max"] if ref["perm_max"].shape[0] else None)


def cof_errors(got, ref):
    return errors(got, ref, COF_FLOAT_KEYS, COF_INT_KEYS)


def cof_bit_equal(a, b):
    return bit_equal(a, b, COF_FLOAT_KEYS + COF_INT_KEYS)


# ------------------------------------------------------------------------------------------------ the bootstrap scan
# Every replicate is a scan of resampled individuals, and only LODs and the places of their maxima come out: the map is the
# identity under every transform and relabelling.  Under the reordering the counts go with their individuals.
BOOT_SCANS = {"boot-full": dict(additive=False), "boot-add": dict(additive=True)}
BOOT_B, BOOT_SEED = 21, 5        # one full replicate tile of 16 and a partial one

BOOT_KEYS = ("boot_max", "boot_arg", "n_boot", "boot_lod")

_BOOT_BASE = {}


def make_boot_base(case):
    """make_base(case) with count[B][n] = qtl.bootstrap_counts(n, 21, 5, use=use) added.  Computed once and shared."""
    if case not in _BOOT_BASE:
        base = make_base(case)
        _BOOT_BASE[case] = dict(base, count=qtl.bootstrap_counts(case[1], BOOT_B, BOOT_SEED, use=base["use"]))
    return _BOOT_BASE[case]


def boot_relabel(base, name):
    """relabel(base, name) of a base with counts: under `reorder` the counts are reordered too, count[:, s]"""
    inp, _ = relabel(base, name)
    count = base["count"][:, order_of(base["count"].shape[1])] if name == "reorder" else base["count"]
    return dict(inp, count=np.ascontiguousarray(count))


def boot_run(ctx, scan, inp):
    """Context.qtl_scan_boot on the inputs `inp`: all six chromosomes, with the profile"""
    return ctx.qtl_scan_boot(inp["origin"], inp["pheno"], inp["count"], cov=inp["cov"], use=inp["use"],
                             additive=BOOT_SCANS[scan]["additive"], profile=True)


def boot_reference(scan, inp):
    """the bootstrap scan's yardstick (literally resampled rows) on the inputs `inp`"""
    return RO.reference_boot(inp["origin"], CS, inp["pheno"], inp["count"], inp["use"], inp["cov"], BOOT_SCANS[scan]["additive"])


_BOOT_REFS = {}


def boot_base_reference(case, scan):
    """(the yardstick of a bootstrap scan on a base case, compared[B][T][C] of its conditions), computed once and shared; the
    conditions are asserted here, on the reference alone"""
    if (case, scan) not in _BOOT_REFS:
        ref = boot_reference(scan, make_boot_base(case))
        _BOOT_REFS[case, scan] = (ref, RO.conditions(ref, K, BOOT_SCANS[scan]["additive"], "%s %s" % (scan, case[0])))
    return _BOOT_REFS[case, scan]


def boot_as_got(ref):
    """a yardstick's dict in the form of the product's outputs"""
    return dict(boot_max=ref["boot_max"], boot_arg=ref["boot_arg"], n_boot=ref["n_boot"], boot_lod=ref["lod"])


def boot_errors(got, ref, compared=None):
    """figures for the log: ref a yardstick's dict or outputs of the product; boot_arg counted on the compared cells"""
    ref = boot_as_got(ref) if "lod" in ref else ref
    differ = got["boot_arg"] != ref["boot_arg"]
    return dict(boot_lod=float(np.abs(got["boot_lod"] - ref["boot_lod"]).max()), boot_max=float(np.abs(got["boot_max"] - ref["boot_max"]).max()),
                boot_arg=int(differ.sum() if compared is None else differ[compared].sum()), n_boot=int((got["n_boot"] != ref["n_boot"]).sum()))


def boot_bit_equal(a, b):
    return bit_equal(a, b, BOOT_KEYS)


# ------------------------------------------------------------------------------------------------ the polygenic scan
# qtl.scan_lmm centres traits and covariates itself (numpy) and hands rotated, whitened columns to cnf2_qtl_scan_cols, which
# centres nothing.  lod, rank, n_used and h2 stay, the effects scale with alpha (a changes sign under swap03; a_i a_j, hence
# the kinship, does not), sigma2 with alpha^2.  The reference is always the Cholesky yardstick on the BASE problem, mapped: at
# the given h2, or at the h2 the run under test returned.
LMM_SCANS = {"lmm-given": dict(loco=True, h2=(0.3, 0.8), permutations=3),
             "lmm-est": dict(loco=False, h2=None, permutations=0)}
LMM_SEED = 4
LMM_H2_BOUND = 1e-4              # the step of the grid of qtllmm_reference.grid_herit


def lmm_keep(inp):
    """the individuals scan_lmm analyses: used, and skipped on no chromosome"""
    o = inp["origin"]
    use = np.ones(o.shape[0], bool) if inp["use"] is None else inp["use"]
    return use & (o[:, CS[:-1]] != 0.0).any(axis=2).all(axis=1)


_LMM_KIN = {}


def lmm_base_kinship(case, loco):
    """K[C][n][n] by the yardstick on the base rows: without chromosome c, or the genome's repeated"""
    if (case, loco) not in _LMM_KIN:
        o = make_base(case)["origin"]
        C = len(CS) - 1
        _LMM_KIN[case, loco] = np.stack([RL.kinship_ref(o, CS, leave_out=c) for c in range(C)]) if loco else \
            np.repeat(RL.kinship_ref(o, CS)[None], C, axis=0)
    return _LMM_KIN[case, loco]


def lmm_run(ctx, scan, inp, rows, permutations=None, kinship=None):
    """qtl.scan_lmm on the inputs `inp` (ctx: a context that holds the map and n_ind; rows: the origin rows as a torch tensor on
    the device)"""
    s = LMM_SCANS[scan]
    return qtl.scan_lmm(ctx, inp["pheno"], kinship=kinship, loco=s["loco"], cov=inp["cov"], use=inp["use"],
                        permutations=s["permutations"] if permutations is None else permutations, seed=LMM_SEED, reml=True,
                        h2=s["h2"], rows=rows)


def lmm_given_h2(scan):
    """h2[T][C] of a scan whose h2 is given"""
    return np.repeat(np.asarray(LMM_SCANS[scan]["h2"], np.float64)[:, None], len(CS) - 1, axis=1)


def lmm_design(inp):
    """(keep, centred traits [nk][T], [1, centred covariates]) as the model has them"""
    keep = lmm_keep(inp)
    y = inp["pheno"][keep] - inp["pheno"][keep].mean(axis=0)
    z = inp["cov"][keep]
    return keep, y, np.concatenate([np.ones((keep.sum(), 1)), z - z.mean(axis=0)], axis=1)


def lmm_reference(inp, kin, h2):
    """The Cholesky yardstick (qtllmm_reference.reference_lmm) on the inputs `inp` with the kinships kin[C][n][n] at h2[T][C];
    added to its dict: h2, n_used[T] and sigma2[T][C] = RSS / (n - nx) of the whitened null model"""
    keep, y, X0 = lmm_design(inp)
    ref = RL.reference_lmm(inp["origin"], CS, inp["pheno"], inp["cov"], h2, lambda c: kin[c], keep=keep)
    sigma2 = np.zeros((y.shape[1], len(CS) - 1))
    for c in range(sigma2.shape[1]):
        for t in range(sigma2.shape[0]):
            (ys, xs), _ = RL.chol_whiten(kin[c][np.ix_(keep, keep)], h2[t][c], y[:, t], X0)
            r = ys - xs @ np.linalg.lstsq(xs, ys, rcond=None)[0]
            sigma2[t, c] = (r @ r) / (len(ys) - X0.shape[1])
    return dict(ref, h2=np.asarray(h2, np.float64), sigma2=sigma2, n_used=np.full(y.shape[1], keep.sum(), np.int32))


_LMM_REFS = {}


def lmm_base_reference(case, scan):
    """the yardstick of a polygenic scan with given h2 on a base case, computed once and shared"""
    if (case, scan) not in _LMM_REFS:
        _LMM_REFS[case, scan] = lmm_reference(make_base(case), lmm_base_kinship(case, LMM_SCANS[scan]["loco"]), lmm_given_h2(scan))
    return _LMM_REFS[case, scan]


_LMM_GRID = {}


def lmm_grid_h2(case, t):
    """the h2 at the maximum of the REML likelihood of trait t of a base case on the grid of step 1e-4, with the genome's
    kinship (Cholesky route; asserts a single local maximum).  Computed once per case and trait."""
    if (case, t) not in _LMM_GRID:
        keep, y, X0 = lmm_design(make_base(case))
        K0 = lmm_base_kinship(case, False)[0][np.ix_(keep, keep)]
        _LMM_GRID[case, t] = RL.grid_herit(K0, y[:, t], X0, reml=True)[0]
    return _LMM_GRID[case, t]


def map_lmm_reference(ref, alpha=1.0, flip=()):
    """The expected outputs of the transformed problem from a base reference of the polygenic scan (with 1 / alpha: the base
    form of a transformed problem's outputs): coef[T][M][2] is multiplied by alpha per trait, and by -1 for a when "a" is in
    `flip`; sigma2[T][C] by alpha^2; lod, rank, n_used and h2 stay."""
    out = dict(ref)
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (ref["coef"].shape[0],))
    f = np.ones((len(alpha), 1, 2)) * alpha[:, None, None]
    if "a" in flip:
        f[:, :, 0] *= -1.0
    out["coef"] = ref["coef"] * f
    out["sigma2"] = ref["sigma2"] * (alpha ** 2)[:, None]
    return out


def lmm_check(got, want, what):
    """qtllmm_reference.compare_lmm, unchanged, at ATOL with at least 0.9 of the cells compared; n_used equal; sigma2 within
    ATOL relative to max(1, |sigma2|)"""
    RL.compare_lmm(got, want, what, share=0.9)
    assert np.array_equal(got["n_used"], want["n_used"]), what + " n_used"
    err_s = (np.abs(got["sigma2"] - want["sigma2"]) / np.maximum(1.0, np.abs(want["sigma2"]))).max()
    print("%s: sigma2 %.3g" % (what, err_s))
    assert err_s <= ATOL, what + " sigma2"


LMM_FLOAT_KEYS = ("lod", "coef", "sigma2", "h2", "perm_max")
LMM_INT_KEYS = ("rank", "n_used")


def lmm_errors(got, ref):
    return errors(got, ref, LMM_FLOAT_KEYS, LMM_INT_KEYS)


def lmm_bit_equal(a, b):
    return bit_equal(a, b, LMM_FLOAT_KEYS + LMM_INT_KEYS)


# ------------------------------------------------------------------------------------------------ kinship sums, the column scan
KIN_RANGES = [(0, 6), (3, 4), (2, 5)]


def check_kinship_relabellings(sums, case, tag):
    """sums(origin, chrom_begin, chrom_end) -> (S[n][n], markers) on the base rows of a case, for every range of KIN_RANGES:
    under swap03 and swap12 the same bits (a_i a_j does not change); under reorder S' = S[s][:, s] within ATOL and S' equal
    to its transpose to the bit (whether the reordered matrix is also bit-equal is printed)"""
    base = make_base(case)
    s = order_of(case[1])
    for c0, c1 in KIN_RANGES:
        S, M = sums(base["origin"], c0, c1)
        want, Mw = RL.kinship_sums_ref(base["origin"], CS, c0, c1)
        assert M == Mw and (np.abs(S - want) / np.maximum(1.0, np.abs(want))).max() <= RL.ATOL
        for name in ("swap03", "swap12"):
            S2, M2 = sums(relabel(base, name)[0]["origin"], c0, c1)
            assert M2 == M and same_bits(S2, S), "%s: the sums change under %s" % (tag, name)
        S3, M3 = sums(relabel(base, "reorder")[0]["origin"], c0, c1)
        err = (np.abs(S3 - S[s][:, s]) / np.maximum(1.0, np.abs(S[s][:, s]))).max()
        print("INVARIANCE %s %s chromosomes %d..%d reorder: %.3g, bit-equal %s" % (tag, case[0], c0, c1, err, same_bits(S3, S[s][:, s])))
        assert M3 == M and err <= RL.ATOL
        assert same_bits(S3, S3.T), tag + ": the reordered sums are not symmetric to the bit"


COLS_CASE = (67, 2, 3, 2, 2, "soft", True)       # n, T, P, nx, ne, rows, scaled (qtllmm_reference.cols_case)

_COLS = []


def cols_base():
    """(inputs, reference) of the column scan's case, computed once and shared"""
    if not _COLS:
        reg, x0, pheno, scale, perm = RL.cols_case(*COLS_CASE)
        _COLS.append((dict(reg=reg, x0=x0, pheno=pheno, scale=scale, perm=perm), RL.cols_reference(reg, x0, pheno, scale, perm)))
    return _COLS[0]


def cols_problems():
    """[(name, inputs, alpha of the traits, divisor of coef)] of the column scan, whose model centres nothing and adds no
    intercept: the traits times 2^+-100; x0 @ diag(2^3, 2^-5); reg 2^7 with scale / 2^7; reg 2^7 alone (coef / 2^7); the
    individuals reordered, perm carried as relabel carries it.  Every factor is a power of two: the inputs stay exact."""
    inp, _ = cols_base()
    s = order_of(inp["reg"].shape[0])
    sinv = np.argsort(s)
    return [("pheno 2^100", dict(inp, pheno=inp["pheno"] * 2.0 ** 100), 2.0 ** 100, 1.0),
            ("pheno 2^-100", dict(inp, pheno=inp["pheno"] * 2.0 ** -100), 2.0 ** -100, 1.0),
            ("x0 diag(2^3, 2^-5)", dict(inp, x0=inp["x0"] * np.array([2.0 ** 3, 2.0 ** -5])), 1.0, 1.0),
            ("reg 2^7, scale 2^-7", dict(inp, reg=inp["reg"] * 2.0 ** 7, scale=inp["scale"] * 2.0 ** -7), 1.0, 1.0),
            ("reg 2^7", dict(inp, reg=inp["reg"] * 2.0 ** 7), 1.0, 2.0 ** 7),
            ("reorder", dict(reg=np.ascontiguousarray(inp["reg"][s]), x0=np.ascontiguousarray(inp["x0"][s]), pheno=inp["pheno"][s],
                             scale=inp["scale"][s], perm=sinv[inp["perm"][:, s]].astype(np.int32)), 1.0, 1.0)]


def map_cols(out, alpha=1.0, divisor=1.0):
    """outputs (or a reference) of the column scan with coef times alpha / divisor and rss0 times alpha^2"""
    return dict(out, coef=out["coef"] * (alpha / divisor), rss0=out["rss0"] * alpha ** 2)
