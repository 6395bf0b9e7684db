"""The yardstick of the maximum-likelihood scan's tests (tests/test_qtlem_host.py, tests/test_gpu_qtlem.py): the EM of
include/cnf2hip.h per marker and column by a route that shares nothing with the product's Schur form
(cnf2freq_amd/csrc/cnf2_qtlem.h).  The data are expanded to 4 n_c rows (the rows of individuals with c_i = 0 deleted), the
M-step is np.linalg.lstsq on the rows scaled by the square roots of their weights, and weights and likelihood are formed in
log space.  Which effects a marker keeps comes from qtlx_reference's sequential pivots: the residual of a column after
projection on every column before it."""
import numpy as np

from qtl_reference import ATOL, CHROM_LENS, PIVOT_DROP, PIVOT_EXACT, PIVOT_WELL, chromstarts_of, columns, noise, reference_scan, skip, soft_rows  # noqa: F401
from qtlx_reference import certain_rows, effects, reference_scanx  # noqa: F401

LN10 = np.log(10.0)
CODES = dict(a=np.array([-1.0, 0.0, 0.0, 1.0]), d=np.array([0.0, 1.0, 1.0, 0.0]), i=np.array([0.0, 1.0, -1.0, 0.0]))
NEAR_TOL = 1e-6          # a deciding gain within this relative distance of tol leaves the cell out of the comparison of iters


def loglik(lp, y, mu, s2):
    """sum_i log sum_g pi_ig phi(y_i; mu_ig, s2) in log space; lp = log pi (-inf for a class without weight).  Returns the
    value and the normalised log weights."""
    lw = lp - (y[:, None] - mu) ** 2 / (2.0 * s2)
    mx = lw.max(axis=1)
    with np.errstate(divide="ignore"):
        lse = mx + np.log(np.exp(lw - mx[:, None]).sum(axis=1))
    return float(lse.sum() - 0.5 * len(y) * np.log(2.0 * np.pi * s2)), lw - lse[:, None]


def em_cell(pi, y, X0, E, max_iter, tol):
    """One fit: pi[n][4], y[n], X0[n][nx], E[4][q] the codes of the kept effects.  A dict: ll0, ll (the trace l_0 .. l_t), beta,
    sigma2, iters, status, gains (of the last two iterations)."""
    n, nx = X0.shape
    q = E.shape[1]
    g0 = np.linalg.lstsq(X0, y, rcond=None)[0]
    rss0 = float(((y - X0 @ g0) ** 2).sum())
    ll0 = -0.5 * n * (np.log(2.0 * np.pi * rss0 / n) + 1.0)
    with np.errstate(divide="ignore"):
        lp = np.log(pi)
    theta, s2 = np.concatenate([g0, np.zeros(q)]), rss0 / n
    Xe = np.concatenate([np.repeat(X0, 4, axis=0), np.tile(E, (n, 1))], axis=1)        # row 4 i + g
    ye = np.repeat(y, 4)
    trace, gains, status, t = [ll0], [], 1, 0
    while t < max_iter:
        mu = (Xe @ theta).reshape(n, 4)
        _, lw = loglik(lp, y, mu, s2)
        sw = np.exp(0.5 * lw).reshape(-1)
        new, _, rk, _ = np.linalg.lstsq(Xe * sw[:, None], ye * sw, rcond=None)
        s2_new = float(((sw * (ye - Xe @ new)) ** 2).sum()) / n
        if rk < nx + q or not (s2_new > 0.0 and np.isfinite(s2_new)):
            status = 2
            break
        theta, s2, t = new, s2_new, t + 1
        ll, _ = loglik(lp, y, (Xe @ theta).reshape(n, 4), s2)
        gains.append((ll - trace[-1]) / LN10)
        trace.append(ll)
        if gains[-1] < tol:
            status = 0
            break
    return dict(ll0=ll0, ll=np.array(trace), beta=theta[nx:], sigma2=s2, iters=t, status=status, gains=gains[-2:], rss0=rss0)


def reference_scan_em(origin, chromstarts, pheno, use=None, cov=None, imprint=False, perm=None, additive=False, max_iter=1000,
                      tol=1e-6):
    """The model of include/cnf2hip.h.  A dict: lod[1 + P][T][M] (block 0 observed), trace[T][M][max_iter + 1] of the observed
    columns' LODs after every iteration (the last value repeated), coef[T][M][ne], sigma2[T][M], iters[T][M], status[T][M],
    near[T][M] (a deciding gain lies within NEAR_TOL of tol), rank[M], relpivot[M][ne], usable[C], n_used[C], rss0[T][C],
    perm_max[P][T][C]."""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    cs = np.asarray(chromstarts, np.int64)
    C = len(cs) - 1
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    Z = np.zeros((n, 0)) if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    K = Z.shape[1]
    X0all = np.concatenate([np.ones((n, 1)), Z], axis=1)
    eff = effects(additive, imprint)
    ne = len(eff)
    hk = reference_scanx(o, cs, np.where(use[:, None], np.nan_to_num(np.asarray(pheno, np.float64).reshape(n, -1)), 0.0)[:, :1],
                         use, cov, 0, imprint, None, additive)
    Y = columns(np.where(use[:, None], np.asarray(pheno, np.float64).reshape(n, -1), 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    lod = np.zeros((Q, T, M))
    trace = np.zeros((T, M, max_iter + 1))
    coef = np.full((T, M, ne), np.nan)
    sigma2 = np.full((T, M), np.nan)
    iters, status, near = np.zeros((T, M), np.int32), np.zeros((T, M), np.int32), np.zeros((T, M), bool)
    rank = np.zeros(M, np.int32)
    usable = np.zeros(C, bool)
    n_used = hk["n_used"].copy()
    rss0_out = np.zeros((T, C))
    for c in range(C):
        keep = use & (o[:, cs[c]] != 0.0).any(axis=1)
        n_c = int(keep.sum())
        X0 = X0all[keep]
        # (K + 4: RSS0 is cnf2_qtl_scan's, which needs that many whatever the flags)
        usable[c] = hk["usable"][c] and n_c >= K + 4
        if not usable[c]:
            continue
        for m in range(cs[c], cs[c + 1]):
            rp = hk["relpivot"][m]
            kept = np.nan_to_num(rp, nan=0.0) >= PIVOT_DROP
            rank[m] = int(kept.sum())
            assert rank[m] == hk["rank"][m][1]
            pi = o[keep, m] / o[keep, m].sum(axis=1, keepdims=True)
            E = np.stack([CODES[e] for e, k in zip(eff, kept) if k], axis=1) if kept.any() else np.zeros((4, 0))
            for qq in range(Q):
                for t in range(T):
                    y = Y[keep, qq, t]
                    r0 = y - X0 @ np.linalg.lstsq(X0, y, rcond=None)[0]
                    rss0 = float((r0 ** 2).sum())
                    if qq == 0:
                        rss0_out[t, c] = rss0
                    if not rss0 > 0.0:
                        continue
                    if qq == 0:
                        sigma2[t, m] = rss0 / n_c
                    if rank[m] == 0:
                        continue
                    f = em_cell(pi, y, X0, E, max_iter, tol)
                    lod[qq, t, m] = max(0.0, (f["ll"][-1] - f["ll0"]) / LN10)
                    if qq == 0:
                        tr = np.maximum(0.0, (f["ll"] - f["ll0"]) / LN10)
                        trace[t, m, :len(tr)] = tr
                        trace[t, m, len(tr):] = tr[-1]
                        coef[t, m, kept] = f["beta"]
                        sigma2[t, m], iters[t, m], status[t, m] = f["sigma2"], f["iters"], f["status"]
                        near[t, m] = any(abs(g - tol) <= NEAR_TOL * abs(tol) for g in f["gains"])
    perm_max = np.zeros((Q - 1, T, C))
    for c in range(C):
        perm_max[:, :, c] = lod[1:, :, cs[c]:cs[c + 1]].max(axis=2)
    return dict(lod=lod, trace=trace, coef=coef, sigma2=sigma2, iters=iters, status=status, near=near, rank=rank,
                relpivot=hk["relpivot"], usable=usable, n_used=n_used, rss0=rss0_out, perm_max=perm_max)


def compared_markers(ref, chromstarts, share=0.99, strict=True):
    """compared[M]: the markers of scanned chromosomes whose every effect is either well conditioned (relative pivot at least
    PIVOT_WELL) or exactly degenerate (at most PIVOT_EXACT, or a raw diagonal of 0).  Asserts on the reference alone what the
    comparison rests on: every marker of a scanned chromosome is of that kind (strict), and at least `share` of all markers
    are compared."""
    cs = np.asarray(chromstarts, np.int64)
    rp = ref["relpivot"]
    fine = np.all(np.isnan(rp) | (rp >= PIVOT_WELL) | (rp <= PIVOT_EXACT), axis=1)
    on = np.repeat(ref["usable"], np.diff(cs))
    assert not strict or np.all(fine[on]), "a marker is neither well conditioned nor exactly degenerate: relative pivots %s" % rp[on & ~fine]
    compared = fine | ~on
    if share:
        assert compared.mean() >= share, "only %.0f %% of the markers are compared" % (100 * compared.mean())
    return compared


def compare_em(got, ref, chromstarts, what="", share=0.99, strict=True, iters=True):
    """every output of a scan against the reference at the compared markers: lod, sigma2 (relative to max(1, .)), coef (relative
    to max(1, |coef|), NaN exactly where the reference drops an effect), perm_max within ATOL; rank, n_used, status and (with
    `iters`: except where ref["near"]) iters with ==.  Prints every figure before it asserts; returns the errors."""
    cm = compared_markers(ref, chromstarts, share, strict)
    err_l = np.abs(got["lod"][:, cm] - ref["lod"][0][:, cm]).max()
    gs, rs = got["sigma2"][:, cm], ref["sigma2"][:, cm]
    assert np.array_equal(np.isnan(gs), np.isnan(rs)), what + ": sigma2 is NaN exactly where nothing is fitted"
    both = ~np.isnan(rs)
    err_s = (np.abs(gs[both] - rs[both]) / np.maximum(1.0, np.abs(rs[both]))).max() if both.any() else 0.0
    gc, rc = got["coef"][:, cm], ref["coef"][:, cm]
    assert np.array_equal(np.isnan(gc), np.isnan(rc)), what + ": a dropped effect is NaN, a kept one a number"
    both = ~np.isnan(rc)
    err_c = (np.abs(gc[both] - rc[both]) / np.maximum(1.0, np.abs(rc[both]))).max() if both.any() else 0.0
    err_r = np.abs(got["rss0"] - ref["rss0"]).max()
    print("%s: lod %.3g over %d cells, sigma2 %.3g, coef %.3g over %d of %d markers, rss0 %.3g, iterations up to %d" %
          (what, err_l, got["lod"][:, cm].size, err_s, err_c, cm.sum(), len(cm), err_r, ref["iters"].max()))
    assert np.array_equal(got["rank"][cm], ref["rank"][cm]), what + " rank"
    assert np.array_equal(got["n_used"], ref["n_used"]), what + " n_used"
    assert err_l <= ATOL, what + " lod"
    assert err_s <= ATOL, what + " sigma2"
    assert err_c <= ATOL, what + " coef"
    assert err_r <= ATOL * max(1.0, np.abs(ref["rss0"]).max()), what + " rss0"
    assert np.isfinite(got["lod"]).all() and np.all(got["lod"] >= 0), what + " lod is finite and not negative"
    off = ~np.repeat(ref["usable"], np.diff(np.asarray(chromstarts, np.int64)))
    assert np.all(got["lod"][:, off] == 0.0) and np.isnan(got["coef"][:, off]).all() and np.all(got["rank"][off] == 0)
    zero = got["rank"] == 0
    assert np.all(got["lod"][:, zero] == 0.0) and np.all(got["iters"][:, zero] == 0) and np.all(got["status"][:, zero] == 0)
    assert np.array_equal(got["status"][:, cm], ref["status"][:, cm]), what + " status"
    if iters:
        ok = ~ref["near"][:, cm]
        assert np.array_equal(got["iters"][:, cm][ok], ref["iters"][:, cm][ok]), what + " iters"
    err_p = 0.0
    if ref["perm_max"].shape[0]:
        err_p = np.abs(got["perm_max"] - ref["perm_max"]).max()
        print("%s: perm_max %.3g over %d cells" % (what, err_p, ref["perm_max"].size))
        assert err_p <= ATOL, what + " perm_max"
    else:
        assert got.get("perm_max") is None
    return dict(lod=err_l, sigma2=err_s, coef=err_c, rss0=err_r, perm_max=err_p)


# ------------------------------------------------------------------------------------------------ the cases of the issue
# fixed iterations (tol = -1)
#         n    K  imprint additive seed T  P  mask   skipped max_iter
CASES = [(24, 0, False, False, 3, 1, 5, False, False, 1),
         (17, 1, True, False, 4, 3, 1, False, False, 2),
         (41, 2, False, True, 6, 3, 0, False, False, 7),
         (67, 2, True, True, 7, 1, 1, False, True, 2),
         (130, 8, True, False, 9, 3, 5, False, False, 7),
         (41, 1, False, False, 5, 1, 1, True, False, 7)]


def make_case(n, K, imprint, additive, seed, T, P, mask, skipped, max_iter=None):
    """(origin, pheno, cov, use, perm) on the map CHROM_LENS: rows soft_rows(n, CHROM_LENS, seed), covariates
    noise(n, K, seed + 1), phenotypes with Mendelian and imprinting effects of the true classes plus noise.  With `mask` two
    individuals are unused and carry NaN phenotypes and covariates; with `skipped` individuals 1 and 4 are skipped on
    chromosome 3."""
    from cnf2freq_amd import qtl
    origin, k = soft_rows(n, CHROM_LENS, seed)
    M = origin.shape[1]
    if skipped:
        origin = skip(origin, [1, 4], 3, CHROM_LENS)
    use = np.ones(n, bool)
    if mask:
        use[[0, n // 2]] = False
    cov = noise(n, K, seed + 1) if K else None
    a, d, im = CODES["a"][k], CODES["d"][k], CODES["i"][k]
    at = [(7 * t + 3) % M for t in range(T)]
    to = [(11 * t + 40) % M for t in range(T)]
    pheno = 0.6 * a[:, at] + 0.3 * d[:, to] + 0.5 * im[:, to] + noise(n, T, seed + 2)
    if K:
        pheno = pheno + 0.3 * cov[:, :1]
        cov = np.where(use[:, None], cov, np.nan)
    pheno = np.where(use[:, None], pheno, np.nan)
    perm = qtl.permutations(n, P, seed, use=use) if P else None
    return origin, pheno, cov, (use if mask else None), perm


_REFS = {}


def case_reference(case):
    """the reference of one of CASES, computed once and shared"""
    if case not in _REFS:
        n, K, imprint, additive, seed, T, P, mask, skipped, max_iter = case
        origin, pheno, cov, use, perm = make_case(*case)
        _REFS[case] = reference_scan_em(origin, chromstarts_of(CHROM_LENS), pheno, use, cov, imprint, perm, additive, max_iter, -1.0)
    return _REFS[case]


# the planted case of the stopping rule and of "not Haley-Knott in disguise"
PLANTED = dict(n=60, seed=5, marker=40, effect=0.8, tol=1e-7, max_iter=1000, short=5)


def planted_case():
    """(origin, true classes, pheno, cov): soft rows of 60 individuals, one covariate, an additive effect of the true classes
    at marker 40"""
    p = PLANTED
    origin, k = soft_rows(p["n"], CHROM_LENS, p["seed"])
    z = noise(p["n"], 1, 6)
    pheno = noise(p["n"], 1, 9) + p["effect"] * CODES["a"][k][:, p["marker"]:p["marker"] + 1] + 0.3 * z
    return origin, k, pheno, z


def planted_reference():
    if "planted" not in _REFS:
        origin, _, pheno, z = planted_case()
        _REFS["planted"] = reference_scan_em(origin, chromstarts_of(CHROM_LENS), pheno, None, z, max_iter=PLANTED["max_iter"],
                                             tol=PLANTED["tol"])
    return _REFS["planted"]


MONOTONE = (1, 2, 3, 5, 8)


def monotone_reference():
    """the planted case at exactly 8 iterations: its trace holds the LOD after every iteration"""
    if "monotone" not in _REFS:
        origin, _, pheno, z = planted_case()
        _REFS["monotone"] = reference_scan_em(origin, chromstarts_of(CHROM_LENS), pheno, None, z, max_iter=MONOTONE[-1], tol=-1.0)
    return _REFS["monotone"]


# ------------------------------------------------------------------------------------------------ degenerate and extreme inputs
def degenerate_rows(n=24, seed=8):
    """soft rows on CHROM_LENS with, on chromosome 2 (markers 3 .. 17): marker 3 without information (every row the same),
    marker 4 certain and homozygous (d and i vanish), marker 5 with o[1] == o[2] (i vanishes), marker 6 with exact zeros in
    some classes.  Returns (origin, the markers)."""
    origin, k = soft_rows(n, CHROM_LENS, seed)
    origin[:, 3] = [0.25, 0.25, 0.25, 0.25]
    origin[:, 4] = certain_rows(np.where(k[:, 4] % 2 == 0, 0, 3))
    mid = 0.5 * (origin[:, 5, 1] + origin[:, 5, 2])
    origin[:, 5, 1] = origin[:, 5, 2] = mid
    origin[1::2, 6, 1] = 0.0
    origin[::2, 6, 0] = 0.0
    origin[:, 6] /= origin[:, 6].sum(axis=1, keepdims=True)
    return origin, dict(flat=3, homozygous=4, symmetric=5, zeros=6)


def outlier_pheno(n=24, seed=8):
    """noise with individual 2 lying 10^3 null standard deviations from the rest"""
    y = noise(n, 1, seed + 3)
    y[2] += 1e3 * y.std()
    return y
