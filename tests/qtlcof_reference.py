"""The yardstick of the cofactor scan's tests (tests/test_qtlcof_host.py, tests/test_gpu_qtlcof.py): per marker a
least-squares fit in numpy of the designs [X0, cofactors] and [X0, cofactors, marker] -- qtlx_reference.lstsq on the explicit
designs, one chromosome and marker at a time, the rows of individuals with c_i = 0 deleted and the columns of the cofactors
that are left out at the marker deleted too.  It shares nothing with the product's Cholesky form
(cnf2freq_amd/csrc/cnf2_qtlcof.h).

The ranks and the relative pivots that decide which coefficients are compared come by a third route: the residual of every
added column after projection on all columns before it."""
import numpy as np

from qtl_reference import ATOL, CHROM_LENS, PIVOT_DROP, PIVOT_EXACT, PIVOT_WELL, chromstarts_of, columns, noise, skip, soft_rows  # noqa: F401
from qtlx_reference import lod_of, lstsq

MAXW = 15


def effect_columns(o, additive=False):
    """[rows][ne]: a = o[3] - o[0] and d = o[1] + o[2] (a only in the additive model) of origin rows o[rows][4]"""
    a, d = o[:, 3] - o[:, 0], o[:, 1] + o[:, 2]
    return a[:, None] if additive else np.stack([a, d], axis=1)


def width(K, Q, additive=False):
    return 1 + K + (1 if additive else 2) * (Q + 1)


def windows(cof, hw, chromstarts):
    """(excl_lo, excl_hi): +-hw markers around every cofactor, clipped to its chromosome"""
    cs = np.asarray(chromstarts, np.int64)
    cof = np.asarray(cof, np.int64).reshape(-1)
    c = np.searchsorted(cs, cof, side="right") - 1
    return np.maximum(cof - hw, cs[c]).astype(np.int32), np.minimum(cof + hw, cs[c + 1] - 1).astype(np.int32)


def chromosome_mask(o, cs, c, cof, use):
    """c_i: used, not skipped on chromosome c, not skipped on the chromosome of any cofactor"""
    keep = use & (o[:, cs[c]] != 0.0).any(axis=1)
    for m in cof:
        cq = int(np.searchsorted(cs, m, side="right") - 1)
        keep = keep & (o[:, cs[cq]] != 0.0).any(axis=1)
    return keep


def reference_scan_cof(origin, chromstarts, pheno, cof, excl_lo, excl_hi, use=None, cov=None, perm=None, additive=False):
    """The model of include/cnf2hip.h by least squares.  A dict: lod[1 + P][T][M] and lod_base[1 + P][T][M] (block 0 observed),
    coef[T][M][ne] of the observed columns (NaN for a dropped effect), rank[M], rank_cof[M], relpivot[M][ne Q + ne] in the
    design's column order (NaN for a raw diagonal of 0 and for a cofactor that is left out), usable[C], n_used[C],
    rss0[T][C], perm_max[P][T][C], candidate[M] (the marker lies in no range)."""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    cs = np.asarray(chromstarts, np.int64)
    C = len(cs) - 1
    cof = np.asarray(cof, np.int64).reshape(-1)
    lo, hi = np.asarray(excl_lo, np.int64).reshape(-1), np.asarray(excl_hi, np.int64).reshape(-1)
    Qn = len(cof)
    ne = 1 if additive else 2
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    Z = np.zeros((n, 0)) if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    K = Z.shape[1]
    nx = K + 1
    W = width(K, Qn, additive)
    assert W <= MAXW
    X0all = np.concatenate([np.ones((n, 1)), Z], axis=1)
    Y = columns(np.where(use[:, None], pheno, 0.0), perm)
    B, T = Y.shape[1], Y.shape[2]
    lod, lod_base = np.zeros((B, T, M)), np.zeros((B, T, M))
    coef = np.full((T, M, ne), np.nan)
    rank, rank_cof = np.zeros(M, np.int32), np.zeros(M, np.int32)
    relpivot = np.full((M, ne * Qn + ne), np.nan)
    usable, n_used, rss0_out = np.zeros(C, bool), np.zeros(C, np.int32), np.zeros((T, C))
    mk = np.arange(M)
    candidate = ~np.any((lo[:, None] <= mk[None, :]) & (mk[None, :] <= hi[:, None]), axis=0) if Qn else np.ones(M, bool)
    for c in range(C):
        keep = chromosome_mask(o, cs, c, cof, use)
        n_c = int(keep.sum())
        n_used[c] = n_c
        X0 = X0all[keep]
        y = Y[keep].reshape(n_c, B * T)
        usable[c] = n_c >= W + 1 and np.linalg.matrix_rank(X0) == nx
        if not usable[c]:
            continue
        rss0 = ((y - X0 @ lstsq(X0, y)) ** 2).sum(axis=0)
        rss0_out[:, c] = rss0[:T]
        cofcols = [effect_columns(o[keep, m], additive) for m in cof]
        for m in range(cs[c], cs[c + 1]):
            active = [q for q in range(Qn) if not lo[q] <= m <= hi[q]]
            place = [ne * q + e for q in active for e in range(ne)] + [ne * Qn + e for e in range(ne)]
            A = np.concatenate([cofcols[q] for q in active] + [effect_columns(o[keep, m], additive)], axis=1)
            ncof = ne * len(active)
            # third route: a column's pivot is what is left of it after projection on every column before it
            kept = np.zeros(A.shape[1], bool)
            for j in range(A.shape[1]):
                before = np.column_stack([X0, A[:, :j]])
                res = A[:, j] - before @ lstsq(before, A[:, j])
                raw = A[:, j] @ A[:, j]
                if raw > 0:
                    relpivot[m, place[j]] = (res @ res) / raw
                    kept[j] = relpivot[m, place[j]] >= PIVOT_DROP
            rank_cof[m], rank[m] = kept[:ncof].sum(), kept[ncof:].sum()
            Xc = np.column_stack([X0, A[:, :ncof]])
            Xf = np.column_stack([X0, A])
            base = lod_of(rss0, ((y - Xc @ lstsq(Xc, y)) ** 2).sum(axis=0), n_c)
            full = lod_of(rss0, ((y - Xf @ lstsq(Xf, y)) ** 2).sum(axis=0), n_c)
            lod_base[:, :, m] = base.reshape(B, T)
            if rank[m] > 0:
                lod[:, :, m] = np.maximum(full - base, 0.0).reshape(B, T)
            if kept[ncof:].any():
                Xk = np.column_stack([X0, A[:, kept]])
                beta = lstsq(Xk, y)[nx + int(kept[:ncof].sum()):, :T]
                coef[:, m, kept[ncof:]] = np.where(rss0[:T, None] > 0, beta.T, np.nan)
    perm_max = np.zeros((B - 1, T, C))
    for c in range(C):
        cand = np.flatnonzero(candidate[cs[c]:cs[c + 1]]) + cs[c]
        if cand.size:
            perm_max[:, :, c] = lod[1:][:, :, cand].max(axis=2)
    return dict(lod=lod, lod_base=lod_base, coef=coef, rank=rank, rank_cof=rank_cof, relpivot=relpivot, usable=usable,
                n_used=n_used, rss0=rss0_out, perm_max=perm_max, candidate=candidate)


def compared_markers(ref, chromstarts, share=0.99, strict=True):
    """compared[M]: the markers of scanned chromosomes whose every column, cofactor columns included, is either well
    conditioned (relative pivot at least PIVOT_WELL) or exactly degenerate (at most PIVOT_EXACT, or a raw diagonal of 0).
    Asserts on the reference alone what the comparison rests on: every marker of a scanned chromosome is of that kind
    (strict), and at least `share` of all markers are compared."""
    cs = np.asarray(chromstarts, np.int64)
    rp = ref["relpivot"]
    fine = np.all(np.isnan(rp) | (rp >= PIVOT_WELL) | (rp <= PIVOT_EXACT), axis=1)
    on = np.repeat(ref["usable"], np.diff(cs))
    assert not strict or np.all(fine[on]), "a marker is neither well conditioned nor exactly degenerate: relative pivots %s" % rp[on & ~fine]
    compared = on & fine
    if share:
        assert compared.mean() >= share, "only %.0f %% of the markers are compared" % (100 * compared.mean())
    return compared


def worst_pivot(ref, chromstarts):
    """the smallest relative pivot of a kept column over the markers of the scanned chromosomes"""
    on = np.repeat(ref["usable"], np.diff(np.asarray(chromstarts, np.int64)))
    rp = ref["relpivot"][on]
    rp = rp[np.isfinite(rp) & (rp >= PIVOT_DROP)]
    return rp.min() if rp.size else np.nan


def compare_cof(got, ref, chromstarts, what="", share=0.99, strict=True):
    """every output of a scan against the reference: lod and lod_base at every cell, coef at the compared markers (NaN exactly
    where the reference drops an effect), rank, rank_cof, n_used, rss0, perm_max.  Prints every figure before it asserts;
    returns the errors."""
    compared = compared_markers(ref, chromstarts, share, strict)
    err_l = np.abs(got["lod"] - ref["lod"][0]).max()
    err_b = np.abs(got["lod_base"] - ref["lod_base"][0]).max()
    gc, rc = got["coef"][:, compared], ref["coef"][:, compared]
    assert np.array_equal(np.isnan(gc), np.isnan(rc)), what + ": a dropped effect is NaN, a kept one a number"
    both = ~np.isnan(rc)
    err_c = (np.abs(gc[both] - rc[both]) / np.maximum(1.0, np.abs(rc[both]))).max() if both.any() else 0.0
    err_r = np.abs(got["rss0"] - ref["rss0"]).max()
    print("%s: lod %.3g, lod_base %.3g over %d cells, coef %.3g over %d of %d markers, rss0 %.3g" %
          (what, err_l, err_b, got["lod"].size, err_c, compared.sum(), len(compared), err_r))
    assert np.array_equal(got["rank"], ref["rank"]), what + " rank"
    assert np.array_equal(got["rank_cof"], ref["rank_cof"]), what + " rank_cof"
    assert np.array_equal(got["n_used"], ref["n_used"]), what + " n_used"
    assert err_l <= ATOL, what + " lod"
    assert err_b <= ATOL, what + " lod_base"
    assert err_c <= ATOL, what + " coef"
    assert err_r <= ATOL * max(1.0, np.abs(ref["rss0"]).max()), what + " rss0"
    for key in ("lod", "lod_base"):
        assert np.isfinite(got[key]).all() and np.all(got[key] >= 0), what + " " + key + " finite and not negative"
    off = ~np.repeat(ref["usable"], np.diff(np.asarray(chromstarts, np.int64)))
    assert np.all(got["lod"][:, off] == 0.0) and np.all(got["lod_base"][:, off] == 0.0) and np.isnan(got["coef"][:, off]).all()
    assert np.all(got["rank"][off] == 0) and np.all(got["rank_cof"][off] == 0)
    assert np.all(got["lod"][:, got["rank"] == 0] == 0.0), what + ": rank 0 gives LOD 0 exactly"
    err_p = 0.0
    if ref["perm_max"].shape[0]:
        err_p = np.abs(got["perm_max"] - ref["perm_max"]).max()
        print("%s: perm_max %.3g over %d cells" % (what, err_p, ref["perm_max"].size))
        assert err_p <= ATOL, what + " perm_max"
    else:
        assert got["perm_max"] is None
    return dict(lod=err_l, lod_base=err_b, coef=err_c, rss0=err_r, perm_max=err_p)


def gram_of(origin, chromstarts, m, pheno_cols, cof, use=None, cov=None, additive=False):
    """What the marker kernel forms for marker m with NO cofactor left out, in numpy: (gram[16][16], xty[R][16], yy[R], n_c)
    for the columns pheno_cols[n][R] -- the inputs of cnf2h_qtlcof_marker, which leaves cofactors out by its skip word"""
    o = np.asarray(origin, np.float64)
    n = o.shape[0]
    cs = np.asarray(chromstarts, np.int64)
    c = int(np.searchsorted(cs, m, side="right") - 1)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    keep = chromosome_mask(o, cs, c, cof, use)
    Z = np.zeros((n, 0)) if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    X = np.column_stack([np.ones(n), Z] + [effect_columns(o[:, q], additive) for q in cof] + [effect_columns(o[:, m], additive)])
    X = np.where(keep[:, None], X, 0.0)
    y = np.where(use[:, None], np.asarray(pheno_cols, np.float64).reshape(n, -1), 0.0)
    W = X.shape[1]
    gram, xty = np.zeros((16, 16)), np.zeros((y.shape[1], 16))
    gram[:W, :W] = X.T @ X
    xty[:, :W] = y.T @ X
    return gram, xty, (np.where(keep[:, None], y, 0.0) ** 2).sum(axis=0), int(keep.sum())


def explicit_multi(origin, chromstarts, pheno, loci, use=None, cov=None, additive=False):
    """The Q-locus model fitted outright, with and without each locus: (lod_full[T], drop_one[T][Q], coef[T][Q][ne]) under
    the mask of all the loci's chromosomes"""
    o = np.asarray(origin, np.float64)
    n = o.shape[0]
    cs = np.asarray(chromstarts, np.int64)
    ne = 1 if additive else 2
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    keep = chromosome_mask(o, cs, int(np.searchsorted(cs, loci[0], side="right") - 1), loci, use)
    Z = np.zeros((n, 0)) if cov is None else np.asarray(cov, np.float64).reshape(n, -1)
    X0 = np.column_stack([np.ones(n), Z])[keep]
    y = np.asarray(pheno, np.float64).reshape(n, -1)[keep]
    n_c = int(keep.sum())
    rss = lambda X: ((y - X @ lstsq(X, y)) ** 2).sum(axis=0)
    cols = [effect_columns(o[keep, m], additive) for m in loci]
    Xf = np.column_stack([X0] + cols)
    rss0, rssf = rss(X0), rss(Xf)
    full = lod_of(rss0, rssf, n_c)
    beta = lstsq(Xf, y)[X0.shape[1]:]
    drop = np.stack([full - lod_of(rss0, rss(np.column_stack([X0] + [cc for k, cc in enumerate(cols) if k != q])), n_c)
                     for q in range(len(loci))], axis=1)
    return full, drop, beta.T.reshape(y.shape[1], len(loci), ne)


def reference_scanner(origin, chromstarts, pheno, cov=None, use=None, additive=False):
    """scanner(cof, excl, permutations, seed) for qtl.forward_select and qtl.fit_multi by the reference alone: the observed
    scan, and with permutations the scan of the permuted Freedman-Lane residuals of the null model [1, cov, every cofactor's
    columns]; the dict has scan_cof's keys (lod and lod_base the observed block)"""
    from cnf2freq_amd import qtl
    o = np.asarray(origin, np.float64)
    n = o.shape[0]
    y = np.asarray(pheno, np.float64).reshape(n, -1)
    u = np.ones(n, bool) if use is None else np.asarray(use) != 0

    def scanner(cof, excl, permutations, seed):
        ref = reference_scan_cof(o, chromstarts, y, cof, excl[0], excl[1], u, cov, None, additive)
        out = dict(ref, lod=ref["lod"][0], lod_base=ref["lod_base"][0], perm_max=None)
        if permutations:
            parts = ([] if cov is None else [np.asarray(cov, np.float64).reshape(n, -1)]) + [effect_columns(o[:, m], additive) for m in cof]
            res = qtl.null_residuals(y, np.concatenate(parts, axis=1) if parts else None, u)
            perm = qtl.permutations(n, permutations, seed, use=u)
            out["perm_max"] = reference_scan_cof(o, chromstarts, res, cof, excl[0], excl[1], u, cov, perm, additive)["perm_max"]
        return out
    return scanner


# ------------------------------------------------------------------------------------------------ the cases of the issue
#         n   K  cofactors                               hw additive seed  T   P  mask  skipped
CASES = [(41, 0, (22, 60), 3, False, 6, 1, 5, False, False),
         (67, 2, (5, 26, 70), 2, False, 7, 3, 1, False, True),
         (67, 2, (5, 40, 70), 2, False, 7, 3, 1, False, True),
         (130, 0, (10, 25, 40, 45, 60, 75), 4, False, 9, 17, 0, False, False),
         (64, 1, (4, 9, 14, 20, 30, 38, 47, 55, 66, 80), 1, True, 5, 1, 33, True, False),
         (24, 0, (0, 2), 0, False, 3, 1, 1, False, False),
         (17, 0, (40,), 2, False, 4, 1, 1, False, False),
         (41, 3, (8, 60), 16, True, 6, 1, 1, True, False)]
# the worst relative pivot of a kept column per case, as the issue states them (two digits)
WORST_PIVOT = (0.125, 0.18, 0.20, 0.20, 0.38, 0.018, 0.034, 0.64)


def case_id(c):
    return "n%d-K%d-cof%s-hw%d%s-T%d-P%d%s" % (c[0], c[1], "_".join(str(m) for m in c[2]), c[3], "-add" if c[4] else "", c[6], c[7],
                                                "-mask" if c[8] else "-skip" if c[9] else "")


def make_case(n, K, cof, hw, additive, seed, T, P, mask, skipped):
    """(origin, pheno, cov, use, perm, excl) on the map CHROM_LENS: rows soft_rows(n, CHROM_LENS, seed), covariates
    noise(n, K, seed + 1), phenotypes with effects at the cofactors and at markers of their own plus noise.  With `mask` two
    individuals are unused and carry NaN phenotypes and covariates; with `skipped` individuals 1 and 4 are skipped on
    chromosome 3.  excl = +-hw markers around every cofactor, clipped to its chromosome."""
    from cnf2freq_amd import qtl
    origin, _ = soft_rows(n, CHROM_LENS, seed)
    M = origin.shape[1]
    if skipped:
        origin = skip(origin, [1, 4], 3, CHROM_LENS)
    use = np.ones(n, bool)
    if mask:
        use[[0, n // 2]] = False
    cov = noise(n, K, seed + 1) if K else None
    a = origin[:, :, 3] - origin[:, :, 0]
    d = origin[:, :, 1] + origin[:, :, 2]
    at = [(7 * t + 3) % M for t in range(T)]
    pheno = 0.6 * a[:, at] + 0.3 * d[:, at] + noise(n, T, seed + 2)
    for k, m in enumerate(cof):
        pheno = pheno + (0.5 + 0.1 * (k % 3)) * a[:, m:m + 1]
    if K:
        pheno = pheno + 0.3 * cov[:, :1]
        cov = np.where(use[:, None], cov, np.nan)
    pheno = np.where(use[:, None], pheno, np.nan)
    perm = qtl.permutations(n, P, seed, use=use) if P else None
    return origin, pheno, cov, (use if mask else None), perm, windows(cof, hw, chromstarts_of(CHROM_LENS))


_REFS = {}


def case_reference(case):
    """the reference of one of CASES, computed once and shared"""
    if case not in _REFS:
        n, K, cof, hw, additive, seed, T, P, mask, skipped = case
        origin, pheno, cov, use, perm, excl = make_case(*case)
        _REFS[case] = reference_scan_cof(origin, chromstarts_of(CHROM_LENS), pheno, cof, excl[0], excl[1], use, cov, perm, additive)
    return _REFS[case]


# ------------------------------------------------------------------------------------------------ planted effects
PLANTED = dict(n=200, seed=11, loci=(42, 67), effects=(0.8, 0.5), noise_seed=13, hw=3, permutations=100, perm_seed=5)


def planted_case():
    """(origin, pheno[n][1]): soft_rows(200, CHROM_LENS, 11) with their true classes k and
    phenotype = noise + 0.8 ([k = 3] - [k = 0]) at marker 42 + 0.5 ([k = 3] - [k = 0]) at marker 67"""
    p = PLANTED
    origin, k = soft_rows(p["n"], CHROM_LENS, p["seed"])
    y = noise(p["n"], 1, p["noise_seed"])[:, 0]
    for m, e in zip(p["loci"], p["effects"]):
        y = y + e * ((k[:, m] == 3).astype(float) - (k[:, m] == 0))
    return origin, y[:, None]


_PLANTED_REF = []


def planted_reference():
    """what the reference alone finds on planted_case, computed once: (plain: the scan without cofactors, cond: the scan with
    cofactor 42 left out within +-hw markers, sel: qtl.forward_select driven by the reference, window in map units of the map
    pos = 2 x index within the chromosome)"""
    if not _PLANTED_REF:
        from cnf2freq_amd import qtl
        p = PLANTED
        origin, pheno = planted_case()
        cs = chromstarts_of(CHROM_LENS)
        scanner = reference_scanner(origin, cs, pheno)
        none = np.zeros(0, np.int32)
        plain = scanner(none, (none, none), 0, 0)
        cond = scanner(np.array([p["loci"][0]], np.int32), windows([p["loci"][0]], p["hw"], cs), 0, 0)
        sel = qtl.forward_select(None, pheno, 5, 2.0 * p["hw"], planted_pos(), permutations=p["permutations"], seed=p["perm_seed"],
                                 scanner=scanner, chromstarts=cs)
        _PLANTED_REF.append((plain, cond, sel))
    return _PLANTED_REF[0]


def planted_pos():
    return np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in CHROM_LENS])
