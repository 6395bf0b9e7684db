"""The yardstick of the extended single-locus scan's tests (tests/test_qtlx_host.py, tests/test_gpu_qtlx.py): per marker a
least-squares fit in numpy of the nested designs Mendelian (a, d), imprinting (+ i) and interaction (+ the products with
the interactive covariates) -- np.linalg.lstsq on the explicit designs (their columns scaled to unit length: lstsq below),
one chromosome and marker at a time, the rows of individuals with c_i = 0 deleted.  It shares nothing with the product's Cholesky form (cnf2freq_amd/csrc/cnf2_qtlx.h).

The ranks and the relative pivots that decide which coefficients are compared come by a third route: the residual of every
added column after projection on all columns before it."""
import numpy as np

from qtl_reference import ATOL, CHROM_LENS, CLAMP, PIVOT_DROP, PIVOT_EXACT, PIVOT_WELL, chromstarts_of, columns, noise, skip, soft_rows  # noqa: F401

MAXW = 15


def effects(additive=False, imprint=False):
    return ["a"] + ([] if additive else ["d"]) + (["i"] if imprint else [])


def design_columns(K, Ki, additive=False, imprint=False):
    """[(effect name, modifier k, stage)] of the added columns in the model's order (include/cnf2hip.h); modifier 0 = none,
    k = covariate k - 1"""
    eff = effects(additive, imprint)
    cols = [(e, 0, 1 if e == "i" else 0) for e in eff]
    cols += [(e, k, 2) for k in range(1, Ki + 1) for e in eff]
    return cols


def width(K, Ki, additive=False, imprint=False):
    return 1 + K + len(effects(additive, imprint)) * (1 + Ki)


def lod_of(rss0, rss1, n_c):
    with np.errstate(divide="ignore", invalid="ignore"):
        drss = np.clip(rss0 - rss1, 0.0, rss0 * CLAMP)
        return np.where(rss0 > 0, 0.5 * n_c * np.log10(rss0 / (rss0 - drss)), 0.0)


def lstsq(X, y):
    """np.linalg.lstsq on the columns of X scaled to unit length (a zero column stays), the solution scaled back.  Exact least
    squares does not depend on the scale of a column and neither does the model's rank rule, which is relative to the
    column's own raw diagonal; lstsq's cut-off, relative to the largest singular value, would drop a column that is merely
    small -- the i of a cross whose two heterozygotes cannot be told apart is the sweep's rounding noise, 1e-17 of the others."""
    norm = np.sqrt((X * X).sum(axis=0))
    norm[norm == 0.0] = 1.0
    beta = np.linalg.lstsq(X / norm, y, rcond=None)[0]
    return (beta.T / norm).T


def reference_scanx(origin, chromstarts, pheno, use=None, cov=None, n_int=0, imprint=False, perm=None, additive=False):
    """The model of include/cnf2hip.h by least squares.  A dict: lod[1 + P][T][M][3] (block 0 observed), coef[T][M][ne (1 + Ki)]
    of the observed columns (NaN for a dropped column), rank[M][3], relpivot[M][ne (1 + Ki)] (NaN for a raw diagonal of 0),
    usable[C], n_used[C], rss0[T][C], perm_max[P][T][C][5]."""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    cs = np.asarray(chromstarts, np.int64)
    C = len(cs) - 1
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    Z = np.zeros((n, 0)) if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    K = Z.shape[1]
    X0all = np.concatenate([np.ones((n, 1)), Z], axis=1)
    nx = K + 1
    cols = design_columns(K, n_int, additive, imprint)
    W = nx + len(cols)
    assert W == width(K, n_int, additive, imprint) and W <= MAXW
    Y = columns(np.where(use[:, None], pheno, 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    lod = np.zeros((Q, T, M, 3))
    coef = np.full((T, M, len(cols)), np.nan)
    rank = np.zeros((M, 3), np.int32)
    relpivot = np.full((M, len(cols)), np.nan)
    usable = np.zeros(C, bool)
    n_used = np.zeros(C, np.int32)
    rss0_out = np.zeros((T, C))
    for c in range(C):
        keep = use & (o[:, cs[c]] != 0.0).any(axis=1)
        n_c = int(keep.sum())
        n_used[c] = n_c
        X0 = X0all[keep]
        y = Y[keep].reshape(n_c, Q * T)
        usable[c] = n_c >= W + 1 and np.linalg.matrix_rank(X0) == nx
        if not usable[c]:
            continue
        r0 = y - X0 @ lstsq(X0, y)
        rss0 = (r0 ** 2).sum(axis=0)
        rss0_out[:, c] = rss0[:T]
        for m in range(cs[c], cs[c + 1]):
            om = o[keep, m]
            val = dict(a=om[:, 3] - om[:, 0], d=om[:, 1] + om[:, 2], i=om[:, 1] - om[:, 2])
            A = np.stack([val[e] * (1.0 if k == 0 else Z[keep, k - 1]) for e, k, _ in cols], axis=1)
            stage = np.array([s for _, _, s in cols])
            # third route: a column's pivot is what is left of it after projection on every column before it
            kept = np.zeros(len(cols), bool)
            for j in range(len(cols)):
                before = np.column_stack([X0, A[:, :j]])
                res = A[:, j] - before @ lstsq(before, A[:, j])
                raw = A[:, j] @ A[:, j]
                if raw > 0:
                    relpivot[m, j] = (res @ res) / raw
                    kept[j] = relpivot[m, j] >= PIVOT_DROP
            rank[m] = np.cumsum([kept[stage == s].sum() for s in range(3)])
            prev = np.zeros(Q * T)
            for s in range(3):
                if (stage == s).any():
                    X = np.column_stack([X0, A[:, stage <= s]])
                    rss = ((y - X @ lstsq(X, y)) ** 2).sum(axis=0)
                    prev = lod_of(rss0, rss, n_c)
                lod[:, :, m, s] = prev.reshape(Q, T)
            if kept.any():
                X = np.column_stack([X0, A[:, kept]])
                beta = lstsq(X, y)
                coef[:, m, kept] = np.where(rss0[:T, None] > 0, beta[nx:, :T].T, np.nan)
    perm_max = np.zeros((Q - 1, T, C, 5))
    stat = np.concatenate([lod[1:], lod[1:, :, :, 1:2] - lod[1:, :, :, 0:1], lod[1:, :, :, 2:3] - lod[1:, :, :, 1:2]], axis=3)
    for c in range(C):
        perm_max[:, :, c] = stat[:, :, cs[c]:cs[c + 1]].max(axis=2)
    return dict(lod=lod, coef=coef, rank=rank, relpivot=relpivot, usable=usable, n_used=n_used, rss0=rss0_out,
                perm_max=perm_max, cols=cols)


def compared_markers(ref, chromstarts, share=0.99, strict=True):
    """compared[M]: the markers of scanned chromosomes whose every column is either well conditioned (relative pivot at
    least PIVOT_WELL) or exactly degenerate (at most PIVOT_EXACT, or a raw diagonal of 0).  Asserts on the reference alone
    what the comparison rests on: every marker of a scanned chromosome is of that kind (strict; on rows that are not made
    for the purpose, strict = False leaves the others out of the comparison of coef instead), and at least `share` of all
    markers are compared."""
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


def comparex(got, ref, chromstarts, what="", share=0.99, strict=True):
    """every output of a scan against the reference: the three LODs and the two differences at every cell, coef at the compared
    markers (NaN exactly where the reference drops a column), rank, n_used, rss0, perm_max; the nesting of the LODs.  Prints
    every figure before it asserts; returns the errors."""
    compared = compared_markers(ref, chromstarts, share, strict)
    rl = ref["lod"][0]
    err_l = np.abs(got["lod"] - rl).max()
    dg = np.stack([got["lod"][..., 1] - got["lod"][..., 0], got["lod"][..., 2] - got["lod"][..., 1]], axis=-1)
    dr = np.stack([rl[..., 1] - rl[..., 0], rl[..., 2] - rl[..., 1]], axis=-1)
    err_d = np.abs(dg - dr).max()
    gc, rc = got["coef"][:, compared], ref["coef"][:, compared]
    assert np.array_equal(np.isnan(gc), np.isnan(rc)), what + ": a dropped column is NaN, a kept one a number"
    both = ~np.isnan(rc)
    err_c = (np.abs(gc[both] - rc[both]) / np.maximum(1.0, np.abs(rc[both]))).max() if both.any() else 0.0
    err_r = np.abs(got["rss0"] - ref["rss0"]).max()
    print("%s: lod %.3g, differences %.3g over %d cells, coef %.3g over %d of %d markers, rss0 %.3g" %
          (what, err_l, err_d, got["lod"].size, err_c, compared.sum(), len(compared), err_r))
    assert np.array_equal(got["rank"], ref["rank"]), what + " rank"
    assert np.array_equal(got["n_used"], ref["n_used"]), what + " n_used"
    assert err_l <= ATOL, what + " lod"
    assert err_d <= ATOL, what + " lod differences"
    assert err_c <= ATOL, what + " coef"
    assert err_r <= ATOL * max(1.0, np.abs(ref["rss0"]).max()), what + " rss0"
    assert np.isfinite(got["lod"]).all() and np.all(got["lod"][..., 0] >= 0) and np.all(dg >= 0), what + " nesting"
    off = ~np.repeat(ref["usable"], np.diff(np.asarray(chromstarts, np.int64)))
    assert np.all(got["lod"][:, off] == 0.0) and np.isnan(got["coef"][:, off]).all() and np.all(got["rank"][off] == 0)
    assert np.all(got["lod"][:, got["rank"][:, 2] == 0] == 0.0), what + ": rank 0 gives LOD 0 exactly"
    err_p = 0.0
    if ref["perm_max"].shape[0]:
        err_p = np.abs(got["perm_max"] - ref["perm_max"]).max()
        print("%s: perm_max %.3g over %d cells" % (what, err_p, ref["perm_max"].size))
        assert err_p <= ATOL, what + " perm_max"
    else:
        assert got["perm_max"] is None
    return dict(lod=err_l, diff=err_d, coef=err_c, rss0=err_r, perm_max=err_p)


def gram_of(origin, chromstarts, m, pheno_cols, use=None, cov=None, n_int=0, imprint=False, additive=False):
    """What the marker kernel forms, in numpy: (gram[16][16], xty[R][16], yy[R], n_c) of marker m's design for the columns
    pheno_cols[n][R] -- the inputs of cnf2h_qtlx_marker"""
    o = np.asarray(origin, np.float64)
    n = o.shape[0]
    cs = np.asarray(chromstarts, np.int64)
    c = int(np.searchsorted(cs, m, side="right") - 1)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    keep = use & (o[:, cs[c]] != 0.0).any(axis=1)
    Z = np.zeros((n, 0)) if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    val = dict(a=o[:, m, 3] - o[:, m, 0], d=o[:, m, 1] + o[:, m, 2], i=o[:, m, 1] - o[:, m, 2])
    cols = design_columns(Z.shape[1], n_int, additive, imprint)
    X = np.column_stack([np.ones(n), Z] + [val[e] * (1.0 if k == 0 else Z[:, k - 1]) for e, k, _ in cols])
    X = np.where(keep[:, None], X, 0.0)
    y = np.where(use[:, None], np.asarray(pheno_cols, np.float64).reshape(n, -1), 0.0)
    W = X.shape[1]
    gram, xty = np.zeros((16, 16)), np.zeros((y.shape[1], 16))
    gram[:W, :W] = X.T @ X
    xty[:, :W] = y.T @ X
    return gram, xty, (np.where(keep[:, None], y, 0.0) ** 2).sum(axis=0), int(keep.sum())


# ------------------------------------------------------------------------------------------------ the cases of the issue
#         n   K  Ki imprint additive seed  T   P   mask   skipped
CASES = [(24, 0, 0, False, False, 3, 1, 33, False, False),
         (17, 0, 0, True, False, 4, 3, 1, False, False),
         (20, 1, 1, False, False, 4, 1, 5, False, False),
         (41, 2, 0, True, False, 6, 3, 0, False, False),
         (40, 2, 1, False, False, 5, 17, 33, False, False),
         (67, 2, 2, True, False, 7, 3, 5, False, False),
         (67, 2, 2, True, False, 7, 1, 1, False, True),
         (130, 5, 2, True, False, 9, 17, 0, False, False),
         (41, 3, 3, False, True, 6, 1, 1, True, False),
         (24, 1, 1, True, True, 3, 3, 33, False, False)]


def make_case(n, K, Ki, imprint, additive, seed, T, P, mask, skipped):
    """(origin, pheno, cov, use, perm) on the map CHROM_LENS: rows soft_rows(n, CHROM_LENS, seed), covariates
    noise(n, K, seed + 1), phenotypes with Mendelian, imprinting and interaction effects plus noise.  With `mask` two
    individuals are unused and carry NaN phenotypes and covariates; with `skipped` individuals 1 and 4 are skipped on
    chromosome 3."""
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
    im = origin[:, :, 1] - origin[:, :, 2]
    at = [(7 * t + 3) % M for t in range(T)]
    to = [(11 * t + 40) % M for t in range(T)]
    pheno = 0.6 * a[:, at] + 0.3 * d[:, to] + 0.5 * im[:, to] + noise(n, T, seed + 2)
    if K:
        pheno = pheno + 0.3 * cov[:, :1] + 0.9 * a[:, at] * cov[:, :1]
        cov = np.where(use[:, None], cov, np.nan)
    pheno = np.where(use[:, None], pheno, np.nan)
    perm = qtl.permutations(n, P, seed, use=use) if P else None
    return origin, pheno, cov, (use if mask else None), perm


_REFS = {}


def case_reference(case):
    """the reference of one of CASES, computed once and shared"""
    if case not in _REFS:
        n, K, Ki, imprint, additive, seed, T, P, mask, skipped = case
        origin, pheno, cov, use, perm = make_case(*case)
        _REFS[case] = reference_scanx(origin, chromstarts_of(CHROM_LENS), pheno, use, cov, Ki, imprint, perm, additive)
    return _REFS[case]


# ------------------------------------------------------------------------------------------------ degenerate designs
def certain_rows(classes):
    """origin[...][4] with every individual certain of its class"""
    k = np.asarray(classes)
    o = np.zeros(k.shape + (4,))
    np.put_along_axis(o, k[..., None], 1.0, axis=-1)
    return o


DEGENERATE = dict(K=1, Ki=1, imprint=True)       # W = 8


def degenerate_case():
    """(lens, origin, pheno, cov, want): 24 individuals, one interactive covariate, imprinting, on six chromosomes --
    [0] ordinary soft rows; [1] rows without information (0.25 each: a = i = 0, d constant); [2] everybody certain and
    homozygous (d = i = 0); [3] o[1] == o[2] everywhere (i = 0); [4] rows for eight individuals only (n_c = W);
    [5] the covariate is constant (0.5) wherever a row carries information -- the other twelve individuals, whose covariate
    varies, have the row (0.5, 0, 0, 0.5) with a = d = i = 0 -- so every product with it is collinear with its main effect.
    (A covariate that is constant over all used individuals makes X0 itself singular: constant_covariate_case.)
    want maps a chromosome to the rank[3] the rule must give at each of its markers."""
    from cnf2freq_amd import synth
    lens, n = (3, 2, 2, 2, 2, 2), 24
    origin, _ = soft_rows(n, lens, 5)
    origin[:, 3:5] = 0.25
    origin[:, 5:7] = certain_rows(np.where(synth.uniform(3, np.arange(n * 2)).reshape(n, 2) < 0.5, 0, 3))
    origin[:, 7:9, 1] = origin[:, 7:9, 2] = 0.5 * (origin[:, 7:9, 1] + origin[:, 7:9, 2])
    origin[8:, 9:11] = 0.0
    origin[:12, 11:13] = np.array([0.5, 0.0, 0.0, 0.5])
    cov = noise(n, 1, 8)
    cov[12:] = 0.5
    a = origin[:, :, 3] - origin[:, :, 0]
    im = origin[:, :, 1] - origin[:, :, 2]
    pheno = noise(n, 2, 4) + np.stack([0.7 * a[:, 5] + 0.5 * im[:, 0], 0.6 * a[:, 11] + 0.8 * a[:, 7] * cov[:, 0]], axis=1)
    want = {0: (2, 3, 6), 1: (0, 0, 0), 2: (1, 1, 2), 3: (2, 2, 4), 4: (0, 0, 0), 5: (2, 3, 3)}
    return lens, origin, pheno, cov, want


def constant_case():
    """(lens, origin, pheno): 16 certain individuals, 4 AA, 4 BB, 4 + 4 heterozygous of either side, two markers on one
    chromosome.  n_c = 16 has an exact square root, so the null design's sums are exact: the constant phenotype (trait 0)
    has RSS0 = 0 exactly -- LODs 0, effects NaN; trait 1 = 1 + 2 i is an ordinary column beside it."""
    k = np.array([0] * 4 + [3] * 4 + [1] * 4 + [2] * 4)
    origin = certain_rows(np.stack([k, np.roll(k, 1)], axis=1))
    i = origin[:, 0, 1] - origin[:, 0, 2]
    return (2,), origin, np.stack([np.full(16, 2.0), 1.0 + 2.0 * i + noise(16, 1, 2)[:, 0]], axis=1)


def constant_covariate_case():
    """(lens, origin, pheno, cov): soft rows of 16 individuals and an interactive covariate that is 0.5 for everybody.  X0 =
    [c, c z] is singular -- with n_c = 16 its second pivot is exactly 0 -- so by the model's rule for X0 nothing is scanned"""
    origin, _ = soft_rows(16, (3,), 5)
    return (3,), origin, noise(16, 1, 4), np.full((16, 1), 0.5)


# ------------------------------------------------------------------------------------------------ planted effects
PLANTED = dict(n=200, seed=11, m_imprint=42, m_interaction=67, e_imprint=0.6, e_interaction=1.2, permutations=200, perm_seed=5)


def planted_case():
    """(origin, pheno, cov): soft_rows(200, CHROM_LENS, seed) with their true classes k, a covariate z = +-0.5, and
    phenotype = noise + e_i ([k = 1] - [k = 2]) at one marker + e_z a_true z at a marker of another chromosome"""
    p = PLANTED
    origin, k = soft_rows(p["n"], CHROM_LENS, p["seed"])
    z = np.where(noise(p["n"], 1, p["seed"] + 1) < 0.0, -0.5, 0.5)
    ki, kz = k[:, p["m_imprint"]], k[:, p["m_interaction"]]
    y = noise(p["n"], 1, p["seed"] + 2)[:, 0]
    y = y + p["e_imprint"] * ((ki == 1).astype(float) - (ki == 2)) + p["e_interaction"] * ((kz == 3).astype(float) - (kz == 0)) * z[:, 0]
    return origin, y[:, None], z


def planted_findings(lod, perm_max, what=""):
    """What a scan of planted_case must show, asserted on lod[1][M][3] and perm_max[P][1][C][5] alone: each planted marker
    lies in the 1.5-LOD interval of its chromosome's peak of the matching difference profile, that peak is above the 5 %
    genome-wide threshold of the statistic, and no other chromosome exceeds it.  Returns the two peaks."""
    from cnf2freq_amd import qtl
    cs = chromstarts_of(CHROM_LENS)
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in CHROM_LENS])
    th = qtl.thresholdsx(perm_max, alpha=(0.05,))
    found = []
    for key, s, m in (("imprint", 0, PLANTED["m_imprint"]), ("interaction", 1, PLANTED["m_interaction"])):
        profile = lod[:, :, s + 1] - lod[:, :, s]
        c = int(np.searchsorted(cs, m, side="right") - 1)
        thr = th[key]["genome"][0, 0]
        peaks = {p["chrom"]: p for p in qtl.peaks(profile, pos, cs, -1.0)}
        pk = peaks[c]
        print("%s %s: peak %.2f at marker %d, interval %d .. %d, planted %d, threshold %.2f, other chromosomes at most %.2f" % (
            what, key, pk["lod"], pk["marker"], pk["lo"], pk["hi"], m, thr, max(p["lod"] for cc, p in peaks.items() if cc != c)))
        assert pk["lo"] <= m <= pk["hi"], key
        assert pk["lod"] > thr > 0.0, key
        assert all(p["lod"] <= pk["lod"] for cc, p in peaks.items() if cc != c), key
        found.append((pk["marker"], pk["lo"], pk["hi"]))
    return found


_PLANTED_REF = []


def planted_reference():
    """(observed reference, perm_max of the Freedman-Lane residuals by the reference) of planted_case, computed once"""
    if not _PLANTED_REF:
        from cnf2freq_amd import qtl
        origin, pheno, cov = planted_case()
        cs = chromstarts_of(CHROM_LENS)
        obs = reference_scanx(origin, cs, pheno, cov=cov, n_int=1, imprint=True)
        perm = qtl.permutations(PLANTED["n"], PLANTED["permutations"], PLANTED["perm_seed"])
        res = qtl.null_residuals(pheno, cov)
        pm = reference_scanx(origin, cs, res, cov=cov, n_int=1, imprint=True, perm=perm)["perm_max"]
        _PLANTED_REF.append((obs, pm))
    return _PLANTED_REF[0]


def tiny_imprint_case():
    """(lens, origin, pheno): soft rows of 40 individuals whose two heterozygotes are equal up to rounding noise -- o[1] and
    o[2] are both set to their mean, then o[1] is moved by a few units in its last place -- as the sweep reports them in a
    cross of inbred lines.  i = o[1] - o[2] is 1e-17 of the other columns and not exactly 0: by the rule, which is relative
    to the column's own length, it is kept, and a fit must treat it as the column it is."""
    lens = (5, 4)
    origin, _ = soft_rows(40, lens, 12)
    mean = 0.5 * (origin[:, :, 1] + origin[:, :, 2])
    step = np.round(4.0 * noise(40 * 9, 1, 13).reshape(40, 9))             # -2 .. 2 units in the last place
    origin[:, :, 2] = mean
    origin[:, :, 1] = mean + step * np.spacing(mean)
    origin[:, 0] = certain_rows(np.where(np.arange(40) % 2 == 0, 0, 3))    # (the masks look at a chromosome's first marker)
    a = origin[:, :, 3] - origin[:, :, 0]
    return lens, origin, (0.5 * a[:, 2] + noise(40, 1, 14)[:, 0])[:, None]
