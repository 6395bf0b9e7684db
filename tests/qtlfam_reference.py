"""The yardstick of the within-family scan's tests (tests/test_qtlfam_host.py, tests/test_gpu_qtlfam.py): per chromosome and
marker the explicit dense design of the nested half-sib model -- one dummy per used cell, the covariates, one slope column
per family -- solved with np.linalg.lstsq, the rows of individuals with c_i = 0 deleted.  It shares nothing with the
product's elimination (cnf2freq_amd/csrc/cnf2_qtlfam.h): no centring within cells, no diagonal block, no Schur complement.

Which families are fitted, and the relative pivots that decide which slopes are compared, come from a third route: the
residual of every slope column after projection on the cells (the fitted rule) and on the cells and covariates (the
conditioning), again by lstsq."""
import numpy as np

from cnf2freq_amd import synth
from qtl_reference import ATOL, CLAMP, PIVOT_DROP, PIVOT_EXACT, PIVOT_WELL, columns, soft_rows      # noqa: F401

SIZES = (1, 2, 3, 4, 5, 8, 9)           # family sizes: the padding edges of the 4-slot step; a family of one is never fitted


def regressor(origin, side):
    """x[n][M]: P(bit = 1) - P(bit = 0) of bit 0 (side 0) or bit 3 (side 1) of the origin rows"""
    o = np.asarray(origin, np.float64)
    return o[..., 1] + o[..., 3] - o[..., 0] - o[..., 2] if side == 0 else o[..., 2] + o[..., 3] - o[..., 0] - o[..., 1]


def sized_families(sizes=SIZES, fine=False, seed=3):
    """(grp[n], cell[n]) for families of the given sizes, the individuals dealt to them in a shuffled order (so that the
    gather list is no identity).  fine: every family of four or more is split into two cells of floor and ceil half."""
    n = int(np.sum(sizes))
    order = np.argsort(synth.uniform(seed, np.arange(n)), kind="stable")
    grp, cell = np.zeros(n, np.int32), np.zeros(n, np.int32)
    at, q = 0, 0
    for f, k in enumerate(sizes):
        members = order[at:at + k]
        at += k
        grp[members] = f
        parts = [members[:k // 2], members[k // 2:]] if fine and k >= 4 else [members]
        for part in parts:
            cell[part] = 100 + 7 * q          # (cell numbers need not be dense)
            q += 1
    return grp, cell


def residual(X, v):
    return v - X @ np.linalg.lstsq(X, v, rcond=None)[0] if X.shape[1] else v


def reference_scan(origin, chromstarts, side, grp, cell, F, pheno, use=None, cov=None, perm=None):
    """The model of include/cnf2hip.h by least squares.  A dict: lod[1 + P][T][M] (block 0 observed), slope[T][M][F] of the
    observed columns, df[M], fitted[M][F], cellpivot[M][F] and relpivot[M][F] (the squared residual of a slope column after
    projection on the cells / on the cells and covariates, over its raw square; NaN for a raw square of 0), scanned[C],
    n_used[C], n_cells[C], rss0[T][C], perm_max[P][T][C]."""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    cs = np.asarray(chromstarts, np.int64)
    C = len(cs) - 1
    grp = np.asarray(grp)
    cell = grp if cell is None else np.asarray(cell)
    use = (np.ones(n, bool) if use is None else np.asarray(use) != 0) & (grp >= 0)
    Z = np.zeros((n, 0)) if cov is None else np.asarray(cov, np.float64).reshape(n, -1)
    K = Z.shape[1]
    Y = columns(np.where(use[:, None], pheno, 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    x_all = regressor(o, side)
    lod = np.zeros((Q, T, M))
    slope = np.full((T, M, F), np.nan)
    df = np.zeros(M, np.int32)
    fitted = np.zeros((M, F), bool)
    cellpivot, relpivot = np.full((M, F), np.nan), np.full((M, F), np.nan)
    scanned = np.zeros(C, bool)
    n_used, n_cells = np.zeros(C, np.int32), np.zeros(C, np.int32)
    rss0_out = np.zeros((T, C))
    for c in range(C):
        keep = use & (o[:, cs[c]] != 0.0).any(axis=1)
        n_c = int(keep.sum())
        ids = np.unique(cell[keep])
        n_used[c], n_cells[c] = n_c, len(ids)
        if n_c == 0:
            continue
        D = (cell[keep][:, None] == ids[None, :]).astype(np.float64)
        X0 = np.concatenate([D, Z[keep]], axis=1)
        y = Y[keep].reshape(n_c, Q * T)
        scanned[c] = n_c - len(ids) - K >= 2 and np.linalg.matrix_rank(X0) == X0.shape[1]
        if not scanned[c]:
            continue
        rss0 = (residual(X0, y) ** 2).sum(axis=0)
        rss0_out[:, c] = rss0[:T]
        g = grp[keep]
        for m in range(cs[c], cs[c + 1]):
            x = x_all[keep, m]
            cols = []
            for p in range(F):
                xp = np.where(g == p, x, 0.0)
                raw = xp @ xp
                if raw > 0:
                    rd, rz = residual(D, xp), residual(X0, xp)
                    cellpivot[m, p], relpivot[m, p] = rd @ rd / raw, rz @ rz / raw
                    fitted[m, p] = cellpivot[m, p] >= PIVOT_DROP
                if fitted[m, p]:
                    cols.append(xp)
            X = np.column_stack([X0] + cols)
            if n_c - X.shape[1] < 1 or np.linalg.matrix_rank(X) < X.shape[1]:
                continue
            df[m] = len(cols)
            beta = np.linalg.lstsq(X, y, rcond=None)[0]
            rss1 = ((y - X @ beta) ** 2).sum(axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                drss = np.clip(rss0 - rss1, 0.0, rss0 * CLAMP)
                l = np.where(rss0 > 0, 0.5 * n_c * np.log10(rss0 / (rss0 - drss)), 0.0)
            lod[:, :, m] = l.reshape(Q, T)
            slope[:, m, fitted[m]] = beta[X0.shape[1]:, :T].T
    perm_max = np.zeros((Q - 1, T, C))
    for c in range(C):
        perm_max[:, :, c] = lod[1:, :, cs[c]:cs[c + 1]].max(axis=2)
    return dict(lod=lod, slope=slope, df=df, fitted=fitted, cellpivot=cellpivot, relpivot=relpivot, scanned=scanned,
                n_used=n_used, n_cells=n_cells, rss0=rss0_out, perm_max=perm_max)


def compared_markers(ref, chromstarts, share=0.9):
    """compared[M]: the markers whose slopes are compared -- fitted as a marker (df > 0) with every fitted family's relative
    pivot at least PIVOT_WELL.  Asserts what the comparison rests on: on a scanned chromosome a dropped family is degenerate
    by construction (identical rows within each of its cells: the residual after the cells at most PIVOT_EXACT, or no raw
    square at all), a fitted one clears the rule by two decades (which families are fitted is no matter of rounding), and at
    least `share` of all markers are compared."""
    cs = np.asarray(chromstarts, np.int64)
    on = np.repeat(ref["scanned"], np.diff(cs))
    cp, rp = ref["cellpivot"], ref["relpivot"]
    none = np.isnan(cp)
    well = none | ~ref["fitted"] | (rp >= PIVOT_WELL)
    exact = none | (ref["fitted"] & (cp >= 100 * PIVOT_DROP)) | (~ref["fitted"] & (cp <= PIVOT_EXACT))
    assert np.all(exact[on]), "a family is neither clearly fitted nor exactly degenerate: pivots %s" % cp[on][~exact[on]]
    compared = on & well.all(axis=1) & (ref["df"] > 0)
    if share:
        assert compared.mean() >= share, "only %.0f %% of the markers have compared slopes" % (100 * compared.mean())
    return compared


def compare(got, ref, chromstarts, what="", share=0.9):
    """lod at every cell, slopes at the compared markers (NaN exactly where the reference has none), df, n_used, n_cells,
    rss0, perm_max; prints every figure before it asserts"""
    compared = compared_markers(ref, chromstarts, share)
    err_l = np.abs(got["lod"] - ref["lod"][0]).max()
    err_r = np.abs(got["rss0"] - ref["rss0"]).max()
    err_s, n_s = 0.0, 0
    if got.get("slope") is not None:
        gs, rs = got["slope"][:, compared], ref["slope"][:, compared]
        assert np.array_equal(np.isnan(got["slope"]), np.isnan(ref["slope"])), what + " which slopes are NaN"
        num = ~np.isnan(rs)
        n_s = int(num.sum())
        err_s = (np.abs(gs[num] - rs[num]) / np.maximum(1.0, np.abs(rs[num]))).max() if n_s else 0.0
    print("%s: lod %.3g over %d cells, slope %.3g over %d values at %d of %d markers, rss0 %.3g" %
          (what, err_l, got["lod"].size, err_s, n_s, compared.sum(), len(compared), err_r))
    assert np.array_equal(got["df"], ref["df"]), what + " df"
    assert np.array_equal(got["n_used"], ref["n_used"]), what + " n_used"
    assert np.array_equal(got["n_cells"], ref["n_cells"]), what + " n_cells"
    assert err_l <= ATOL, what + " lod"
    assert err_s <= ATOL, what + " slope"
    assert err_r <= ATOL * max(1.0, np.abs(ref["rss0"]).max()), what + " rss0"
    assert np.all(got["lod"] >= 0) and np.isfinite(got["lod"]).all()
    assert np.all(got["lod"][:, ref["df"] == 0] == 0.0), what + " lod where nothing is fitted"
    if ref["perm_max"].shape[0]:
        err_p = np.abs(got["perm_max"] - ref["perm_max"]).max()
        print("%s: perm_max %.3g over %d cells" % (what, err_p, ref["perm_max"].size))
        assert err_p <= ATOL, what + " perm_max"
    return compared


# ------------------------------------------------------------------------------------------------ the shared cases
#        T   P  K  side  fine   mask   skip
CASES = [(1, 0, 0, 0, False, False, False),          # one column
         (4, 3, 1, 1, True, True, False),            # 16 columns: one full tile of the cap
         (17, 0, 8, 0, False, False, True),          # 17 columns; the instantiation for more than two covariates
         (3, 33, 2, 1, True, True, True),            # 102 columns: the second wave of a block
         (2, 7, 8, 0, True, False, False)]           # permutations through the other instantiation
SKIP_CHROM = 3


def make_case(T, P, K, side, fine, mask, skipped, seed=11):
    """(origin, grp, cell, F, pheno, cov, use, perm) on the map CHROM_LENS with the families SIZES.  mask: one member of the
    families of 9 and of 5 is not used (NaN phenotypes and covariates).  skipped: on chromosome SKIP_CHROM the family of 2 is
    emptied and the family of 3 keeps one member, so it loses its slope there."""
    from cnf2freq_amd import qtl
    from qtl_reference import CHROM_LENS, noise, skip
    grp, cell = sized_families(fine=fine)
    n, F = len(grp), len(SIZES)
    origin, _ = soft_rows(n, CHROM_LENS, seed + n)
    M = origin.shape[1]
    if skipped:
        gone = np.concatenate([np.flatnonzero(grp == 1), np.flatnonzero(grp == 2)[:2]])
        origin = skip(origin, gone, SKIP_CHROM, CHROM_LENS)
    use = np.ones(n, bool)
    if mask:
        use[[np.flatnonzero(grp == 6)[1], np.flatnonzero(grp == 4)[0]]] = False
    cov = synth.uniform(seed * 16 + 9, np.arange(n * K)).reshape(n, K) * 2.0 - 1.0 if K else None
    x = regressor(origin, side)
    sign = np.where(grp % 2 == 0, 1.0, -1.0)
    at = [(7 * t + 3) % M for t in range(T)]
    pheno = 0.8 * sign[:, None] * x[:, at] + 0.1 * (cell % 5)[:, None] + noise(n, T, seed)
    if K:
        pheno = pheno + 0.3 * cov[:, :1]
        cov = np.where(use[:, None], cov, np.nan)
    pheno = np.where(use[:, None], pheno, np.nan)
    perm = qtl.permutations(n, P, seed, use=use, strata=cell) if P else None
    return origin, grp, (cell if fine else None), F, pheno, cov, (use if mask else None), perm
