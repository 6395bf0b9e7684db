"""The yardstick of the polygenic scan's tests (tests/test_qtllmm_host.py, tests/test_gpu_kinship.py, tests/test_gpu_qtlcols.py,
tests/test_gpu_qtllmm.py): numpy, sharing nothing with the product.

  kinship       A @ A.T on the explicit a columns
  column scan   np.linalg.lstsq on the explicit columns [x0, s reg(m)], one marker at a time; rank and relative pivots from
                the residuals of the regressors after projection on x0, as tests/qtl_reference.py does
  mixed model   whitening by the CHOLESKY factor of V = h2 K + (1 - h2) I, then lstsq -- no eigenvectors anywhere -- and
                the same for the likelihood that est_herit maximises, on a grid of step 1e-4

The Cholesky and eigen routes agree within 7e-13 in LOD on soft_rows (CHROM_LENS, n = 13, 24, 67, 130, h2 = 0, 0.3, 0.8,
0.99), so the bar is the project's ATOL = 1e-9, with h2 at most 0.99 in the cases."""
import numpy as np

from cnf2freq_amd import qtl, synth
from qtl_reference import (ATOL, CHROM_LENS, CLAMP, PIVOT_DROP, PIVOT_EXACT, PIVOT_WELL, chromstarts_of, columns, noise,
                           soft_rows)

__all__ = ["ATOL", "a_columns", "ad_columns", "kinship_sums_ref", "kinship_ref", "cols_columns", "cols_reference", "cols_compared",
           "cols_compare", "chol_whiten", "lmm_reference", "reference_lmm", "compare_lmm", "lmm_loglik", "grid_herit", "gaussian_like", "chromstarts_of", "cols_case", "lmm_inputs"]


def a_columns(origin):
    o = np.asarray(origin, np.float64)
    return o[:, :, 3] - o[:, :, 0]


def ad_columns(origin, additive=False):
    """reg[n][M][ne]: (a, d) of every marker"""
    o = np.asarray(origin, np.float64)
    a, d = o[:, :, 3] - o[:, :, 0], o[:, :, 1] + o[:, :, 2]
    return a[:, :, None].copy() if additive else np.stack([a, d], axis=2)


def kinship_sums_ref(origin, chromstarts, c0, c1):
    cs = np.asarray(chromstarts, np.int64)
    A = a_columns(origin)[:, cs[c0]:cs[c1]]
    return A @ A.T, int(cs[c1] - cs[c0])


def kinship_ref(origin, chromstarts, leave_out=None):
    cs = np.asarray(chromstarts, np.int64)
    keep = np.ones(cs[-1], bool)
    if leave_out is not None:
        keep[cs[leave_out]:cs[leave_out + 1]] = False
    A = a_columns(origin)[:, keep]
    return (1.0 + A @ A.T / keep.sum()) / 2.0


def gaussian_like(n, M, ne, seed):
    """reg[n][M][ne] of columns that are no probabilities: sums of twelve uniforms minus six, as rotated columns are"""
    u = synth.uniform(seed * 16 + 5, np.arange(n * M * ne * 12)).reshape(n, M, ne, 12)
    return u.sum(axis=3) - 6.0


def cols_columns(pheno, perm):
    """Y[n][(1 + P) T]: column p T + t, the observed block first"""
    Y = columns(pheno, perm)
    return Y.reshape(Y.shape[0], -1)


def cols_reference(reg, x0, pheno, scale=None, perm=None):
    """cnf2_qtl_scan_cols by least squares.  A dict: lod[1 + P][T][M], coef[T][M][2], rank[M], relpivot[M][2], usable,
    rss0[T], perm_max[P][T]."""
    reg = np.asarray(reg, np.float64)
    n, M, ne = reg.shape
    X0 = np.asarray(x0, np.float64).reshape(n, -1)
    nx = X0.shape[1]
    y = np.asarray(pheno, np.float64).reshape(n, -1)
    T = y.shape[1]
    Y = cols_columns(y, perm)
    Q = Y.shape[1] // T
    s = np.ones(n) if scale is None else np.asarray(scale, np.float64)
    lod, coef = np.zeros((Q, T, M)), np.full((T, M, 2), np.nan)
    rank, relpivot = np.zeros(M, np.int32), np.full((M, 2), np.nan)
    usable = n >= nx + 3 and np.linalg.matrix_rank(X0) == nx
    rss0_out = np.zeros(T)
    if usable:
        proj = lambda v: v - X0 @ np.linalg.lstsq(X0, v, rcond=None)[0]
        rss0 = (proj(Y) ** 2).sum(axis=0)
        rss0_out = rss0[:T].copy()
        for m in range(M):
            a = s * reg[:, m, 0]
            d = s * reg[:, m, 1] if ne == 2 else np.zeros(n)
            ra, rd = proj(a), proj(d)
            saa, sdd = a @ a, d @ d
            keep_a = saa > 0 and ra @ ra >= PIVOT_DROP * saa
            pd = rd @ rd - ((ra @ rd) ** 2 / (ra @ ra) if keep_a else 0.0)
            keep_d = ne == 2 and sdd > 0 and pd >= PIVOT_DROP * sdd
            rank[m] = int(keep_a) + int(keep_d)
            relpivot[m] = [ra @ ra / saa if saa > 0 else np.nan, pd / sdd if sdd > 0 else np.nan]
            X = np.column_stack([X0, a] + ([d] if ne == 2 else []))
            beta = np.linalg.lstsq(X, Y, rcond=None)[0]
            rss1 = ((Y - X @ beta) ** 2).sum(axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                drss = np.clip(rss0 - rss1, 0.0, rss0 * CLAMP)
                l = np.where(rss0 > 0, 0.5 * n * np.log10(rss0 / (rss0 - drss)), 0.0)
            lod[:, :, m] = l.reshape(Q, T)
            if rank[m] == ne:
                coef[:, m, 0] = beta[nx, :T]
                if ne == 2:
                    coef[:, m, 1] = beta[nx + 1, :T]
    return dict(lod=lod, coef=coef, rank=rank, relpivot=relpivot, usable=usable, rss0=rss0_out, perm_max=lod[1:].max(axis=2), ne=ne)


def cols_compared(ref, share=0.9):
    """compared[M]: full rank with every kept relative pivot at least PIVOT_WELL.  Asserts what the comparison rests on, on
    the reference alone: every marker is either that well conditioned or exactly degenerate, and at least `share` are compared."""
    cols = list(range(ref["ne"]))
    rp = ref["relpivot"][:, cols]
    well = np.all(np.nan_to_num(rp, nan=0.0) >= PIVOT_WELL, axis=1)
    exact = np.all(np.isnan(rp) | (rp >= PIVOT_WELL) | (rp <= PIVOT_EXACT), axis=1)
    if ref["usable"]:
        assert np.all(exact), "a marker is neither well conditioned nor exactly degenerate: relative pivots %s" % rp[~exact]
    compared = well & (ref["rank"] == len(cols)) & bool(ref["usable"])
    if share:
        assert compared.mean() >= share, "only %.0f %% of the markers have compared coefficients" % (100 * compared.mean())
    return compared


def cols_compare(got, ref, what="", share=0.9):
    """lod at every cell, coef at the compared markers and NaN exactly where the rank drops a column, rank, rss0, perm_max;
    prints every figure before it asserts"""
    ne = ref["ne"]
    compared = cols_compared(ref, share)
    err_l = np.abs(got["lod"] - ref["lod"][0]).max()
    live = (ref["rss0"] > 0) & bool(ref["usable"])             # (a column with RSS0 = 0 reports NaN, whatever lstsq makes of it)
    gc, rc = got["coef"][live][:, compared, :ne], ref["coef"][live][:, compared, :ne]
    err_c = (np.abs(gc - rc) / np.maximum(1.0, np.abs(rc))).max() if gc.size else 0.0
    err_r = (np.abs(got["rss0"] - ref["rss0"]) / np.maximum(1.0, np.abs(ref["rss0"]))).max()
    print("%s: lod %.3g over %d cells, coef %.3g over %d of %d markers, rss0 %.3g" %
          (what, err_l, got["lod"].size, err_c, compared.sum(), len(compared), err_r))
    assert np.array_equal(got["rank"], ref["rank"]), what + " rank"
    assert err_l <= ATOL, what + " lod"
    assert err_c <= ATOL, what + " coef"
    assert err_r <= ATOL, what + " rss0"
    assert np.all(got["lod"] >= 0) and np.isfinite(got["lod"]).all()
    nan = np.isnan(got["coef"][live])
    if ne == 1:
        assert nan[:, :, 1].all(), "one regressor reports no second effect"
        assert np.array_equal(nan[:, :, 0], np.broadcast_to(got["rank"] == 0, nan[:, :, 0].shape))
    else:
        assert np.array_equal(nan.sum(axis=2), np.broadcast_to(2 - got["rank"], nan.shape[:2])), "NaN exactly where the rank drops a column"
    assert np.isnan(got["coef"][~live]).all()
    if ref["perm_max"].shape[0]:
        err_p = np.abs(got["perm_max"] - ref["perm_max"]).max()
        print("%s: perm_max %.3g over %d cells" % (what, err_p, ref["perm_max"].size))
        assert err_p <= ATOL, what + " perm_max"
    return compared


def chol_whiten(K, h2, *arrays):
    """L^-1 of every array, V = h2 K + (1 - h2) I = L L'; also log det V"""
    n = K.shape[0]
    L = np.linalg.cholesky(h2 * np.asarray(K, np.float64) + (1.0 - h2) * np.eye(n))
    return [np.linalg.solve(L, np.asarray(a, np.float64)) for a in arrays], 2.0 * np.log(np.diag(L)).sum()


def lmm_reference(K, y, X0, reg, h2):
    """One trait of the mixed-model scan at a given h2 on reg[n][m][ne]: whiten y, X0 and every regressor by the Cholesky
    factor, then cols_reference (lstsq).  X0 carries its intercept; y[n]."""
    n, m, ne = reg.shape
    (ys, xs, rs), _ = chol_whiten(K, h2, np.asarray(y, np.float64).reshape(n, 1), X0, reg.reshape(n, m * ne))
    return cols_reference(rs.reshape(n, m, ne), xs, ys)


def reference_lmm(origin, cs, pheno, cov, h2, kin_of, keep=None, additive=False):
    """scan_lmm by the Cholesky route: per chromosome c the kinship kin_of(c) of the kept individuals, the centred trait and
    [1, centred cov], every trait at its h2[t][c].  lod[T][M], coef[T][M][2], rank[T][M], and compared[T][M]"""
    n, M = origin.shape[:2]
    keep = np.ones(n, bool) if keep is None else keep
    y = pheno[keep] - pheno[keep].mean(axis=0)
    X0 = np.ones((keep.sum(), 1)) if cov is None else np.concatenate([np.ones((keep.sum(), 1)), cov[keep] - cov[keep].mean(axis=0)], axis=1)
    T = y.shape[1]
    out = dict(lod=np.zeros((T, M)), coef=np.full((T, M, 2), np.nan), rank=np.zeros((T, M), np.int32), compared=np.zeros((T, M), bool))
    for c in range(len(cs) - 1):
        sl = slice(cs[c], cs[c + 1])
        reg = ad_columns(origin[keep][:, sl], additive)
        K = kin_of(c)[np.ix_(keep, keep)]
        for t in range(T):
            ref = lmm_reference(K, y[:, t], X0, reg, h2[t][c])
            out["lod"][t, sl], out["coef"][t, sl], out["rank"][t, sl] = ref["lod"][0, 0], ref["coef"][0], ref["rank"]
            out["compared"][t, sl] = cols_compared(ref, share=0)
    return out


def compare_lmm(got, ref, what, share=0.9, traits=None):
    ts = list(range(ref["lod"].shape[0])) if traits is None else traits
    err_l = np.abs(got["lod"][ts] - ref["lod"]).max()
    cmp_ = ref["compared"]
    gc, rc = got["coef"][ts][cmp_], ref["coef"][cmp_]
    err_c = (np.abs(gc - rc) / np.maximum(1.0, np.abs(rc))).max()
    print("%s: lod %.3g over %d cells, coef %.3g over %d of %d cells" % (what, err_l, ref["lod"].size, err_c, cmp_.sum(), cmp_.size))
    assert cmp_.mean() >= share
    assert np.array_equal(got["rank"][ts], ref["rank"]), what + " rank"
    assert err_l <= ATOL, what + " lod"
    assert err_c <= ATOL, what + " coef"


def lmm_loglik(K, y, X0, h2, reml=True):
    """the log-likelihood est_herit maximises, in its Cholesky form"""
    n, nx = X0.shape
    (ys, xs), logdet_v = chol_whiten(K, h2, np.asarray(y, np.float64).reshape(n), X0)
    r = ys - xs @ np.linalg.lstsq(xs, ys, rcond=None)[0]
    rss = float(r @ r)
    if not reml:
        return -(n * np.log(2 * np.pi * rss / n) + n + logdet_v) / 2.0
    df = n - nx
    return -(df * np.log(2 * np.pi * rss / df) + df + logdet_v + np.linalg.slogdet(xs.T @ xs)[1]) / 2.0


def grid_herit(K, y, X0, reml=True, step=1e-4, single=True):
    """(h2 of the grid's maximum over 0 .. 0.999, the grid's values); asserts a single local maximum when asked"""
    grid = np.arange(0.0, 0.999 + step / 2, step)
    vals = np.array([lmm_loglik(K, y, X0, h, reml) for h in grid])
    if single:
        d = np.diff(vals)
        d = np.sign(d[np.abs(d) > 1e-9 * max(1.0, np.abs(vals).max())])      # (steps within the likelihood's own rounding: flat)
        assert np.count_nonzero(np.diff(d) != 0) <= 1 and (len(d) == 0 or d[0] > 0 or np.all(d < 0)), "the grid has more than one local maximum"
    return float(grid[int(np.argmax(vals))]), vals


# ------------------------------------------------------------------------------------- the cases the suites share
# rows of five individuals: the seed whose rows keep every relative pivot above 1e-3 (cols_compared asserts it)
SOFT_SEEDS = {5: 2}


def cols_case(n, T, P, nx, ne, kind, scaled, M=84, seed=11):
    """(reg[n][M][ne], x0[n][nx], pheno[n][T], scale or None, perm or None)"""
    if kind == "soft":
        origin, _ = soft_rows(n, CHROM_LENS, SOFT_SEEDS.get(n, seed + n))
        reg = ad_columns(origin, ne == 1)[:, :M]
    else:
        reg = gaussian_like(n, M, ne, seed + n)
    x0 = np.concatenate([np.ones((n, 1)), synth.uniform(seed * 16 + 9, np.arange(n * 8)).reshape(n, 8) * 2.0 - 1.0], axis=1)[:, :nx]
    scale = 0.5 + synth.uniform(seed * 16 + 10, np.arange(n)) if scaled else None
    s = np.ones(n) if scale is None else scale
    at = [(7 * t + 3) % M for t in range(T)]
    pheno = 0.8 * s[:, None] * reg[:, at, 0] + 0.4 * s[:, None] * reg[:, at, ne - 1] + noise(n, T, seed) + 0.3 * x0[:, :1]
    perm = qtl.permutations(n, P, seed) if P else None
    return reg, x0, pheno, scale, perm


CS = chromstarts_of(CHROM_LENS)


def lmm_inputs(n, seed, K_cov=1):
    origin, _ = soft_rows(n, CHROM_LENS, seed)
    K = kinship_ref(origin, CS)
    reg = ad_columns(origin)
    X0 = np.ones((n, 1))
    if K_cov:
        z = synth.uniform(seed * 16 + 9, np.arange(n * K_cov)).reshape(n, K_cov)
        X0 = np.concatenate([X0, z - z.mean(axis=0)], axis=1)
    (g,), _ = chol_whiten(K, 0.5, noise(n, 1, seed + 1)[:, 0])
    y = 0.7 * reg[:, 20, 0] + 2.0 * (K @ g) + noise(n, 1, seed + 2)[:, 0]
    return origin, K, reg, X0, y - y.mean()
