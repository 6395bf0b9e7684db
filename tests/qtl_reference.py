"""The yardstick of the QTL scan's tests (tests/test_qtl_host.py, tests/test_gpu_qtl.py): hand-made origin rows and a
per-marker least-squares fit in numpy -- np.linalg.lstsq on the explicit design, one chromosome and marker at a time, the
rows of individuals with c_i = 0 deleted.  It shares nothing with the product's Schur form (cnf2freq_amd/csrc/cnf2_qtl.h).

The rank and the relative pivots that decide which coefficients are compared come from a third route, the residuals of a
and d after projection on the null design."""
import numpy as np

from cnf2freq_amd import synth

ATOL = 1e-9              # the project's bar for f64 results: absolute on lod, relative to max(1, |coef|) on coef
PIVOT_DROP = 1e-8        # the model's rank rule (include/cnf2hip.h)
PIVOT_WELL = 1e-3        # coefficients are compared where every kept relative pivot is at least this
PIVOT_EXACT = 1e-12      # ... and a dropped column must be degenerate by construction: relative pivot at most this
CLAMP = 1.0 - 2.0 ** -52

CHROM_LENS = (1, 2, 15, 16, 17, 33)      # every tile edge of 16 markers, and a chromosome start inside every would-be tile


def chromstarts_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def soft_rows(n, lens, seed, switch=0.15, floor=0.45):
    """origin[n][M][4]: soft one-hot rows.  Per individual and chromosome two gametes, each a two-state Markov chain along
    the markers (a switch with probability `switch` per gap); the true class is k = g1 + 2 g2 and the row puts a weight of
    floor .. 1 on it and spreads the rest over the other three in random shares (the spread of the weights keeps a and d of
    a handful of individuals from lying in one plane with the intercept where only two of the three genotypes occur).  Returns (origin, true class [n][M])."""
    cs = chromstarts_of(lens)
    M = int(cs[-1])
    u = lambda stream, shape: synth.uniform(seed * 16 + stream, np.arange(int(np.prod(shape)))).reshape(shape)
    g = np.zeros((2, n, M), np.int64)
    start, flip = u(0, (2, n, M)) < 0.5, u(1, (2, n, M)) < switch
    for c in range(len(lens)):
        for m in range(cs[c], cs[c + 1]):
            g[:, :, m] = start[:, :, m] if m == cs[c] else g[:, :, m - 1] ^ flip[:, :, m]
    k = g[0] + 2 * g[1]
    w = floor + (1.0 - floor) * u(2, (n, M))
    share = 0.05 + u(3, (n, M, 4))
    share[np.arange(n)[:, None], np.arange(M)[None, :], k] = 0.0
    share *= ((1.0 - w) / share.sum(axis=2))[:, :, None]
    share[np.arange(n)[:, None], np.arange(M)[None, :], k] = w
    return share, k


def skip(origin, individuals, chrom, lens):
    """the rows of `individuals` on chromosome `chrom` set to zero: skipped there, as the origin sweep reports it"""
    cs = chromstarts_of(lens)
    o = origin.copy()
    o[np.asarray(individuals), cs[chrom]:cs[chrom + 1]] = 0.0
    return o


def noise(n, T, seed):
    return synth.uniform(seed * 16 + 7, np.arange(n * T)).reshape(n, T) - 0.5


def columns(pheno, perm):
    """Y[n][1 + P][T]: the observed phenotypes and the permuted ones, pheno[perm[p][i]] at individual i"""
    y = np.asarray(pheno, np.float64)
    blocks = [y] + ([] if perm is None else [y[np.asarray(p)] for p in perm])
    return np.stack(blocks, axis=1)


def reference_scan(origin, chromstarts, pheno, use=None, cov=None, perm=None, additive=False):
    """The model of include/cnf2hip.h by least squares.  A dict: lod[1 + P][T][M] (block 0 observed), coef[T][M][2] of the
    observed columns, rank[M], relpivot[M][2] (NaN for a raw diagonal of 0), usable[C], n_used[C], rss0[T][C],
    perm_max[P][T][C]."""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    cs = np.asarray(chromstarts, np.int64)
    C = len(cs) - 1
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    X0all = np.ones((n, 1)) if cov is None else np.concatenate([np.ones((n, 1)), np.asarray(cov, np.float64).reshape(n, -1)], axis=1)
    nx = X0all.shape[1]
    Y = columns(np.where(use[:, None], pheno, 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    lod = np.zeros((Q, T, M))
    coef = np.full((T, M, 2), np.nan)
    rank = np.zeros(M, np.int32)
    relpivot = np.full((M, 2), np.nan)
    usable = np.zeros(C, bool)
    n_used = np.zeros(C, np.int32)
    rss0_out = np.zeros((T, C))
    for c in range(C):
        keep = use & (o[:, cs[c]] != 0.0).any(axis=1)
        n_c = int(keep.sum())
        n_used[c] = n_c
        X0 = X0all[keep]
        y = Y[keep].reshape(n_c, Q * T)
        usable[c] = n_c >= nx + 3 and np.linalg.matrix_rank(X0) == nx
        if not usable[c]:
            continue
        r0 = y - X0 @ np.linalg.lstsq(X0, y, rcond=None)[0]
        rss0 = (r0 ** 2).sum(axis=0)
        rss0_out[:, c] = rss0[:T]
        for m in range(cs[c], cs[c + 1]):
            a = o[keep, m, 3] - o[keep, m, 0]
            d = o[keep, m, 1] + o[keep, m, 2]
            ra = a - X0 @ np.linalg.lstsq(X0, a, rcond=None)[0]
            rd = d - X0 @ np.linalg.lstsq(X0, d, rcond=None)[0]
            saa, sdd = a @ a, d @ d
            keep_a = saa > 0 and ra @ ra >= PIVOT_DROP * saa
            pd = rd @ rd - ((ra @ rd) ** 2 / (ra @ ra) if keep_a else 0.0)
            keep_d = (not additive) and sdd > 0 and pd >= PIVOT_DROP * sdd
            rank[m] = int(keep_a) + int(keep_d)
            relpivot[m] = [ra @ ra / saa if saa > 0 else np.nan, pd / sdd if sdd > 0 else np.nan]
            X = np.column_stack([X0, a] if additive else [X0, a, d])
            beta = np.linalg.lstsq(X, y, rcond=None)[0]
            rss1 = ((y - X @ beta) ** 2).sum(axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                drss = np.clip(rss0 - rss1, 0.0, rss0 * CLAMP)
                l = np.where(rss0 > 0, 0.5 * n_c * np.log10(rss0 / (rss0 - drss)), 0.0)
            lod[:, :, m] = l.reshape(Q, T)
            if rank[m] == (1 if additive else 2):
                coef[:, m, 0] = beta[nx, :T]
                if not additive:
                    coef[:, m, 1] = beta[nx + 1, :T]
    perm_max = np.zeros((Q - 1, T, C))
    for c in range(C):
        perm_max[:, :, c] = lod[1:, :, cs[c]:cs[c + 1]].max(axis=2)
    return dict(lod=lod, coef=coef, rank=rank, relpivot=relpivot, usable=usable, n_used=n_used, rss0=rss0_out,
                perm_max=perm_max)


def compared_markers(ref, chromstarts, additive=False, share=0.9):
    """compared[M]: the markers whose coefficients are compared -- full rank (2, or 1 in the additive model) with every kept
    relative pivot at least PIVOT_WELL.  Asserts what the comparison rests on: every marker of a usable chromosome is
    either that well conditioned or exactly degenerate (a dropped column has relative pivot at most PIVOT_EXACT or a raw
    diagonal of 0), and at least `share` of all markers are compared."""
    cs = np.asarray(chromstarts, np.int64)
    rp = ref["relpivot"]
    cols = [0] if additive else [0, 1]
    well = np.all(np.nan_to_num(rp[:, cols], nan=0.0) >= PIVOT_WELL, axis=1)
    exact = np.all(np.isnan(rp[:, cols]) | (rp[:, cols] >= PIVOT_WELL) | (rp[:, cols] <= PIVOT_EXACT), axis=1)
    on = np.repeat(ref["usable"], np.diff(cs))
    assert np.all(exact[on]), "a marker is neither well conditioned nor exactly degenerate: relative pivots %s" % rp[on & ~exact]
    compared = on & well & (ref["rank"] == len(cols))
    if share:
        assert compared.mean() >= share, "only %.0f %% of the markers have compared coefficients" % (100 * compared.mean())
    return compared


def compare(got, ref, chromstarts, additive=False, what="", share=0.9):
    """lod at every cell, coef at the compared markers (and NaN exactly where the rank drops a column), rank, n_used, rss0,
    perm_max; prints every figure before it asserts"""
    compared = compared_markers(ref, chromstarts, additive, share)
    err_l = np.abs(got["lod"] - ref["lod"][0]).max()
    gc, rc = got["coef"][:, compared], ref["coef"][:, compared]
    if additive:
        assert np.isnan(got["coef"][:, :, 1]).all(), "the additive model reports no dominance effect"
        gc, rc = gc[:, :, 0], rc[:, :, 0]
    err_c = (np.abs(gc - rc) / np.maximum(1.0, np.abs(rc))).max() if gc.size else 0.0
    err_r = np.abs(got["rss0"] - ref["rss0"]).max()
    print("%s: lod %.3g over %d cells, coef %.3g over %d of %d markers, rss0 %.3g" %
          (what, err_l, got["lod"].size, err_c, compared.sum(), len(compared), err_r))
    assert np.array_equal(got["rank"], ref["rank"]), what + " rank"
    assert np.array_equal(got["n_used"], ref["n_used"]), what + " n_used"
    assert err_l <= ATOL, what + " lod"
    assert err_c <= ATOL, what + " coef"
    assert err_r <= ATOL * max(1.0, np.abs(ref["rss0"]).max()), what + " rss0"
    assert np.all(got["lod"] >= 0) and np.isfinite(got["lod"]).all()
    drop_a, drop_d = got["rank"] == 0, (got["rank"] < 2) if not additive else np.ones_like(got["rank"], bool)
    on = np.repeat(ref["usable"], np.diff(np.asarray(chromstarts, np.int64)))
    well_rank1 = on & (got["rank"] == 1) & ~compared & (not additive)
    # a rank-1 marker of the full model keeps a or d: the kept one is a number, the other NaN
    assert np.isnan(got["coef"][:, drop_a & drop_d]).all()
    assert (np.isnan(got["coef"][:, well_rank1]).sum(axis=2) == 1).all()
    if ref["perm_max"].shape[0]:
        err_p = np.abs(got["perm_max"] - ref["perm_max"]).max()
        print("%s: perm_max %.3g over %d cells" % (what, err_p, ref["perm_max"].size))
        assert err_p <= ATOL, what + " perm_max"
    return compared
