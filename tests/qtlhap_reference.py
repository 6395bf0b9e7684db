"""The reference of the founder-haplotype scan (cnf2_qtl_scan_hap), shared by the CPU and the GPU suite: per marker the explicit
dense design -- the intercept, the covariates and Z[i][h] = sum_k [col[i][k] == h] descent[i][m][k] -- on the rows with c_i = 1,
fitted by numpy.linalg.lstsq.  The kept set comes from sequential residuals: column h is regressed on the null design and the
columns kept before it, and its relative pivot is |residual|^2 / |column|^2; it is kept at 1e-8 and above, as the definition
says (include/cnf2hip.h).  A marker is INSIDE THE CONDITIONING RULE when every kept relative pivot is >= 1e-3 and every
dropped one is <= 1e-12: only there do two factorisations agree on the coefficients to the project's bar, and only there
are coefficients compared -- asserted on the reference before the code under test runs."""
import numpy as np

PIVOT = 1e-8
KEPT_MIN, DROPPED_MAX = 1e-3, 1e-12


def design(descent_m, col, H):
    """Z[n][H] of one marker from its rows descent_m[n][8]; a cell with col < 0 adds nothing"""
    d, col = np.asarray(descent_m, np.float64), np.asarray(col)
    Z = np.zeros((d.shape[0], H))
    for k in range(8):
        ok = col[:, k] >= 0
        np.add.at(Z, (np.flatnonzero(ok), col[ok, k]), d[ok, k])
    return Z


def in_model(col, H, use=None):
    col = np.asarray(col)
    m = ((col >= 0) & (col < H)).all(axis=1)
    return m if use is None else m & (np.asarray(use) != 0)


def refined_lstsq(X, y):
    """numpy.linalg.lstsq with two steps of iterative refinement, the residual formed in extended precision.  Founder-allele
    effects are contrasts between columns that nearly add up to the intercept: they reach 1e3 and more at a well-conditioned
    marker, and a plain lstsq carries its relative error of 1e-12 into them -- above the bar the comparison is held to
    (measured against 40-digit arithmetic: 2.3e-9 for the plain solve, 3e-12 with refinement)."""
    beta = np.linalg.lstsq(X, y, rcond=None)[0]
    Xl, yl = X.astype(np.longdouble), y.astype(np.longdouble)
    for _ in range(2):
        r = (yl - Xl @ beta.astype(np.longdouble)).astype(np.float64)
        beta = beta + np.linalg.lstsq(X, r, rcond=None)[0]
    return beta


def marker(descent_m, col, H, y, cov=None, c=None):
    """One marker: dict(lod[T], df, coef[T][H], rss0[T], n_used, kept[H] bool, pivots[H] relative, inside bool)"""
    y = np.asarray(y, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    rows = in_model(col, H, c)
    n_c = int(rows.sum())
    K = 0 if cov is None else np.asarray(cov).reshape(n, -1).shape[1]
    X0 = np.ones((n_c, 1)) if K == 0 else np.concatenate([np.ones((n_c, 1)), np.asarray(cov, np.float64).reshape(n, -1)[rows]], axis=1)
    Z = design(np.asarray(descent_m)[rows], np.asarray(col)[rows], H)
    yu = y[rows]
    out = dict(lod=np.zeros(T), df=0, coef=np.full((T, H), np.nan), rss0=np.zeros(T), n_used=n_c, kept=np.zeros(H, bool),
               pivots=np.zeros(H), inside=False)
    scanned = n_c >= K + 4 and np.linalg.matrix_rank(X0) == K + 1
    if not scanned:
        return out
    res0 = yu - X0 @ np.linalg.lstsq(X0, yu, rcond=None)[0]
    out["rss0"] = (res0 ** 2).sum(axis=0)
    basis = X0
    for h in range(H):
        z = Z[:, h]
        raw = float(z @ z)
        if raw > 0:
            r = z - basis @ np.linalg.lstsq(basis, z, rcond=None)[0]
            out["pivots"][h] = float(r @ r) / raw
            if out["pivots"][h] >= PIVOT:
                out["kept"][h] = True
                basis = np.concatenate([basis, z[:, None]], axis=1)
    kept = out["kept"]
    out["inside"] = bool((out["pivots"][kept] >= KEPT_MIN).all() and (out["pivots"][~kept] <= DROPPED_MAX).all())
    df = int(kept.sum())
    if n_c - 1 - K - df < 1:
        out["kept"][:] = False
        return out
    out["df"] = df
    beta = refined_lstsq(basis, yu)
    rss1 = ((yu - basis @ beta) ** 2).sum(axis=0)
    out["coef"][:, kept] = beta[K + 1:].T
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.clip(out["rss0"] - rss1, 0.0, out["rss0"] * (1.0 - 2.0 ** -52))
        out["lod"] = np.where((out["rss0"] > 0) & (d > 0), 0.5 * n_c * np.log10(out["rss0"] / (out["rss0"] - d)), 0.0)
    return out


def scan(descent, col, H, y, chromstarts, cov=None, use=None):
    """The whole map: dict(lod[T][M], df[M], coef[T][M][H], rss0[T][C], n_used[C], inside[M], pivots[M][H], kept[M][H])"""
    d = np.asarray(descent, np.float64)
    y = np.asarray(y, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, M = d.shape[:2]
    T = y.shape[1]
    cs = np.asarray(chromstarts)
    C = len(cs) - 1
    base = in_model(col, H, use)
    out = dict(lod=np.zeros((T, M)), df=np.zeros(M, np.int32), coef=np.full((T, M, H), np.nan), rss0=np.zeros((T, C)),
               n_used=np.zeros(C, np.int32), inside=np.zeros(M, bool), pivots=np.zeros((M, H)), kept=np.zeros((M, H), bool))
    for c in range(C):
        cm = base & (d[:, cs[c]] != 0).any(axis=1)
        out["n_used"][c] = cm.sum()
        for m in range(cs[c], cs[c + 1]):
            r = marker(d[:, m], col, H, y, cov, cm)
            out["lod"][:, m], out["df"][m], out["coef"][:, m] = r["lod"], r["df"], r["coef"]
            out["inside"][m], out["pivots"][m], out["kept"][m] = r["inside"], r["pivots"], r["kept"]
            out["rss0"][:, c] = r["rss0"]
    return out


def exact_phenotypes(n, T, seed, use=None):
    """y[n][T], multiples of 2^-8 that add up to 0 over the used individuals: their mean is exactly 0 and every permutation of
    them within the used individuals has the same sums to the bit"""
    rng = np.random.default_rng(seed)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    y = np.round(rng.normal(size=(n, T)) * 256.0)
    idx = np.flatnonzero(use)
    y[idx[-1]] -= y[idx].sum(axis=0)
    return y / 256.0
