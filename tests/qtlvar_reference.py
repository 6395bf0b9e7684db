"""The yardstick of the variance-QTL scan's tests (tests/test_qtlvar_host.py, tests/test_gpu_qtlvar.py,
tests/test_gpu_qtlvar_invariance.py): the double generalised linear model of include/cnf2hip.h per marker and column in
numpy, from the definition, by a route that shares nothing with the product's packed Cholesky form
(cnf2freq_amd/csrc/cnf2_qtlvar.h).  The designs X and V are explicit matrices, with the rows of individuals with c_i = 0
deleted and the trait and the covariates as given (not centred: both designs hold an intercept); the two solves are
np.linalg.solve.  Which effects a marker keeps comes from qtlx_reference's sequential pivots.

Per fit the yardstick keeps the trace of iterates, the smallest relative pivot of both weighted factors over the steps, the
largest |eta| and `near`: a deciding gain within NEAR_TOL relative of tol, or a trial step's loss within NEAR_LOSS relative
of LOSS.  Independent of the stopping rule, `anchor` maximises the same likelihood in longdouble without a stopping rule and
with an elimination of its own; the converged yardstick must agree with it (assert_anchor)."""
import numpy as np

from qtl_reference import ATOL, CHROM_LENS, PIVOT_DROP, PIVOT_EXACT, PIVOT_WELL, chromstarts_of, columns, noise, reference_scan, skip, soft_rows  # noqa: F401
from qtlx_reference import certain_rows, effects, reference_scanx  # noqa: F401
from qtlem_reference import CODES  # noqa: F401
from qtlbin_reference import solve_ld

LN10 = np.log(10.0)
LOG2PI = np.log(2.0 * np.pi)
NULL_ITER, NULL_TOL = 50, 1e-13
HALVINGS, LOSS, ETA_LIMIT = 8, 1e-9, 700.0
ETA_MAX = 50.0           # cells whose log variances stay within this are compared
NEAR_TOL = 1e-6          # relative to tol
NEAR_LOSS = 1e-3         # relative to LOSS
FITS = ("mean-only", "variance-only", "full")


def loglik(X, V, y, beta, gamma):
    """l(beta, gamma) and the largest |eta|"""
    eta = V @ gamma
    r = y - X @ beta
    with np.errstate(over="ignore", invalid="ignore"):
        ll = -0.5 * float((LOG2PI + eta + r * r * np.exp(-eta)).sum())
    return ll, float(np.abs(eta).max()) if len(eta) else 0.0


def relpivot(G):
    """the smallest pivot of G's Cholesky factor relative to its diagonal entry; raises LinAlgError without a factor"""
    L = np.linalg.cholesky(G)
    return float((np.diag(L) ** 2 / np.diag(G)).min())


def dglm(X, V, y, beta, gamma, ll_start, max_iter, tol):
    """The iteration of include/cnf2hip.h from (beta, gamma), whose log-likelihood is ll_start.  A dict: ll (the trace
    l_0 .. l_t), beta, gamma, iters, status, near, halvings (the most of a step), relpivot (the smallest of both factors over
    the steps), maxeta."""
    beta, gamma = np.array(beta, np.float64), np.array(gamma, np.float64)
    trace, t, near, most_h, rp, maxeta = [float(ll_start)], 0, False, 0, 1.0, float(np.abs(V @ gamma).max())
    while True:
        ll = trace[-1]
        with np.errstate(all="ignore"):
            w = np.exp(-(V @ gamma))
            G = X.T @ (X * w[:, None])
            try:
                rp = min(rp, relpivot(G))
                b1 = np.linalg.solve(G, X.T @ (w * y))
                r = y - X @ b1
                q = w * r * r
                H = V.T @ (V * q[:, None])
                rp = min(rp, relpivot(H))
                delta = np.linalg.solve(H, V.T @ (q - 1.0))
            except np.linalg.LinAlgError:
                status = 2
                break
        if not (np.isfinite(b1).all() and np.isfinite(gamma + delta).all()):
            status = 2
            break
        taken = None
        for h in range(HALVINGS + 1):
            g1 = gamma + delta / 2.0 ** h
            l1, me = loglik(X, V, y, b1, g1)
            if not np.isfinite(l1) or me > ETA_LIMIT:
                break
            loss = (ll - l1) / LN10
            near = near or abs(loss - LOSS) <= NEAR_LOSS * LOSS
            if loss <= LOSS:
                taken = h
                break
        if taken is None:
            status = 2
            break
        most_h, maxeta = max(most_h, taken), max(maxeta, me)
        gain = (l1 - ll) / LN10
        near = near or abs(gain - tol) <= NEAR_TOL * abs(tol)
        beta, gamma, t = b1, g1, t + 1
        trace.append(l1)
        if gain < tol:
            status = 0
            break
        if t >= max_iter:
            status = 1
            break
    return dict(ll=np.array(trace), beta=beta, gamma=gamma, iters=t, status=status, near=near, halvings=most_h, relpivot=rp,
                maxeta=maxeta)


def null_fit(X0, V0, y, centre):
    """the null fit of a column on (X0, V0), or None where the column is not scanned; `centre` is the trait's mean over the
    used individuals, which the model's start beta = 0 refers to"""
    if not y.min() < y.max():
        return None
    g = np.zeros(V0.shape[1])
    yc = y - centre
    g[0] = np.log((yc * yc).sum() / len(y))
    b = np.zeros(X0.shape[1])
    b[0] = centre
    f = dglm(X0, V0, y, b, g, loglik(X0, V0, y, b, g)[0], NULL_ITER, NULL_TOL)
    if f["status"] != 0 or f["iters"] < 1:
        return None
    return f


def anchor(X, V, y, rounds=200):
    """the maximum of l over (beta, gamma) in longdouble: `rounds` alternations of the exact beta and a Newton step in gamma
    halved until l does not fall, from the homoscedastic fit; no start from the null fit, no stopping rule, no double solver"""
    X, V, y = (np.array(a, np.longdouble) for a in (X, V, y))
    ld = lambda g, b: -0.5 * (np.longdouble(LOG2PI) + V @ g + (y - X @ b) ** 2 * np.exp(-(V @ g))).sum()
    gamma = np.zeros(V.shape[1], np.longdouble)
    beta = solve_ld(X.T @ X, X.T @ y)
    gamma[0] = np.log(((y - X @ beta) ** 2).mean())
    for _ in range(rounds):
        w = np.exp(-(V @ gamma))
        beta = solve_ld(X.T @ (X * w[:, None]), X.T @ (w * y))
        q = w * (y - X @ beta) ** 2
        delta = solve_ld(V.T @ (V * q[:, None]), V.T @ (q - 1))
        l0, s = ld(gamma, beta), np.longdouble(1.0)
        while s > 1e-6 and not ld(gamma + s * delta, beta) >= l0:
            s /= 2
        if s > 1e-6:
            gamma = gamma + s * delta
    return float(ld(gamma, beta))


def threshold(K, n_var, ne):
    """the fewest individuals of a scanned chromosome"""
    return (1 + K + ne) + (1 + n_var + ne) + 1


def reference_scan_var(origin, chromstarts, pheno, use=None, cov=None, n_var=0, imprint=False, perm=None, additive=False,
                       max_iter=50, tol=1e-7, anchor_every=0):
    """The model of include/cnf2hip.h.  A dict: lod[1 + P][T][M][3] (block 0 observed), ll[T][M][3] the fits' l, trace[T][M]
    [max_iter + 1] of the observed columns' joint LOD after every iteration of the full fit (the last value repeated),
    coef_mean and coef_var[T][M][ne], iters, status, near, halvings[T][M][3], minpivot and maxeta[T][M] (over the three fits),
    rank[M], relpivot[M][ne], usable[C], n_used[C], ll0[T][C], null_iters[T][C], perm_max[P][T][C][3]; with anchor_every =
    k > 0 also anchor_err, the largest |l - anchor's l| / ln 10 over the fits of the observed cells of every k-th marker that
    stopped by tol."""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    cs = np.asarray(chromstarts, np.int64)
    C = len(cs) - 1
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    Z = np.zeros((n, 0)) if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    K = Z.shape[1]
    X0all = np.concatenate([np.ones((n, 1)), Z], axis=1)
    V0all = X0all[:, :1 + n_var]
    eff = effects(additive, imprint)
    ne = len(eff)
    yy = np.where(use[:, None], np.nan_to_num(np.asarray(pheno, np.float64).reshape(n, -1)), 0.0)
    hk = reference_scanx(o, cs, yy[:, :1], use, cov, 0, imprint, None, additive)
    usable = hk["usable"] & (hk["n_used"] >= threshold(K, n_var, ne))
    Y = columns(yy, perm)
    Q, T = Y.shape[1], Y.shape[2]
    lod = np.zeros((Q, T, M, 3))
    ll = np.zeros((T, M, 3))
    trace = np.zeros((T, M, max_iter + 1))
    coef_mean, coef_var = np.full((T, M, ne), np.nan), np.full((T, M, ne), np.nan)
    iters, status = np.zeros((T, M, 3), np.int32), np.zeros((T, M, 3), np.int32)
    near, halvings = np.zeros((T, M, 3), bool), np.zeros((T, M, 3), np.int32)
    minpivot, maxeta = np.ones((T, M)), np.zeros((T, M))
    rank = np.zeros(M, np.int32)
    ll0_out, null_iters = np.zeros((T, C)), np.zeros((T, C), np.int32)
    anchor_err = 0.0
    for c in range(C):
        if not usable[c]:
            continue
        keep = use & (o[:, cs[c]] != 0.0).any(axis=1)
        X0, V0 = X0all[keep], V0all[keep]
        nulls = [[null_fit(X0, V0, Y[keep, qq, t], Y[use, qq, t].mean()) for t in range(T)] for qq in range(Q)]
        for t in range(T):
            if nulls[0][t] is not None:
                ll0_out[t, c], null_iters[t, c] = nulls[0][t]["ll"][-1], nulls[0][t]["iters"]
        for m in range(cs[c], cs[c + 1]):
            kept = np.nan_to_num(hk["relpivot"][m], nan=0.0) >= PIVOT_DROP
            rank[m] = int(kept.sum())
            assert rank[m] == hk["rank"][m][1]
            if rank[m] == 0:
                continue
            om = o[keep, m]
            val = dict(a=om[:, 3] - om[:, 0], d=om[:, 1] + om[:, 2], i=om[:, 1] - om[:, 2])
            E = np.column_stack([val[e] for e, k in zip(eff, kept) if k])
            designs = [(np.column_stack([X0, E]), V0), (X0, np.column_stack([V0, E])),
                       (np.column_stack([X0, E]), np.column_stack([V0, E]))]
            for qq in range(Q):
                for t in range(T):
                    f0 = nulls[qq][t]
                    if f0 is None:
                        continue
                    y, l0 = Y[keep, qq, t], f0["ll"][-1]
                    fits = []
                    for X, V in designs:
                        b = np.concatenate([f0["beta"], np.zeros(X.shape[1] - X0.shape[1])])
                        g = np.concatenate([f0["gamma"], np.zeros(V.shape[1] - V0.shape[1])])
                        fits.append(dglm(X, V, y, b, g, l0, max_iter, tol))
                    lf = [f["ll"][-1] for f in fits]
                    lod[qq, t, m] = np.maximum(0.0, np.array([lf[2] - l0, lf[2] - lf[1], lf[2] - lf[0]]) / LN10)
                    if qq:
                        continue
                    ll[t, m] = lf
                    tr = np.maximum(0.0, (fits[2]["ll"] - l0) / LN10)
                    trace[t, m, :len(tr)] = tr
                    trace[t, m, len(tr):] = tr[-1]
                    coef_mean[t, m, kept] = fits[2]["beta"][X0.shape[1]:]
                    coef_var[t, m, kept] = fits[2]["gamma"][V0.shape[1]:]
                    for k, f in enumerate(fits):
                        iters[t, m, k], status[t, m, k], near[t, m, k], halvings[t, m, k] = f["iters"], f["status"], f["near"], f["halvings"]
                    minpivot[t, m] = min(f["relpivot"] for f in fits)
                    maxeta[t, m] = max(f["maxeta"] for f in fits)
                    if anchor_every and m % anchor_every == 0:
                        for f, (X, V) in zip(fits, designs):
                            if f["status"] == 0 and f["maxeta"] <= ETA_MAX:
                                anchor_err = max(anchor_err, abs(f["ll"][-1] - anchor(X, V, y)) / LN10)
    perm_max = np.zeros((Q - 1, T, C, 3))
    for c in range(C):
        perm_max[:, :, c] = lod[1:, :, cs[c]:cs[c + 1]].max(axis=2)
    return dict(lod=lod, ll=ll, trace=trace, coef_mean=coef_mean, coef_var=coef_var, iters=iters, status=status, near=near,
                halvings=halvings, minpivot=minpivot, maxeta=maxeta, rank=rank, relpivot=hk["relpivot"], usable=usable,
                n_used=hk["n_used"], ll0=ll0_out, null_iters=null_iters, perm_max=perm_max, anchor_err=anchor_err)


def compared_cells(ref, chromstarts, share=0.99, strict=True):
    """compared[T][M]: the cells of markers whose every effect is either well conditioned (relative pivot at least PIVOT_WELL)
    or exactly degenerate (at most PIVOT_EXACT, or a raw diagonal of 0), or whose chromosome is not scanned; whose weighted
    factors kept every relative pivot at PIVOT_WELL or above; and whose log variances stayed within ETA_MAX."""
    cs = np.asarray(chromstarts, np.int64)
    rp = ref["relpivot"]
    fine = np.all(np.isnan(rp) | (rp >= PIVOT_WELL) | (rp <= PIVOT_EXACT), axis=1)
    on = np.repeat(ref["usable"], np.diff(cs))
    assert not strict or np.all(fine[on]), "a marker is neither well conditioned nor exactly degenerate: relative pivots %s" % rp[on & ~fine]
    cells = (fine | ~on)[None, :] & (ref["maxeta"] <= ETA_MAX) & (ref["minpivot"] >= PIVOT_WELL)
    if share:
        assert cells.mean() >= share, "only %.0f %% of the cells are compared" % (100 * cells.mean())
    return cells


def compare_var(got, ref, chromstarts, what="", share=0.99, strict=True, iters=True):
    """every output of a scan against the reference at the compared cells: lod and ll0 within ATOL, the coefficients relative
    to max(1, |coef|) (NaN exactly where the reference has none), perm_max within ATOL; rank (at markers with a compared
    cell), n_used and, outside ref["near"], status and iters with ==.  Prints every figure before it asserts; returns the
    errors."""
    cc = compared_cells(ref, chromstarts, share, strict)
    cm = cc.any(axis=0)
    err_l = np.abs(got["lod"] - ref["lod"][0])[cc].max()
    err_c = 0.0
    for key in ("coef_mean", "coef_var"):
        gc, rc = got[key][cc], ref[key][cc]
        assert np.array_equal(np.isnan(gc), np.isnan(rc)), what + ": a dropped effect is NaN, a kept one a number (" + key + ")"
        both = ~np.isnan(rc)
        if both.any():
            err_c = max(err_c, (np.abs(gc[both] - rc[both]) / np.maximum(1.0, np.abs(rc[both]))).max())
    err_0 = np.abs(got["ll0"] - ref["ll0"]).max()
    print("%s: lod %.3g over %d of %d cells, coef %.3g, ll0 %.3g, iterations up to %d, halvings up to %d, near %d, largest |eta| %.3g, "
          "smallest pivot %.3g" % (what, err_l, cc.sum(), cc.size, err_c, err_0, ref["iters"].max(), ref["halvings"].max(),
                                   ref["near"].sum(), ref["maxeta"].max(), ref["minpivot"].min()))
    assert np.array_equal(got["rank"][cm], ref["rank"][cm]), what + " rank"
    assert np.array_equal(got["n_used"], ref["n_used"]), what + " n_used"
    assert err_l <= ATOL, what + " lod"
    assert err_c <= ATOL, what + " coef"
    assert err_0 <= ATOL, what + " ll0"
    assert np.array_equal(got["ll0"] == 0.0, ref["ll0"] == 0.0), what + " ll0 is 0 where nothing is scanned"
    assert np.isfinite(got["lod"]).all() and np.all(got["lod"] >= 0), what + " lod is finite and not negative"
    off = ~np.repeat(ref["usable"], np.diff(np.asarray(chromstarts, np.int64)))
    assert np.all(got["lod"][:, off] == 0.0) and np.isnan(got["coef_mean"][:, off]).all() and np.isnan(got["coef_var"][:, off]).all()
    assert np.all(got["rank"][off] == 0)
    zero = got["rank"] == 0
    assert np.all(got["lod"][:, zero] == 0.0) and np.all(got["iters"][:, zero] == 0) and np.all(got["status"][:, zero] == 0)
    if iters:
        ok = cc[..., None] & ~ref["near"]
        assert np.array_equal(got["status"][ok], ref["status"][ok]), what + " status"
        assert np.array_equal(got["iters"][ok], ref["iters"][ok]), what + " iters"
    err_p = 0.0
    if ref["perm_max"].shape[0]:
        err_p = np.abs(got["perm_max"] - ref["perm_max"]).max()
        print("%s: perm_max %.3g over %d cells" % (what, err_p, ref["perm_max"].size))
        assert err_p <= ATOL, what + " perm_max"
    else:
        assert got.get("perm_max") is None
    return dict(lod=err_l, coef=err_c, ll0=err_0, perm_max=err_p)


# ------------------------------------------------------------------------------------------------ the cases of the issue
# fixed iterations (tol = -1): every K + 1 instance, every n_var, every design; the n decide the lane walk of 64
#         n    K  n_var imprint additive seed T  P  mask   skipped max_iter
CASES = [(41, 2, 0, False, False, 3, 1, 0, False, False, 4),      # less than one round; (a, d)
         (41, 2, 1, True, False, 5, 1, 1, False, False, 3),       # (a, d, i)
         (63, 3, 3, True, True, 21, 1, 1, False, False, 3),       # one short of a round; (a, i)
         (64, 0, 0, False, False, 4, 1, 1, False, False, 3),      # exactly one round, no covariates
         (65, 4, 2, False, False, 22, 1, 1, False, False, 3),     # one past a round
         (67, 2, 2, True, False, 7, 1, 1, False, True, 3),        # individuals 1 and 4 skipped on chromosome 3
         (96, 5, 1, True, False, 23, 1, 0, False, False, 3),      # 1.5 rounds
         (127, 6, 0, False, True, 24, 1, 1, True, False, 3),      # (a), with a `use` mask
         (129, 7, 3, True, True, 25, 1, 0, False, False, 3),      # one past two rounds; (a, i)
         (130, 8, 3, True, False, 9, 2, 5, False, False, 3)]      # three rounds, the widest designs, T = 2, P = 5


def case_id(c):
    return "n%d-K%d-v%d-%s%s-T%d-P%d-it%d%s" % (c[0], c[1], c[2], "i" if c[3] else "m", "-add" if c[4] else "", c[6], c[7], c[10],
                                                "-mask" if c[8] else "-skip" if c[9] else "")


def gauss(shape, seed):
    """standard normal draws by Box and Muller from synth.uniform"""
    from cnf2freq_amd import synth
    k = int(np.prod(shape))
    u1 = synth.uniform(seed * 16 + 12, np.arange(k))
    u2 = synth.uniform(seed * 16 + 13, np.arange(k))
    return (np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)).reshape(shape)


def student4(shape, seed):
    """t(4) draws: a normal over the root of a chi-square with 4 degrees of freedom over 4"""
    z = gauss(tuple(shape) + (5,), seed)
    return z[..., 0] / np.sqrt((z[..., 1:] ** 2).sum(axis=-1) / 4.0)


def make_case(n, K, n_var, imprint, additive, seed, T, P, mask, skipped, max_iter=None):
    """(origin, pheno, cov, use, perm) on the map CHROM_LENS: rows soft_rows(n, CHROM_LENS, seed), covariates
    noise(n, K, seed + 1), normal phenotypes with a mean and a log-variance effect of the true classes and of the first
    covariate.  With `mask` two individuals are unused and carry NaN phenotypes and covariates; with `skipped` individuals 1
    and 4 are skipped on chromosome 3."""
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
    mu = 0.2 + 0.5 * a[:, at] + 0.3 * d[:, to]
    eta = 0.6 * a[:, to] - 0.4 * im[:, at]
    if K:
        mu = mu + 1.0 * cov[:, :1]
        eta = eta + 0.8 * cov[:, :1]
        cov = np.where(use[:, None], cov, np.nan)
    pheno = np.where(use[:, None], mu + np.exp(0.5 * eta) * gauss((n, T), seed + 2), np.nan)
    perm = qtl.permutations(n, P, seed, use=use) if P else None
    return origin, pheno, cov, (use if mask else None), perm


_REFS = {}


def case_reference(case, max_iter=None, tol=-1.0):
    """the reference of one of CASES (at its own max_iter and fixed iterations, or as asked), computed once and shared"""
    key = (case, max_iter, tol)
    if key not in _REFS:
        n, K, n_var, imprint, additive, seed, T, P, mask, skipped, mi = case
        origin, pheno, cov, use, perm = make_case(*case)
        _REFS[key] = reference_scan_var(origin, chromstarts_of(CHROM_LENS), pheno, use, cov, n_var, imprint, perm, additive,
                                        mi if max_iter is None else max_iter, tol, anchor_every=0 if tol < 0 else 7)
    return _REFS[key]


def assert_conditions(refs):
    """what the comparison rests on, over the cells of `refs` together: at least 0.99 compared, at most 0.01 near"""
    cs = chromstarts_of(CHROM_LENS)
    cells = np.concatenate([compared_cells(r, cs, share=0, strict=True).reshape(-1) for r in refs])
    near = np.concatenate([r["near"].reshape(-1) for r in refs])
    print("compared %.4f of %d cells, near %.4f" % (cells.mean(), cells.size, near.mean()))
    assert cells.mean() >= 0.99 and near.mean() <= 0.01


def assert_anchor(ref, what=""):
    """the converged yardstick against the longdouble run that knows nothing of the stopping rule"""
    print("%s: the yardstick's converged l against the longdouble anchor: %.3g LOD" % (what, ref["anchor_err"]))
    assert ref["anchor_err"] <= ATOL


# the planted case of the stopping rule and of "not a mean scan in disguise": an additive log-variance effect, no mean effect
PLANTED = dict(n=130, seed=5, noise_seed=9, marker=40, effect=1.0, tol=1e-7, max_iter=50, short=5)


def planted_case():
    """(origin, true classes, pheno, cov): soft rows of 130 individuals, one covariate, an additive log-variance effect of 1.0
    of the true classes at marker 40 and no mean effect"""
    p = PLANTED
    origin, k = soft_rows(p["n"], CHROM_LENS, p["seed"])
    z = noise(p["n"], 1, 6)
    eta = p["effect"] * CODES["a"][k][:, p["marker"]:p["marker"] + 1]
    return origin, k, 0.5 * z + np.exp(0.5 * eta) * gauss((p["n"], 1), p["noise_seed"]), z


def planted_reference():
    if "planted" not in _REFS:
        origin, _, pheno, z = planted_case()
        _REFS["planted"] = reference_scan_var(origin, chromstarts_of(CHROM_LENS), pheno, None, z, 0, max_iter=PLANTED["max_iter"],
                                              tol=PLANTED["tol"], anchor_every=7)
    return _REFS["planted"]


def planted_linear_reference():
    """Haley-Knott regression of the same column"""
    if "planted_hk" not in _REFS:
        origin, _, pheno, z = planted_case()
        _REFS["planted_hk"] = reference_scan(origin, chromstarts_of(CHROM_LENS), pheno, None, z)
    return _REFS["planted_hk"]


def assert_planted(ref, hk):
    """on the references alone: the variance LOD peaks within one marker of the planted one and is at least 3 there, the
    Haley-Knott LOD there is at most 1, and both stop rules decide cells at max_iter = short"""
    p = PLANTED
    lv, lm = ref["lod"][0, 0, :, 2], hk["lod"][0, 0]
    print("planted: variance LOD peak %.2f at %d, %.2f at %d; Haley-Knott LOD there %.2f" %
          (lv.max(), lv.argmax(), lv[p["marker"]], p["marker"], lm[p["marker"]]))
    assert abs(int(lv.argmax()) - p["marker"]) <= 1 and lv[p["marker"]] >= 3.0
    assert lm[p["marker"]] <= 1.0
    more = (ref["iters"] > p["short"])[~ref["near"]]
    print("planted: %d fits need more than %d iterations, %d do not" % (more.sum(), p["short"], (~more).sum()))
    assert more.sum() >= 10 and (~more).sum() >= 10, "both stop rules must decide fits at max_iter = short"


def planted_tight_reference():
    """the planted case stopped by 1e-12 LOD: the closed forms are asserted there"""
    if "planted_tight" not in _REFS:
        origin, _, pheno, z = planted_case()
        _REFS["planted_tight"] = reference_scan_var(origin, chromstarts_of(CHROM_LENS), pheno, None, z, 0, max_iter=PLANTED["max_iter"],
                                                    tol=1e-12)
    return _REFS["planted_tight"]


def hk_identity_bound():
    """With n_var = 0 the mean-only fit against the null fit is Haley-Knott's LOD, n_c / 2 log10(RSS0 / RSS1): ten times the
    yardstick's own largest error on that identity over the planted case's markers (only rounding separates the two)"""
    ref, hk = planted_tight_reference(), planted_linear_reference()
    own = float(np.abs((ref["ll"][0, :, 0] - np.repeat(ref["ll0"][0], np.diff(chromstarts_of(CHROM_LENS)))) / LN10 - hk["lod"][0, 0]).max())
    print("Haley-Knott identity: the yardstick's own error %.3g, the product's bound %.3g" % (own, 10 * own))
    return 10 * own


MONOTONE = (1, 2, 3, 5, 8)


def monotone_reference():
    """the planted case at exactly 8 iterations: its trace holds the joint LOD after every iteration of the full fit"""
    if "monotone" not in _REFS:
        origin, _, pheno, z = planted_case()
        _REFS["monotone"] = reference_scan_var(origin, chromstarts_of(CHROM_LENS), pheno, None, z, 0, max_iter=MONOTONE[-1], tol=-1.0)
    return _REFS["monotone"]


# a case whose trace takes a halving: t(4) noise on few individuals
HALVING = dict(n=41, K=1, n_var=1, seed=0, tol=1e-7, max_iter=50)


def halving_case():
    """(origin, pheno, cov): 41 individuals, one covariate in both parts, t(4) noise"""
    p = HALVING
    origin, k = soft_rows(p["n"], CHROM_LENS, p["seed"])
    z = noise(p["n"], 1, p["seed"] + 1)
    return origin, 0.5 * z + student4((p["n"], 1), p["seed"] + 2), z


def halving_reference():
    if "halving" not in _REFS:
        p = HALVING
        origin, pheno, z = halving_case()
        _REFS["halving"] = reference_scan_var(origin, chromstarts_of(CHROM_LENS), pheno, None, z, p["n_var"], imprint=True,
                                              max_iter=p["max_iter"], tol=p["tol"])
    return _REFS["halving"]


# ------------------------------------------------------------------------------------------------ an edge of the lane walk
EMPTY_ROUND = dict(n=130, seed=32, max_iter=50, tol=1e-7)


def empty_round_case():
    """(origin, pheno, cov, use) of 130 individuals of whom 64 .. 127 are not used: every lane's second step of the walk of 64
    is masked, and the third round holds individuals 128 and 129.  K = 1, n_var = 1, effects a and d."""
    p = EMPTY_ROUND
    origin, k = soft_rows(p["n"], CHROM_LENS, p["seed"])
    use = np.ones(p["n"], bool)
    use[64:128] = False
    z = noise(p["n"], 1, p["seed"] + 1)
    mu = 0.2 + 0.6 * CODES["a"][k][:, [3]] + 1.0 * z
    eta = 0.7 * CODES["a"][k][:, [40]]
    return origin, mu + np.exp(0.5 * eta) * gauss((p["n"], 1), p["seed"] + 2), z, use


def empty_round_reference():
    if "empty_round" not in _REFS:
        origin, pheno, z, use = empty_round_case()
        _REFS["empty_round"] = reference_scan_var(origin, chromstarts_of(CHROM_LENS), pheno, use, z, 1, max_iter=EMPTY_ROUND["max_iter"],
                                                  tol=EMPTY_ROUND["tol"])
    return _REFS["empty_round"]


THRESHOLD = dict(n=24, K=3, n_var=1, seed=10, chrom=4, need=11)     # (1 + 3 + 2) + (1 + 1 + 2) + 1 for the effects (a, i)


def threshold_case(n_c):
    """(origin, pheno, cov) of 24 individuals with three covariates of whom only the first n_c are there on chromosome 4 (the
    others are skipped on it).  For the design (a, i) with one variance covariate n_c = 11 is scanned there, n_c = 10 is not."""
    p = THRESHOLD
    cs = chromstarts_of(CHROM_LENS)
    origin, _ = soft_rows(p["n"], CHROM_LENS, p["seed"])
    origin[n_c:, cs[p["chrom"]]:cs[p["chrom"] + 1]] = 0.0
    return origin, gauss((p["n"], 1), p["seed"] + 3), noise(p["n"], p["K"], p["seed"] + 4)
