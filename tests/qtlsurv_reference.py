"""The yardstick of the survival-trait scan's tests (tests/test_qtlsurv_host.py, tests/test_gpu_qtlsurv.py): Cox's regression
of include/cnf2hip.h per marker and column in numpy, by a route that shares nothing with the product's running sums along the
risk order (cnf2freq_amd/csrc/cnf2_qtlsurv.h).  The design is explicit, with the rows of individuals with c_i = 0 deleted and
the covariates as given (not centred); the partial likelihood, its score and its information come from the direct risk-set
definition -- per event k the selection t_j >= t_k, one row of a 0/1 matrix per event -- with no order, no running sum and no
tie groups; the step is np.linalg.solve.  Which effects a marker keeps comes from qtlx_reference's sequential pivots.

Independent of the stopping rule, `anchor` maximises the same likelihood in longdouble by 60 Newton steps from theta = 0 with
an elimination of its own; the converged yardstick must agree with it (assert_anchor)."""
import numpy as np

from cnf2freq_amd import synth
from qtl_reference import ATOL, CHROM_LENS, PIVOT_DROP, chromstarts_of, columns, noise, reference_scan, skip, soft_rows  # noqa: F401
from qtlx_reference import effects, reference_scanx  # noqa: F401
from qtlem_reference import CODES, degenerate_rows  # noqa: F401
from qtlbin_reference import NEAR_TOL, ETA_MAX, compared_cells, solve_ld, reference_scan_binary  # noqa: F401

LN10 = np.log(10.0)
NULL_ITER, NULL_TOL = 50, 1e-13


def risk_sets(t, d):
    """R[k][j] = 1 where individual j is at risk at the time of event k (t_j >= t_k), one row per event; and the events"""
    ev = np.flatnonzero(d == 1.0)
    return (t[None, :] >= t[ev, None]).astype(np.float64), ev


def terms(X, R, ev, theta, order=2):
    """l(theta), the score, the information and the largest |eta - mean eta| by the direct definition:
    l = sum_k [eta_k - log S0_k], s = sum_k [x_k - S1_k / S0_k], G = sum_k [S2_k / S0_k - (S1_k / S0_k)(S1_k / S0_k)']
    with S0_k, S1_k, S2_k the sums of w, w x, w x x' over the risk set of event k"""
    eta = X @ theta
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        w = np.exp(eta)
        S0 = R @ w
        ll = float((eta[ev] - np.log(S0)).sum())
        me = float(np.abs(eta - eta.mean()).max()) if len(eta) else 0.0
        if order < 2 or not np.isfinite(ll):
            return ll, None, None, me
        p = X.shape[1]
        E1 = (R @ (w[:, None] * X)) / S0[:, None]
        S2 = (R @ (w[:, None] * (X[:, :, None] * X[:, None, :]).reshape(len(w), p * p))).reshape(-1, p, p)
        G = (S2 / S0[:, None, None]).sum(axis=0) - E1.T @ E1
        s = X[ev].sum(axis=0) - E1.sum(axis=0)
    return ll, s, G, me


def newton(X, R, ev, theta, ll_start, max_iter, tol):
    """Newton's method by the rule of include/cnf2hip.h from theta, whose log-likelihood is ll_start (None: computed).  A dict:
    ll (the trace l_0 .. l_t), theta, iters, status, gains (of the last two iterations), maxeta."""
    theta = np.array(theta, np.float64)
    trace, gains, t, maxeta, prev = [], [], 0, 0.0, None
    while True:
        ll, s, G, me = terms(X, R, ev, theta)
        if t >= 1 and not np.isfinite(ll):          # the pass broke down: back to the iterate before
            theta, t, status = prev, t - 1, 2
            break
        maxeta = max(maxeta, me)
        if t == 0 and ll_start is not None:
            ll = ll_start
        if t >= 1:
            gains.append((ll - trace[-1]) / LN10)
        trace.append(ll)
        if t >= 1 and gains[-1] < tol:
            status = 0
            break
        if t >= 1 and t >= max_iter:
            status = 1
            break
        try:
            if not np.isfinite(G).all():
                raise np.linalg.LinAlgError
            np.linalg.cholesky(G)
            new = theta + np.linalg.solve(G, s)
        except np.linalg.LinAlgError:
            status = 2
            break
        if not np.isfinite(new).all():
            status = 2
            break
        prev, theta, t = theta, new, t + 1
    return dict(ll=np.array(trace), theta=theta, iters=t, status=status, gains=gains[-2:], maxeta=maxeta)


def null_fit(Z, R, ev):
    """(l0, gamma0) of a column on the covariates Z, or None where the column is not scanned"""
    if len(ev) == 0:
        return None
    K = Z.shape[1]
    if K == 0:
        l0 = terms(Z, R, ev, np.zeros(0), order=0)[0]
        return (l0, np.zeros(0)) if np.isfinite(l0) else None
    f = newton(Z, R, ev, np.zeros(K), None, NULL_ITER, NULL_TOL)
    if f["status"] != 0 or f["iters"] < 1:
        return None
    return float(f["ll"][-1]), f["theta"]


def closed_form_null(t, d):
    """l0 without covariates: -sum over the distinct event times of (events there) log(individuals at risk there)"""
    return -sum(((t == v) & (d == 1.0)).sum() * np.log((t >= v).sum()) for v in np.unique(t[d == 1.0]))


def anchor(X, t, d, steps=60):
    """the maximum of l over theta by `steps` Newton steps from theta = 0 in longdouble: no start from the null fit, no
    stopping rule, no double-precision solver; a loop over the events"""
    X = np.array(X, np.longdouble)
    theta = np.zeros(X.shape[1], np.longdouble)
    ev = np.flatnonzero(d == 1.0)

    def pass_(theta, step):
        eta = X @ theta
        w = np.exp(eta)
        ll, s, G = np.longdouble(0.0), np.zeros_like(theta), np.zeros((len(theta), len(theta)), np.longdouble)
        for k in ev:
            r = t >= t[k]
            S0 = w[r].sum()
            ll += eta[k] - np.log(S0)
            if step:
                e1 = (w[r, None] * X[r]).sum(axis=0) / S0
                s += X[k] - e1
                G += (X[r].T @ (w[r, None] * X[r])) / S0 - np.outer(e1, e1)
        return ll, s, G
    for _ in range(steps):
        _, s, G = pass_(theta, True)
        theta = theta + solve_ld(G, s)
    return float(pass_(theta, False)[0])


def reference_scan_surv(origin, chromstarts, time, status, use=None, cov=None, imprint=False, perm=None, additive=False,
                        max_iter=50, tol=1e-7, anchor_every=0):
    """The model of include/cnf2hip.h.  A dict: lod[1 + P][T][M] (block 0 observed), trace[T][M][max_iter + 1] of the observed
    columns' LODs after every iteration (the last value repeated), coef[T][M][ne], iters[T][M], status[T][M], near[T][M] (a
    deciding gain lies within NEAR_TOL of tol), maxeta[T][M], rank[M], relpivot[M][ne], usable[C], n_used[C], ll0[T][C],
    n_events[T][C], perm_max[P][T][C]; with anchor_every = k > 0 also anchor_err, the largest |LOD - anchor's LOD| over the
    observed cells of every k-th marker that stopped by tol."""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    cs = np.asarray(chromstarts, np.int64)
    C = len(cs) - 1
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    Z = np.zeros((n, 0)) if cov is None else np.where(use[:, None], np.asarray(cov, np.float64).reshape(n, -1), 0.0)
    eff = effects(additive, imprint)
    ne = len(eff)
    tt = np.where(use[:, None], np.nan_to_num(np.asarray(time, np.float64).reshape(n, -1)), 0.0)
    dd = np.where(use[:, None], np.nan_to_num(np.asarray(status, np.float64).reshape(n, -1)), 0.0)
    hk = reference_scanx(o, cs, tt[:, :1], use, cov, 0, imprint, None, additive)
    Tm, Dm = columns(tt, perm), columns(dd, perm)
    Q, T = Tm.shape[1], Tm.shape[2]
    lod = np.zeros((Q, T, M))
    trace = np.zeros((T, M, max_iter + 1))
    coef = np.full((T, M, ne), np.nan)
    iters, status_o, near = np.zeros((T, M), np.int32), np.zeros((T, M), np.int32), np.zeros((T, M), bool)
    maxeta = np.zeros((T, M))
    rank = np.zeros(M, np.int32)
    ll0_out, n_events = np.zeros((T, C)), np.zeros((T, C), np.int32)
    anchor_err = 0.0
    for c in range(C):
        keep = use & (o[:, cs[c]] != 0.0).any(axis=1)
        Zc = Z[keep]
        K = Zc.shape[1]
        n_events[:, c] = Dm[keep, 0].sum(axis=0)
        if not hk["usable"][c]:
            continue
        sets = [[risk_sets(Tm[keep, qq, t], Dm[keep, qq, t]) for t in range(T)] for qq in range(Q)]
        nulls = [[null_fit(Zc, *sets[qq][t]) for t in range(T)] for qq in range(Q)]
        for t in range(T):
            if nulls[0][t] is not None:
                ll0_out[t, c] = nulls[0][t][0]
        for m in range(cs[c], cs[c + 1]):
            kept = np.nan_to_num(hk["relpivot"][m], nan=0.0) >= PIVOT_DROP
            rank[m] = int(kept.sum())
            assert rank[m] == hk["rank"][m][1]
            if rank[m] == 0:
                continue
            om = o[keep, m]
            val = dict(a=om[:, 3] - om[:, 0], d=om[:, 1] + om[:, 2], i=om[:, 1] - om[:, 2])
            X = np.column_stack([Zc] + [val[e] for e, k in zip(eff, kept) if k])
            for qq in range(Q):
                for t in range(T):
                    if nulls[qq][t] is None:
                        continue
                    l0, g0 = nulls[qq][t]
                    f = newton(X, *sets[qq][t], np.concatenate([g0, np.zeros(rank[m])]), l0, max_iter, tol)
                    lod[qq, t, m] = max(0.0, (f["ll"][-1] - l0) / LN10)
                    if qq == 0:
                        tr = np.maximum(0.0, (f["ll"] - l0) / LN10)
                        trace[t, m, :len(tr)] = tr
                        trace[t, m, len(tr):] = tr[-1]
                        coef[t, m, kept] = f["theta"][K:]
                        iters[t, m], status_o[t, m], maxeta[t, m] = f["iters"], f["status"], f["maxeta"]
                        near[t, m] = any(abs(g - tol) <= NEAR_TOL * abs(tol) for g in f["gains"])
                        if anchor_every and m % anchor_every == 0 and f["status"] == 0 and f["maxeta"] <= ETA_MAX:
                            anchor_err = max(anchor_err, abs(f["ll"][-1] - anchor(X, Tm[keep, 0, t], Dm[keep, 0, t])) / LN10)
    perm_max = np.zeros((Q - 1, T, C))
    for c in range(C):
        perm_max[:, :, c] = lod[1:, :, cs[c]:cs[c + 1]].max(axis=2)
    return dict(lod=lod, trace=trace, coef=coef, iters=iters, status=status_o, near=near, maxeta=maxeta, rank=rank,
                relpivot=hk["relpivot"], usable=hk["usable"], n_used=hk["n_used"], ll0=ll0_out, n_events=n_events, perm_max=perm_max,
                anchor_err=anchor_err)


def compare_surv(got, ref, chromstarts, what="", share=0.99, strict=True, iters=True):
    """every output of a scan against the reference at the compared cells (qtlbin_reference.compared_cells: well-conditioned
    or exactly degenerate pivots, largest |eta| at most ETA_MAX): lod and ll0 within ATOL, coef relative to max(1, |coef|)
    (NaN exactly where the reference has none), perm_max within ATOL; rank (at markers with a compared cell), n_used,
    n_events and status with ==, iters with == except where ref["near"].  Prints every figure before it asserts; returns the
    errors."""
    cc = compared_cells(ref, chromstarts, share, strict)
    cm = cc.any(axis=0)
    err_l = np.abs(got["lod"] - ref["lod"][0])[cc].max()
    gc, rc = got["coef"][cc], ref["coef"][cc]
    both = ~np.isnan(rc)
    err_c = (np.abs(gc[both] - rc[both]) / np.maximum(1.0, np.abs(rc[both]))).max() if both.any() else 0.0
    err_0 = np.abs(got["ll0"] - ref["ll0"]).max()
    print("%s: lod %.3g over %d of %d cells, coef %.3g, ll0 %.3g, iterations up to %d, near %d, largest |eta| %.3g" %
          (what, err_l, cc.sum(), cc.size, err_c, err_0, ref["iters"].max(), ref["near"].sum(), ref["maxeta"].max()))
    assert np.array_equal(np.isnan(gc), np.isnan(rc)), what + ": a dropped effect is NaN, a kept one a number"
    assert np.array_equal(got["rank"][cm], ref["rank"][cm]), what + " rank"
    assert np.array_equal(got["n_used"], ref["n_used"]), what + " n_used"
    assert np.array_equal(got["n_events"], ref["n_events"]), what + " n_events"
    assert err_l <= ATOL, what + " lod"
    assert err_c <= ATOL, what + " coef"
    assert err_0 <= ATOL, what + " ll0"
    assert np.array_equal(got["ll0"] == 0.0, ref["ll0"] == 0.0) and np.all(got["ll0"] <= 0.0), what + " ll0 is 0 where nothing is scanned"
    assert np.isfinite(got["lod"]).all() and np.all(got["lod"] >= 0), what + " lod is finite and not negative"
    off = ~np.repeat(ref["usable"], np.diff(np.asarray(chromstarts, np.int64)))
    assert np.all(got["lod"][:, off] == 0.0) and np.isnan(got["coef"][:, off]).all() and np.all(got["rank"][off] == 0)
    zero = got["rank"] == 0
    assert np.all(got["lod"][:, zero] == 0.0) and np.all(got["iters"][:, zero] == 0) and np.all(got["status"][:, zero] == 0)
    assert np.array_equal(got["status"][cc], ref["status"][cc]), what + " status"
    if iters:
        ok = cc & ~ref["near"]
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
# n decides the rounds of 64 positions; every K = 0 .. 8 once (the kernels are compiled once per K + 1); the designs (a, d),
# (a), (a, i), (a, d, i); `grid` > 0 rounds the times up to multiples of 1 / grid, which makes tie groups
#         n    K  imprint additive seed T  P  mask   skipped max_iter grid
CASES = [(41, 2, False, False, 3, 2, 0, False, False, 5, 0),        # less than one round; (a, d)
         (63, 3, True, True, 21, 1, 1, False, False, 3, 4),         # one short of a round; (a, i); ties
         (64, 0, False, False, 4, 1, 1, False, False, 3, 0),        # exactly one round, no covariates
         (65, 4, False, False, 22, 1, 1, False, True, 3, 4),        # one past a round; skipped individuals; ties
         (127, 6, False, True, 24, 1, 1, True, False, 3, 0),        # (a), with a `use` mask
         (129, 7, True, True, 25, 1, 1, False, False, 3, 8),        # one past two rounds; (a, i); ties
         (130, 8, True, False, 9, 2, 5, False, False, 4, 0),        # three rounds, the widest design (a, d, i); T = 2, P = 5
         (67, 5, True, False, 23, 1, 1, False, True, 3, 2),         # skipped individuals inside coarse tie groups
         (41, 1, True, True, 26, 2, 0, False, False, 3, 0)]         # K = 1
STOP = dict(max_iter=50, tol=1e-7)           # the stopping rule the cases also run under
HOST_CASES = (CASES[0], CASES[3], CASES[1])  # what tests/test_qtlsurv_host.py runs cell by cell


def case_id(c):
    return "n%d-K%d-%s%s-T%d-P%d-it%d%s%s" % (c[0], c[1], "i" if c[2] else "m", "-add" if c[3] else "", c[5], c[6], c[9],
                                              "-mask" if c[7] else "-skip" if c[8] else "", "-ties" if c[10] else "")


def draw_times(eta, seed, censored=0.3, grid=0):
    """(time, status) of exponential lifetimes with hazard exp(eta) and independent exponential censoring times whose rate
    (found by bisection) makes the expected share of censored individuals `censored` (by synth.uniform); grid > 0: the times
    rounded up to multiples of 1 / grid"""
    u = synth.uniform(seed * 16 + 11, np.arange(eta.size)).reshape(eta.shape)
    v = synth.uniform(seed * 16 + 12, np.arange(eta.size)).reshape(eta.shape)
    h = np.exp(eta)
    lo, hi = 0.0, 1e6
    for _ in range(200):
        rate = 0.5 * (lo + hi)
        lo, hi = (rate, hi) if (rate / (rate + h)).mean() < censored else (lo, rate)
    life, cens = -np.log1p(-u) / h, -np.log1p(-v) / rate
    time, status = np.minimum(life, cens), (life <= cens).astype(np.float64)
    if grid:
        time = np.ceil(time * grid) / grid
    return time, status


def make_case(n, K, imprint, additive, seed, T, P, mask, skipped, max_iter=None, grid=0):
    """(origin, time, status, cov, use, perm) on the map CHROM_LENS: rows soft_rows(n, CHROM_LENS, seed), covariates
    noise(n, K, seed + 1), lifetimes from a proportional-hazards model of the true classes plus the first covariate, 30 %
    censored.  With `mask` two individuals are unused and carry NaN times, statuses and covariates; with `skipped`
    individuals 1 and 4 are skipped on chromosome 3."""
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
    eta = 0.7 * a[:, at] + 0.4 * d[:, to] - 0.5 * im[:, to]
    if K:
        eta = eta + 1.0 * cov[:, :1]
        cov = np.where(use[:, None], cov, np.nan)
    time, status = draw_times(eta, seed + 2, grid=grid)
    time, status = np.where(use[:, None], time, np.nan), np.where(use[:, None], status, np.nan)
    perm = qtl.permutations(n, P, seed, use=use) if P else None
    return origin, time, status, cov, (use if mask else None), perm


_REFS = {}


def case_reference(case, max_iter=None, tol=-1.0):
    """the reference of one of CASES (at its own max_iter and fixed iterations, or as asked), computed once and shared"""
    key = (case, max_iter, tol)
    if key not in _REFS:
        n, K, imprint, additive, seed, T, P, mask, skipped, mi, grid = case
        origin, time, status, cov, use, perm = make_case(*case)
        _REFS[key] = reference_scan_surv(origin, chromstarts_of(CHROM_LENS), time, status, use, cov, imprint, perm, additive,
                                         mi if max_iter is None else max_iter, tol,
                                         anchor_every=0 if tol < 0 else 14 if n < 100 else 42)     # (the anchor is a Python loop over the events)
    return _REFS[key]


def assert_conditions(refs):
    """what the comparison rests on, over the cells of `refs` together: at least 0.99 compared, at most 0.01 near"""
    cs = chromstarts_of(CHROM_LENS)
    cells = np.concatenate([compared_cells(r, cs, share=0, strict=True).reshape(-1) for r in refs])
    near = np.concatenate([r["near"].reshape(-1) for r in refs])
    print("compared %.4f of %d cells, near %.4f" % (cells.mean(), cells.size, near.mean()))
    assert cells.mean() >= 0.99 and near.mean() <= 0.01


def assert_anchor(ref, what=""):
    """the converged yardstick against the longdouble Newton run that knows nothing of the stopping rule"""
    print("%s: the yardstick's converged LOD against the longdouble anchor: %.3g" % (what, ref["anchor_err"]))
    assert ref["anchor_err"] <= ATOL


# ------------------------------------------------------------------------------------------------ hand-made ties and censoring
HAND = dict(n=130, seed=41, K=1, max_iter=50, tol=1e-7)


def hand_case(which):
    """(origin, time, status, cov, use) of 130 individuals, K = 1, effects (a, d), made by hand from distinct times 130 .. 1
    in the order of the individuals (individual i has position i of the risk order) and a status pattern with 30 % censored:
      "span"       positions 60 .. 70 share one time: a tie group across the boundary of the first round
      "censored"   positions 20 .. 25 share one time and are all censored: a group without an event
      "masked"     positions 30 .. 36 share one time; 32 is skipped on chromosome 3 and 34 is not used
      "first"      position 0 has an event;  "last": position 129 has an event and position 0 has not
      "single"     one event in all, at position 41 (the yardstick scans it: the covariate of that individual lies inside its risk set's)
      "ninety"     90 % censored
      "none"       everybody censored: nothing is scanned
      "empty"      individuals 64 .. 127 are not used: a round of the lane walk in which nobody is unmasked"""
    p = HAND
    n = p["n"]
    origin, k = soft_rows(n, CHROM_LENS, p["seed"])
    z = noise(n, 1, p["seed"] + 1)
    time = np.arange(n, 0, -1).astype(np.float64)
    u = synth.uniform(p["seed"] * 16 + 13, np.arange(n))
    status = (u >= 0.3).astype(np.float64)
    use = np.ones(n, bool)
    if which == "span":
        time[60:71] = time[60]
    elif which == "censored":
        time[20:26] = time[20]
        status[20:26] = 0.0
    elif which == "masked":
        time[30:37] = time[30]
        status[30:37] = 1.0
        origin = skip(origin, [32], 3, CHROM_LENS)
        use[34] = False
    elif which == "first":
        status[0] = 1.0
    elif which == "last":
        status[0], status[n - 1] = 0.0, 1.0
    elif which == "single":
        status[:] = 0.0
        status[41] = 1.0
    elif which == "ninety":
        status = (u >= 0.9).astype(np.float64)
    elif which == "none":
        status[:] = 0.0
    elif which == "empty":
        use[64:128] = False
    else:
        raise KeyError(which)
    # the times follow the genotype at marker 40 a little, so that the fits have something to find: swap neighbours
    a = CODES["a"][k][:, 40]
    if which in ("first", "last", "ninety", "empty"):
        for i in range(0, n - 1, 2):
            if a[i] > a[i + 1]:
                time[[i, i + 1]] = time[[i + 1, i]]
    return origin, time[:, None], status[:, None], z, (None if use.all() else use)


HAND_CASES = ("span", "censored", "masked", "first", "last", "single", "ninety", "none", "empty")


def hand_reference(which):
    if ("hand", which) not in _REFS:
        origin, time, status, z, use = hand_case(which)
        _REFS[("hand", which)] = reference_scan_surv(origin, chromstarts_of(CHROM_LENS), time, status, use, z,
                                                     max_iter=HAND["max_iter"], tol=HAND["tol"])
    return _REFS[("hand", which)]


# ------------------------------------------------------------------------------------------------ the planted locus
PLANTED = dict(n=60, seed=5, marker=40, effect=1.2, tol=1e-7, max_iter=50, censored=0.4)


def planted_case():
    """(origin, time, status, cov): soft rows of 60 individuals, one covariate, an additive effect of 1.2 on the log hazard of
    the true classes at marker 40; 40 % censored"""
    p = PLANTED
    origin, k = soft_rows(p["n"], CHROM_LENS, p["seed"])
    z = noise(p["n"], 1, 6)
    eta = p["effect"] * CODES["a"][k][:, p["marker"]:p["marker"] + 1] + 0.5 * z
    time, status = draw_times(eta, 9, censored=p["censored"])
    return origin, time, status, z


def planted_references():
    """(Cox, Haley-Knott regression of the times as numbers, logistic regression of the status)"""
    if "planted" not in _REFS:
        origin, time, status, z = planted_case()
        cs = chromstarts_of(CHROM_LENS)
        _REFS["planted"] = (reference_scan_surv(origin, cs, time, status, None, z, max_iter=PLANTED["max_iter"], tol=PLANTED["tol"],
                                                anchor_every=1),
                            reference_scan(origin, cs, time, None, z),
                            reference_scan_binary(origin, cs, status, None, z, max_iter=50, tol=1e-7))
    return _REFS["planted"]


def assert_planted(ref, hk, bn):
    """on the references alone: the Cox profile peaks at the planted marker and differs from the linear scan of the times and
    from the logistic scan of the status by more than 0.2 LOD somewhere"""
    lc, ll, lb = ref["lod"][0, 0], hk["lod"][0, 0], bn["lod"][0, 0]
    print("planted: Cox peak %.2f at %d; linear scan of the times: peak %.2f at %d, largest difference %.2f; logistic scan of the "
          "status: peak %.2f at %d, largest difference %.2f" %
          (lc.max(), lc.argmax(), ll.max(), ll.argmax(), np.abs(lc - ll).max(), lb.max(), lb.argmax(), np.abs(lc - lb).max()))
    assert lc.argmax() == PLANTED["marker"]
    assert np.abs(lc - ll).max() > 0.2 and np.abs(lc - lb).max() > 0.2


MONOTONE = (1, 2, 3, 5, 8)


def monotone_reference():
    """the planted case at exactly 8 iterations: its trace holds the LOD after every iteration"""
    if "monotone" not in _REFS:
        origin, time, status, z = planted_case()
        _REFS["monotone"] = reference_scan_surv(origin, chromstarts_of(CHROM_LENS), time, status, None, z, max_iter=MONOTONE[-1], tol=-1.0)
    return _REFS["monotone"]


def perfect_order_case(n=24, seed=4, marker=8):
    """(origin, time, status): certain rows (one-hot on the true class) of 24 individuals whose times are ordered perfectly by
    a at `marker` -- everybody with a = 1 dies before everybody with a = 0, and those before everybody with a = -1, all
    observed -- so that the partial likelihood grows without bound in the effect of a there"""
    origin, k = soft_rows(n, CHROM_LENS, seed)
    o = np.zeros_like(origin)
    np.put_along_axis(o, k[:, :, None], 1.0, axis=2)
    a = o[:, marker, 3] - o[:, marker, 0]
    order = np.argsort(-a, kind="stable")
    time = np.empty(n)
    time[order] = np.arange(1.0, n + 1.0)
    return o, time[:, None], np.ones((n, 1))


THRESHOLD = dict(n=24, K=3, seed=10, chrom=4, W=6)     # W = 1 + K + 2 for the effects (a, i)


def threshold_case(n_c):
    """(origin, time, status, cov) of 24 individuals with three covariates of whom only the first n_c are there on chromosome
    4 (the others are skipped on it).  For the design (a, i), W = 6: n_c = 7 is scanned there, n_c = 6 is not."""
    p = THRESHOLD
    cs = chromstarts_of(CHROM_LENS)
    origin, _ = soft_rows(p["n"], CHROM_LENS, p["seed"])
    origin[n_c:, cs[p["chrom"]]:cs[p["chrom"] + 1]] = 0.0
    time, status = draw_times(np.zeros((p["n"], 1)), p["seed"] + 3)
    status[:7, 0] = [1, 1, 0, 1, 1, 0, 1]
    return origin, time, status, noise(p["n"], p["K"], p["seed"] + 4)
