"""The reference of the variance-component scan (cnf2_qtl_scan_vc), shared by the CPU and the GPU suite; numpy only, nothing of the
product.  Per marker the explicit Z[i][h] = sum_k [col[i][k] == h] descent[i][m][k] on the rows with c_i = 1, A an orthonormal
basis of null(X0') from a full QR, Z~ = A'Z and y~ = A'y; the restricted log-likelihood of h from the Cholesky factor of
I + g Z~Z~', g = h / (1 - h):
    f(h) = ( nu log10(RSS0 / q) - log10|I + g Z~Z~'| ) / 2,    q = y~'(I + g Z~Z~')^-1 y~ clamped below at RSS0 2^-52.
The search is the definition's (include/cnf2hip.h): the 41 grid points, the first arg-max, then golden section on the dense
likelihood between the neighbouring grid points down to a width of 1e-9.  The eigenvalues are numpy.linalg.eigvalsh of
W = Z~'Z~.  The BLUP g Z~'(I + g Z~Z~')^-1 y~ and q / nu are evaluated at whatever h they are asked for: q has a slope in h, and
no search on function values locates h better than the square root of their rounding error, so the residual variance of a run
is compared at the h the run returned, as the BLUP is.

A CELL IS COMPARED when the dense likelihood has one local maximum on a grid of step 1e-3 and no eigenvalue of the marker
lies in (1e-13, 1e-7) x d_max, where the rank rule (1e-10 d_max) would hang on rounding; the suites assert on the reference,
before the code under test runs, that at least 0.9 of the cells of a case qualify."""
import numpy as np

GRID, HMAX = 41, 0.999
FLAT = 1e-12            # differences of f below this are no slope (counting local maxima)


def design(descent_m, col, H):
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


class Marker:
    """the dense pieces of one marker: Zt[nu][H], yt[nu][T], rss0[T], nu"""

    def __init__(self, descent_m, col, H, y, cov, c):
        y = np.asarray(y, np.float64)
        y = y[:, None] if y.ndim == 1 else y
        n, self.T = y.shape
        self.H = H
        rows = in_model(col, H, c)
        self.n_c = int(rows.sum())
        K = 0 if cov is None else np.asarray(cov).reshape(n, -1).shape[1]
        self.nu = self.n_c - 1 - K
        X0 = np.ones((self.n_c, 1)) if K == 0 else np.concatenate([np.ones((self.n_c, 1)), np.asarray(cov, np.float64).reshape(n, -1)[rows]], axis=1)
        self.scanned = self.n_c >= K + 4 and np.linalg.matrix_rank(X0) == K + 1
        self.rss0 = np.zeros(self.T)
        self.eval = np.zeros(H)
        if not self.scanned:
            return
        A = np.linalg.qr(X0, mode="complete")[0][:, K + 1:]
        self.Zt = A.T @ design(np.asarray(descent_m)[rows], np.asarray(col)[rows], H)
        self.yt = A.T @ y[rows]
        self.rss0 = (self.yt ** 2).sum(axis=0)
        self.eval = np.clip(np.linalg.eigvalsh(self.Zt.T @ self.Zt)[::-1], 0.0, None)
        self.ZZ = self.Zt @ self.Zt.T

    def q_logdet(self, h):
        """q[len(h)][T] (not clamped) and log10|I + g Z~Z~'|[len(h)] through stacked Cholesky factors"""
        h = np.atleast_1d(np.asarray(h, np.float64))
        q, ld = np.zeros((len(h), self.T)), np.zeros(len(h))
        for a in range(0, len(h), 128):
            g = h[a:a + 128] / (1.0 - h[a:a + 128])
            L = np.linalg.cholesky(np.eye(self.nu)[None] + g[:, None, None] * self.ZZ[None])
            x = np.linalg.solve(L, np.broadcast_to(self.yt, (len(g),) + self.yt.shape))
            q[a:a + 128] = (x ** 2).sum(axis=1)
            ld[a:a + 128] = 2.0 * np.log10(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1)
        return q, ld

    def f(self, h):
        """f[len(h)][T]"""
        q, ld = self.q_logdet(h)
        q = np.maximum(q, self.rss0 * 2.0 ** -52)
        return 0.5 * (self.nu * np.log10(self.rss0 / q) - ld[:, None])

    def f_screen(self, h):
        """f[len(h)][T] of the same dense nu x nu matrix through numpy.linalg.eigh of Z~Z~': what counts the local maxima on the
        grid of step 1e-3 (a thousand Cholesky factors per marker would be most of the suites' time); the search and every
        compared figure go through the Cholesky factors above"""
        lam, U = np.linalg.eigh(self.ZZ)
        lam = np.clip(lam, 0.0, None)
        g = (np.asarray(h, np.float64) / (1.0 - np.asarray(h, np.float64)))[:, None]
        w = 1.0 / (1.0 + g * lam[None])                                   # [len(h)][nu]
        q = np.maximum(w @ (U.T @ self.yt) ** 2, self.rss0 * 2.0 ** -52)
        return 0.5 * (self.nu * np.log10(self.rss0 / q) - np.log10(1.0 + g * lam[None]).sum(axis=1)[:, None])

    def sigma2(self, h, t):
        return float(max(self.q_logdet([h])[0][0, t], self.rss0[t] * 2.0 ** -52)) / self.nu

    def blup(self, h, t):
        g = h / (1.0 - h)
        return g * self.Zt.T @ np.linalg.solve(np.eye(self.nu) + g * self.ZZ, self.yt[:, t])


def count_maxima(f):
    d = np.diff(f)
    d = d[np.abs(d) >= FLAT]
    if len(d) == 0:
        return 1
    s = np.sign(d)
    return int(s[0] < 0) + int(((s[:-1] > 0) & (s[1:] < 0)).sum()) + int(s[-1] > 0)


def golden(fun, a, b, width=1e-9):
    r = (np.sqrt(5.0) - 1.0) / 2.0
    c, d = b - r * (b - a), a + r * (b - a)
    fc, fd = fun(c), fun(d)
    while b - a > width:
        if fc >= fd:
            b, d, fd = d, c, fc
            c = b - r * (b - a)
            fc = fun(c)
        else:
            a, c, fc = c, d, fd
            d = a + r * (b - a)
            fd = fun(d)
    return 0.5 * (a + b)


def marker(descent_m, col, H, y, cov=None, c=None):
    """One marker: dict(lod[T], h[T], rss0[T], eval[H], rank, n_used, compared[T] bool, clear: no eigenvalue near the rank rule,
    dense: the Marker)"""
    mk = Marker(descent_m, col, H, y, cov, c)
    T = mk.T
    out = dict(lod=np.zeros(T), h=np.zeros(T), rss0=mk.rss0, eval=mk.eval, rank=0, n_used=mk.n_c, compared=np.zeros(T, bool), dense=mk, clear=True)
    if not mk.scanned:
        out["compared"][:] = True
        return out
    dmax = mk.eval[0]
    out["rank"] = int((mk.eval > 1e-10 * dmax).sum())
    clear = out["clear"] = not ((mk.eval > 1e-13 * dmax) & (mk.eval < 1e-7 * dmax)).any()
    if mk.nu < 2 or out["rank"] == 0:
        out["compared"][:] = clear
        return out
    hj = HMAX * np.arange(GRID) / (GRID - 1)
    fj = mk.f(hj)
    fj[0] = 0.0
    fine = mk.f_screen(np.arange(1000) * 1e-3)
    for t in range(T):
        if not mk.rss0[t] > 0:
            out["compared"][t] = clear
            continue
        js = int(np.argmax(fj[:, t]))
        h = golden(lambda x: mk.f([x])[0, t], hj[max(js - 1, 0)], hj[min(js + 1, GRID - 1)])
        lod = float(mk.f([h])[0, t])
        if lod > 0:
            out["lod"][t], out["h"][t] = lod, h
        out["compared"][t] = clear and count_maxima(fine[:, t]) == 1
    return out


def scan(descent, col, H, y, chromstarts, cov=None, use=None):
    """The whole map: dict(lod[T][M], h[T][M], eval[M][H], rank[M], rss0[T][C], n_used[C], compared[T][M], clear[M], dense[M])"""
    d = np.asarray(descent, np.float64)
    y = np.asarray(y, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, M = d.shape[:2]
    T = y.shape[1]
    cs = np.asarray(chromstarts)
    C = len(cs) - 1
    base = in_model(col, H, use)
    out = dict(lod=np.zeros((T, M)), h=np.zeros((T, M)), eval=np.zeros((M, H)), rank=np.zeros(M, np.int32), rss0=np.zeros((T, C)),
               n_used=np.zeros(C, np.int32), compared=np.zeros((T, M), bool), clear=np.zeros(M, bool), dense=[None] * M)
    for c in range(C):
        cm = base & (d[:, cs[c]] != 0).any(axis=1)
        out["n_used"][c] = cm.sum()
        for m in range(cs[c], cs[c + 1]):
            r = marker(d[:, m], col, H, y, cov, cm)
            out["lod"][:, m], out["h"][:, m], out["eval"][m], out["rank"][m] = r["lod"], r["h"], r["eval"], r["rank"]
            out["compared"][:, m], out["dense"][m], out["clear"][m] = r["compared"], r["dense"], r["clear"]
            out["rss0"][:, c] = r["rss0"]
    return out


def check(got, want, what, atol=1e-9, blup=True):
    """The comparison of both suites: n_used, rss0, rank and the eigenvalues everywhere; LOD (atol), h (1e-5), and at the h the
    run returned sigma2 (atol) and the BLUP (atol times its largest entry) on the cells compared; sigma2 also inside what the
    reference's own h^ +- 1e-5 allows.  Returns the worst differences."""
    cmp = want["compared"]
    assert cmp.mean() >= 0.9, what + ": at least 0.9 of the cells are compared (%.3f)" % cmp.mean()
    assert np.array_equal(got["n_used"], want["n_used"]), what
    np.testing.assert_allclose(got["rss0"], want["rss0"], rtol=1e-12, atol=atol, err_msg=what)
    assert np.all(got["rank"] >= 0), what + ": the Jacobi iteration converged at every marker"
    clear = want["clear"]
    assert np.array_equal(got["rank"][clear], want["rank"][clear]), what
    dmax = np.maximum(want["eval"][:, :1], 1e-300)
    worst = dict(eval=float((np.abs(got["eval"] - want["eval"]) / dmax).max()), lod=0.0, h=0.0, sigma2=0.0, blup=0.0, pair=-np.inf)
    T, M = want["lod"].shape
    for t in range(T):
        for m in range(M):
            if not cmp[t, m]:
                continue
            worst["lod"] = max(worst["lod"], abs(got["lod"][t, m] - want["lod"][t, m]))
            worst["h"] = max(worst["h"], abs(got["h"][t, m] - want["h"][t, m]))
            mk = want["dense"][m]
            if not mk.scanned or mk.nu < 1:
                continue
            hr = float(got["h"][t, m])
            worst["sigma2"] = max(worst["sigma2"], abs(got["sigma2"][t, m] - mk.sigma2(hr, t)))
            # ... and it belongs to the reference's own h^: q falls as h rises, and the run's h is within 1e-5 of h^, so its
            # sigma2 lies between the dense q / nu at h^ + 1e-5 and at h^ - 1e-5
            h0 = float(want["h"][t, m])
            lo, hi = mk.sigma2(min(h0 + 1e-5, HMAX), t), mk.sigma2(max(h0 - 1e-5, 0.0), t)
            worst["pair"] = max(worst["pair"], lo - got["sigma2"][t, m], got["sigma2"][t, m] - hi)
            if blup and got.get("blup") is not None:
                u = mk.blup(hr, t) if hr > 0 else np.zeros(mk.H)
                worst["blup"] = max(worst["blup"], float(np.abs(got["blup"][t, m] - u).max() / max(np.abs(u).max(), 1e-300)) if hr > 0
                                    else float(np.abs(got["blup"][t, m]).max()))
    print("%s: %d of %d cells compared; largest difference lod %.3g, h %.3g, sigma2 %.3g, blup (relative) %.3g, eigenvalues (of d_max) %.3g"
          % (what, cmp.sum(), cmp.size, worst["lod"], worst["h"], worst["sigma2"], worst["blup"], worst["eval"]))
    assert worst["lod"] <= atol and worst["sigma2"] <= atol and worst["blup"] <= atol, what
    assert worst["h"] <= 1e-5, what
    assert worst["pair"] <= atol, what + ": sigma2 outside what the reference's h^ +- 1e-5 allows by %.3g" % worst["pair"]
    assert worst["eval"] <= 1e-12, what
    assert np.all(got["lod"] >= 0) and np.all(np.isfinite(got["lod"])) and np.all((got["h"] == 0) == (got["lod"] == 0))
    return worst
