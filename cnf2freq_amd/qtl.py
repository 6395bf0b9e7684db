"""QTL scans on the origin rows: Context.qtl_scan / Context.sweep_qtl (cnf2_qtl_scan, cnf2_sweep_qtl) and how to read them.

The scan is Haley-Knott regression of phenotypes on a = P(BB) - P(AA) and d = P(AB) + P(BA) at every marker (the model:
include/cnf2hip.h); it runs on the GPU for the observed phenotypes and for every permuted one.  This module makes the
permutations, the residuals that are permuted when there are covariates (Freedman-Lane), turns the permutations' maxima into
thresholds and reads peaks with their LOD-drop support intervals off a profile.  Nothing here scans."""
import numpy as np

from . import synth


def permutations(n, P, seed, use=None, strata=None):
    """perm[P][n] (int32): permutation p gives individual i the phenotype of perm[p][i].  Within every stratum the used
    individuals, in ascending order idx[0..k), are ordered by the key synth.splitmix64(seed, p * n + i) with a stable
    argsort: perm[p][idx[j]] = idx[order[j]].  Unused individuals map to themselves.  No sequential generator enters, so
    the same lines in another language give the same arrays (cnf2h_qtl_permutations of the host library, which
    `cnF2freq --qtl` uses)."""
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    strata = np.zeros(n, np.int64) if strata is None else np.asarray(strata)
    if use.shape != (n,) or strata.shape != (n,):
        raise ValueError("use and strata must be [n]")
    perm = np.tile(np.arange(n, dtype=np.int32), (P, 1))
    groups = [np.flatnonzero(use & (strata == s)) for s in np.unique(strata[use])] if use.any() else []
    for p in range(P):
        keys = synth.splitmix64(seed, np.uint64(p) * np.uint64(n) + np.arange(n, dtype=np.uint64))
        for idx in groups:
            perm[p, idx] = idx[np.argsort(keys[idx], kind="stable")]
    return perm


_permutations = permutations      # (scan's argument of the same name is a count)


def null_residuals(pheno, cov=None, use=None):
    """[n][T]: the residuals of every phenotype column on the null design [1, cov] over the used individuals (0 for the
    others).  With covariates a permutation test permutes these, not the raw values (Freedman and Lane 1983); without,
    the two give the same LODs."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n = y.shape[0]
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    X = np.ones((n, 1))
    if cov is not None:
        z = np.asarray(cov, np.float64)
        X = np.concatenate([X, z[:, None] if z.ndim == 1 else z], axis=1)
    res = np.zeros_like(y)
    if use.any():
        beta = np.linalg.lstsq(X[use], y[use], rcond=None)[0]
        res[use] = y[use] - X[use] @ beta
    return res


def scan(ctx, pheno, cov=None, use=None, permutations=0, seed=0, additive=False):
    """The scan of a whole cross on the context's uploaded pedigree: one origin sweep with the rows left on the device, then
    per pattern of missing phenotypes (NaN) one observed scan with the pattern's own `use`, and with permutations > 0 one
    more on the permuted residuals of the null model.  A dict: lod[T][M], coef[T][M][2], rank[T][M] (the design, and with
    it the rank, depends on who is used), n_used[T][C], perm_max[P][T][C] or None."""
    import torch
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    M, C = ctx.n_markers, ctx.n_chrom
    dev = torch.device("cuda", ctx.device)          # the context's GPU, whatever torch's current one is
    t = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    d_f, d_l, d_o, d_s, d_c = t(n, C, 8), t(n, C), t(n, M, 4), t(M, 4), t(C, dtype=torch.int32)
    ctx.sweep_origins_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_o.data_ptr(), None, d_s.data_ptr(), d_c.data_ptr())
    ctx.sync()
    out = dict(lod=np.zeros((T, M)), coef=np.full((T, M, 2), np.nan), rank=np.zeros((T, M), np.int32),
               n_used=np.zeros((T, C), np.int32), perm_max=np.zeros((permutations, T, C)) if permutations else None)
    missing = ~np.isfinite(y)
    patterns = {}
    for k in range(T):
        patterns.setdefault(missing[:, k].tobytes(), []).append(k)
    for cols in patterns.values():
        u = use & ~missing[:, cols[0]]
        yk = np.where(u[:, None], y[:, cols], 0.0)
        got = ctx.qtl_scan_device(n, d_o.data_ptr(), yk, cov=cov, use=u, additive=additive)
        out["lod"][cols], out["coef"][cols] = got["lod"], got["coef"]
        out["rank"][cols], out["n_used"][cols] = got["rank"], got["n_used"]
        if permutations:
            perm = _permutations(n, permutations, seed, use=u)
            res = null_residuals(yk, cov, u)
            out["perm_max"][:, cols] = ctx.qtl_scan_device(n, d_o.data_ptr(), res, cov=cov, use=u, perm=perm,
                                                           additive=additive)["perm_max"]
    return out


def quantile_index(P, alpha):
    """index into P ascending values of the (1 - alpha) threshold: the smallest value that at most alpha P values exceed"""
    return min(P - 1, max(0, int(np.ceil((1.0 - alpha) * P)) - 1))


def thresholds(perm_max, alpha=(0.05, 0.01)):
    """From perm_max[P][T][C]: genome[len(alpha)][T], the thresholds of the maximum over the whole map, and
    chromosome[len(alpha)][T][C], those of one chromosome scanned alone.  A threshold is the order statistic number
    ceil((1 - alpha) P) of the P maxima: at most alpha P permutations exceed it (the conservative convention)."""
    pm = np.asarray(perm_max, np.float64)
    if pm.ndim != 3 or pm.shape[0] == 0:
        raise ValueError("perm_max must be [P][T][C] with P >= 1")
    P = pm.shape[0]
    genome_sorted = np.sort(pm.max(axis=2), axis=0)
    chrom_sorted = np.sort(pm, axis=0)
    idx = [quantile_index(P, a) for a in alpha]
    return dict(alpha=tuple(alpha), genome=genome_sorted[idx], chromosome=chrom_sorted[idx])


def peaks(lod, pos, chromstarts, threshold, drop=1.5, coef=None):
    """Per trait and chromosome the marker with the largest LOD, where that is above the threshold (a number or one per
    trait): a list of dicts with trait, chrom, marker, lod, the LOD-drop support interval lo .. hi (the markers around the
    peak, without a gap, whose LOD is within `drop` of it; pos_lo, pos_hi their positions) and, with coef[T][M][2], the
    effects at the peak.  The first marker wins a tie."""
    lod = np.asarray(lod, np.float64)
    lod = lod[None, :] if lod.ndim == 1 else lod
    T, M = lod.shape
    cs = np.asarray(chromstarts, np.int64)
    pos = np.asarray(pos, np.float64)
    thr = np.broadcast_to(np.asarray(threshold, np.float64), (T,))
    found = []
    for t in range(T):
        for c in range(len(cs) - 1):
            seg = lod[t, cs[c]:cs[c + 1]]
            k = int(np.argmax(seg))
            if not seg[k] > thr[t]:
                continue
            lo = hi = k
            while lo > 0 and seg[lo - 1] >= seg[k] - drop:
                lo -= 1
            while hi + 1 < len(seg) and seg[hi + 1] >= seg[k] - drop:
                hi += 1
            m = int(cs[c]) + k
            p = dict(trait=t, chrom=c, marker=m, lod=float(seg[k]), lo=int(cs[c]) + lo, hi=int(cs[c]) + hi,
                     pos=float(pos[m]), pos_lo=float(pos[cs[c] + lo]), pos_hi=float(pos[cs[c] + hi]))
            if coef is not None:
                p["additive"], p["dominance"] = (float(v) for v in np.asarray(coef)[t, m])
            found.append(p)
    return found
