"""The yardstick of the linked pair scan's tests (tests/test_qtl2_linked_host.py, tests/test_gpu_qtl2_linked.py): the
per-pair least-squares fit of tests/qtl2_reference.py with the full model on the pairs of one chromosome too -- there the
interaction columns are the expectations of the products under the pair's joint row -- and a synthetic joint to feed it: per
individual and pair a coupling of the two origin rows that is not their product."""
import numpy as np

from qtl_reference import columns
from qtl2_reference import MIN_EXTRA, added_columns, chrom_of, lod_of, sequential_pivots

U, V = np.divmod(np.arange(16), 4)
A_OF = np.array([-1.0, 0.0, 0.0, 1.0])       # a and d of a certain individual of class 0 .. 3
D_OF = np.array([0.0, 1.0, 1.0, 0.0])


def linked(sel, chromstarts):
    """[(j, k)]: the pairs of indices into sel on one chromosome, ascending j, then ascending k (cnf2_linked_pairs)"""
    sc = chrom_of(sel, chromstarts)
    return [(j, k) for j in range(len(sel)) for k in range(j + 1, len(sel)) if sc[j] == sc[k]]


def north_west(p, q):
    """the north-west-corner coupling of two distributions on 0 .. 3: a 4 x 4 table with margins p and q that puts its mass
    as near the diagonal as the margins allow"""
    p, q = np.array(p, np.float64), np.array(q, np.float64)
    t = np.zeros((4, 4))
    i = j = 0
    while i < 4 and j < 4:
        m = min(p[i], q[j])
        t[i, j] = m
        p[i] -= m
        q[j] -= m
        if p[i] <= 0 and i < 4:
            i += 1
        elif q[j] <= 0:
            j += 1
    return t


def synthetic_joint(origin, chromstarts, sel):
    """joint[n][n_pairs][16] for the linked pairs of sel: half the product of the two rows, half their north-west-corner
    coupling.  Margins: the rows; entries not negative; not a product.  A skipped individual's rows (all zero) give zeros."""
    o = np.asarray(origin, np.float64)
    pairs = linked(sel, chromstarts)
    J = np.zeros((o.shape[0], len(pairs), 16))
    for i in range(o.shape[0]):
        for x, (j, k) in enumerate(pairs):
            p, q = o[i, sel[j]], o[i, sel[k]]
            J[i, x] = (0.5 * np.outer(p, q) + 0.5 * north_west(p, q)).reshape(16)
    return J


def product_joint(origin, chromstarts, sel):
    """joint[n][n_pairs][16] = the outer product of the two rows"""
    o = np.asarray(origin, np.float64)
    pairs = linked(sel, chromstarts)
    return np.stack([(o[:, sel[j], :, None] * o[:, sel[k], None, :]).reshape(-1, 16) for j, k in pairs], axis=1)


def interaction_columns(J, additive):
    """the interaction columns of a pair from its joint rows J[n][16]: E[a1 a2], E[a1 d2], E[d1 a2], E[d1 d2]"""
    e = lambda f, g: J @ (f[U] * g[V])
    if additive:
        return [e(A_OF, A_OF)]
    return [e(A_OF, A_OF), e(A_OF, D_OF), e(D_OF, A_OF), e(D_OF, D_OF)]


def reference_scan2_linked(origin, joint, chromstarts, sel, pheno, use=None, cov=None, perm=None, additive=False):
    """qtl2_reference.reference_scan2 with the same-chromosome branch given its interaction columns from joint[n][n_pairs][16]
    (the linked pairs of sel in cnf2_linked_pairs' order): lod_full and rank_full at every pair, relpivot of all eight
    columns, perm_max[..][1], [..][2] over all pairs.  `cross` is every pair of the upper triangle, so that
    qtl2_reference.compare2 compares lod_full there; `two_chrom` the pairs on two chromosomes."""
    o = np.asarray(origin, np.float64)
    n = o.shape[0]
    cs = np.asarray(chromstarts, np.int64)
    C, sel = len(cs) - 1, np.asarray(sel, np.int64)
    L, sc = len(sel), chrom_of(sel, cs)
    row_of = {p: x for x, p in enumerate(linked(sel, cs))}
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    X0all = np.ones((n, 1)) if cov is None else np.concatenate([np.ones((n, 1)), np.asarray(cov, np.float64).reshape(n, -1)], axis=1)
    nx = X0all.shape[1]
    pheno = np.asarray(pheno, np.float64).reshape(n, -1)
    Y = columns(np.where(use[:, None], pheno, 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    lod_add, lod_full = np.full((Q, T, L, L), np.nan), np.full((Q, T, L, L), np.nan)
    rank_add, rank_full = np.full((L, L), -1, np.int32), np.full((L, L), -1, np.int32)
    relpivot = np.full((L, L, 8), np.nan)
    usable, n_used, rss0_out = np.zeros((C, C), bool), np.zeros((C, C), np.int32), np.zeros((T, C, C))
    present = o[:, cs[:-1]].any(axis=2)
    for c1 in range(C):
        for c2 in range(c1, C):
            keep = use & present[:, c1] & present[:, c2]
            n_c = int(keep.sum())
            n_used[c1, c2] = n_used[c2, c1] = n_c
            X0 = np.where(keep[:, None], X0all, 0.0)[keep]
            ok = n_c >= (nx - 1) + MIN_EXTRA and np.linalg.matrix_rank(X0) == nx
            usable[c1, c2] = usable[c2, c1] = ok
            pairs = [(j, k) for j in np.flatnonzero(sc == c1) for k in np.flatnonzero(sc == c2) if j < k]
            if not ok:
                for j, k in pairs:
                    lod_add[:, :, j, k], rank_add[j, k] = 0.0, 0
                    lod_full[:, :, j, k], rank_full[j, k] = 0.0, 0
                continue
            y = Y[keep].reshape(n_c, Q * T)
            rss0 = ((y - X0 @ np.linalg.lstsq(X0, y, rcond=None)[0]) ** 2).sum(axis=0)
            rss0_out[:, c1, c2] = rss0_out[:, c2, c1] = rss0[:T]
            for j, k in pairs:
                add, inter = added_columns(o[keep, sel[j]], o[keep, sel[k]], additive, c1 == c2)
                if c1 == c2:
                    inter = interaction_columns(np.asarray(joint)[keep, row_of[(j, k)]], additive)
                rel, kept = sequential_pivots(X0, add + inter)
                relpivot[j, k, :len(rel)] = rel
                rank_add[j, k] = sum(kept[:len(add)])
                Xa = np.column_stack([X0] + add)
                rss_a = ((y - Xa @ np.linalg.lstsq(Xa, y, rcond=None)[0]) ** 2).sum(axis=0)
                lod_add[:, :, j, k] = lod_of(rss0, rss_a, n_c).reshape(Q, T)
                rank_full[j, k] = sum(kept)
                Xf = np.column_stack([Xa] + inter)
                rss_f = ((y - Xf @ np.linalg.lstsq(Xf, y, rcond=None)[0]) ** 2).sum(axis=0)
                lod_full[:, :, j, k] = lod_of(rss0, np.minimum(rss_f, rss_a), n_c).reshape(Q, T)
    upper = np.arange(L)[:, None] < np.arange(L)[None, :]
    two_chrom = (sc[:, None] != sc[None, :]) & upper
    perm_max = np.zeros((Q - 1, T, 3))
    if Q > 1:
        perm_max[:, :, 0] = lod_add[1:][:, :, upper].max(axis=2)
        perm_max[:, :, 1] = lod_full[1:][:, :, upper].max(axis=2)
        perm_max[:, :, 2] = (lod_full[1:] - lod_add[1:])[:, :, upper].max(axis=2)
    return dict(lod_add=lod_add, lod_full=lod_full, rank_add=rank_add, rank_full=rank_full, relpivot=relpivot, usable=usable,
                n_used=n_used, rss0=rss0_out, perm_max=perm_max, cross=upper, upper=upper, two_chrom=two_chrom)


def zero_cM_case(n=40, seed=5):
    """(lens, origin, joint, sel, pheno): one chromosome of three markers; markers 0 and 1 lie at one position and their
    rows are equal -- the joint of that pair is diagonal --, marker 2 is an ordinary linked locus.  In the pair (0, 1) the
    second locus repeats the first: a2 and d2 are dropped, and so is every interaction column -- E[a1 a2] = E[a^2] = p0 + p3
    = 1 - d1 and E[d1 d2] = E[d^2] = d1 lie in the span of the intercept and d1, E[a1 d2] and E[d1 a2] are zero: ranks (2, 2),
    and lod_full = lod_add.  Two loci at one position cannot interact."""
    from qtl_reference import noise, soft_rows
    lens = (3,)
    origin, _ = soft_rows(n, lens, seed)
    origin[:, 1] = origin[:, 0]
    sel = np.arange(3, dtype=np.int32)
    joint = synthetic_joint(origin, [0, 3], sel)
    diag = np.zeros((n, 16))
    diag[:, [0, 5, 10, 15]] = origin[:, 0]
    joint[:, 0] = diag
    a = origin[:, :, 3] - origin[:, :, 0]
    pheno = noise(n, 2, seed + 2) + np.stack([0.8 * a[:, 0] * a[:, 2], 0.5 * a[:, 0]], axis=1)
    return lens, origin, joint, sel, pheno
