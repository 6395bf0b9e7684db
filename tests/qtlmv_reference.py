"""The yardstick of the multi-trait scan's tests (tests/test_qtlmv_host.py, tests/test_gpu_qtlmv.py): per chromosome, group
and marker np.linalg.lstsq of the T columns on the explicit null and full designs, the rows of individuals with c_i = 0
deleted, E0 and E1 from the residuals and lod = n_c / 2 (logdet E0 - logdet E1) / ln 10 by slogdet.  It shares nothing with
the whitened Schur form of the product (cnf2freq_amd/csrc/cnf2_qtlmv.h).  The marker rank comes by qtl_reference's third
route; which traits are kept, by the residuals of every trait on the null design and the traits kept before it."""
import numpy as np

from cnf2freq_amd import qtl, synth
from qtl_reference import (ATOL, CHROM_LENS, PIVOT_DROP, PIVOT_EXACT, PIVOT_WELL, chromstarts_of, columns, compared_markers,
                           noise, reference_scan, skip, soft_rows)

COND_MAX = 1e5           # E0 of every scanned chromosome and group is at most this badly conditioned
LAMBDA_MIN = 2.0 ** -52  # the model's clamp (include/cnf2hip.h)

#        n   T   P  K  additive
CASES = [(5, 1, 0, 0, False),
         (13, 2, 5, 0, False),
         (17, 3, 33, 2, False),          # 34 groups: three waves at T4 = 4
         (64, 5, 17, 0, False),          # T4 = 8 with padding, 18 groups
         (67, 8, 9, 2, False),           # T4 = 8 full; n not a multiple of the unroll
         (67, 9, 5, 0, False),           # T4 = 16 padded; a second wave with two groups
         (64, 16, 4, 2, True),           # additive; a second wave with one group
         (24, 16, 1, 0, False)]          # few degrees of freedom

# the rows of five individuals that keep every marker well conditioned (tests/test_gpu_qtl.py)
ROW_SEEDS = {5: 2}


def make_case(n, T, P, K, seed=11):
    """(origin, pheno, cov, use, perm) on the map CHROM_LENS: soft rows; traits noise + 0.5 (k[:, 20] - 1.5), mixed by
    I + 0.1 (U - 0.5); for n > 12 individual 2 is unused and carries NaN, and individuals 1 and 3 are skipped on chromosome 2"""
    origin, k = soft_rows(n, CHROM_LENS, ROW_SEEDS.get(n, seed + n))
    use = None
    U = synth.uniform(seed * 16 + 11, np.arange(T * T)).reshape(T, T)
    pheno = (noise(n, T, seed) + 0.5 * (k[:, 20:21] - 1.5)) @ (np.eye(T) + 0.1 * (U - 0.5))
    cov = synth.uniform(seed * 16 + 9, np.arange(n * K)).reshape(n, K) * 2.0 - 1.0 if K else None
    if K:
        pheno = pheno + 0.3 * cov[:, :1]
    if n > 12:
        origin = skip(origin, [1, 3], 2, CHROM_LENS)
        use = np.ones(n, bool)
        use[2] = False
        pheno[2] = np.nan
        if K:
            cov[2] = np.nan
    perm = qtl.permutations(n, P, seed, use=use) if P else None
    return origin, pheno, cov, use, perm


def kept_traits(R0):
    """(kept[T], relpivot[T]) of the residuals R0[n_c][T] on the null design, in trait order: the squared length of what the
    traits kept before leave of trait t, over its own; NaN for a trait without any"""
    T = R0.shape[1]
    kept, rel = np.zeros(T, bool), np.full(T, np.nan)
    for t in range(T):
        r = R0[:, t]
        ett = r @ r
        if not ett > 1e-24 * max(1.0, np.abs(R0).max() ** 2):          # (a constant trait: 0 in the model, rounding here)
            continue
        prev = R0[:, kept]
        res = r - prev @ np.linalg.lstsq(prev, r, rcond=None)[0] if prev.shape[1] else r
        rel[t] = res @ res / ett
        kept[t] = rel[t] >= PIVOT_DROP
    return kept, rel


def reference_scan_mv(origin, chromstarts, pheno, use=None, cov=None, perm=None, additive=False):
    """A dict: lod[1 + P][M] (group 0 observed), rank[M], relpivot[M][2], usable[C] (the observed group is scanned),
    trait_rank[C], n_used[C], perm_max[P][C], and the conditions of a comparison: cond[C][1 + P] of E0 over the kept traits
    and trait_relpivot[C][1 + P][T] (both NaN where the chromosome is not fitted)."""
    o = np.asarray(origin, np.float64)
    n, M, _ = o.shape
    cs = np.asarray(chromstarts, np.int64)
    C = len(cs) - 1
    pheno = np.asarray(pheno, np.float64).reshape(n, -1)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    X0all = np.ones((n, 1)) if cov is None else np.concatenate([np.ones((n, 1)), np.asarray(cov, np.float64).reshape(n, -1)], axis=1)
    nx = X0all.shape[1]
    Y = columns(np.where(use[:, None], pheno, 0.0), perm)
    Q, T = Y.shape[1], Y.shape[2]
    # the marker ranks, their relative pivots and n_c by the single scan's reference (one trait is enough for those)
    one = reference_scan(o, cs, np.where(use[:, None], pheno[:, :1], 0.0), use, cov, None, additive)
    lod = np.zeros((Q, M))
    rank = one["rank"].copy()
    usable = np.zeros(C, bool)
    trait_rank = np.zeros(C, np.int32)
    cond = np.full((C, Q), np.nan)
    trp = np.full((C, Q, T), np.nan)
    for c in range(C):
        keep = use & (o[:, cs[c]] != 0.0).any(axis=1)
        n_c = int(keep.sum())
        X0 = np.where(np.isfinite(X0all[keep]), X0all[keep], 0.0)
        fit = n_c >= nx + 2 + T and np.linalg.matrix_rank(X0) == nx
        kept = np.zeros((Q, T), bool)
        if fit:
            y = Y[keep].reshape(n_c, Q * T)
            R0 = (y - X0 @ np.linalg.lstsq(X0, y, rcond=None)[0]).reshape(n_c, Q, T)
            for q in range(Q):
                kept[q], trp[c, q] = kept_traits(R0[:, q])
                if kept[q].any():
                    cond[c, q] = np.linalg.cond(R0[:, q][:, kept[q]].T @ R0[:, q][:, kept[q]])
        trait_rank[c] = kept[0].sum()
        usable[c] = kept[0].any()
        if not usable[c]:
            rank[cs[c]:cs[c + 1]] = 0
        if not kept.any():
            continue
        ld0 = np.zeros(Q)
        for q in range(Q):
            if kept[q].any():
                r = R0[:, q][:, kept[q]]
                ld0[q] = np.linalg.slogdet(r.T @ r)[1]
        for m in range(cs[c], cs[c + 1]):
            a = o[keep, m, 3] - o[keep, m, 0]
            d = o[keep, m, 1] + o[keep, m, 2]
            X = np.column_stack([X0, a] if additive else [X0, a, d])
            R1 = (y - X @ np.linalg.lstsq(X, y, rcond=None)[0]).reshape(n_c, Q, T)
            for q in range(Q):
                if not kept[q].any():
                    continue
                r = R1[:, q][:, kept[q]]
                sign, ld1 = np.linalg.slogdet(r.T @ r)
                lam = np.exp(ld1 - ld0[q]) if sign > 0 else 0.0
                lam = min(max(lam, LAMBDA_MIN), 1.0)
                lod[q, m] = -0.5 * n_c * np.log10(lam) if lam < 1.0 else 0.0
    perm_max = np.zeros((Q - 1, C))
    for c in range(C):
        perm_max[:, c] = lod[1:, cs[c]:cs[c + 1]].max(axis=1)
    return dict(lod=lod, rank=rank, relpivot=one["relpivot"], usable=usable, marker_usable=one["usable"], trait_rank=trait_rank,
                n_used=one["n_used"], perm_max=perm_max, cond=cond, trait_relpivot=trp)


def conditions(ref, chromstarts, additive=False, share=0.9):
    """What a comparison at ATOL rests on, asserted on the reference alone: cond(E0) <= COND_MAX for every chromosome and
    group; every trait's relative pivot at least PIVOT_WELL, or at most PIVOT_EXACT (or without any) where a trait is
    degenerate by construction; every marker well conditioned or exactly degenerate (qtl_reference.compared_markers)."""
    cond, rp = ref["cond"], ref["trait_relpivot"]
    assert np.all(np.isnan(cond) | (cond <= COND_MAX)), "cond(E0) reaches %.3g" % np.nanmax(cond)
    assert np.all(np.isnan(rp) | (rp >= PIVOT_WELL) | (rp <= PIVOT_EXACT)), "a trait's relative pivot is %.3g" % np.nanmin(
        np.where(rp > PIVOT_EXACT, rp, np.nan))
    compared_markers(dict(relpivot=ref["relpivot"], usable=ref["marker_usable"], rank=ref["rank"]), chromstarts, additive, 0)
    on = np.repeat(ref["usable"], np.diff(np.asarray(chromstarts, np.int64)))
    if share:
        assert (on & (ref["rank"] == (1 if additive else 2))).mean() >= share
    return np.nanmax(cond) if np.isfinite(cond).any() else 0.0


def compare(got, ref, what=""):
    """lod, rank, trait_rank, n_used and perm_max; prints every figure before it asserts.  Returns the two errors."""
    err_l = np.abs(got["lod"] - ref["lod"][0]).max()
    err_p = np.abs(got["perm_max"] - ref["perm_max"]).max() if ref["perm_max"].shape[0] else 0.0
    print("%s: lod %.3g over %d markers (largest %.2f), perm_max %.3g over %d cells" %
          (what, err_l, got["lod"].size, ref["lod"][0].max(), err_p, ref["perm_max"].size))
    assert np.array_equal(got["rank"], ref["rank"]), what + " rank"
    assert np.array_equal(got["trait_rank"], ref["trait_rank"]), what + " trait_rank"
    assert np.array_equal(got["n_used"], ref["n_used"]), what + " n_used"
    assert err_l <= ATOL, what + " lod"
    assert err_p <= ATOL, what + " perm_max"
    assert np.all(got["lod"] >= 0) and np.isfinite(got["lod"]).all()
    return err_l, err_p


_REFS = {}


def case_reference(case):
    """(inputs, reference) of a case of CASES, computed once and shared (nothing changes them)"""
    if case not in _REFS:
        n, T, P, K, additive = case
        inputs = make_case(n, T, P, K)
        origin, pheno, cov, use, perm = inputs
        _REFS[case] = (inputs, reference_scan_mv(origin, chromstarts_of(CHROM_LENS), pheno, use, cov, perm, additive))
    return _REFS[case]


def centred(v, use):
    """the columns of v minus their means over the used individuals, as the scan forms them (unused rows 0)"""
    v = np.asarray(v, np.float64)
    u = np.ones(len(v), bool) if use is None else np.asarray(use) != 0
    out = np.zeros_like(v)
    out[u] = v[u] - v[u].mean(axis=0)
    return out
