"""The yardstick of the multiple-imputation scan's tests (tests/test_qtlimp_host.py, tests/test_gpu_qtlimp.py): every draw's
states are turned into explicit one-hot origin rows and go through qtl_reference.reference_scan, the per-marker least-squares
fit in numpy; the draws are then combined with a two-pass maximum and sum in longdouble.  It shares nothing with the
product's class arithmetic, Schur form or online recurrence (cnf2freq_amd/csrc/cnf2_qtlimp.h).

The conditions a comparison rests on are asserted here, on the reference alone, before anything of the product runs."""
import numpy as np

from cnf2freq_amd import qtl, synth
from qtl_reference import (ATOL, CHROM_LENS, PIVOT_DROP, chromstarts_of, compared_markers, noise, reference_scan,  # noqa: F401
                           soft_rows)

COMBINE_BOUND = 9e-16    # the float64 two-pass combination against the longdouble one (absolute, in LOD units)
SHARE = 0.9              # at least this share of the markers has every draw compared
SKIPPED = 255


def encode(classes, seed):
    """states (uint8) of origin classes k = bit0 + 2 bit3, with bits 1, 2, 4 and 5 filled with noise"""
    k = np.asarray(classes, np.int64)
    junk = (synth.uniform(seed * 16 + 12, np.arange(k.size)).reshape(k.shape) * 16).astype(np.int64)
    g = (k & 1) | ((k >> 1) << 3) | ((junk & 3) << 1) | (((junk >> 2) & 3) << 4)
    return g.astype(np.uint8)


def synthetic_states(n, lens, D, seed):
    """state[n][D][M]: draw d is the base path (soft_rows' true classes for `seed`) with a fifth of its cells taken from an
    independent path of its own; the bits the model ignores are noise"""
    base = soft_rows(n, lens, seed)[1]
    M = base.shape[1]
    k = np.empty((n, D, M), np.int64)
    for d in range(D):
        other = soft_rows(n, lens, seed * 1024 + 17 + d)[1]
        take = synth.uniform((seed * 1024 + d) * 16 + 11, np.arange(n * M)).reshape(n, M) < 0.2
        k[:, d] = np.where(take, other, base)
    return encode(k, seed)


def skip_states(state, individuals, chrom, lens):
    """the states of `individuals` on chromosome `chrom` set to 0xFF in every draw: skipped there"""
    cs = chromstarts_of(lens)
    s = state.copy()
    s[np.asarray(individuals), :, cs[chrom]:cs[chrom + 1]] = SKIPPED
    return s


def classes_of(state):
    """k (255 stays 255), written out here once more: the product's qtl.sampled_classes is tested against it"""
    g = np.asarray(state, np.int64)
    return np.where(g == SKIPPED, SKIPPED, (g & 1) + 2 * ((g >> 3) & 1))


def one_hot(state_d):
    """origin[n][M][4] of one draw's states [n][M]: 1 at the class, an all-zero row where skipped"""
    k = classes_of(state_d)
    return (k[:, :, None] == np.arange(4)[None, None, :]).astype(np.float64)


def combine(lod_d, dtype=np.longdouble):
    """m + log10(sum_d 10^(lod_d - m) / D) along axis 0 in two passes, and the weights 10^(lod_d - m) / s"""
    l = np.asarray(lod_d, dtype)
    m = l.max(axis=0)
    w = dtype(10.0) ** (l - m)
    s = w.sum(axis=0)
    return m + np.log10(s / dtype(l.shape[0])), w / s


def reference_imp(state, chromstarts, pheno, use=None, cov=None, perm=None, additive=False):
    """The model of include/cnf2hip.h (cnf2_qtl_scan_imp).  A dict: lod[1 + P][T][M] the combined LOD (block 0 observed),
    lod64 the same combined in float64, coef[T][M][2] (NaN where a draw has none), rank[M] the smallest over the draws,
    n_used[C], rss0[T][C], usable[C], perm_max[P][T][C], draw_lod[D][T][M], draws: the D references of reference_scan."""
    st = np.asarray(state, np.uint8)
    n, D, M = st.shape
    refs = [reference_scan(one_hot(st[:, d]), chromstarts, pheno, use, cov, perm, additive) for d in range(D)]
    lods = np.stack([r["lod"] for r in refs])                                   # [D][1 + P][T][M]
    lod, w = combine(lods)
    lod64 = combine(lods, np.float64)[0]
    coefs = np.stack([r["coef"] for r in refs])                                 # [D][T][M][2]
    coef = (w[:, 0, :, :, None] * coefs.astype(np.longdouble)).sum(axis=0)
    cs = np.asarray(chromstarts, np.int64)
    perm_max = np.zeros((lod.shape[0] - 1, lod.shape[1], len(cs) - 1))
    for c in range(len(cs) - 1):
        perm_max[:, :, c] = lod[1:, :, cs[c]:cs[c + 1]].max(axis=2)
    for r in refs[1:]:
        assert np.array_equal(r["n_used"], refs[0]["n_used"]) and np.array_equal(r["usable"], refs[0]["usable"])
    return dict(lod=lod.astype(np.float64), lod64=lod64, combine_err=float(np.abs(lod64 - lod).max()), coef=coef.astype(np.float64),
                rank=np.min([r["rank"] for r in refs], axis=0), n_used=refs[0]["n_used"], rss0=refs[0]["rss0"],
                usable=refs[0]["usable"], perm_max=perm_max, draw_lod=lods[:, 0], draws=refs)


def conditions(ref, chromstarts, additive=False, what="", share=SHARE):
    """Asserted on the yardstick before anything runs: in every draw every marker of a usable chromosome is well
    conditioned or exactly degenerate (qtl_reference.compared_markers), and at least `share` of the markers have every draw
    compared.  Returns (compared[M], shares[D])."""
    per = np.stack([compared_markers(r, chromstarts, additive, share=0) for r in ref["draws"]])
    shares = per.mean(axis=1)
    compared = per.all(axis=0)
    print("%s: compared share per draw %.3f .. %.3f, every draw %.3f; float64 against longdouble combination %.3g" %
          (what, shares.min(), shares.max(), compared.mean(), ref["combine_err"]))
    assert compared.mean() >= share, what + ": too few markers have every draw compared"
    return compared, shares


def kept(ref, additive=False):
    """keep[M][2]: the column is kept in every draw, by the relative pivots of the draws' references"""
    rp = np.stack([r["relpivot"] for r in ref["draws"]])                        # [D][M][2]
    keep = np.nan_to_num(rp, nan=0.0) >= PIVOT_DROP
    if additive:
        keep[:, :, 1] = False
    return keep.all(axis=0)


def compare(got, ref, chromstarts, additive=False, what="", share=SHARE):
    """lod at every cell, coef at the compared markers and NaN exactly where a draw drops the column, rank, n_used, rss0,
    perm_max and, where given, draw_lod; prints every figure before it asserts"""
    compared, _ = conditions(ref, chromstarts, additive, what, share)
    err_l = np.abs(got["lod"] - ref["lod"][0]).max()
    cols = [0] if additive else [0, 1]
    gc, rc = got["coef"][:, compared][:, :, cols], ref["coef"][:, compared][:, :, cols]
    err_c = (np.abs(gc - rc) / np.maximum(1.0, np.abs(rc))).max() if gc.size else 0.0
    err_r = np.abs(got["rss0"] - ref["rss0"]).max()
    err_d = np.abs(got["draw_lod"] - ref["draw_lod"]).max() if got.get("draw_lod") is not None else 0.0
    print("%s: lod %.3g over %d cells, coef %.3g over %d of %d markers, rss0 %.3g, draw_lod %.3g" %
          (what, err_l, got["lod"].size, err_c, compared.sum(), len(compared), err_r, err_d))
    assert np.array_equal(got["rank"], ref["rank"]), what + " rank"
    assert np.array_equal(got["n_used"], ref["n_used"]), what + " n_used"
    assert err_l <= ATOL, what + " lod"
    assert err_c <= ATOL, what + " coef"
    assert err_d <= ATOL, what + " draw_lod"
    assert err_r <= ATOL * max(1.0, np.abs(ref["rss0"]).max()), what + " rss0"
    assert np.all(got["lod"] >= 0) and np.isfinite(got["lod"]).all()
    cs = np.asarray(chromstarts, np.int64)
    live = np.repeat(ref["usable"], np.diff(cs))[None, :] & np.repeat(ref["rss0"] > 0, np.diff(cs), axis=1)   # [T][M]
    want_nan = ~(kept(ref, additive)[None, :, :] & live[:, :, None])
    assert np.array_equal(np.isnan(got["coef"]), want_nan), what + ": a coefficient is NaN exactly where a draw drops its column"
    if ref["perm_max"].shape[0]:
        err_p = np.abs(got["perm_max"] - ref["perm_max"]).max()
        print("%s: perm_max %.3g over %d cells" % (what, err_p, ref["perm_max"].size))
        assert err_p <= ATOL, what + " perm_max"
    return compared


# ------------------------------------------------------------------------------------------------ the cases of the issue
#             n   D   K  T  P  additive seed
CPU_CASES = [(41, 17, 2, 2, 0, False, 3),
             (41, 3, 8, 1, 0, False, 4),
             (63, 16, 0, 1, 0, True, 5),
             (65, 65, 1, 2, 0, False, 6),
             (130, 2, 3, 2, 0, False, 7)]
# the GPU's: every n, D, K and P of the issue, both models; 130: the individuals 64 .. 127 are not used; 67: individuals 0-2
# are skipped on chromosome SKIPPED_CHROM; 63 with P = 20 and T = 1: a 16-column tile holds the observed column and permuted ones
GPU_CASES = [(41, 17, 2, 2, 3, False, 3),
             (41, 3, 8, 1, 0, False, 4),
             (63, 16, 0, 1, 20, True, 5),
             (65, 65, 1, 3, 3, False, 6),
             (130, 2, 3, 2, 20, False, 7),
             (64, 1, 2, 1, 3, False, 8),
             (67, 2, 0, 2, 0, True, 9)]
SKIPPED_CHROM = 3


def make_case(n, D, K, T, P, additive, seed, special=True):
    """(state, pheno, cov, use, perm) of a case on CHROM_LENS: synthetic states, traits with a locus each (on the base path)
    plus noise, uniform covariates, the permutations of qtl.permutations.  With `special` the cases of 130 and 67
    individuals get their unused and skipped individuals."""
    state = synthetic_states(n, CHROM_LENS, D, seed)
    M = state.shape[2]
    use = None
    if special and n == 130:
        use = np.ones(n, bool)
        use[64:128] = False
    if special and n == 67:
        state = skip_states(state, [0, 1, 2], SKIPPED_CHROM, CHROM_LENS)
    cov = synth.uniform(seed * 16 + 9, np.arange(n * K)).reshape(n, K) * 2.0 - 1.0 if K else None
    k = soft_rows(n, CHROM_LENS, seed)[1]
    a = (k == 3).astype(np.float64) - (k == 0)
    d = ((k == 1) | (k == 2)).astype(np.float64)
    at = [(11 * t + M - 9) % M for t in range(T)]
    pheno = 0.5 * a[:, at] + 0.25 * d[:, at] + noise(n, T, seed)
    if K:
        pheno = pheno + 0.3 * cov[:, :1]
    perm = qtl.permutations(n, P, seed, use=use) if P else None
    return state, pheno, cov, use, perm


_cache = {}


def case_reference(case, special=True):
    """(inputs, reference), computed once per case and shared: nothing changes it"""
    key = (case, special)
    if key not in _cache:
        state, pheno, cov, use, perm = make_case(*case, special=special)
        ref = reference_imp(state, chromstarts_of(CHROM_LENS), pheno, use, cov, perm, case[5])
        _cache[key] = ((state, pheno, cov, use, perm), ref)
    return _cache[key]
