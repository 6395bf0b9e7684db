"""The yardstick of the bootstrap scan's tests (tests/test_qtlboot_host.py, tests/test_gpu_qtlboot.py): for every replicate
the used rows are literally repeated by their counts (np.repeat) and the resampled data set goes through
qtl_reference.reference_scan, the per-marker least-squares fit in numpy.  It shares nothing with the product's weighted sums
(cnf2freq_amd/csrc/cnf2_qtlboot.h): no weights, no Schur complement, no centring.

The conditions a comparison rests on are asserted here, on the reference alone, before anything of the product runs."""
import numpy as np

from cnf2freq_amd import qtl, synth
from qtl_reference import (ATOL, CHROM_LENS, PIVOT_EXACT, PIVOT_WELL, chromstarts_of, noise, reference_scan, skip,  # noqa: F401
                           soft_rows)

ARG_GAP = 1e-6           # boot_arg is compared where the best LOD of a chromosome leads the second best by at least this
ARG_SHARE = 0.9          # ... which must hold for at least this share of the (replicate, trait, chromosome) cells


def reference_boot(origin, chromstarts, pheno, count, use=None, cov=None, additive=False, chrom_begin=0, chrom_end=None):
    """The model of include/cnf2hip.h (cnf2_qtl_scan_boot) by least squares on literally resampled rows.  A dict:
    lod[B][T][M'], boot_max[B][T][C'], boot_arg[B][T][C'] (global marker indices, -1 where unusable), gap[B][T][C'] (best minus
    second best LOD of the chromosome; inf for a single marker), n_boot[B][C'], usable[B][C'], distinct[B][C'] (individuals
    drawn at least once and not skipped), relpivot[B][M'][2], rank[B][M']."""
    o = np.asarray(origin, np.float64)
    n = o.shape[0]
    cs = np.asarray(chromstarts, np.int64)
    chrom_end = len(cs) - 1 if chrom_end is None else chrom_end
    m_lo, m_hi = int(cs[chrom_begin]), int(cs[chrom_end])
    sub = cs[chrom_begin:chrom_end + 1] - m_lo
    Cn, Mn = chrom_end - chrom_begin, m_hi - m_lo
    y = np.asarray(pheno, np.float64).reshape(n, -1)
    T = y.shape[1]
    z = None if cov is None else np.asarray(cov, np.float64).reshape(n, -1)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    count = np.asarray(count, np.int64).reshape(-1, n)
    B = count.shape[0]
    assert np.all(count >= 0) and np.all(count[:, ~use] == 0)
    out = dict(lod=np.zeros((B, T, Mn)), boot_max=np.zeros((B, T, Cn)), boot_arg=np.full((B, T, Cn), -1, np.int32),
               gap=np.full((B, T, Cn), np.inf), n_boot=np.zeros((B, Cn), np.int32), usable=np.zeros((B, Cn), bool),
               distinct=np.zeros((B, Cn), np.int32), relpivot=np.full((B, Mn, 2), np.nan), rank=np.zeros((B, Mn), np.int32))
    on = use[:, None] & (o[:, cs[chrom_begin:chrom_end]] != 0.0).any(axis=2)          # [n][C']
    for b in range(B):
        rows = np.repeat(np.arange(n), count[b])
        out["distinct"][b] = ((count[b] > 0)[:, None] & on).sum(axis=0)
        if len(rows) == 0:
            continue
        ref = reference_scan(o[rows, m_lo:m_hi], sub, y[rows], None, None if z is None else z[rows], None, additive)
        out["lod"][b], out["n_boot"][b], out["usable"][b] = ref["lod"][0], ref["n_used"], ref["usable"]
        out["relpivot"][b], out["rank"][b] = ref["relpivot"], ref["rank"]
        for c in range(Cn):
            if not ref["usable"][c]:
                continue
            seg = ref["lod"][0][:, sub[c]:sub[c + 1]]
            k = np.argmax(seg, axis=1)
            out["boot_max"][b, :, c] = seg[np.arange(T), k]
            out["boot_arg"][b, :, c] = m_lo + sub[c] + k
            if seg.shape[1] > 1:
                srt = np.sort(seg, axis=1)
                out["gap"][b, :, c] = srt[:, -1] - srt[:, -2]
    return out


def sub_range(ref, chromstarts, chrom_begin, chrom_end, base_begin=0):
    """the reference of a sub-range of chromosomes cut out of a reference of a wider one (every chromosome is fitted alone)"""
    cs = np.asarray(chromstarts, np.int64)
    m0 = cs[base_begin]
    cols = slice(chrom_begin - base_begin, chrom_end - base_begin)
    mk = slice(int(cs[chrom_begin] - m0), int(cs[chrom_end] - m0))
    r = {k: ref[k][:, :, cols] for k in ("boot_max", "boot_arg", "gap")}
    r.update({k: ref[k][:, cols] for k in ("n_boot", "usable", "distinct")})
    r.update(lod=ref["lod"][:, :, mk], relpivot=ref["relpivot"][:, mk], rank=ref["rank"][:, mk])
    return r


def conditions(ref, K, additive=False, what=""):
    """What the comparison rests on, asserted on the reference before anything runs: every replicate is usable everywhere and
    has at least K + 6 distinct individuals on every scanned chromosome (RSS1 stays away from the clamp); every marker of
    every replicate is well conditioned or exactly degenerate (the rank rule cannot go either way); at least ARG_SHARE of the
    cells have their best LOD ARG_GAP ahead.  Returns compared[B][T][C'], the cells whose boot_arg is compared."""
    assert ref["usable"].all(), what + ": a replicate is unusable"
    assert ref["distinct"].min() >= K + 6, "%s: a replicate has only %d distinct individuals" % (what, ref["distinct"].min())
    cols = [0] if additive else [0, 1]
    rp = ref["relpivot"][:, :, cols]
    assert np.all(np.isnan(rp) | (rp >= PIVOT_WELL) | (rp <= PIVOT_EXACT)), what + ": a pivot is neither well conditioned nor exactly degenerate"
    compared = ref["gap"] >= ARG_GAP
    print("%s: %d .. %d distinct individuals, smallest relative pivot %.3g, smallest gap %.3g, %.3f of the cells compared" %
          (what, ref["distinct"].min(), ref["distinct"].max(), np.nanmin(rp), ref["gap"].min(), compared.mean()))
    assert compared.mean() >= ARG_SHARE, what + ": too few cells have a clear best marker"
    return compared


def compare(got, ref, compared, what=""):
    """boot_lod (where asked for), boot_max, boot_arg and n_boot against the reference; prints every figure before it asserts"""
    err_m = np.abs(got["boot_max"] - ref["boot_max"]).max()
    err_l = np.abs(got["boot_lod"] - ref["lod"]).max() if got.get("boot_lod") is not None else 0.0
    wrong = int((got["boot_arg"] != ref["boot_arg"])[compared].sum())
    print("%s: boot_lod %.3g over %d cells, boot_max %.3g over %d, boot_arg %d of %d differ" %
          (what, err_l, ref["lod"].size, err_m, ref["boot_max"].size, wrong, int(compared.sum())))
    assert np.array_equal(got["n_boot"], ref["n_boot"]), what + " n_boot"
    assert err_l <= ATOL, what + " boot_lod"
    assert err_m <= ATOL, what + " boot_max"
    assert wrong == 0, what + " boot_arg"
    cs_ok = (got["boot_arg"] >= 0) == ref["usable"][:, None, :]
    assert cs_ok.all(), what + " usable"
    assert np.all(got["boot_max"] >= 0) and np.isfinite(got["boot_max"]).all()


# ------------------------------------------------------------------------------------------------ the cases of the issue
#        n   T  K   B  additive lens         seed
CASES = [(24, 1, 0, 5, False, CHROM_LENS, 3),           # a partial replicate tile
         (33, 3, 2, 17, False, CHROM_LENS, 4),          # individuals 0-2 skipped on one chromosome, one unused individual (NaN), a second replicate group of one
         (67, 2, 1, 33, True, CHROM_LENS, 5),           # three replicate groups; n no multiple of 4 or 16
         (130, 1, 8, 16, False, (17, 33), 9)]           # nx = QTL_NX, exactly one full replicate tile
SKIPPED_CHROM = 3


def make_case(n, T, K, B, additive, lens, seed):
    """(origin, pheno, cov, use, count) of a case: soft rows, traits with a locus each plus noise, uniform covariates, the
    counts of qtl.bootstrap_counts.  The case of 33 individuals has 0-2 skipped on chromosome SKIPPED_CHROM and individual 7
    unused with NaN phenotypes and covariates."""
    origin, _ = soft_rows(n, lens, seed)
    M = origin.shape[1]
    use = None
    if n == 33:
        origin = skip(origin, [0, 1, 2], SKIPPED_CHROM, lens)
        use = np.ones(n, bool)
        use[7] = False
    cov = synth.uniform(seed * 16 + 9, np.arange(n * K)).reshape(n, K) * 2.0 - 1.0 if K else None
    a = origin[:, :, 3] - origin[:, :, 0]
    d = origin[:, :, 1] + origin[:, :, 2]
    at = [(11 * t + M - 9) % M for t in range(T)]
    pheno = 0.8 * a[:, at] + 0.4 * d[:, at] + noise(n, T, seed)
    if K:
        pheno = pheno + 0.3 * cov[:, :1]
    if use is not None:
        pheno = np.where(use[:, None], pheno, np.nan)
        cov = None if cov is None else np.where(use[:, None], cov, np.nan)
    count = qtl.bootstrap_counts(n, B, seed, use=use)
    return origin, pheno, cov, use, count


_cache = {}


def case_reference(case):
    """(inputs, reference of the full range), computed once per case and shared: nothing changes it"""
    if case not in _cache:
        n, T, K, B, additive, lens, seed = case
        origin, pheno, cov, use, count = make_case(*case)
        ref = reference_boot(origin, chromstarts_of(lens), pheno, count, use, cov, additive)
        _cache[case] = ((origin, pheno, cov, use, count), ref)
    return _cache[case]
