"""Reading the placement profile of Context.sweep_place (cnf2_sweep_place): where does each candidate marker go?

place_sum[q][m] is the growth of the summed log-likelihood when candidate q is laid on the map at marker m, over the
individuals for which that is possible; n_zero[q][m] counts those for which it is not; null[q] is the unlinked baseline.
(place_sum - null) / ln 10 is the LOD of the position against "not on this map"."""
import numpy as np

LN10 = float(np.log(10.0))


def lod_profile(place_sum, null):
    """LOD[Q][M] = (place_sum - null) / ln 10."""
    return (np.asarray(place_sum, np.float64) - np.asarray(null, np.float64)[:, None]) / LN10


def best_positions(place_sum, n_zero, null, pos, chromstarts, drop=1.0):
    """Per candidate, among the markers with the fewest impossible individuals: the marker with the largest LOD (the first
    of equals), its chromosome and position, the LOD there, the contiguous support interval around it on that chromosome
    (markers that are eligible and within `drop` LOD of the peak; it stops at the chromosome's ends), and the best LOD of
    an eligible marker on any other chromosome (-inf where there is none).  Returns a dict of arrays of length Q: marker,
    chrom, pos, lod, support_lo, support_hi (positions), support_lo_marker, support_hi_marker, n_zero, other_lod."""
    lod = lod_profile(place_sum, null)
    n_zero = np.asarray(n_zero)
    pos = np.asarray(pos, np.float64)
    cs = np.asarray(chromstarts, np.int64)
    Q, M = lod.shape
    assert n_zero.shape == (Q, M) and pos.shape == (M,) and cs[0] == 0 and cs[-1] == M
    chrom_of = np.searchsorted(cs, np.arange(M), side="right") - 1
    out = dict(marker=np.zeros(Q, np.int64), chrom=np.zeros(Q, np.int64), pos=np.zeros(Q), lod=np.zeros(Q),
               support_lo=np.zeros(Q), support_hi=np.zeros(Q), support_lo_marker=np.zeros(Q, np.int64),
               support_hi_marker=np.zeros(Q, np.int64), n_zero=np.zeros(Q, np.int64), other_lod=np.full(Q, -np.inf))
    for q in range(Q):
        fewest = n_zero[q].min()
        eligible = n_zero[q] == fewest
        best = int(np.argmax(np.where(eligible, lod[q], -np.inf)))
        c = int(chrom_of[best])
        inside = eligible & (lod[q] >= lod[q, best] - drop)
        lo = hi = best
        while lo - 1 >= cs[c] and inside[lo - 1]:
            lo -= 1
        while hi + 1 < cs[c + 1] and inside[hi + 1]:
            hi += 1
        other = eligible & (chrom_of != c)
        out["marker"][q], out["chrom"][q], out["pos"][q], out["lod"][q] = best, c, pos[best], lod[q, best]
        out["support_lo_marker"][q], out["support_hi_marker"][q] = lo, hi
        out["support_lo"][q], out["support_hi"][q] = pos[lo], pos[hi]
        out["n_zero"][q] = fewest
        if other.any():
            out["other_lod"][q] = lod[q][other].max()
    return out
