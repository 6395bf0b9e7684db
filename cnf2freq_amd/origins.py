"""Reading the origin sweep of Context.sweep_origins (cnf2_sweep_origins): from which grandparent does each of an individual's
two alleles descend at every marker?

origin[i][m][k], k = bit 0 + 2 bit 3, is the probability that the allele from the first parent descends from that parent's
first (bit 0 = 0) or second (bit 0 = 1) parent, and likewise bit 3 for the second parent's side.  The frame is absolute
(include/cnf2hip.h): with F1 parents that list line A first, k = 0 / 3 are AA / BB and k = 1, 2 the two heterozygotes by
side.  These rows are what a QTL scan regresses on; their sums over individuals are the segregation check of a cross."""
import copy
import math

import numpy as np

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def line_genotypes(origin):
    """[..., 4] -> [..., 3] = (k0, k1 + k2, k3): both alleles from the parents' first parent, one from each, both from the
    second -- AA, AB, BB in an F2."""
    o = np.asarray(origin, np.float64)
    assert o.shape[-1] == 4
    return np.stack([o[..., 0], o[..., 1] + o[..., 2], o[..., 3]], axis=-1)


def segregation_report(origin_sum, n_contrib, chromstarts):
    """Per marker, from the sums of a sweep_origins call: a dict of arrays of length M (expected / collapsed: [M][4], [M][3]) with
      n             the individuals that contribute (n_contrib of the marker's chromosome),
      expected      origin_sum, the expected count of each of the four classes,
      collapsed     line_genotypes(origin_sum), the expected counts of the three unphased classes,
      ratio_first   the share of the first parents' gametes that carry their second parent's allele (bit 0): the
                    transmission ratio of that side, 0.5 without distortion; ratio_second likewise for bit 3,
      chi2_4        the chi-square statistic of `expected` against 1:1:1:1 (3 d.f.), p_4 its upper tail,
      chi2_3        the statistic of `collapsed` against 1:2:1 (2 d.f.), p_3 its upper tail.
    The counts are sums of probabilities, not of observations: the statistics are conservative where the data say little.
    Markers of a chromosome without contributors report NaN (n stays 0)."""
    s = np.asarray(origin_sum, np.float64)
    cs = np.asarray(chromstarts, np.int64)
    M = s.shape[0]
    assert s.shape == (M, 4) and cs[0] == 0 and cs[-1] == M and len(n_contrib) == len(cs) - 1
    n = np.repeat(np.asarray(n_contrib, np.int64), np.diff(cs))
    nn = np.where(n > 0, n, 1).astype(np.float64)
    none = n == 0
    col = line_genotypes(s)
    e4 = nn[:, None] * np.array([0.25, 0.25, 0.25, 0.25])
    e3 = nn[:, None] * np.array([0.25, 0.5, 0.25])
    chi4 = ((s - e4) ** 2 / e4).sum(axis=1)
    chi3 = ((col - e3) ** 2 / e3).sum(axis=1)
    # upper tails in closed form: 2 d.f. exp(-x/2); 3 d.f. erfc(sqrt(x/2)) + sqrt(2x/pi) exp(-x/2)
    p3 = np.exp(-chi3 / 2.0)
    p4 = _erfc(np.sqrt(chi4 / 2.0)) + np.sqrt(2.0 * chi4 / np.pi) * np.exp(-chi4 / 2.0)
    nan = lambda a: np.where(none.reshape((M,) + (1,) * (a.ndim - 1)), np.nan, a)
    return dict(n=n, expected=nan(s), collapsed=nan(col), ratio_first=nan((s[:, 1] + s[:, 3]) / nn),
                ratio_second=nan((s[:, 2] + s[:, 3]) / nn), chi2_4=nan(chi4), p_4=nan(p4), chi2_3=nan(chi3), p_3=nan(p3))


def information_content(origin):
    """Per marker Var_i(a_i) / 0.5 with a = k3 - k0, the additive information content of line-origin probabilities: the
    variance over the individuals of the expected additive coefficient against the 0.5 it has in an F2 whose origins are
    known.  origin[n][M][4]; skipped individuals (all-zero rows) are left out; NaN where nobody is left."""
    o = np.asarray(origin, np.float64)
    assert o.ndim == 3 and o.shape[2] == 4
    a = o[:, :, 3] - o[:, :, 0]
    there = o.sum(axis=2) > 0
    cnt = there.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(there, a, 0.0).sum(axis=0) / cnt
        var = np.where(there, (a - mean) ** 2, 0.0).sum(axis=0) / cnt
    return var / 0.5


def linked_pairs(sel, chromstarts):
    """pairs[n_pairs][2] (int32): the pairs j < k of indices into sel (strictly ascending marker indices) whose markers lie on
    one chromosome, in ascending j, then ascending k -- the rows of Context.sweep_pairs (cnf2_linked_pairs)."""
    sel = np.asarray(sel, np.int64)
    cs = np.asarray(chromstarts, np.int64)
    if sel.ndim != 1 or (np.diff(sel) <= 0).any() or (len(sel) and (sel[0] < 0 or sel[-1] >= cs[-1])):
        raise ValueError("sel must be strictly ascending marker indices of the map")
    sc = np.searchsorted(cs, sel, side="right") - 1
    out = [(j, k) for j in range(len(sel)) for k in range(j + 1, len(sel)) if sc[k] == sc[j]]
    return np.asarray(out, np.int32).reshape(-1, 2)


# the cells 4 u + v of a pair row in which the side's origin differs between the loci: bit 0 of the class (the first parent's
# gamete), bit 1 (the second parent's)
_U, _V = np.divmod(np.arange(16), 4)
RECOMBINANT_FIRST = (_U & 1) != (_V & 1)
RECOMBINANT_SECOND = (_U >> 1) != (_V >> 1)


def pair_recombination(joint_sum, n_contrib, pairs, sel, chromstarts):
    """Per pair of a sweep_pairs call, from its sums: the expected share of recombinant gametes between the two loci on each
    side, read from the two-locus table.  A dict of arrays of length n_pairs: marker1, marker2 (map indices), chrom, n (the
    contributors of the chromosome), table [n_pairs][4][4] = joint_sum / n (rows: class at the first locus), first = the
    share of the first parents' gametes whose origin differs between the loci (an odd number of crossovers), second
    likewise for the second parents'.  For adjacent loci these are the means of sweep_crossovers' xi[.][0] and xi[.][3].
    NaN where a chromosome has no contributors (n stays 0)."""
    s = np.asarray(joint_sum, np.float64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    sel = np.asarray(sel, np.int64)
    cs = np.asarray(chromstarts, np.int64)
    if s.shape != (len(pairs), 16) or len(n_contrib) != len(cs) - 1:
        raise ValueError("joint_sum must be [n_pairs][16] and n_contrib [C]")
    m1, m2 = sel[pairs[:, 0]], sel[pairs[:, 1]]
    chrom = np.searchsorted(cs, m1, side="right") - 1
    if (chrom != np.searchsorted(cs, m2, side="right") - 1).any():
        raise ValueError("a pair spans two chromosomes")
    n = np.asarray(n_contrib, np.int64)[chrom]
    with np.errstate(invalid="ignore", divide="ignore"):
        table = np.where(n[:, None] > 0, s / n[:, None], np.nan)
    return dict(marker1=m1, marker2=m2, chrom=chrom, n=n, table=table.reshape(-1, 4, 4),
                first=table[:, RECOMBINANT_FIRST].sum(axis=1), second=table[:, RECOMBINANT_SECOND].sum(axis=1))


# The descent rows of Context.sweep_descent (cnf2_sweep_descent): per side a class k = 2 w + b, "the allele from this parent
# descends from that parent's par[.][w], strand b of that grandparent" -- first side k = 2 bit0 + (bit0 ? bit2 : bit1), second
# side k = 2 bit3 + (bit3 ? bit5 : bit4).  DESCENT_MASK[j][g]: state g belongs to cell j of the row (0..3 first side, 4..7 second)
_G = np.arange(64)
_B = [(_G >> t) & 1 for t in range(6)]
_K1 = 2 * _B[0] + np.where(_B[0] == 1, _B[2], _B[1])
_K2 = 2 * _B[3] + np.where(_B[3] == 1, _B[5], _B[4])
DESCENT_MASK = np.stack([_K1 == k for k in range(4)] + [_K2 == k for k in range(4)])


def descent_columns(par, dous, by="haplotype"):
    """(col[n][8] int32, grandparents): the model column of every cell of the analysed individuals' descent rows, and the records
    of the distinct grandparents in ascending order (their numbers g are the positions in that list).  Cell 4 s + 2 w + b of
    individual i belongs to grandparent par[par[dous[i]][s]][w], strand b:
      by="haplotype"   column 2 g + b: one effect per founder haplotype,
      by="founder"     column g: one effect per founder (unphased or inbred founders),
      by="line"        column w, the grandparent's position in its child's par entry.
    A side whose parent is missing or has no two recorded parents gets -1 in its four cells."""
    if by not in ("haplotype", "founder", "line"):
        raise ValueError("by must be 'haplotype', 'founder' or 'line'")
    par = np.asarray(par, np.int64).reshape(-1, 2)
    dous = np.asarray(dous, np.int64).reshape(-1)
    gp = np.full((len(dous), 2, 2), -1, np.int64)
    for s in range(2):
        p = par[dous, s]
        ok = p >= 0
        g = np.where(ok[:, None], par[np.maximum(p, 0)], -1)
        gp[:, s] = np.where((g >= 0).all(axis=1)[:, None], g, -1)
    grand = np.unique(gp[gp >= 0])
    num = np.searchsorted(grand, np.maximum(gp, 0))
    col = np.full((len(dous), 8), -1, np.int32)
    for s in range(2):
        for w in range(2):
            for b in range(2):
                c = {"haplotype": 2 * num[:, s, w] + b, "founder": num[:, s, w], "line": np.full(len(dous), w)}[by]
                col[:, 4 * s + 2 * w + b] = np.where(gp[:, s, w] >= 0, c, -1)
    return col, grand.astype(np.int32)


def descent_calls(descent):
    """(cls[..., 2], prob[..., 2]) from descent rows [..., 8]: per side the most probable class 2 w + b (int8; the lowest on
    a tie) and its probability.  A skipped individual's all-zero rows call class -1 with probability 0."""
    d = np.asarray(descent, np.float64)
    assert d.shape[-1] == 8
    sides = d.reshape(d.shape[:-1] + (2, 4))
    cls = sides.argmax(axis=-1).astype(np.int8)
    prob = sides.max(axis=-1)
    cls[~(sides.sum(axis=-1) > 0)] = -1
    return cls, prob


def with_positions(ped, positions_cM_per_chrom):
    """(ped2, is_marker): the pedigree with a column without data (alleles 0, sure 0, hw 0.5 in every row) inserted at every
    position of positions_cM_per_chrom[c] on chromosome c, and is_marker[M2], False at the inserted columns.  The origin
    rows of ped2 at the inserted columns are the posteriors at those positions: the map is Haldane, so the gaps compose
    exactly, and a column without data has a constant emission -- the rows of the real markers do not change.
    Positions outside a chromosome's first and last marker are refused (ValueError), and so is a position equal to a
    marker's (ask for the marker) or given twice."""
    cs = np.asarray(ped.chromstarts, np.int64)
    pos = np.asarray(ped.pos, np.float64)
    C = len(cs) - 1
    if len(positions_cM_per_chrom) != C:
        raise ValueError("one list of positions per chromosome: %d, not %d" % (C, len(positions_cM_per_chrom)))
    new_pos, src, starts = [], [], [0]
    for c in range(C):
        p = pos[cs[c]:cs[c + 1]]
        add = np.sort(np.asarray(positions_cM_per_chrom[c], np.float64).reshape(-1))
        if len(add):
            if not np.isfinite(add).all() or add[0] < p[0] or add[-1] > p[-1]:
                raise ValueError("chromosome %d: positions must lie between its first and last marker (%g .. %g cM)" % (c, p[0], p[-1]))
            if np.isin(add, p).any():
                raise ValueError("chromosome %d: a position equals a marker's: ask for the marker" % c)
            if (np.diff(add) == 0).any():
                raise ValueError("chromosome %d: a position is given twice" % c)
        allp = np.concatenate([p, add])
        idx = np.concatenate([np.arange(cs[c], cs[c + 1]), np.full(len(add), -1, np.int64)])
        order = np.argsort(allp, kind="stable")
        new_pos.append(allp[order])
        src.append(idx[order])
        starts.append(starts[-1] + len(allp))
    src = np.concatenate(src)
    is_marker = src >= 0
    take = np.where(is_marker, src, 0)
    ped2 = copy.copy(ped)
    ped2.pos = np.concatenate(new_pos)
    ped2.chromstarts = np.asarray(starts, np.int32)
    ped2.allele = np.where(is_marker[None, :, None], np.asarray(ped.allele)[:, take], 0).astype(np.uint8)
    ped2.sure = np.where(is_marker[None, :, None], np.asarray(ped.sure)[:, take], 0.0)
    ped2.hw = np.where(is_marker[None, :], np.asarray(ped.hw)[:, take], 0.5)
    if ped.truth is not None:
        ped2.truth = None         # (the generator does not know the inserted columns)
    return ped2, is_marker
