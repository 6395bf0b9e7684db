"""Reading the leave-one-marker-out sweep of Context.sweep_loo (cnf2_sweep_loo): which genotypes, and which markers, does the
rest of the data contradict?

loo[i][m] is the cost in nats of individual i's window data at marker m given its data at every other marker of the
chromosome; unlinked[i][m] the cost of the same data with the marker off the map.  A genotype that implies a double crossover
between close neighbours costs several nats; a marker that does not belong where the map has it costs every individual a
little, and its own-position LOD, sum_i (unlinked - loo) / ln 10, falls to zero or below."""
import numpy as np

LN10 = float(np.log(10.0))
IGNORED = -1e30
MAD_TO_SIGMA = 1.4826      # a normal distribution's standard deviation over its median absolute deviation


def marker_report(loo_sum, unlinked_sum, n_contrib, chromstarts):
    """Per marker, from the sums of a sweep_loo call: a dict of arrays of length M with
      n         the individuals that contribute (n_contrib of the marker's chromosome),
      mean_cost loo_sum / n, the mean cost per contributing individual (NaN where nobody contributes),
      lod       (unlinked_sum - loo_sum) / ln 10, the LOD of the marker's own position against "off the map",
      z         the robust z-score of mean_cost within its chromosome: (x - median) / (1.4826 MAD); 0 where the chromosome's
                MAD is 0 (also a chromosome of one marker), NaN where mean_cost is."""
    loo_sum = np.asarray(loo_sum, np.float64)
    unlinked_sum = np.asarray(unlinked_sum, np.float64)
    cs = np.asarray(chromstarts, np.int64)
    M = loo_sum.shape[0]
    assert unlinked_sum.shape == (M,) and cs[0] == 0 and cs[-1] == M and len(n_contrib) == len(cs) - 1
    n = np.repeat(np.asarray(n_contrib, np.int64), np.diff(cs))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(n > 0, loo_sum / np.maximum(n, 1), np.nan)
    z = np.full(M, np.nan)
    for c in range(len(cs) - 1):
        x = mean[cs[c]:cs[c + 1]]
        if np.isnan(x).any():
            continue
        med = np.median(x)
        mad = np.median(np.abs(x - med))
        z[cs[c]:cs[c + 1]] = (x - med) / (MAD_TO_SIGMA * mad) if mad > 0 else 0.0
    return dict(n=n, mean_cost=mean, lod=(unlinked_sum - loo_sum) / LN10, z=z)


def flag_genotypes(loo, threshold):
    """The cells of loo[n][M] at or above `threshold` nats, CNF2_IGNORED cells (skipped individuals) left out: a list of
    (individual, marker, cost) ordered by individual, then marker."""
    loo = np.asarray(loo, np.float64)
    hit = (loo != IGNORED) & (loo >= threshold)
    ii, mm = np.nonzero(hit)       # row-major: by individual, then marker
    return [(int(i), int(m), float(loo[i, m])) for i, m in zip(ii, mm)]
