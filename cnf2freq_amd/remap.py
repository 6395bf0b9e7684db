"""EM re-estimation of the marker map from crossover posteriors: every step is a sweep with crossover posteriors on the
device (Context.sweep_crossovers: only the [M][6] sums come back), the M-step of cnf2h_map_mstep on the host (closed form
when genrec[0] == genrec[1], a safeguarded Newton iteration otherwise) and a re-upload of the positions.  The summed window
log-likelihood that the sweep reports is the EM objective, so it cannot decrease from step to step."""
import numpy as np

from . import host

DEFAULT_GENREC = (-0.02, -0.02, -0.02)


def summed_loglik(loglik):
    """sum of the log-likelihoods of every (individual, chromosome) that is not skipped (<= CNF2_MINFACTOR or NaN)"""
    ll = np.asarray(loglik)
    ok = np.isfinite(ll) & (ll >= -1e15)
    return float(ll[ok].sum())


def estimate_map(ctx, ped, iterations=1, genrec=None):
    """`iterations` EM steps of the map of `ped` on the context (which holds ped's rows and pedigree).  Returns (positions
    after the last step, summed log-likelihood before every step and after the last one: iterations + 1 values).  The
    context is left with the new map uploaded."""
    if iterations < 1:
        raise ValueError("iterations must be at least 1")
    g = np.asarray(DEFAULT_GENREC if genrec is None else genrec, np.float64)
    cs = np.asarray(ped.chromstarts, np.int32)
    pos = np.array(ped.pos, np.float64)
    ctx.upload_map(pos, cs, g)
    lls = []
    for k in range(iterations + 1):
        r = ctx.sweep_crossovers(rows=False)
        lls.append(summed_loglik(r["loglik"]))
        if k == iterations:
            break
        pos = host.map_mstep(pos, cs, r["xo_sum"], r["n_contrib"], g)
        ctx.upload_map(pos, cs, g)
    return pos, np.array(lls)
