"""The reference of the descent rows (cnf2_sweep_descent), shared by the CPU and the GPU suite: the state posterior gamma of
tests/test_origins_host.py's oracle_origins -- the oracle's alpha / beta store in numpy, per mode alpha after the emission x
beta normalised per marker, the modes weighted with exp(factors[s] - factor), masked modes, modes without a likelihood and
modes more than 40 below the total dropped, renormalised -- times origins.DESCENT_MASK, and the same gamma times the origin
and bit masks for the identities.  Fixtures are computed once per process and left unchanged."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import oracle_ped
from cnf2freq_amd import origins, synth
from test_origins_host import BIT_MASK, ORIGIN_MASK

DESCENT = origins.DESCENT_MASK.astype(np.float64)      # [8][64]


def oracle_descent(ped, threads=None):
    """dict(descent[n][M][8], origin[n][M][4], bits[n][M][6], loglik[n][C], compared): zeros where the oracle skips the
    individual; compared counts the (individual, chromosome) pairs with rows"""
    o = oracle_ped(ped)
    cs = np.asarray(ped.chromstarts)
    n, M, C = len(ped.dous), ped.n_markers, len(cs) - 1
    des, org, bits = np.zeros((n, M, 8)), np.zeros((n, M, 4)), np.zeros((n, M, 6))
    ll = np.zeros((n, C))
    ok = np.zeros((n, C), bool)

    def work(j):
        ind = int(ped.dous[j])
        for c in range(C):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            res = o.sweep_ind(ind, int(ped.gen[ind]), first=first, last=last, mode=2, dosage=False, keep_store=True)
            factor = res["factor"]
            ll[j, c] = factor
            if not res["ok"] or not (factor >= -1e15):
                continue
            fw = res["fwbw"]
            sl = slice(first, last + 1)
            gamma = np.zeros((last - first + 1, 64))
            wsum = 0.0
            for s in range(8):
                fs = res["factors"][s]
                if fs < -1e29 or not (fs > -1e14) or factor - fs > 40.0:
                    continue
                gam = fw[s, sl, 2] * fw[s, sl, 1]
                w = np.exp(fs - factor)
                gamma += w * gam / gam.sum(axis=1, keepdims=True)
                wsum += w
            if not wsum > 0:
                continue
            ok[j, c] = True
            gamma /= wsum
            des[j, sl] = gamma @ DESCENT.T
            org[j, sl] = gamma @ ORIGIN_MASK.T
            bits[j, sl] = gamma @ BIT_MASK.T

    threads = threads or max(1, min(16, len(os.sched_getaffinity(0)), n))
    with ThreadPoolExecutor(threads) as ex:      # (the oracle's C code is reentrant and ctypes drops the GIL)
        list(ex.map(work, range(n)))
    return dict(descent=des, origin=org, bits=bits, loglik=ll, compared=int(ok.sum()))


def check_identities(descent, origin_bits, atol=1e-12):
    """d0 + d1 = 1 - bits[0], d2 + d3 = bits[0], d4 + d5 = 1 - bits[3], d6 + d7 = bits[3] on the rows that are not all zero,
    and each side sums to 1"""
    d, b = np.asarray(descent), np.asarray(origin_bits)
    live = d.sum(axis=-1) > 0
    for lo, t in ((0, 0), (4, 3)):
        np.testing.assert_allclose((d[..., lo] + d[..., lo + 1])[live], 1.0 - b[..., t][live], rtol=0, atol=atol)
        np.testing.assert_allclose((d[..., lo + 2] + d[..., lo + 3])[live], b[..., t][live], rtol=0, atol=atol)
        np.testing.assert_allclose(d[..., lo:lo + 4].sum(axis=-1)[live], 1.0, rtol=0, atol=atol)
    assert np.all(d >= 0)


# the phased founder cross of the planted-truth checks
FOUNDER_ARGS = (3, 12, 17, 2, 777, 0.2, 0.98)
_CACHE = {}


def founder_cross(args=FOUNDER_ARGS):
    """(pedigree, descent_truth[n][2][M], oracle rows as oracle_descent returns them), once per argument tuple"""
    if args not in _CACHE:
        ped, truth = synth.make_founder_cross(*args)
        _CACHE[args] = (ped, truth, oracle_descent(ped))
    return _CACHE[args]


def truth_shares(descent, truth):
    """per side, the share of cells (individual, marker) whose arg-max class is the true one"""
    cls, _ = origins.descent_calls(descent)
    return [float((cls[:, :, s] == truth[:, s]).mean()) for s in range(2)]
