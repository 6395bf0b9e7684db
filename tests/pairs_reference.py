"""The yardstick of the pair sweep (cnf2_sweep_pairs): the joint origin classes of two markers of one chromosome, in numpy on
the CPU oracle's alpha / beta store.  Per shift mode the alpha after the emission of the first locus is split by origin
class into four vectors, which are carried marker by marker with the explicit 64 x 64 transition of
tests/test_gpu_crossovers.py and the oracle's path-free emission, rescaled by their common total; at a selected marker the
sixteen masked sums against beta, normalised within the mode and weighted as tests/test_origins_host.oracle_origins
weights the modes.  Shared by tests/test_pairs_host.py (CPU) and tests/test_gpu_pairs.py."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import oracle_ped
from test_gpu_crossovers import rates, transition
from test_origins_host import ORIGIN_MASK


def linked(sel, chromstarts):
    """[(j, k)]: the pairs of indices into sel on one chromosome, ascending j, then ascending k"""
    cs = np.asarray(chromstarts)
    sc = np.searchsorted(cs, np.asarray(sel), side="right") - 1
    return [(j, k) for j in range(len(sel)) for k in range(j + 1, len(sel)) if sc[j] == sc[k]]


def oracle_pairs(ped, sel=None, threads=None, emissions=None):
    """(joint[n][n_pairs][16], pairs[n_pairs][2], (individual, chromosome) jobs compared) for the markers sel (default: all);
    zeros where the oracle skips the individual on the chromosome.  emissions: a dict the caller keeps for this pedigree, in
    which the oracle's emission vectors (per individual, mode and marker: they do not depend on sel) are remembered from one
    selection to the next"""
    o = oracle_ped(ped)
    cs = np.asarray(ped.chromstarts)
    n, M, C = len(ped.dous), ped.n_markers, len(cs) - 1
    sel = np.arange(M) if sel is None else np.asarray(sel)
    pairs = linked(sel, cs)
    index = {p: i for i, p in enumerate(pairs)}
    joint = np.zeros((n, len(pairs), 16))
    ok = np.zeros((n, C), bool)
    Ts = {m: transition(rates(ped.pos, m))[0] for c in range(C) for m in range(cs[c], cs[c + 1] - 1)}
    G = range(64)

    def work(j):
        ind = int(ped.dous[j])
        for c in range(C):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            mine = [a for a in range(len(sel)) if first <= sel[a] <= last]
            res = o.sweep_ind(ind, int(ped.gen[ind]), first=first, last=last, mode=2, dosage=False, keep_store=True)
            factor = res["factor"]
            if not res["ok"] or not (factor >= -1e15):
                continue
            fw = res["fwbw"]
            acc = np.zeros((len(pairs), 16))
            wsum = np.zeros(len(pairs))
            any_mode = False
            for s in range(8):
                fs = res["factors"][s]
                if fs < -1e29 or not (fs > -1e14) or factor - fs > 40.0:
                    continue
                any_mode = True
                w = np.exp(fs - factor)
                e = {} if emissions is None else emissions.setdefault((ind, s), {})
                for ia, a in enumerate(mine[:-1]):
                    V = fw[s, sel[a], 2][None, :] * ORIGIN_MASK
                    tot = V.sum()
                    if not tot > 0:
                        continue
                    V = V / tot
                    targets = {int(sel[b]): b for b in mine[ia + 1:]}
                    for m in range(int(sel[a]) + 1, int(sel[mine[-1]]) + 1):
                        if m not in e:
                            e[m] = np.array([o.emission(ind, m, g, -1, s) for g in G])
                        V = (V @ Ts[m - 1]) * e[m][None, :]
                        tot = V.sum()
                        if not tot > 0:
                            break
                        V = V / tot
                        if m in targets:
                            J = (V * fw[s, m, 1][None, :]) @ ORIGIN_MASK.T
                            Z = J.sum()
                            if Z > 0:
                                p = index[(a, targets[m])]
                                acc[p] += w * (J / Z).reshape(16)
                                wsum[p] += w
            if not any_mode:
                continue
            ok[j, c] = True
            there = wsum > 0
            joint[j, there] += acc[there] / wsum[there, None]

    threads = threads or max(1, min(16, len(os.sched_getaffinity(0)), n))
    with ThreadPoolExecutor(threads) as ex:      # (the oracle's C code is reentrant and ctypes drops the GIL)
        list(ex.map(work, range(n)))
    return joint, np.asarray(pairs, np.int32).reshape(-1, 2), int(ok.sum())


_KEPT = {}


def oracle_pairs_of(case):
    """(pedigree, joint, pairs, compared) of a fixture with every marker selected, computed once and left unchanged"""
    from test_loo_host import fixture_ped
    if case not in _KEPT:
        ped = fixture_ped(case)
        _KEPT[case] = (ped,) + oracle_pairs(ped)
    return _KEPT[case]


def margins(joint):
    """(the class distribution at the first locus, at the second) of rows [..., 16]"""
    J = np.asarray(joint).reshape(joint.shape[:-1] + (4, 4))
    return J.sum(axis=-1), J.sum(axis=-2)


def recombinant_mass(joint):
    """(the mass with u & 1 != v & 1, with u >> 1 != v >> 1) of rows [..., 16]"""
    u, v = np.divmod(np.arange(16), 4)
    return joint[..., (u & 1) != (v & 1)].sum(axis=-1), joint[..., (u >> 1) != (v >> 1)].sum(axis=-1)
