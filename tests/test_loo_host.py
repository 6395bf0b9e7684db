"""CPU suite of the leave-one-marker-out sweep: reading its output (cnf2freq_amd/qc.py), the C ABI's declaration and export,
the command line's option checks, and the planted-error fixture shown sound on the CPU oracle's store.  The helpers that
form loo / unlinked from the oracle are shared with the GPU suite (tests/test_gpu_loo.py)."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN_CASES, ROOT, load_golden, load_trajectory, oracle_ped
from cnf2freq_amd import qc, synth

IGNORED = -1e30


def fixture_ped(case):
    return load_golden(case)[0] if case in GOLDEN_CASES else load_trajectory(case)[0]


def oracle_loo(ped, threads=None):
    """(loo[n][M], loglik[n][C], pairs compared) from the oracle's alpha / beta store in numpy:
    loo = log sum_s exp(fs - factor) sum_g fw[s,m,0] fw[s,m,1] exp(ff[s,m,0] - ff[s,m,2]) / sum_g fw[s,m,2] fw[s,m,1]
    over the modes with a likelihood (slot 0 alpha before the emission, 1 beta, 2 alpha after it; ff their cumulative log
    scales): each term is L_s,-m / L_s, weighted with L_s / L.  CNF2_IGNORED where the oracle skips the individual or leaves
    every mode at the floor (an impossible genotype: no mode has a likelihood)."""
    o = oracle_ped(ped)
    cs = np.asarray(ped.chromstarts)
    n, M, C = len(ped.dous), ped.n_markers, len(cs) - 1
    out = np.zeros((n, M))
    ll = np.zeros((n, C))
    ok = np.zeros((n, C), bool)

    def work(j):
        ind = int(ped.dous[j])
        for c in range(C):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            res = o.sweep_ind(ind, int(ped.gen[ind]), first=first, last=last, mode=2, dosage=False, keep_store=True)
            factor = res["factor"]
            ll[j, c] = factor
            if not res["ok"] or not (factor >= -1e15) or not (res["factors"] > -1e14).any():
                out[j, first:last + 1] = IGNORED
                continue
            ok[j, c] = True
            fw, ff = res["fwbw"], res["fwbwfactors"]
            sl = slice(first, last + 1)
            val = np.zeros(last - first + 1)
            for s in range(8):
                fs = res["factors"][s]
                if fs < -1e29 or not (fs > -1e14):
                    continue
                num = (fw[s, sl, 0] * fw[s, sl, 1]).sum(axis=1) * np.exp(ff[s, sl, 0] - ff[s, sl, 2])
                den = (fw[s, sl, 2] * fw[s, sl, 1]).sum(axis=1)
                val += np.exp(fs - factor) * num / den
            out[j, sl] = np.log(val)

    threads = threads or max(1, min(16, len(os.sched_getaffinity(0)), n))
    with ThreadPoolExecutor(threads) as ex:      # (the oracle's C code is reentrant and ctypes drops the GIL)
        list(ex.map(work, range(n)))
    return out, ll, int(ok.sum())


def oracle_unlinked(ped, active):
    """unlinked[n][M] = -log(mean over the analysed modes of (1/64) sum_g e_s,m(g)) from the oracle's emission; active[n][8]"""
    o = oracle_ped(ped)
    n, M = len(ped.dous), ped.n_markers
    out = np.zeros((n, M))
    for j, ind in enumerate(ped.dous):
        for m in range(M):
            tot = sum(o.emission(int(ind), m, g, -1, s) for s in range(8) if active[j, s] for g in range(64))
            out[j, m] = -np.log(tot / (64.0 * active[j].sum()))
    return out


def planted_f2(n_ind=40, markers=30, seed=7, count=12):
    """The F2 of synth.make_f2(n_ind, markers, 1, seed) with `count` genotypes swapped to the other homozygote, each in a
    run of three equal homozygous genotypes: a double crossover within two gaps unless the genotype is wrong.  Cells
    (child j, marker m) are drawn with RandomState(seed) -- j = randint(n_ind), m = randint(2, M - 3) -- and accepted when
    the child's genotype at m is 1/1 or 2/2, both neighbours carry the same genotype and no planted cell of that child
    lies fewer than 3 markers away.  Returns (pedigree, planted[n][M] bool)."""
    ped = synth.make_f2(n_ind, markers, 1, seed=seed)
    ped.allele = ped.allele.copy()
    M = ped.n_markers
    rs = np.random.RandomState(seed)
    planted = np.zeros((n_ind, M), bool)
    while planted.sum() < count:
        j, m = rs.randint(n_ind), rs.randint(2, M - 3)
        row = ped.row_of[ped.dous[j]]
        a = ped.allele[row]
        hom = a[m, 0] == a[m, 1] and a[m, 0] in (1, 2)
        same = np.array_equal(a[m - 1], a[m]) and np.array_equal(a[m + 1], a[m])
        if not hom or not same or planted[j, max(0, m - 2):m + 3].any():
            continue
        planted[j, m] = True
    for j, m in zip(*np.nonzero(planted)):
        row = ped.row_of[ped.dous[j]]
        ped.allele[row, m] = 3 - ped.allele[row, m]
    return ped, planted


# ---------------------------------------------------------------------------------------------- qc
def test_marker_report_on_hand_made_sums():
    # two chromosomes [0, 5) with 4 contributors and [5, 6) with 2
    loo_sum = np.array([4.0, 8.0, 4.0, 40.0, 6.0, 3.0])
    unl_sum = loo_sum + np.array([2.0, 1.0, 0.0, -3.0, 4.0, 1.0]) * np.log(10.0)
    r = qc.marker_report(loo_sum, unl_sum, [4, 2], [0, 5, 6])
    assert list(r["n"]) == [4, 4, 4, 4, 4, 2]
    np.testing.assert_allclose(r["mean_cost"], [1.0, 2.0, 1.0, 10.0, 1.5, 1.5], rtol=1e-15)
    np.testing.assert_allclose(r["lod"], [2.0, 1.0, 0.0, -3.0, 4.0, 1.0], rtol=1e-12, atol=1e-12)
    # chromosome 0: median 1.5, absolute deviations 0.5 0.5 0.5 8.5 0 -> MAD 0.5
    np.testing.assert_allclose(r["z"][:5], (np.array([1.0, 2.0, 1.0, 10.0, 1.5]) - 1.5) / (1.4826 * 0.5), rtol=1e-12)
    assert r["z"][5] == 0.0            # a chromosome of one marker: MAD 0
    assert np.argmax(r["z"]) == 3


def test_marker_report_without_contributors_and_flat_chromosome():
    r = qc.marker_report(np.array([0.0, 0.0, 3.0, 3.0, 3.0]), np.zeros(5), [0, 3], [0, 2, 5])
    assert np.isnan(r["mean_cost"][:2]).all() and np.isnan(r["z"][:2]).all()
    np.testing.assert_allclose(r["mean_cost"][2:], 1.0)
    assert np.all(r["z"][2:] == 0.0)


def test_flag_genotypes_order_threshold_and_ignored():
    loo = np.array([[0.1, 6.0, 5.0, 4.999],
                    [IGNORED, IGNORED, IGNORED, IGNORED],
                    [7.5, 0.0, 0.2, 5.5]])
    got = qc.flag_genotypes(loo, 5.0)
    assert got == [(0, 1, 6.0), (0, 2, 5.0), (2, 0, 7.5), (2, 3, 5.5)]
    assert qc.flag_genotypes(loo, 100.0) == []
    # a threshold below every cost still leaves the skipped individual out
    assert len(qc.flag_genotypes(loo, -1.0)) == 8


# ---------------------------------------------------------------------------------------------- C ABI
def test_symbols_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi
    hdr = open(os.path.join(ROOT, "include", "cnf2hip.h")).read()
    L = capi.load()
    for sym, method in (("cnf2_sweep_loo", "sweep_loo"), ("cnf2_loo_rows", "loo_rows")):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        assert sym in capi.SYMBOLS
        assert hasattr(L, sym)
        assert hasattr(capi.Context, method)


# ---------------------------------------------------------------------------------------------- command line
EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def run_cli(tmp_path, *extra):
    import __graft_entry__ as g
    g.build()
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))


def test_cli_loo_refuses_two_gpus(tmp_path):
    r = run_cli(tmp_path, "--gpus", "2", "--loo", "l.txt")
    assert r.returncode == 2
    assert "single GPU" in r.stderr
    assert not (tmp_path / "l.txt").exists()


def test_cli_loo_threshold_needs_loo(tmp_path):
    r = run_cli(tmp_path, "--loo-threshold", "4")
    assert r.returncode == 2
    assert "--loo FILE" in r.stderr


# ---------------------------------------------------------------------------------------------- planted errors
@pytest.mark.parametrize("n_ind,markers,seed,low_planted,high_clean", [(40, 30, 7, 5.71, 3.30), (24, 40, 11, 6.41, 2.84)])
def test_planted_errors_stand_out_on_the_oracle(n_ind, markers, seed, low_planted, high_clean):
    """every planted cell costs more than every other cell, from the oracle's store: the fixture of the GPU test is sound"""
    ped, planted = planted_f2(n_ind, markers, seed)
    assert planted.sum() == 12
    loo, _, compared = oracle_loo(ped)
    assert compared == n_ind
    lo, hi = loo[planted].min(), loo[~planted].max()
    print("smallest planted cost %.2f, largest other cost %.2f" % (lo, hi))
    assert lo > hi
    assert abs(lo - low_planted) < 0.01 and abs(hi - high_clean) < 0.01
    flagged = qc.flag_genotypes(loo, 5.0)
    assert [(i, m) for i, m, _ in flagged] == [(int(i), int(m)) for i, m in zip(*np.nonzero(planted))]


@pytest.mark.parametrize("value", ["abc", "4x", "", "nan"])
def test_cli_loo_threshold_must_be_a_number(tmp_path, value):
    r = run_cli(tmp_path, "--loo", "l.txt", "--loo-threshold", value)
    assert r.returncode == 2
    assert "needs a number" in r.stderr
    assert not (tmp_path / "l.txt").exists()
