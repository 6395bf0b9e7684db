"""GPU suite: crossover posteriors (cnf2_sweep_crossovers, cnf2_crossover_rows) and the EM step of the map built on them
(cnf2freq_amd/remap.py, cnf2h_map_mstep).  xi_t(m) = posterior probability that state bit t flips between markers m and
m+1; checked against an independent numpy form from the oracle's alpha / beta store with an explicit 64 x 64 transition,
against the Fisher identity (the derivative of the summed log-likelihood in an interval length), against planted
crossovers, and for invariance under the sweep's flags."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_CASES, ROOT, load_golden, load_trajectory, oracle_ped
from cnf2freq_amd import synth

pytestmark = pytest.mark.gpu

BITS = np.arange(64)
TYPEGENS = np.array([1, 0, 0, 1, 0, 0])


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def rates(pos, m, genrec=(-0.02, -0.02, -0.02)):
    d = pos[m + 1] - pos[m]
    if d <= 0:
        return np.zeros(6)
    return np.array([0.5 * (1.0 - np.exp(genrec[TYPEGENS[t]] * d)) for t in range(6)])


def transition(r):
    """explicit 64 x 64 T[g, g'] = prod_t (r_t if bit t differs else 1 - r_t)"""
    diff = BITS[:, None] ^ BITS[None, :]
    T = np.ones((64, 64))
    for t in range(6):
        T *= np.where((diff >> t) & 1, r[t], 1.0 - r[t])
    return T, diff


FLIPS = [(((BITS[:, None] ^ BITS[None, :]) >> t) & 1) == 1 for t in range(6)]      # [t][g, g']: bit t differs


def oracle_xi(o, ind, gen, pos, first, last, Ts=None):
    """xi[len][6] of one individual and chromosome from the oracle's store: for every shift mode the pairwise posterior
    P(g at m, g' at m+1) = alpha_m(g) T(g, g') gamma_{m+1}(g') / (T^t alpha_m)(g'), gamma = posterior of the state; modes
    weighted by exp(factors[s] - factor) with the 40-log-unit rule.  Also returns the largest deviation of the pairwise
    posterior's margin over g' from the state posterior at m.  Ts: a dict that keeps the transition of every gap for the
    next call on the same map."""
    res = o.sweep_ind(int(ind), gen, first=first, last=last, mode=2, keep_store=True)
    nm = last - first + 1
    xi = np.zeros((nm, 6))
    worst = 0.0
    factor = res["factor"]
    if not res["ok"] or not (factor >= -1e15):
        return xi, worst
    fw = res["fwbw"]
    for s in range(8):
        fs = res["factors"][s]
        if fs < -1e29 or factor - fs > 40.0:
            continue
        ws = np.exp(fs - factor)
        for k in range(nm - 1):
            m = first + k
            r = rates(pos, m)
            if not r.any():
                continue
            if Ts is None:
                T = transition(r)[0]
            else:
                if m not in Ts:
                    Ts[m] = transition(r)[0]
                T = Ts[m]
            al = fw[s, m, 2]
            gam = fw[s, m + 1, 2] * fw[s, m + 1, 1]
            if gam.sum() <= 0:
                continue
            gam = gam / gam.sum()
            am = al @ T
            cond = np.where(am > 0, gam / np.where(am > 0, am, 1.0), 0.0)
            J = al[:, None] * T * cond[None, :]
            for t in range(6):
                xi[k, t] += ws * J[FLIPS[t]].sum()
            st = fw[s, m, 2] * fw[s, m, 1]
            if st.sum() > 0:
                worst = max(worst, np.abs(J.sum(axis=1) - st / st.sum()).max())
    return xi, worst


def summed_loglik(ll):
    ok = np.isfinite(ll) & (ll >= -1e15)
    return ll[ok].sum()


def oracle_xi_all(ped):
    """xi[n][M][6] of every analysed individual on every chromosome (oracle_xi; zeros where the oracle skips the pair)"""
    o = oracle_ped(ped)
    cs = ped.chromstarts
    want = np.zeros((len(ped.dous), ped.n_markers, 6))
    Ts = {}
    for j, ind in enumerate(ped.dous):
        for c in range(len(cs) - 1):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            want[j, first:last + 1], worst = oracle_xi(o, ind, int(ped.gen[ind]), ped.pos, first, last, Ts)
            assert worst < 1e-10, "pairwise posterior does not sum to the state posterior"
    return want


def check_against_oracle(ctx, ped, got=None, want=None, rows=True):
    """every individual and chromosome of `got` (default: a plain cnf2_sweep_crossovers call) and, with `rows`, of
    cnf2_crossover_rows against oracle_xi (`want`: oracle_xi_all(ped) computed earlier)"""
    got = ctx.sweep_crossovers() if got is None else got
    want = oracle_xi_all(ped) if want is None else want
    cs = ped.chromstarts
    checked, worst = 0, 0.0
    for j in range(len(ped.dous)):
        for c in range(len(cs) - 1):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            fused = got["xo"][j, first:last + 1]
            np.testing.assert_allclose(fused, want[j, first:last + 1], rtol=1e-9, atol=1e-12)
            if rows:
                np.testing.assert_allclose(ctx.crossover_rows(j, c), want[j, first:last + 1], rtol=1e-9, atol=1e-12)
            assert np.all(fused[-1] == 0.0)
            checked += int(want[j, first:last + 1].any())
            worst = max(worst, np.abs(fused - want[j, first:last + 1]).max())
    print("xi against the oracle: largest difference %.3g over %d (individual, chromosome) pairs with crossovers" % (worst, checked))
    assert checked > 0
    return got


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_crossovers_match_oracle_goldens(capi, case):
    ped, _ = load_golden(case)
    ctx = capi.Context(0)
    ctx.upload(ped)
    check_against_oracle(ctx, ped)
    ctx.close()


def test_crossovers_match_oracle_tied_windows(capi):
    """the ail_ties trajectory pedigree: windows with tie groups go through the tied kernels in cnf2_sweep"""
    ped, _, _ = load_trajectory("ail_ties")
    ctx = capi.Context(0)
    ctx.upload(ped)
    tab = np.array([ctx.window_info(j)["tie"] for j in range(len(ped.dous))])
    assert (tab >= 0).any(), "the fixture should hold tied windows"
    check_against_oracle(ctx, ped)
    ctx.close()


def test_factors_bit_equal_and_invariance(capi):
    ped = synth.make_outbred3(6, 4, 60, 2, seed=31, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n = len(ped.dous)
    base = ctx.sweep_crossovers()
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(base["factors"], plain["factors"])
    assert np.array_equal(base["loglik"], plain["loglik"])
    # device sums against the host sum of the per-individual rows
    np.testing.assert_allclose(base["xo_sum"], base["xo"].sum(axis=0), rtol=1e-12, atol=1e-13)
    ok = np.isfinite(base["loglik"]) & (base["loglik"] >= -1e15)
    assert np.array_equal(base["n_contrib"], ok.sum(axis=0))
    assert np.all((base["xo"] >= 0) & (base["xo"] <= 1 + 1e-12))
    for kw in (dict(static_jobs=True), dict(full_spill=True), dict(ties_general=True)):
        r = ctx.sweep_crossovers(**kw)
        np.testing.assert_allclose(r["xo"], base["xo"], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(r["xo_sum"], base["xo_sum"], rtol=1e-12, atol=1e-15)
        assert np.array_equal(r["loglik"], ctx.sweep(dosage=False, **kw)["loglik"])
    ctx.set_batch_jobs(3)
    r = ctx.sweep_crossovers()
    np.testing.assert_allclose(r["xo"], base["xo"], rtol=1e-12, atol=1e-15)
    # a split range adds up
    a = ctx.sweep_crossovers(0, n // 3)
    b = ctx.sweep_crossovers(n // 3, n)
    np.testing.assert_allclose(np.concatenate([a["xo"], b["xo"]]), base["xo"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(a["xo_sum"] + b["xo_sum"], base["xo_sum"], rtol=1e-12, atol=1e-13)
    assert np.array_equal(a["n_contrib"] + b["n_contrib"], base["n_contrib"])
    # rows=False gives the same sums
    r = ctx.sweep_crossovers(rows=False)
    assert r["xo"] is None
    np.testing.assert_allclose(r["xo_sum"], base["xo_sum"], rtol=1e-12, atol=1e-13)
    ctx.close()


def test_fisher_identity(capi):
    """d/d(dist_j) of the summed log-likelihood = sum_ind sum_t (xi_t / r_t - (1 - xi_t) / (1 - r_t)) r_t'(d)"""
    ped = synth.make_outbred3(5, 4, 40, 2, seed=5, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_crossovers()
    pos0 = np.array(ped.pos, np.float64)
    cs = ped.chromstarts
    h = 1e-4
    for m in (3, 17, int(cs[1]) + 5, int(cs[1]) + 30):
        c = int(np.searchsorted(cs, m, side="right")) - 1
        end = int(cs[c + 1])
        r = rates(pos0, m)
        d = pos0[m + 1] - pos0[m]
        g = np.full(6, -0.02)
        dr = -0.5 * g * np.exp(g * d)
        S = got["xo_sum"][m]
        C = got["n_contrib"][c]
        analytic = np.sum((S / r - (C - S) / (1 - r)) * dr)
        vals = []
        for sgn in (1, -1):
            p = pos0.copy()
            p[m + 1:end] += sgn * h
            ctx.upload_map(p, cs)
            vals.append(summed_loglik(ctx.sweep(dosage=False)["loglik"]))
        ctx.upload_map(pos0, cs)
        numeric = (vals[0] - vals[1]) / (2 * h)
        assert abs(numeric - analytic) <= 1e-5 * max(1.0, abs(analytic)), (m, numeric, analytic)
    ctx.close()


def test_planted_crossovers(capi):
    """F2 with few errors: the posterior expected number of crossovers of the two meioses that made the individuals
    (columns 0 and 3) is close to the planted number, and the posterior mass sits around each planted crossover."""
    n, M = 2000, 500
    ped = synth.make_f2(n, M, 1, seed=77, chrom_cm=150.0, sure=0.001)
    pos, starts = np.array(ped.pos), np.array(ped.chromstarts)
    g0 = synth._meiosis(77, 1, n, pos, starts)
    g1 = synth._meiosis(77, 2, n, pos, starts)
    true = np.diff(g0.astype(np.int8), axis=1) != 0
    true1 = np.diff(g1.astype(np.int8), axis=1) != 0
    n_true = int(true.sum() + true1.sum())
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_crossovers()
    xo = got["xo"]
    est = xo[:, :, 0].sum() + xo[:, :, 3].sum()
    rel = abs(est - n_true) / n_true
    print("planted %d crossovers, posterior expectation %.1f (%.2f %%)" % (n_true, est, 100 * rel))
    assert rel < 0.03
    # the two parents' meioses of an F2 are exchangeable: judge the pair by their sum around every planted crossover
    both = xo[:, :-1, 0] + xo[:, :-1, 3]
    hits, total = 0, 0
    for i, m in zip(*np.nonzero(true | true1)):
        lo, hi = max(0, m - 2), min(both.shape[1], m + 3)
        total += 1
        hits += both[i, lo:hi].sum() > 0.5
    frac = hits / total
    print("planted crossovers with posterior mass > 0.5 within +-2 intervals: %.3f" % frac)
    assert frac > 0.9
    ctx.close()


def test_em_map_monotone_and_recovers_truth(capi, monkeypatch):
    """F2 simulated on a non-uniform true map, EM started from the uniform map of the same length: the summed
    log-likelihood does not decrease and after 20 steps the interval lengths are within sampling error of the truth"""
    from cnf2freq_amd import remap
    n, M = 1500, 60
    rng = np.random.default_rng(3)
    true_steps = rng.uniform(0.4, 4.5, M)                     # M intervals: M markers + the dummy marker
    true_map = np.concatenate([[0.0], np.cumsum(true_steps)])
    monkeypatch.setattr(synth, "make_map", lambda n_chrom, mpc, chrom_cm=100.0, dummy=True:
                        (true_map.copy(), np.array([0, M + 1], np.int32)))
    ped = synth.make_f2(n, M, 1, seed=91, sure=0.001)
    true_pos = np.array(ped.pos, np.float64)
    assert np.array_equal(true_pos, true_map)
    ped.pos = np.linspace(0.0, true_map[-1], M + 1)
    ctx = capi.Context(0)
    ctx.upload(ped)
    pos, lls = remap.estimate_map(ctx, ped, 20)
    assert len(lls) == 21
    assert np.all(np.diff(lls) >= -1e-7 * np.abs(lls[1:])), lls
    # every interval: 2n meioses of the F2 parents carry the information (Haldane, r ~ d / 100)
    d_est, d_true = np.diff(pos), np.diff(true_pos)
    r = 0.5 * (1 - np.exp(-0.02 * d_true))
    se = np.sqrt(r * (1 - r) / (2 * n)) / (0.01 * np.exp(-0.02 * d_true))
    z = (d_est - d_true) / se
    print("EM 20 steps: loglik %.3f -> %.3f; |z| max %.2f, rms %.2f" % (lls[0], lls[-1], np.abs(z).max(), np.sqrt((z ** 2).mean())))
    assert np.sqrt((z ** 2).mean()) < 2.0
    assert np.abs(z).max() < 5.0
    ctx.close()


# ---------------------------------------------------------------------------------------------- command line
EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def run_demo(tmp_path, *extra, check=True):
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=600, check=check, cwd=str(tmp_path))


def test_cli_crossovers_and_remap(capi, tmp_path):
    from cnf2freq_amd import host
    out_a, out_b = tmp_path / "a.out", tmp_path / "b.out"
    run_demo(tmp_path, "--output", str(out_a))
    xo, mp = tmp_path / "xo.txt", tmp_path / "new.map"
    r = run_demo(tmp_path, "--output", str(out_b), "--crossovers", str(xo), "--remap", str(mp), "--remap-iterations", "2")
    assert out_a.read_bytes() == out_b.read_bytes()
    steps = [ln for ln in r.stderr.splitlines() if ln.startswith("remap step")]
    assert len(steps) == 3
    lls = [float(ln.split()[-1]) for ln in steps]
    assert lls[1] >= lls[0] - 1e-6 * abs(lls[0]) and lls[2] >= lls[1] - 1e-6 * abs(lls[1])
    # the map as the readers see it
    old = [float(v) for v in open(os.path.join(DEMO, "demoplantimpute.map")).read().split()]
    new = [float(v) for v in mp.read_text().split()]
    assert len(new) == len(old)
    starts = lambda p: [0] + [i for i in range(1, len(p)) if p[i] < p[i - 1]] + [len(p)]
    assert starts(new) == starts(old)
    # framing of the crossover file: per chromosome and analysed individual "name:chrom", a line per marker, a blank line
    blocks = xo.read_text().split("\n\n")
    assert blocks[-1] == ""
    blocks = blocks[:-1]
    nst = starts(old)
    lens = [nst[c + 1] - nst[c] for c in range(len(nst) - 1)]
    assert len(blocks) % len(lens) == 0 and len(blocks) > 0
    per = len(blocks) // len(lens)
    for b, blk in enumerate(blocks):
        lines = blk.split("\n")
        name, chrom = lines[0].rsplit(":", 1)
        assert int(chrom) == b // per + 1
        assert len(lines) == 1 + lens[b // per]
        vals = np.array([[float(v) for v in ln.split("\t")] for ln in lines[1:]])
        assert vals.shape[1] == 6 and np.all((vals >= 0) & (vals <= 1))
        assert np.all(vals[-1] == 0)
    # the M-step file round-trips through the shared writer too
    host.write_map(str(tmp_path / "again.map"), np.array(new), np.array(nst, np.int32))


def test_cli_multi_gpu_refused(capi, tmp_path):
    r = run_demo(tmp_path, "--gpus", "2", "--crossovers", str(tmp_path / "xo.txt"), check=False)
    assert r.returncode == 2
    assert "single GPU" in r.stderr
