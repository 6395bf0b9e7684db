"""GPU suite: Viterbi decoding (cnf2_sweep_viterbi, Context.sweep_viterbi, cnf2freq_amd/viterbi.py, cnF2freq --viterbi).
logmax[s] is the max-product twin of factors[s]; the decoded path is the argmax state sequence in the best mode.  Checked
against a numpy max-product from the oracle's store (emission up to a per-marker constant, explicit 64 x 64 transition),
against brute-force enumeration of every path, against the closed form of an individual without information, for the
sweep's bookkeeping and flags, against planted crossovers, and on the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_CASES, ROOT, load_golden, load_trajectory, oracle_ped
from cnf2freq_amd import synth
from cnf2freq_amd.viterbi import crossover_calls

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
    return T


def logs(x):
    with np.errstate(divide="ignore"):
        return np.log(x)


def max_and_sum(E, Ts):
    """log max-product and log sum-product over state paths of (1/64) prod_m E[m](g_m) prod_m Ts[m](g_m, g_m+1)"""
    v = E[0] / 64.0
    a = v.copy()
    lv = la = 0.0
    for m in range(1, len(E)):
        v = (v[:, None] * Ts[m - 1]).max(axis=0) * E[m]
        a = (a @ Ts[m - 1]) * E[m]
        sv, sa = v.max(), a.sum()
        if sv <= 0 or sa <= 0:
            return -np.inf, -np.inf
        lv += np.log(sv)
        la += np.log(sa)
        v /= sv
        a /= sa
    return lv + np.log(v.max()), la + np.log(a.sum())


def path_score(E, Ts, path):
    s = np.log(1.0 / 64.0) + logs(E[0][path[0]])
    for m in range(1, len(E)):
        s += logs(Ts[m - 1][path[m - 1], path[m]]) + logs(E[m][path[m]])
    return s


def check_against_oracle(ctx, ped, got=None, o=None):
    """every individual and chromosome of `got` (default: a plain cnf2_sweep_viterbi call) against the oracle's store (`o`:
    the pedigree's oracle, where the caller keeps one)"""
    o = oracle_ped(ped) if o is None else o
    got = ctx.sweep_viterbi() if got is None else got
    cs = ped.chromstarts
    checked, worst = 0, 0.0
    for j, ind in enumerate(ped.dous):
        gen = int(ped.gen[ind])
        for c in range(len(cs) - 1):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            res = o.sweep_ind(int(ind), gen, first=first, last=last, mode=2, keep_store=True)
            sstar = int(got["shift"][j, c])
            path = got["state"][j, first:last + 1].astype(np.int64)
            if not res["ok"] or not (res["factor"] >= -1e15) or not (res["factors"] > -1e14).any():
                assert sstar == -1 and np.all(path == 0xFF)
                continue
            assert 0 <= sstar < 8 and np.all(path < 64)
            fw = res["fwbw"]
            Ts = [transition(rates(ped.pos, m)) for m in range(first, last)]
            best = None
            for s in range(8):
                fs = got["factors"][j, c, s]
                if res["factors"][s] < -1e29:
                    assert got["logmax"][j, c, s] == capi_ignored()
                    continue
                num, den = fw[s, first:last + 1, 2], fw[s, first:last + 1, 0]
                E = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
                lmax, lsum = max_and_sum(E, Ts)
                if not np.isfinite(lsum):
                    continue
                d = lmax - lsum
                assert abs((got["logmax"][j, c, s] - fs) - d) <= 1e-8 * (1 + abs(d)), (j, c, s)
                worst = max(worst, abs((got["logmax"][j, c, s] - fs) - d) / (1 + abs(d)))
                if s == sstar:
                    best = (E, lmax, d)
            assert best is not None
            E, lmax, d = best
            assert abs(path_score(E, Ts, path) - lmax) <= 1e-8 * (1 + abs(d)), (j, c)
            checked += 1
    print("logmax - factors against the oracle: largest difference %.3g of (1 + |value|) over %d (individual, chromosome) pairs" % (worst, checked))
    assert checked > 0
    return got


def capi_ignored():
    from cnf2freq_amd import capi
    return capi.IGNORED


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_viterbi_matches_oracle_goldens(capi, case):
    ped, _ = load_golden(case)
    ctx = capi.Context(0)
    ctx.upload(ped)
    check_against_oracle(ctx, ped)
    ctx.close()


def test_viterbi_matches_oracle_tied_windows(capi):
    """the ail_ties trajectory pedigree: windows with tie groups take the tied route of the sweep"""
    ped, _, _ = load_trajectory("ail_ties")
    ctx = capi.Context(0)
    ctx.upload(ped)
    tab = np.array([ctx.window_info(j)["tie"] for j in range(len(ped.dous))])
    assert (tab >= 0).any(), "the fixture should hold tied windows"
    got = check_against_oracle(ctx, ped)
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(got["factors"], plain["factors"])
    assert np.array_equal(got["loglik"], plain["loglik"])
    ctx.close()


def test_viterbi_brute_force(capi):
    """three markers: every one of the 64^3 paths of every mode enumerated"""
    ped = synth.make_random_windows(24, n_markers=3, seed=11)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_viterbi()
    cs = ped.chromstarts
    checked = 0
    for j in range(len(ped.dous)):
        for c in range(len(cs) - 1):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            if got["shift"][j, c] < 0:
                continue
            E = np.array([ctx.emission(j, m) for m in range(first, last + 1)])      # [marker][mode][64]
            Ts = [transition(rates(ped.pos, m)) for m in range(first, last)]
            lT = [logs(T) for T in Ts]
            for s in range(8):
                lm = got["logmax"][j, c, s]
                if lm <= -1e29:
                    continue
                lE = logs(E[:, s, :])
                if len(E) == 3:
                    tot = (np.log(1.0 / 64.0) + lE[0][:, None, None] + lT[0][:, :, None] + lE[1][None, :, None]
                           + lT[1][None, :, :] + lE[2][None, None, :])
                else:
                    tot = np.log(1.0 / 64.0) + lE[0] if len(E) == 1 else \
                        np.log(1.0 / 64.0) + lE[0][:, None] + lT[0] + lE[1][None, :]
                want = tot.max()
                if not np.isfinite(want):
                    continue
                assert abs(lm - want) <= 1e-9 * (1 + abs(want)), (j, c, s, lm, want)
                if s == got["shift"][j, c]:
                    path = got["state"][j, first:last + 1].astype(np.int64)
                    sc = path_score(E[:, s, :], Ts, path)
                    assert abs(sc - want) <= 1e-9 * (1 + abs(want))
                    checked += 1
    assert checked > 0
    ctx.close()


def uninformative(ctx, ped, j):
    """True if individual j's emission is the same for every state, for each mode and marker"""
    for m in range(ped.n_markers):
        e = ctx.emission(j, m)
        ok = np.all(e == e[:, :1], axis=1)
        if not ok.all():
            return False
    return True


def test_viterbi_closed_form_without_information(capi):
    """an individual whose emission does not depend on the state: the path stays in state 0, and logmax - factors is
    log(1/64) plus the log of the transition's diagonal over the gaps"""
    found = 0
    cands = [load_golden("f2_ungenotyped")[0], synth.make_f2(6, 30, 2, seed=3, missing=1.0)]
    for ped in cands:
        ctx = capi.Context(0)
        ctx.upload(ped)
        got = ctx.sweep_viterbi()
        cs = ped.chromstarts
        for j in range(len(ped.dous)):
            if not uninformative(ctx, ped, j):
                continue
            for c in range(len(cs) - 1):
                first, last = int(cs[c]), int(cs[c + 1]) - 1
                if got["shift"][j, c] < 0:
                    continue
                found += 1
                assert np.all(got["state"][j, first:last + 1] == 0)
                lm = got["logmax"][j, c]
                act = lm > -1e29
                top = lm[act].max()
                assert got["shift"][j, c] == np.nonzero(act & (lm == top))[0][0]
                want = np.log(1.0 / 64.0) + sum(np.log(1.0 - rates(ped.pos, m)).sum() for m in range(first, last))
                for s in np.nonzero(act)[0]:
                    assert abs(lm[s] - got["factors"][j, c, s] - want) <= 1e-10 * (1 + abs(want)), (j, c, s)
        ctx.close()
    assert found > 0, "no individual without information in the fixtures"


def test_viterbi_bookkeeping(capi):
    import torch
    ped = synth.make_outbred3(6, 4, 60, 2, seed=31, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n = len(ped.dous)
    base = ctx.sweep_viterbi()
    for fs in (False, True):
        r = base if not fs else ctx.sweep_viterbi(full_spill=True)
        plain = ctx.sweep(dosage=False, full_spill=fs)
        assert np.array_equal(r["factors"], plain["factors"])
        assert np.array_equal(r["loglik"], plain["loglik"])
    act = base["logmax"] > -1e29
    assert act.any()
    assert np.all(base["logmax"][act] <= base["factors"][act] + 1e-9 * np.abs(base["factors"][act]))
    live = base["shift"] >= 0
    assert np.all(base["path_logpost"][live] <= 1e-9) and np.all(np.isnan(base["path_logpost"][~live]))
    keys = ("factors", "loglik", "logmax", "state", "shift")
    for r in (ctx.sweep_viterbi(), ctx.sweep_viterbi(static_jobs=True)):
        for k in keys:
            assert np.array_equal(r[k], base[k], equal_nan=True), k
    a, b = ctx.sweep_viterbi(0, n // 3), ctx.sweep_viterbi(n // 3, n)
    for k in keys:
        assert np.array_equal(np.concatenate([a[k], b[k]]), base[k]), k
    # other kernels for the same decoding: equal to rounding; where the paths differ, their scores agree
    cs = ped.chromstarts
    for kw in (dict(full_spill=True), dict(ties_general=True)):
        r = ctx.sweep_viterbi(**kw)
        np.testing.assert_allclose(r["logmax"], base["logmax"], rtol=1e-12)
        diff = np.nonzero(np.any(r["state"] != base["state"], axis=1))[0]
        for j in diff:
            for c in range(len(cs) - 1):
                first, last = int(cs[c]), int(cs[c + 1]) - 1
                p0, p1 = base["state"][j, first:last + 1], r["state"][j, first:last + 1]
                if np.array_equal(p0, p1):
                    continue
                s0, s1 = base["shift"][j, c], r["shift"][j, c]
                E0 = np.array([ctx.emission(j, m)[s0] for m in range(first, last + 1)])
                E1 = np.array([ctx.emission(j, m)[s1] for m in range(first, last + 1)])
                Ts = [transition(rates(ped.pos, m)) for m in range(first, last)]
                a0, a1 = path_score(E0, Ts, p0.astype(int)), path_score(E1, Ts, p1.astype(int))
                assert abs(a0 - a1) <= 1e-12 * (1 + abs(a0)), (j, c)
    # device outputs
    dev = torch.device("cuda", 0)
    C_, M = ctx.n_chrom, ctx.n_markers
    t = dict(factors=torch.empty((n, C_, 8), dtype=torch.float64, device=dev),
             loglik=torch.empty((n, C_), dtype=torch.float64, device=dev),
             logmax=torch.empty((n, C_, 8), dtype=torch.float64, device=dev),
             state=torch.empty((n, M), dtype=torch.uint8, device=dev),
             shift=torch.empty((n, C_), dtype=torch.int32, device=dev))
    import ctypes as C
    rc = ctx.L.cnf2_sweep_viterbi(ctx.h, 0, n, *[C.c_void_p(t[k].data_ptr()) for k in keys], capi.OUT_DEVICE)
    assert rc == 0, ctx.L.cnf2_last_error(ctx.h)
    ctx.sync()
    for k in keys:
        assert np.array_equal(t[k].cpu().numpy(), base[k]), k
    ctx.close()


def test_viterbi_factors_bit_equal_f2(capi):
    """an F2 (both parents homozygous everywhere: the producer's specialised forms) over long chromosomes"""
    ped = synth.make_f2(40, 400, 2, seed=2)
    ctx = capi.Context(0)
    ctx.upload(ped)
    for fs in (False, True):
        r, plain = ctx.sweep_viterbi(full_spill=fs), ctx.sweep(dosage=False, full_spill=fs)
        assert np.array_equal(r["factors"], plain["factors"])
        assert np.array_equal(r["loglik"], plain["loglik"])
        assert np.all(r["shift"] >= 0) and np.all(r["path_logpost"] <= 1e-9)
    ctx.close()


def test_crossover_calls_helper():
    state = np.array([[0, 1, 1, 9, 11], [0xFF, 0xFF, 0xFF, 0, 0]], np.uint8)
    calls = crossover_calls(state, [0, 3, 5])
    want = [(0, 0, 0, 0), (0, 1, 3, 1)]
    assert [tuple(r) for r in calls] == want


def test_planted_crossovers(capi):
    """F2 with few errors: the decoded crossovers of the two meioses that made the individuals (columns 0 and 3, judged
    together: they are exchangeable) match the planted ones within +-2 intervals"""
    n, M = 2000, 500
    ped = synth.make_f2(n, M, 1, seed=77, chrom_cm=150.0, sure=0.001)
    pos, starts = np.array(ped.pos), np.array(ped.chromstarts)
    g0 = synth._meiosis(77, 1, n, pos, starts)
    g1 = synth._meiosis(77, 2, n, pos, starts)
    true = np.diff(g0.astype(np.int8), axis=1) != 0
    true1 = np.diff(g1.astype(np.int8), axis=1) != 0
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_viterbi()
    calls = crossover_calls(got["state"], ped.chromstarts)
    calls = calls[(calls[:, 3] == 0) | (calls[:, 3] == 3)]
    dec = np.zeros((n, true.shape[1]), np.int32)
    np.add.at(dec, (calls[:, 0], calls[:, 2]), 1)
    planted = true.astype(np.int32) + true1.astype(np.int32)
    n_true, n_dec = int(planted.sum()), int(dec.sum())

    def matched(a, b):
        hits = 0
        for i, m in zip(*np.nonzero(a)):
            lo, hi = max(0, m - 2), min(b.shape[1], m + 3)
            hits += min(int(a[i, m]), int(b[i, lo:hi].sum()))
        return hits
    rec, prec = matched(planted, dec) / n_true, matched(dec, planted) / max(n_dec, 1)
    print("planted %d crossovers, decoded %d; matched %.3f of planted, %.3f of decoded" % (n_true, n_dec, rec, prec))
    assert abs(n_dec - n_true) <= 0.05 * n_true
    assert rec >= 0.9 and prec >= 0.9
    ctx.close()


# ---------------------------------------------------------------------------------------------- command line
EXE = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
DEMO = os.path.join(ROOT, "tests", "golden", "demo")


def run_demo(tmp_path, *extra, check=True):
    args = [EXE, "--mapfile", os.path.join(DEMO, "demoplantimpute.map"), "--pedfile", os.path.join(DEMO, "demoplantimpute.ped"),
            "--genfile", os.path.join(DEMO, "demoplantimpute.gen"), "--count", "2", "--quiet", *extra]
    return subprocess.run(args, capture_output=True, text=True, timeout=600, check=check, cwd=str(tmp_path))


def test_cli_viterbi(capi, tmp_path):
    out_a, out_b, vit = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "vit.txt"
    run_demo(tmp_path, "--output", str(out_a))
    run_demo(tmp_path, "--output", str(out_b), "--viterbi", str(vit))
    assert out_a.read_bytes() == out_b.read_bytes()
    old = [float(v) for v in open(os.path.join(DEMO, "demoplantimpute.map")).read().split()]
    nst = [0] + [i for i in range(1, len(old)) if old[i] < old[i - 1]] + [len(old)]
    lens = [nst[c + 1] - nst[c] for c in range(len(nst) - 1)]
    blocks = vit.read_text().split("\n\n")
    assert blocks[-1] == ""
    blocks = blocks[:-1]
    assert len(blocks) % len(lens) == 0 and len(blocks) > 0
    per = len(blocks) // len(lens)
    live = 0
    for b, blk in enumerate(blocks):
        lines = blk.split("\n")
        head = lines[0].split("\t")
        assert len(head) == 3
        name, chrom = head[0].rsplit(":", 1)
        assert int(chrom) == b // per + 1
        assert len(lines) == 1 + lens[b // per]
        if head[1] == "-":
            assert head[2] == "-" and all(ln == "\t".join("-" * 6) for ln in lines[1:])
            continue
        live += 1
        assert 0 <= int(head[1]) < 8 and float(head[2]) <= 1e-6
        bits = np.array([[int(v) for v in ln.split("\t")] for ln in lines[1:]])
        assert bits.shape[1] == 6 and np.all((bits == 0) | (bits == 1))
    assert live > 0


def test_cli_viterbi_multi_gpu_refused(capi, tmp_path):
    r = run_demo(tmp_path, "--gpus", "2", "--viterbi", str(tmp_path / "vit.txt"), check=False)
    assert r.returncode == 2
    assert "single GPU" in r.stderr
