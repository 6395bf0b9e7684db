"""GPU suite: posterior sampling of inheritance paths (cnf2_sweep_sample, Context.sweep_sample, cnf2freq_amd/sampling.py,
cnF2freq --sample).  Every pick of every draw is replayed with the numpy generator against the oracle's forward vectors,
logp against the exact log posterior; the draws' distribution against brute-force enumeration, the state and crossover
posteriors and the Viterbi path; the sweep's bookkeeping and flags; an F2 at size; the command line."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import stats

from conftest import GOLDEN_CASES, load_golden, load_trajectory, oracle_ped
from cnf2freq_amd import sampling, synth
from cnf2freq_amd.viterbi import crossover_calls
from test_gpu_viterbi import DEMO, rates, run_demo, transition

pytestmark = pytest.mark.gpu

ORDER = np.asarray(sampling.STATE_ORDER)
INV = np.argsort(ORDER)
TAIL = 1e-9


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def counted(factors, loglik):
    """P(s | data) of the modes the dosage rows count (0 for the others)"""
    ok = (factors > -1e14) & (factors - loglik >= -40.0)
    return np.where(ok, np.exp(np.minimum(factors - loglik, 0.0)), 0.0)


def check_picks(u, w, g, order, what):
    """u[K], w[K][n] weights by state, g[K] the chosen states: u W inside the chosen state's interval of the inverse CDF in
    `order`, within +-1e-9 W; a weight of 0 is never chosen.  Returns log(w(g) / W)."""
    K = len(g)
    inv = np.argsort(order)
    wo = w[:, order]
    cum = np.cumsum(wo, axis=1)
    W = cum[:, -1]
    pos = inv[g]
    hi = cum[np.arange(K), pos]
    wg = wo[np.arange(K), pos]
    lo = hi - wg
    t = u * W
    assert np.all(wg > 0), (what, np.nonzero(wg <= 0)[0][:5])
    bad = ~((t >= lo - 1e-9 * W) & (t < hi + 1e-9 * W))
    assert not bad.any(), (what, np.nonzero(bad)[0][:5], t[bad][:3], lo[bad][:3], hi[bad][:3])
    return np.log(wg / W)


def gap_transitions(ped):
    return {m: transition(rates(ped.pos, m)) for m in range(ped.n_markers - 1)}


def replay(ped, got, seed, inds=None, ind0=0, o=None, Ts=None):
    """every pick of every draw of the analysed individuals `inds` (local indices of `got`) against the oracle's alpha;
    logp against the exact log posterior of the drawn (mode, path).  Returns the number of (individual, chromosome) checked."""
    o = oracle_ped(ped) if o is None else o
    Ts = gap_transitions(ped) if Ts is None else Ts
    K = got["state"].shape[1]
    cs = ped.chromstarts
    M = ped.n_markers
    ks = np.arange(K)
    inds = range(got["state"].shape[0]) if inds is None else inds
    checked = 0
    for j in inds:
        ind = int(ped.dous[ind0 + j])
        for c in range(len(cs) - 1):
            first, last = int(cs[c]), int(cs[c + 1]) - 1
            sh = got["shift"][j, :, c]
            path = got["state"][j, :, first:last + 1].astype(np.int64)
            lp = got["logp"][j, :, c]
            res = o.sweep_ind(ind, int(ped.gen[ind]), first=first, last=last, mode=2, keep_store=True)
            if not res["ok"] or not (res["factor"] >= -1e15) or not (res["factors"] > -1e14).any():
                assert np.all(sh == -1) and np.all(path == 0xFF) and np.all(np.isnan(lp)), (j, c)
                continue
            assert np.all((sh >= 0) & (sh < 8)) and np.all(path < 64), (j, c)
            pw = counted(got["factors"][j, c], got["loglik"][j, c])
            u = sampling.uniforms(seed, ind0 + j, ks, M + c)
            check_picks(u, np.broadcast_to(pw, (K, 8)), sh, np.arange(8), ("mode", j, c))
            want = got["factors"][j, c, sh] - got["loglik"][j, c]
            A = res["fwbw"][:, first:last + 1, 2, :]
            L = last - first + 1
            u = sampling.uniforms(seed, ind0 + j, ks[:, None], np.arange(first, last + 1)[None, :])
            want = want + check_picks(u[:, L - 1], A[sh, L - 1], path[:, L - 1], ORDER, ("last", j, c))
            for ml in range(L - 2, -1, -1):
                T = Ts[first + ml]
                w = A[sh, ml] * T[:, path[:, ml + 1]].T
                want = want + check_picks(u[:, ml], w, path[:, ml], ORDER, ("step", j, c, ml))
            assert np.all(np.abs(lp - want) <= 1e-8 * (1 + np.abs(want))), (j, c, np.max(np.abs(lp - want)))
            checked += 1
    return checked


def many_draws(ctx, K, seed):
    """K draws per individual and chromosome, beyond the 1 024 of one call: calls of 1 024 draws with seeds seed, seed + 1, ..."""
    parts = [ctx.sweep_sample(draws=min(1024, K - k0), seed=seed + i) for i, k0 in enumerate(range(0, K, 1024))]
    out = dict(factors=parts[0]["factors"], loglik=parts[0]["loglik"])
    for k in ("state", "shift", "logp"):
        out[k] = np.concatenate([q[k] for q in parts], axis=1)
    return out


def binom_ok(count, n, p):
    """two-sided binomial tail probability of `count` successes in n trials >= TAIL; p exactly 0 or 1 must match exactly"""
    count, p = np.asarray(count), np.clip(np.asarray(p, dtype=np.float64), 0.0, 1.0)
    ok = np.ones(count.shape, bool)
    z, one = p == 0.0, p == 1.0
    ok[z] = count[z] == 0
    ok[one] = count[one] == n
    mid = ~(z | one)
    lo = stats.binom.cdf(count[mid], n, p[mid])
    hi = stats.binom.sf(count[mid] - 1, n, p[mid])
    ok[mid] = np.minimum(1.0, 2.0 * np.minimum(lo, hi)) >= TAIL
    return ok


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_sample_replays_on_goldens(capi, case):
    ped, _ = load_golden(case)
    ctx = capi.Context(0)
    ctx.upload(ped)
    got = ctx.sweep_sample(draws=64, seed=1234)
    assert replay(ped, got, 1234) > 0
    if case == "random_windows":
        # masked modes and modes at the floor are never drawn
        f = got["factors"]
        n_dead = int(np.sum(f <= -1e14))
        assert n_dead > 0
        sh = got["shift"]
        for j in range(sh.shape[0]):
            for c in range(sh.shape[2]):
                for s in sh[j, :, c][sh[j, :, c] >= 0]:
                    assert f[j, c, s] > -1e14
    ctx.close()


def test_sample_tied_windows(capi):
    ped, _, _ = load_trajectory("ail_ties")
    ctx = capi.Context(0)
    ctx.upload(ped)
    tab = np.array([ctx.window_info(j)["tie"] for j in range(len(ped.dous))])
    assert (tab >= 0).any(), "the fixture should hold tied windows"
    got = ctx.sweep_sample(draws=16, seed=99)
    assert replay(ped, got, 99) > 0
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(got["factors"], plain["factors"])
    assert np.array_equal(got["loglik"], plain["loglik"])
    ctx.close()


def test_sample_brute_force(capi):
    """three markers: the exact distribution over (mode, 64^3 paths) from the emission; a G-test per individual"""
    ped = synth.make_random_windows(24, n_markers=3)
    ctx = capi.Context(0)
    ctx.upload(ped)
    K = 1024
    got = ctx.sweep_sample(draws=K, seed=5)
    cs = ped.chromstarts
    assert len(cs) == 2 and cs[1] - cs[0] == 3
    Ts = [transition(rates(ped.pos, m)) for m in range(2)]
    tested = 0
    for j in range(len(ped.dous)):
        sh = got["shift"][j, :, 0]
        if sh[0] < 0:
            assert np.all(sh == -1)
            continue
        E = np.array([ctx.emission(j, m) for m in range(3)])           # [marker][mode][64]
        pw = counted(got["factors"][j, 0], got["loglik"][j, 0])
        joint = np.zeros((8, 64, 64, 64))
        for s in np.nonzero(pw > 0)[0]:
            t = (E[0, s][:, None, None] / 64.0 * Ts[0][:, :, None] * E[1, s][None, :, None] * Ts[1][None, :, :]
                 * E[2, s][None, None, :])
            joint[s] = pw[s] * t / t.sum()
        joint /= joint.sum()
        st = got["state"][j].astype(np.int64)
        cell = ((sh * 64 + st[:, 0]) * 64 + st[:, 1]) * 64 + st[:, 2]
        flat = joint.ravel()
        assert np.all(flat[cell] > 0)
        # logp of every draw is the exact log posterior of the drawn (mode, path)
        want = got["factors"][j, 0, sh] - got["loglik"][j, 0] + np.log(flat[cell] / (pw[sh] / pw.sum()))
        assert np.all(np.abs(got["logp"][j, :, 0] - want) <= 1e-9 * (1 + np.abs(want))), j
        # G-test: cells with expected count >= 5, the rest pooled
        exp_ = K * flat
        big = np.nonzero(exp_ >= 5)[0]
        hit = np.isin(cell, big)
        o_big = np.array([np.sum(cell[hit] == b) for b in big])
        o_rest = K - o_big.sum()
        e_big = exp_[big]
        e_rest = K - e_big.sum()
        O = np.concatenate([o_big, [o_rest]]) if e_rest > 1e-9 else o_big
        Ex = np.concatenate([e_big, [e_rest]]) if e_rest > 1e-9 else e_big
        if len(O) < 2:
            continue
        nz = O > 0
        G = 2.0 * np.sum(O[nz] * np.log(O[nz] / Ex[nz]))
        p = stats.chi2.sf(G, len(O) - 1)
        assert p > 1e-6, (j, G, len(O), p)
        tested += 1
    assert tested > 0
    ctx.close()


def test_sample_frequencies_match_posteriors(capi):
    """state-bit frequencies against the store's posteriors, flip frequencies against sweep_crossovers, K = 4096"""
    ped = synth.make_outbred3(3, 3, 12, 1, seed=41, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    K = 4096
    got = many_draws(ctx, K, 2024)
    xo = ctx.sweep_crossovers()
    o = oracle_ped(ped)
    cs = ped.chromstarts
    first, last = int(cs[0]), int(cs[1]) - 1
    bits = np.arange(6)
    n_checked = 0
    for j in range(len(ped.dous)):
        ind = int(ped.dous[j])
        res = o.sweep_ind(ind, int(ped.gen[ind]), first=first, last=last, mode=2, keep_store=True)
        sh = got["shift"][j, :, 0]
        if sh[0] < 0:
            continue
        pw = counted(got["factors"][j, 0], got["loglik"][j, 0])
        pw = pw / pw.sum()
        fw = res["fwbw"]
        post = np.zeros((last - first + 1, 64))
        for s in np.nonzero(pw > 0)[0]:
            q = fw[s, first:last + 1, 2, :] * fw[s, first:last + 1, 1, :]
            post += pw[s] * q / q.sum(axis=1, keepdims=True)
        pbit = (post[:, :, None] * ((np.arange(64)[:, None] >> bits) & 1)[None]).sum(axis=1)      # [marker][6]
        st = got["state"][j, :, first:last + 1].astype(np.int64)
        cnt = ((st[:, :, None] >> bits) & 1).sum(axis=0)
        ok = binom_ok(cnt, K, pbit)
        assert ok.all(), (j, np.argwhere(~ok)[:5], cnt[~ok][:5], pbit[~ok][:5])
        flips = (((st[:, 1:] ^ st[:, :-1])[:, :, None] >> bits) & 1).sum(axis=0)                  # [gap][6]
        xi = xo["xo"][j, first:last]
        ok = binom_ok(flips, K, xi)
        assert ok.all(), (j, np.argwhere(~ok)[:5], flips[~ok][:5], xi[~ok][:5])
        n_checked += 1
    assert n_checked > 0
    ctx.close()


def test_sample_agrees_with_viterbi(capi):
    """no draw above the MAP path's log posterior; a draw equal to it has its log posterior; on an informative F2 the
    number of draws equal to the MAP (mode, path) agrees with exp(path_logpost)"""
    for ped, K in ((synth.make_outbred3(3, 3, 20, 1, seed=8, random_hw=True, random_sure=True), 256),
                   (synth.make_f2(12, 6, 1, seed=21, chrom_cm=40.0, sure=0.001), 4096)):
        ctx = capi.Context(0)
        ctx.upload(ped)
        vit = ctx.sweep_viterbi()
        got = many_draws(ctx, K, 3)
        cs = ped.chromstarts
        for j in range(len(ped.dous)):
            for c in range(len(cs) - 1):
                first, last = int(cs[c]), int(cs[c + 1]) - 1
                if vit["shift"][j, c] < 0:
                    assert np.all(got["shift"][j, :, c] == -1)
                    continue
                lp, best = got["logp"][j, :, c], vit["path_logpost"][j, c]
                assert np.all(lp <= best + 1e-9), (j, c)
                same = (got["shift"][j, :, c] == vit["shift"][j, c]) & np.all(
                    got["state"][j, :, first:last + 1] == vit["state"][j, first:last + 1], axis=1)
                assert np.all(np.abs(lp[same] - best) <= 1e-9), (j, c)
                assert binom_ok(np.array([same.sum()]), K, np.array([np.exp(best)]))[0], (j, c, same.sum(), np.exp(best))
        ctx.close()


def test_sample_bookkeeping(capi):
    import torch
    ped = synth.make_outbred3(6, 4, 60, 2, seed=31, random_hw=True, random_sure=True)
    ctx = capi.Context(0)
    ctx.upload(ped)
    n = len(ped.dous)
    keys = ("factors", "loglik", "state", "shift", "logp")
    base = ctx.sweep_sample(draws=64, seed=77)
    for fs in (False, True):
        r = base if not fs else ctx.sweep_sample(draws=64, seed=77, full_spill=True)
        plain = ctx.sweep(dosage=False, full_spill=fs)
        assert np.array_equal(r["factors"], plain["factors"])
        assert np.array_equal(r["loglik"], plain["loglik"])
    assert np.all(base["shift"] >= 0)
    for r in (ctx.sweep_sample(draws=64, seed=77), ctx.sweep_sample(draws=64, seed=77, static_jobs=True)):
        for k in keys:
            assert np.array_equal(r[k], base[k], equal_nan=True), k
    a, b = ctx.sweep_sample(0, n // 3, draws=64, seed=77), ctx.sweep_sample(n // 3, n, draws=64, seed=77)
    for k in keys:
        assert np.array_equal(np.concatenate([a[k], b[k]]), base[k], equal_nan=True), k
    r5 = ctx.sweep_sample(draws=5, seed=77)
    for k in ("state", "shift", "logp"):
        assert np.array_equal(r5[k], base[k][:, :5], equal_nan=True), k
    other = ctx.sweep_sample(draws=64, seed=78)
    assert not np.array_equal(other["state"], base["state"])
    # the other kernels for the same draws: every pick replays (the draws themselves may differ in rounding)
    o = oracle_ped(ped)
    Ts = gap_transitions(ped)
    sub = list(range(0, n, 5))
    assert replay(ped, base, 77, inds=sub, o=o, Ts=Ts) > 0
    for kw in (dict(full_spill=True), dict(ties_general=True)):
        r = ctx.sweep_sample(draws=64, seed=77, **kw)
        assert replay(ped, r, 77, inds=sub, o=o, Ts=Ts) > 0
    # device outputs
    dev = torch.device("cuda", 0)
    Cn, M, K = ctx.n_chrom, ctx.n_markers, 64
    t = dict(factors=torch.empty((n, Cn, 8), dtype=torch.float64, device=dev),
             loglik=torch.empty((n, Cn), dtype=torch.float64, device=dev),
             state=torch.empty((n, K, M), dtype=torch.uint8, device=dev),
             shift=torch.empty((n, K, Cn), dtype=torch.int32, device=dev),
             logp=torch.empty((n, K, Cn), dtype=torch.float64, device=dev))
    rc = ctx.L.cnf2_sweep_sample(ctx.h, 0, n, K, 77, *[C.c_void_p(t[k].data_ptr()) for k in keys], capi.OUT_DEVICE)
    assert rc == 0, ctx.L.cnf2_last_error(ctx.h)
    ctx.sync()
    for k in keys:
        assert np.array_equal(t[k].cpu().numpy(), base[k] if k != "logp" else np.nan_to_num(base[k], nan=capi.IGNORED)), k
    # logp may be NULL
    st = np.zeros((n, 2, M), np.uint8)
    sh = np.zeros((n, 2, Cn), np.int32)
    f, ll = np.zeros((n, Cn, 8)), np.zeros((n, Cn))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert ctx.L.cnf2_sweep_sample(ctx.h, 0, n, 2, 77, p(f), p(ll), p(st), p(sh), None, 0) == 0
    assert np.array_equal(st, base["state"][:, :2]) and np.array_equal(sh, base["shift"][:, :2])
    # the draw count is checked
    for bad in (0, 1025):
        assert ctx.L.cnf2_sweep_sample(ctx.h, 0, n, bad, 77, p(f), p(ll), p(st), p(sh), None, 0) == -2
    ctx.close()


def make_f2_lengths(n, lens, seed, zero_gap, sure=0.02):
    """F2 over chromosomes of the given marker counts (the longest at 150 cM, short ones 7 cM per gap); the gap after
    marker `zero_gap` has length 0"""
    pos_l, starts = [], [0]
    for L in lens:
        step = 150.0 / L if L > 100 else 7.0
        pos_l.append(np.arange(L, dtype=np.float64) * step)
        starts.append(starts[-1] + L)
    pos = np.concatenate(pos_l)
    pos[zero_gap + 1] = pos[zero_gap]
    starts = np.array(starts, np.int32)
    par, gen, empty, row_of, dous = synth.f2_pedigree_tables(n)
    a, s, h = synth.f2_genotype_rows(0, n, pos, starts, seed=seed, sure=sure)
    M = len(pos)
    allele = np.zeros((3 + n, M, 2), np.uint8)
    sr = np.zeros((3 + n, M, 2))
    hw = np.full((3 + n, M), 0.5)
    allele[1], allele[2] = 1, 2
    sr[1:3] = sure
    allele[3:], sr[3:], hw[3:] = a, s, h
    names = ["A", "B"]
    for i in range(n):
        names += ["F2_%d" % i, "F2_%d_f" % i, "F2_%d_m" % i]
    ped = synth.Pedigree(names, par, gen, empty, row_of, allele, sr, hw, pos, starts, dous)
    ped.founder_flags()
    return ped


def test_sample_at_size(capi):
    """2 000 F2 individuals, chromosomes of 1, 2, 9, 12 and 2 501 markers (a zero-length gap in the third), K = 65: two
    backward walks.  8 strided individuals replayed; the mean number of crossovers of meioses 0 and 3 agrees with xi."""
    n = 2000
    lens = [1, 2, 9, 12, 2501]
    ped = make_f2_lengths(n, lens, seed=5, zero_gap=3 + 4)
    ctx = capi.Context(0)
    ctx.upload(ped)
    K = 65
    got = ctx.sweep_sample(draws=K, seed=11)
    plain = ctx.sweep(dosage=False)
    assert np.array_equal(got["factors"], plain["factors"]) and np.array_equal(got["loglik"], plain["loglik"])
    assert np.all(got["shift"] >= 0)
    zg = 3 + 4
    assert np.all(got["state"][:, :, zg] == got["state"][:, :, zg + 1])
    inds = list(range(0, n, n // 8))[:8]
    sub = {k: got[k][inds] for k in ("state", "shift", "logp")}
    sub.update(factors=got["factors"][inds], loglik=got["loglik"][inds])
    # replay the strided individuals: local index i of `sub` is individual inds[i]
    o = oracle_ped(ped)
    Ts = gap_transitions(ped)
    for i, j in enumerate(inds):
        one = {k: v[i:i + 1] for k, v in sub.items()}
        assert replay(ped, one, 11, inds=[0], ind0=j, o=o, Ts=Ts) == len(lens)
    # crossovers of meioses 0 and 3 over all individuals and the first 8 draws against the crossover posteriors
    M = ped.n_markers
    st = got["state"][:, :8].reshape(n * 8, M)
    calls = crossover_calls(st, ped.chromstarts)
    n_draw = np.sum((calls[:, 3] == 0) | (calls[:, 3] == 3)) / (n * 8)
    xo = ctx.sweep_crossovers(rows=False)
    n_xi = (xo["xo_sum"][:, 0].sum() + xo["xo_sum"][:, 3].sum()) / n
    assert abs(n_draw - n_xi) <= 0.01 * n_xi, (n_draw, n_xi)
    ctx.close()


def test_cli_sample(capi, tmp_path):
    out_a, out_b = tmp_path / "a.out", tmp_path / "b.out"
    s1, s2 = tmp_path / "s1.txt", tmp_path / "s2.txt"
    run_demo(tmp_path, "--output", str(out_a))
    run_demo(tmp_path, "--output", str(out_b), "--sample", str(s1), "--draws", "3", "--seed", "7")
    run_demo(tmp_path, "--sample", str(s2), "--draws", "3", "--seed", "7")
    assert out_a.read_bytes() == out_b.read_bytes()
    assert s1.read_bytes() == s2.read_bytes()
    old = [float(v) for v in open(os.path.join(DEMO, "demoplantimpute.map")).read().split()]
    nst = [0] + [i for i in range(1, len(old)) if old[i] < old[i - 1]] + [len(old)]
    lens = [nst[c + 1] - nst[c] for c in range(len(nst) - 1)]
    blocks = s1.read_text().split("\n\n")
    assert blocks[-1] == ""
    blocks = blocks[:-1]
    assert len(blocks) % (3 * len(lens)) == 0 and len(blocks) > 0
    per = len(blocks) // len(lens)
    live = 0
    for b, blk in enumerate(blocks):
        lines = blk.split("\n")
        head = lines[0].split("\t")
        assert len(head) == 4
        name, chrom = head[0].rsplit(":", 1)
        assert int(chrom) == b // per + 1
        assert int(head[1]) == b % 3
        assert len(lines) == 1 + lens[b // per]
        if head[2] == "-":
            assert head[3] == "-" and all(ln == "\t".join("-" * 6) for ln in lines[1:])
            continue
        live += 1
        assert 0 <= int(head[2]) < 8 and float(head[3]) <= 1e-6
        bits = np.array([[int(v) for v in ln.split("\t")] for ln in lines[1:]])
        assert bits.shape[1] == 6 and np.all((bits == 0) | (bits == 1))
    assert live > 0
