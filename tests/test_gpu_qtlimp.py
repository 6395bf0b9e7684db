"""GPU suite: the multiple-imputation QTL scan (cnf2_qtl_scan_imp, cnf2_set_qtlimp_columns, Context.qtl_scan_imp,
qtl.sample_states / scan_imp).  The single scan's model on every draw of sampled states, combined on the likelihood scale,
checked against per-draw least squares on explicit one-hot rows with a two-pass longdouble combination
(tests/qtlimp_reference.py) at the shapes where the tiling can go wrong; what must hold to the bit; the refusals; and the
sampler's draws against the origin rows of the same sweep."""
import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, noise
from qtlimp_reference import GPU_CASES, SKIPPED_CHROM, case_reference, compare, encode, make_case, one_hot, reference_imp

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod", "coef", "rank", "rss0", "n_used", "perm_max", "draw_lod")
IDS = ["n%d_D%d_K%d_P%d" % (c[0], c[1], c[2], c[4]) for c in GPU_CASES]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens=CHROM_LENS):
    """a context that holds a map only: what cnf2_qtl_scan_imp needs"""
    cs = chromstarts_of(lens)
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in lens])
    ctx = capi.Context(0)
    ctx.upload_map(pos, cs)
    return ctx, cs


def same_bits(a, b, keys=OUT_KEYS):
    for k in keys:
        if a.get(k) is None:
            assert b.get(k) is None, k
        else:
            assert a[k].tobytes() == b[k].tobytes(), k


def device_outputs(torch, T, M, C, P, D, fill=77):
    dev = torch.device("cuda", 0)
    t = lambda *shape, dtype=torch.float64: torch.full(shape, fill, dtype=dtype, device=dev)
    return dict(lod=t(T, M), coef=t(T, M, 2), rank=t(M, dtype=torch.int32), rss0=t(T, C), n_used=t(C, dtype=torch.int32),
                perm_max=t(P, T, C) if P else None, draw_lod=t(D, T, M))


def pointers(d):
    return {k: (None if v is None else v.data_ptr()) for k, v in d.items()}


# ------------------------------------------------------------------------------------- 1. the scan on synthetic states
@pytest.mark.parametrize("case", GPU_CASES, ids=IDS)
def test_scan_against_the_yardstick(capi, case):
    import torch
    n, D, K, T, P, additive, seed = case
    (state, pheno, cov, use, perm), ref = case_reference(case)
    ctx, cs = map_context(capi)
    M, C = int(cs[-1]), len(cs) - 1
    what = "n %d D %d K %d P %d" % (n, D, K, P)
    if n == 67:
        assert ref["n_used"][SKIPPED_CHROM] == n - 3 and (ref["n_used"][:SKIPPED_CHROM] == n).all()
    if n == 130:
        assert (ref["n_used"] == 66).all()
    got = ctx.qtl_scan_imp(state, pheno, cov=cov, use=use, perm=perm, additive=additive, draw_lods=True)
    compare(got, ref, cs, additive, what)
    # a second call, every column cap, the batch cap: the same bits; without the profiles of the draws too
    same_bits(got, ctx.qtl_scan_imp(state, pheno, cov=cov, use=use, perm=perm, additive=additive, draw_lods=True))
    ctx.set_batch_jobs(5)
    for cap in (1, 4, 0):
        ctx.set_qtlimp_columns(cap)
        same_bits(got, ctx.qtl_scan_imp(state, pheno, cov=cov, use=use, perm=perm, additive=additive, draw_lods=True))
    ctx.set_batch_jobs(0)
    same_bits(got, ctx.qtl_scan_imp(state, pheno, cov=cov, use=use, perm=perm, additive=additive), OUT_KEYS[:-1])
    # device states read in place, host outputs; then device outputs
    d_state = torch.from_numpy(state).to(torch.device("cuda", 0))
    same_bits(got, ctx.qtl_scan_imp_device(n, D, d_state.data_ptr(), pheno, cov=cov, use=use, perm=perm, additive=additive,
                                           draw_lods=True))
    d = device_outputs(torch, T, M, C, P, D)
    ctx.qtl_scan_imp_device(n, D, d_state.data_ptr(), pheno, cov=cov, use=use, perm=perm, additive=additive, d_out=pointers(d))
    ctx.sync()
    same_bits(got, {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()})
    # every draw's profile against the single scan of its one-hot rows
    worst, equal = 0.0, 0
    for j in range(D):
        single = ctx.qtl_scan(one_hot(state[:, j]), pheno, cov=cov, use=use, additive=additive)
        worst = max(worst, np.abs(single["lod"] - got["draw_lod"][j]).max())
        equal += single["lod"].tobytes() == got["draw_lod"][j].tobytes()
    print("%s: draw_lod against qtl_scan of the one-hot rows %.3g; %d of %d draws equal to the bit" % (what, worst, equal, D))
    assert worst <= ATOL
    ctx.close()


# ------------------------------------------------------------------------------------- 2. what holds to the bit
def test_identical_draws_and_the_identity_permutation(capi):
    n, D, K, T, P, additive, seed = 41, 5, 2, 2, 3, False, 3
    state, pheno, cov, use, _ = make_case(n, 1, K, T, 0, additive, seed)
    ctx, cs = map_context(capi)
    k = qtl.sampled_classes(state)
    one = ctx.qtl_scan_imp(state, pheno, cov=cov, draw_lods=True)
    # D copies of the draw, each with other noise in the ignored bits: the draw's own cells
    many = ctx.qtl_scan_imp(encode(np.repeat(k, D, axis=1), 21), pheno, cov=cov, draw_lods=True)
    same_bits(one, many, OUT_KEYS[:-1])
    assert many["lod"].tobytes() == many["draw_lod"][0].tobytes()
    assert all(many["draw_lod"][j].tobytes() == one["draw_lod"][0].tobytes() for j in range(D))
    assert one["lod"].max() > 1.0
    # the identity permutation has the observed profile's maxima
    state3 = make_case(n, 3, K, T, 0, additive, seed)[0]
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3)[0], ident])
    got = ctx.qtl_scan_imp(state3, pheno, cov=cov, perm=perm)
    observed = np.stack([got["lod"][:, cs[c]:cs[c + 1]].max(axis=1) for c in range(len(cs) - 1)], axis=1)
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed)
    ctx.close()


def test_a_class_absent_in_some_draws_only(capi):
    """marker 20 has no heterozygote in draw 1 (d dropped there: rank 1, the dominance effect NaN); marker 30 has only
    heterozygotes of one kind in draw 2 (a is 0 and d the intercept: rank 0, both NaN, and that draw's LOD is 0)"""
    n, D, K, T, P, additive, seed = 41, 3, 2, 2, 3, False, 3
    state, pheno, cov, use, perm = make_case(n, D, K, T, P, additive, seed)
    k = qtl.sampled_classes(state).astype(np.int64)
    k[:, 1, 20] = np.where((k[:, 1, 20] == 1) | (k[:, 1, 20] == 2), 3, k[:, 1, 20])
    k[:, 2, 30] = 1
    state = encode(k, 5)
    ctx, cs = map_context(capi)
    ref = reference_imp(state, cs, pheno, use, cov, perm, additive)
    assert ref["rank"][20] == 1 and ref["rank"][30] == 0 and (np.delete(ref["rank"], [20, 30]) == 2).all()
    got = ctx.qtl_scan_imp(state, pheno, cov=cov, use=use, perm=perm, draw_lods=True)
    compared = compare(got, ref, cs, additive, "absent classes")
    assert not compared[20] and not compared[30] and compared.sum() == len(compared) - 2
    assert np.isnan(got["coef"][:, 20, 1]).all() and np.isfinite(got["coef"][:, 20, 0]).all()
    assert np.isnan(got["coef"][:, 30]).all() and np.all(got["draw_lod"][2, :, 30] == 0.0)
    ctx.close()


# ------------------------------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_outputs_alone(capi):
    import torch
    n, D, K, T, P, additive, seed = 41, 3, 2, 2, 3, False, 3
    state, pheno, cov, use, perm = make_case(n, D, K, T, P, additive, seed)
    ctx, cs = map_context(capi)
    M, C = int(cs[-1]), len(cs) - 1
    good = ctx.qtl_scan_imp(state, pheno, cov=cov, perm=perm, draw_lods=True)
    out_of_range, partial_draw, partial_marker, first_cell = state.copy(), state.copy(), state.copy(), state.copy()
    out_of_range[7, 1, 40] = 64
    partial_draw[7, 2, cs[3]:cs[4]] = 255                 # skipped in one draw of the chromosome only
    partial_marker[7, :, cs[4] + 5] = 255                 # ... at one marker of every draw only
    first_cell[7, 0, cs[2]] = 255                         # ... in the cell the mask is read from only
    holed = pheno.copy()
    holed[6, 1] = np.nan
    twice = perm.copy()
    twice[1, 3] = twice[1, 2]
    cases = [dict(state=out_of_range), dict(state=partial_draw), dict(state=partial_marker), dict(state=first_cell),
             dict(state=np.full((n, D, M), 254, np.uint8)), dict(state=state[:, :0]), dict(state=np.zeros((n, 1025, M), np.uint8)),
             dict(pheno=holed), dict(perm=twice), dict(cov=np.zeros((n, 9)))]
    dev = torch.device("cuda", 0)
    for kw in cases:
        st = np.ascontiguousarray(kw.get("state", state))
        args = (kw.get("pheno", pheno), kw.get("cov", cov), None, kw.get("perm", perm), True)
        # host states, host outputs
        out = {k: np.full_like(v, 77) for k, v in good.items()}
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx._qtlimp_call(n, st.shape[1], st.ctypes.data_as(capi.C.c_void_p), *args, 0, out=out)
        assert all(np.all(v == 77) for v in out.values()), kw.keys()
        # device states, device outputs: the check is a kernel
        d_state = torch.from_numpy(st).to(dev) if st.size else torch.zeros(1, dtype=torch.uint8, device=dev)
        d = device_outputs(torch, T, M, C, P, max(1, st.shape[1]) if st.shape[1] <= 16 else 1)
        with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
            ctx._qtlimp_call(n, st.shape[1], capi.C.c_void_p(d_state.data_ptr()), *args,
                             capi.QTL_STATE_DEVICE | capi.OUT_DEVICE, out=pointers(d))
        ctx.sync()
        assert all(bool((v == 77).all()) for v in d.values()), kw.keys()
    with pytest.raises(capi.Cnf2Error, match=r"failed \(-2\)"):
        ctx._qtlimp_call(n, D, None, pheno, cov, None, perm, False, 0)
    # an individual skipped on a whole chromosome in every draw is no refusal
    whole = state.copy()
    whole[7, :, cs[3]:cs[4]] = 255
    ok = ctx.qtl_scan_imp(whole, pheno, cov=cov, perm=perm)
    assert ok["n_used"][3] == n - 1 and (np.delete(ok["n_used"], 3) == n).all()
    same_bits(good, ctx.qtl_scan_imp(state, pheno, cov=cov, perm=perm, draw_lods=True))
    ctx.close()


# ------------------------------------------------------------------------------------- 4. through the sweep
@pytest.fixture(scope="module")
def swept(capi):
    """make_f2(40, 30, 1, seed=7) swept once: the context, 256 draws left on the device (with a host copy) and the origin rows"""
    ped = synth.make_f2(40, 30, 1, seed=7)
    ctx = capi.Context(0)
    ctx.upload(ped)
    d_states = qtl.sample_states(ctx, 256, seed=5)
    rows = ctx.sweep_origins()["origin"]
    yield ped, ctx, d_states, d_states.cpu().numpy(), rows
    ctx.close()


def test_sampled_class_frequencies_follow_the_origin_rows(swept):
    """per individual and marker the share of the 256 draws in class k against origin[k] of the same pedigree's origin sweep:
    within 5 binomial standard deviations plus 1 / D"""
    ped, ctx, d_states, states, rows = swept
    n, D, M = states.shape
    assert (n, M) == (len(ped.dous), ped.n_markers) and D == 256 and states.dtype == np.uint8
    host_draws = ctx.sweep_sample(draws=D, seed=5)["state"]
    assert np.array_equal(host_draws, states)
    k = qtl.sampled_classes(states)
    on = k[:, 0, :] != 255
    assert np.array_equal(on, (rows != 0.0).any(axis=2)) and np.all((k == 255) == ~on[:, None, :])
    freq = np.stack([(k == c).mean(axis=1) for c in range(4)], axis=2)              # [n][M][4]
    p = np.clip(rows, 0.0, 1.0)
    bound = 5.0 * np.sqrt(p * (1.0 - p) / D) + 1.0 / D
    excess = (np.abs(freq - rows) - bound)[on]
    print("class frequencies of %d draws against the origin rows: largest |difference| %.4f, largest excess over the bound %.4f"
          % (D, np.abs(freq - rows)[on].max(), excess.max()))
    assert excess.max() <= 0.0


def test_scan_imp_on_the_swept_cross(swept):
    """qtl.scan_imp on 16 of the swept draws against the yardstick on the same states, per pattern of missing phenotypes and
    with permutations; a planted effect's peak lies inside the support interval qtl.scan gives -- on the yardstick first"""
    ped, ctx, d_states, states, rows = swept
    n, M = len(ped.dous), ped.n_markers
    cs, D, P, planted = ped.chromstarts, 16, 3, 11
    truth = ped.allele[3:, planted, :].astype(np.float64).sum(axis=1) - 3.0
    assert set(np.unique(truth)) == {-1.0, 0.0, 1.0}
    pheno = np.stack([0.5 * truth + noise(n, 1, 31)[:, 0], 0.3 * truth + noise(n, 1, 32)[:, 0]], axis=1)
    pheno[5, 1] = np.nan
    d16 = d_states[:, :D].contiguous()
    st16 = np.ascontiguousarray(states[:, :D])
    hk = qtl.scan(ctx, pheno[:, :1])
    pk = qtl.peaks(hk["lod"], ped.pos, cs, 3.0)
    assert len(pk) == 1 and pk[0]["lo"] <= planted <= pk[0]["hi"], pk
    refs = []
    for t in range(2):
        u = np.isfinite(pheno[:, t])
        yk = np.where(u, pheno[:, t], 0.0)[:, None]
        perm = qtl.permutations(n, P, 9, use=u)
        ref = reference_imp(st16, cs, yk, u)
        ref["perm_max"] = reference_imp(st16, cs, qtl.null_residuals(yk, None, u), u, None, perm)["perm_max"]
        refs.append(ref)
    best = int(np.argmax(refs[0]["lod"][0, 0]))
    print("planted %d: qtl.scan's interval %d .. %d (peak %d, LOD %.2f); the yardstick's imputation peak %d, LOD %.2f" %
          (planted, pk[0]["lo"], pk[0]["hi"], pk[0]["marker"], pk[0]["lod"], best, refs[0]["lod"][0, 0, best]))
    assert pk[0]["lo"] <= best <= pk[0]["hi"]
    got = qtl.scan_imp(ctx, pheno, permutations=P, perm_seed=9, states=d16, draw_lods=True)
    for t in range(2):
        one = dict(lod=got["lod"][t:t + 1], coef=got["coef"][t:t + 1], rank=got["rank"][t], n_used=got["n_used"][t],
                   rss0=refs[t]["rss0"], perm_max=got["perm_max"][:, t:t + 1], draw_lod=got["draw_lod"][:, t:t + 1])
        compare(one, refs[t], cs, False, "scan_imp trait %d" % t)
    assert got["n_used"][0, 0] == n and got["n_used"][1, 0] == n - 1
    found = qtl.peaks(got["lod"][:1], ped.pos, cs, 3.0, coef=got["coef"][:1])
    assert len(found) == 1 and pk[0]["lo"] <= found[0]["marker"] <= pk[0]["hi"] and found[0]["marker"] == best
    thr = qtl.thresholds(got["perm_max"])
    assert np.all(thr["genome"] >= 0.0)
    # a sweep of the call's own: the same draws (a draw depends on the seed, the individual and its number only)
    again = qtl.scan_imp(ctx, pheno, draws=D, seed=5)
    same_bits(got, again, ("lod", "coef", "rank", "n_used"))


# ------------------------------------------------------------------------------------- 5. command line
def test_cli_qtlimp(capi, tmp_path):
    """cnF2freq --qtlimp on an F2 of 14 on two chromosomes written to files: two traits with different missing values, a
    covariate, permutations.  --output is the same bytes with and without it, and the file's figures are qtl.scan_imp's for
    the same seeds to the printed digits (the state the call sees is the readers' after postmarkerdata, which
    host.Run.from_files reaches through the same readers)."""
    import os
    import subprocess
    from conftest import ROOT
    from cnf2freq_amd import host
    from test_gpu_qtl import write_f2_files
    ped = synth.make_f2(14, 9, 2, seed=3)
    n, M = len(ped.dous), ped.n_markers
    files, names = write_f2_files(ped, tmp_path)
    truth = ped.allele[3:, 4, :].astype(np.float64).sum(axis=1) - 3.0
    pheno = np.stack([truth + noise(n, 1, 5)[:, 0], noise(n, 1, 6)[:, 0]], axis=1)
    pheno[3, 1] = np.nan
    age = np.round(synth.uniform(77, np.arange(n)) * 10.0, 3)
    fmt = lambda v: "NA" if v != v else repr(float(v))
    ph = tmp_path / "pheno.txt"
    ph.write_text("id weight age height\n" + "".join("%s %s %s %s\n" % (names[i], fmt(pheno[i, 0]), fmt(age[i]), fmt(pheno[i, 1]))
                                                      for i in range(n)))
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1"]
    out_a, out_b, q = tmp_path / "a.out", tmp_path / "b.out", tmp_path / "qi.txt"
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    run("--output", str(out_a))
    run("--output", str(out_b), "--qtlimp", str(q), "--phenofile", str(ph), "--qtl-covariates", "age", "--qtl-permutations", "10",
        "--qtl-seed", "4", "--qtl-imp-draws", "5", "--qtl-imp-seed", "8")
    assert out_a.read_bytes() == out_b.read_bytes()
    blocks = q.read_text().split("\n\n")
    assert len(blocks) == 2
    rows = [ln.split("\t") for ln in blocks[0].split("\n")]
    assert len(rows) == M and all(len(r) == 4 + 3 * 2 for r in rows)
    num = lambda v: np.nan if v == "-" else float(v)
    lod = np.array([[float(r[4 + 3 * t]) for r in rows] for t in range(2)])
    coef = np.array([[[num(r[5 + 3 * t]), num(r[6 + 3 * t])] for r in rows] for t in range(2)])
    thr = np.array([[float(v) for v in ln.split("\t")[1:]] for ln in blocks[1].strip("\n").split("\n")])
    assert [ln.split("\t")[0] for ln in blocks[1].strip("\n").split("\n")] == ["weight", "height"]
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, list(ped.chromstarts), n)
    want = qtl.scan_imp(ctx, pheno, draws=5, seed=8, cov=age, permutations=10, perm_seed=4)
    ctx.close()
    r.close()
    wthr = qtl.thresholds(want["perm_max"])["genome"]
    print("file against qtl.scan_imp: lod %.3g, coef %.3g, thresholds %.3g" %
          (np.abs(lod - want["lod"]).max(), np.nanmax(np.abs(coef - want["coef"])), np.abs(thr - wthr.T).max()))
    assert [int(r_[2]) for r_ in rows] == list(np.repeat(want["n_used"][0], np.diff(ped.chromstarts)))
    assert np.array_equal([int(r_[3]) for r_ in rows], want["rank"][0])
    assert want["lod"][0].max() > 1.0 and want["n_used"][1, 0] == n - 1
    np.testing.assert_allclose(lod, want["lod"], rtol=0, atol=0.51e-5)
    assert np.array_equal(np.isnan(coef), np.isnan(want["coef"]))
    np.testing.assert_allclose(coef, want["coef"], rtol=0, atol=0.51e-5)
    np.testing.assert_allclose(thr, wthr.T, rtol=0, atol=0.51e-5)
