"""GPU suite: the linked pair scan (cnf2_qtl_scan2_linked, Context.qtl_scan2_linked, qtl.scan2(linked=True),
cnF2freq --qtl2-linked): cnf2_qtl_scan2 with the full model on the pairs of one chromosome too, their interaction columns
taken from the joint rows of cnf2_sweep_pairs.  Checked against the least-squares fit of tests/qtl2_linked_reference.py on a
synthetic joint at the shapes of tests/test_gpu_qtl2.py, against cnf2_qtl_scan2 where the two must agree to the bit, on a
degenerate pair, for its permutations, on planted linked epistasis through a real pair sweep, and through the command line."""
import os
import subprocess

import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import ATOL, CHROM_LENS, PIVOT_DROP, PIVOT_EXACT, PIVOT_WELL, chromstarts_of, noise
from qtl2_reference import compare2, compared_pairs
from qtl2_linked_reference import linked, product_joint, reference_scan2_linked, synthetic_joint, zero_cM_case
from test_gpu_qtl2 import ALL, CASES, OUT_KEYS, make_case, map_context, same_bits, write_f2_files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


# ------------------------------------------------------------------------------------- 1. values on hand-made rows
@pytest.mark.parametrize("n,K,seed,T,P,mask,skipped,additive", CASES[:5])
def test_linked_scan_on_hand_made_rows(capi, n, K, seed, T, P, mask, skipped, additive):
    """every output against the least-squares fit with all 84 markers selected (3 486 pairs, 890 of them on one chromosome)
    and a synthetic joint; the conditions of the comparison are asserted on the reference before the product runs; the
    same bits with column tiles of 16, on a second call and from device inputs; everything but lod_full / rank_full of the
    linked pairs and the last two maxima is cnf2_qtl_scan2's, to the bit"""
    import torch
    origin, pheno, cov, use, perm = make_case(n, K, seed, T, P, mask, skipped)
    cs = chromstarts_of(CHROM_LENS)
    joint = synthetic_joint(origin, cs, ALL)
    assert joint.shape[1] == 890
    ref = reference_scan2_linked(origin, joint, cs, ALL, pheno, use, cov, perm, additive)
    compared_pairs(ref)
    ctx, _ = map_context(capi, CHROM_LENS)
    got = ctx.qtl_scan2_linked(origin, joint, ALL, pheno, cov=cov, use=use, perm=perm, additive=additive)
    compare2(got, ref, "linked, n %d K %d T %d P %d" % (n, K, T, P))
    plain = ctx.qtl_scan2(origin, ALL, pheno, cov=cov, use=use, perm=perm, additive=additive)
    same_bits(got, plain, ("lod_add", "rank_add", "rss0", "n_used"))
    two = ref["two_chrom"]
    assert got["lod_full"][:, two].tobytes() == plain["lod_full"][:, two].tobytes()
    assert got["rank_full"][two].tobytes() == plain["rank_full"][two].tobytes()
    one = ref["upper"] & ~two
    assert np.isnan(plain["lod_full"][:, one]).all() and np.isfinite(got["lod_full"][:, one]).all()
    if P:
        assert got["perm_max"][:, :, 0].tobytes() == plain["perm_max"][:, :, 0].tobytes()
        assert np.all(got["perm_max"][:, :, 1:] >= plain["perm_max"][:, :, 1:])
    same_bits(got, ctx.qtl_scan2_linked(origin, joint, ALL, pheno, cov=cov, use=use, perm=perm, additive=additive))
    ctx.set_qtl2_columns(16)
    same_bits(got, ctx.qtl_scan2_linked(origin, joint, ALL, pheno, cov=cov, use=use, perm=perm, additive=additive))
    ctx.set_qtl2_columns(0)
    d_o, d_j = torch.from_numpy(origin).cuda(), torch.from_numpy(joint).cuda()
    same_bits(got, ctx.qtl_scan2_linked_device(n, d_o.data_ptr(), d_j.data_ptr(), ALL, pheno, cov=cov, use=use, perm=perm, additive=additive))
    ctx.close()


# ------------------------------------------------------------------------------------- 2. against cnf2_qtl_scan2
def dyadic_rows(n, M, seed):
    """origin[n][M][4] with entries that are multiples of 1/8: every product of two entries and every sum of four products
    is exact"""
    w = np.floor(synth.uniform(seed, np.arange(n * M * 3)).reshape(n, M, 3) * 3.0)          # 0 .. 2 eighths each
    o = np.zeros((n, M, 4))
    o[:, :, 1:] = w / 8.0
    o[:, :, 0] = 1.0 - o[:, :, 1:].sum(axis=2)
    k = np.floor(synth.uniform(seed + 1, np.arange(n * M)).reshape(n, M) * 4.0).astype(int)   # ... and the large entry moved about
    idx = (np.arange(4)[None, None, :] + k[:, :, None]) % 4
    return np.take_along_axis(o, idx, axis=2)


@pytest.mark.parametrize("additive", [False, True])
def test_exact_product_joint_is_the_scan_on_two_chromosomes(capi, additive):
    """a joint that is the exact outer product of the rows, nobody skipped: two loci of one chromosome are fitted the bits
    that cnf2_qtl_scan2 gives the same rows on a map that puts them on two chromosomes"""
    n, T = 48, 3
    origin = dyadic_rows(n, 6, 11)
    pheno = noise(n, T, 4) + (origin[:, 1, 3] - origin[:, 1, 0])[:, None] * (origin[:, 4, 3] - origin[:, 4, 0])[:, None]
    perm = qtl.permutations(n, 2, 8)
    sel = np.array([1, 4], np.int32)
    one_map, _ = map_context(capi, (6,))
    two_map, _ = map_context(capi, (3, 3))
    joint = product_joint(origin, [0, 6], sel)
    assert joint.shape == (n, 1, 16) and np.array_equal(joint * 64.0, np.round(joint * 64.0))
    got = one_map.qtl_scan2_linked(origin, joint, sel, pheno, perm=perm, additive=additive)
    want = two_map.qtl_scan2(origin, sel, pheno, perm=perm, additive=additive)
    none = one_map.qtl_scan2(origin, sel, pheno, perm=perm, additive=additive)
    one_map.close()
    two_map.close()
    assert np.isnan(none["lod_full"]).all() and none["rank_full"][0, 1] == -1
    for k in ("lod_add", "lod_full", "rank_add", "rank_full", "perm_max"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["rank_full"][0, 1] == (3 if additive else 8) and np.all(got["lod_full"][:, 0, 1] > got["lod_add"][:, 0, 1])


# ------------------------------------------------------------------------------------- 3. a degenerate pair
def test_zero_cM_pair(capi):
    """the pair whose second locus repeats the first, with the diagonal joint of a gap of 0 cM: a2, d2 and all four interaction
    columns are dropped (E[a1 a2] = 1 - d1, E[d1 d2] = d1, the other two are zero), ranks (2, 2) and lod_full = lod_add; ranks
    compared with =="""
    lens, origin, joint, sel, pheno = zero_cM_case()
    cs = chromstarts_of(lens)
    ref = reference_scan2_linked(origin, joint, cs, sel, pheno)
    rp = ref["relpivot"]
    assert not ((rp > PIVOT_EXACT) & (rp < 100 * PIVOT_DROP)).any()
    assert (ref["rank_add"][0, 1], ref["rank_full"][0, 1]) == (2, 2)
    ctx, _ = map_context(capi, lens)
    got = ctx.qtl_scan2_linked(origin, joint, sel, pheno)
    ctx.close()
    compare2(got, ref, "the 0 cM pair", share=0.0)
    assert (got["rank_add"][0, 1], got["rank_full"][0, 1]) == (2, 2) and (got["rank_add"][0, 2], got["rank_full"][0, 2]) == (4, 8)
    assert got["lod_full"][:, 0, 1].tobytes() == got["lod_add"][:, 0, 1].tobytes()
    err = np.abs(got["lod_full"] - ref["lod_full"][0])[:, ref["upper"]].max()
    print("lod_full at the three pairs against the reference: %.3g" % err)
    assert err <= ATOL


# ------------------------------------------------------------------------------------- 4. permutations and refusals
def test_identity_permutation_and_refusals(capi):
    n, T, K = 40, 3, 2
    origin, pheno, cov, _, _ = make_case(n, K, 5, T, 0, False, False)
    use = np.ones(n, bool)
    use[4] = False
    sel = np.ascontiguousarray(ALL[::4])
    ctx, cs = map_context(capi, CHROM_LENS)
    joint = synthetic_joint(origin, cs, sel)
    ident = np.arange(n, dtype=np.int32)
    perm = np.stack([ident, qtl.permutations(n, 1, 3, use=use)[0], ident])
    got = ctx.qtl_scan2_linked(origin, joint, sel, pheno, cov=cov, use=use, perm=perm)
    ref = reference_scan2_linked(origin, joint, cs, sel, pheno, use, cov, perm)
    compare2(got, ref, "identity permutation, linked", share=0.98)
    up = ref["upper"]
    observed = np.stack([got["lod_add"][:, up].max(axis=1), got["lod_full"][:, up].max(axis=1),
                         (got["lod_full"] - got["lod_add"])[:, up].max(axis=1)], axis=1)
    assert got["perm_max"][0].tobytes() == observed.tobytes() and got["perm_max"][2].tobytes() == observed.tobytes()
    assert not np.array_equal(got["perm_max"][1], observed)
    # refused, with the outputs left alone: a NULL joint, and what cnf2_qtl_scan2 refuses in sel
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    for j_ptr, s in ((None, sel), (p(joint), [3, 2, 10]), (p(joint), [2, 2, 10]), (p(joint), [2, 10, int(cs[-1])]), (p(joint), [5])):
        s = np.asarray(s, np.int32)
        out = {k: np.full_like(v, 77) for k, v in got.items()}
        ph, cv, us, pm = ctx._qtl_inputs(n, pheno, cov, use, perm)
        rc = ctx.L.cnf2_qtl_scan2_linked(ctx.h, n, p(origin), j_ptr, len(s), p(s), T, p(ph), p(us), K, p(cv), len(pm), p(pm),
                                         *[p(out[k]) for k in OUT_KEYS], 0)
        assert rc == -2 and all(np.all(v == 77) for v in out.values()), s
    # a selection without two loci on one chromosome: the joint is not read, the result is cnf2_qtl_scan2's
    lone = np.array([0, 1, 3, 18, 34, 51], np.int32)
    assert len(linked(lone, cs)) == 0
    same_bits(ctx.qtl_scan2_linked(origin, np.zeros((n, 0, 16)), lone, pheno, cov=cov, use=use, perm=perm),
              ctx.qtl_scan2(origin, lone, pheno, cov=cov, use=use, perm=perm))
    ctx.close()


# ------------------------------------------------------------------------------------- 5. planted linked epistasis
PLANTED = (8, 20)        # two markers of chromosome 0, twelve apart, both among every second marker


def test_planted_linked_epistasis(capi):
    """An F2 of 200 with a pure a1 a2 effect of the true genotypes at two markers of one chromosome.  On the product's own
    rows and joint the reference has its best full pair of chromosome 0 within two selected loci of the planted one;
    qtl.scan2(linked=True) agrees with the reference and its lod_int exceeds the 5 % threshold of 100 permutations;
    qtl.scan2 without the flag returns the arrays of the plain calls, to the bit.
    Where the two are compared: the rows of a well-typed F2 are nearly certain, and for two loci a few cM apart the
    interaction columns come near the span of the others (at 0 cM they lie in it: zero_cM_case), with relative pivots
    between the drop rule and PIVOT_WELL.  A LOD of such a design carries the rounding of its sums times the reciprocal of
    the pivot, in the reference's least squares as in the product's factorisation, so LODs are compared, as compare2 compares
    them, at the pairs whose kept pivots are all at least PIVOT_WELL, and ranks at the pairs with no pivot within a factor 100
    of the rule.  The pairs on two chromosomes are more than half of all; the best full pair of chromosome 0 must be among the
    compared ones."""
    ped = synth.make_f2(200, 30, 2, seed=7)
    n = len(ped.dous)
    m1, m2 = PLANTED
    g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
    pheno = (1.5 * g(m1) * g(m2) + 2.0 * noise(n, 1, 31)[:, 0])[:, None]
    sel = qtl.select_every(ped.chromstarts, 2)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = ctx.sweep_origins()["origin"]
    joint = ctx.sweep_pairs(sel)["joint"]
    ref = reference_scan2_linked(rows, joint, ped.chromstarts, sel, pheno)
    rp, up = ref["relpivot"], ref["upper"]
    cmp = up & np.all(np.isnan(rp) | (rp >= PIVOT_WELL) | (rp <= PIVOT_EXACT), axis=2)
    sure = up & ~((rp > PIVOT_EXACT) & (rp < 100 * PIVOT_DROP)).any(axis=2)
    one = up & ~ref["two_chrom"]
    print("pairs %d, LODs compared at %d (%d of the %d on one chromosome), ranks at %d" % (up.sum(), cmp.sum(), (cmp & one).sum(),
                                                                                          one.sum(), sure.sum()))
    assert cmp.sum() > up.sum() // 2 and cmp[ref["two_chrom"]].all()
    rs = qtl.pair_summary(ref["lod_add"][0], ref["lod_full"][0], sel, ped.chromstarts)
    first = [r for r in rs if (r["chrom1"], r["chrom2"]) == (0, 0)][0]
    print("the reference's best full pair on chromosome 0: %s, planted %s" % (first["full"], PLANTED))
    assert abs(first["full"][0] - m1) <= 4 and abs(first["full"][1] - m2) <= 4, first       # two selected loci = 4 markers
    assert cmp[list(sel).index(first["full"][0]), list(sel).index(first["full"][1])]
    got = qtl.scan2(ctx, pheno, sel, permutations=100, seed=5, linked=True)
    assert np.array_equal(got["rank_add"][0][sure], ref["rank_add"][sure]) and np.array_equal(got["rank_full"][0][sure], ref["rank_full"][sure])
    err_a = np.abs(got["lod_add"] - ref["lod_add"][0])[:, cmp].max()
    err_f = np.abs(got["lod_full"] - ref["lod_full"][0])[:, cmp].max()
    print("qtl.scan2(linked=True) against the reference: lod_add %.3g, lod_full %.3g" % (err_a, err_f))
    assert err_a <= ATOL and err_f <= ATOL
    gs = [r for r in qtl.pair_summary(got["lod_add"], got["lod_full"], sel, ped.chromstarts) if (r["chrom1"], r["chrom2"]) == (0, 0)][0]
    assert gs["full"] == first["full"] and gs["add"] == first["add"] and abs(gs["lod_int"] - first["lod_int"]) <= ATOL
    thr = qtl.thresholds2(got["perm_max"])
    print("lod_full %.2f lod_add %.2f lod_int %.2f at %s; 5 %% thresholds add %.2f full %.2f int %.2f" % (
        gs["lod_full"], gs["lod_add"], gs["lod_int"], gs["full"], thr["add"][0, 0], thr["full"][0, 0], thr["int"][0, 0]))
    assert gs["lod_int"] > thr["int"][0, 0] > 0.0 and gs["lod_full"] > thr["full"][0, 0] > 0.0
    # without the flag: today's arrays
    d_rows = qtl.origin_rows(ctx)
    plain = qtl.scan2(ctx, pheno, sel, permutations=3, seed=5, rows=d_rows)
    direct = ctx.qtl_scan2_device(n, d_rows.data_ptr(), sel, pheno)
    for k in ("lod_add", "lod_full"):
        assert plain[k].tobytes() == direct[k].tobytes(), k
    assert np.isnan(plain["lod_full"][0][ref["upper"] & ~ref["two_chrom"]]).all()
    res = qtl.null_residuals(pheno, None, np.ones(n, bool))
    perm = qtl.permutations(n, 3, 5, use=np.ones(n, bool))
    assert plain["perm_max"].tobytes() == ctx.qtl_scan2_device(n, d_rows.data_ptr(), sel, res, perm=perm)["perm_max"].tobytes()
    ctx.close()


# ------------------------------------------------------------------------------------- 6. command line
def test_cli_qtl2_linked(capi, tmp_path):
    """cnF2freq --qtl2 --qtl2-linked on an F2 of 30 on two chromosomes written to files, as tests/test_gpu_qtl2.py's check
    (8): with --count 1 every figure of the file is qtl.scan2(linked=True)'s on host.Run.from_files of the same files, to the
    printed digits -- the chromosomes with themselves carry a full pair now --; --output is the same bytes with and without
    the options"""
    from conftest import ROOT
    from cnf2freq_amd import host
    ped = synth.make_f2(30, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n, M, cs = 30, ped.n_markers, np.asarray(ped.chromstarts)
    g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
    y = np.stack([g(2) * g(8) + noise(n, 1, 2)[:, 0], noise(n, 1, 3)[:, 0] * 4.0 + g(2)], axis=1)
    y[3, 1] = y[8, 1] = np.nan
    age = np.round(synth.uniform(5, np.arange(n)) * 10.0, 3)
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    table = ["id w age h"] + ["%s %s %s %s" % (names[i], cell(y[i, 0]), cell(age[i]), cell(y[i, 1])) for i in range(n) if i != 6]
    ph = tmp_path / "pheno.txt"
    ph.write_text("\n".join(table) + "\n")
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    base = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--phenofile", str(ph),
            "--qtl-covariates", "age", "--qtl-permutations", "25", "--qtl-seed", "4"]
    run = lambda *extra: subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
    p = lambda name: str(tmp_path / name)
    run("--output", p("a.out"), "--qtl2", p("q2.txt"), "--qtl2-every", "2")
    run("--output", p("b.out"), "--qtl2", p("q2l.txt"), "--qtl2-every", "2", "--qtl2-linked")
    read = lambda name: open(p(name), "rb").read()
    assert read("a.out") == read("b.out")
    plain_rows = [ln.split("\t") for ln in read("q2.txt").decode().split("\n\n")[0].split("\n")]
    blocks = read("q2l.txt").decode().split("\n\n")
    rows = [ln.split("\t") for ln in blocks[0].split("\n")]
    thr = [ln.split("\t") for ln in blocks[1].strip("\n").split("\n")]
    # the additive half of every line, and the whole line of a pair of two chromosomes, are the plain file's
    assert len(rows) == len(plain_rows) == 6
    for x, q in zip(rows, plain_rows):
        assert x[:9] == q[:9]
        if x[1] != x[2]:
            assert x == q
        else:
            assert q[9:] == ["-"] * 7 and "-" not in x[9:]
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    use = np.ones(n, bool)
    use[6] = False
    sel = qtl.select_every(cs, 2)
    want = qtl.scan2(ctx, y, sel, cov=np.where(use, age, 0.0), use=use, permutations=25, seed=4, linked=True)
    ctx.close()
    r.close()
    summary = qtl.pair_summary(want["lod_add"], want["lod_full"], sel, cs)
    assert len(summary) == 6 and all(s["full"] is not None for s in summary)
    worst = 0.0
    for x, s in zip(rows, summary):
        assert (x[0], int(x[1]), int(x[2])) == (["w", "h"][s["trait"]], s["chrom1"] + 1, s["chrom2"] + 1)
        assert (int(x[4]), int(x[5])) == s["add"] and (int(x[9]), int(x[10])) == s["full"]
        for text, value in ((x[8], s["lod_add"]), (x[13], s["lod_full"]), (x[14], s["lod_add_at_full"]), (x[15], s["lod_int"])):
            assert len(text.split(".")[1]) == 5
            worst = max(worst, abs(float(text) - value))
    wthr = qtl.thresholds2(want["perm_max"])
    for t, line in enumerate(thr):
        for s, key in enumerate(("add", "full", "int")):
            for a in range(2):
                worst = max(worst, abs(float(line[1 + 2 * s + a]) - wthr[key][a, t]))
    print("file against qtl.scan2(linked=True): %.3g" % worst)
    assert worst <= 0.51e-5
