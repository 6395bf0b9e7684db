"""GPU suite: the polygenic (mixed-model) scan, qtl.scan_lmm with qtl.kinship and qtl.est_herit on cnf2_kinship_sums and
cnf2_qtl_scan_cols.  The yardstick (tests/qtllmm_reference.py) whitens with the Cholesky factor of V = h2 K + (1 - h2) I and
fits by lstsq -- no eigenvectors -- on hand-made rows and on the rows of two swept pedigrees.  Nothing here asks for the
same bits from two calls of scan_lmm: the eigensolver is torch's."""
import ctypes as C

import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import CHROM_LENS, noise, soft_rows
from qtllmm_reference import (ATOL, chromstarts_of, cols_reference, compare_lmm, grid_herit, kinship_ref,  # noqa: F401
                              reference_lmm)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def rows_context(capi, lens, n):
    """a context that holds a map and stands for n analysed individuals: what the scans on given rows need"""
    cs = chromstarts_of(lens)
    ctx = capi.Context(0)
    ctx.upload_map(np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in lens]), cs)
    ctx.n_ind = n
    return ctx, cs


def hand_made(n, seed, T=2):
    origin, _ = soft_rows(n, CHROM_LENS, seed)
    a = origin[:, :, 3] - origin[:, :, 0]
    cov = synth.uniform(seed * 16 + 9, np.arange(n)).reshape(n, 1)
    K = kinship_ref(origin, chromstarts_of(CHROM_LENS))
    g = np.linalg.cholesky(K + 1e-9 * np.eye(n)) @ noise(n, T, seed + 1)
    pheno = 0.7 * a[:, [20, 60][:T]] + 1.5 * g + noise(n, T, seed + 2) + 0.3 * cov
    return origin, pheno, cov


# ------------------------------------------------------------------------------------- 1. hand-made rows, given h2
def test_identity_kinship_is_the_plain_scan(capi):
    import torch
    n = 24
    origin, pheno, cov = hand_made(n, 31)
    ctx, cs = rows_context(capi, CHROM_LENS, n)
    rows = torch.from_numpy(origin).cuda()
    want = qtl.scan(ctx, pheno, cov=cov, rows=rows)
    for h2 in (0.0, 0.4):
        got = qtl.scan_lmm(ctx, pheno, kinship=np.eye(n), cov=cov, h2=h2, rows=rows)
        err_l = np.abs(got["lod"] - want["lod"]).max()
        both = np.isfinite(want["coef"])
        err_c = (np.abs(got["coef"][both] - want["coef"][both]) / np.maximum(1.0, np.abs(want["coef"][both]))).max()
        print("identity, h2 %.1f: lod %.3g coef %.3g" % (h2, err_l, err_c))
        assert err_l <= ATOL and err_c <= ATOL and np.array_equal(got["rank"], want["rank"])
        assert np.array_equal(np.isfinite(got["coef"]), both) and np.all(got["h2"] == h2) and list(got["n_used"]) == [n, n]
    ctx.close()


@pytest.mark.parametrize("n", [24, 67])
@pytest.mark.parametrize("loco", [True, False])
def test_realised_kinship_at_given_h2(capi, n, loco):
    import torch
    origin, pheno, cov = hand_made(n, 50 + n)
    ctx, cs = rows_context(capi, CHROM_LENS, n)
    rows = torch.from_numpy(origin).cuda()
    kin_of = lambda c: kinship_ref(origin, cs, leave_out=c if loco else None)
    for h2 in (0.0, 0.3, 0.8):
        got = qtl.scan_lmm(ctx, pheno, loco=loco, cov=cov, h2=h2, rows=rows)
        ref = reference_lmm(origin, cs, pheno, cov, np.full((2, len(CHROM_LENS)), h2), kin_of)
        compare_lmm(got, ref, "n %d loco %s h2 %.1f" % (n, loco, h2))
        assert np.all(got["h2"] == h2) and got["perm_max"] is None and np.all(got["sigma2"] > 0)
    # the kinship handed over as a matrix, per chromosome and one for the genome: the same route
    Ks = np.stack([kin_of(c) for c in range(len(CHROM_LENS))]) if loco else kin_of(0)
    again = qtl.scan_lmm(ctx, pheno, kinship=Ks, cov=cov, h2=0.8, rows=rows)
    assert np.abs(again["lod"] - got["lod"]).max() <= ATOL
    # units and offsets of the trait: LOD and rank at a given h2
    moved = qtl.scan_lmm(ctx, 3.0 * pheno + 7.0, loco=loco, cov=cov, h2=0.8, rows=rows)
    assert np.abs(moved["lod"] - got["lod"]).max() <= ATOL and np.array_equal(moved["rank"], got["rank"])
    ctx.close()


def test_additive_and_refusals(capi):
    import torch
    n = 24
    origin, pheno, cov = hand_made(n, 31)
    ctx, cs = rows_context(capi, CHROM_LENS, n)
    rows = torch.from_numpy(origin).cuda()
    got = qtl.scan_lmm(ctx, pheno, cov=cov, h2=0.3, additive=True, rows=rows)
    ref = reference_lmm(origin, cs, pheno, cov, np.full((2, 6), 0.3), lambda c: kinship_ref(origin, cs, leave_out=c), additive=True)
    assert np.isnan(got["coef"][:, :, 1]).all()
    ref["compared"] = np.stack([ref["compared"], np.zeros_like(ref["compared"])], axis=2)
    compare_lmm(got, ref, "additive", share=0.45)
    with pytest.raises(ValueError):
        qtl.scan_lmm(ctx, pheno[:-1], rows=rows)
    with pytest.raises(ValueError):
        qtl.scan_lmm(ctx, pheno, kinship=np.eye(n + 1), rows=rows)
    with pytest.raises(ValueError):
        qtl.scan_lmm(ctx, pheno, h2=1.0, rows=rows)
    ctx.close()


# ------------------------------------------------------------------------------------- 2. estimated h2, missing values, permutations
def device_array(capi, ptr, shape):
    """a host copy of the doubles behind a device pointer"""
    out = np.zeros(shape)
    hip = C.CDLL(capi.hip_runtimes()[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0
    return out


def test_estimated_h2_missing_values_and_permutations(capi):
    import torch
    n, P = 67, 5
    origin, pheno, cov = hand_made(n, 91)
    pheno[[3, 17, 40], 1] = np.nan                       # the second trait: a pattern, a kept set and eigenvectors of its own
    ctx, cs = rows_context(capi, CHROM_LENS, n)
    rows = torch.from_numpy(origin).cuda()
    calls, plain = [], ctx.qtl_scan_cols_device

    def recording(nk, n_mark, ne, d_reg, x0, y, scale=None, perm=None):
        got = plain(nk, n_mark, ne, d_reg, x0, y, scale=scale, perm=perm)
        if perm is not None:
            calls.append(dict(reg=device_array(capi, d_reg, (nk, n_mark, ne)), x0=x0.copy(), pheno=y.copy(), scale=scale.copy(),
                              perm=perm.copy(), perm_max=got["perm_max"].copy()))
        return got
    ctx.qtl_scan_cols_device = recording
    got = qtl.scan_lmm(ctx, pheno, loco=False, cov=cov, permutations=P, seed=4, rows=rows)
    ctx.qtl_scan_cols_device = plain
    assert list(got["n_used"]) == [n, n - 3] and got["perm_max"].shape == (P, 2, len(CHROM_LENS))
    K = kinship_ref(origin, cs)
    for t in range(2):
        keep = np.isfinite(pheno[:, t])
        assert np.all(got["h2"][t] == got["h2"][t, 0]) and np.all(got["sigma2"][t] == got["sigma2"][t, 0])
        ref = reference_lmm(origin, cs, pheno[:, [t]], cov, [got["h2"][t]], lambda c: K, keep=keep)
        compare_lmm(got, ref, "trait %d, estimated h2 %.6f" % (t, got["h2"][t, 0]), traits=[t])
        y = pheno[keep, t] - pheno[keep, t].mean()
        X0 = np.concatenate([np.ones((keep.sum(), 1)), cov[keep] - cov[keep].mean(axis=0)], axis=1)
        best, vals = grid_herit(K[np.ix_(keep, keep)], y, X0, reml=True)
        print("trait %d: h2 %.6f, the grid's maximum at %.4f" % (t, got["h2"][t, 0], best))
        assert abs(got["h2"][t, 0] - best) <= 1e-4
    # the permutations: the maxima of a least-squares scan over the very columns the product permuted -- its whitened
    # null-model residuals, which are orthogonal to the whitened null design
    assert len(calls) == 2 * len(CHROM_LENS)
    for k, call in enumerate(calls):
        t, c = k // len(CHROM_LENS), k % len(CHROM_LENS)          # (a pattern runs through its chromosomes before the next)
        nk = call["reg"].shape[0]
        assert np.array_equal(call["perm"], qtl.permutations(nk, P, 4))
        assert np.abs(call["x0"].T @ call["pheno"]).max() <= 1e-9 * np.abs(call["pheno"]).max() * nk
        ref = cols_reference(call["reg"], call["x0"], call["pheno"], call["scale"], call["perm"])
        err = np.abs(got["perm_max"][:, t, c] - ref["perm_max"][:, 0]).max()
        print("permutations, trait %d chromosome %d: %.3g" % (t, c, err))
        assert err <= ATOL
    # units and offsets: with h2 estimated, the golden section ends at a width of 1e-8, so h2 agrees within 1e-7 and a
    # LOD, whose slope in h2 stays below 1e2 here, within 1e-5
    moved = qtl.scan_lmm(ctx, 3.0 * pheno + 7.0, loco=False, cov=cov, rows=rows)
    print("3 y + 7: h2 %.3g lod %.3g" % (np.abs(moved["h2"] - got["h2"]).max(), np.abs(moved["lod"] - got["lod"]).max()))
    assert np.abs(moved["h2"] - got["h2"]).max() <= 1e-7 and np.abs(moved["lod"] - got["lod"]).max() <= 1e-5
    assert np.array_equal(moved["rank"], got["rank"])
    # thresholds and peaks read the result as they read scan's
    thr = qtl.thresholds(got["perm_max"])
    assert thr["genome"].shape == (2, 2) and thr["chromosome"].shape == (2, 2, len(CHROM_LENS)) and np.all(thr["genome"] > 0)
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in CHROM_LENS])
    found = qtl.peaks(got["lod"], pos, cs, 0.0, coef=got["coef"])
    assert len(found) == 2 * len(CHROM_LENS) and all(got["lod"][p["trait"], p["marker"]] == p["lod"] for p in found)
    ctx.close()


# ------------------------------------------------------------------------------------- 3. through the sweep
def sweep_peds():
    return [("f2", synth.make_f2(24, 17, 2, seed=7)),
            ("outbred3", synth.make_outbred3(3, 4, 9, 2, seed=5, missing=0.2, random_hw=True, random_sure=True))]


@pytest.mark.parametrize("which", [0, 1])
def test_through_the_sweep(capi, which):
    name, ped = sweep_peds()[which]
    n, M = len(ped.dous), ped.n_markers
    cs = np.asarray(ped.chromstarts, np.int64)
    ctx = capi.Context(0)
    ctx.upload(ped)
    rows = qtl.origin_rows(ctx)
    origin = rows.cpu().numpy()
    a = origin[:, :, 3] - origin[:, :, 0]
    pheno = np.stack([a[:, 4], a[:, M - 3]], axis=1) + noise(n, 2, 8)
    cov = synth.uniform(21, np.arange(n)).reshape(n, 1)
    use = np.ones(n, bool)
    use[2] = False
    got = qtl.scan_lmm(ctx, pheno, cov=cov, use=use, rows=rows)
    keep = use & (origin[:, cs[:-1]] != 0).any(axis=2).all(axis=1)
    assert list(got["n_used"]) == [keep.sum()] * 2
    kin_of = lambda c: kinship_ref(origin, cs, leave_out=c)
    ref = reference_lmm(origin, cs, pheno, cov, got["h2"], kin_of, keep=keep)
    compare_lmm(got, ref, "sweep " + name, share=0.5)
    # the kinship of the product against numpy's, and every returned h2 against the grid (the rows are the sweep's, so no
    # seed is chosen here and the grid is not asked for a single local maximum; that is the host suite's part)
    L = qtl.kinship(ctx, rows=rows, loco=True).cpu().numpy()
    assert max(np.abs(L[c] - kin_of(c)).max() for c in range(len(cs) - 1)) <= ATOL
    X0 = np.concatenate([np.ones((keep.sum(), 1)), cov[keep] - cov[keep].mean(axis=0)], axis=1)
    for t in range(2):
        y = pheno[keep, t] - pheno[keep, t].mean()
        for c in range(len(cs) - 1):
            best, _ = grid_herit(kin_of(c)[np.ix_(keep, keep)], y, X0, reml=True, single=False)
            print("sweep %s: trait %d without chromosome %d: h2 %.6f, the grid's maximum at %.4f" % (name, t, c, got["h2"][t, c], best))
            assert abs(got["h2"][t, c] - best) <= 1e-4
    # without a sweep of its own the call makes one
    own = qtl.scan_lmm(ctx, pheno, cov=cov, use=use, h2=0.3)
    given = qtl.scan_lmm(ctx, pheno, cov=cov, use=use, h2=0.3, rows=rows)
    assert np.abs(own["lod"] - given["lod"]).max() <= ATOL
    ctx.close()
