"""GPU suite: the column scan (cnf2_qtl_scan_cols, Context.qtl_scan_cols / qtl_scan_cols_device): ordinary least squares on
prepared columns against a per-marker np.linalg.lstsq (tests/qtllmm_reference.py) -- regressors from soft origin rows and
Gaussian-like ones, with and without scale, every width of the null design, both numbers of regressors, the shapes of
tests/test_gpu_qtl.py, every block length at a tile edge -- its degenerate cells, and the existing scan as a cross-check."""
import numpy as np
import pytest

from qtl_reference import CHROM_LENS, soft_rows
from qtllmm_reference import ATOL, ad_columns, chromstarts_of, cols_case, cols_compare, cols_compared, cols_reference

pytestmark = pytest.mark.gpu

OUT_KEYS = ("lod", "coef", "rank", "rss0", "perm_max")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def same_bits(a, b):
    for k in OUT_KEYS:
        if a[k] is None:
            assert b[k] is None
        else:
            assert a[k].tobytes() == b[k].tobytes(), k


#        n   T   P  nx ne kind     scale   M     (n, T, P): the pairs of tests/test_gpu_qtl.py; nx = 9 is QTL_NX
CASES = [(5, 1, 0, 1, 2, "soft", False, 84),
         (13, 3, 1, 3, 2, "gauss", True, 33),
         (17, 17, 5, 9, 1, "gauss", True, 17),
         (64, 1, 33, 3, 1, "soft", False, 16),
         (67, 3, 33, 9, 2, "soft", True, 15),
         (67, 17, 5, 1, 2, "gauss", False, 1),       # R = 102: the second wave of a block, a partial column tile of 16
         (64, 17, 33, 3, 2, "soft", True, 84),       # R = 578: three column groups of 256
         (67, 3, 1, 9, 1, "soft", True, 84),
         (17, 1, 0, 1, 1, "gauss", False, 33)]


@pytest.mark.parametrize("n,T,P,nx,ne,kind,scaled,M", CASES)
def test_scan_on_prepared_columns(capi, n, T, P, nx, ne, kind, scaled, M):
    """lod, coef, rank, rss0 and perm_max against the least-squares fit; the same bits on a second call, with column tiles of
    16 and from device regressors"""
    import torch
    reg, x0, pheno, scale, perm = cols_case(n, T, P, nx, ne, kind, scaled, M=M)
    ref = cols_reference(reg, x0, pheno, scale, perm)
    cols_compared(ref)                            # the conditions of the comparison, on the reference, before anything runs
    ctx = capi.Context(0)
    got = ctx.qtl_scan_cols(reg, x0, pheno, scale=scale, perm=perm)
    cols_compare(got, ref, "n %d T %d P %d nx %d ne %d %s M %d" % (n, T, P, nx, ne, kind, M))
    assert (got["perm_max"] is None) == (P == 0)
    same_bits(got, ctx.qtl_scan_cols(reg, x0, pheno, scale=scale, perm=perm))
    ctx.set_qtl_columns(16)
    same_bits(got, ctx.qtl_scan_cols(reg, x0, pheno, scale=scale, perm=perm))
    ctx.set_qtl_columns(0)
    d_r = torch.from_numpy(np.ascontiguousarray(reg)).cuda()
    same_bits(got, ctx.qtl_scan_cols_device(n, M, ne, d_r.data_ptr(), x0, pheno, scale=scale, perm=perm))
    ctx.close()


def test_documented_cells(capi):
    n, M = 12, 5
    reg, x0, pheno, _, _ = cols_case(n, 2, 0, 3, 2, "gauss", False, M=M)
    reg[:, 1] = 0.0                                                       # an all-zero regressor
    reg[:, 2, 1] = 3.0 * reg[:, 2, 0]                                     # the second column in the span of the first
    y = np.concatenate([pheno, np.zeros((n, 1))], axis=1)                 # a column with RSS0 = 0
    ctx = capi.Context(0)
    got = ctx.qtl_scan_cols(reg, x0, y)
    assert list(got["rank"]) == [2, 0, 1, 2, 2] and got["rss0"][2] == 0.0 and np.all(got["rss0"][:2] > 0)
    assert np.all(got["lod"][:, 1] == 0.0) and np.isnan(got["coef"][:, 1]).all()
    assert np.isfinite(got["coef"][:2, 2, 0]).all() and np.isnan(got["coef"][:, 2, 1]).all()
    assert np.all(got["lod"][2] == 0.0) and np.isnan(got["coef"][2]).all() and np.all(got["lod"][:2, [0, 2, 3, 4]] > 0)
    cols_compare(got, cols_reference(reg, x0, y), "degenerate cells", share=0)
    for kw in (dict(reg=reg[:5], x0=x0[:5], pheno=y[:5]),                 # n < nx + 3
               dict(reg=reg, x0=np.concatenate([x0[:, :2], 2.0 * x0[:, :1]], axis=1), pheno=y)):      # x0 without full rank
        g = ctx.qtl_scan_cols(**kw)
        assert np.all(g["rank"] == 0) and np.all(g["lod"] == 0.0) and np.isnan(g["coef"]).all() and np.all(g["rss0"] == 0.0)
    # refused, with the outputs left alone
    ident = np.arange(n, dtype=np.int32)
    twice = ident.copy()
    twice[3] = 2
    holed = y.copy()
    holed[4, 0] = np.nan
    for kw in (dict(x0=x0, pheno=y, perm=twice[None]), dict(x0=x0, pheno=holed, perm=ident[None]),
               dict(x0=np.ones((n, 10)), pheno=y, perm=ident[None]), dict(x0=x0, pheno=y, perm=ident[None], scale=np.full(n, np.inf))):
        out = dict(lod=np.full((3, M), 77.0), coef=np.full((3, M, 2), 77.0), rank=np.full(M, 77, np.int32), rss0=np.full(3, 77.0),
                   perm_max=np.full((1, 3), 77.0))
        with pytest.raises(capi.Cnf2Error):
            ctx.qtl_scan_cols(reg, out=out, **kw)
        assert all(np.all(v == 77) for v in out.values())
    with pytest.raises(ValueError):
        ctx.qtl_scan_cols(np.zeros((n, M, 3)), x0, y)
    ctx.close()


@pytest.mark.parametrize("additive", [False, True])
def test_against_the_existing_scan(capi, additive):
    """x0 = [1, centred cov], reg = (a, d) of one chromosome's rows, no scale: cnf2_qtl_scan's lod and coef"""
    from cnf2freq_amd import synth
    n, T = 67, 3
    origin, _ = soft_rows(n, CHROM_LENS, 78)
    cs = chromstarts_of(CHROM_LENS)
    cov = synth.uniform(99, np.arange(n * 2)).reshape(n, 2)
    a = origin[:, :, 3] - origin[:, :, 0]
    pheno = a[:, [3, 40, 70]] + synth.uniform(98, np.arange(n * T)).reshape(n, T)
    ctx = capi.Context(0)
    ctx.upload_map(np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in CHROM_LENS]), cs)
    want = ctx.qtl_scan(origin, pheno, cov=cov, additive=additive)
    x0 = np.concatenate([np.ones((n, 1)), cov - cov.mean(axis=0)], axis=1)
    yc = pheno - pheno.mean(axis=0)
    for c in range(len(CHROM_LENS)):
        got = ctx.qtl_scan_cols(ad_columns(origin[:, cs[c]:cs[c + 1]], additive), x0, yc)
        sl = slice(cs[c], cs[c + 1])
        err_l = np.abs(got["lod"] - want["lod"][:, sl]).max()
        both = np.isfinite(want["coef"][:, sl])
        assert np.array_equal(both, np.isfinite(got["coef"]))
        err_c = np.abs(got["coef"][both] - want["coef"][:, sl][both]).max()
        print("chromosome %d: lod %.3g coef %.3g" % (c, err_l, err_c))
        assert err_l <= ATOL and err_c <= ATOL * max(1.0, np.abs(want["coef"][:, sl][both]).max())
        assert np.array_equal(got["rank"], want["rank"][sl])
        assert np.abs(got["rss0"] - want["rss0"][:, c]).max() <= ATOL * max(1.0, want["rss0"].max())
    ctx.close()
