"""GPU suite: the kinship sums (cnf2_kinship_sums, Context.kinship_sums / kinship_sums_device, qtl.kinship): the SYRK over
the markers on the f64 matrix cores against numpy's A @ A.T (tests/qtllmm_reference.py), at every edge of its tiling, with
both forms of the sum (one pass; chunks of 256 markers added in rounds), for its symmetry and its reproducibility."""
import numpy as np
import pytest

from cnf2freq_amd import qtl
from qtl_reference import CHROM_LENS, skip, soft_rows
from qtllmm_reference import ATOL, chromstarts_of, kinship_sums_ref

pytestmark = pytest.mark.gpu

RANGES = [(0, 6), (0, 1), (4, 5), (2, 5)]          # whole map, chromosome 0 alone (one marker), chromosome 4 alone, 2 .. 4
# The kernel's edges in n: the result tile of an instruction (16), a wave's quarter (64), a block's tile (128: one block,
# then three and six with a mirrored tile) -- one n on each side of each -- and the issue's sizes
SIZES = [5, 15, 16, 17, 63, 64, 65, 67, 127, 128, 129, 130, 257]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens):
    cs = chromstarts_of(lens)
    ctx = capi.Context(0)
    ctx.upload_map(np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in lens]), cs)
    return ctx, cs


def check(got, cnt, origin, cs, c0, c1, what):
    ref, ref_cnt = kinship_sums_ref(origin, cs, c0, c1)
    err = (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()
    print("%s chromosomes %d..%d (%d markers): %.3g" % (what, c0, c1, ref_cnt, err))
    assert cnt == ref_cnt
    assert err <= ATOL
    assert got.tobytes() == got.T.copy().tobytes(), "S equals S.T to the bit"


@pytest.mark.parametrize("n", SIZES)
def test_sums_on_hand_made_rows(capi, n):
    import torch
    origin, _ = soft_rows(n, CHROM_LENS, 40 + n)
    origin = skip(origin, [1], 4, CHROM_LENS)
    ctx, cs = map_context(capi, CHROM_LENS)
    d_o = torch.from_numpy(origin).cuda()
    for c0, c1 in RANGES:
        got, cnt = ctx.kinship_sums(origin, c0, c1)
        check(got, cnt, origin, cs, c0, c1, "n %d" % n)
        again, _ = ctx.kinship_sums(origin, c0, c1)
        assert again.tobytes() == got.tobytes()
        from_dev, cnt_dev = ctx.kinship_sums_device(n, d_o.data_ptr(), c0, c1)
        assert from_dev.tobytes() == got.tobytes() and cnt_dev == cnt
        d_s = torch.full((n, n), 77.0, dtype=torch.float64, device="cuda")
        d_c = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        assert ctx.kinship_sums_device(n, d_o.data_ptr(), c0, c1, d_sum=d_s.data_ptr(), d_n_markers=d_c.data_ptr()) is None
        ctx.sync()
        assert d_s.cpu().numpy().tobytes() == got.tobytes() and int(d_c.item()) == cnt
    got, _ = ctx.kinship_sums(origin, 4, 5)
    assert np.all(got[1] == 0.0) and np.all(got[:, 1] == 0.0), "an individual skipped on the chromosome: exactly 0"
    ctx.close()


@pytest.mark.parametrize("n", [17, 130])
def test_split_marker_range(capi, n):
    """more than 256 markers and n <= 1920: chunks of 256 markers, 34 of them on the whole map -- two rounds of the finish
    kernel -- two on chromosome 1, whose last is partial"""
    lens = (8200, 300)
    origin, _ = soft_rows(n, lens, 7 + n)
    ctx, cs = map_context(capi, lens)
    for c0, c1 in [(0, 2), (1, 2)]:
        got, cnt = ctx.kinship_sums(origin, c0, c1)
        check(got, cnt, origin, cs, c0, c1, "split, n %d" % n)
        assert ctx.kinship_sums(origin, c0, c1)[0].tobytes() == got.tobytes()
    ctx.close()


@pytest.mark.parametrize("n", [1920, 1921])
def test_either_side_of_the_split_threshold(capi, n):
    """257 markers: n = 1920 (120 block tiles) sums two chunks, n = 1921 (136) the whole range in one pass"""
    lens = (257,)
    origin, _ = soft_rows(n, lens, 3)
    ctx, cs = map_context(capi, lens)
    got, cnt = ctx.kinship_sums(origin)
    check(got, cnt, origin, cs, 0, 1, "n %d" % n)
    ctx.close()


def test_kinship_and_loco(capi):
    import torch
    n = 24
    origin, _ = soft_rows(n, CHROM_LENS, 3)
    ctx, cs = map_context(capi, CHROM_LENS)
    rows = torch.from_numpy(origin).cuda()
    S, M = ctx.kinship_sums_device(n, rows.data_ptr())
    K = qtl.kinship(ctx, rows=rows)
    assert K.dtype == torch.float64 and K.is_cuda and tuple(K.shape) == (n, n)
    assert np.abs(K.cpu().numpy() - (1.0 + S / M) / 2.0).max() <= 1e-15
    L = qtl.kinship(ctx, rows=rows, loco=True)
    assert tuple(L.shape) == (len(CHROM_LENS), n, n)
    for c in range(len(CHROM_LENS)):
        Sc, Mc = ctx.kinship_sums_device(n, rows.data_ptr(), c, c + 1)
        want = (1.0 + (S - Sc) / (M - Mc)) / 2.0
        assert np.abs(L[c].cpu().numpy() - want).max() <= 1e-15
        rest, _ = kinship_sums_ref(origin[:, np.r_[0:cs[c], cs[c + 1]:cs[-1]]], [0, M - Mc], 0, 1)
        assert np.abs(want - (1.0 + rest / (M - Mc)) / 2.0).max() <= ATOL
    ctx.close()
    one, _ = map_context(capi, (5,))
    with pytest.raises(ValueError):
        qtl.kinship(one, rows=rows[:, :5].contiguous(), loco=True)
    one.close()


def test_refusals_write_nothing(capi):
    n = 17
    origin, _ = soft_rows(n, CHROM_LENS, 3)
    ctx, _ = map_context(capi, CHROM_LENS)
    out, cnt = np.full((n, n), 77.0), np.full(1, 77, np.int32)
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    for c0, c1, ptr in [(3, 3, p(origin)), (-1, 2, p(origin)), (0, 7, p(origin)), (0, 6, None)]:
        assert ctx.L.cnf2_kinship_sums(ctx.h, n, ptr, c0, c1, p(out), p(cnt), 0) == -2
        assert np.all(out == 77.0) and cnt[0] == 77
    assert ctx.L.cnf2_kinship_sums(ctx.h, 0, p(origin), 0, 6, p(out), p(cnt), 0) == -2
    with pytest.raises(capi.Cnf2Error):
        ctx.kinship_sums_device(n, None)             # the context holds no rows of a sweep_qtl
    ctx.close()
