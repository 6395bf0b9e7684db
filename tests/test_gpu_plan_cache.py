"""GPU suite (-m gpu): the sweep's plan kept across sweeps (cnf2_plan.h PlanKey, cnf2_last_plan_reused).

A context keeps the job list, the groups of four and eight and their device copies of its last sweep; a call with an equal key
takes them as they stand.  On test_gpu_producer_masks.py's F2 of 21: a second equal call reports reuse and the same bits; after
everything the plan depends on -- the rows behind a window's uniformity, the pedigree, the range, each flag that routes windows,
the grid reserve, the cap on the lines -- the next call reports no reuse and gives the bits of a context that never swept
anything else; the call after it reuses again."""
import numpy as np
import pytest

from test_gpu_producer_masks import C33, _sweep, f2_of_21
from test_gpu_uniform_states import ONE_BLOCK, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    assert c.load().cnf2_device_count() >= 1, "no HIP device: the product path has no fallback"
    return c


def _fresh(capi, ped, prepare=None, dous=None, **kw):
    """The sweep of a context that has swept nothing else."""
    ctx = capi.Context(0)
    try:
        ctx.upload(ped, dous=dous)
        if prepare:
            prepare(ctx)
        out = _sweep(capi, ctx, **kw)
        assert not ctx.last_plan_reused()
        return out
    finally:
        ctx.close()


@pytest.fixture()
def kept(capi):
    """(pedigree, context, its default sweep): the context has swept twice, the second time on the kept plan."""
    ped = f2_of_21()
    ctx = capi.Context(0)
    ctx.upload(ped)
    first = _sweep(capi, ctx)
    assert not ctx.last_plan_reused()
    again = _sweep(capi, ctx)
    assert ctx.last_plan_reused()
    _same(again, first, "the second equal call")
    yield ped, ctx, first
    ctx.close()


def _changed(capi, ctx, want, what, **kw):
    """The call after a change plans anew and gives `want`; the same call again reuses and gives `want`."""
    got = _sweep(capi, ctx, **kw)
    assert not ctx.last_plan_reused(), what + ": reused a plan that no longer holds"
    _same(got, want, what)
    got = _sweep(capi, ctx, **kw)
    assert ctx.last_plan_reused(), what + ": the second call"
    _same(got, want, what + ", the second call")


def test_reuse_does_not_depend_on_what_the_call_writes(capi, kept):
    ped, ctx, first = kept
    nd = _sweep(capi, ctx, dosage=False)
    assert ctx.last_plan_reused()
    assert np.array_equal(nd["factors"], first["factors"]) and np.array_equal(nd["loglik"], first["loglik"])
    _same(_sweep(capi, ctx, static_jobs=True), first, "static jobs")
    assert ctx.last_plan_reused()
    assert ctx.last_uniform_pack8() == dict(eights=8, jobs=64) and ctx.last_line_records()["on_records"] == 84


def test_a_row_update_that_changes_uniformity(capi, kept):
    ped, ctx, first = kept
    allele = ped.allele[2:3].copy()
    allele[0, C33 + 9] = (1, 2)                    # founder B heterozygous at one marker: no window is uniform any more
    ctx.update_rows(2, allele, ped.sure[2:3], ped.hw[2:3])
    ped2 = f2_of_21()
    ped2.allele[2, C33 + 9] = (1, 2)
    want = _fresh(capi, ped2)
    assert not np.array_equal(want["dosage"], first["dosage"])
    _changed(capi, ctx, want, "founder B heterozygous")
    assert ctx.last_uniform_pack() == dict(jobs=0, groups=0)
    ctx.update_rows(2, ped.allele[2:3], ped.sure[2:3], ped.hw[2:3])
    _changed(capi, ctx, first, "rows restored")
    assert ctx.last_uniform_pack8() == dict(eights=8, jobs=64)


def test_a_new_pedigree_and_another_range(capi, kept):
    ped, ctx, first = kept
    _changed(capi, ctx, _fresh(capi, ped, ind_begin=1, ind_end=20), "range [1, 20)", ind_begin=1, ind_end=20)
    _changed(capi, ctx, _fresh(capi, ped, ind_begin=0, ind_end=19), "range [0, 19): the same number from another start",
             ind_begin=0, ind_end=19)
    dous = ped.dous[::-1].copy()
    ctx.upload_pedigree(ped.par, ped.empty, ped.gen, ped.row_of, dous)
    want = _fresh(capi, ped, dous=dous)
    assert np.array_equal(want["loglik"], first["loglik"][::-1])
    _changed(capi, ctx, want, "the individuals in reverse order")


FLAGS = ["NO_TIES", "FULL_SPILL", "MERGE_MODES", "XPOSE", "FLUSH_TINY", "ALL_STATES", "NO_LINE_RECORDS", "NO_UNIFORM_PACK",
         "NO_UNIFORM_PACK8"]


def test_each_flag_that_enters_the_plan(capi, kept):
    ped, ctx, first = kept
    for name in FLAGS:
        flag = getattr(capi, name)
        _changed(capi, ctx, _fresh(capi, ped, extra_flags=flag), name, extra_flags=flag)
        _changed(capi, ctx, first, "without " + name)


def test_grid_reserve_and_line_cap(capi, kept):
    ped, ctx, first = kept
    ctx.set_grid_reserve(ONE_BLOCK)
    _changed(capi, ctx, _fresh(capi, ped, prepare=lambda c: c.set_grid_reserve(ONE_BLOCK)), "one block")
    ctx.set_grid_reserve(0)
    _changed(capi, ctx, first, "reserve lifted")
    ctx.set_line_records(1)
    _changed(capi, ctx, _fresh(capi, ped, prepare=lambda c: c.set_line_records(1)), "one line")
    ctx.set_line_records(0)
    _changed(capi, ctx, _fresh(capi, ped, prepare=lambda c: c.set_line_records(0)), "no line")
    assert ctx.last_line_records()["lines"] == 0 and ctx.last_uniform_pack() == dict(jobs=0, groups=0)
    ctx.set_line_records(-1)
    _changed(capi, ctx, first, "cap lifted")


def test_other_entry_points_between_two_sweeps(capi, kept):
    """The Viterbi mode sweeps the same lists (it reuses them); the batched consumers overwrite the job list on the device."""
    ped, ctx, first = kept
    vit = ctx.sweep_viterbi()
    assert ctx.last_plan_reused()
    assert np.array_equal(vit["factors"], first["factors"]) and np.array_equal(vit["loglik"], first["loglik"])
    _same(_sweep(capi, ctx), first, "after the Viterbi call")
    assert ctx.last_plan_reused()
    ctx.sweep_accumulate(ctx.descendants())
    _changed(capi, ctx, first, "after a batched consumer")
