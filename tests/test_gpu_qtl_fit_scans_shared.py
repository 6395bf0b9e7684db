"""The EM, binary, survival and variance scans share one driver and one kind of buffer set in the library.  Here they run
interleaved on ONE context, so that a scan handed another scan's buffer, or a size another call left behind, shows: every
call of the sequence

    binary A -- survival -- variance -- EM -- binary B (larger n, T = 2, P = 5, K = 8) -- binary A again

must give, bit for bit and with None where there is nothing, what the same call gives on a fresh context -- once with host
rows and host outputs, once with device rows and OUT_DEVICE outputs.  Before the second half every scan's column cap is set
to 1, which the results do not depend on.  The cases are from the CASES of the four reference modules, on CHROM_LENS (84
markers): binary A has no covariates, the survival case a `use` mask, the variance case skipped individuals, the EM case
three traits.  The product is compared with itself only; the yardsticks are in the four scans' own test files."""
import numpy as np
import pytest

import qtlbin_reference as RB
import qtlem_reference as RE
import qtlsurv_reference as RS
import qtlvar_reference as RV
from qtl_reference import CHROM_LENS, chromstarts_of

pytestmark = pytest.mark.gpu

FIRST_HALF = 3      # calls before the column caps are set to 1
_FRESH = {}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi):
    """a context that holds a map only: what the four scans need"""
    cs = chromstarts_of(CHROM_LENS)
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in CHROM_LENS])
    ctx = capi.Context(0)
    ctx.upload_map(pos, cs)
    return ctx


def sequence():
    """(name, scan, n, origin, the column arrays, keyword arguments) per call, at fixed iterations (tol = -1)"""
    calls = []

    def add(name, scan, case):
        made = {"em": RE, "binary": RB, "surv": RS, "var": RV}[scan].make_case(*case)
        origin, cols, (cov, use, perm) = made[0], made[1:-3], made[-3:]
        kw = dict(cov=cov, use=use, perm=perm, tol=-1.0)
        if scan == "surv":
            n, K, kw["imprint"], kw["additive"], _, T, P, mask, _, kw["max_iter"], _ = case
        elif scan == "var":
            n, K, kw["n_var"], kw["imprint"], kw["additive"], _, T, P, mask, _, kw["max_iter"] = case
        else:
            n, K, kw["imprint"], kw["additive"], _, T, P, mask, _, kw["max_iter"] = case
        calls.append((name, scan, n, origin, cols, kw))
        return n, K, T, P, mask

    n_a, K_a = add("binary A", "binary", RB.CASES[1])[:2]
    assert add("survival", "surv", RS.CASES[4])[4]              # a mask
    add("variance", "var", RV.CASES[5])
    add("EM", "em", RE.CASES[1])
    n_b, _, T_b, P_b, _ = add("binary B", "binary", RB.CASES[3])
    calls.append(calls[0])                                      # binary A again
    assert K_a == 0 and n_b > n_a and T_b >= 2 and P_b > 0 and all(c[2] <= 130 for c in calls)
    return calls


def fresh(capi, call):
    """the call's host outputs on a context of its own, computed once and left unchanged"""
    name, scan, n, origin, cols, kw = call
    if name not in _FRESH:
        ctx = map_context(capi)
        _FRESH[name] = getattr(ctx, "qtl_scan_" + scan)(origin, *cols, **kw)
        ctx.close()
    return _FRESH[name]


def same_bits(got, want, what):
    assert list(got) == list(want), what
    for k in want:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_interleaved_on_one_context(capi, device):
    import torch
    calls = sequence()
    ctx = map_context(capi)
    for i, call in enumerate(calls):
        name, scan, n, origin, cols, kw = call
        want = fresh(capi, call)
        if i == FIRST_HALF:
            for cap in ("em", "bin", "surv", "var"):
                getattr(ctx, "set_qtl%s_columns" % cap)(1)
        if not device:
            got = getattr(ctx, "qtl_scan_" + scan)(origin, *cols, **kw)
        else:
            d_o = torch.from_numpy(origin).cuda()
            d = {k: None if v is None else torch.full(v.shape, 77, dtype=torch.int32 if v.dtype == np.int32 else torch.float64,
                                                      device=d_o.device) for k, v in want.items()}
            getattr(ctx, "qtl_scan_%s_device" % scan)(n, d_o.data_ptr(), *cols, flags=capi.OUT_DEVICE,
                                                      out={k: None if v is None else v.data_ptr() for k, v in d.items()}, **kw)
            ctx.sync()
            got = {k: None if v is None else v.cpu().numpy() for k, v in d.items()}
        same_bits(got, want, "%s (call %d, %s outputs)" % (name, i, "device" if device else "host"))
    ctx.close()
