"""GPU suite: what the variance-QTL scan (cnf2_qtl_scan_var) must not depend on.  The model has an intercept in both parts
and works on centred columns, so with the inputs of tests/qtl_invariance.py (values on a grid, exact transforms):

    y -> alpha y + beta     the LODs, coef_var, rank, iters and status stay, coef_mean scales with alpha, ll0 moves by
                            -n_c ln |alpha|
    z_k -> g z_k + d        nothing moves (a variance covariate's coefficient is not reported)
    swap03                  the sign of a flips in both parts
    swap12                  the sign of i flips in both parts
    covswap, reorder        no LOD moves (both covariates are variance covariates where they are exchanged)

Everything within ATOL of the untransformed run, which is itself compared with the yardstick (tests/qtlvar_reference.py);
iters and status outside the yardstick's `near` cells."""
import numpy as np
import pytest

import qtl_invariance as I
import qtlvar_reference as R
from qtl_reference import ATOL

pytestmark = pytest.mark.gpu

STOP = dict(imprint=True, max_iter=50, tol=1e-7)
NAMES = ("a", "d", "i")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


@pytest.fixture(scope="module")
def ctx(capi):
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in I.CHROM_LENS])
    c = capi.Context(0)
    c.upload_map(pos, I.CS)
    yield c
    c.close()


def run(ctx, inp, n_var):
    return ctx.qtl_scan_var(inp["origin"], inp["pheno"], cov=inp["cov"], n_var=n_var, use=inp["use"], perm=inp["perm"], **STOP)


_REFS = {}


def base_reference(case, n_var):
    if (case, n_var) not in _REFS:
        b = I.make_base(case)
        _REFS[case, n_var] = R.reference_scan_var(b["origin"], I.CS, b["pheno"], b["use"], b["cov"], n_var, perm=b["perm"], **STOP)
    return _REFS[case, n_var]


_RUNS = {}


def base_run(ctx, case, n_var):
    """the untransformed run, compared with the yardstick once"""
    if (case, n_var) not in _RUNS:
        ref = base_reference(case, n_var)
        R.compared_cells(ref, I.CS)
        assert ref["near"].mean() <= 0.01
        got = run(ctx, I.make_base(case), n_var)
        R.compare_var(got, ref, I.CS, "%s n_var %d" % (case[0], n_var))
        _RUNS[case, n_var] = got
    return _RUNS[case, n_var]


def check(got, base, ref, what, alpha=None, flip=()):
    """`got` against the untransformed run `base` mapped by alpha[T] (the traits' scales) and flip (effects whose sign changes)"""
    alpha = np.ones(got["lod"].shape[0]) if alpha is None else np.asarray(alpha, np.float64)
    sign = np.array([-1.0 if e in flip else 1.0 for e in NAMES])
    want_m = base["coef_mean"] * sign
    want_v = base["coef_var"] * sign
    want_0 = np.where(base["ll0"] == 0.0, 0.0, base["ll0"] - base["n_used"][None, :] * np.log(np.abs(alpha))[:, None])
    err = dict(lod=np.abs(got["lod"] - base["lod"]).max(), perm_max=np.abs(got["perm_max"] - base["perm_max"]).max(),
               coef_var=np.nanmax(np.abs(got["coef_var"] - want_v) / np.maximum(1.0, np.abs(want_v))),
               coef_mean=np.nanmax(np.abs(got["coef_mean"] / alpha[:, None, None] - want_m) / np.maximum(1.0, np.abs(want_m))),
               ll0=np.abs(got["ll0"] - want_0).max())
    print("%s: %s" % (what, ", ".join("%s %.3g" % kv for kv in err.items())))
    assert np.array_equal(np.isnan(got["coef_mean"]), np.isnan(base["coef_mean"])) and np.array_equal(np.isnan(got["coef_var"]), np.isnan(base["coef_var"]))
    assert np.array_equal(got["rank"], base["rank"]) and np.array_equal(got["n_used"], base["n_used"])
    ok = ~ref["near"]
    assert np.array_equal(got["iters"][ok], base["iters"][ok]) and np.array_equal(got["status"][ok], base["status"][ok]), what
    assert all(v <= ATOL for v in err.values()), what
    return err


@pytest.mark.parametrize("name", sorted(I.TRANSFORMS))
@pytest.mark.parametrize("case", I.CASES, ids=I.CASE_IDS)
def test_units_and_offsets(ctx, case, name):
    """y -> alpha y + beta and z_k -> g z_k + d, one variance covariate"""
    tr = I.TRANSFORMS[name]
    base, ref = base_run(ctx, case, 1), base_reference(case, 1)
    got = run(ctx, I.apply(I.make_base(case), tr), 1)
    check(got, base, ref, "%s transform %s" % (case[0], name), alpha=tr["alpha"])


@pytest.mark.parametrize("name", I.RELABELLINGS)
@pytest.mark.parametrize("case", I.CASES, ids=I.CASE_IDS)
def test_relabellings(ctx, case, name):
    """swap03 flips a, swap12 flips i, exchanged covariates and reordered individuals move nothing; two variance covariates"""
    base, ref = base_run(ctx, case, 2), base_reference(case, 2)
    inp, flip = I.relabel(I.make_base(case), name)
    got = run(ctx, inp, 2)
    check(got, base, ref, "%s %s" % (case[0], name), flip=flip)
