"""CPU suite: the host side of the multiple-imputation scan (cnf2_qtl_scan_imp).  The yardstick's own conditions at the
issue's shapes, one marker's combined cells through the shared header (cnf2h_qtlimp_marker, cnf2freq_amd/csrc/cnf2_qtlimp.h)
against it, what the recurrence promises to the bit, the refusals, and the argument checks of cnf2freq_amd/qtl.py."""
import numpy as np
import pytest

from cnf2freq_amd import qtl
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of
from qtlimp_reference import COMBINE_BOUND, CPU_CASES, case_reference, classes_of, conditions, encode, one_hot

IDS = ["n%d_D%d_K%d" % c[:3] for c in CPU_CASES]


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    h.load()
    return h


def centred(v, use):
    """the columns minus their means over the used individuals, as the scan forms them"""
    v = np.array(v, np.float64)
    v[use] -= v[use].mean(axis=0)
    v[~use] = 0.0
    return v


# ------------------------------------------------------------------------------------- 1. the yardstick alone
@pytest.mark.parametrize("case", CPU_CASES, ids=IDS)
def test_yardstick_conditions(case):
    """every marker is compared in every draw, and the float64 two-pass combination is the longdouble one to 9e-16"""
    n, D, K, T, P, additive, seed = case
    _, ref = case_reference(case, special=False)
    compared, shares = conditions(ref, chromstarts_of(CHROM_LENS), additive, "n %d D %d K %d" % (n, D, K))
    assert np.all(shares == 1.0) and compared.all()
    assert ref["combine_err"] <= COMBINE_BOUND


# ------------------------------------------------------------------------------------- 2. one marker on the CPU
@pytest.mark.parametrize("case", CPU_CASES, ids=IDS)
def test_marker_against_the_yardstick(host, case):
    n, D, K, T, P, additive, seed = case
    (state, pheno, cov, use, perm), ref = case_reference(case, special=False)
    cs = chromstarts_of(CHROM_LENS)
    um = np.ones(n, bool)
    y, z = centred(pheno, um), None if cov is None else centred(cov, um)
    cols = [0] if additive else [0, 1]
    worst_l = worst_c = worst_d = 0.0
    for m in range(state.shape[2]):
        got = host.qtlimp_marker(state[:, :, m], y, cov=z, additive=additive)
        assert got["rank"] == ref["rank"][m] and got["n_used"] == n
        worst_l = max(worst_l, np.abs(got["lod"] - ref["lod"][0, :, m]).max())
        worst_d = max(worst_d, np.abs(got["draw_lod"] - ref["draw_lod"][:, :, m]).max())
        rc = ref["coef"][:, m][:, cols]
        worst_c = max(worst_c, (np.abs(got["coef"][:, cols] - rc) / np.maximum(1.0, np.abs(rc))).max())
        if additive:
            assert np.isnan(got["coef"][:, 1]).all()
    print("n %d D %d K %d: lod %.3g, draw_lod %.3g, coef %.3g over %d markers" % (n, D, K, worst_l, worst_d, worst_c, cs[-1]))
    assert worst_l <= ATOL and worst_d <= ATOL and worst_c <= ATOL


def small_case(n=24, T=2, K=1, seed=2):
    from cnf2freq_amd import synth
    k = (synth.uniform(seed * 16, np.arange(n * 3)).reshape(n, 3) * 4).astype(np.int64)
    k[:4, :] = np.arange(4)[:, None]                      # every class occurs in every draw
    um = np.ones(n, bool)
    y = centred(0.6 * ((k[:, :1] == 3) * 1.0 - (k[:, :1] == 0)) + synth.uniform(seed * 16 + 1, np.arange(n * T)).reshape(n, T), um)
    z = centred(synth.uniform(seed * 16 + 2, np.arange(n * K)).reshape(n, K), um)
    return k, y, z


def test_identical_draws_give_the_single_draw_to_the_bit(host):
    k, y, z = small_case()
    one = host.qtlimp_marker(encode(k[:, :1], 1), y, cov=z)
    for D in (2, 3, 7, 64):
        # (other noise in the ignored bits of every copy)
        many = host.qtlimp_marker(encode(np.repeat(k[:, :1], D, axis=1), D), y, cov=z)
        assert np.array_equal(many["lod"], one["lod"]) and np.array_equal(many["coef"], one["coef"])
        assert many["rank"] == one["rank"] == 2 and np.array_equal(many["draw_lod"], np.repeat(one["draw_lod"], D, axis=0))
    assert one["lod"].min() > 0.0 and np.isfinite(one["coef"]).all()


def test_one_draw_is_the_single_scan_of_its_one_hot_row(host):
    """D = 1 against cnf2h_qtl_boot_marker, the single scan's cell on the CPU, with every individual drawn once: to the bit"""
    k, y, z = small_case(n=31, T=3, K=2, seed=5)
    c = np.ones(31, bool)
    c[[2, 17]] = False
    for additive in (False, True):
        for j in range(3):
            st = encode(k[:, j:j + 1], j)
            got = host.qtlimp_marker(st, y, cov=z, c=c, additive=additive)
            want = host.qtl_boot_marker(one_hot(st)[:, 0], y, np.ones(31, np.int32), cov=z, c=c, additive=additive)
            assert np.array_equal(got["lod"], want["lod"]) and np.array_equal(got["lod"], got["draw_lod"][0])
            assert np.array_equal(got["coef"], want["coef"], equal_nan=True) and got["rank"] == want["rank"]
            assert np.array_equal(got["rss0"], want["rss0"]) and got["n_used"] == want["n_bc"] == 29


def test_a_column_dropped_in_one_draw(host):
    """draw 1 has no heterozygote: its d column is dropped, so the combined dominance effect is NaN and the rank is 1"""
    k, y, z = small_case()
    k[:, 1] = np.where((k[:, 1] == 1) | (k[:, 1] == 2), 3, k[:, 1])
    got = host.qtlimp_marker(encode(k, 3), y, cov=z)
    assert got["rank"] == 1
    assert np.isnan(got["coef"][:, 1]).all() and np.isfinite(got["coef"][:, 0]).all()
    assert np.isfinite(got["lod"]).all() and got["lod"].min() > 0.0
    both = host.qtlimp_marker(encode(k[:, [0, 2]], 3), y, cov=z)
    assert both["rank"] == 2 and np.isfinite(both["coef"]).all()
    # ... and the combined LOD is the log of the mean likelihood ratio of the three draws
    assert np.allclose(got["lod"], np.log10((10.0 ** got["draw_lod"]).mean(axis=0)), rtol=0, atol=1e-12)


def test_marker_refusals(host):
    k, y, z = small_case()
    st = encode(k, 1)
    host.qtlimp_marker(st, y, cov=z)
    bad = st.copy()
    bad[5, 1] = 64
    with pytest.raises(ValueError):
        host.qtlimp_marker(bad, y, cov=z)
    bad[5, 1] = 255
    with pytest.raises(ValueError):
        host.qtlimp_marker(bad, y, cov=z)
    c = np.ones(len(k), bool)
    c[5] = False
    host.qtlimp_marker(bad, y, cov=z, c=c)                 # under a cleared mask the value is not read
    with pytest.raises(ValueError):
        host.qtlimp_marker(np.zeros((len(k), 1025), np.uint8), y, cov=z)
    with pytest.raises(ValueError):
        host.qtlimp_marker(np.zeros((len(k), 0), np.uint8), y, cov=z)
    with pytest.raises(ValueError):
        host.qtlimp_marker(st, y, cov=np.zeros((len(k), 9)))


# ------------------------------------------------------------------------------------- 3. the Python side
def test_sampled_classes():
    g = np.arange(64, dtype=np.uint8)
    k = qtl.sampled_classes(g)
    assert k.dtype == np.uint8 and np.array_equal(k, classes_of(g))
    assert np.array_equal(k[[0, 1, 8, 9, 0b110110, 0b111111]], [0, 1, 2, 3, 0, 3])
    mixed = np.array([[3, 255], [255, 8]], np.uint8)
    assert np.array_equal(qtl.sampled_classes(mixed), [[1, 255], [255, 2]])
    for bad in (64, 128, 254):
        with pytest.raises(ValueError):
            qtl.sampled_classes(np.array([0, bad], np.uint8))
    with pytest.raises(ValueError):
        qtl.sampled_classes(np.array([0, 1], np.int64))


class _NoGpu:
    """a context that fails the test as soon as anything is asked of the GPU"""
    n_ind, n_markers, n_chrom, device = 6, 5, 1, 0

    def __getattr__(self, name):
        raise AssertionError("scan_imp touched the context (%s) before it had checked its arguments" % name)


def test_scan_imp_value_errors():
    ctx, y = _NoGpu(), np.zeros((6, 2))
    states = np.zeros((6, 4, 5), np.uint8)
    for kwargs in (dict(pheno=np.zeros((5, 2))), dict(pheno=np.zeros((6, 2, 1))), dict(pheno=y, draws=0), dict(pheno=y, draws=1025),
                   dict(pheno=y, permutations=-1), dict(pheno=y, use=np.ones(5)), dict(pheno=y, states=states[:5]),
                   dict(pheno=y, states=states[:, :, :4]), dict(pheno=y, states=states[:, :0]), dict(pheno=y, states=states[0])):
        with pytest.raises(ValueError):
            qtl.scan_imp(ctx, **kwargs)


def test_symbols(host):
    from cnf2freq_amd import capi
    assert "cnf2h_qtlimp_marker" in host.SYMBOLS and hasattr(host.load(), "cnf2h_qtlimp_marker")
    L = capi.load()
    for name in ("cnf2_qtl_scan_imp", "cnf2_set_qtlimp_columns"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert capi.QTL_STATE_DEVICE == 1 << 29
    assert capi.QTL_STATE_DEVICE not in (capi.QTL_ADDITIVE, capi.QTL_ORIGIN_DEVICE, capi.QTL_REG_DEVICE, capi.QTL_IMPRINT,
                                         capi.NO_LINE_RECORDS, capi.NO_UNIFORM_PACK, capi.NO_UNIFORM_PACK8)


# ------------------------------------------------------------------------------------- 4. command line
def test_cli_usage_errors(host, tmp_path):
    """every one of these ends with status 2 and a message before a GPU is asked for"""
    import os
    import re
    import subprocess
    from conftest import ROOT
    exe, demo = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq"), os.path.join(ROOT, "tests", "golden", "demo")
    files = [os.path.join(demo, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    ph = tmp_path / "p.txt"
    ph.write_text("id weight\nC 1.0\nD NA\nF 2.5\n")
    base = ["--qtlimp", "i.txt", "--phenofile", str(ph)]
    for extra, text in ((["--qtlimp", "i.txt"], "^--qtlimp FILE needs --phenofile FILE$"),
                        (base + ["--qtl-imp-draws", "0"], "^--qtl-imp-draws must be 1 .. 1024$"),
                        (base + ["--qtl-imp-draws", "1025"], "^--qtl-imp-draws must be 1 .. 1024$"),
                        (base + ["--gpus", "2"], r"^--qtlimp needs a single GPU \(--gpus 1\)"),
                        (["--qtl-imp-draws", "4"], "^--qtl-imp-draws and --qtl-imp-seed need --qtlimp FILE$"),
                        (["--qtl-imp-seed", "5", "--qtl", "q.txt", "--phenofile", str(ph)],
                         "^--qtl-imp-draws and --qtl-imp-seed need --qtlimp FILE$"),
                        (base + ["--qtl-covariates", "height"], "height"),
                        # an existing message, word for word
                        (["--phenofile", str(ph)], "--phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed and --qtl-additive need --qtl FILE or --qtl2 FILE$")):
        args = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--count", "1", "--quiet", *extra]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 2, (extra, r.returncode, r.stderr[-300:])
        assert re.search(text, r.stderr, re.M), (extra, r.stderr[-300:])
        assert not (tmp_path / "i.txt").exists() and not (tmp_path / "q.txt").exists()
