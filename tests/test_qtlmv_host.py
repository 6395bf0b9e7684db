"""CPU suite: the host side of the multi-trait scan (cnf2_qtl_scan_mv).  One (marker, group) cell through the shared algebra
(cnf2h_qtlmv_marker, cnf2freq_amd/csrc/cnf2_qtlmv.h) against the least-squares determinants of tests/qtlmv_reference.py, the
group tile of cnf2_qtlplan.h, qtl.scan_mv's complete-case rule on a stub, and the command line's usage errors."""
import numpy as np
import pytest

from cnf2freq_amd import qtl
from qtl_reference import ATOL, CHROM_LENS, chromstarts_of, columns
from qtlmv_reference import CASES, case_reference, centred, conditions


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    h.load()
    return h


# ------------------------------------------------------------------------------------- 1. one cell on the CPU
@pytest.mark.parametrize("case", CASES, ids=["n%d-T%d" % c[:2] for c in CASES])
def test_marker_against_least_squares_determinants(host, case):
    n, T, P, K, additive = case
    (origin, pheno, cov, use, perm), ref = case_reference(case)
    cs = chromstarts_of(CHROM_LENS)
    worst_cond = conditions(ref, cs, additive)
    um = np.ones(n, bool) if use is None else use
    Y = columns(centred(pheno, um), perm)                      # [n][1 + P][T]
    z = None if cov is None else centred(cov, um)
    worst = 0.0
    for c in range(len(CHROM_LENS)):
        cm = um & (origin[:, cs[c]] != 0.0).any(axis=1)
        for m in range(cs[c], cs[c + 1]):
            for q in range(1 + P):
                got = host.qtlmv_marker(origin[:, m], Y[:, q], cov=z, c=cm, additive=additive)
                worst = max(worst, abs(got["lod"] - ref["lod"][q, m]))
                if q == 0:
                    assert got["rank"] == ref["rank"][m] and got["trait_rank"] == ref["trait_rank"][c]
                    assert got["n_used"] == ref["n_used"][c]
    print("n %d T %d: lod %.3g over %d cells, cond(E0) up to %.3g" % (n, T, worst, ref["lod"].size, worst_cond))
    assert worst <= ATOL


def test_marker_documented_cells(host):
    """a copy of a trait and a constant trait are dropped and change nothing; only constant traits: LOD exactly 0; fewer
    than K + 3 + T individuals: not scanned; bad arguments refused"""
    from qtl_reference import noise, soft_rows
    n = 20
    origin, _ = soft_rows(n, (3,), 6)
    o = origin[:, 1]
    y = centred(noise(n, 3, 6), None)
    base = host.qtlmv_marker(o, y)
    assert base == dict(lod=base["lod"], rank=2, trait_rank=3, n_used=n) and base["lod"] > 0.0
    copy = host.qtlmv_marker(o, np.column_stack([y, y[:, 1]]))
    assert copy["trait_rank"] == 3 and copy["lod"] == base["lod"]
    flat = host.qtlmv_marker(o, np.column_stack([y[:, 0], np.zeros(n), y[:, 1:]]))
    assert flat["trait_rank"] == 3 and abs(flat["lod"] - base["lod"]) <= ATOL
    none = host.qtlmv_marker(o, np.zeros((n, 2)))
    assert none == dict(lod=0.0, rank=0, trait_rank=0, n_used=n)
    cm = np.zeros(n, bool)
    cm[:6] = True                                            # K + 3 + T = 7 with K = 1
    z = centred(noise(n, 1, 7), None)
    few = host.qtlmv_marker(o, y, cov=z, c=cm)
    assert few == dict(lod=0.0, rank=0, trait_rank=0, n_used=6)
    cm[6] = True
    assert host.qtlmv_marker(o, y, cov=z, c=cm)["trait_rank"] == 3
    # T = 1 is the single scan's cell
    one = host.qtl_boot_marker(o, y[:, :1], np.ones(n, np.int32))
    assert abs(host.qtlmv_marker(o, y[:, :1])["lod"] - one["lod"][0]) <= ATOL
    for bad in (dict(y=np.zeros((n, 17))), dict(y=y, cov=np.zeros((n, 9)))):
        with pytest.raises(ValueError):
            host.qtlmv_marker(o, **bad)


# ------------------------------------------------------------------------------------- 2. the group tile
def test_group_tile(host):
    t = host.qtl_group_tile
    # few individuals: 4096 columns of the padded image, in whole groups; never more than G
    assert t(100, 4, 10000, 9999, 10) == 1024 and t(100, 3, 10000, 9999, 10) == 1024
    assert t(100, 5, 10000, 9999, 10) == 512 and t(100, 8, 10000, 9999, 10) == 512
    assert t(100, 9, 10000, 9999, 10) == 256 and t(100, 16, 10000, 9999, 10) == 256
    assert t(100, 16, 7, 6, 10) == 7 and t(100, 1, 1, 0, 10) == 1
    # the 1 GB rule: 2^30 / (8 n) columns, at least 16 of them, at least one group
    n = 1 << 20
    assert t(n, 4, 1000, 999, 10) == 128 // 4 and t(n, 16, 1000, 999, 10) == 128 // 16
    assert t(1 << 23, 4, 1000, 999, 10) == 4 and t(1 << 23, 16, 1000, 999, 10) == 1 and t(1 << 26, 16, 1000, 999, 10) == 1
    # the 256 MB rule on the maxima: n_tiles doubles per group, only with permutations
    tiles = 1 << 20
    assert t(100, 4, 10000, 9999, tiles) == (1 << 28) // (8 * tiles) == 32
    assert t(100, 4, 10000, 9999, 1 << 26) == 1
    assert t(100, 4, 1, 0, 1 << 26) == 1
    # the cap counts groups
    assert t(100, 4, 10000, 9999, 10, 3) == 3 and t(100, 16, 2, 1, 10, 3) == 2 and t(100, 4, 10000, 9999, 10, 0) == 1024
    for bad in ((100, 0, 1, 0, 1), (100, 17, 1, 0, 1), (100, 4, 0, 0, 1), (-1, 4, 1, 0, 1)):
        with pytest.raises(ValueError):
            t(*bad)


# ------------------------------------------------------------------------------------- 3. complete cases
class StubRows:
    def data_ptr(self):
        return 64


class StubContext:
    """what qtl.scan_mv asks of a context, recording every call"""
    n_ind, n_markers, n_chrom = 6, 5, 2

    def __init__(self):
        self.calls = []

    def qtl_scan_mv_device(self, n, d_origin, pheno, cov=None, use=None, perm=None, additive=False):
        self.calls.append(dict(n=n, d_origin=d_origin, pheno=np.array(pheno), cov=cov, use=np.array(use), perm=perm, additive=additive))
        P = 0 if perm is None else len(perm)
        return dict(lod=np.arange(5.0), rank=np.full(5, 2, np.int32), trait_rank=np.full(2, pheno.shape[1], np.int32),
                    n_used=np.full(2, int(np.sum(use)), np.int32), perm_max=np.ones((P, 2)) if P else None)


def test_scan_mv_takes_complete_cases():
    y = np.arange(18.0).reshape(6, 3)
    y[1, 2] = np.nan
    y[4, 0] = np.inf
    use = np.array([1, 1, 1, 0, 1, 1], bool)
    ctx = StubContext()
    out = qtl.scan_mv(ctx, y, use=use, rows=StubRows())
    assert len(ctx.calls) == 1 and out["perm_max"] is None
    call = ctx.calls[0]
    assert list(call["use"]) == [True, False, True, False, False, True] and call["d_origin"] == 64 and call["perm"] is None
    assert np.isfinite(call["pheno"]).all() and np.array_equal(call["pheno"][[0, 2, 5]], y[[0, 2, 5]])
    assert list(out["n_used"]) == [3, 3] and out["lod"].shape == (5,)
    # with permutations: a second call, the permutations of the complete cases, perm_max as thresholds and peaks read it
    cov = np.arange(6.0)[:, None] ** 2
    out = qtl.scan_mv(ctx, y, cov=cov, use=use, permutations=4, seed=3, additive=True, rows=StubRows())
    assert len(ctx.calls) == 3 and out["perm_max"].shape == (4, 1, 2)
    second = ctx.calls[2]
    assert np.array_equal(second["perm"], qtl.permutations(6, 4, 3, use=call["use"])) and second["additive"]
    assert np.allclose(second["pheno"], qtl.null_residuals(call["pheno"], cov, call["use"]))
    assert qtl.thresholds(out["perm_max"])["genome"].shape == (2, 1)
    with pytest.raises(ValueError):
        qtl.scan_mv(ctx, y[:5], rows=StubRows())


# ------------------------------------------------------------------------------------- 4. symbols and the command line
def test_symbols(host):
    from cnf2freq_amd import capi
    assert {"cnf2_qtl_scan_mv", "cnf2_set_qtlmv_groups"} <= set(capi.SYMBOLS)
    assert {"cnf2h_qtlmv_marker", "cnf2h_qtl_group_tile"} <= set(host.SYMBOLS)
    L = host.load()
    assert all(hasattr(L, s) for s in ("cnf2h_qtlmv_marker", "cnf2h_qtl_group_tile"))
    assert hasattr(capi.Context, "qtl_scan_mv") and hasattr(capi.Context, "qtl_scan_mv_device") and hasattr(qtl, "scan_mv")


def test_cli_usage_errors(host, tmp_path):
    """every one of these ends with status 2 and a message before a GPU is asked for"""
    import os
    import re
    import subprocess
    from conftest import ROOT
    exe, demo = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq"), os.path.join(ROOT, "tests", "golden", "demo")
    files = [os.path.join(demo, "demoplantimpute." + e) for e in ("map", "ped", "gen")]
    ph = tmp_path / "p.txt"
    ph.write_text("id weight height\nC 1.0 2.0\nD NA 1.0\nF 2.5 3.0\n")
    wide = tmp_path / "wide.txt"
    wide.write_text("id " + " ".join("t%d" % t for t in range(17)) + "\n" + "C " + " ".join(["1.0"] * 17) + "\n")
    base = ["--qtlmv", "m.txt", "--phenofile", str(ph)]
    for extra, text in ((["--qtlmv", "m.txt"], "^--qtlmv FILE needs --phenofile FILE$"),
                        (base + ["--qtl-traits", "weight,girth"], "^--qtl-traits: the phenotype file has no trait girth$"),
                        (["--qtlmv", "m.txt", "--phenofile", str(wide)], "^--qtlmv takes 1 .. 16 traits, not 17$"),
                        (base + ["--gpus", "2"], r"^--qtlmv needs a single GPU \(--gpus 1\)"),
                        (["--qtl-traits", "weight", "--qtl", "q.txt", "--phenofile", str(ph)], "^--qtl-traits needs --qtlmv FILE$")):
        args = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--count", "1", "--quiet", *extra]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 2, (extra, r.returncode, r.stderr[-300:])
        assert re.search(text, r.stderr, re.M), (extra, r.stderr[-300:])
        assert not (tmp_path / "m.txt").exists() and not (tmp_path / "q.txt").exists()
