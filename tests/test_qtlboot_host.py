"""CPU suite: the host side of the bootstrap scan (cnf2_qtl_scan_boot).  The counts of qtl.bootstrap_counts against
cnf2h_qtl_bootstrap_counts, one (replicate, marker) cell through the shared algebra (cnf2h_qtl_boot_marker,
cnf2freq_amd/csrc/cnf2_qtlboot.h) against least squares on literally resampled rows (tests/qtlboot_reference.py), and the
two interval readers of cnf2freq_amd/qtl.py on hand-made arrays."""
import numpy as np
import pytest

from cnf2freq_amd import qtl
from qtl_reference import ATOL, chromstarts_of
from qtlboot_reference import CASES, case_reference, conditions


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    h.load()
    return h


# ------------------------------------------------------------------------------------- 1. the counts
def test_bootstrap_counts_match_the_host_library(host):
    n, B = 37, 9
    use = np.ones(n, bool)
    use[[3, 20, 36]] = False
    strata = (np.arange(n) * 7 % 3).astype(np.int32)
    for u, st in ((None, None), (use, None), (None, strata), (use, strata)):
        py = qtl.bootstrap_counts(n, B, 5, use=u, strata=st)
        assert py.dtype == np.int32 and py.shape == (B, n)
        assert np.array_equal(py, host.qtl_bootstrap_counts(n, B, 5, use=u, strata=st))
        um = np.ones(n, bool) if u is None else u
        sm = np.zeros(n, np.int32) if st is None else st
        assert np.all(py >= 0) and np.all(py[:, ~um] == 0)
        for s in np.unique(sm):
            assert np.all(py[:, um & (sm == s)].sum(axis=1) == (um & (sm == s)).sum())     # a stratum keeps its size
        assert len({r.tobytes() for r in py}) == B                                         # the replicates differ
    a, b = qtl.bootstrap_counts(n, B, 5), qtl.bootstrap_counts(n, B, 6)
    assert not np.array_equal(a, b)
    assert np.array_equal(a, qtl.bootstrap_counts(n, B, 5))
    assert np.array_equal(a[:4], qtl.bootstrap_counts(n, 4, 5))                            # replicate b does not depend on B
    assert qtl.bootstrap_counts(n, 0, 5).shape == (0, n)


def test_bootstrap_counts_follow_the_written_rule():
    """draw j of replicate b picks idx[floor(u k)] with u = synth.uniform(seed, b n + j): spelled out one draw at a time"""
    from cnf2freq_amd import synth
    n, B, seed = 11, 3, 8
    use = np.ones(n, bool)
    use[4] = False
    idx = np.flatnonzero(use)
    want = np.zeros((B, n), np.int32)
    for b in range(B):
        for j in idx:
            want[b, idx[int(np.floor(float(synth.uniform(seed, b * n + int(j))) * len(idx)))]] += 1
    assert np.array_equal(qtl.bootstrap_counts(n, B, seed, use=use), want)


# ------------------------------------------------------------------------------------- 2. one cell on the CPU
def centred(v, use):
    """the columns minus their unweighted means over the used individuals, as the scan forms them"""
    v = np.array(v, np.float64)
    v[use] -= v[use].mean(axis=0)
    v[~use] = 0.0
    return v


@pytest.mark.parametrize("case", CASES, ids=["n%d" % c[0] for c in CASES])
def test_boot_marker_against_resampled_least_squares(host, case):
    n, T, K, B, additive, lens, seed = case
    (origin, pheno, cov, use, count), ref = case_reference(case)
    conditions(ref, K, additive, "n %d" % n)
    cs = chromstarts_of(lens)
    um = np.ones(n, bool) if use is None else use
    y = centred(pheno, um)
    z = None if cov is None else centred(cov, um)
    worst = 0.0
    for c in range(len(lens)):
        cm = um & (origin[:, cs[c]] != 0.0).any(axis=1)
        for b in range(B):
            for m in range(cs[c], cs[c + 1]):
                got = host.qtl_boot_marker(origin[:, m], y, count[b], cov=z, c=cm, additive=additive)
                assert got["n_bc"] == ref["n_boot"][b, c]
                assert got["rank"] == ref["rank"][b, m]
                worst = max(worst, np.abs(got["lod"] - ref["lod"][b, :, m]).max())
    print("n %d: lod %.3g over %d cells" % (n, worst, ref["lod"].size))
    assert worst <= ATOL


def test_boot_marker_documented_cells(host):
    """all the weight on K + 3 individuals: not fitted; a binary covariate that the replicate makes constant: not fitted; a
    negative count: refused"""
    from qtl_reference import noise, soft_rows
    n = 20
    origin, _ = soft_rows(n, (3,), 6)
    y = noise(n, 1, 6)
    few = np.zeros(n, np.int32)
    few[:4] = 1                                             # K = 1: K + 3 individuals
    z = (np.arange(n) % 2).astype(np.float64)[:, None] - 0.5
    got = host.qtl_boot_marker(origin[:, 1], y, few, cov=z)
    assert got["n_bc"] == 4 and got["rank"] == 0 and got["lod"][0] == 0.0 and np.isnan(got["coef"]).all()
    even = np.where(np.arange(n) % 2 == 0, 2, 0).astype(np.int32)      # only the individuals with z = -0.5
    got = host.qtl_boot_marker(origin[:, 1], y, even, cov=z)
    assert got["n_bc"] == n and got["rank"] == 0 and got["lod"][0] == 0.0
    assert host.qtl_boot_marker(origin[:, 1], y, np.ones(n, np.int32), cov=z)["lod"][0] > 0.0
    bad = np.ones(n, np.int32)
    bad[5] = -1
    with pytest.raises(ValueError):
        host.qtl_boot_marker(origin[:, 1], y, bad, cov=z)


# ------------------------------------------------------------------------------------- 3. the interval readers
def test_boot_interval_on_hand_made_arrays():
    pos = np.array([0.0, 1.0, 2.5, 4.0, 7.0, 7.0])
    # every replicate on one marker
    r = qtl.boot_interval(np.full(40, 3), pos)
    assert (r["lo"], r["hi"], r["pos_lo"], r["pos_hi"], r["V"], r["left_out"]) == (3, 3, 4.0, 4.0, 40, 0)
    assert r["share"][3] == 1.0 and r["share"].sum() == 1.0
    # -1 entries are left out and counted; nothing usable: NaN and -1
    r = qtl.boot_interval(np.array([-1, 2, -1, 2, 1, -1]), pos)
    assert (r["V"], r["left_out"]) == (3, 3) and np.allclose(r["share"], [0, 1 / 3, 2 / 3, 0, 0, 0])
    assert (r["lo"], r["hi"]) == (1, 2)
    r = qtl.boot_interval(np.array([-1, -1]), pos)
    assert r["V"] == 0 and r["left_out"] == 2 and r["lo"] == r["hi"] == -1 and np.isnan(r["pos_lo"]) and np.isnan(r["pos_hi"])
    assert np.all(r["share"] == 0.0)
    # a tie in mass between two markers: the order statistics decide, lo = p_(floor(0.025 V)), hi = p_(ceil(0.975 V) - 1)
    r = qtl.boot_interval(np.array([1] * 100 + [3] * 100), pos)
    assert (r["lo"], r["hi"], r["pos_lo"], r["pos_hi"]) == (1, 3, 1.0, 4.0) and r["share"][1] == r["share"][3] == 0.5
    # V = 200: the cut points are the entries number 5 and 194 of the sorted positions (0.975 * 200 = 195, not 196)
    arg = np.array([0] * 5 + [2] * 189 + [3] * 1 + [4] * 5)
    r = qtl.boot_interval(arg, pos)
    assert (r["lo"], r["hi"]) == (2, 3)
    r = qtl.boot_interval(np.array([0] * 6 + [2] * 189 + [4] * 5), pos)
    assert (r["lo"], r["hi"]) == (0, 2)
    # level: the 50 % interval of the same replicates; equal positions sort by marker
    assert qtl.boot_interval(arg, pos, level=0.5)["lo"] == 2
    r = qtl.boot_interval(np.array([5] * 10 + [4] * 10), pos)
    assert (r["lo"], r["hi"]) == (4, 5)
    with pytest.raises(ValueError):
        qtl.boot_interval(np.array([6]), pos)


def test_bayes_interval_on_hand_made_arrays():
    cs = chromstarts_of((4, 1, 3))
    pos = np.array([0.0, 10.0, 20.0, 30.0, 0.0, 0.0, 4.0, 6.0])
    lod = np.array([0.0, 3.0, 0.0, 0.0, 1.0, 2.0, 2.0, 2.0])
    # chromosome 0: half-gap widths 5, 10, 10, 5; posterior of marker 1 = 10000 / 10020
    r = qtl.bayes_interval(lod, pos, cs, 0)
    assert (r["lo"], r["hi"]) == (1, 1) and np.isclose(r["mass"], 10000.0 / 10020.0) and np.isclose(r["posterior"].sum(), 1.0)
    assert np.allclose(r["posterior"], np.array([5.0, 10000.0, 10.0, 5.0]) / 10020.0)
    r = qtl.bayes_interval(lod, pos, cs, 0, prob=0.999)
    assert (r["lo"], r["hi"]) == (1, 2) and (r["pos_lo"], r["pos_hi"]) == (10.0, 20.0)       # 0 .. 1 holds 0.9985, 1 .. 2 holds 0.9990
    # a single marker is its own interval
    r = qtl.bayes_interval(lod, pos, cs, 1)
    assert (r["lo"], r["hi"], r["mass"]) == (4, 4, 1.0)
    # equal LODs: the posterior is the widths 2, 3, 1 over 6; 0.8 needs markers 5 and 6 (0.833), the run 6 .. 7 holds 0.667
    r = qtl.bayes_interval(lod, pos, cs, 2, prob=0.8)
    assert (r["lo"], r["hi"]) == (5, 6) and np.isclose(r["mass"], 5.0 / 6.0)
    r = qtl.bayes_interval(lod, pos, cs, 2, prob=0.5)
    assert (r["lo"], r["hi"]) == (6, 6) and np.isclose(r["mass"], 0.5)
    with pytest.raises(ValueError):
        qtl.bayes_interval(lod, pos, cs, 3)


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
    base = ["--qtlboot", "b.txt", "--phenofile", str(ph)]
    for extra, text in ((["--qtlboot", "b.txt", "--qtl-boot-chrom", "1"], "^--qtlboot FILE needs --phenofile FILE$"),
                        (base, r"^--qtlboot FILE needs --qtl-boot-chrom C with C = 1 \.\. 1, the chromosomes of the map$"),
                        (base + ["--qtl-boot-chrom", "2"], "^--qtlboot FILE needs --qtl-boot-chrom C with C = 1 .. 1"),
                        (base + ["--qtl-boot-chrom", "1", "--qtl-boot-replicates", "0"], "^--qtl-boot-replicates must be 1 .. 1000000$"),
                        (base + ["--qtl-boot-chrom", "1", "--gpus", "2"], r"^--qtlboot needs a single GPU \(--gpus 1\)"),
                        (["--qtl-boot-chrom", "1"], "^--qtl-boot-chrom and --qtl-boot-replicates need --qtlboot FILE$"),
                        (["--qtl-boot-replicates", "5", "--qtl", "q.txt", "--phenofile", str(ph)],
                         "^--qtl-boot-chrom and --qtl-boot-replicates need --qtlboot FILE$"),
                        # an existing message, word for word
                        (["--phenofile", str(ph)], "--phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed and --qtl-additive need --qtl FILE or --qtl2 FILE$")):
        args = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--count", "1", "--quiet", *extra]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 2, (extra, r.returncode, r.stderr[-300:])
        assert re.search(text, r.stderr, re.M), (extra, r.stderr[-300:])
        assert not (tmp_path / "b.txt").exists() and not (tmp_path / "q.txt").exists()
