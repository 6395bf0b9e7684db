"""CPU suite: the M-step of the marker map (cnf2h_map_mstep, csrc/host/cnf2_remap.cpp) and the map writer that the
`--remap` flag and cnf2freq_amd/remap.py share (cnf2h_write_map)."""
import numpy as np
import pytest

TYPEGENS = np.array([1, 0, 0, 1, 0, 0])


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    h.load()
    return h


def objective(d, S, C, genrec):
    g = np.array([genrec[t] for t in TYPEGENS])
    r = 0.5 * (1.0 - np.exp(g * d))
    return np.sum(S * np.log(r) + (C - S) * np.log1p(-r))


def one(host, S, C, genrec, dist=10.0):
    pos = np.array([0.0, dist])
    out = host.map_mstep(pos, [0, 2], np.array([S, np.zeros(6)]), [C], genrec)
    assert out[0] == 0.0
    return out[1]


def test_closed_form_equal_rates(host):
    S = np.array([3.0, 1.0, 2.5, 4.0, 0.5, 1.0])
    C = 100
    d = one(host, S, C, [-0.02, -0.02, -0.02])
    r = S.sum() / (6 * C)
    assert d == pytest.approx(np.log(1 - 2 * r) / -0.02, rel=1e-14)


@pytest.mark.parametrize("genrec", [(-0.02, -0.03, -0.02), (-0.05, -0.01, 0.0), (-0.011, -0.04, -0.02)])
@pytest.mark.parametrize("seed", range(4))
def test_newton_matches_brute_force(host, genrec, seed):
    rng = np.random.default_rng(seed)
    C = int(rng.integers(5, 500))
    S = rng.uniform(0, 0.3, 6) * C
    d = one(host, S, C, genrec)
    grid = np.linspace(1e-3, 400, 400001)
    g = np.array([genrec[t] for t in TYPEGENS])
    r = 0.5 * (1.0 - np.exp(np.outer(grid, g)))
    vals = (S * np.log(r) + (C - S) * np.log1p(-r)).sum(axis=1)
    k = int(np.argmax(vals))
    lo, hi = grid[max(k - 1, 0)], grid[min(k + 1, len(grid) - 1)]
    assert lo - 1e-9 <= d <= hi + 1e-9, (d, grid[k])
    # and it is a maximum at least as good as the grid's best
    assert objective(d, S, C, genrec) >= vals[k] - 1e-9 * abs(vals[k])


def test_clamps_and_untouched_intervals(host):
    # no crossovers at all: r clamped to 1e-9 (the interval does not close); every meiosis recombined: r clamped to 0.499
    d0 = one(host, np.zeros(6), 50, [-0.02, -0.02, -0.02])
    assert d0 == pytest.approx(np.log(1 - 2e-9) / -0.02, rel=1e-12) and d0 > 0
    d1 = one(host, np.full(6, 50.0), 50, [-0.02, -0.02, -0.02])
    assert d1 == pytest.approx(np.log(1 - 2 * 0.499) / -0.02, rel=1e-12)
    d2 = one(host, np.full(6, 50.0), 50, [-0.02, -0.03, -0.02])
    assert np.isfinite(d2) and d2 > 0
    # zero-length gaps, chromosomes without contributors and the chromosome starts stay as they are
    pos = np.array([5.0, 5.0, 8.0, 12.0, 1.0, 3.0, 4.0])
    cs = np.array([0, 4, 7], np.int32)
    xs = np.full((7, 6), 2.0)
    out = host.map_mstep(pos, cs, xs, [40, 0])
    assert out[0] == 5.0 and out[1] == 5.0 and out[4] == 1.0
    assert np.array_equal(out[4:], pos[4:])
    r = 12.0 / (6 * 40)
    dd = np.log(1 - 2 * r) / -0.02
    np.testing.assert_allclose(np.diff(out[1:4]), [dd, dd], rtol=1e-14)


def test_map_writer_round_trip(host, tmp_path):
    pos = np.array([0.0, 1.25, 1.0 / 3.0 + 2, 7.5, 0.5, 0.75, 10.0])
    cs = np.array([0, 4, 7], np.int32)
    p = tmp_path / "m.map"
    host.write_map(str(p), pos, cs)
    back = np.array([float(v) for v in p.read_text().split()])
    assert np.array_equal(back, pos)
    # a chromosome grown past the next one's first position would merge with it: refused loudly
    bad = pos.copy()
    bad[4:] += 20.0
    with pytest.raises(RuntimeError, match="same chromosomes"):
        host.write_map(str(tmp_path / "bad.map"), bad, cs)


def test_cli_refuses_crossover_flags_it_cannot_honour(host, tmp_path):
    """checked before any GPU is touched: the flags of several ranks, and --remap-iterations without --remap, exit 2"""
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    demo = os.path.join(ROOT, "tests", "golden", "demo")
    base = [exe, "--mapfile", os.path.join(demo, "demoplantimpute.map"), "--pedfile", os.path.join(demo, "demoplantimpute.ped"),
            "--genfile", os.path.join(demo, "demoplantimpute.gen"), "--quiet"]
    r = subprocess.run(base + ["--gpus", "2", "--crossovers", str(tmp_path / "xo.txt")], capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and "single GPU" in r.stderr
    r = subprocess.run(base + ["--remap-iterations", "3"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and "--remap-iterations needs --remap" in r.stderr
