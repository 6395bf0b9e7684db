"""Host side of posterior sampling (no GPU): the generator the draws use (cnf2freq_amd/sampling.py against SplitMix64's
check values and a big-integer restatement), the state order, and the command-line combinations that are refused before
any GPU is touched."""
import os
import subprocess

import numpy as np
import pytest

from cnf2freq_amd import sampling, synth

M64 = (1 << 64) - 1


def mix_int(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u_int(seed, i, k, j):
    key = mix_int(mix_int(mix_int(seed) ^ i) ^ k)
    return (mix_int(key ^ j) >> 11) * 2.0 ** -53


def test_splitmix64_check_values():
    assert int(synth.splitmix64(0, 0)) == 0xE220A8397B1DCDAF
    assert int(synth.splitmix64(0x9E3779B97F4A7C15, 0)) == 0x6E789E6AA1B965F4
    assert mix_int(0) == 0xE220A8397B1DCDAF and mix_int(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_uniforms_match_big_int_restatement():
    rng = np.random.default_rng(5)
    seeds = [0, 1, 7, (1 << 63), (1 << 63) + 12345, M64, int(rng.integers(0, 1 << 62)) * 3]
    for seed in seeds:
        ind = rng.integers(0, 100000, 40)
        draw = rng.integers(0, 1024, 40)
        j = rng.integers(0, 300000, 40)
        got = sampling.uniforms(seed, ind, draw, j)
        assert got.dtype == np.float64 and got.shape == (40,)
        want = np.array([u_int(seed, int(a), int(b), int(c)) for a, b, c in zip(ind, draw, j)])
        assert np.array_equal(got, want), seed
        assert np.all((got >= 0.0) & (got < 1.0))
    # broadcasting: one individual, every draw and marker
    g = sampling.uniforms(3, 11, np.arange(5)[:, None], np.arange(7)[None, :])
    assert g.shape == (5, 7)
    assert g[4, 6] == u_int(3, 11, 4, 6)


def test_state_order_is_a_permutation():
    order = np.asarray(sampling.STATE_ORDER)
    assert order.shape == (64,)
    assert np.array_equal(np.sort(order), np.arange(64))


def run_cli(tmp_path, *extra):
    from conftest import ROOT
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    demo = os.path.join(ROOT, "tests", "golden", "demo")
    base = [exe, "--mapfile", os.path.join(demo, "demoplantimpute.map"), "--pedfile", os.path.join(demo, "demoplantimpute.ped"),
            "--genfile", os.path.join(demo, "demoplantimpute.gen"), "--quiet"]
    return subprocess.run(base + list(extra), capture_output=True, text=True, timeout=120, cwd=str(tmp_path))


@pytest.mark.parametrize("extra, msg", [
    (("--gpus", "2", "--sample", "s.txt"), "single GPU"),
    (("--draws", "3"), "--sample"),
    (("--seed", "7"), "--sample"),
    (("--sample", "s.txt", "--draws", "0"), "--draws"),
    (("--sample", "s.txt", "--draws", "1025"), "--draws"),
])
def test_cli_refuses_sampling_flags_it_cannot_honour(tmp_path, extra, msg):
    """checked before any GPU is touched: exit code 2 and a message"""
    r = run_cli(tmp_path, *extra)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert msg in r.stderr
    assert not (tmp_path / "s.txt").exists()
