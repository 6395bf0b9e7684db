"""bench.py --gpus N starts N ranks by itself (no launcher around it): the parent must not have imported anything that
initialises HIP when it spawns `python -m torch.distributed.run ...` as a child, and it leaves with the child's exit
code.  The partition the ranks take is the reference's own (cnF2freq.cpp:5297-5299).  On a box without a GPU the ranks
stop with "bench.py needs a GPU" -- which is exactly what shows that N of them were started."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def test_requested_gpus_parsing():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.requested_gpus(["--steps", "3"]) == 1
    assert bench.requested_gpus(["--gpus", "4", "--steps", "3"]) == 4
    assert bench.requested_gpus(["--steps", "3", "--gpus=8"]) == 8


def test_a_rank_or_one_gpu_never_spawns(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    assert bench.launch_ranks(["--gpus", "1"]) is None
    assert bench.launch_ranks([]) is None
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert bench.launch_ranks(["--gpus", "2"]) is None      # already a rank of a launcher's group


def test_parent_spawns_ranks_before_touching_hip(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("the CPU form of this test: the GPU form is test_bench_two_ranks_without_a_launcher")
    trace = tmp_path / "parent.json"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["CNF2_BENCH_PARENT_TRACE"] = str(trace)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--backend", "gloo", "--single-device", "--inds", "16",
                        "--chroms", "1", "--snps-per-chrom", "50", "--steps", "1", "--warmup", "0", "--cpu-seconds", "0"],
                       env=env, capture_output=True, text=True, timeout=600)
    t = json.load(open(trace))
    mods = set(t["modules"])
    for bad in ("torch", "numpy", "ctypes", "cnf2freq_amd", "cnf2freq_amd.capi", "__graft_entry__"):
        assert bad not in mods, "the parent had imported %s before the spawn" % bad
    assert t["cmd"][1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in t["cmd"]
    assert t["cmd"][t["cmd"].index("--nproc-per-node") + 1] == "2"
    assert "--standalone" in t["cmd"] and "127.0.0.1" in t["cmd"]       # torchrun picks the rendezvous port itself
    # no GPU here: the ranks refuse to run (no CPU fallback), and the parent relays the failure
    assert r.returncode != 0
    assert "needs a GPU" in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip() == ""


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sweep", "iterations"])
def test_bench_two_ranks_without_a_launcher(mode):
    """`python bench.py --gpus 2 --full` on a one-GPU box (gloo transport, both ranks on GPU 0): one JSON line, n_gpus = 2, a
    roofline entry per rank and the CPU baseline beside it."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, BENCH, "--gpus", "2", "--backend", "gloo", "--single-device", "--steps", "2", "--warmup", "1", "--full"]
    if mode == "sweep":
        cmd += ["--inds", "300", "--chroms", "2", "--snps-per-chrom", "400", "--cpu-seconds", "1"]
    else:
        cmd += ["--workload", "outbred", "--iterations", "2", "--inds", "240", "--chroms", "2", "--snps-per-chrom", "300",
                "--cpu-seconds", "1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["value"] > 0
    if mode == "sweep":
        assert out["scaling"] == "weak"
        assert len(out["roofline"]["per_rank"]) == 2
        assert all(p["kernel_ms"] > 0 for p in out["roofline"]["per_rank"])
        assert out["cpu_baseline"]["value"] > 0
        assert all(out["checks"].values())
    else:
        assert out["scaling"] == "strong"
        assert "exchange_bytes_per_iteration" in out


def test_dump_outputs_is_a_fixed_sample_within_the_cap(tmp_path):
    """--dump-outputs: small arrays whole, a large one as a seeded sample of (row, column) positions with the positions beside
    it; the same shapes give the same files, float64, under 64 MB in all."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n, m = 4000, 5000
    dosage = torch.arange(n * m * 3, dtype=torch.float64).view(n, m, 3)
    arrays = {"loglik": torch.linspace(-1.0, -2.0, n * 2, dtype=torch.float64).view(n, 2), "dosage": dosage,
              "allele": np.full((n, m, 2), 2, np.uint8)}
    budget = 8 << 20
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["allele.npy", "allele_index.npy", "dosage.npy", "dosage_index.npy", "loglik.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget + 128 * len(files)
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b), f
    assert np.array_equal(np.load(tmp_path / "a" / "loglik.npy"), arrays["loglik"].numpy())
    idx = np.load(tmp_path / "a" / "dosage_index.npy").astype(np.int64)
    assert len(np.unique(idx[:, 0] * m + idx[:, 1])) == len(idx) > 1000
    assert np.array_equal(np.load(tmp_path / "a" / "dosage.npy"), dosage.numpy()[idx[:, 0], idx[:, 1]])
    assert (np.load(tmp_path / "a" / "allele.npy") == 2).all()
    assert bench.DUMP_BYTES + 4096 <= 64 * 10 ** 6


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run (no --full): one JSON line with the headline fields, --steps timed steps, none of the extras; its
    --dump-outputs files are the last timed step's outputs, the same in two runs with the same arguments."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    outs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--inds", "300", "--chroms", "2",
                            "--snps-per-chrom", "400", "--dump-outputs", str(tmp_path / d)],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        outs.append(json.loads(lines[0]))
    out = outs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "f64"
    assert out["checks"] is None
    for k in ("cpu_baseline", "iteration_probe", "merge_modes"):
        assert k not in out, k
    f = np.load(tmp_path / "a" / "factors.npy")
    ll = np.load(tmp_path / "a" / "loglik.npy")
    dos = np.load(tmp_path / "a" / "dosage.npy")
    assert f.shape == (300, 2, 8) and ll.shape == (300, 2) and dos.shape == (300, 802, 3)
    assert np.isfinite(ll).all() and (ll < 0).all() and np.allclose(dos.sum(axis=2), 1.0, atol=1e-9)
    assert np.isclose(ll.sum(), out["loglik_checksum"], rtol=1e-12)
    for name in ("factors", "loglik", "dosage"):
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))), name
