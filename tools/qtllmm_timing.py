"""Measurement aid: wall time, ending in a device synchronise, of the polygenic scan's parts on a synthetic F2 (synth.make_f2);
config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs (+1 dummy marker each), one trait, no covariate.
  1. cnf2_kinship_sums over the whole map (device rows, device outputs) beside torch's A @ A.T on an extracted a image
     [n][M] -- one process, the calls alternating, best of `repeats` with the spread -- and the largest difference of the two
  2. one qtl.scan_lmm call (one kinship for the genome: one eigendecomposition) split into kinship, eigh, the column scans
     and the rest (rotation by torch matmuls, est_herit, host work), by timing the functions it calls
usage: python tools/qtllmm_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

a = [int(x) for x in sys.argv[1:5]] + [10000, 2500, 20, 3][len(sys.argv[1:5]):]
n, snps, chroms, reps = a
t0 = time.perf_counter()
ped = synth.make_f2(n, snps, chroms, seed=2)
gen_s = time.perf_counter() - t0
ctx = capi.Context(0)
ctx.upload(ped)
M, dev = ped.n_markers, torch.device("cuda", 0)
t0 = time.perf_counter()
org = qtl.origin_rows(ctx)
torch.cuda.synchronize(dev)
print("%d F2 x %d markers (%d chromosomes; input %.1f s, origin sweep %.2f s); times in s, ending in a synchronise" % (
    n, M, chroms, gen_s, time.perf_counter() - t0), flush=True)

# ---- 1. the kinship sums beside torch
img = (org[:, :, 3] - org[:, :, 0]).contiguous()
S = torch.zeros((n, n), dtype=torch.float64, device=dev)
cnt = torch.zeros(1, dtype=torch.int32, device=dev)
out = {}


def ours():
    ctx.kinship_sums_device(n, org.data_ptr(), 0, chroms, d_sum=S.data_ptr(), d_n_markers=cnt.data_ptr())
    ctx.sync()


def theirs():
    out["t"] = img @ img.T
    torch.cuda.synchronize(dev)


calls = [("cnf2_kinship_sums", ours), ("torch A @ A.T", theirs)]
for _, fn in calls:
    fn()
times = {name: [] for name, _ in calls}
for _ in range(reps):
    for name, fn in calls:
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
flop = 2.0 * n * n * M
for name, _ in calls:
    t = min(times[name])
    print("  %-20s %.4f (all: %s; spread %.2f %%), %.1f Tflop/s of the full product" % (
        name, t, " ".join("%.4f" % v for v in times[name]), 100 * (max(times[name]) - t) / t, flop / t / 1e12), flush=True)
print("  largest difference of the two, relative to the largest sum: %.3g; S == S.T to the bit: %s" % (
    float((S - out["t"]).abs().max() / S.abs().max()), bool(torch.equal(S, S.T))), flush=True)
del img, out

# ---- 2. one scan_lmm call, split
g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
cs = np.asarray(ped.chromstarts, np.int64)
pheno = 0.3 * g(int((cs[0] + cs[1]) // 2)) + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5)
spent = {"kinship": 0.0, "eigh": 0.0, "column scans": 0.0}


def timed(key, fn):
    def run(*args, **kw):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = fn(*args, **kw)
        torch.cuda.synchronize(dev)
        spent[key] += time.perf_counter() - t0
        return r
    return run


qtl._kinship = timed("kinship", qtl._kinship)
qtl._eigh = timed("eigh", qtl._eigh)
ctx.qtl_scan_cols_device = timed("column scans", ctx.qtl_scan_cols_device)
t0 = time.perf_counter()
res = qtl.scan_lmm(ctx, pheno, loco=False, rows=org)
torch.cuda.synchronize(dev)
total = time.perf_counter() - t0
print("qtl.scan_lmm, loco=False, one trait: %.2f in all" % total)
for key, v in spent.items():
    print("  %-14s %.3f" % (key, v))
print("  %-14s %.3f (rotation U'[a, d] by torch matmuls, est_herit, host work)" % ("the rest", total - sum(spent.values())))
print("  h2 %.4f, largest LOD %.2f at marker %d (effect planted at %d)" % (
    res["h2"][0, 0], res["lod"].max(), int(np.argmax(res["lod"][0])), int((cs[0] + cs[1]) // 2)))
ctx.close()
