"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scan_mv against cnf2_qtl_scan of the same tree on
the same device rows, the same traits and the same permutations -- the same R = T (1 + P) columns and so the same product;
the ratio shows what the null fit per group, the padding of the traits to 4, 8 or 16 columns and the whitening cost.  One
process, the two calls alternating, tools/qtl_timing.py's set-up: a synthetic F2 (synth.make_f2), config 2 of BASELINE:
10 000 individuals x 20 chromosomes x 2 500 SNPs (+1 dummy marker each).
usage: python tools/qtlmv_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3] [T:P,T:P,...=4:1000,16:250]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

a = [int(x) for x in sys.argv[1:5]] + [10000, 2500, 20, 3][len(sys.argv[1:5]):]
n, snps, chroms, reps = a
shapes = [tuple(int(v) for v in x.split(":")) for x in (sys.argv[5] if len(sys.argv) > 5 else "4:1000,16:250").split(",")]
t0 = time.perf_counter()
ped = synth.make_f2(n, snps, chroms, seed=2)
gen_s = time.perf_counter() - t0
ctx = capi.Context(0)
ctx.upload(ped)
M, dev = ped.n_markers, torch.device("cuda", 0)
f = torch.empty((n, chroms, 8), dtype=torch.float64, device=dev)
ll = torch.empty((n, chroms), dtype=torch.float64, device=dev)
org = torch.empty((n, M, 4), dtype=torch.float64, device=dev)
osum = torch.empty((M, 4), dtype=torch.float64, device=dev)
cnt = torch.empty(chroms, dtype=torch.int32, device=dev)
ctx.sweep_origins_device(0, n, f.data_ptr(), ll.data_ptr(), org.data_ptr(), None, osum.data_ptr(), cnt.data_ptr())
ctx.sync()
truth = ped.allele[3:, M // 3, :].astype(np.float64).sum(axis=1) - 3.0
print("%d F2 x %d markers (%d chromosomes; input %.1f s), best of %d; times in s, ending in a synchronise" % (n, M, chroms, gen_s, reps))
for T, P in shapes:
    noise = synth.uniform(77, np.arange(n * T)).reshape(n, T) - 0.5
    pheno = 0.15 * truth[:, None] + 2.0 * noise + 0.5 * noise[:, :1]          # a small effect on every trait, correlated noise
    perm = qtl.permutations(n, P, 3)
    out = {}

    def single():
        out["single"] = ctx.qtl_scan_device(n, org.data_ptr(), pheno, perm=perm)

    def joint():
        out["joint"] = ctx.qtl_scan_mv_device(n, org.data_ptr(), pheno, perm=perm)

    calls = (("cnf2_qtl_scan", single), ("cnf2_qtl_scan_mv", joint))
    for _, fn in calls:
        fn()
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    R, T4 = T * (1 + P), 4 if T <= 4 else (8 if T <= 8 else 16)
    flop = 2.0 * (2 * M) * n * R
    ts, tj = min(times["cnf2_qtl_scan"]), min(times["cnf2_qtl_scan_mv"])
    print("T = %d, P = %d (R = %d columns, %d padded; %.3g FLOP in the product)" % (T, P, R, T4 * (1 + P), flop))
    for name, _ in calls:
        print("  %-18s %.4f (all: %s)" % (name, min(times[name]), " ".join("%.4f" % v for v in times[name])))
    print("  joint / single %.3f; joint: %.2f TFLOP/s of useful product, single: %.2f" % (tj / ts, flop / tj / 1e12, flop / ts / 1e12))
    s, j = out["single"], out["joint"]
    print("  joint peak LOD %.2f at marker %d (planted %d), single traits at most %.2f; 5 %% genome-wide threshold of the joint LOD %.2f" %
          (j["lod"].max(), int(j["lod"].argmax()), M // 3, s["lod"].max(), qtl.thresholds(j["perm_max"][:, None, :])["genome"][0, 0]))
ctx.close()
