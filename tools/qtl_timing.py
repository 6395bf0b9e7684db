"""Measurement aid: wall time, ending in a device synchronise, of cnf2_qtl_scan on device rows against the origin sweep that
makes the rows (cnf2_sweep_origins, device outputs) and, as the yardstick of the scan's hot path only, against torch.matmul
in f64 of the same [2 M x n] x [n x R] product on a and d materialised beforehand (the torch run never enters the product:
it does not gather a and d from the 32-byte rows, masks nothing and has no epilogue).  One process, the three alternating,
on a synthetic F2 (synth.make_f2); config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs (+1 dummy marker
each).  One trait; P permutations for every P of the list.
usage: python tools/qtl_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3] [P,P,...=0,100,1000]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

PEAK = 78.6e12          # f64 matrix peak of the MI355X, FLOP/s
a = [int(x) for x in sys.argv[1:5]] + [10000, 2500, 20, 3][len(sys.argv[1:5]):]
n, snps, chroms, reps = a
perms = [int(x) for x in (sys.argv[5] if len(sys.argv) > 5 else "0,100,1000").split(",")]
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


def sweep():
    ctx.sweep_origins_device(0, n, f.data_ptr(), ll.data_ptr(), org.data_ptr(), None, osum.data_ptr(), cnt.data_ptr())
    ctx.sync()


sweep()
# a phenotype with an additive effect at one marker, and the matmul's operands: A[2 M][n] = (a; d) materialised
truth = ped.allele[3:, M // 3, :].astype(np.float64).sum(axis=1) - 3.0
pheno = (0.5 * truth + 2.0 * (synth.uniform(77, np.arange(n)) - 0.5))[:, None]
A = torch.empty((2 * M, n), dtype=torch.float64, device=dev)
A[:M] = (org[:, :, 3] - org[:, :, 0]).T
A[M:] = (org[:, :, 1] + org[:, :, 2]).T
print("%d F2 x %d markers (%d chromosomes; input %.1f s), one trait, best of %d; times in s, ending in a synchronise" % (n, M, chroms, gen_s, reps))
for P in perms:
    R = 1 + P
    perm = qtl.permutations(n, P, 3) if P else None
    res = qtl.null_residuals(pheno)
    Y = torch.from_numpy(np.concatenate([res] + [res[p] for p in (perm if P else [])], axis=1)).to(dev)
    out = {}

    def scan():
        out["got"] = ctx.qtl_scan_device(n, org.data_ptr(), res, perm=perm)      # (ends in the call's own synchronise)

    def matmul():
        out["C"] = torch.matmul(A, Y)
        torch.cuda.synchronize()

    calls = (("cnf2_sweep_origins", sweep), ("cnf2_qtl_scan", scan), ("torch.matmul f64", matmul))
    for _, fn in calls:
        fn()
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    flop = 2.0 * (2 * M) * n * R
    ts, tm, tw = min(times["cnf2_qtl_scan"]), min(times["torch.matmul f64"]), min(times["cnf2_sweep_origins"])
    spread = max(times["torch.matmul f64"]) - tm
    print("P = %d (R = %d columns, %.3g FLOP in the product)" % (P, R, flop))
    for name, _ in calls:
        print("  %-20s %.4f (all: %s)" % (name, min(times[name]), " ".join("%.4f" % v for v in times[name])))
    print("  scan: %.2f TFLOP/s = %.3f of the %.1f TFLOP/s f64 matrix peak (whole call over the product's FLOP); scan / sweep %.3f; "
          "scan / matmul %.2f (matmul %.2f TFLOP/s, its own spread %.4f s)" % (flop / ts / 1e12, flop / ts / PEAK, PEAK / 1e12, ts / tw, ts / tm, flop / tm / 1e12, spread))
    g = out["got"]
    print("  peak LOD %.2f at marker %d (planted %d)%s" % (g["lod"].max(), int(g["lod"].argmax()), M // 3,
          "; 5 %% genome-wide threshold %.2f" % qtl.thresholds(g["perm_max"])["genome"][0, 0] if P else ""))
    del out["C"], Y
ctx.close()
